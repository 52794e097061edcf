"""(CPU) The backward-error checks of tests/backward_error.py on LAPACK and on the numpy model of
the inverse-based substitution: the plain bound admits LAPACK on every designed input, the design
bound admits the model, the plain bound refuses the model where the design predicts, the design bound
refuses a perturbed factor, and the long-double references (logpdf, gradient) are as exact as they are
taken to be; the forward bound of the gradient's alpha admits LAPACK and the model.

Figures of this file (worst entry / bound, 60 designed inputs: 5 designs x 4 noise levels x 3 sizes):
  LAPACK / plain_bound: factor 0.013 - 0.093, solve 0.002 - 0.056;
  model / design_bound: factor 0.008 - 0.055, solve 0.001 - 0.037;
  model / plain_bound at noise <= 1e-6: dates 296 - 2.0e5 (all six above 10); unif 18.6, 8.0, 6.4 at
    1e-6 and 82.6, 11.3, 16.4 at 1e-8 (N = 129, 300, 700): every one above the bound, and above 10 times
    the bound at every size for one of the two noise levels. (With numpy.linalg.inv, whose LU leaves
    rounding noise above the diagonal of the inverse, the model is 10 to 1e13 times outside BOTH bounds on
    entries of C near 1e-36; the kernels' inverse is exactly triangular and so is the model's.)
"""
import functools

import numpy as np
import pytest
import scipy.linalg

from oracle import restatement as R
from tests import backward_error as B
from tests import hp_oracle as H

KEYS = B.input_ids()
IDS = [B.input_name(k) for k in KEYS]


@functools.lru_cache(maxsize=None)
def analysis(key):
    """Worst ratios of LAPACK's and the model's factor and solve on one designed input."""
    X, terms, noise, v = B.designed_input(*key)
    C = R.gram(X, terms, noise)
    N = len(v)
    out = {}
    L = np.linalg.cholesky(C)
    z = scipy.linalg.solve_triangular(L, v, lower=True, check_finite=False)
    E, A = B.factor_residual(L, C)
    e, a = B.solve_residual(L, z, v)
    out["lapack"] = (B.worst_ratio(E, B.plain_bound(A, N)), B.worst_ratio(e, B.plain_bound(a, N)))
    L = B.substitution_model(C)
    z = B.substitution_model_solve(L, v)
    E, A = B.factor_residual(L, C)
    e, a = B.solve_residual(L, z, v)
    out["model_plain"] = (B.worst_ratio(E, B.plain_bound(A, N)), B.worst_ratio(e, B.plain_bound(a, N)))
    out["model_design"] = (B.worst_ratio(E, B.design_bound(L, A)), B.worst_ratio(e, B.design_bound_solve(L, z, a)))
    print(f"BACKWARD cpu {B.input_name(key)}: LAPACK/plain {out['lapack'][0]:.3f} {out['lapack'][1]:.3f}, "
          f"model/plain {out['model_plain'][0]:.3g} {out['model_plain'][1]:.3g}, "
          f"model/design {out['model_design'][0]:.3f} {out['model_design'][1]:.3f}")
    return out


def test_long_double_is_extended():
    """The residuals mean what the module says only with a 64-bit significand (elsewhere the module
    warns and forms them with mpmath on row subsets; this suite's complete residuals need the type)."""
    assert B.HAVE_LD and np.finfo(np.longdouble).eps <= 2.0 ** -63


def test_every_design_and_size_is_there():
    assert len(KEYS) == 60 and len(set(IDS)) == 60
    assert set(B.designed_inputs(sizes=(129,), noises=(0.1,))) == {f"{d}-0.1-129" for d in B.DESIGNS}


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_lapack_within_plain_bound(key):
    """The admission rule of a designed input: LAPACK factors it and stays within the plain bound."""
    rf, rs = analysis(key)["lapack"]
    assert rf <= 1.0 and rs <= 1.0, (rf, rs)


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_model_within_design_bound(key):
    rf, rs = analysis(key)["model_design"]
    assert rf <= 1.0 and rs <= 1.0, (rf, rs)


@pytest.mark.parametrize("name", ["dates", "unif"])
@pytest.mark.parametrize("N", B.SIZES)
def test_plain_bound_refuses_the_model(name, N):
    """The plain check sees the inverse-based substitution: at noise <= 1e-6 the model is outside the
    plain bound on every such input, and by more than 10 times at every size (dates: at both noise
    levels; unif: at one of the two at least, module docstring)."""
    r = [analysis((name, noise, N))["model_plain"][0] for noise in (1e-6, 1e-8)]
    assert min(r) > 1.0 and max(r) > 10.0, r
    if name == "dates":
        assert min(r) > 10.0, r


@pytest.mark.parametrize("key", [("unif", 0.1, 300), ("dates", 1e-6, 300), ("sorted", 1e-4, 700)], ids=B.input_name)
def test_design_bound_refuses_a_perturbed_block(key):
    """One 16 x 16 panel block of a good factor scaled by 1 + 1e-10 (a wrong Dinv block's footprint)."""
    X, terms, noise, v = B.designed_input(*key)
    C = R.gram(X, terms, noise)
    L = B.substitution_model(C)
    E, A = B.factor_residual(L, C)
    assert B.worst_ratio(E, B.design_bound(L, A)) <= 1.0
    L[160:176, 32:48] *= 1.0 + 1e-10
    rows = np.arange(160, 176)
    E, A = B.factor_residual(L, C, rows)
    r = B.worst_ratio(E, B.design_bound(L, A, rows))
    print(f"BACKWARD cpu perturbed block {B.input_name(key)}: worst/design {r:.3g}")
    assert r > 10.0, r


def test_rows_subset_is_the_complete_residual():
    X, terms, noise, v = B.designed_input("unif", 1e-6, 300)
    C = R.gram(X, terms, noise)
    L = B.substitution_model(C)
    E, A = B.factor_residual(L, C)
    rows = B.subset_rows(300)
    assert {0, 15, 16, 127, 128, 129, 298, 299} <= set(rows.tolist()) and len(rows) >= 54
    Er, Ar = B.factor_residual(L, C, rows)
    assert np.array_equal(Er, E[rows]) and np.allclose(Ar, A[rows], rtol=1e-14, atol=0)
    assert np.array_equal(B.design_bound(L, A)[rows], B.design_bound(L, A[rows], rows))


def test_alpha_bound_on_lapack_and_model():
    """|C alpha - y| of LAPACK's solves and of the model's forward solve within design_bound_alpha."""
    X, terms, noise, y = B.designed_input("dates", 1e-6, 300)
    C = R.gram(X, terms, noise)
    for L, forward in ((np.linalg.cholesky(C), lambda L: scipy.linalg.solve_triangular(L, y, lower=True)),
                       (B.substitution_model(C), lambda L: B.substitution_model_solve(L, y))):
        z = forward(L)
        alpha = scipy.linalg.solve_triangular(L, z, lower=True, trans="T", check_finite=False)
        e, _ = B.spd_solve_residual(C, alpha, y, L)
        assert B.worst_ratio(e, B.design_bound_alpha(L, alpha)) <= 1.0


@pytest.mark.parametrize("key", [("unif", 1e-6, 300), ("dates", 1e-4, 129), ("ou", 1e-8, 300)], ids=B.input_name)
def test_mean_bound_on_lapack(key):
    """The posterior mean at the training points by riding rows, restated with LAPACK's solves:
    mean_j = (L^-1 k_j) . z against (C - noise I) alpha within mean_bound plus the entries' term (the
    restatement's entries: constants 1, tests/test_hp_oracle.py)."""
    X, terms, noise, y = B.designed_input(*key)
    C = R.gram(X, terms, noise)
    K = R.cross_gram(X, X, terms)
    L = np.linalg.cholesky(C)
    z = scipy.linalg.solve_triangular(L, y, lower=True, check_finite=False)
    alpha = scipy.linalg.solve_triangular(L, z, lower=True, trans="T", check_finite=False)
    rows = B.subset_rows(len(y), extra=2)
    mean = np.zeros(len(y))
    for j in rows:
        mean[j] = scipy.linalg.solve_triangular(L, K[j], lower=True, check_finite=False) @ z
    e = B.mean_residual(C, alpha, noise, mean, rows)
    b = B.mean_bound(L, z, alpha, noise, rows)
    ent = B.entry_error_term(X, terms[0], alpha, rows, ((1, 1), (1, 1))) + B.U * np.abs(np.diag(C)[rows] * alpha[rows])
    r, r0 = B.worst_ratio(e, b + ent), B.worst_ratio(e, b)
    print(f"BACKWARD cpu mean {B.input_name(key)}: worst/bound {r:.3g} (without the entries' term {r0:.3g})")
    assert r <= 1.0, r
    # the same mean against K alpha with the K it was computed from: no entries' term, and a solve
    # wrong by 1e-6 (one entry of the riding row) is seen (1e-9 is not, at noise 1e-6: the bound
    # carries |w_j| . |L^T||alpha|, 1e4 times the mean there)
    sharp = np.abs(B._rows_times(K[rows], alpha[:, None], mean[rows, None]))[:, 0]
    rs = B.worst_ratio(sharp, b)
    print(f"BACKWARD cpu mean {B.input_name(key)}: against K alpha, worst/bound {rs:.3g}")
    assert rs <= 1.0, rs
    w = scipy.linalg.solve_triangular(L, K[rows[-1]], lower=True, check_finite=False)
    w[5] *= 1.0 + 1e-6
    bad = np.abs(B._rows_times(K[rows[-1:]], alpha[:, None], np.array([[w @ z]])))[0, 0]
    assert bad > b[-1], (bad, b[-1])


def test_long_double_reference_against_50_digits():
    """ld_logpdf against hp_oracle.logpdf_of (50 digits, the same fp64 matrix) at N = 129, noise 1e-8:
    within 1e-6 of the error LAPACK itself has there (measured: 2.9e-8 of it; 1.5e-3 without the
    first-order refinement, which is why the reference has it). One size: the 50-digit run takes 15 s."""
    X, terms, noise, v = B.designed_input("dates", 1e-8, 129)
    C = R.gram(X, terms, noise)
    ref = H.logpdf_of(H.MP.matrix(C.tolist()), v)
    lap = abs(H.mpf(R.logpdf_from_cov(C, v)[0]) - ref)
    errs = {}
    for refine in (True, False):
        ld = B.ld_logpdf(C, v, refine)[0]
        hi = float(ld)
        errs[refine] = abs(H.mpf(hi) + H.mpf(float(ld - np.longdouble(hi))) - ref)
    print(f"BACKWARD cpu yardstick: |ld - exact| / |LAPACK - exact| = {float(errs[True] / lap):.3g} "
          f"(unrefined {float(errs[False] / lap):.3g}), LAPACK's relative error {float(lap / abs(ref)):.3g}")
    assert lap > 0 and errs[True] <= H.mpf(10) ** -6 * lap


# ------------------------------------------------------------------- the long-double reference gradient
PRODUCT = [(B.SQEXP, 0, 1.3, 0), (B.LINEAR, 1, 0.4, 0), (B.CAT, 2, 0.0, 0), (B.OU, 0, 2.5, 1), (B.NOISE, -1, 0.2, 2)]


@pytest.mark.skipif(not B.HAVE_LD, reason="no 64-bit-significand long double")
@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("noise", [0.1, 1e-4])
def test_long_double_gradient_against_50_digits(N, noise):
    """ld_logpdf_grad against hp_oracle.grad_from (50 digits) on the same fp64 C and dC, a product-group
    formula: every output within 64 cond(C) 2^-64 of (|ref| + scale) (a few dozen roundings at 2^-64,
    which the inverse multiplies by cond(C) at most), alpha of max |alpha|."""
    rng = np.random.default_rng(40 + N)
    X = np.column_stack([rng.uniform(0, 2, N), rng.normal(size=N), rng.integers(0, 2, N).astype(float)])
    v = rng.normal(size=N)
    C = R.gram(X, PRODUCT, noise)
    dCs = B.grad_derivatives(X, PRODUCT)
    alpha, dp, dn, sc, scn, _ = B.ld_logpdf_grad(C, X, PRODUCT, v, with_scale=True)
    rdv, rdp, rdn, rsc, rscn = H.grad_from(H.MP.matrix(C.tolist()), [H.MP.matrix(d.tolist()) for d in dCs], v)
    tol = 64 * np.linalg.cond(C) * 2.0 ** -64

    def err(x, ref):                                   # |x - ref| of a long double against 50 digits
        hi = float(x)
        return abs(H.mpf(hi) + H.mpf(float(x - np.longdouble(hi))) - ref)

    assert max(err(alpha[i], -rdv[i]) for i in range(N)) <= tol * max(abs(a) for a in rdv)
    for t in range(len(PRODUCT)):
        assert err(dp[t], rdp[t]) <= tol * (abs(rdp[t]) + rsc[t]), (t, dp[t], rdp[t])
        assert abs(sc[t] - float(rsc[t])) <= 1e-14 * float(rsc[t])
    assert err(dn, rdn) <= tol * (abs(rdn) + rscn)
    assert abs(scn - float(rscn)) <= 1e-14 * float(rscn)


@pytest.mark.skipif(not B.HAVE_LD, reason="no 64-bit-significand long double")
@pytest.mark.parametrize("name", B.DESIGNS)
def test_long_double_gradient_against_lapack(name):
    """N = 129, noise 1e-6: fp64 LAPACK (logpdf_grad_potri's arithmetic; lapack_grad is bitwise that)
    is within its own expected error of the long-double gradient, cond(C) 2^-53 of the scale."""
    X, terms, noise, v = B.designed_input(name, 1e-6, 129)
    C = R.gram(X, terms, noise)
    alpha, dp, dn, sc, scn, Ci = B.ld_logpdf_grad(C, X, terms, v, with_scale=True)
    la, ldp, ldn = B.lapack_grad(C, X, terms, v)
    _, pdv, pdp, pdn = R.logpdf_grad_potri(X, terms, noise, v)
    assert np.array_equal(-la, pdv) and np.array_equal(ldp, pdp) and ldn == pdn
    rsc, rscn = R.logpdf_grad_scale(X, terms, noise, v)
    bound = np.linalg.cond(C) * B.U
    assert np.all(np.abs(rsc - sc) <= 10 * bound * sc) and abs(rscn - scn) <= 10 * bound * scn
    ea = float(np.max(np.abs(la - alpha)) / np.max(np.abs(alpha)))
    ep = B.worst_ratio(np.abs(np.asarray(ldp - dp, dtype=np.float64)), sc)
    en = float(abs(ldn - dn)) / scn
    print(f"BACKWARD cpu gradient yardstick {name}-1e-06-129: cond {bound / B.U:.3g}; LAPACK's error over "
          f"cond u scale: alpha {ea / bound:.3g}, dparam {ep / bound:.3g}, dnoise {en / bound:.3g}")
    assert ea <= bound and ep <= bound and en <= bound


@pytest.mark.skipif(not B.HAVE_LD, reason="no 64-bit-significand long double")
@pytest.mark.parametrize("key", [("unif", 1e-8, 300), ("dates", 1e-6, 300), ("composite", 0.1, 300)], ids=B.input_name)
def test_alpha_forward_bound_on_lapack_and_model(key):
    """alpha_forward_bound admits alpha = Y z with LAPACK's factor and with the model's (the explicit
    16 x 16 inverses), with the slack of a worst-case bound (measured: worst entry / bound 2e-4 to
    2e-3). On unif-1e-08-300 the model's alpha is 55 times LAPACK's error from the long-double alpha, by
    substitution and by Y z alike: the loss is the factor's, not the route's."""
    X, terms, noise, v = B.designed_input(*key)
    C = R.gram(X, terms, noise)
    alpha, _, _, _, _, Ci = B.ld_logpdf_grad(C, X, terms, v, with_scale=True)
    errs = {}
    for name, L, z in (("lapack", np.linalg.cholesky(C), None), ("model", B.substitution_model(C), None)):
        z = (scipy.linalg.solve_triangular(L, v, lower=True, check_finite=False) if name == "lapack"
             else B.substitution_model_solve(L, v))
        a = B._tri_inverse(L).T @ z
        e = np.abs(np.asarray(a - alpha, dtype=np.float64))
        r = B.worst_ratio(e, B.alpha_forward_bound(L, z, a, Ci))
        errs[name] = float(e.max())
        print(f"BACKWARD cpu alpha forward {B.input_name(key)} {name}: worst/bound {r:.3g}, max error {e.max():.3g}")
        assert r <= 1.0, (name, r)
        if name == "model":
            bs = scipy.linalg.solve_triangular(L, z, lower=True, trans="T", check_finite=False)
            errs["model_subst"] = float(np.max(np.abs(np.asarray(bs - alpha, dtype=np.float64))))
    if key == ("unif", 1e-8, 300):
        assert errs["model"] > 10 * errs["lapack"] and errs["model_subst"] > 10 * errs["lapack"], errs
    if noise == 0.1:      # well conditioned: the bound is far below 1e-9 and sees one entry 1e-8 off
        L = B.substitution_model(C)
        z = B.substitution_model_solve(L, v)
        a = B._tri_inverse(L).T @ z
        i = int(np.argmax(np.abs(a)))
        a[i] *= 1.0 + 1e-8
        e = np.abs(np.asarray(a - alpha, dtype=np.float64))
        assert e[i] > B.alpha_forward_bound(L, z, a, Ci)[i]


def test_gradient_inputs_are_admitted():
    """tests/test_gpu_backward.py skips a gradient input that LAPACK finds not positive definite; at most
    a quarter may go that way. Here, with LAPACK alone on the restatement's C: none does."""
    keys = [k for k in KEYS if k[2] in (300, 700)]
    bad = []
    for key in keys:
        X, terms, noise, v = B.designed_input(*key)
        try:
            np.linalg.cholesky(R.gram(X, terms, noise))
        except np.linalg.LinAlgError:
            bad.append(key)
    assert len(keys) == 40 and 4 * len(bad) <= len(keys), bad
    assert not bad
