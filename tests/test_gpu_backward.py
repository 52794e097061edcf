"""Backward error of the HIP factorisation and of its solves on ill-conditioned covariance matrices
(DESIGN.md §5.2): |L L^T - C|, |L z - v| and |C alpha - y| entry by entry against bounds that are
functions of the outputs alone (tests/backward_error.py derives them from the kernel code), and the
forward error of logpdf and of the gradient (dv, dparam, dnoise) against long-double references, on
the designed inputs of backward_error.designed_inputs: five designs x noise 0.1 .. 1e-8 x N = 129, 300,
700.

C is the GPU's own Gram (Context.gram: bitwise what an evaluation builds,
test_gpu_entrywise.test_gram_inside_an_evaluation), so the entries' error does not mix in.

Contexts (switches are read when a context is created), one per substitution site:
  tail         the library default: the whole matrix in the persistent tail (potrf_diag2_body,
               tail_trsm and tail_trsm_pipe);
  launches     GAPLAC_TAILK=0: per-column launches (potrf_diag_kernel, trsm_subst_kernel);
  launch_pair  GAPLAC_TAIL_S=0: the super-panel launch pair;
  spw3_tail8   GAPLAC_SPW=3, GAPLAC_TAIL_S=8, used at N = 2049 (17 tiles): super-panels, paired bulk
               updates, then the tail. (At N <= 700 its six tile columns lie whole in the tail: the
               `tail` context's schedule, so the designed sizes do not run in it.) At N = 2049 the
               `tail` context runs too (a 17-column tail).
  spw1         GAPLAC_SPW=1: the gradient's identity rows through 3 (N = 300) and 6 (N = 700)
               super-panels (the gradient never takes the tail: in `tail` it runs the default
               super-panel width, one and two super-panels).
gaplac_factor runs gaplac_logpdf's evaluation (eval_device with no riding rows beyond v, the
schedule chosen from the context's switches alone) and copies L and the riding row out, so every
switch reaches it.

Each test prints its figures before it asserts; DESIGN.md §5.2 tabulates them.
"""
import functools
import os

import numpy as np
import pytest
import scipy.linalg

from gaplac_amd.backend import Context
from oracle import restatement as R
from tests import backward_error as B
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

CONTEXTS = {
    "tail": {},
    "launches": {"GAPLAC_TAILK": "0"},
    "launch_pair": {"GAPLAC_TAIL_S": "0"},
    "spw3_tail8": {"GAPLAC_SPW": "3", "GAPLAC_TAIL_S": "8"},
    "spw1": {"GAPLAC_SPW": "1"},
}
SMALL_CTX = ["tail", "launches", "launch_pair"]
BIG_CTX = ["spw3_tail8", "tail"]
KEYS = B.input_ids()
IDS = [B.input_name(k) for k in KEYS]
BIG_N = 2049
BIG_KEYS = B.input_ids(sizes=(BIG_N,), noises=(0.1, 1e-6))
BIG_IDS = [B.input_name(k) for k in BIG_KEYS]
ALPHA_KEYS = [k for k in KEYS if k[2] in (300, 700)]


def make_ctx(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctxs():
    if not gpu_available():
        pytest.skip("no GPU")
    cs = {name: make_ctx(env) for name, env in CONTEXTS.items()}
    yield cs
    for c in cs.values():
        c.close()


@functools.lru_cache(maxsize=None)
def designed(key):
    return B.designed_input(*key)


_gram, _lapack, _ref = {}, {}, {}


def gram_of(ctxs, key):
    """The GPU's Gram of one designed input, built once (any context builds the same)."""
    if key not in _gram:
        X, terms, noise, v = designed(key)
        _gram[key] = np.ascontiguousarray(ctxs["tail"].gram(X, terms, noise))
    return _gram[key]


def lapack_of(ctxs, key, rows=None):
    """(worst LAPACK / plain ratio of the factor, of the solve) on the GPU's Gram: LAPACK factors it."""
    if key not in _lapack:
        C = gram_of(ctxs, key)
        v = designed(key)[3]
        L = np.linalg.cholesky(C)
        z = scipy.linalg.solve_triangular(L, v, lower=True, check_finite=False)
        E, A = B.factor_residual(L, C, rows)
        e, a = B.solve_residual(L, z, v)
        _lapack[key] = (B.worst_ratio(E, B.plain_bound(A, len(v))), B.worst_ratio(e, B.plain_bound(a, len(v))))
    return _lapack[key]


def check_factor(ctxs, cname, key, rows=None):
    X, terms, noise, v = designed(key)
    N = len(v)
    C = gram_of(ctxs, key)
    lap = lapack_of(ctxs, key, rows)                  # (raises where LAPACK finds C not positive definite)
    L, z = ctxs[cname].factor(X, terms, noise, v)     # info > 0 raises PosDefException
    L = np.ascontiguousarray(L)
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(z))
    E, A = B.factor_residual(L, C, rows)
    e, a = B.solve_residual(L, z, v)
    rd, rp = B.worst_ratio(E, B.design_bound(L, A, rows)), B.worst_ratio(E, B.plain_bound(A, N))
    sd, sp = B.worst_ratio(e, B.design_bound_solve(L, z, a)), B.worst_ratio(e, B.plain_bound(a, N))
    print(f"BACKWARD factor[{cname}] {B.input_name(key)}: worst/design {rd:.4f}, worst/plain {rp:.4f}, "
          f"LAPACK worst/plain {lap[0]:.4f}")
    print(f"BACKWARD solve[{cname}] {B.input_name(key)}: worst/design {sd:.4f}, worst/plain {sp:.4f}, "
          f"LAPACK worst/plain {lap[1]:.4f}")
    assert lap[0] <= 1.0 and lap[1] <= 1.0, lap       # the input's admission rule
    assert rd <= 1.0 and sd <= 1.0, (rd, sd)
    if noise == 0.1:
        assert rp <= 1.0 and sp <= 1.0, (rp, sp)


# --------------------------------------------------------------------------------------------- factor
@pytest.mark.parametrize("key", KEYS, ids=IDS)
@pytest.mark.parametrize("cname", SMALL_CTX)
def test_factor_and_riding_row(ctxs, cname, key):
    """The complete residual at N <= 700, in every context."""
    check_factor(ctxs, cname, key)


@pytest.mark.parametrize("key", BIG_KEYS, ids=BIG_IDS)
@pytest.mark.parametrize("cname", BIG_CTX)
def test_factor_and_riding_row_17_tiles(ctxs, cname, key):
    """N = 2049: rows 0, 15, 16, 127, 128, 129, 1023, 1024, N-2, N-1 and 54 seeded random rows of the
    factor's residual (the riding row's is complete)."""
    rows = B.subset_rows(BIG_N)
    assert {0, 15, 16, 127, 128, 129, 1023, 1024, BIG_N - 2, BIG_N - 1} <= set(rows.tolist())
    check_factor(ctxs, cname, key, rows)


# ---------------------------------------------------------------------------------------------- alpha
@pytest.mark.parametrize("key", ALPHA_KEYS, ids=[B.input_name(k) for k in ALPHA_KEYS])
def test_alpha_residual(ctxs, key):
    """alpha = C^-1 y of the fitted posterior: |C alpha - y| within backward_error.design_bound_alpha
    (Higham Thm 10.4's three gamma_N with the pivots' and the partial sums' additions, and the
    substitution term of the factor and of the forward solve; the back-substitution is plain). The
    bound is evaluated with the L of Context.factor (the bound needs |L| only)."""
    X, terms, noise, y = designed(key)
    c = ctxs["tail"]
    C = gram_of(ctxs, key)
    L, _ = c.factor(X, terms, noise, y)
    L = np.ascontiguousarray(L)
    with c.fit(X, terms, noise, y, cap=128) as fit:
        alpha = fit.alpha()
    assert np.all(np.isfinite(alpha))
    e, a = B.spd_solve_residual(C, alpha, y, L)
    r = B.worst_ratio(e, B.design_bound_alpha(L, alpha))
    rp = B.worst_ratio(e, B.gamma(3 * len(y) + 1) * a)
    print(f"BACKWARD alpha[tail] {B.input_name(key)}: worst/design {r:.4f}, worst/plain {rp:.4f}")
    assert r <= 1.0, r


MEAN_KEYS = [k for k in ALPHA_KEYS if k[0] != "composite"]


@pytest.mark.parametrize("key", MEAN_KEYS, ids=[B.input_name(k) for k in MEAN_KEYS])
def test_posterior_mean_at_training_points(ctxs, key):
    """posterior_mean_var at Xs = X (the riding-row solve of N cross-covariance rows, then w_j . z)
    against the products with alpha, on backward_error.subset_rows, two ways:

    * sharp: against K alpha with the very cross-covariance rows K the GPU computes (column i of K from
      an N = 1 posterior at x_i with y = 1, noise 0: C = L = z = 1 and the mean is the entry itself,
      test_gpu_entrywise.test_cross_covariance), within backward_error.mean_bound: nothing but the two
      solves' and the product's roundings;
    * as a user sees it: against C alpha - noise alpha with the Gram's C, within mean_bound plus the
      entries' term: the cross-covariance (library exp, constants 2 and 1) and the Gram (table exp,
      constants 4 and 4 or 1, tests/test_gpu_entrywise.py) are two roundings of one entry, and
      C_jj = fl(k_jj + noise) adds u |C_jj alpha_j|. On the dates design (offset 2.4e6: a scaled
      coordinate's rounding alone is 1e-11 of the argument) this term is 400 to 850 times the rest,
      which is why the sharp form is there; on the designs at offset 0 it is below a tenth of it.

    mean_bound takes z = (L^T + dL2) alpha with the fitted posterior's alpha: the riding row z of an
    evaluation does not depend on the rows riding beside it. The fitted posterior's own mean_var
    (the same arithmetic from the kept factor) is held to the same bounds."""
    from tests.test_gpu_entrywise import C_E_LIBM, C_E_TABLE, C_U
    X, terms, noise, y = designed(key)
    N = len(y)
    c = ctxs["tail"]
    C = gram_of(ctxs, key)
    L, z = c.factor(X, terms, noise, y)
    L = np.ascontiguousarray(L)
    with c.fit(X, terms, noise, y, cap=1024) as fit:
        alpha = fit.alpha()
        fmean = fit.mean_var(X)[0]
    mean = c.posterior_mean_var(X, terms, noise, y, X)[0]
    rows = B.subset_rows(N, extra=6)
    K = np.empty((len(rows), N))
    for i in range(N):
        K[:, i] = c.posterior_mean_var(X[i:i + 1], terms, 0.0, np.ones(1), X[rows])[0]
    b = B.mean_bound(L, z, alpha, noise, rows)
    kind = terms[0][0]
    ent = (B.entry_error_term(X, terms[0], alpha, rows, ((C_E_LIBM, C_U[kind, "plain"]), (C_E_TABLE, C_U[kind, "gram"])))
           + B.U * np.abs(np.diag(C)[rows] * alpha[rows]))
    for what, m in (("posterior_mean_var", mean), ("fit.mean_var", fmean)):
        sharp = np.abs(B._rows_times(K, alpha[:, None], m[rows, None]))[:, 0]
        user = B.mean_residual(C, alpha, noise, m, rows)
        rs, ru = B.worst_ratio(sharp, b), B.worst_ratio(user, b + ent)
        print(f"BACKWARD mean[tail] {what} {B.input_name(key)}: against K alpha worst/bound {rs:.4f}; against "
              f"C alpha - noise alpha worst/bound {ru:.4f} (entries' term / rest: {float(np.max(ent / b)):.3g})")
        assert rs <= 1.0 and ru <= 1.0, (what, rs, ru)


# -------------------------------------------------------------------------------- the promise, forward
def forward_record(ctxs, key):
    """(relative error of the GPU's logpdf, of LAPACK's, the GPU's logdet and quad errors over |logpdf|)
    against the long-double reference on the GPU's own Gram."""
    if key not in _ref:
        X, terms, noise, v = designed(key)
        C = gram_of(ctxs, key)
        ref = B.ld_logpdf(C, v)
        lp, ld, q = ctxs["tail"].logpdf(X, terms, noise, v, full=True)
        lap = R.logpdf_from_cov(C, v)[0]
        s = abs(ref[0])
        _ref[key] = (float(abs(lp - ref[0]) / s), float(abs(lap - ref[0]) / s),
                     float(abs(ld - ref[1]) / s), float(abs(q - ref[2]) / s))
        print(f"BACKWARD forward[tail] {B.input_name(key)}: logpdf relative error {_ref[key][0]:.3e}, "
              f"LAPACK {_ref[key][1]:.3e}; logdet {_ref[key][2]:.3e}, quad {_ref[key][3]:.3e} of |logpdf|")
    return _ref[key]


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_forward_promise(ctxs, key):
    """Where LAPACK itself is within 1e-10 of the long-double reference (a condition on the input, not
    a tolerance of the GPU), the GPU's logpdf is within README's 1e-9. Elsewhere (noise 1e-8 on the
    smooth designs) the figures are printed only."""
    gpu, lap, _, _ = forward_record(ctxs, key)
    assert np.isfinite(gpu)
    if lap <= 1e-10:
        assert gpu <= 1e-9, (gpu, lap)


def test_forward_condition_covers_three_quarters(ctxs):
    ok = [k for k in KEYS if forward_record(ctxs, k)[1] <= 1e-10]
    print(f"BACKWARD forward: {len(ok)} of {len(KEYS)} designed inputs meet LAPACK <= 1e-10")
    assert 4 * len(ok) >= 3 * len(KEYS), len(ok)
    assert all(forward_record(ctxs, k)[0] <= 1e-9 for k in ok)


# ------------------------------------------------------------------------------------------- gradient
GRAD_CTX = ["tail", "spw1"]
_grad_ref, _grad_rec = {}, {}


def grad_reference(ctxs, key):
    """(long-double alpha, dparam, dnoise, scale, scale of dnoise; LAPACK's errors against them: of dv,
    of each dparam, of dnoise; |C^-1|) on the GPU's Gram, once per input; None where LAPACK finds the
    Gram not positive definite (the admission rule)."""
    if key not in _grad_ref:
        X, terms, noise, v = designed(key)
        C = gram_of(ctxs, key)
        try:
            la, ldp, ldn = B.lapack_grad(C, X, terms, v)
        except np.linalg.LinAlgError:
            _grad_ref[key] = None
            return None
        alpha, dp, dn, sc, scn, Ci = B.ld_logpdf_grad(C, X, terms, v, with_scale=True)
        lap = (float(np.max(np.abs(la - alpha))), np.abs(np.asarray(ldp - dp, dtype=np.float64)), float(abs(ldn - dn)))
        _grad_ref[key] = (alpha, dp, dn, sc, scn, lap, Ci)
    return _grad_ref[key]


@pytest.mark.skipif(not B.HAVE_LD, reason="no 64-bit-significand long double")
@pytest.mark.parametrize("key", ALPHA_KEYS, ids=[B.input_name(k) for k in ALPHA_KEYS])
@pytest.mark.parametrize("cname", GRAD_CTX)
def test_gradient_against_lapack_yardstick(ctxs, cname, key):
    """gaplac_logpdf_grad on the designed inputs against backward_error.ld_logpdf_grad on the GPU's own
    Gram. The explicit-inverse route Y Y^T has no derived bound here, so the yardstick of dparam and
    dnoise is fp64 LAPACK's error (logpdf_grad_potri's arithmetic) on the same matrix:
        GPU error <= max(1e-9 (|ref| + scale), 10 x LAPACK's error),
    one decimal digit behind LAPACK where the input is too ill-conditioned for the README's 1e-9.

    dv = -alpha does not meet that: on unif-1e-06-300 and unif-1e-08-300 it is 11.5 and 34.7 times
    LAPACK's error (0.24 to 2.6 times on the other inputs beyond the floor), in both contexts alike. The
    cause is not the gradient's route (alpha = Y z with the explicit Y = L^-T): the numpy model of the
    factor (backward_error.substitution_model, the 16 x 16 explicit inverses of the panel's
    substitution) loses the same 55 times against LAPACK on that input whether alpha is then solved
    for by substitution or by Y z, and LAPACK's factor with an explicit inverse loses nothing
    (DESIGN.md §5.2). It is the factor's substitution term, C_SUB gamma_16 |X_b| T_b of design_bound,
    which cond(C) carries into alpha. So dv is held entry by entry to the bound derived from it,
        |dv + alpha| <= max(1e-9 max |alpha|, backward_error.alpha_forward_bound),
    in place of the factor 10; its ratio to LAPACK is printed."""
    ref = grad_reference(ctxs, key)
    if ref is None:
        pytest.skip("LAPACK finds the Gram not positive definite")
    alpha, rdp, rdn, sc, scn, (lap_v, lap_p, lap_n), Ci = ref
    X, terms, noise, v = designed(key)
    c = ctxs[cname]
    lp, dv, dp, dn = c.logpdf_grad(X, terms, noise, v)
    assert np.isfinite(lp) and np.all(np.isfinite(dv)) and np.all(np.isfinite(dp)) and np.isfinite(dn)
    L, z = c.factor(X, terms, noise, v)               # (the bound needs |L| and |z| only, as test_alpha_residual's)
    amax = float(np.max(np.abs(alpha)))
    evec = np.abs(np.asarray(dv + alpha, dtype=np.float64))
    bound = np.maximum(1e-9 * amax, B.alpha_forward_bound(np.ascontiguousarray(L), z, -dv, Ci))
    ev = float(np.max(evec))
    ep = np.abs(np.asarray(dp - rdp, dtype=np.float64))
    en = float(abs(dn - rdn))
    rows = [("dv", ev, lap_v, amax)]
    rows += [(f"dparam[{t}]", float(ep[t]), float(lap_p[t]), float(abs(rdp[t])) + sc[t]) for t in range(len(terms))]
    rows.append(("dnoise", en, lap_n, float(abs(rdn)) + scn))
    worst = {}
    for what, e, l, s in rows:
        ratio = 0.0 if e == 0.0 else (e / l if l > 0.0 else np.inf)
        over = e > 1e-9 * s
        if over:
            kind = what[:6]
            worst[kind] = max(worst.get(kind, 0.0), ratio)
        print(f"BACKWARD gradient[{cname}] {B.input_name(key)} {what}: GPU {e:.3e}, LAPACK {l:.3e}, ratio {ratio:.3g}, "
              f"GPU / (|ref| + scale) {e / s if s > 0.0 else 0.0:.3e}{' (beyond 1e-9)' if over else ''}")
    rb = B.worst_ratio(evec, bound)
    print(f"BACKWARD gradient[{cname}] {B.input_name(key)} dv: worst entry / max(floor, derived bound) {rb:.3g}")
    _grad_rec[cname, key] = (worst, rb)
    assert rb <= 1.0, rb
    for what, e, l, s in rows[1:]:
        assert e <= max(1e-9 * s, 10.0 * l), (what, e, l, s)


@pytest.mark.skipif(not B.HAVE_LD, reason="no 64-bit-significand long double")
def test_gradient_yardstick_covers_three_quarters(ctxs):
    """At most a quarter of the designed inputs may be skipped by the admission rule (none is: LAPACK
    factors every GPU Gram). Prints, per noise level, the worst GPU / LAPACK ratio among the entries
    beyond 1e-9 (|ref| + scale) and dv's worst entry over its bound, of the cases that ran before."""
    skipped = [k for k in ALPHA_KEYS if grad_reference(ctxs, k) is None]
    print(f"BACKWARD gradient: {len(skipped)} of {len(ALPHA_KEYS)} designed inputs skipped")
    for noise in B.NOISES:
        recs = [r for (c, k), r in _grad_rec.items() if k[1] == noise]
        if recs:
            per = {kind: max((w.get(kind, 0.0) for w, _ in recs)) for kind in ("dv", "dparam", "dnoise")}
            print(f"BACKWARD gradient: noise {noise:g}: worst GPU / LAPACK ratio among the entries beyond the 1e-9 floor: "
                  f"dv {per['dv']:.3g}, dparam {per['dparam']:.3g}, dnoise {per['dnoise']:.3g}; "
                  f"dv worst / max(floor, derived bound) {max(rb for _, rb in recs):.3g}")
    assert 4 * len(skipped) <= len(ALPHA_KEYS), skipped


# ---------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("cname", SMALL_CTX + ["spw3_tail8"])
def test_factor_is_deterministic(ctxs, cname):
    key = ("dates", 1e-8, 700) if cname != "spw3_tail8" else ("dates", 1e-6, BIG_N)
    X, terms, noise, v = designed(key)
    L1, z1 = ctxs[cname].factor(X, terms, noise, v)
    L2, z2 = ctxs[cname].factor(X, terms, noise, v)
    assert np.array_equal(L1, L2) and np.array_equal(z1, z2)
