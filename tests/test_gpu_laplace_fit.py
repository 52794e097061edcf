"""The fitted Laplace posterior (gaplac_laplace_fit_create and the gaplac_fit_* queries on it, HIP
through the C-ABI): the mode found once, the factor of B kept, many test sets queried.

Bars. Against tests/laplace_oracle.py: mean within 1e-9 max(1, max |mean|), variance and every
covariance entry within 1e-9 max(1, kdiag), the bars of tests/test_gpu_laplace.py. log q, the mode,
a, iters and converged are bitwise the one-shot entry's (the same iteration, to the launch). Where
no rule forces bitwise equality (a row at another position, in a set of another size, under another
cap) results agree to 1e-13 relative, the bar of tests/test_gpu_fit.py; identical calls are bitwise
equal. Observation-space predictions within 1e-9 max(1, |ref|) of tests/laplace_predict_oracle.py
on the oracle's mean and variance.
"""
import warnings

import numpy as np
import pytest
import scipy.linalg

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd.backend import ArgumentError, Context, PosDefException
from oracle import restatement as R
from tests import laplace_oracle as LO
from tests import laplace_predict_oracle as PO
from tests import test_gpu_fit as TF
from tests.conftest import gpu_available
from tests.test_gpu_laplace import _gp_of

pytestmark = pytest.mark.gpu
TOL = 1e-9
SIZES = [(1, 1), (5, 3), (127, 129), (128, 128), (129, 1), (300, 1000), (1000, 64)]
TERMS = ["sqexp", "composite"]
LIKS = ["bernoulli", "poisson", "gaussian"]


@pytest.fixture(scope="module")
def ctx():
    if not gpu_available():
        pytest.skip("no GPU")
    c = Context(0)
    yield c
    c.close()


def lfit(ctx, c, cap=1024, **kw):
    return ctx.laplace_fit(c["X"], c["terms"], LO.JITTER, c["lik"], c["y"], lik_param=c["lik_param"], cap=cap, **kw)


def one_shot(ctx, c, **kw):
    return ctx.laplace_logpdf(c["X"], c["terms"], LO.JITTER, c["lik"], c["y"], lik_param=c["lik_param"], full=True, **kw)


def close_to(m, v, rm, rv, kd, what):
    em = np.max(np.abs(m - rm)) / max(1.0, np.max(np.abs(rm)))
    print(f"{what}: mean error {em:.3e} of the bar's scale")
    assert em <= TOL
    if v is not None:
        ev = np.max(np.abs(v - rv) / np.maximum(1.0, np.abs(kd)))
        print(f"{what}: variance error {ev:.3e} of the bar's scale")
        assert ev <= TOL


@pytest.mark.parametrize("cap", [128, 1024])
@pytest.mark.parametrize("lik_name", LIKS)
@pytest.mark.parametrize("terms_name", TERMS)
@pytest.mark.parametrize("N,M", SIZES)
def test_sizes(ctx, N, M, terms_name, lik_name, cap):
    c = LO.case(N, M, terms_name, lik_name)
    ref = one_shot(ctx, c)
    with lfit(ctx, c, cap) as fit:
        assert (fit.kind, fit.N, fit.cap) == ("laplace", N, cap)
        assert (fit.lik, fit.lik_param, fit.jitter) == (c["lik"], c["lik_param"], LO.JITTER)
        what = f"N={N} M={M} {terms_name} {lik_name} cap={cap}"
        close_to(*fit.mean_var(c["Xs"]), c["mean"], c["var"], c["kdiag"], "mean_var " + what)
        close_to(fit.mean(c["Xs"]), None, c["mean"], c["var"], c["kdiag"], "mean " + what)
        # the same iteration as the one-shot entry, to the bit
        assert fit.logq == ref.logq == fit.logpdf
        assert np.array_equal(fit.f_hat(), ref.f) and np.array_equal(fit.alpha(), ref.a)
        assert (fit.iters, fit.converged) == (ref.iters, ref.converged) and fit.converged
        assert fit.iters == c["res"].iters
        assert abs(fit.quad - float(ref.a @ ref.f)) <= 1e-12 * max(1.0, abs(fit.quad))
        assert abs(fit.logdet - 2.0 * np.sum(np.log(np.diag(c["res"].L)))) <= TOL * max(1.0, abs(fit.logdet))


@pytest.mark.parametrize("terms_name", TERMS)
def test_gaussian_likelihood_is_the_exact_fit(ctx, terms_name):
    c = LO.case(300, 1000, terms_name, "gaussian")
    with lfit(ctx, c, 128) as fit, ctx.fit(c["X"], c["terms"], 0.1 + LO.JITTER, c["y"], cap=128) as exact:
        m, v = fit.mean_var(c["Xs"])
        close_to(m, v, *exact.mean_var(c["Xs"]), c["kdiag"], f"against the exact fit, {terms_name}")
        ym, yv = fit.predict(c["Xs"])
        assert np.array_equal(ym, m) and np.array_equal(yv, v + 0.1)
        assert exact.kind == "exact"
        em, ev = exact.predict(c["Xs"])  # the Gaussian case with lik_param = noise
        xm, xv = exact.mean_var(c["Xs"])
        assert np.array_equal(em, xm) and np.array_equal(ev, xv + (0.1 + LO.JITTER))
        with pytest.raises(ArgumentError):
            exact.f_hat()
        assert not hasattr(exact, "logq")


def test_product_groups_and_noise_term(ctx):
    rng = np.random.default_rng(12)
    N, M = 260, 190
    X = np.column_stack([rng.uniform(0, 5, N), rng.normal(size=N)])
    Xs = np.column_stack([rng.uniform(0, 5, M), rng.normal(size=M)])
    terms = [(_native.SQEXP, 0, 1.3, 0), (_native.LINEAR, 1, 0.4, 0), (_native.OU, 0, 2.5, 1),
             (_native.NOISE, -1, 0.2, 2)]
    y = (rng.normal(size=N) > 0).astype(np.float64)
    ref = LO.laplace(X, terms, LO.JITTER, LO.BERNOULLI, y)
    rm, rv = LO.posterior_mean_var(ref, X, terms, Xs)
    kd = R.kernel_diag(Xs, terms)
    for cap in (128, 1024):
        with ctx.laplace_fit(X, terms, LO.JITTER, "bernoulli", y, cap=cap) as fit:
            close_to(*fit.mean_var(Xs), rm, rv, kd, f"groups mean_var cap={cap}")
            close_to(fit.mean(Xs), None, rm, rv, kd, f"groups mean cap={cap}")
            assert abs(fit.logq - ref.logq) <= TOL * max(1.0, abs(ref.logq))


def cov_oracle(c, noise_s):
    res = c["res"]
    Ks = R.cross_gram(c["Xs"], c["X"], c["terms"])
    V = scipy.linalg.solve_triangular(res.L, res.sw[:, None] * Ks.T, lower=True, check_finite=False)
    return R.gram(c["Xs"], c["terms"], noise_s) - V.T @ V


@pytest.mark.parametrize("lik_name", ["bernoulli", "poisson"])
@pytest.mark.parametrize("N,M,cap", [(5, 3, 256), (129, 1, 256), (127, 129, 256), (300, 1000, 1024)])
def test_mean_cov(ctx, N, M, cap, lik_name):
    c = LO.case(N, M, "composite", lik_name)
    scale = max(1.0, np.max(c["kdiag"]))
    with lfit(ctx, c, cap) as fit:
        m0, v0 = fit.mean_var(c["Xs"])
        for noise_s in (0.0, 0.05):
            mean, C = fit.mean_cov(c["Xs"], noise_s)
            e = np.max(np.abs(C - cov_oracle(c, noise_s))) / scale
            ed = np.max(np.abs(np.diag(C) - noise_s - v0)) / scale
            print(f"N={N} M={M} {lik_name} noise_s={noise_s}: covariance error {e:.3e}, diagonal against mean_var {ed:.3e}")
            assert e <= TOL and ed <= TOL
            assert np.array_equal(C, C.T)
            close_to(mean, None, c["mean"], None, None, "mean_cov's mean")
            assert np.array_equal(mean, m0)


def test_mean_cov_of_an_exact_fit_and_its_limits(ctx):
    X, Xs, y, rm, rv, kd, _ = TF.oracle(300, 1000)
    with ctx.fit(X, TF.COMPOSITE, 0.1, y, cap=256) as fit:
        for noise_s in (0.0, 0.05):
            mean, C = fit.mean_cov(Xs[:200], noise_s)
            pm, pC = ctx.posterior_mean_cov(X, TF.COMPOSITE, 0.1, y, Xs[:200], noise_s)
            e = np.max(np.abs(C - pC)) / max(1.0, np.max(kd))
            print(f"exact fit, noise_s={noise_s}: covariance against posterior_mean_cov {e:.3e}")
            assert e <= TOL and np.array_equal(C, C.T)
            close_to(mean, None, pm, None, None, "exact mean_cov's mean")
        with pytest.raises(ArgumentError, match="cap"):
            fit.mean_cov(Xs[:257])
        with pytest.raises(ArgumentError):
            fit.mean_cov(Xs[:5], -0.1)
        with pytest.raises(ArgumentError):
            fit.mean_cov(Xs[:5], float("nan"))
        lib, out = ctx.lib, np.full(9, 7.0)
        assert lib.gaplac_fit_mean_cov(fit.h, 3, Xs.ctypes.data, 1000, 0.0, out.ctypes.data, out.ctypes.data, 2) == -1
        assert lib.gaplac_fit_mean_cov(fit.h, 3, None, 3, 0.0, None, out.ctypes.data, 3) == -1
        assert np.all(np.isnan(out))  # NaN-filled first
        m, C = fit.mean_cov(np.zeros((0, 3)))
        assert m.shape == (0,) and C.shape == (0, 0)
        assert np.all(np.isfinite(fit.mean_cov(Xs[:5])[1]))  # usable after every failure


@pytest.mark.parametrize("lik_name", ["bernoulli", "poisson"])
@pytest.mark.parametrize("terms_name", TERMS)
def test_predict(ctx, terms_name, lik_name):
    c = LO.case(300, 1000, terms_name, lik_name)
    rng = np.random.default_rng(5)
    ys = (rng.uniform(size=1000) < 0.5).astype(np.float64) if lik_name == "bernoulli" else \
        rng.poisson(np.exp(np.clip(c["mean"], -5.0, 3.0))).astype(np.float64)
    ref = PO.predict(c["lik"], c["mean"], c["var"], ys, Q=32)
    with lfit(ctx, c) as fit:
        out = fit.predict(c["Xs"], ys)
        assert len(fit.predict(c["Xs"])) == 2
    for name, o, r in zip(("ymean", "yvar", "logp"), out, ref):
        e = np.max(np.abs(o - r) / np.maximum(1.0, np.abs(r)))
        print(f"{terms_name} {lik_name}: {name} error {e:.3e}")
        assert e <= TOL


@pytest.mark.parametrize("lik_name", ["bernoulli", "poisson"])
def test_repeatable_and_independent_of_the_query_shape(ctx, lik_name):
    c = LO.case(300, 1000, "composite", lik_name)
    Xs = c["Xs"][:257]
    with lfit(ctx, c, 128) as fit, lfit(ctx, c, 1024) as big:
        m, v = fit.mean_var(Xs)
        m2, v2 = fit.mean_var(Xs)
        assert np.array_equal(m, m2) and np.array_equal(v, v2)
        mm = fit.mean(Xs)
        assert np.array_equal(mm, fit.mean(Xs))
        assert np.array_equal(fit.alpha(), big.alpha()) and np.array_equal(fit.f_hat(), big.f_hat())
        C = fit.mean_cov(Xs[:100])[1]
        assert np.array_equal(C, fit.mean_cov(Xs[:100])[1])

        def same(a, b):
            assert np.max(np.abs(a - b)) <= 1e-13 * max(1.0, np.max(np.abs(b)))

        mr, vr = fit.mean_var(Xs[::-1])
        same(mr[::-1], m)
        same(vr[::-1], v)
        same(fit.mean(Xs[::-1])[::-1], mm)
        for j in (0, 127, 128, 256):
            m1, v1 = fit.mean_var(Xs[j:j + 1])
            same(m1, m[j:j + 1])
            same(v1, v[j:j + 1])
            same(fit.mean(Xs[j:j + 1]), mm[j:j + 1])
        mb, vb = big.mean_var(Xs)
        same(mb, m)
        same(vb, v)
        same(big.mean(Xs), mm)


def test_the_context_stays_free_between_queries(ctx):
    c = LO.case(300, 1000, "composite", "poisson")
    o = LO.case(127, 129, "composite", "bernoulli")
    X2, Xs2, y2, rm2, rv2, kd2, _ = TF.oracle(513, 513)
    with lfit(ctx, c, 128) as fit:
        before = fit.mean_var(c["Xs"]), fit.mean(c["Xs"]), fit.alpha(), fit.f_hat(), fit.mean_cov(c["Xs"][:100])[1]
        lp = ctx.logpdf(X2, TF.COMPOSITE, 0.1, y2)
        ctx.logpdf_grad(X2, TF.COMPOSITE, 0.2, y2)
        g = ctx.laplace_logpdf_grad(o["X"], o["terms"], LO.JITTER, o["lik"], o["y"])
        with ctx.fit(X2, TF.COMPOSITE, 0.1, y2, cap=128) as exact, lfit(ctx, o, 128) as second:
            after = fit.mean_var(c["Xs"]), fit.mean(c["Xs"]), fit.alpha(), fit.f_hat(), fit.mean_cov(c["Xs"][:100])[1]
            close_to(*exact.mean_var(Xs2), rm2, rv2, kd2, "exact fit beside a Laplace fit")
            close_to(*second.mean_var(o["Xs"]), o["mean"], o["var"], o["kdiag"], "second Laplace fit")
            assert exact.logpdf == lp
        assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
        assert all(np.array_equal(b, a) for b, a in zip(before[1:], after[1:]))
        assert abs(g.logq - o["res"].logq) <= TOL * max(1.0, abs(o["res"].logq))


def test_a_non_finite_w_gives_no_handle(ctx):
    c = LO.case(129, 1, "sqexp", "poisson")
    a0 = np.full(129, 1e3)
    with np.errstate(over="ignore"):
        assert not np.all(np.isfinite(LO.lik_terms(c["lik"], 0.0, c["y"], c["res"].K @ a0)[2]))  # the oracle's W
    with pytest.raises(PosDefException) as e:
        lfit(ctx, c, a0=a0)
    assert e.value.info > 0
    assert ctx.lib.gaplac_last_error(ctx.h).decode().startswith("B = I + sqrt(W) K sqrt(W)")
    with lfit(ctx, c) as fit:  # the context goes on
        close_to(*fit.mean_var(c["Xs"]), c["mean"], c["var"], c["kdiag"], "after a failed create")


def test_max_iter_1_gives_a_handle_of_the_last_iterate(ctx):
    c = LO.case(300, 1000, "composite", "poisson")
    with pytest.warns(RuntimeWarning, match="did not converge"):
        fit = lfit(ctx, c, 128, max_iter=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rm, rv = ctx.laplace_posterior_mean_var(c["X"], c["terms"], LO.JITTER, c["lik"], c["y"], c["Xs"], max_iter=1)
        ref = one_shot(ctx, c, max_iter=1)
    with fit:
        assert fit.converged is False and fit.iters == 1 and fit.logq == ref.logq
        m, v = fit.mean_var(c["Xs"])
        em = np.max(np.abs(m - rm)) / max(1.0, np.max(np.abs(rm)))
        ev = np.max(np.abs(v - rv) / np.maximum(1.0, np.abs(c["kdiag"])))
        print(f"max_iter=1: mean {em:.3e}, variance {ev:.3e} against the one-shot entry")
        assert em <= 1e-11 and ev <= 1e-11


def test_edges(ctx):
    Xs = LO.inputs(5, 3)[1]
    X0 = np.zeros((0, Xs.shape[1]))
    kd = R.kernel_diag(Xs, LO.COMPOSITE)
    with ctx.laplace_fit(X0, LO.COMPOSITE, LO.JITTER, "poisson", np.zeros(0)) as fit:  # N = 0: the prior
        assert fit.N == 0 and fit.logq == 0.0 and fit.converged and fit.iters == 0 and fit.kind == "laplace"
        m, v = fit.mean_var(Xs)
        assert np.all(m == 0.0) and np.allclose(v, kd, rtol=1e-15, atol=0)
        assert np.all(fit.mean(Xs) == 0.0) and fit.alpha().shape == (0,) and fit.f_hat().shape == (0,)
        m, C = fit.mean_cov(Xs, 0.05)
        assert np.all(m == 0.0) and np.max(np.abs(C - R.gram(Xs, LO.COMPOSITE, 0.05))) <= TOL * max(1.0, kd.max())
        ym, yv = fit.predict(Xs)
        assert np.max(np.abs(ym - np.exp(0.5 * kd)) / np.exp(0.5 * kd)) <= 1e-12
    c = LO.case(5, 3, "composite", "bernoulli")
    fit = lfit(ctx, c, 1)
    m, v = fit.mean_var(np.zeros((0, 3)))  # M = 0 writes nothing
    assert m.shape == v.shape == (0,) and fit.mean(np.zeros((0, 3))).shape == (0,)
    with pytest.raises(ArgumentError):
        fit.mean_var(np.zeros((4, 2)))
    with pytest.raises(ArgumentError, match="cap"):
        fit.mean_cov(c["Xs"][:2])  # M = cap + 1
    lib, nan, X = ctx.lib, np.full(3, 7.0), c["X"]
    assert lib.gaplac_fit_mean_var(fit.h, 3, X.ctypes.data, 2, nan.ctypes.data, nan.ctypes.data) == -1  # ldxs < M
    assert np.all(np.isnan(nan))  # NaN-filled first
    for kw in (dict(cap=0), dict(max_iter=0), dict(tol=0.0)):
        with pytest.raises(ArgumentError):
            lfit(ctx, c, **kw)
    with pytest.raises(ArgumentError):
        ctx.laplace_fit(c["X"], c["terms"], LO.JITTER, "bernoulli", c["y"] + 2.0)
    assert np.all(np.isfinite(fit.mean_var(c["Xs"])[0]))  # usable after every failure
    fit.close()
    fit.close()
    with pytest.raises(ArgumentError):
        fit.mean_var(c["Xs"])
    with pytest.raises(ArgumentError):
        fit.f_hat()


def test_a_fit_whose_context_is_closed():
    if not gpu_available():
        pytest.skip("no GPU")
    c = LO.case(5, 3, "composite", "poisson")
    ctx = Context(0)
    fit = lfit(ctx, c)
    ctx.close()
    for call in (lambda: fit.mean_var(c["Xs"]), fit.alpha, fit.f_hat, lambda: fit.mean_cov(c["Xs"])):
        with pytest.raises(ArgumentError):
            call()
    fit.close()


def test_columns_of_the_persistent_tail_agree_with_the_one_shot_call(ctx):
    # the inputs of test_gpu_fit's test of the same name (N = 12000, 94 tile columns), y := 1 where
    # that y > 0, Bernoulli: B's last columns are factored inside the persistent tail and the query
    # solves the rows against them with the super-panel launches. No CPU oracle at this size.
    rng = np.random.default_rng(41)
    N, M = 12000, 1024
    X = np.column_stack([rng.uniform(0, 10, N), rng.integers(0, N // 3, N).astype(float)])
    Xs = np.column_stack([rng.uniform(0, 10, M), rng.integers(0, N // 3, M).astype(float)])
    y = (rng.normal(size=N) > 0).astype(np.float64)
    terms = [(_native.SQEXP, 0, 1.5, 0), (_native.OU, 0, 3.0, 1), (_native.CAT, 1, 0.0, 2), (_native.NOISE, -1, 0.1, 3)]
    m1, v1 = ctx.laplace_posterior_mean_var(X, terms, LO.JITTER, "bernoulli", y, Xs)
    with ctx.laplace_fit(X, terms, LO.JITTER, "bernoulli", y, cap=1024) as fit:
        m2, v2 = fit.mean_var(Xs)
    em = np.max(np.abs(m1 - m2)) / max(1.0, np.max(np.abs(m1)))
    ev = np.max(np.abs(v1 - v2)) / max(1.0, np.max(np.abs(v1)))
    print(f"N=12000: mean {em:.3e}, variance {ev:.3e} of the bar's scale")
    assert em <= 1e-11 and ev <= 1e-11


def test_abstractgps_surface(ctx):
    c = LO.case(127, 129, "composite", "bernoulli")
    lgp = AG.LatentGP(_gp_of(c["terms"]), AG.BernoulliLikelihood(), LO.JITTER)
    cols = [0, 0, 1, 2]
    xs = c["Xs"][:, cols]
    post = AG.posterior(AG.LaplaceApproximation(), lgp(c["X"][:, cols]), c["y"], ctx=ctx)
    ys = (np.arange(129) % 2).astype(np.float64)
    with post.fit(cap=256) as fp, lfit(ctx, c, 256) as fit:
        assert isinstance(fp, AG.FittedLaplacePosteriorGP)
        m, v = fp.mean_and_var(xs)
        bm, bv = fit.mean_var(c["Xs"])
        assert np.array_equal(m, bm) and np.array_equal(v, bv)
        assert np.array_equal(fp.mean(xs), fit.mean(c["Xs"])) and np.array_equal(fp.var(xs), bv)
        assert all(np.array_equal(a, b) for a, b in zip(fp.mean_and_cov(xs, 0.05), fit.mean_cov(c["Xs"], 0.05)))
        assert all(np.array_equal(a, b) for a, b in zip(fp.predict(xs, ys), fit.predict(c["Xs"], ys)))
        assert np.array_equal(fp.f_hat, post.f_hat) and fp.logq == post.logq
        close_to(m, v, c["mean"], c["var"], c["kdiag"], "abstractgps")
    with post.fit() as warm:  # the mode now known: the fit starts from it
        assert abs(warm.logq - post.logq) <= 1e-12 * max(1.0, abs(post.logq))
