"""The fitted posterior (gaplac_fit_*, HIP through the C-ABI): factor once, query many test sets.

Bars (those of tests/test_gpu_posterior.py): mean within 1e-9 max(1, max |mean|), variance within
1e-9 max(1, kdiag), both against oracle.restatement.posterior_mean_var. The matrix-free mean
K(xs, X) alpha is a different arithmetic from the oracle's; on these inputs a numpy cho_solve
alpha route differs from the oracle by at most 9.3e-13 of the bar's scale (2.1e-12 at N = 2000),
so the bar leaves more than two orders of margin. alpha() within 1e-9 max |alpha| of
scipy.linalg.cho_solve on the oracle's Gram matrix. Where no rule forces bitwise equality (a row
queried at another position, in a set of another size, or under another cap) results agree to
1e-13 relative, the bar of tests/test_gpu_components.py; identical calls are bitwise equal.
"""
import numpy as np
import pytest
import scipy.linalg

from gaplac_amd import abstractgps as AG
from gaplac_amd import formula as F
from gaplac_amd._native import CAT, LINEAR, NOISE, OU, SQEXP
from gaplac_amd.backend import ArgumentError, Context, PosDefException
from oracle import restatement as R
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
TOL = 1e-9
SIZES = [(1, 1), (5, 3), (127, 129), (128, 128), (129, 1), (300, 1000), (700, 257), (1000, 64), (513, 513)]
COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (LINEAR, 2, 0.5, 3)]


@pytest.fixture(scope="module")
def ctx():
    if not gpu_available():
        pytest.skip("no GPU")
    c = Context(0)
    yield c
    c.close()


def composite(N, M):
    """The inputs of test_gpu_posterior.test_sizes_composite."""
    rng = np.random.default_rng(N * 7 + M)

    def cols(n):
        return np.column_stack([rng.uniform(0, 10, n), rng.integers(0, 40, n).astype(float), rng.normal(size=n)])

    X, Xs = cols(N), cols(M)
    y = rng.normal(size=N)
    return X, Xs, y


_oracle = {}


def oracle(N, M):
    """(X, Xs, y, mean, var, kdiag, alpha) of one composite case, computed once."""
    if (N, M) not in _oracle:
        X, Xs, y = composite(N, M)
        rm, rv = R.posterior_mean_var(X, COMPOSITE, 0.1, y, Xs)
        kd = R.kernel_diag(Xs, COMPOSITE)
        C = R.gram(X, COMPOSITE, 0.1)
        ra = scipy.linalg.cho_solve(scipy.linalg.cho_factor(C, lower=True), y)
        for a in (X, Xs, y, rm, rv, kd, ra):
            a.setflags(write=False)
        _oracle[(N, M)] = (X, Xs, y, rm, rv, kd, ra)
    return _oracle[(N, M)]


def close_to(m, v, rm, rv, kd, what):
    em = np.max(np.abs(m - rm)) / max(1.0, np.max(np.abs(rm)))
    print(f"{what}: mean error {em:.3e} of the bar's scale")
    assert em <= TOL
    if v is not None:
        ev = np.max(np.abs(v - rv) / np.maximum(1.0, np.abs(kd)))
        print(f"{what}: variance error {ev:.3e} of the bar's scale")
        assert ev <= TOL


@pytest.mark.parametrize("cap", [128, 1024])
@pytest.mark.parametrize("N,M", SIZES)
def test_sizes_composite(ctx, N, M, cap):
    X, Xs, y, rm, rv, kd, ra = oracle(N, M)
    with ctx.fit(X, COMPOSITE, 0.1, y, cap=cap) as fit:
        assert (fit.N, fit.cap) == (N, cap)
        m, v = fit.mean_var(Xs)
        close_to(m, v, rm, rv, kd, f"mean_var N={N} M={M} cap={cap}")
        close_to(fit.mean(Xs), None, rm, rv, kd, f"mean N={N} M={M} cap={cap}")
        a = fit.alpha()
        ea = np.max(np.abs(a - ra)) / np.max(np.abs(ra))
        print(f"alpha N={N}: error {ea:.3e} of max |alpha|")
        assert ea <= TOL


def test_product_groups_and_noise_term(ctx):
    rng = np.random.default_rng(12)
    N, M = 260, 190
    X = np.column_stack([rng.uniform(0, 5, N), rng.normal(size=N)])
    Xs = np.column_stack([rng.uniform(0, 5, M), rng.normal(size=M)])
    terms = [(SQEXP, 0, 1.3, 0), (LINEAR, 1, 0.4, 0), (OU, 0, 2.5, 1), (NOISE, -1, 0.2, 2)]
    y = rng.normal(size=N)
    rm, rv = R.posterior_mean_var(X, terms, 0.1, y, Xs)
    kd = R.kernel_diag(Xs, terms)
    for cap in (128, 1024):
        with ctx.fit(X, terms, 0.1, y, cap=cap) as fit:
            m, v = fit.mean_var(Xs)
            close_to(m, v, rm, rv, kd, f"groups mean_var cap={cap}")
            close_to(fit.mean(Xs), None, rm, rv, kd, f"groups mean cap={cap}")


def test_fit_value_is_the_logpdf_entrys(ctx):
    for N, M in ((5, 3), (300, 1000), (1000, 64)):
        X, Xs, y = oracle(N, M)[:3]
        lp, ld, q = ctx.logpdf(X, COMPOSITE, 0.1, y, full=True)
        with ctx.fit(X, COMPOSITE, 0.1, y) as fit:
            assert fit.logpdf == lp and fit.logdet == ld and fit.quad == q


def test_repeatable_and_independent_of_the_query_shape(ctx):
    X, Xs, y = oracle(700, 257)[:3]
    with ctx.fit(X, COMPOSITE, 0.1, y, cap=128) as fit, ctx.fit(X, COMPOSITE, 0.1, y, cap=1024) as big:
        m, v = fit.mean_var(Xs)
        m2, v2 = fit.mean_var(Xs)
        assert np.array_equal(m, m2) and np.array_equal(v, v2)
        mm = fit.mean(Xs)
        assert np.array_equal(mm, fit.mean(Xs))
        assert np.array_equal(fit.alpha(), fit.alpha())
        assert np.array_equal(fit.alpha(), big.alpha())  # two fits of the same data

        def same(a, b):
            assert np.max(np.abs(a - b)) <= 1e-13 * max(1.0, np.max(np.abs(b)))

        mr, vr = fit.mean_var(Xs[::-1])  # reversed: every row at another position, in another chunk
        same(mr[::-1], m)
        same(vr[::-1], v)
        same(fit.mean(Xs[::-1])[::-1], mm)
        for j in (0, 127, 128, 256):  # one row alone
            m1, v1 = fit.mean_var(Xs[j:j + 1])
            same(m1, m[j:j + 1])
            same(v1, v[j:j + 1])
            same(fit.mean(Xs[j:j + 1]), mm[j:j + 1])
        mb, vb = big.mean_var(Xs)  # another cap: one chunk instead of three
        same(mb, m)
        same(vb, v)
        same(big.mean(Xs), mm)


def test_the_context_stays_free_between_queries(ctx):
    X, Xs, y = oracle(300, 1000)[:3]
    X2, Xs2, y2 = oracle(513, 513)[:3]
    with ctx.fit(X, COMPOSITE, 0.1, y, cap=128) as fit:
        before = fit.mean_var(Xs), fit.mean(Xs), fit.alpha()
        # other data through the same context: its workspace is overwritten three times
        ctx.logpdf(X2, COMPOSITE, 0.2, y2)
        ctx.logpdf_grad(X2, COMPOSITE, 0.2, y2)
        m2, v2 = ctx.posterior_mean_var(X2, COMPOSITE, 0.1, y2, Xs2)
        with ctx.fit(X2, COMPOSITE, 0.1, y2, cap=128) as other:  # two fits alive on one context
            after = fit.mean_var(Xs), fit.mean(Xs), fit.alpha()
            mo, vo = other.mean_var(Xs2)
        assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
        assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
        _, _, _, rm, rv, kd, _ = oracle(513, 513)
        close_to(mo, vo, rm, rv, kd, "second fit")
        close_to(m2, v2, rm, rv, kd, "one-shot call between the queries")


def test_edges(ctx):
    terms = [(SQEXP, 0, 1.0, 0), (LINEAR, 0, 0.5, 1)]
    Xs = np.linspace(0, 1, 7)[:, None]
    with ctx.fit(np.zeros((0, 1)), terms, 0.1, np.zeros(0)) as fit:  # N = 0: the prior
        assert fit.N == 0 and fit.logpdf == 0.0
        m, v = fit.mean_var(Xs)
        assert np.all(m == 0.0) and np.allclose(v, R.kernel_diag(Xs, terms), rtol=0, atol=1e-15)
        assert np.all(fit.mean(Xs) == 0.0) and fit.alpha().shape == (0,)
    X, _, y = oracle(5, 3)[:3]
    fit = ctx.fit(X, COMPOSITE, 0.1, y, cap=1)
    m, v = fit.mean_var(np.zeros((0, 3)))  # M = 0 writes nothing
    assert m.shape == v.shape == (0,) and fit.mean(np.zeros((0, 3))).shape == (0,)
    with pytest.raises(ArgumentError):
        fit.mean_var(np.zeros((4, 2)))  # another number of columns
    lib, nan = ctx.lib, np.full(3, 7.0)
    assert lib.gaplac_fit_mean_var(fit.h, -1, None, 0, None, nan.ctypes.data) == -1
    assert lib.gaplac_fit_mean_var(fit.h, 3, X.ctypes.data, 2, nan.ctypes.data, nan.ctypes.data) == -1  # ldxs < M
    assert np.all(np.isnan(nan))  # NaN-filled first
    assert lib.gaplac_fit_mean(fit.h, 3, None, 3, nan.ctypes.data) == -1
    assert lib.gaplac_fit_mean(fit.h, 3, X.ctypes.data, 5, None) == -1
    with pytest.raises(ArgumentError):
        ctx.fit(X, COMPOSITE, 0.1, y, cap=0)
    with pytest.raises(ArgumentError):
        ctx.fit(X, COMPOSITE, 0.1, y[:-1])
    assert np.all(np.isfinite(fit.mean_var(X)[0]))  # usable after every failure
    fit.close()
    fit.close()
    with pytest.raises(ArgumentError):
        fit.mean_var(X)
    with pytest.raises(ArgumentError):
        fit.alpha()


def test_nonpd_raises_and_the_context_stays_usable(ctx):
    X = np.repeat(np.arange(8.0), 4)[:, None]
    with pytest.raises(PosDefException):
        ctx.fit(X, [(CAT, 0, 0.0, 0)], 0.0, np.ones(32))
    assert b"positive definite" in ctx.lib.gaplac_last_error(ctx.h)
    Xc, Xs, y, rm, rv, kd, _ = oracle(5, 3)
    with ctx.fit(Xc, COMPOSITE, 0.1, y) as fit:
        close_to(*fit.mean_var(Xs), rm, rv, kd, "after a PosDefException")


def test_a_fit_whose_context_is_closed():
    if not gpu_available():
        pytest.skip("no GPU")
    X, Xs, y = oracle(5, 3)[:3]
    c = Context(0)
    fit = c.fit(X, COMPOSITE, 0.1, y)
    c.close()
    with pytest.raises(ArgumentError):
        fit.mean_var(Xs)
    with pytest.raises(ArgumentError):
        fit.alpha()
    fit.close()


def test_columns_of_the_persistent_tail_agree_with_the_one_shot_call(ctx):
    # N = 12000 (94 tile columns), the inputs of test_gpu_posterior.test_tail_and_superpanel_paths_agree:
    # the plain evaluation behind the fit factors its last columns inside the persistent tail, and
    # the query solves the rows against them with the super-panel launches
    rng = np.random.default_rng(41)
    N, M = 12000, 1024
    X = np.column_stack([rng.uniform(0, 10, N), rng.integers(0, N // 3, N).astype(float)])
    Xs = np.column_stack([rng.uniform(0, 10, M), rng.integers(0, N // 3, M).astype(float)])
    y = rng.normal(size=N)
    terms = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (NOISE, -1, 0.1, 3)]
    m1, v1 = ctx.posterior_mean_var(X, terms, 0.1, y, Xs)
    with ctx.fit(X, terms, 0.1, y, cap=1024) as fit:
        m2, v2 = fit.mean_var(Xs)
    em = np.max(np.abs(m1 - m2)) / max(1.0, np.max(np.abs(m1)))
    ev = np.max(np.abs(v1 - v2)) / max(1.0, np.max(np.abs(v1)))
    print(f"N=12000: mean {em:.3e}, variance {ev:.3e} of the bar's scale")
    assert em <= 1e-11 and ev <= 1e-11


def test_large_n_properties(ctx):
    N = 16384
    rng = np.random.default_rng(2)
    t = rng.uniform(0, 10, N)
    g = rng.integers(0, N // 3, N).astype(float)
    X = np.column_stack([t, g])
    y = rng.normal(size=N)
    terms = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2)]
    idx = rng.choice(N, 600, replace=False)
    bar = 1e-8 * max(1.0, np.max(np.abs(y)))
    with ctx.fit(X, terms, 0.1, y) as fit:
        alpha = fit.alpha()
        m, v = fit.mean_var(X[idx])
        mm = fit.mean(X[idx])
    _, dv, _, _ = ctx.logpdf_grad(X, terms, 0.1, y)  # dv = -alpha
    e1 = np.max(np.abs(m - (y[idx] - 0.1 * alpha[idx])))
    e2 = np.max(np.abs(mm - (y[idx] - 0.1 * alpha[idx])))
    e3 = np.max(np.abs(alpha + dv))
    print(f"N=16384: mean_var {e1:.3e}, mean {e2:.3e}, alpha {e3:.3e} (bar {bar:.3e})")
    assert e1 <= bar and e2 <= bar and e3 <= bar
    assert np.all(v > 0) and np.all(v < 3.0)


def test_abstractgps_surface(ctx):
    # src/plotting.jl:1-12 with the posterior fitted once: mean_and_var over a 100-point range
    rng = np.random.default_rng(13)
    N = 400
    x = rng.uniform(-5, 5, N)
    y = np.sin(x) + 0.3 * rng.normal(size=N)
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))
    fx = AG.FiniteGP(gp, x, 0.1)
    xt = np.linspace(x.min() - 1, x.max() + 1, 100)
    rm, rv = R.posterior_mean_var(x[:, None], fx.terms, 0.1, y, xt[:, None])
    with AG.posterior(fx, y, ctx=ctx).fit() as fp:
        assert isinstance(fp, AG.FittedPosteriorGP)
        m, v = AG.mean_and_var(fp, xt)
        assert np.max(np.abs(m - rm)) <= TOL * max(1.0, np.max(np.abs(rm)))
        assert np.max(np.abs(v - rv)) <= TOL
        assert np.max(np.abs(fp.mean(xt) - rm)) <= TOL * max(1.0, np.max(np.abs(rm)))
        assert np.array_equal(fp.var(xt), v)
