"""Parity of the joint posterior entries gaplac_posterior_mean_cov / _rand / _logpdf (HIP,
through the C-ABI) against the CPU recipe of tests/joint_oracle.py (pinned to scikit-learn by
tests/test_joint_oracle.py), and against gaplac_posterior_mean_var.

Bars (the project's north-star 1e-9): mean within 1e-9 max(1, max |mean|); every entry of
Sigma* within 1e-9 max(1, max kernel_diag(Xs)) (the variance bar of tests/test_gpu_posterior.py)
and exactly symmetric; draws within 1e-9 max(1, max |draw|); logpdf 1e-9 relative, logdet and
quad as tests/test_gpu_multi.py judges them. The draws pass through a difference of matrices
and a second Cholesky, hence 1e-9 and not gaplac_rand's 1e-12: two CPU routes to the reference
differ by at most 7.0e-13 of max |draw| and 4.4e-13 relative in logpdf on these inputs.
"""
from ctypes import byref, c_double, c_void_p

import numpy as np
import pytest

from gaplac_amd import abstractgps as AG
from gaplac_amd import formula as F
from gaplac_amd._native import CAT, LINEAR, NOISE, OU, SQEXP, term_array
from gaplac_amd.backend import ArgumentError, Context, PosDefException
from oracle import restatement as R
from tests import joint_oracle as J
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
TOL = 1e-9
COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (LINEAR, 2, 0.5, 3)]
SIZES = [(1, 1), (5, 3), (127, 129), (128, 128), (129, 1), (300, 1000), (700, 257), (513, 513), (1000, 64)]
_cases = {}


def case(N, M):
    if (N, M) not in _cases:
        _cases[(N, M)] = J.Case(N, M, COMPOSITE)
    return _cases[(N, M)]


@pytest.fixture(scope="module")
def ctx():
    if not gpu_available():
        pytest.skip("no GPU")
    c = Context(0)
    yield c
    c.close()


def check_cov(S, ref, kd):
    bar = TOL * max(1.0, np.max(kd))
    print("max |cov - oracle|", np.max(np.abs(S - ref)), "bar", bar)
    assert np.max(np.abs(S - ref)) <= bar
    assert np.array_equal(S, S.T)


def check_logpdf(got, ref):
    (lp, ld, q), (rl, rd, rq) = got, ref
    print("max rel logpdf", np.max(np.abs(lp - rl) / np.abs(rl)), "logdet", abs(ld - rd), "quad", np.max(np.abs(q - rq)))
    assert np.all(np.abs(lp - rl) <= TOL * np.abs(rl))
    assert abs(ld - rd) <= TOL * np.min(np.abs(rl))
    assert np.all(np.abs(q - rq) <= TOL * np.abs(rl))


@pytest.mark.parametrize("N,M", SIZES)
def test_mean_and_cov(ctx, N, M):
    c = case(N, M)
    for noise_s, ref in ((0.0, c.cov0), (0.1, c.cov)):
        m, S = ctx.posterior_mean_cov(c.X, COMPOSITE, 0.1, c.y, c.Xs, noise_s)
        print("max |mean - oracle|", np.max(np.abs(m - c.mean)))
        assert np.max(np.abs(m - c.mean)) <= TOL * max(1.0, np.max(np.abs(c.mean)))
        check_cov(S, ref, c.kd)


@pytest.mark.parametrize("N,M", SIZES)
def test_draws_and_logpdf(ctx, N, M):
    c = case(N, M)
    D = ctx.posterior_rand(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1, c.Z)
    bar = TOL * max(1.0, np.max(np.abs(c.draws)))
    print("max |draw - oracle|", np.max(np.abs(D - c.draws)), "bar", bar)
    assert D.shape == c.draws.shape and np.max(np.abs(D - c.draws)) <= bar
    got = ctx.posterior_logpdf(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1, c.Ys, full=True)
    assert got[0].shape == (5,) and got[2].shape == (5,)
    check_logpdf(got, c.lp)


def test_product_groups_and_noise_term(ctx):
    rng = np.random.default_rng(12)
    N, M = 260, 190
    X = np.column_stack([rng.uniform(0, 5, N), rng.normal(size=N)])
    Xs = np.column_stack([rng.uniform(0, 5, M), rng.normal(size=M)])
    terms = [(SQEXP, 0, 1.3, 0), (LINEAR, 1, 0.4, 0), (OU, 0, 2.5, 1), (NOISE, -1, 0.2, 2)]
    y = rng.normal(size=N)
    Z = rng.normal(size=(M, 3))
    kd = R.kernel_diag(Xs, terms)
    for noise_s in (0.0, 0.1):
        rm, rS = J.mean_cov(X, terms, 0.1, y, Xs, noise_s)
        m, S = ctx.posterior_mean_cov(X, terms, 0.1, y, Xs, noise_s)
        assert np.max(np.abs(m - rm)) <= TOL * max(1.0, np.max(np.abs(rm)))
        check_cov(S, rS, kd)
    ref = J.draws(rm, rS, Z)
    D = ctx.posterior_rand(X, terms, 0.1, y, Xs, 0.1, Z)
    assert np.max(np.abs(D - ref)) <= TOL * max(1.0, np.max(np.abs(ref)))
    Ys = ref + 0.3 * rng.normal(size=(M, 3))
    check_logpdf(ctx.posterior_logpdf(X, terms, 0.1, y, Xs, 0.1, Ys, full=True), J.logpdf(rm, rS, Ys))


def test_abstractgps_surface(ctx):
    rng = np.random.default_rng(13)
    N, M = 400, 100
    x = rng.uniform(-5, 5, N)
    y = np.sin(x) + 0.3 * rng.normal(size=N)
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))
    fx = AG.FiniteGP(gp, x, 0.1)
    xt = np.linspace(x.min() - 1, x.max() + 1, M)
    fp = AG.posterior(fx, y, ctx=ctx)
    fpx = fp(xt, 0.05)
    assert len(fpx) == M
    rm, rS = J.mean_cov(x[:, None], fx.terms, 0.1, y, xt[:, None], 0.05)
    m, S = AG.mean_and_cov(fpx)
    assert np.max(np.abs(m - rm)) <= TOL * max(1.0, np.max(np.abs(rm)))
    check_cov(S, rS, np.ones(M))
    assert np.array_equal(AG.cov(fpx), S)
    a = AG.rand(fpx, n=4, rng=np.random.default_rng(1))
    Z = np.random.default_rng(1).standard_normal((M, 4))
    b = AG.rand(fpx, z=Z)
    ref = J.draws(rm, rS, Z)
    assert a.shape == (M, 4) and np.array_equal(a, b)
    assert np.max(np.abs(a - ref)) <= TOL * max(1.0, np.max(np.abs(ref)))
    one = AG.rand(fpx, z=Z[:, 2])
    assert one.shape == (M,) and np.max(np.abs(one - b[:, 2])) <= 1e-13 * max(1.0, np.max(np.abs(one)))
    assert AG.rand(fpx, rng=np.random.default_rng(1)).shape == (M,)
    Ys = ref + 0.3 * rng.normal(size=(M, 4))
    lp = AG.logpdf(fpx, Ys)
    rl = J.logpdf(rm, rS, Ys)[0]
    assert lp.shape == (4,) and np.all(np.abs(lp - rl) <= TOL * np.abs(rl))
    s = AG.logpdf(fpx, Ys[:, 1])
    assert np.ndim(s) == 0 and abs(s - rl[1]) <= TOL * abs(rl[1])
    with pytest.raises(F.ArgumentError):
        AG.logpdf(fpx, Ys[:-1])
    with pytest.raises(F.ArgumentError):
        AG.rand(fpx, z=Z[:-1])
    # a prior FiniteGP goes where it went before
    assert AG.rand(fx, n=2, rng=np.random.default_rng(1), ctx=ctx).shape == (N, 2)
    assert np.ndim(AG.logpdf(fx, y, ctx=ctx)) == 0


def raw_head(ctx, X, terms, noise, y, Xs, noise_s):
    Xc, Xsc = np.asfortranarray(X, dtype=np.float64), np.asfortranarray(Xs, dtype=np.float64)
    yc = np.ascontiguousarray(y, dtype=np.float64)
    (N, D), M = Xc.shape, Xsc.shape[0]
    keep = (Xc, Xsc, yc)
    return keep, (ctx.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), term_array(terms), float(noise),
                  yc.ctypes.data_as(c_void_p), M, Xsc.ctypes.data_as(c_void_p), max(M, 1), float(noise_s))


def P(a):
    return a.ctypes.data_as(c_void_p)


def test_leading_dimensions_and_padding_rows(ctx):
    c = case(127, 129)
    M, Rn = 129, 5
    keep, head = raw_head(ctx, c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1)
    m, S = ctx.posterior_mean_cov(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1)
    mo = np.empty(M)
    So = np.full((M + 3, M), -7.5, order="F")
    assert ctx.lib.gaplac_posterior_mean_cov(*head, P(mo), P(So), M + 3) == 0
    assert np.array_equal(mo, m) and np.array_equal(So[:M], S) and np.all(So[M:] == -7.5)
    # either output may be NULL
    mo2 = np.empty(M)
    assert ctx.lib.gaplac_posterior_mean_cov(*head, P(mo2), None, 0) == 0 and np.array_equal(mo2, m)
    So2 = np.empty((M, M), order="F")
    assert ctx.lib.gaplac_posterior_mean_cov(*head, None, P(So2), M) == 0 and np.array_equal(So2, S)
    D = ctx.posterior_rand(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1, c.Z)
    Zp = np.full((M + 5, Rn), np.nan, order="F")
    Zp[:M] = c.Z
    out = np.full((M + 7, Rn), -7.5, order="F")
    assert ctx.lib.gaplac_posterior_rand(*head, Rn, P(Zp), M + 5, P(out), M + 7) == 0
    assert np.array_equal(out[:M], D) and np.all(out[M:] == -7.5)
    ref = ctx.posterior_logpdf(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1, c.Ys, full=True)
    Yp = np.full((M + 2, Rn), np.nan, order="F")
    Yp[:M] = c.Ys
    lp, q, ld = np.empty(Rn), np.empty(Rn), c_double()
    assert ctx.lib.gaplac_posterior_logpdf(*head, Rn, P(Yp), M + 2, P(lp), byref(ld), P(q)) == 0
    assert np.array_equal(lp, ref[0]) and ld.value == ref[1] and np.array_equal(q, ref[2])
    lp2 = np.empty(Rn)
    assert ctx.lib.gaplac_posterior_logpdf(*head, Rn, P(Yp), M + 2, P(lp2), None, None) == 0
    assert np.array_equal(lp2, ref[0])


def test_empty_inputs(ctx):
    terms = [(SQEXP, 0, 1.0, 0), (LINEAR, 0, 0.5, 1)]
    X = np.arange(6.0)[:, None]
    y = np.ones(6)
    Xs = np.linspace(0, 1, 4)[:, None]
    # M = 0
    m, S = ctx.posterior_mean_cov(X, terms, 0.1, y, np.zeros((0, 1)), 0.1)
    assert m.shape == (0,) and S.shape == (0, 0)
    assert ctx.posterior_rand(X, terms, 0.1, y, np.zeros((0, 1)), 0.1, np.zeros((0, 3))).shape == (0, 3)
    keep, head0 = raw_head(ctx, X, terms, 0.1, y, np.zeros((0, 1)), 0.1)
    can, ldv = np.full(3, -7.5), c_double(-7.5)
    assert ctx.lib.gaplac_posterior_logpdf(*head0, 3, None, 0, P(can), byref(ldv), P(can)) == 0
    assert np.all(can == -7.5) and ldv.value == -7.5
    out = np.full((2, 3), -7.5, order="F")
    assert ctx.lib.gaplac_posterior_rand(*head0, 3, None, 0, P(out), 2) == 0 and np.all(out == -7.5)
    assert ctx.lib.gaplac_posterior_mean_cov(*head0, P(can), P(out), 2) == 0
    assert np.all(can == -7.5) and np.all(out == -7.5)
    # R = 0
    assert ctx.posterior_rand(X, terms, 0.1, y, Xs, 0.1, np.zeros((4, 0))).shape == (4, 0)
    lp, ld, q = ctx.posterior_logpdf(X, terms, 0.1, y, Xs, 0.1, np.zeros((4, 0)), full=True)
    assert lp.shape == (0,) and q.shape == (0,)
    keep, head = raw_head(ctx, X, terms, 0.1, y, Xs, 0.1)
    assert ctx.lib.gaplac_posterior_logpdf(*head, 0, None, 4, P(can), byref(ldv), P(can)) == 0
    assert np.all(can == -7.5) and ldv.value == -7.5
    out = np.full((6, 3), -7.5, order="F")
    assert ctx.lib.gaplac_posterior_rand(*head, 0, None, 4, P(out), 6) == 0 and np.all(out == -7.5)
    # bad terms are reported before the empty return
    with pytest.raises(ArgumentError):
        ctx.posterior_rand(X, [(SQEXP, 0, -1.0, 0)], 0.1, y, Xs, 0.1, np.zeros((4, 0)))
    # N = 0: the prior at the test points
    X0, y0 = np.zeros((0, 1)), np.zeros(0)
    m, S = ctx.posterior_mean_cov(X0, terms, 0.1, y0, Xs, 0.2)
    assert np.all(m == 0.0) and np.array_equal(S, ctx.gram(Xs, terms, 0.2))
    assert np.max(np.abs(S - R.gram(Xs, terms, 0.2))) <= 1e-12
    Z = np.random.default_rng(3).normal(size=(4, 3))
    assert np.array_equal(ctx.posterior_rand(X0, terms, 0.1, y0, Xs, 0.2, Z), ctx.rand_multi(Xs, terms, 0.2, Z))
    a = ctx.posterior_logpdf(X0, terms, 0.1, y0, Xs, 0.2, Z, full=True)
    b = ctx.logpdf_multi(Xs, terms, 0.2, Z, full=True)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    So = np.full((6, 4), -7.5, order="F")
    keep, headn = raw_head(ctx, X0, terms, 0.1, y0, Xs, 0.2)
    assert ctx.lib.gaplac_posterior_mean_cov(*headn, None, P(So), 6) == 0
    assert np.array_equal(So[:4], S) and np.all(So[4:] == -7.5)


def test_argument_errors(ctx):
    terms = [(SQEXP, 0, 1.0, 0)]
    X = np.arange(6.0)[:, None]
    y = np.ones(6)
    Xs = np.linspace(0, 1, 4)[:, None]
    with pytest.raises(ArgumentError):
        ctx.posterior_mean_cov(X, terms, 0.1, y[:-1], Xs)
    with pytest.raises(ArgumentError):
        ctx.posterior_mean_cov(X, terms, 0.1, y, np.zeros((4, 2)))
    with pytest.raises(ArgumentError):
        ctx.posterior_rand(X, terms, 0.1, y, Xs, 0.1, np.zeros((5, 2)))
    with pytest.raises(ArgumentError):
        ctx.posterior_rand(X, terms, 0.1, y, Xs, 0.1, np.zeros(4))
    with pytest.raises(ArgumentError):
        ctx.posterior_logpdf(X, terms, 0.1, y, Xs, 0.1, np.zeros((3, 2)))
    with pytest.raises(ArgumentError):
        ctx.posterior_logpdf(X, terms, 0.1, y, Xs, 0.1, np.zeros(4))
    mc, rd, lg = ctx.lib.gaplac_posterior_mean_cov, ctx.lib.gaplac_posterior_rand, ctx.lib.gaplac_posterior_logpdf
    A = np.zeros((4, 4), order="F")
    B = np.zeros((4, 2), order="F")
    o = np.zeros((4, 2), order="F")
    v = np.zeros(4)
    ld = c_double()
    bad = []
    for ns in (-0.1, float("nan"), float("inf")):
        keep, h = raw_head(ctx, X, terms, 0.1, y, Xs, ns)
        bad += [mc(*h, P(v), P(A), 4), rd(*h, 2, P(B), 4, P(o), 4), lg(*h, 2, P(B), 4, P(v), byref(ld), None)]
    keep, h = raw_head(ctx, X, terms, 0.1, y, Xs, 0.1)
    hneg = h[:9] + (-1,) + h[10:]           # M < 0
    hnull = h[:10] + (None,) + h[11:]       # Xs NULL
    hld = h[:11] + (3,) + h[12:]            # ldxs < M
    for hh in (hneg, hnull, hld):
        bad += [mc(*hh, P(v), P(A), 4), rd(*hh, 2, P(B), 4, P(o), 4), lg(*hh, 2, P(B), 4, P(v), byref(ld), None)]
    bad += [mc(*h, P(v), P(A), 3),                                            # ldc < M
            rd(*h, -1, P(B), 4, P(o), 4), rd(*h, 2, None, 4, P(o), 4),        # R < 0, Z NULL
            rd(*h, 2, P(B), 3, P(o), 4), rd(*h, 2, P(B), 4, P(o), 3),         # ldz < M, ldo < M
            rd(*h, 2, P(B), 4, None, 4),                                      # out NULL
            lg(*h, -1, P(B), 4, P(v), byref(ld), None), lg(*h, 2, None, 4, P(v), byref(ld), None),
            lg(*h, 2, P(B), 3, P(v), byref(ld), None), lg(*h, 2, P(B), 4, None, byref(ld), None)]
    for rc in bad:
        assert rc == -1, bad
        with pytest.raises(ArgumentError):
            ctx._check(rc)
    # the context stays usable
    assert np.all(np.isfinite(ctx.posterior_mean_cov(X, terms, 0.1, y, Xs, 0.1)[1]))


def test_nonpd_training_matrix(ctx):
    X = np.repeat(np.arange(8.0), 4)[:, None]
    terms = [(CAT, 0, 0.0, 0)]
    y = np.ones(32)
    Xs = X[:3]
    with pytest.raises(PosDefException):
        ctx.posterior_mean_cov(X, terms, 0.0, y, Xs, 0.1)
    with pytest.raises(PosDefException):
        ctx.posterior_rand(X, terms, 0.0, y, Xs, 0.1, np.ones((3, 2)))
    with pytest.raises(PosDefException):
        ctx.posterior_logpdf(X, terms, 0.0, y, Xs, 0.1, np.ones((3, 2)))
    assert b"training covariance" in ctx.lib.gaplac_last_error(ctx.h)
    keep, h = raw_head(ctx, X, terms, 0.0, y, Xs, 0.1)
    m, S = np.zeros(3), np.zeros((3, 3), order="F")
    rc = ctx.lib.gaplac_posterior_mean_cov(*h, P(m), P(S), 3)
    assert rc > 0 and np.all(np.isnan(m)) and np.all(np.isnan(S))
    B, o = np.ones((3, 2), order="F"), np.zeros((3, 2), order="F")
    assert ctx.lib.gaplac_posterior_rand(*h, 2, P(B), 3, P(o), 3) == rc and np.all(np.isnan(o))
    lp, q, ld = np.zeros(2), np.zeros(2), c_double(0.0)
    assert ctx.lib.gaplac_posterior_logpdf(*h, 2, P(B), 3, P(lp), byref(ld), P(q)) == rc
    assert np.all(np.isnan(lp)) and np.all(np.isnan(q)) and np.isnan(ld.value)
    # the context stays usable
    c = case(5, 3)
    m, S = ctx.posterior_mean_cov(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1)
    check_cov(S, c.cov, c.kd)


def test_nonpd_test_point_covariance(ctx):
    # a repeated test point with noise_s = 0 makes Sigma* singular: its second leading minor
    # has a pivot that is zero up to rounding. With a CAT kernel and test points away from every
    # training level Sigma* is exactly [[1, 1], [1, 1]] and the second pivot exactly 0.
    X = np.repeat(np.arange(8.0), 4)[:, None]
    terms = [(CAT, 0, 0.0, 0)]
    y = np.ones(32)
    Xs = np.array([[100.0], [100.0]])
    m, S = ctx.posterior_mean_cov(X, terms, 0.1, y, Xs, 0.0)   # no second factorisation: returned as it is
    assert np.array_equal(S, np.ones((2, 2))) and np.all(m == 0.0)
    keep, h = raw_head(ctx, X, terms, 0.1, y, Xs, 0.0)
    B, o = np.ones((2, 2), order="F"), np.zeros((2, 2), order="F")
    assert ctx.lib.gaplac_posterior_rand(*h, 2, P(B), 2, P(o), 2) == 2 and np.all(np.isnan(o))
    assert b"test-point covariance" in ctx.lib.gaplac_last_error(ctx.h)
    lp, ld = np.zeros(2), c_double(0.0)
    assert ctx.lib.gaplac_posterior_logpdf(*h, 2, P(B), 2, P(lp), byref(ld), None) == 2
    assert np.all(np.isnan(lp)) and np.isnan(ld.value)
    assert ctx.posterior_rand(X, terms, 0.1, y, Xs, 0.1, np.ones((2, 2))).shape == (2, 2)


def test_consistent_with_posterior_mean_var(ctx):
    for N, M in ((127, 129), (700, 257), (300, 1000)):
        c = case(N, M)
        m0, v0 = ctx.posterior_mean_var(c.X, COMPOSITE, 0.1, c.y, c.Xs)
        m, S = ctx.posterior_mean_cov(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1)
        print((N, M), "mean bitwise:", bool(np.array_equal(m, m0)), "max |diag - var|", np.max(np.abs(np.diag(S) - 0.1 - v0)))
        assert np.max(np.abs(m - m0)) <= 1e-13
        assert np.all(np.abs(np.diag(S) - 0.1 - v0) <= 1e-12 * np.maximum(1.0, c.kd))


def test_permutations(ctx):
    c = case(300, 1000)
    rng = np.random.default_rng(9)
    perm = rng.permutation(c.M)
    m, S = ctx.posterior_mean_cov(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1)
    mp, Sp = ctx.posterior_mean_cov(c.X, COMPOSITE, 0.1, c.y, c.Xs[perm], 0.1)
    print("permuted covariance bitwise:", bool(np.array_equal(S[np.ix_(perm, perm)], Sp)),
          "mean bitwise:", bool(np.array_equal(m[perm], mp)))
    assert np.max(np.abs(S[np.ix_(perm, perm)] - Sp)) <= 1e-13
    assert np.max(np.abs(m[perm] - mp)) <= 1e-13
    D = ctx.posterior_rand(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1, c.Z)
    cp = rng.permutation(5)
    Dc = ctx.posterior_rand(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1, c.Z[:, cp])
    print("permuted columns bitwise:", bool(np.array_equal(D[:, cp], Dc)))
    assert np.max(np.abs(D[:, cp] - Dc)) <= 1e-13 * max(1.0, np.max(np.abs(D)))
    one = ctx.posterior_rand(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1, c.Z[:, 3:4])
    print("a column alone bitwise:", bool(np.array_equal(one[:, 0], D[:, 3])))
    assert np.max(np.abs(one[:, 0] - D[:, 3])) <= 1e-13 * max(1.0, np.max(np.abs(D)))
    # Rows: the Cholesky factor of P Sigma* P^T is not P L*, so for the same Z the draws at
    # permuted test points are not the permuted draws; they are draws of the same Gaussian from
    # another square root. Put back in the original order they must therefore have the quad
    # |L*^{-1}(d - m)|^2 = |Z_r|^2 under the un-permuted call (1e-9 relative).
    Dp = ctx.posterior_rand(c.X, COMPOSITE, 0.1, c.y, c.Xs[perm], 0.1, c.Z)
    lp = ctx.posterior_logpdf(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1, Dp[np.argsort(perm)], full=True)
    zz = (c.Z * c.Z).sum(0)
    print("permuted rows: quad of the un-permuted draws rel", np.max(np.abs(lp[2] - zz) / zz))
    assert np.all(np.abs(lp[2] - zz) <= TOL * zz)


def test_superpanel_path_agrees_with_the_tail(monkeypatch):
    if not gpu_available():
        pytest.skip("no GPU")
    c = case(700, 257)
    with Context(0) as cx:
        a = (cx.posterior_mean_cov(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1)[1],
             cx.posterior_rand(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1, c.Z),
             cx.posterior_logpdf(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1, c.Ys))
    monkeypatch.setenv("GAPLAC_TAILK", "0")
    with Context(0) as cx:
        b = (cx.posterior_mean_cov(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1)[1],
             cx.posterior_rand(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1, c.Z),
             cx.posterior_logpdf(c.X, COMPOSITE, 0.1, c.y, c.Xs, 0.1, c.Ys))
    for u, v in zip(a, b):
        print("tail vs super-panels", np.max(np.abs(u - v)) / max(1.0, np.max(np.abs(v))))
        assert np.max(np.abs(u - v)) <= 1e-11 * max(1.0, np.max(np.abs(v)))


def big_inputs(N, M, seed):
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(0, 10, N), rng.integers(0, max(N // 3, 1), N).astype(float)])
    Xs = np.column_stack([rng.uniform(0, 10, M), rng.integers(0, max(N // 3, 1), M).astype(float)])
    terms = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2)]
    return X, Xs, rng.normal(size=N), terms, rng


def round_trip(ctx, X, terms, y, Xs, Z):
    D = ctx.posterior_rand(X, terms, 0.1, y, Xs, 0.1, Z)
    lp, ld, q = ctx.posterior_logpdf(X, terms, 0.1, y, Xs, 0.1, D, full=True)
    zz = (Z * Z).sum(0)
    print("round trip max rel", np.max(np.abs(q - zz) / zz))
    assert np.all(np.abs(q - zz) <= TOL * zz)
    _, ld1, _ = ctx.posterior_logpdf(X, terms, 0.1, y, Xs, 0.1, D[:, :1], full=True)
    print("logdet from both shapes of call:", ld, ld1)
    assert abs(ld - ld1) <= TOL * abs(ld)
    return D


def test_superpanel_phase_in_the_first_factorisation(ctx):
    # N = 10300 (81 tile columns): one super-panel, then the tail carrying the 3 tile rows
    X, Xs, y, terms, rng = big_inputs(10300, 300, 10300)
    round_trip(ctx, X, terms, y, Xs, rng.normal(size=(300, 2)))
    m0, v0 = ctx.posterior_mean_var(X, terms, 0.1, y, Xs)
    m, S = ctx.posterior_mean_cov(X, terms, 0.1, y, Xs, 0.1)
    assert np.max(np.abs(m - m0)) <= 1e-13 and np.array_equal(S, S.T)
    assert np.all(np.abs(np.diag(S) - 0.1 - v0) <= 1e-12 * np.maximum(1.0, R.kernel_diag(Xs, terms)))


def test_superpanel_phase_in_the_second_factorisation(ctx):
    # M = 10300: the factorisation of Sigma* has a super-panel phase, then the tail (with the
    # riding rows in posterior_logpdf)
    X, Xs, y, terms, rng = big_inputs(300, 10300, 300)
    round_trip(ctx, X, terms, y, Xs, rng.normal(size=(10300, 2)))


def test_large_n_agrees_with_posterior_mean_var(ctx):
    X, _, y, terms, rng = big_inputs(16384, 1, 2)
    idx = rng.choice(16384, 600, replace=False)
    m0, v0 = ctx.posterior_mean_var(X, terms, 0.1, y, X[idx])
    m, S = ctx.posterior_mean_cov(X, terms, 0.1, y, X[idx], 0.1)
    print("mean bitwise:", bool(np.array_equal(m, m0)), "max |diag - var|", np.max(np.abs(np.diag(S) - 0.1 - v0)))
    assert np.max(np.abs(m - m0)) <= 1e-13
    assert np.all(np.abs(np.diag(S) - 0.1 - v0) <= 1e-12 * np.maximum(1.0, R.kernel_diag(X[idx], terms)))
    assert np.array_equal(S, S.T)
