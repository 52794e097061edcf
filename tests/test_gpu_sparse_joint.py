"""Parity of the joint forms of the inducing-point posterior, gaplac_sparse_posterior_mean_cov /
_rand / _logpdf (HIP, through the C-ABI), against the CPU recipe of tests/sparse_joint_oracle.py
(its two routes pinned to each other by tests/test_sparse_joint_oracle.py): the dense N x N route
up to N = 2000, the Woodbury route above; and against gaplac_sparse_posterior_mean_var.

Bars (the project's north-star 1e-9, as tests/test_gpu_joint.py): mean within 1e-9 max(1, max
|mean|); every entry of Sigma* within 1e-9 max(1, max kernel_diag(Xs)) and exactly symmetric;
draws within 1e-9 max(1, max |draw|); logpdf 1e-9 relative, logdet and quad within 1e-9 of
|logpdf|. The two CPU routes differ by at most 3.0e-15, 2.8e-12, 1.9e-12 and 3.7e-14 of those
scales on these inputs. Each test prints its observed maxima before it asserts.
"""
from ctypes import byref, c_double, c_void_p

import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd import formula as F
from gaplac_amd._native import CAT, LINEAR, NOISE, OU, SQEXP, term_array
from gaplac_amd.backend import ArgumentError, Context, PosDefException
from oracle import restatement as R
from tests import joint_oracle as J
from tests import sparse_joint_oracle as SJ
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
TOL = 1e-9
COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (LINEAR, 2, 0.5, 3)]
SIZES = [(300, 1, 1), (300, 5, 3), (700, 127, 129), (1000, 129, 128), (513, 128, 127), (129, 129, 130),
         (2000, 257, 257), (600, 64, 513), (400, 300, 1000)]
_cases = {}


def case(N, Mz, Ms, jitter=1e-6):
    key = (N, Mz, Ms, jitter)
    if key not in _cases:
        _cases[key] = SJ.Case(N, Mz, Ms, COMPOSITE, 0.1, jitter, 0.1)
    return _cases[key]


@pytest.fixture(scope="module")
def ctx():
    if not gpu_available():
        pytest.skip("no GPU")
    c = Context(0)
    yield c
    c.close()


def args(c):
    return c.X, c.terms, c.noise, c.y, c.Z, c.jitter, c.Xs


def check_mean(m, ref):
    print("max |mean - oracle|", np.max(np.abs(m - ref)), "bar", TOL * max(1.0, np.max(np.abs(ref))))
    assert np.max(np.abs(m - ref)) <= TOL * max(1.0, np.max(np.abs(ref)))


def check_cov(S, ref, kd):
    bar = TOL * max(1.0, np.max(kd))
    print("max |cov - oracle|", np.max(np.abs(S - ref)), "bar", bar)
    assert np.max(np.abs(S - ref)) <= bar
    assert np.array_equal(S, S.T)


def check_draws(D, ref):
    bar = TOL * max(1.0, np.max(np.abs(ref)))
    print("max |draw - oracle|", np.max(np.abs(D - ref)), "bar", bar)
    assert D.shape == ref.shape and np.max(np.abs(D - ref)) <= bar


def check_logpdf(got, ref):
    (lp, ld, q), (rl, rd, rq) = got, ref
    print("max rel logpdf", np.max(np.abs(lp - rl) / np.abs(rl)), "logdet", abs(ld - rd), "quad", np.max(np.abs(q - rq)))
    assert np.all(np.abs(lp - rl) <= TOL * np.abs(rl))
    assert abs(ld - rd) <= TOL * np.min(np.abs(rl))
    assert np.all(np.abs(q - rq) <= TOL * np.abs(rl))


def check_case(ctx, c):
    for noise_s, ref in ((0.0, c.cov0), (0.1, c.cov)):
        m, S = ctx.sparse_posterior_mean_cov(*args(c), noise_s)
        assert m.shape == (c.Ms,) and S.shape == (c.Ms, c.Ms)
        check_mean(m, c.mean)
        check_cov(S, ref, c.kd)
    check_draws(ctx.sparse_posterior_rand(*args(c), 0.1, c.E), c.draws)
    got = ctx.sparse_posterior_logpdf(*args(c), 0.1, c.Ys, full=True)
    assert got[0].shape == (5,) and got[2].shape == (5,)
    check_logpdf(got, c.lp)


@pytest.mark.parametrize("jitter", [1e-6, 1e-2])
@pytest.mark.parametrize("N,Mz,Ms", SIZES)
def test_sizes_composite(ctx, N, Mz, Ms, jitter):
    check_case(ctx, case(N, Mz, Ms, jitter))


def test_three_chunks_woodbury_reference(ctx):
    c = case(2051, 129, 130)
    assert ctx.sparse_split(2051, 129) == (3, 1024)
    check_case(ctx, c)


def test_consistent_with_sparse_posterior_mean_var(ctx):
    for N, Mz, Ms in ((700, 127, 129), (513, 128, 127), (400, 300, 1000), (2051, 129, 130)):
        c = case(N, Mz, Ms)
        m0, v0 = ctx.sparse_posterior_mean_var(*args(c))
        m, S = ctx.sparse_posterior_mean_cov(*args(c), 0.1)
        print((N, Mz, Ms), "mean bitwise:", bool(np.array_equal(m, m0)), "max |mean - mean_var's|",
              np.max(np.abs(m - m0)), "max |diag - noise_s - var| / max(1, kdiag)",
              np.max(np.abs(np.diag(S) - 0.1 - v0) / np.maximum(1.0, c.kd)))
        assert np.max(np.abs(m - m0)) <= 1e-13 * max(1.0, np.max(np.abs(m0)))
        assert np.all(np.abs(np.diag(S) - 0.1 - v0) <= 1e-12 * np.maximum(1.0, c.kd))


def test_repeatable_bitwise(ctx):
    c, o = case(2051, 129, 130), case(300, 5, 3)
    a = (ctx.sparse_posterior_mean_cov(*args(c), 0.1), ctx.sparse_posterior_rand(*args(c), 0.1, c.E),
         ctx.sparse_posterior_logpdf(*args(c), 0.1, c.Ys, full=True))
    ctx.sparse_posterior_logpdf(*args(o), 0.1, o.Ys)                        # (other entries, another shape, between)
    b0 = ctx.sparse_posterior_mean_cov(*args(c), 0.1)
    ctx.sparse_posterior_mean_var(*args(o))
    b1 = ctx.sparse_posterior_rand(*args(c), 0.1, c.E)
    ctx.sparse_posterior_mean_cov(*args(o), 0.0)
    b2 = ctx.sparse_posterior_logpdf(*args(c), 0.1, c.Ys, full=True)
    assert np.array_equal(a[0][0], b0[0]) and np.array_equal(a[0][1], b0[1])
    assert np.array_equal(a[1], b1)
    assert np.array_equal(a[2][0], b2[0]) and a[2][1] == b2[1] and np.array_equal(a[2][2], b2[2])


def test_permutations(ctx):
    c = case(400, 300, 1000)
    rng = np.random.default_rng(9)
    perm = rng.permutation(c.Ms)
    head = args(c)[:-1]
    m, S = ctx.sparse_posterior_mean_cov(*head, c.Xs, 0.1)
    mp, Sp = ctx.sparse_posterior_mean_cov(*head, c.Xs[perm], 0.1)
    print("permuted covariance bitwise:", bool(np.array_equal(S[np.ix_(perm, perm)], Sp)),
          "mean bitwise:", bool(np.array_equal(m[perm], mp)), "max diff", np.max(np.abs(S[np.ix_(perm, perm)] - Sp)),
          np.max(np.abs(m[perm] - mp)))
    assert np.max(np.abs(S[np.ix_(perm, perm)] - Sp)) <= 1e-13
    assert np.max(np.abs(m[perm] - mp)) <= 1e-13
    D = ctx.sparse_posterior_rand(*head, c.Xs, 0.1, c.E)
    cp = rng.permutation(5)
    Dc = ctx.sparse_posterior_rand(*head, c.Xs, 0.1, c.E[:, cp])
    print("permuted columns bitwise:", bool(np.array_equal(D[:, cp], Dc)))
    assert np.max(np.abs(D[:, cp] - Dc)) <= 1e-13 * max(1.0, np.max(np.abs(D)))
    one = ctx.sparse_posterior_rand(*head, c.Xs, 0.1, c.E[:, 3:4])
    print("a column alone bitwise:", bool(np.array_equal(one[:, 0], D[:, 3])))
    assert np.max(np.abs(one[:, 0] - D[:, 3])) <= 1e-13 * max(1.0, np.max(np.abs(D)))
    # Rows: the Cholesky factor of P Sigma* P^T is not P L*, so the draws at permuted test points
    # are draws of the same Gaussian from another square root: put back in the original order
    # they have the quad |L*^{-1}(d - m)|^2 = |E_r|^2 under the un-permuted call.
    Dp = ctx.sparse_posterior_rand(*head, c.Xs[perm], 0.1, c.E)
    lp = ctx.sparse_posterior_logpdf(*head, c.Xs, 0.1, Dp[np.argsort(perm)], full=True)
    zz = (c.E * c.E).sum(0)
    print("permuted rows: quad of the un-permuted draws rel", np.max(np.abs(lp[2] - zz) / zz))
    assert np.all(np.abs(lp[2] - zz) <= TOL * zz)


def test_product_groups_and_noise_term(ctx):
    rng = np.random.default_rng(12)
    N, Mz, Ms = 260, 70, 190
    X = np.column_stack([rng.uniform(0, 5, N), rng.normal(size=N)])
    Z = np.column_stack([rng.uniform(0, 5, Mz), rng.normal(size=Mz)])
    Xs = np.column_stack([rng.uniform(0, 5, Ms), rng.normal(size=Ms)])
    terms = [(SQEXP, 0, 1.3, 0), (LINEAR, 1, 0.4, 0), (OU, 0, 2.5, 1), (NOISE, -1, 0.2, 2)]
    y = rng.normal(size=N)
    E = rng.normal(size=(Ms, 3))
    kd = R.kernel_diag(Xs, terms)
    for noise_s in (0.0, 0.1):
        rm, rS = SJ.dense(X, terms, 0.1, y, Z, 1e-6, Xs, noise_s)
        m, S = ctx.sparse_posterior_mean_cov(X, terms, 0.1, y, Z, 1e-6, Xs, noise_s)
        check_mean(m, rm)
        check_cov(S, rS, kd)
    ref = J.draws(rm, rS, E)
    check_draws(ctx.sparse_posterior_rand(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1, E), ref)
    Ys = ref + 0.3 * rng.normal(size=(Ms, 3))
    check_logpdf(ctx.sparse_posterior_logpdf(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1, Ys, full=True), J.logpdf(rm, rS, Ys))


def raw_head(ctx, X, terms, noise, y, Z, jitter, Xs, noise_s):
    Xc, Zc, Xsc = (np.asfortranarray(a, dtype=np.float64) for a in (X, Z, Xs))
    yc = np.ascontiguousarray(y, dtype=np.float64)
    (N, D), Mz, Ms = Xc.shape, Zc.shape[0], Xsc.shape[0]
    keep = (Xc, Zc, Xsc, yc)
    return keep, (ctx.h, N, D, P(Xc), max(N, 1), len(terms), term_array(terms), float(noise), P(yc), Mz, P(Zc),
                  max(Mz, 1), float(jitter), Ms, P(Xsc), max(Ms, 1), float(noise_s))


def P(a):
    return a.ctypes.data_as(c_void_p)


def test_leading_dimensions_and_padding_rows(ctx):
    c = case(700, 127, 129)
    Ms, Rn = 129, 5
    keep, head = raw_head(ctx, *args(c), 0.1)
    m, S = ctx.sparse_posterior_mean_cov(*args(c), 0.1)
    mo = np.empty(Ms)
    So = np.full((Ms + 3, Ms), -7.5, order="F")
    assert ctx.lib.gaplac_sparse_posterior_mean_cov(*head, P(mo), P(So), Ms + 3) == 0
    assert np.array_equal(mo, m) and np.array_equal(So[:Ms], S) and np.all(So[Ms:] == -7.5)
    # either output may be NULL
    mo2 = np.empty(Ms)
    assert ctx.lib.gaplac_sparse_posterior_mean_cov(*head, P(mo2), None, 0) == 0 and np.array_equal(mo2, m)
    So2 = np.empty((Ms, Ms), order="F")
    assert ctx.lib.gaplac_sparse_posterior_mean_cov(*head, None, P(So2), Ms) == 0 and np.array_equal(So2, S)
    # larger leading dimensions of X, Z and Xs, NaN in the rows beyond
    Xp, Zp, Xsp = (np.full((a.shape[0] + 3, 3), np.nan, order="F") for a in (c.X, c.Z, c.Xs))
    Xp[:700], Zp[:127], Xsp[:129] = c.X, c.Z, c.Xs
    hp = head[:3] + (P(Xp), 703) + head[5:10] + (P(Zp), 130) + head[12:14] + (P(Xsp), 132) + head[16:]
    So3 = np.empty((Ms, Ms), order="F")
    assert ctx.lib.gaplac_sparse_posterior_mean_cov(*hp, P(mo2), P(So3), Ms) == 0
    assert np.array_equal(mo2, m) and np.array_equal(So3, S)
    D = ctx.sparse_posterior_rand(*args(c), 0.1, c.E)
    Ep = np.full((Ms + 5, Rn), np.nan, order="F")
    Ep[:Ms] = c.E
    out = np.full((Ms + 7, Rn), -7.5, order="F")
    assert ctx.lib.gaplac_sparse_posterior_rand(*head, Rn, P(Ep), Ms + 5, P(out), Ms + 7) == 0
    assert np.array_equal(out[:Ms], D) and np.all(out[Ms:] == -7.5)
    ref = ctx.sparse_posterior_logpdf(*args(c), 0.1, c.Ys, full=True)
    Yp = np.full((Ms + 2, Rn), np.nan, order="F")
    Yp[:Ms] = c.Ys
    lp, q, ld = np.empty(Rn), np.empty(Rn), c_double()
    assert ctx.lib.gaplac_sparse_posterior_logpdf(*head, Rn, P(Yp), Ms + 2, P(lp), byref(ld), P(q)) == 0
    assert np.array_equal(lp, ref[0]) and ld.value == ref[1] and np.array_equal(q, ref[2])
    lp2 = np.empty(Rn)
    assert ctx.lib.gaplac_sparse_posterior_logpdf(*head, Rn, P(Yp), Ms + 2, P(lp2), None, None) == 0
    assert np.array_equal(lp2, ref[0])


def test_empty_sets_follow_the_header(ctx):
    terms = [(SQEXP, 0, 1.0, 0), (LINEAR, 0, 0.5, 1)]
    X = np.arange(6.0)[:, None]
    y = np.ones(6)
    Z = np.array([[0.5], [2.5], [4.5]])
    Xs = np.linspace(0, 1, 4)[:, None]
    e0 = np.zeros((0, 1))
    can, ldv = np.full(3, -7.5), c_double(-7.5)
    # Ms = 0
    m, S = ctx.sparse_posterior_mean_cov(X, terms, 0.1, y, Z, 1e-6, e0, 0.1)
    assert m.shape == (0,) and S.shape == (0, 0)
    assert ctx.sparse_posterior_rand(X, terms, 0.1, y, Z, 1e-6, e0, 0.1, np.zeros((0, 3))).shape == (0, 3)
    keep, head0 = raw_head(ctx, X, terms, 0.1, y, Z, 1e-6, e0, 0.1)
    assert ctx.lib.gaplac_sparse_posterior_logpdf(*head0, 3, None, 0, P(can), byref(ldv), P(can)) == 0
    assert np.all(can == -7.5) and ldv.value == -7.5
    out = np.full((2, 3), -7.5, order="F")
    assert ctx.lib.gaplac_sparse_posterior_rand(*head0, 3, None, 0, P(out), 2) == 0 and np.all(out == -7.5)
    assert ctx.lib.gaplac_sparse_posterior_mean_cov(*head0, P(can), P(out), 2) == 0
    assert np.all(can == -7.5) and np.all(out == -7.5)
    # R = 0
    assert ctx.sparse_posterior_rand(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1, np.zeros((4, 0))).shape == (4, 0)
    lp, ld, q = ctx.sparse_posterior_logpdf(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1, np.zeros((4, 0)), full=True)
    assert lp.shape == (0,) and q.shape == (0,)
    keep, head = raw_head(ctx, X, terms, 0.1, y, Z, 1e-6, Xs, 0.1)
    assert ctx.lib.gaplac_sparse_posterior_logpdf(*head, 0, None, 4, P(can), byref(ldv), P(can)) == 0
    assert np.all(can == -7.5) and ldv.value == -7.5
    out = np.full((6, 3), -7.5, order="F")
    assert ctx.lib.gaplac_sparse_posterior_rand(*head, 0, None, 4, P(out), 6) == 0 and np.all(out == -7.5)
    # bad terms are reported before the empty return
    with pytest.raises(ArgumentError):
        ctx.sparse_posterior_rand(X, [(SQEXP, 0, -1.0, 0)], 0.1, y, Z, 1e-6, Xs, 0.1, np.zeros((4, 0)))
    # N = 0, and Mz = 0: the prior at the test points
    E = np.random.default_rng(3).normal(size=(4, 3))
    for Xn, yn, Zn in ((e0, np.zeros(0), Z), (X, y, e0)):
        m, S = ctx.sparse_posterior_mean_cov(Xn, terms, 0.1, yn, Zn, 1e-6, Xs, 0.2)
        assert np.all(m == 0.0) and np.array_equal(S, ctx.gram(Xs, terms, 0.2))
        assert np.max(np.abs(S - R.gram(Xs, terms, 0.2))) <= 1e-12
        assert np.array_equal(ctx.sparse_posterior_rand(Xn, terms, 0.1, yn, Zn, 1e-6, Xs, 0.2, E),
                              ctx.rand_multi(Xs, terms, 0.2, E))
        a = ctx.sparse_posterior_logpdf(Xn, terms, 0.1, yn, Zn, 1e-6, Xs, 0.2, E, full=True)
        b = ctx.logpdf_multi(Xs, terms, 0.2, E, full=True)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
        So = np.full((6, 4), -7.5, order="F")
        keep, headn = raw_head(ctx, Xn, terms, 0.1, yn, Zn, 1e-6, Xs, 0.2)
        assert ctx.lib.gaplac_sparse_posterior_mean_cov(*headn, None, P(So), 6) == 0
        assert np.array_equal(So[:4], S) and np.all(So[4:] == -7.5)


def test_argument_errors(ctx):
    terms = [(SQEXP, 0, 1.0, 0)]
    X = np.arange(6.0)[:, None]
    y = np.ones(6)
    Z = np.array([[0.5], [2.5], [4.5]])
    Xs = np.linspace(0, 1, 4)[:, None]
    with pytest.raises(ArgumentError):
        ctx.sparse_posterior_mean_cov(X, terms, 0.1, y[:-1], Z, 1e-6, Xs)
    with pytest.raises(ArgumentError):
        ctx.sparse_posterior_mean_cov(X, terms, 0.1, y, Z, 1e-6, np.zeros((4, 2)))
    with pytest.raises(ArgumentError):
        ctx.sparse_posterior_mean_cov(X, terms, 0.1, y, np.zeros((3, 2)), 1e-6, Xs)
    with pytest.raises(ArgumentError):
        ctx.sparse_posterior_rand(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1, np.zeros((5, 2)))
    with pytest.raises(ArgumentError):
        ctx.sparse_posterior_rand(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1, np.zeros(4))
    with pytest.raises(ArgumentError):
        ctx.sparse_posterior_logpdf(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1, np.zeros((3, 2)))
    with pytest.raises(ArgumentError):
        ctx.sparse_posterior_logpdf(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1, np.zeros(4))
    mc, rd, lg = (ctx.lib.gaplac_sparse_posterior_mean_cov, ctx.lib.gaplac_sparse_posterior_rand,
                  ctx.lib.gaplac_sparse_posterior_logpdf)
    B = np.ones((4, 2), order="F")

    def all_three(h, code):
        """The three entries with the head h: each returns `code` and leaves its outputs NaN."""
        v, A, o, lp, q, ld = np.zeros(4), np.zeros((4, 4), order="F"), np.zeros((4, 2), order="F"), np.zeros(2), \
            np.zeros(2), c_double(0.0)
        rcs = [mc(*h, P(v), P(A), 4), rd(*h, 2, P(B), 4, P(o), 4), lg(*h, 2, P(B), 4, P(lp), byref(ld), P(q))]
        assert rcs == [code] * 3, (rcs, code, ctx.lib.gaplac_last_error(ctx.h))
        if h[13] > 0:       # (Ms < 0: nothing to fill)
            assert np.all(np.isnan(v)) and np.all(np.isnan(A)) and np.all(np.isnan(o))
            assert np.all(np.isnan(lp)) and np.all(np.isnan(q)) and np.isnan(ld.value)
        with pytest.raises(ArgumentError):
            ctx._check(code)

    def usable():
        rm, rS = SJ.woodbury(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1)
        m, S = ctx.sparse_posterior_mean_cov(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1)
        assert np.max(np.abs(m - rm)) <= TOL * max(1.0, np.max(np.abs(rm))) and np.max(np.abs(S - rS)) <= TOL

    for noise, jitter in ((0.0, 1e-6), (-0.1, 1e-6), (float("nan"), 1e-6), (float("inf"), 1e-6), (0.1, -1e-6),
                          (0.1, float("nan"))):
        keep, h = raw_head(ctx, X, terms, noise, y, Z, jitter, Xs, 0.1)
        all_three(h, _native.E_PARAM)
        usable()
    for ns in (-0.1, float("nan"), float("inf")):
        keep, h = raw_head(ctx, X, terms, 0.1, y, Z, 1e-6, Xs, ns)
        all_three(h, _native.E_ARG)
        usable()
    keep, h = raw_head(ctx, X, terms, 0.1, y, Z, 1e-6, Xs, 0.1)
    for hh in (h[:9] + (-1,) + h[10:],          # Mz < 0
               h[:10] + (None,) + h[11:],       # Z NULL
               h[:11] + (2,) + h[12:],          # ldz < Mz
               h[:13] + (-1,) + h[14:],         # Ms < 0
               h[:14] + (None,) + h[15:],       # Xs NULL
               h[:15] + (3,) + h[16:],          # ldxs < Ms
               h[:3] + (None,) + h[4:],         # X NULL
               h[:4] + (5,) + h[5:],            # ldx < N
               h[:1] + (-1,) + h[2:]):          # N < 0
        all_three(hh, _native.E_ARG)
        usable()
    v, A, o, ld = np.zeros(4), np.zeros((4, 4), order="F"), np.zeros((4, 2), order="F"), c_double()
    bad = [mc(*h, P(v), P(A), 3),                                             # ldc < Ms
           rd(*h, -1, P(B), 4, P(o), 4), rd(*h, 2, None, 4, P(o), 4),         # R < 0, E NULL
           rd(*h, 2, P(B), 3, P(o), 4), rd(*h, 2, P(B), 4, P(o), 3),          # lde < Ms, ldo < Ms
           rd(*h, 2, P(B), 4, None, 4),                                       # out NULL
           lg(*h, -1, P(B), 4, P(v), byref(ld), None), lg(*h, 2, None, 4, P(v), byref(ld), None),
           lg(*h, 2, P(B), 3, P(v), byref(ld), None), lg(*h, 2, P(B), 4, None, byref(ld), None)]
    assert bad == [_native.E_ARG] * len(bad), bad
    usable()


def test_sizes_past_the_grids_are_refused(ctx):
    terms = [(SQEXP, 0, 1.0, 0)]
    Z = np.array([[0.5], [2.5], [4.5]])
    Xs = np.linspace(0, 1, 4)[:, None]
    big = np.zeros((65535 * 128 - 3, 1))                    # N + Ms: one tile row past the cross-covariance grid
    keep, h = raw_head(ctx, big, terms, 0.1, big[:, 0], Z, 1e-6, Xs, 0.1)
    v, A = np.zeros(4), np.zeros((4, 4), order="F")
    assert ctx.lib.gaplac_sparse_posterior_mean_cov(*h, P(v), P(A), 4) == _native.E_OOM
    assert np.all(np.isnan(v)) and np.all(np.isnan(A))
    X = np.arange(6.0)[:, None]
    Rb = 65535 * 128 + 1                                    # R: one tile row past the transposing grid
    keep, h = raw_head(ctx, X, terms, 0.1, np.ones(6), Z, 1e-6, Xs[:1], 0.1)
    Eb, ob = np.zeros((1, Rb), order="F"), np.zeros((1, Rb), order="F")
    assert ctx.lib.gaplac_sparse_posterior_rand(*h, Rb, P(Eb), 1, P(ob), 1) == _native.E_OOM
    assert np.all(np.isnan(ob))
    assert ctx.lib.gaplac_sparse_posterior_logpdf(*h, Rb, P(Eb), 1, P(ob), None, None) == _native.E_OOM
    assert np.all(np.isnan(ob))
    with pytest.raises(Exception) as e:
        ctx._check(_native.E_OOM)
    assert not isinstance(e.value, (ArgumentError, PosDefException))
    m, S = ctx.sparse_posterior_mean_cov(X, terms, 0.1, np.ones(6), Z, 1e-6, Xs, 0.1)     # still usable
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(S))


def test_nonpd_inducing_covariance(ctx):
    X = np.repeat(np.arange(8.0), 4)[:, None]
    terms = [(CAT, 0, 0.0, 0)]
    y = np.ones(32)
    Zd = np.array([[0.0], [1.0], [2.0], [1.0], [3.0]])      # a repeated level, jitter 0: the fourth pivot is exactly 0
    Xs = X[:3]
    with pytest.raises(PosDefException) as e:
        ctx.sparse_posterior_mean_cov(X, terms, 0.1, y, Zd, 0.0, Xs, 0.1)
    assert e.value.info == 4
    with pytest.raises(PosDefException):
        ctx.sparse_posterior_rand(X, terms, 0.1, y, Zd, 0.0, Xs, 0.1, np.ones((3, 2)))
    with pytest.raises(PosDefException):
        ctx.sparse_posterior_logpdf(X, terms, 0.1, y, Zd, 0.0, Xs, 0.1, np.ones((3, 2)))
    assert b"inducing covariance" in ctx.lib.gaplac_last_error(ctx.h)
    keep, h = raw_head(ctx, X, terms, 0.1, y, Zd, 0.0, Xs, 0.1)
    m, S = np.zeros(3), np.zeros((3, 3), order="F")
    assert ctx.lib.gaplac_sparse_posterior_mean_cov(*h, P(m), P(S), 3) == 4
    assert np.all(np.isnan(m)) and np.all(np.isnan(S))
    B, o = np.ones((3, 2), order="F"), np.zeros((3, 2), order="F")
    assert ctx.lib.gaplac_sparse_posterior_rand(*h, 2, P(B), 3, P(o), 3) == 4 and np.all(np.isnan(o))
    lp, q, ld = np.zeros(2), np.zeros(2), c_double(0.0)
    assert ctx.lib.gaplac_sparse_posterior_logpdf(*h, 2, P(B), 3, P(lp), byref(ld), P(q)) == 4
    assert np.all(np.isnan(lp)) and np.all(np.isnan(q)) and np.isnan(ld.value)
    # the context stays usable: with jitter the same inputs factor
    assert ctx.sparse_posterior_rand(X, terms, 0.1, y, Zd, 1e-6, Xs, 0.1, np.ones((3, 2))).shape == (3, 2)


def test_nonpd_test_point_covariance(ctx):
    # Z = the 8 levels, Xs = two copies of a level absent from Z: A = B = 0 and, at noise_s = 0,
    # Sigma* is exactly [[1, 1], [1, 1]]: the second pivot of the third factorisation is exactly 0.
    X = np.repeat(np.arange(8.0), 4)[:, None]
    terms = [(CAT, 0, 0.0, 0)]
    y = np.ones(32)
    Z = np.arange(8.0)[:, None]
    Xs = np.array([[100.0], [100.0]])
    m, S = ctx.sparse_posterior_mean_cov(X, terms, 0.1, y, Z, 1e-6, Xs, 0.0)      # no third factorisation
    assert np.array_equal(S, np.ones((2, 2))) and np.all(m == 0.0)
    keep, h = raw_head(ctx, X, terms, 0.1, y, Z, 1e-6, Xs, 0.0)
    B, o = np.ones((2, 2), order="F"), np.zeros((2, 2), order="F")
    assert ctx.lib.gaplac_sparse_posterior_rand(*h, 2, P(B), 2, P(o), 2) == 2 and np.all(np.isnan(o))
    assert b"test-point covariance" in ctx.lib.gaplac_last_error(ctx.h)
    lp, q, ld = np.zeros(2), np.zeros(2), c_double(0.0)
    assert ctx.lib.gaplac_sparse_posterior_logpdf(*h, 2, P(B), 2, P(lp), byref(ld), P(q)) == 2
    assert np.all(np.isnan(lp)) and np.all(np.isnan(q)) and np.isnan(ld.value)
    assert b"test-point covariance" in ctx.lib.gaplac_last_error(ctx.h)
    D = ctx.sparse_posterior_rand(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1, np.ones((2, 2)))
    assert D.shape == (2, 2) and np.all(np.isfinite(D))


def test_superpanel_phase_in_the_third_factorisation(ctx):
    # Ms = 10300 (81 tile columns): the factorisation of Sigma* has a super-panel phase, then the
    # tail (with the riding rows in sparse_posterior_logpdf)
    N, Mz, Ms = 300, 129, 10300
    rng = np.random.default_rng(300)
    cols = lambda n: np.column_stack([rng.uniform(0, 10, n), rng.integers(0, max(N // 3, 1), n).astype(float)])
    X, Xs = cols(N), cols(Ms)                               # (tests/test_gpu_joint.py's big_inputs, then Z)
    terms = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2)]
    y = rng.normal(size=N)
    Z = cols(Mz)
    E = rng.normal(size=(Ms, 2))
    D = ctx.sparse_posterior_rand(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1, E)
    lp, ld, q = ctx.sparse_posterior_logpdf(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1, D, full=True)
    zz = (E * E).sum(0)
    print("round trip max rel", np.max(np.abs(q - zz) / zz))
    assert np.all(np.abs(q - zz) <= TOL * zz)
    _, ld1, _ = ctx.sparse_posterior_logpdf(X, terms, 0.1, y, Z, 1e-6, Xs, 0.1, D[:, :1], full=True)
    print("logdet from both shapes of call:", ld, ld1)
    assert abs(ld - ld1) <= TOL * abs(ld)


def test_abstractgps_surface(ctx):
    rng = np.random.default_rng(13)
    N, Mz, Ms = 400, 12, 100
    x = rng.uniform(-5, 5, N)
    y = np.sin(x) + 0.3 * rng.normal(size=N)
    z = np.linspace(-5, 5, Mz)
    xt = np.linspace(x.min() - 1, x.max() + 1, Ms)
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))
    fx = gp(x, 0.1)
    fp = AG.posterior(AG.VFE(gp(z, 1e-6)), fx, y, ctx=ctx)
    fpx = fp(xt, 0.05)
    assert isinstance(fpx, AG.FinitePosteriorGP) and len(fpx) == Ms
    rm, rS = SJ.dense(x, fx.terms, 0.1, y, z, 1e-6, xt, 0.05)
    m, S = AG.mean_and_cov(fpx)
    check_mean(m, rm)
    check_cov(S, rS, np.ones(Ms))
    assert np.array_equal(m, fp.mean(xt))
    assert np.array_equal(AG.cov(fpx), S)
    a = AG.rand(fpx, n=4, rng=np.random.default_rng(1))
    E = np.random.default_rng(1).standard_normal((Ms, 4))
    b = AG.rand(fpx, z=E)
    ref = J.draws(rm, rS, E)
    assert a.shape == (Ms, 4) and np.array_equal(a, b)
    check_draws(a, ref)
    one = AG.rand(fpx, z=E[:, 2])
    assert one.shape == (Ms,) and np.max(np.abs(one - b[:, 2])) <= 1e-13 * max(1.0, np.max(np.abs(one)))
    assert AG.rand(fpx, rng=np.random.default_rng(1)).shape == (Ms,)
    Ys = ref + 0.3 * rng.normal(size=(Ms, 4))
    lp = AG.logpdf(fpx, Ys)
    rl = J.logpdf(rm, rS, Ys)[0]
    print("max rel logpdf", np.max(np.abs(lp - rl) / np.abs(rl)))
    assert lp.shape == (4,) and np.all(np.abs(lp - rl) <= TOL * np.abs(rl))
    s = AG.logpdf(fpx, Ys[:, 1])
    assert np.ndim(s) == 0 and abs(s - rl[1]) <= TOL * abs(rl[1])
    full = AG.logpdf(fpx, Ys[:, 1], full=True)
    assert full[0] == s and np.ndim(full[1]) == 0 and np.ndim(full[2]) == 0
    with pytest.raises(F.ArgumentError):
        AG.logpdf(fpx, Ys[:-1])
    with pytest.raises(F.ArgumentError):
        AG.rand(fpx, z=E[:-1])
    # the exact forms go where they went before
    ex = AG.posterior(fx, y, ctx=ctx)(xt, 0.05)
    assert type(ex) is AG.FinitePosteriorGP
    em, eS = AG.mean_and_cov(ex)
    gm, gS = ctx.posterior_mean_cov(x, fx.terms, 0.1, y, xt, 0.05)
    assert np.array_equal(em, gm) and np.array_equal(eS, gS)
    assert np.array_equal(AG.rand(ex, z=E), ctx.posterior_rand(x, fx.terms, 0.1, y, xt, 0.05, E))
    assert np.array_equal(AG.logpdf(ex, Ys), ctx.posterior_logpdf(x, fx.terms, 0.1, y, xt, 0.05, Ys))
    assert AG.rand(fx, n=2, rng=np.random.default_rng(1), ctx=ctx).shape == (N, 2)
