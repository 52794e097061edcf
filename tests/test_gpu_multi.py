"""Parity of the matrix forms gaplac_logpdf_multi / _device and gaplac_rand_multi (HIP,
through the C-ABI) against the CPU restatement, and against the single-vector entries.

The oracle factors once per case: L = cholesky_lower, W = L \\ Y, quad_r = sum_k W[k,r]^2,
logdet from R.logpdf of column 0 (per-column R.logpdf agrees with that recipe to 2e-16).
Bars: logpdf_r <= 1e-9 relative, logdet and quad as tests/test_gpu_parity.py judges them
(within 1e-9 of |logpdf|); samples within 1e-12 of max |sample| (tests/test_gpu_posterior.py).
"""
import ctypes
from ctypes import byref, c_double, c_void_p

import numpy as np
import pytest
import scipy.linalg

from gaplac_amd import abstractgps as AG
from gaplac_amd import formula as F
from gaplac_amd._native import CAT, LINEAR, OU, SQEXP, term_array
from gaplac_amd.backend import ArgumentError, Context, PosDefException
from oracle import restatement as R
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
RTOL = 1e-9
COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (LINEAR, 2, 0.5, 3)]


@pytest.fixture(scope="module")
def ctx():
    if not gpu_available():
        pytest.skip("no GPU")
    c = Context(0)
    yield c
    c.close()


def cols(rng, n):
    return np.column_stack([rng.uniform(0, 10, n), rng.integers(0, 40, n).astype(float), rng.normal(size=n)])


def oracle_multi(X, terms, noise, Y):
    L = R.cholesky_lower(X, terms, noise)
    W = scipy.linalg.solve_triangular(L, Y, lower=True, check_finite=False)
    quad = (W * W).sum(0)
    logdet = R.logpdf(X, terms, noise, Y[:, 0])[1]
    lp = -((X.shape[0] * R.LOG2PI + logdet) + quad) / 2
    return lp, logdet, quad


def check_against_oracle(lp, ld, q, ref):
    rl, rd, rq = ref
    print("max rel logpdf", np.max(np.abs(lp - rl) / np.abs(rl)), "logdet", abs(ld - rd), "quad", np.max(np.abs(q - rq)))
    assert np.all(np.abs(lp - rl) <= RTOL * np.abs(rl))
    assert abs(ld - rd) <= RTOL * np.min(np.abs(rl))
    assert np.all(np.abs(q - rq) <= RTOL * np.abs(rl))


# (300, 6144) / (300, 6145): 48 tile rows fit beside the persistent tail's 80 columns, 49 do not
@pytest.mark.parametrize("N,Rn", [(1, 1), (5, 3), (127, 129), (128, 128), (129, 1), (300, 1000), (513, 513),
                                  (700, 257), (300, 6144), (300, 6145)])
def test_sizes_composite(ctx, N, Rn):
    rng = np.random.default_rng(N * 7 + Rn)
    X = cols(rng, N)
    Y = rng.normal(size=(N, Rn))
    lp, ld, q = ctx.logpdf_multi(X, COMPOSITE, 0.1, Y, full=True)
    assert lp.shape == (Rn,) and q.shape == (Rn,)
    check_against_oracle(lp, ld, q, oracle_multi(X, COMPOSITE, 0.1, Y))


def test_superpanel_rows_agree_with_the_tail(monkeypatch):
    # (700, 257): by default the whole matrix and its 3 tile rows run in the persistent tail;
    # GAPLAC_TAILK=0 runs every column as a super-panel with the rows on their own streams
    if not gpu_available():
        pytest.skip("no GPU")
    rng = np.random.default_rng(700 * 7 + 257)
    X = cols(rng, 700)
    Y = rng.normal(size=(700, 257))
    with Context(0) as c:
        a = c.logpdf_multi(X, COMPOSITE, 0.1, Y, full=True)
    monkeypatch.setenv("GAPLAC_TAILK", "0")
    with Context(0) as c:
        b = c.logpdf_multi(X, COMPOSITE, 0.1, Y, full=True)
    assert np.max(np.abs(a[0] - b[0]) / np.abs(b[0])) <= 1e-11
    assert abs(a[1] - b[1]) <= 1e-11 * abs(b[1])
    assert np.max(np.abs(a[2] - b[2]) / np.abs(b[2])) <= 1e-11


@pytest.fixture(scope="module")
def big():
    # N = 10300 (81 tile columns): the smallest order with a super-panel phase (one panel)
    # and a tail (80 columns) that carries the rows
    rng = np.random.default_rng(10300)
    N = 10300
    X = np.column_stack([rng.uniform(0, 10, N), rng.integers(0, N // 3, N).astype(float)])
    terms = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2)]
    return X, terms, rng.normal(size=(N, 300))


def test_superpanel_then_tail_matches_single_logpdf(ctx, big):
    X, terms, Y = big
    lp, ld, q = ctx.logpdf_multi(X, terms, 0.1, Y, full=True)
    for r in (0, 150, 299):
        sl, sd, sq = ctx.logpdf(X, terms, 0.1, Y[:, r], full=True)
        print("column", r, "rel", abs(lp[r] - sl) / abs(sl))
        assert abs(lp[r] - sl) <= RTOL * abs(sl)
        assert abs(q[r] - sq) <= RTOL * abs(sl)
        assert abs(ld - sd) <= RTOL * abs(sl)


def test_round_trip_of_samples(ctx, big):
    X, terms, Z = big
    S = ctx.rand_multi(X, terms, 0.1, Z)
    _, _, q = ctx.logpdf_multi(X, terms, 0.1, S, full=True)
    zz = (Z * Z).sum(0)
    print("round trip max rel", np.max(np.abs(q - zz) / zz))
    assert np.all(np.abs(q - zz) <= 1e-9 * zz)


def test_every_column_takes_one_path(ctx):
    rng = np.random.default_rng(77)
    N, Rn = 300, 200
    X = cols(rng, N)
    y = rng.normal(size=N)
    same = ctx.logpdf_multi(X, COMPOSITE, 0.1, np.tile(y[:, None], (1, Rn)), full=True)
    for a in (same[0], same[2]):
        print("identical columns bitwise:", bool(np.all(a == a[0])))
        assert np.max(np.abs(a - a[0])) <= 1e-13 * abs(a[0])
    Y = rng.normal(size=(N, Rn))
    perm = rng.permutation(Rn)
    a = ctx.logpdf_multi(X, COMPOSITE, 0.1, Y, full=True)
    b = ctx.logpdf_multi(X, COMPOSITE, 0.1, Y[:, perm], full=True)
    for u, v in ((a[0], b[0]), (a[2], b[2])):
        print("permuted columns bitwise:", bool(np.array_equal(u[perm], v)))
        assert np.max(np.abs(u[perm] - v) / np.abs(v)) <= 1e-13


def raw_args(ctx, X, terms, noise):
    Xc = np.asfortranarray(X, dtype=np.float64)
    N, D = Xc.shape
    return Xc, (ctx.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), term_array(terms), float(noise))


def test_leading_dimensions_and_padding_rows(ctx):
    rng = np.random.default_rng(5)
    N, Rn = 129, 70
    X = cols(rng, N)
    Y = rng.normal(size=(N, Rn))
    Xc, head = raw_args(ctx, X, COMPOSITE, 0.1)
    ref = ctx.logpdf_multi(X, COMPOSITE, 0.1, Y, full=True)
    Yp = np.full((N + 3, Rn), np.nan, order="F")
    Yp[:N] = Y
    lp, q, ld = np.empty(Rn), np.empty(Rn), c_double()
    rc = ctx.lib.gaplac_logpdf_multi(*head, Rn, Yp.ctypes.data_as(c_void_p), N + 3, lp.ctypes.data_as(c_void_p),
                                     byref(ld), q.ctypes.data_as(c_void_p))
    assert rc == 0
    assert np.array_equal(lp, ref[0]) and ld.value == ref[1] and np.array_equal(q, ref[2])
    sref = ctx.rand_multi(X, COMPOSITE, 0.1, Y)
    Zp = np.full((N + 5, Rn), np.nan, order="F")
    Zp[:N] = Y
    out = np.full((N + 7, Rn), -7.5, order="F")
    rc = ctx.lib.gaplac_rand_multi(*head, Rn, Zp.ctypes.data_as(c_void_p), N + 5, out.ctypes.data_as(c_void_p), N + 7)
    assert rc == 0
    assert np.array_equal(out[:N], sref)
    assert np.all(out[N:] == -7.5)  # the canaries in the padding rows


@pytest.mark.parametrize("N,Rn", [(1, 1), (2, 5), (127, 3), (128, 16), (129, 17), (511, 130), (513, 64), (1000, 257)])
def test_rand_multi_matches_oracle_and_single_rand(ctx, N, Rn):
    rng = np.random.default_rng(N + Rn)
    X = np.column_stack([rng.uniform(-5, 5, N), rng.integers(0, 9, N).astype(float)])
    terms = [(SQEXP, 0, 1.2, 0), (CAT, 1, 0.0, 1)]
    Z = rng.normal(size=(N, Rn))
    S = ctx.rand_multi(X, terms, 0.1, Z)
    assert S.shape == (N, Rn)
    ref = R.rand_from(X, terms, 0.1, Z)
    bar = 1e-12 * max(1.0, np.max(np.abs(ref)))
    print("max |S - oracle|", np.max(np.abs(S - ref)), "bar", bar)
    assert np.max(np.abs(S - ref)) <= bar
    for r in sorted({0, Rn // 2, Rn - 1}):
        assert np.max(np.abs(S[:, r] - ctx.rand(X, terms, 0.1, Z[:, r]))) <= bar


def test_nonpd_raises_and_fills_nan(ctx):
    X = np.repeat(np.arange(8.0), 4)[:, None]
    terms = [(CAT, 0, 0.0, 0)]
    Y = np.ones((32, 3))
    with pytest.raises(PosDefException):
        ctx.logpdf_multi(X, terms, 0.0, Y)
    with pytest.raises(PosDefException):
        ctx.rand_multi(X, terms, 0.0, Y)
    Xc, head = raw_args(ctx, X, terms, 0.0)
    Yc = np.asfortranarray(Y)
    lp, q, ld = np.zeros(3), np.zeros(3), c_double(0.0)
    rc = ctx.lib.gaplac_logpdf_multi(*head, 3, Yc.ctypes.data_as(c_void_p), 32, lp.ctypes.data_as(c_void_p), byref(ld),
                                     q.ctypes.data_as(c_void_p))
    assert rc > 0 and np.all(np.isnan(lp)) and np.all(np.isnan(q)) and np.isnan(ld.value)
    out = np.zeros((32, 3), order="F")
    rc2 = ctx.lib.gaplac_rand_multi(*head, 3, Yc.ctypes.data_as(c_void_p), 32, out.ctypes.data_as(c_void_p), 32)
    assert rc2 == rc and np.all(np.isnan(out))
    # the context stays usable
    assert np.all(np.isfinite(ctx.logpdf_multi(np.arange(4.0), [(SQEXP, 0, 1.0, 0)], 0.1, np.ones((4, 2)))))


def test_empty_inputs(ctx):
    terms = [(SQEXP, 0, 1.0, 0)]
    X = np.arange(6.0)[:, None]
    lp, ld, q = ctx.logpdf_multi(X, terms, 0.1, np.zeros((6, 0)), full=True)
    assert lp.shape == (0,) and q.shape == (0,)
    assert ctx.rand_multi(X, terms, 0.1, np.zeros((6, 0))).shape == (6, 0)
    lp, ld, q = ctx.logpdf_multi(np.zeros((0, 1)), terms, 0.1, np.zeros((0, 4)), full=True)
    assert lp.shape == (4,) and np.all(lp == 0.0) and np.all(np.signbit(lp)) and ld == 0.0 and np.all(q == 0.0)
    assert ctx.rand_multi(np.zeros((0, 1)), terms, 0.1, np.zeros((0, 4))).shape == (0, 4)
    # R = 0 writes nothing; N = 0 leaves out untouched (raw calls with canaries)
    Xc, head = raw_args(ctx, X, terms, 0.1)
    can = np.full(4, -7.5)
    ldv = c_double(-7.5)
    assert ctx.lib.gaplac_logpdf_multi(*head, 0, None, 6, can.ctypes.data_as(c_void_p), byref(ldv), None) == 0
    assert np.all(can == -7.5) and ldv.value == -7.5
    _, head0 = raw_args(ctx, np.zeros((0, 1)), terms, 0.1)
    out = np.full((2, 4), -7.5, order="F")
    assert ctx.lib.gaplac_rand_multi(*head0, 4, None, 0, out.ctypes.data_as(c_void_p), 2) == 0
    assert np.all(out == -7.5)
    # bad terms are reported before the R = 0 return
    with pytest.raises(ArgumentError):
        ctx.logpdf_multi(X, [(SQEXP, 0, -1.0, 0)], 0.1, np.zeros((6, 0)))


def test_argument_errors(ctx):
    terms = [(SQEXP, 0, 1.0, 0)]
    X = np.arange(6.0)[:, None]
    with pytest.raises(ArgumentError):
        ctx.logpdf_multi(X, terms, 0.1, np.zeros((5, 2)))
    with pytest.raises(ArgumentError):
        ctx.rand_multi(X, terms, 0.1, np.zeros((7, 2)))
    with pytest.raises(ArgumentError):
        ctx.logpdf_multi(X, terms, 0.1, np.zeros(6))
    Xc, head = raw_args(ctx, X, terms, 0.1)
    Y = np.zeros((6, 2), order="F")
    o = np.zeros((6, 2), order="F")
    yp, op = Y.ctypes.data_as(c_void_p), o.ctypes.data_as(c_void_p)
    ld = c_double()
    lm, rm = ctx.lib.gaplac_logpdf_multi, ctx.lib.gaplac_rand_multi
    bad = [lm(*head, -1, yp, 6, op, byref(ld), None), lm(*head, 2, None, 6, op, byref(ld), None),
           lm(*head, 2, yp, 5, op, byref(ld), None), lm(*head, 2, yp, 6, None, byref(ld), None),
           rm(*head, -1, yp, 6, op, 6), rm(*head, 2, None, 6, op, 6), rm(*head, 2, yp, 5, op, 6),
           rm(*head, 2, yp, 6, op, 5), rm(*head, 2, yp, 6, None, 6)]
    for rc in bad:
        with pytest.raises(ArgumentError):
            ctx._check(rc)


def test_abstractgps_surface(ctx):
    rng = np.random.default_rng(21)
    N, Rn = 200, 6
    x = rng.uniform(-5, 5, N)
    g = rng.integers(0, 12, N).astype(float)
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))
    fx = AG.FiniteGP(gp, x, 0.1)
    Y = rng.normal(size=(N, Rn))
    lp = AG.logpdf(fx, Y, ctx=ctx)
    assert lp.shape == (Rn,)
    one = np.array([AG.logpdf(fx, Y[:, r], ctx=ctx) for r in range(Rn)])
    assert np.all(np.abs(lp - one) <= RTOL * np.abs(one))
    a = AG.rand(fx, n=4, rng=np.random.default_rng(1), ctx=ctx)
    b = AG.rand(fx, z=np.random.default_rng(1).standard_normal((N, 4)), ctx=ctx)
    assert a.shape == (N, 4) and np.array_equal(a, b)
    assert AG.rand(fx, rng=np.random.default_rng(1), ctx=ctx).shape == (N,)  # neither: as before
    table = {"x": x, "g": g}
    names = [f"y{r}" for r in range(Rn)]
    for r, nm in enumerate(names):
        table[nm] = Y[:, r]
    f1, f2 = "y0 ~| SqExp(:x; l=1.5) + Cat(:g)", "y0 ~| OU(:x; l=2)"
    bayes, lp1, lp2 = AG.select_formulae(f1, f2, table, ctx=ctx, responses=names)
    assert bayes.shape == lp1.shape == lp2.shape == (Rn,)
    for r, nm in enumerate(names):
        sb, s1, s2 = AG.select_formulae(f1.replace("y0", nm), f2.replace("y0", nm), table, ctx=ctx)
        assert abs(lp1[r] - s1) <= RTOL * abs(s1) and abs(lp2[r] - s2) <= RTOL * abs(s2)
        assert abs(bayes[r] - sb) <= RTOL * (abs(s1) + abs(s2))  # a difference of two 1e-9 results
