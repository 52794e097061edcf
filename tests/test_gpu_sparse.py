"""Parity of the inducing-point (VFE) entries gaplac_sparse_elbo / gaplac_sparse_posterior_mean_var
(HIP, through the C-ABI) against the CPU recipe of tests/sparse_oracle.py (its two routes pinned to
each other by tests/test_sparse_oracle.py): the dense N x N route up to N = 2000, the Woodbury
route above.

Bars (the project's north-star 1e-9): elbo and dtc 1e-9 relative; logdet, quad and trace within
1e-9 |dtc| (as tests/test_gpu_joint.py's check_logpdf judges logdet and quad); mean within
1e-9 max(1, max |mean|); variance within 1e-9 max(1, kdiag) (tests/test_gpu_posterior.py). The
two CPU routes differ by at most 6.7e-14, 2.9e-12 and 5.7e-16 of those scales on these inputs.
Each test prints its observed maxima before it asserts.
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
from tests import sparse_oracle as S
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
TOL = 1e-9
COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (LINEAR, 2, 0.5, 3)]
SIX = [(300, 1), (300, 5), (700, 127), (1000, 129), (2000, 257), (513, 513)]
PADDING = [(1, 1, 1), (5, 129, 3), (127, 128, 129), (129, 127, 128)]
_cases = {}


def case(N, Mz, Ms, jitter=1e-6):
    key = (N, Mz, Ms, jitter)
    if key not in _cases:
        _cases[key] = S.Case(N, Mz, Ms, COMPOSITE, 0.1, jitter)
    return _cases[key]


@pytest.fixture(scope="module")
def ctx():
    if not gpu_available():
        pytest.skip("no GPU")
    c = Context(0)
    yield c
    c.close()


def check_elbo(got, ref):
    scale = abs(ref["dtc"])
    print("rel elbo", abs(got["elbo"] - ref["elbo"]) / abs(ref["elbo"]), "rel dtc", abs(got["dtc"] - ref["dtc"]) / scale,
          "logdet", abs(got["logdet"] - ref["logdet"]), "quad", abs(got["quad"] - ref["quad"]),
          "trace", abs(got["trace"] - ref["trace"]), "bar", TOL * scale)
    assert abs(got["elbo"] - ref["elbo"]) <= TOL * abs(ref["elbo"])
    assert abs(got["dtc"] - ref["dtc"]) <= TOL * scale
    for k in ("logdet", "quad", "trace"):
        assert abs(got[k] - ref[k]) <= TOL * scale, k


def check_post(m, v, rm, rv, kd):
    print("max |mean - oracle|", np.max(np.abs(m - rm)), "bar", TOL * max(1.0, np.max(np.abs(rm))),
          "max |var - oracle| / max(1, kdiag)", np.max(np.abs(v - rv) / np.maximum(1.0, np.abs(kd))))
    assert np.max(np.abs(m - rm)) <= TOL * max(1.0, np.max(np.abs(rm)))
    assert np.all(np.abs(v - rv) <= TOL * np.maximum(1.0, np.abs(kd)))


def check_case(ctx, c):
    got = ctx.sparse_elbo(c.X, c.terms, c.noise, c.y, c.Z, c.jitter, full=True)
    check_elbo(got, c.ref)
    m, v = ctx.sparse_posterior_mean_var(c.X, c.terms, c.noise, c.y, c.Z, c.jitter, c.Xs)
    assert m.shape == (c.Ms,) and v.shape == (c.Ms,)
    check_post(m, v, c.ref["mean"], c.ref["var"], c.kd)
    return got, m, v


@pytest.mark.parametrize("jitter", [1e-6, 1e-2])
@pytest.mark.parametrize("N,Mz", SIX)
def test_sizes_composite(ctx, N, Mz, jitter):
    check_case(ctx, case(N, Mz, 64, jitter))


@pytest.mark.parametrize("N,Mz,Ms", PADDING)
def test_padding_edges(ctx, N, Mz, Ms):
    check_case(ctx, case(N, Mz, Ms))


@pytest.mark.parametrize("Mz", [5, 129])
@pytest.mark.parametrize("k", range(4))
def test_split_edges(ctx, Mz, k):
    _, c = ctx.sparse_split(1, Mz)
    N = (c - 1, c, c + 1, 2 * c + 3)[k]
    assert N <= 20000                                   # (the smallest ragged two-chunk shape stays quick)
    assert ctx.sparse_split(N, Mz) == (-(-N // c), c)   # N stands on the chunk edge
    check_case(ctx, case(N, Mz, 7))


def test_split_rule(ctx):
    with Context(0) as other:                           # neither the call nor the context matters
        for N, Mz in ((0, 0), (1, 1), (2051, 129), (16384, 1024), (262144, 4096), (10**6, 4096)):
            a = ctx.sparse_split(N, Mz)
            assert a == ctx.sparse_split(N, Mz) == other.sparse_split(N, Mz)
            assert a[1] % 1024 == 0 and a[0] == -(-N // a[1])
    with pytest.raises(ArgumentError):
        ctx.sparse_split(-1, 1)


def test_many_chunks_and_tiles(ctx):
    # 20 chunks over 3 x 3 tiles of S: the Woodbury route is the reference above N = 2000
    c = case(20000, 300, 7)
    assert ctx.sparse_split(20000, 300) == (20, 1024)
    check_case(ctx, c)


def test_long_chunks_closed_form(ctx):
    # N = 15000 rows at Mz = 4096 (561 tiles) is past the cap on partial tiles: 8 chunks of 2048
    # rows, the last one ragged. A Cat kernel with the inducing points at the categories has
    # Kuu = I, so with c_g observations summing to s_g in category g and d = 1 + jitter:
    # S = noise I + diag(c) / d, w = s / sqrt(d), and everything follows in closed form.
    N, G, noise, jit = 15000, 4096, 0.1, 1e-2
    assert ctx.sparse_split(N, G) == (8, 2048)
    rng = np.random.default_rng(5)
    g = rng.integers(0, G, N)
    y = rng.normal(size=N)
    X, Z = g.astype(float)[:, None], np.arange(G, dtype=float)[:, None]
    terms = [(CAT, 0, 0.0, 0)]
    d = 1.0 + jit
    cnt = np.bincount(g, minlength=G).astype(float)
    s = np.bincount(g, weights=y, minlength=G)
    Sd = noise + cnt / d
    logdet = (N - G) * np.log(noise) + np.sum(np.log(Sd))
    quad = (y @ y - np.sum(s * s / d / Sd)) / noise
    dtc = -((N * R.LOG2PI + logdet) + quad) / 2
    trace = N * (1.0 - 1.0 / d)
    ref = dict(elbo=dtc - trace / (2 * noise), dtc=dtc, trace=trace, logdet=logdet, quad=quad)
    check_elbo(ctx.sparse_elbo(X, terms, noise, y, Z, jit, full=True), ref)
    gs = np.array([0, 1, 17, G - 1, G + 5])             # (the last one is a category nobody observed)
    m, v = ctx.sparse_posterior_mean_var(X, terms, noise, y, Z, jit, gs.astype(float)[:, None])
    seen = gs < G
    rm = np.where(seen, s[np.minimum(gs, G - 1)] / d / Sd[np.minimum(gs, G - 1)], 0.0)
    rv = np.where(seen, 1.0 - 1.0 / d + noise / d / Sd[np.minimum(gs, G - 1)], 1.0)
    check_post(m, v, rm, rv, np.ones(len(gs)))


def test_repeatable_bitwise(ctx):
    c = case(2051, 129, 7)
    a = ctx.sparse_elbo(c.X, c.terms, 0.1, c.y, c.Z, 1e-6, full=True)
    pa = ctx.sparse_posterior_mean_var(c.X, c.terms, 0.1, c.y, c.Z, 1e-6, c.Xs)
    ctx.sparse_elbo(c.X[:700], c.terms, 0.1, c.y[:700], c.Z[:5], 1e-2)      # (another shape in between)
    b = ctx.sparse_elbo(c.X, c.terms, 0.1, c.y, c.Z, 1e-6, full=True)
    pb = ctx.sparse_posterior_mean_var(c.X, c.terms, 0.1, c.y, c.Z, 1e-6, c.Xs)
    assert a == b
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])


def test_the_two_entries_agree(ctx):
    # With C = Q + noise I the mean at the training points is m = Q C^{-1} y = y - noise C^{-1} y,
    # and elbo's quad(y) = y^T C^{-1} y is a quadratic form: for t supported on the first 64 points
    # t^T C^{-1} y = (quad(y + t) - quad(y) - quad(t)) / 2, so t . m[:64] = t . y[:64] - noise t^T C^{-1} y.
    c = case(1000, 129, 64)
    X, y, Z = c.X, c.y, c.Z
    m, _ = ctx.sparse_posterior_mean_var(X, COMPOSITE, 0.1, y, Z, 1e-6, X[:64])
    t = np.zeros(len(y))
    t[:64] = np.random.default_rng(3).normal(size=64)
    q = [ctx.sparse_elbo(X, COMPOSITE, 0.1, v, Z, 1e-6, full=True)["quad"] for v in (y + t, y, t)]
    implied = float(t[:64] @ y[:64]) - 0.1 * (q[0] - q[1] - q[2]) / 2
    bar = TOL * np.sum(np.abs(t)) * max(1.0, np.max(np.abs(m)))     # (the mean's bar, entry by entry)
    print("|t . mean - implied|", abs(float(t[:64] @ m) - implied), "bar", bar)
    assert abs(float(t[:64] @ m) - implied) <= bar


def test_product_groups_and_noise_term(ctx):
    rng = np.random.default_rng(12)
    N, Mz, Ms = 260, 70, 190
    X = np.column_stack([rng.uniform(0, 5, N), rng.normal(size=N)])
    Z = np.column_stack([rng.uniform(0, 5, Mz), rng.normal(size=Mz)])
    Xs = np.column_stack([rng.uniform(0, 5, Ms), rng.normal(size=Ms)])
    terms = [(SQEXP, 0, 1.3, 0), (LINEAR, 1, 0.4, 0), (OU, 0, 2.5, 1), (NOISE, -1, 0.2, 2)]
    y = rng.normal(size=N)
    ref = S.dense(X, terms, 0.1, y, Z, 1e-6, Xs)
    check_elbo(ctx.sparse_elbo(X, terms, 0.1, y, Z, 1e-6, full=True), ref)
    m, v = ctx.sparse_posterior_mean_var(X, terms, 0.1, y, Z, 1e-6, Xs)
    check_post(m, v, ref["mean"], ref["var"], R.kernel_diag(Xs, terms))


@pytest.mark.parametrize("N", [129, 300])
def test_exact_when_the_inducing_points_are_the_data(ctx, N):
    rng = np.random.default_rng(N)
    X = S.cols(rng, N)
    y = rng.normal(size=N)
    Xs = S.cols(rng, 40)
    terms = [(OU, 0, 3.0, 0), (CAT, 1, 0.0, 1), (LINEAR, 2, 0.5, 2)]
    lp = ctx.logpdf(X, terms, 0.1, y)
    got = ctx.sparse_elbo(X, terms, 0.1, y, X, 0.0, full=True)
    print("rel dtc", abs(got["dtc"] - lp) / abs(lp), "rel elbo", abs(got["elbo"] - lp) / abs(lp), "trace", got["trace"])
    assert abs(got["dtc"] - lp) <= TOL * abs(lp)
    assert abs(got["elbo"] - lp) <= TOL * abs(lp)
    m, v = ctx.sparse_posterior_mean_var(X, terms, 0.1, y, X, 0.0, Xs)
    rm, rv = ctx.posterior_mean_var(X, terms, 0.1, y, Xs)
    check_post(m, v, rm, rv, R.kernel_diag(Xs, terms))


def test_lower_bound(ctx):
    c = case(2000, 257, 64)
    got = ctx.sparse_elbo(c.X, COMPOSITE, 0.1, c.y, c.Z, 1e-6, full=True)
    lp = ctx.logpdf(c.X, COMPOSITE, 0.1, c.y)
    print("elbo", got["elbo"], "dtc", got["dtc"], "logpdf", lp, "trace", got["trace"])
    assert got["elbo"] <= lp
    assert got["trace"] >= 0
    assert got["elbo"] <= got["dtc"]


def _raw_elbo(ctx, X, terms, noise, y, Z, ldz, jitter):
    Xc, Zc = np.asfortranarray(X), np.asfortranarray(Z)
    out = [c_double(7.0) for _ in range(5)]
    rc = ctx.lib.gaplac_sparse_elbo(ctx.h, Xc.shape[0], Xc.shape[1], Xc.ctypes.data_as(c_void_p), max(1, Xc.shape[0]),
                                    len(terms), term_array(terms), noise, np.ascontiguousarray(y).ctypes.data_as(c_void_p),
                                    Zc.shape[0], Zc.ctypes.data_as(c_void_p), ldz, jitter, *(byref(o) for o in out))
    return rc, [o.value for o in out]


def test_failures_leave_nan_and_a_usable_context(ctx):
    c = case(300, 5, 64)
    terms = [(CAT, 1, 0.0, 0)]
    Zd = c.Z.copy()
    Zd[1] = Zd[0]                                       # k = 0 or 1 exactly: the second pivot is exactly 0
    with pytest.raises(PosDefException) as e:
        ctx.sparse_elbo(c.X, terms, 0.1, c.y, Zd, 0.0)
    assert e.value.info == 2
    rc, out = _raw_elbo(ctx, c.X, terms, 0.1, c.y, Zd, 5, 0.0)
    assert rc == 2 and np.all(np.isnan(out))
    assert b"inducing covariance" in ctx.lib.gaplac_last_error(ctx.h)
    Xc, Zc, Xsc = np.asfortranarray(c.X), np.asfortranarray(Zd), np.asfortranarray(c.Xs)
    m, v = np.full(64, 7.0), np.full(64, 7.0)
    rc = ctx.lib.gaplac_sparse_posterior_mean_var(
        ctx.h, 300, 3, Xc.ctypes.data_as(c_void_p), 300, 1, term_array(terms), 0.1, c.y.ctypes.data_as(c_void_p),
        5, Zc.ctypes.data_as(c_void_p), 5, 0.0, 64, Xsc.ctypes.data_as(c_void_p), 64, m.ctypes.data_as(c_void_p),
        v.ctypes.data_as(c_void_p))
    assert rc == 2 and np.all(np.isnan(m)) and np.all(np.isnan(v))
    check_case(ctx, c)                                  # the next call on the same context is correct
    for noise, jitter in ((0.0, 1e-6), (-0.1, 1e-6), (float("nan"), 1e-6), (float("inf"), 1e-6), (0.1, -1e-6),
                          (0.1, float("nan"))):
        with pytest.raises(ArgumentError):
            ctx.sparse_elbo(c.X, COMPOSITE, noise, c.y, c.Z, jitter)
        with pytest.raises(ArgumentError):
            ctx.sparse_posterior_mean_var(c.X, COMPOSITE, noise, c.y, c.Z, jitter, c.Xs)
        rc, out = _raw_elbo(ctx, c.X, COMPOSITE, noise, c.y, c.Z, 5, jitter)
        assert rc == _native.E_PARAM and np.all(np.isnan(out))
    rc, out = _raw_elbo(ctx, c.X, COMPOSITE, 0.1, c.y, c.Z, 4, 1e-6)      # ldz < Mz
    assert rc == _native.E_ARG and np.all(np.isnan(out))
    with pytest.raises(ArgumentError):
        ctx.sparse_elbo(c.X, COMPOSITE, 0.1, c.y[:-1], c.Z, 1e-6)
    with pytest.raises(ArgumentError):
        ctx.sparse_elbo(c.X, COMPOSITE, 0.1, c.y, c.Z[:, :2], 1e-6)
    check_case(ctx, c)


def test_empty_sets_follow_the_header(ctx):
    c = case(300, 5, 64)
    e0 = np.zeros((0, 3))
    got = ctx.sparse_elbo(e0, COMPOSITE, 0.1, np.zeros(0), c.Z, 1e-6, full=True)           # N = 0
    assert all(got[k] == 0.0 for k in got)
    kd = R.kernel_diag(c.Xs, COMPOSITE)
    m, v = ctx.sparse_posterior_mean_var(e0, COMPOSITE, 0.1, np.zeros(0), c.Z, 1e-6, c.Xs)
    assert np.all(m == 0.0) and np.allclose(v, kd, rtol=0, atol=1e-15)
    got = ctx.sparse_elbo(c.X, COMPOSITE, 0.1, c.y, e0, 1e-6, full=True)                   # Mz = 0: Q = 0
    yy, N = float(c.y @ c.y), 300
    dtc = -((N * R.LOG2PI + N * np.log(0.1)) + yy / 0.1) / 2
    trace = float(np.sum(R.kernel_diag(c.X, COMPOSITE)))
    check_elbo(got, dict(elbo=dtc - trace / 0.2, dtc=dtc, trace=trace, logdet=N * np.log(0.1), quad=yy / 0.1))
    m, v = ctx.sparse_posterior_mean_var(c.X, COMPOSITE, 0.1, c.y, e0, 1e-6, c.Xs)
    assert np.all(m == 0.0) and np.allclose(v, kd, rtol=0, atol=1e-15)
    m, v = ctx.sparse_posterior_mean_var(c.X, COMPOSITE, 0.1, c.y, c.Z, 1e-6, e0)          # Ms = 0
    assert m.shape == (0,) and v.shape == (0,)


def test_abstractgps_surface(ctx):
    rng = np.random.default_rng(13)
    N, Mz, Ms = 400, 12, 100
    x = rng.uniform(-5, 5, N)
    y = np.sin(x) + 0.3 * rng.normal(size=N)
    z = np.linspace(-5, 5, Mz)
    xt = np.linspace(x.min() - 1, x.max() + 1, Ms)
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))
    fx = gp(x, 0.1)
    vfe = AG.VFE(gp(z, 1e-6))
    full = ctx.sparse_elbo(x, fx.terms, 0.1, y, z, 1e-6, full=True)
    assert AG.elbo(vfe, fx, y, ctx=ctx) == full["elbo"]
    assert AG.dtc(vfe, fx, y, ctx=ctx) == full["dtc"]
    assert AG.elbo(vfe, fx, y, ctx=ctx, full=True) == full
    post = AG.posterior(vfe, fx, y, ctx=ctx)
    assert isinstance(post, AG.ApproxPosteriorGP)
    m, v = ctx.sparse_posterior_mean_var(x, fx.terms, 0.1, y, z, 1e-6, xt)
    am, av = AG.mean_and_var(post, xt)
    assert np.array_equal(am, m) and np.array_equal(av, v)
    assert np.array_equal(post.mean(xt), m) and np.array_equal(post.var(xt), v)
    ref = S.dense(x, fx.terms, 0.1, y, z, 1e-6, xt)
    check_elbo(full, ref)
    check_post(m, v, ref["mean"], ref["var"], np.ones(Ms))
    # the exact form behaves as before
    em, ev = AG.mean_and_var(AG.posterior(fx, y, ctx=ctx), xt)
    rm, rv = ctx.posterior_mean_var(x, fx.terms, 0.1, y, xt)
    assert np.array_equal(em, rm) and np.array_equal(ev, rv)
    with pytest.raises(F.ArgumentError):
        AG.elbo(vfe, fx, y[:-1], ctx=ctx)
