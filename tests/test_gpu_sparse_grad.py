"""Parity of gaplac_sparse_elbo_grad (HIP, through the C-ABI) against the dense N x N route of
tests/sparse_grad_oracle.py (pinned to the Woodbury route and to central differences of the bound
by tests/test_sparse_grad_oracle.py).

Bars (the project's 1e-9): dparam[t] within 1e-9 of (|ref| + its addend magnitude |diag addend| +
sum |G_uf o dKuf| + sum |G_uu o dKuu|), as tests/test_gpu_grad.py judges its entries (they cancel
to 1e-7 of that magnitude on these inputs); dnoise and djitter 1e-9 relative; dy within 1e-9 of
max |dy|; dparam of CAT exactly 0; elbo bitwise gaplac_sparse_elbo's. The two CPU routes differ by
at most 2.6e-15, 3.3e-14, 4.0e-13 and 6.4e-13 of those scales. Each test prints its observed
maxima before it asserts.
"""
import math
from ctypes import byref, c_double, c_void_p

import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd import formula as F
from gaplac_amd._native import CAT, LINEAR, NOISE, OU, SQEXP, term_array
from gaplac_amd.backend import ArgumentError, Context, PosDefException
from gaplac_amd.mcmc import MCMCModel
from oracle import restatement as R
from tests import sparse_grad_oracle as G
from tests import sparse_oracle as S
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
TOL = 1e-9
COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (LINEAR, 2, 0.5, 3)]
PRODUCT = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 0), (CAT, 1, 0.0, 1), (LINEAR, 2, 0.5, 1), (NOISE, 0, 0.05, 2)]
SHAPES = [(1, 1), (5, 129), (127, 128), (129, 127), (300, 5), (700, 127), (1000, 129), (513, 513), (2000, 257)]
_cases = {}


class Case(S.Case):
    """sparse_oracle.Case's inputs with the gradient's dense reference, computed once."""

    def __init__(self, N, Mz, terms, jitter):
        super().__init__(N, Mz, 1, terms, 0.1, jitter)  # (one test point: X, Z and y come first in the draw order)
        self.grad = G.dense(self.X, terms, 0.1, self.y, self.Z, jitter)


def case(N, Mz, jitter=1e-6, terms=COMPOSITE):
    key = (N, Mz, jitter, tuple(terms))
    if key not in _cases:
        _cases[key] = Case(N, Mz, terms, jitter)
    return _cases[key]


@pytest.fixture(scope="module")
def ctx():
    if not gpu_available():
        pytest.skip("no GPU")
    c = Context(0)
    yield c
    c.close()


def check_grad(got, ref, terms):
    elbo, dy, dp, dn, dj = got
    ep = np.abs(dp - ref["dparam"]) / (np.abs(ref["dparam"]) + ref["scale"]).clip(1e-300)
    print("rel elbo", abs(elbo - ref["elbo"]) / abs(ref["elbo"]), "dparam / (|ref| + addends)", ep,
          "cancellation |ref| / addends", np.abs(ref["dparam"]) / ref["scale"].clip(1e-300),
          "rel dnoise", abs(dn - ref["dnoise"]) / abs(ref["dnoise"]), "rel djitter", abs(dj - ref["djitter"]) / abs(ref["djitter"]),
          "dy / max|dy|", np.max(np.abs(dy - ref["dy"])) / np.max(np.abs(ref["dy"])))
    assert abs(elbo - ref["elbo"]) <= TOL * abs(ref["elbo"])
    for t, term in enumerate(terms):
        assert abs(dp[t] - ref["dparam"][t]) <= TOL * (abs(ref["dparam"][t]) + ref["scale"][t]), (t, dp[t], ref["dparam"][t])
        if term[0] == CAT:
            assert dp[t] == 0.0
    assert abs(dn - ref["dnoise"]) <= TOL * abs(ref["dnoise"])
    assert abs(dj - ref["djitter"]) <= TOL * abs(ref["djitter"])
    assert np.max(np.abs(dy - ref["dy"])) <= TOL * np.max(np.abs(ref["dy"]))


def run(ctx, c):
    got = ctx.sparse_elbo_grad(c.X, c.terms, c.noise, c.y, c.Z, c.jitter)
    assert got[1].shape == (c.N,) and got[2].shape == (len(c.terms),)
    assert got[0] == ctx.sparse_elbo(c.X, c.terms, c.noise, c.y, c.Z, c.jitter)  # bitwise
    return got


@pytest.mark.parametrize("N,Mz", SHAPES)
def test_shapes_composite(ctx, N, Mz):
    c = case(N, Mz)
    check_grad(run(ctx, c), c.grad, c.terms)


@pytest.mark.parametrize("N,Mz", [(700, 127), (513, 513)])
def test_larger_jitter(ctx, N, Mz):
    c = case(N, Mz, 1e-2)
    check_grad(run(ctx, c), c.grad, c.terms)


def test_product_groups_and_noise_term(ctx):
    c = case(700, 127, 1e-6, PRODUCT)
    check_grad(run(ctx, c), c.grad, c.terms)


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]


def test_repeatable_bitwise_and_dirty_workspace(ctx):
    c = case(1000, 129)
    a = run(ctx, c)
    b = run(ctx, c)
    assert same(a, b)
    big = case(2000, 257)                               # a larger unrelated evaluation dirties every buffer
    ctx.sparse_elbo_grad(big.X, big.terms, 0.1, big.y, big.Z, 1e-2)
    ctx.logpdf_grad(big.X, big.terms, 0.1, big.y)
    assert same(a, run(ctx, c))
    with Context(0) as other:
        assert same(a, run(other, c))
    p = case(700, 127, 1e-6, PRODUCT)
    assert same(run(ctx, p), run(ctx, p))


@pytest.mark.parametrize("N", [129, 300])
def test_exact_when_the_inducing_points_are_the_data(ctx, N):
    # Z = X, jitter 0: Q = K, the bound is tight (trace = 0, its derivative vanishes) and the
    # gradient is logpdf_grad's; the bar is this entry's own addend magnitude at Z = X
    rng = np.random.default_rng(N)
    X = S.cols(rng, N)
    y = rng.normal(size=N)
    terms = [(OU, 0, 3.0, 0), (CAT, 1, 0.0, 1), (LINEAR, 2, 0.5, 2)]
    lp, dv, dp, dn = ctx.logpdf_grad(X, terms, 0.1, y)
    elbo, dy, dparam, dnoise, _ = ctx.sparse_elbo_grad(X, terms, 0.1, y, X, 0.0)
    scale = G.dense(X, terms, 0.1, y, X, 0.0)["scale"]
    print("rel elbo", abs(elbo - lp) / abs(lp), "dparam / (|ref| + addends)",
          np.abs(dparam - dp) / (np.abs(dp) + scale).clip(1e-300),
          "dy / max|dy|", np.max(np.abs(dy - dv)) / np.max(np.abs(dv)), "rel dnoise", abs(dnoise - dn) / abs(dn))
    assert abs(elbo - lp) <= TOL * abs(lp)
    for t in range(len(terms)):
        assert abs(dparam[t] - dp[t]) <= TOL * (abs(dp[t]) + scale[t]), (t, dparam[t], dp[t])
    assert dparam[1] == 0.0
    assert np.max(np.abs(dy - dv)) <= TOL * np.max(np.abs(dv))


def _raw(ctx, X, terms, noise, y, Z, ldz, jitter, nulls=False):
    Xc, Zc = np.asfortranarray(X), np.asfortranarray(Z)
    N, T = Xc.shape[0], len(terms)
    elbo, dn, dj = c_double(7.0), c_double(7.0), c_double(7.0)
    dy, dp = np.full(max(N, 1), 7.0), np.full(max(T, 1), 7.0)
    outs = ((byref(elbo), None, None, None, None) if nulls else
            (byref(elbo), dy.ctypes.data_as(c_void_p), dp.ctypes.data_as(c_void_p), byref(dn), byref(dj)))
    rc = ctx.lib.gaplac_sparse_elbo_grad(ctx.h, N, Xc.shape[1], Xc.ctypes.data_as(c_void_p), max(1, N), T,
                                         term_array(terms), noise, np.ascontiguousarray(y).ctypes.data_as(c_void_p),
                                         Zc.shape[0], Zc.ctypes.data_as(c_void_p), ldz, jitter, *outs)
    return rc, elbo.value, dy[:N], dp[:T], dn.value, dj.value


def all_nan(r):
    return math.isnan(r[1]) and np.all(np.isnan(r[2])) and np.all(np.isnan(r[3])) and math.isnan(r[4]) and math.isnan(r[5])


def test_empty_sets_and_null_outputs(ctx):
    c = case(300, 5)
    e0 = np.zeros((0, 3))
    elbo, dy, dp, dn, dj = ctx.sparse_elbo_grad(e0, COMPOSITE, 0.1, np.zeros(0), c.Z, 1e-6)       # N = 0
    assert elbo == 0.0 and dy.shape == (0,) and np.all(dp == 0.0) and dn == 0.0 and dj == 0.0
    elbo, dy, dp, dn, dj = ctx.sparse_elbo_grad(c.X, PRODUCT, 0.1, c.y, e0, 1e-6)                 # Mz = 0
    assert elbo == ctx.sparse_elbo(c.X, PRODUCT, 0.1, c.y, e0, 1e-6)
    dd = [b[0] for b in G.derivative_blocks(c.X, e0, PRODUCT)]
    trace = float(np.sum(R.kernel_diag(c.X, PRODUCT)))
    assert np.allclose(dy, -c.y / 0.1, rtol=1e-15, atol=0)
    assert np.allclose(dp, -np.array(dd) / 0.2, rtol=1e-14, atol=0) and dp[2] == 0.0 and dj == 0.0
    assert abs(dn - (0.5 * (float(c.y @ c.y) / 0.01 - 300 / 0.1) + trace / 0.02)) <= 1e-12 * abs(dn)
    full = run(ctx, c)
    r = _raw(ctx, c.X, COMPOSITE, 0.1, c.y, c.Z, 5, 1e-6, nulls=True)                            # every optional output NULL
    assert r[0] == 0 and r[1] == full[0]
    rc = ctx.lib.gaplac_sparse_elbo_grad(ctx.h, 300, 3, np.asfortranarray(c.X).ctypes.data_as(c_void_p), 300, 4,
                                         term_array(COMPOSITE), 0.1, c.y.ctypes.data_as(c_void_p), 5,
                                         np.asfortranarray(c.Z).ctypes.data_as(c_void_p), 5, 1e-6, None, None, None,
                                         None, None)
    assert rc == _native.E_ARG                                                                    # out_elbo NULL
    assert same(full, run(ctx, c))


def test_failures_leave_nan_and_a_usable_context(ctx):
    c = case(300, 5)
    ref = run(ctx, c)
    cat = [(CAT, 1, 0.0, 0)]
    Zd = c.Z.copy()
    Zd[1] = Zd[0]                                       # the inducing covariance's second pivot is exactly 0
    with pytest.raises(PosDefException) as e:
        ctx.sparse_elbo_grad(c.X, cat, 0.1, c.y, Zd, 0.0)
    assert e.value.info == 2
    r = _raw(ctx, c.X, cat, 0.1, c.y, Zd, 5, 0.0)
    assert r[0] == 2 and all_nan(r)
    assert b"inducing covariance" in ctx.lib.gaplac_last_error(ctx.h)
    # S = noise I + V V^T is positive definite in exact arithmetic; a LINEAR term on inputs of 1e140
    # makes V V^T a rank-2 matrix of entries ~1e286 whose three other pivots are rounding noise of
    # either sign, far above the noise: the first draw whose value entry reports S (7 of 8 do in
    # expectation) must fail the same way here
    lin, info = [(LINEAR, 2, 0.5, 0)], 0
    for seed in range(8):
        Xh = c.X.copy()
        Xh[:, 2] = 1e140 * (1.0 + np.random.default_rng(seed).uniform(size=300))
        try:
            ctx.sparse_elbo(Xh, lin, 0.1, c.y, c.Z, 1e-6)
        except PosDefException as e:
            info = e.info
            break
    assert info > 0 and b"S = noise I" in ctx.lib.gaplac_last_error(ctx.h)
    r = _raw(ctx, Xh, lin, 0.1, c.y, c.Z, 5, 1e-6)
    assert r[0] == info and all_nan(r)
    assert b"S = noise I" in ctx.lib.gaplac_last_error(ctx.h)
    big = np.zeros((65535 * 128 + 1, 1))                # one tile row past the cross-covariance grid: no chunking
    r = _raw(ctx, big, [(SQEXP, 0, 1.0, 0)], 0.1, big[:, 0], c.Z[:, :1], 5, 1e-6)
    assert r[0] == _native.E_OOM and all_nan(r)
    assert same(ref, run(ctx, c))                       # the next call on the same context is correct
    for noise, jitter in ((0.0, 1e-6), (-0.1, 1e-6), (float("nan"), 1e-6), (float("inf"), 1e-6), (0.1, -1e-6),
                          (0.1, float("nan"))):
        with pytest.raises(ArgumentError):
            ctx.sparse_elbo_grad(c.X, COMPOSITE, noise, c.y, c.Z, jitter)
        r = _raw(ctx, c.X, COMPOSITE, noise, c.y, c.Z, 5, jitter)
        assert r[0] == _native.E_PARAM and all_nan(r)
    r = _raw(ctx, c.X, COMPOSITE, 0.1, c.y, c.Z, 4, 1e-6)                                         # ldz < Mz
    assert r[0] == _native.E_ARG and all_nan(r)
    r = _raw(ctx, c.X, [(SQEXP, 7, 1.0, 0)], 0.1, c.y, c.Z, 5, 1e-6)                              # a column past D
    assert r[0] == _native.E_COL and all_nan(r)
    r = _raw(ctx, c.X, [(9, 0, 1.0, 0)], 0.1, c.y, c.Z, 5, 1e-6)                                  # an unknown kind
    assert r[0] == _native.E_KIND and all_nan(r)
    with pytest.raises(ArgumentError):
        ctx.sparse_elbo_grad(c.X, COMPOSITE, 0.1, c.y[:-1], c.Z, 1e-6)
    with pytest.raises(ArgumentError):
        ctx.sparse_elbo_grad(c.X, COMPOSITE, 0.1, c.y, c.Z[:, :2], 1e-6)
    assert same(ref, run(ctx, c))


def test_abstractgps_surface(ctx, monkeypatch):
    rng = np.random.default_rng(13)
    x = rng.uniform(-5, 5, 400)
    y = np.sin(x) + 0.3 * rng.normal(size=400)
    z = np.linspace(-5, 5, 12)
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))
    fx, vfe = gp(x, 0.1), AG.VFE(gp(z, 1e-6))
    assert same(AG.elbo_and_gradient(vfe, fx, y, ctx=ctx), ctx.sparse_elbo_grad(x, fx.terms, 0.1, y, z, 1e-6))
    assert AG.elbo_and_gradient(vfe, fx, y, ctx=ctx)[0] == AG.elbo(vfe, fx, y, ctx=ctx)
    monkeypatch.setenv("GAPLAC_HIP", "0")
    with pytest.raises(AG.BackendDisabled):
        AG.elbo_and_gradient(vfe, fx, y, ctx=ctx)


def test_mcmc_model_with_inducing_inputs_matches_central_differences(ctx):
    # N = 700, Mz = 127: d/dl and two entries of d/dfx of the model's own logdensity. Central
    # differences at step h carry h^2 f''' / 6 of truncation and ~10 eps |lp| / h of rounding:
    # the bar is test_grad_oracle's 1e-6 (of max(1, |fd|)) plus that rounding floor.
    rng = np.random.default_rng(700 * 7 + 127)
    N, Mz = 700, 127
    table = {"y": rng.normal(size=N), "x": rng.uniform(0, 10, N), "t": rng.uniform(0, 10, N)}
    Z = np.column_stack([rng.uniform(0, 10, Mz), rng.uniform(0, 10, Mz)])
    m = MCMCModel("y ~| SqExp(:x) + OU(:t; l=3)", table, ["x"], ctx=ctx, inducing=Z, jitter=1e-6)
    fx = 0.5 * rng.normal(size=N)
    ell = 2.5
    lp, dell, dfx = m.logdensity_and_gradient(ell, fx)
    assert lp == m.logdensity(ell, fx)
    h = 1e-4
    fd = (m.logdensity(ell + h, fx) - m.logdensity(ell - h, fx)) / (2 * h)
    floor = 10 * 2.2e-16 * abs(lp) / h
    print("dl", dell, fd, abs(dell - fd), "bar", 1e-6 * max(1.0, abs(fd)) + floor)
    assert abs(dell - fd) <= 1e-6 * max(1.0, abs(fd)) + floor
    for i in (3, N - 1):
        e = np.zeros(N)
        e[i] = 1e-5
        fd = (m.logdensity(ell, fx + e) - m.logdensity(ell, fx - e)) / 2e-5
        floor = 10 * 2.2e-16 * abs(lp) / 1e-5
        print("dfx", i, dfx[i], fd, abs(dfx[i] - fd), "bar", 1e-6 * max(1.0, abs(fd)) + floor)
        assert abs(dfx[i] - fd) <= 1e-6 * max(1.0, abs(fd)) + floor
    assert m.memo.calls == 1
