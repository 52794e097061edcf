"""Parity of gaplac_sparse_elbo_grad_z's dZ (HIP, through the C-ABI) against the dense N x N route
of tests/sparse_grad_z_oracle.py (pinned to the Woodbury route and to central differences of the
bound by tests/test_sparse_grad_z_oracle.py).

Bar (the project's 1e-9, the way dparam is judged): every entry of dZ within 1e-9 of (|ref| + its
addend magnitude sum |G_uf o d1 Kuf| + 2 sum |G_uu o d1 Kuu|); the entries cancel to about 1e-8 of
that magnitude on these inputs, and the two CPU routes differ by at most 6.2e-13 of it. Columns that
only CAT reads, or nothing, are exactly 0. Every other output is bitwise gaplac_sparse_elbo_grad's.
Each test prints its observed maxima before it asserts.
"""
import math
from ctypes import byref, c_double, c_void_p

import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd import formula as F
from gaplac_amd import vfe_fit
from gaplac_amd._native import CAT, LINEAR, NOISE, OU, SQEXP, term_array
from gaplac_amd.backend import Context, PosDefException
from tests import sparse_grad_z_oracle as GZ
from tests import sparse_oracle as S
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
TOL = 1e-9
COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (LINEAR, 2, 0.5, 3)]
PRODUCT = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 0), (CAT, 1, 0.0, 1), (LINEAR, 2, 0.5, 1), (NOISE, 0, 0.05, 2)]
NO_OU = [(SQEXP, 0, 1.5, 0), (CAT, 1, 0.0, 1), (LINEAR, 2, 0.5, 2)]
SHAPES = [(1, 1), (5, 129), (127, 128), (129, 127), (300, 5), (700, 127), (1000, 129), (513, 513), (2000, 257)]
_cases = {}


class Case(S.Case):
    """sparse_oracle.Case's inputs with dZ's dense reference, computed once."""

    def __init__(self, N, Mz, terms, jitter):
        super().__init__(N, Mz, 1, terms, 0.1, jitter)  # (one test point: X, Z and y come first in the draw order)
        self.dZ, self.scale = GZ.dense(self.X, terms, 0.1, self.y, self.Z, jitter)


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


def same(a, b):
    return (a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:5] == b[3:5] and
            (len(a) < 6 or len(b) < 6 or np.array_equal(a[5], b[5])))


def run(ctx, c):
    got = ctx.sparse_elbo_grad(c.X, c.terms, c.noise, c.y, c.Z, c.jitter, wrt_z=True)
    assert len(got) == 6 and got[5].shape == c.Z.shape
    plain = ctx.sparse_elbo_grad(c.X, c.terms, c.noise, c.y, c.Z, c.jitter)
    assert len(plain) == 5 and same(got[:5], plain)     # every other output: bitwise the entry without dZ
    return got


def check_dz(dZ, ref, scale, what=""):
    err = np.abs(dZ - ref) / (np.abs(ref) + scale).clip(1e-300)
    live = scale > 0
    print(what, "dZ / (|ref| + addends): max", err.max(), "cancellation |ref| / addends: min",
          (np.abs(ref[live]) / scale[live]).min() if live.any() else None)
    assert np.all(np.isfinite(dZ))
    assert np.all(np.abs(dZ - ref) <= TOL * (np.abs(ref) + scale)), np.argwhere(np.abs(dZ - ref) > TOL * (np.abs(ref) + scale))[:5]


def check(ctx, c):
    got = run(ctx, c)
    check_dz(got[5], c.dZ, c.scale, (c.N, c.Mz, c.jitter))
    for t in c.terms:
        only_cat = t[0] == CAT and not any(s[1] == t[1] and s[0] in (SQEXP, OU, LINEAR) for s in c.terms)
        if only_cat:
            assert np.all(got[5][:, t[1]] == 0.0) and not np.any(np.signbit(got[5][:, t[1]]))
    return got


@pytest.mark.parametrize("N,Mz", SHAPES)
def test_shapes_composite(ctx, N, Mz):
    check(ctx, case(N, Mz))


@pytest.mark.parametrize("N,Mz", [(700, 127), (513, 513)])
def test_larger_jitter(ctx, N, Mz):
    check(ctx, case(N, Mz, 1e-2))


def test_product_groups_and_noise_term(ctx):
    check(ctx, case(700, 127, 1e-6, PRODUCT))


def test_repeatable_bitwise_and_dirty_workspace(ctx):
    c = case(1000, 129)
    a = run(ctx, c)
    assert same(a, run(ctx, c))
    big = case(2000, 257)                               # a larger unrelated evaluation dirties every buffer
    ctx.sparse_elbo_grad(big.X, big.terms, 0.1, big.y, big.Z, 1e-2, wrt_z=True)
    ctx.logpdf_grad(big.X, big.terms, 0.1, big.y)
    assert same(a, run(ctx, c))
    with Context(0) as other:
        assert same(a, run(other, c))
    p = case(700, 127, 1e-6, PRODUCT)
    assert same(run(ctx, p), run(ctx, p))


def _raw(ctx, X, terms, noise, y, Z, jitter, lddz, null_dz=False):
    Xc, Zc = np.asfortranarray(X), np.asfortranarray(Z)
    N, T, (Mz, D) = Xc.shape[0], len(terms), Zc.shape
    elbo, dn, dj = c_double(7.0), c_double(7.0), c_double(7.0)
    dy, dp = np.full(max(N, 1), 7.0), np.full(max(T, 1), 7.0)
    dz = np.full((max(lddz, Mz, 1), max(D, 1)), 7.0, order="F")
    rc = ctx.lib.gaplac_sparse_elbo_grad_z(ctx.h, N, D, Xc.ctypes.data_as(c_void_p), max(1, N), T, term_array(terms),
                                           noise, np.ascontiguousarray(y).ctypes.data_as(c_void_p), Mz,
                                           Zc.ctypes.data_as(c_void_p), max(1, Mz), jitter, byref(elbo),
                                           dy.ctypes.data_as(c_void_p), dp.ctypes.data_as(c_void_p), byref(dn), byref(dj),
                                           None if null_dz else dz.ctypes.data_as(c_void_p), lddz)
    return rc, (elbo.value, dy[:N], dp[:T], dn.value, dj.value), dz


def all_nan(r):
    return math.isnan(r[0]) and np.all(np.isnan(r[1])) and np.all(np.isnan(r[2])) and math.isnan(r[3]) and math.isnan(r[4])


def test_layout_null_and_exact_zero_columns(ctx):
    c = case(300, 5)
    ref = run(ctx, c)
    rc, outs, dz = _raw(ctx, c.X, COMPOSITE, 0.1, c.y, c.Z, 1e-6, 5 + 3)      # lddz = Mz + 3
    assert rc == 0 and same(outs, ref[:5])
    assert np.array_equal(dz[:5], ref[5]) and np.all(dz[5:] == 7.0)           # the sentinel rows are untouched
    rc, outs, dz = _raw(ctx, c.X, COMPOSITE, 0.1, c.y, c.Z, 1e-6, 0, null_dz=True)
    assert rc == 0 and same(outs, ref[:5]) and np.all(dz == 7.0)              # out_dZ NULL: gaplac_sparse_elbo_grad
    rc, outs, dz = _raw(ctx, c.X, COMPOSITE, 0.1, c.y, c.Z, 1e-6, 4)          # lddz < Mz
    assert rc == _native.E_ARG and all_nan(outs)
    assert b"lddz" in ctx.lib.gaplac_last_error(ctx.h)
    rng = np.random.default_rng(5)                                            # a fourth column that no term reads
    X4, Z4 = np.column_stack([c.X, rng.normal(size=300)]), np.column_stack([c.Z, rng.normal(size=5)])
    got = ctx.sparse_elbo_grad(X4, COMPOSITE, 0.1, c.y, Z4, 1e-6, wrt_z=True)
    assert got[5].shape == (5, 4) and np.array_equal(got[5][:, :3], ref[5])
    for d in (1, 3):
        assert np.all(got[5][:, d] == 0.0) and not np.any(np.signbit(got[5][:, d]))
    assert same(ref, run(ctx, c))


def test_permuting_the_inducing_points_permutes_the_rows(ctx):
    c = case(700, 127)
    perm = np.random.default_rng(1).permutation(127)
    got = ctx.sparse_elbo_grad(c.X, c.terms, 0.1, c.y, c.Z[perm], 1e-6, wrt_z=True)
    check_dz(got[5], c.dZ[perm], c.scale[perm], "permuted")


def test_empty_sets(ctx):
    c = case(300, 5)
    e0 = np.zeros((0, 3))
    got = ctx.sparse_elbo_grad(e0, COMPOSITE, 0.1, np.zeros(0), c.Z, 1e-6, wrt_z=True)            # N = 0
    assert got[0] == 0.0 and got[5].shape == (5, 3) and np.all(got[5] == 0.0)
    got = ctx.sparse_elbo_grad(c.X, COMPOSITE, 0.1, c.y, e0, 1e-6, wrt_z=True)                    # Mz = 0
    assert got[5].shape == (0, 3) and same(got[:5], ctx.sparse_elbo_grad(c.X, COMPOSITE, 0.1, c.y, e0, 1e-6))
    rc, outs, dz = _raw(ctx, c.X, COMPOSITE, 0.1, c.y, e0, 1e-6, 2)
    assert rc == 0 and np.all(dz == 7.0)                                                          # nothing is written


def test_posdef_failure_leaves_nan_and_a_usable_context(ctx):
    c = case(300, 5)
    ref = run(ctx, c)
    cat = [(CAT, 1, 0.0, 0)]
    Zd = c.Z.copy()
    Zd[1] = Zd[0]                                       # the inducing covariance's second pivot is exactly 0
    with pytest.raises(PosDefException) as e:
        ctx.sparse_elbo_grad(c.X, cat, 0.1, c.y, Zd, 0.0, wrt_z=True)
    assert e.value.info == 2
    rc, outs, dz = _raw(ctx, c.X, cat, 0.1, c.y, Zd, 0.0, 5)
    assert rc == 2 and all_nan(outs) and np.all(np.isnan(dz))
    assert same(ref, run(ctx, c))                       # the next call on the same context is correct


def test_central_differences_of_the_device_bound(ctx):
    # N = 700, Mz = 127, no OU term (a step would cross its kinks), h = 1e-5: h^2 f''' / 6 of
    # truncation and ~10 eps |elbo| / h of rounding, the bar of test_gpu_sparse_grad.py's mcmc test
    c = case(700, 127, 1e-6, NO_OU)
    got = check(ctx, c)
    h = 1e-5
    for m, d in ((0, 0), (63, 0), (126, 2)):
        e = np.zeros(c.Z.shape)
        e[m, d] = h
        fd = (ctx.sparse_elbo(c.X, NO_OU, 0.1, c.y, c.Z + e, 1e-6) - ctx.sparse_elbo(c.X, NO_OU, 0.1, c.y, c.Z - e, 1e-6)) / (2 * h)
        bar = 1e-6 * max(1.0, abs(fd)) + 10 * 2.2e-16 * abs(got[0]) / h
        print("dZ", (m, d), got[5][m, d], fd, abs(got[5][m, d] - fd), "bar", bar)
        assert abs(got[5][m, d] - fd) <= bar


def test_abstractgps_surface(ctx, monkeypatch):
    rng = np.random.default_rng(13)
    x = rng.uniform(-5, 5, 400)
    y = np.sin(x) + 0.3 * rng.normal(size=400)
    z = np.linspace(-5, 5, 12)
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))
    fx, vfe = gp(x, 0.1), AG.VFE(gp(z, 1e-6))
    a = AG.elbo_and_gradient(vfe, fx, y, ctx=ctx, wrt_inducing=True)
    assert len(a) == 6 and a[5].shape == (12, 1)        # (a 1-D z is one column)
    assert same(a, ctx.sparse_elbo_grad(x, fx.terms, 0.1, y, z, 1e-6, wrt_z=True))
    assert len(AG.elbo_and_gradient(vfe, fx, y, ctx=ctx)) == 5
    monkeypatch.setenv("GAPLAC_HIP", "0")
    with pytest.raises(AG.BackendDisabled):
        AG.elbo_and_gradient(vfe, fx, y, ctx=ctx, wrt_inducing=True)


def test_fit_inducing_climbs_the_bound(ctx):
    rng = np.random.default_rng(400)
    x = np.sort(rng.uniform(0, 10, 400))
    y = np.sin(x) + 0.3 * rng.normal(size=400)
    Z0 = np.linspace(0.1, 0.9, 8)                       # bunched in the left tenth of the range
    Z, elbo, history = vfe_fit.fit_inducing(ctx, x, [(SQEXP, 0, 1.0, 0)], 0.1, y, Z0, jitter=1e-6, maxiter=30)
    print("bound", history[0], "->", elbo, "in", len(history) - 1, "steps; Z", np.sort(Z[:, 0]))
    assert Z.shape == (8, 1) and elbo > history[0]
    assert all(b >= a for a, b in zip(history, history[1:]))
