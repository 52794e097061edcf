"""The device-resident entries (gaplac_logpdf_device, gaplac_logpdf_grad_device,
gaplac_logpdf_multi_device: the three the benchmark times) on torch tensors: bitwise the results of
their host twins, within the suite's 1e-9 of the oracle, for leading dimensions beyond N, a base
pointer that is only 8-byte aligned, NaN in every padding row, inputs left unchanged, and a
non-positive-definite model that leaves NaN outputs and a usable context.
"""
from ctypes import byref, c_double, c_void_p

import numpy as np
import pytest

from gaplac_amd._native import CAT, NOISE, OU, SQEXP, term_array
from gaplac_amd.backend import Context, PosDefException
from oracle import restatement as R
from tests.conftest import gpu_available
from tests.test_gpu_multi import check_against_oracle, oracle_multi

pytestmark = pytest.mark.gpu
TOL = 1e-9
COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (NOISE, -1, 1.0, 3)]
_refs = {}


@pytest.fixture(scope="module")
def ctx():
    if not gpu_available():
        pytest.skip("no GPU")
    c = Context(0)
    yield c
    c.close()


def inputs(N, Rn=1):
    rng = np.random.default_rng(1000 * N + Rn)
    X = np.column_stack([rng.uniform(0, 10, N), rng.integers(0, max(1, N // 4), N).astype(float)])
    return X, rng.standard_normal((N, Rn))


class DeviceMatrix:
    """A column-major matrix with leading dimension ld in a NaN-filled device buffer, starting
    `offset` doubles into the allocation (offset 1: the matrix is only 8-byte aligned)."""

    def __init__(self, M, ld, offset):
        import torch
        rows, ncol = M.shape
        assert ld >= rows
        self.buf = torch.full((offset + ld * ncol + 2,), float("nan"), dtype=torch.float64, device="cuda")
        for c in range(ncol):
            a = offset + c * ld
            self.buf[a:a + rows] = torch.from_numpy(np.ascontiguousarray(M[:, c]))
        torch.cuda.synchronize()
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + 8 * offset
        assert self.ptr % 16 == (8 if offset % 2 else 0)
        self.ld = ld

    def unchanged(self):
        import torch
        torch.cuda.synchronize()
        return torch.equal(self.buf.view(torch.int64), self.before.view(torch.int64))


def oracle_single(N):
    if ("s", N) not in _refs:
        X, Y = inputs(N)
        _refs["s", N] = (R.logpdf(X, COMPOSITE, 0.1, Y[:, 0]), R.logpdf_grad(X, COMPOSITE, 0.1, Y[:, 0]),
                         R.logpdf_grad_scale(X, COMPOSITE, 0.1, Y[:, 0]))
    return _refs["s", N]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("N", [1, 129, 700])
def test_logpdf_device(ctx, N, pad, offset):
    X, Y = inputs(N)
    v = Y[:, 0]
    dX, dv = DeviceMatrix(X, N + pad, offset), DeviceMatrix(Y, N, offset)
    got = ctx.logpdf_device(N, 2, dX.ptr, dX.ld, COMPOSITE, 0.1, dv.ptr, full=True)
    assert got == ctx.logpdf(X, COMPOSITE, 0.1, v, full=True)
    rl, rd, rq = oracle_single(N)[0]
    assert abs(got[0] - rl) <= TOL * abs(rl) and abs(got[1] - rd) <= TOL * abs(rl) and abs(got[2] - rq) <= TOL * abs(rl)
    assert dX.unchanged() and dv.unchanged()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("N", [1, 129, 700])
def test_logpdf_grad_device(ctx, N, pad, offset):
    X, Y = inputs(N)
    v = Y[:, 0]
    dX, dv = DeviceMatrix(X, N + pad, offset), DeviceMatrix(Y, N, offset)
    lp, gv, gp, gn = ctx.logpdf_grad_device(N, 2, dX.ptr, dX.ld, COMPOSITE, 0.1, dv.ptr)
    hl, hv, hp, hn = ctx.logpdf_grad(X, COMPOSITE, 0.1, v)
    assert lp == hl and np.array_equal(gv, hv) and np.array_equal(gp, hp) and gn == hn
    lp2, none, gp2, gn2 = ctx.logpdf_grad_device(N, 2, dX.ptr, dX.ld, COMPOSITE, 0.1, dv.ptr, want_dv=False)
    assert none is None and lp2 == hl and np.array_equal(gp2, hp) and gn2 == hn
    _, (rl, rdv, rdp, rdn), (scale, scalen) = oracle_single(N)
    assert abs(lp - rl) <= TOL * abs(rl)
    assert np.max(np.abs(gv - rdv)) <= TOL * max(1.0, np.max(np.abs(rdv)))
    assert np.all(np.abs(gp - rdp) <= TOL * (np.abs(rdp) + scale))
    assert abs(gn - rdn) <= TOL * (abs(rdn) + scalen)
    assert dX.unchanged() and dv.unchanged()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("padx,pady", [(0, 0), (3, 5), (0, 5)])
@pytest.mark.parametrize("N,Rn", [(129, 1), (300, 130)])
def test_logpdf_multi_device(ctx, N, Rn, padx, pady, offset):
    """dY is read in place with the caller's ldy (the host twin always packs a copy with ld = N)."""
    X, Y = inputs(N, Rn)
    dX, dY = DeviceMatrix(X, N + padx, offset), DeviceMatrix(Y, N + pady, offset)
    lp, ld, q = ctx.logpdf_multi_device(N, 2, dX.ptr, dX.ld, COMPOSITE, 0.1, Rn, dY.ptr, dY.ld, full=True)
    hl, hd, hq = ctx.logpdf_multi(X, COMPOSITE, 0.1, Y, full=True)
    assert np.array_equal(lp, hl) and ld == hd and np.array_equal(q, hq)
    if ("m", N, Rn) not in _refs:
        _refs["m", N, Rn] = oracle_multi(X, COMPOSITE, 0.1, Y)
    check_against_oracle(lp, ld, q, _refs["m", N, Rn])
    assert dX.unchanged() and dY.unchanged()


def test_non_positive_definite_model_leaves_nan_and_a_usable_context(ctx):
    N = 32
    X = np.repeat(np.arange(8.0), 4)[:, None]                     # equal categories, no noise: singular
    Y = np.ones((N, 3))
    terms = [(CAT, 0, 0.0, 0)]
    dX, dY = DeviceMatrix(X, N + 3, 1), DeviceMatrix(Y, N + 5, 1)
    with pytest.raises(PosDefException) as e:
        ctx.logpdf(X, terms, 0.0, Y[:, 0])
    for call in (lambda: ctx.logpdf_device(N, 1, dX.ptr, dX.ld, terms, 0.0, dY.ptr),
                 lambda: ctx.logpdf_grad_device(N, 1, dX.ptr, dX.ld, terms, 0.0, dY.ptr),
                 lambda: ctx.logpdf_multi_device(N, 1, dX.ptr, dX.ld, terms, 0.0, 3, dY.ptr, dY.ld)):
        with pytest.raises(PosDefException) as ed:
            call()
        assert ed.value.info == e.value.info
    head = (ctx.h, N, 1, c_void_p(dX.ptr), dX.ld, 1, term_array(terms), 0.0)
    a, b, c = c_double(0.0), c_double(0.0), c_double(0.0)
    rc = ctx.lib.gaplac_logpdf_device(*head, c_void_p(dY.ptr), byref(a), byref(b), byref(c))
    assert rc == e.value.info and np.isnan(a.value) and np.isnan(b.value) and np.isnan(c.value)
    a, dn, gv, gp = c_double(0.0), c_double(0.0), np.zeros(N), np.zeros(1)
    rc = ctx.lib.gaplac_logpdf_grad_device(*head, c_void_p(dY.ptr), byref(a), gv.ctypes.data_as(c_void_p),
                                           gp.ctypes.data_as(c_void_p), byref(dn))
    assert rc == e.value.info and np.isnan(a.value) and np.isnan(dn.value) and np.all(np.isnan(gv)) and np.all(np.isnan(gp))
    lp, q, ld = np.zeros(3), np.zeros(3), c_double(0.0)
    rc = ctx.lib.gaplac_logpdf_multi_device(*head, 3, c_void_p(dY.ptr), dY.ld, lp.ctypes.data_as(c_void_p), byref(ld),
                                            q.ctypes.data_as(c_void_p))
    assert rc == e.value.info and np.all(np.isnan(lp)) and np.all(np.isnan(q)) and np.isnan(ld.value)
    assert dX.unchanged() and dY.unchanged()
    # the context stays usable, on the same device buffers
    ok = [(CAT, 0, 0.0, 0), (NOISE, -1, 0.5, 1)]
    assert ctx.logpdf_device(N, 1, dX.ptr, dX.ld, ok, 0.0, dY.ptr) == ctx.logpdf(X, ok, 0.0, Y[:, 0])
    assert np.array_equal(ctx.logpdf_multi_device(N, 1, dX.ptr, dX.ld, ok, 0.0, 3, dY.ptr, dY.ld),
                          ctx.logpdf_multi(X, ok, 0.0, Y))
