"""gaplac_sparse_elbo_grad on the CPU, no device: the exported symbols, the dry walk of its
launches (gaplac_plan_check_sparse_grad: the value's three stages, the order-Mz launches against
the gradient's scratch, alpha and the product kernel against the first workspace and the scratch)
with both negative controls, the backend switch in front of elbo_and_gradient, and the mcmc
model's host logic with inducing inputs.
"""
import ctypes

import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd import formula as F
from gaplac_amd import mcmc as M

SHAPES = [(1, 1), (5, 129), (127, 128), (129, 127), (300, 5), (700, 127), (1000, 129), (513, 513), (2000, 257),
          (262144, 4096)]


def plan(N, Mz, spw=4, short_ws=0):
    lib = _native.load()
    launches, violations = ctypes.c_int64(), ctypes.c_int64()
    msg = ctypes.create_string_buffer(256)
    rc = lib.gaplac_plan_check_sparse_grad(N, Mz, spw, short_ws, ctypes.byref(launches), ctypes.byref(violations),
                                           msg, 256)
    return rc, launches.value, violations.value, msg.value.decode()


def value_plan(N, Mz, spw=4, short_ws=0):
    lib = _native.load()
    launches, violations = ctypes.c_int64(), ctypes.c_int64()
    rc = lib.gaplac_plan_check_sparse(N, Mz, 0, spw, short_ws, ctypes.byref(launches), ctypes.byref(violations), None, 0)
    return rc, launches.value, violations.value


def test_the_two_symbols_are_exported():
    lib = _native.load()
    for name in ("gaplac_sparse_elbo_grad", "gaplac_plan_check_sparse_grad"):
        assert name in _native.EXPORTED
        assert hasattr(lib, name)


@pytest.mark.parametrize("N,Mz", SHAPES)
def test_every_launch_inside_its_workspace(N, Mz):
    for spw in ((1, 4, 8) if N <= 2000 else (4,)):
        rc, launches, violations, msg = plan(N, Mz, spw)
        assert rc == 0, (N, Mz, spw, rc, msg)
        assert violations == 0, (N, Mz, spw, msg)
        # the value's walk, then per tile column of the two factors a substitution (and from the
        # second on an update), and the fixed launches behind them
        nt = (Mz + 128) // 128
        _, l0, _ = value_plan(N, Mz, spw)
        assert launches >= l0 + 2 * (2 * nt - 1) + 10, (N, Mz, launches, l0)


@pytest.mark.parametrize("short_ws", [1, 2])
@pytest.mark.parametrize("N,Mz", [(1, 1), (128, 128), (300, 1000), (1000, 300), (2051, 5), (262144, 4096)])
def test_negative_controls_report_the_short_workspace(N, Mz, short_ws):
    rc, launches, violations, msg = plan(N, Mz, 4, short_ws)
    assert rc == 0
    # more violations than the value's walk alone: the gradient's own launches leave the short
    # workspace too (1: the product kernel's riding rows; 2: the scratch's last storage)
    _, _, v0 = value_plan(N, Mz, 4, short_ws)
    assert v0 >= 1 and violations >= v0 + 1, (violations, v0)
    assert "touches elements" in msg


def test_bad_arguments():
    for a in ((0, 1), (10, 0), (10, 1, 0), (10, 1, 9), (10, 1, 4, 3), (10, 1, 4, -1), (65535 * 128 + 1, 1)):
        assert plan(*a)[0] == _native.E_ARG, a


def test_switch_gates_elbo_and_gradient(monkeypatch):
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))
    fx = AG.FiniteGP(gp, np.linspace(0, 1, 8)[:, None], 0.1)
    vfe = AG.VFE(gp(np.linspace(0, 1, 3), 1e-6))
    with pytest.raises(F.ArgumentError):
        AG.elbo_and_gradient(vfe, fx, np.zeros(7))
    monkeypatch.setenv("GAPLAC_HIP", "0")
    with pytest.raises(AG.BackendDisabled):
        AG.elbo_and_gradient(vfe, fx, np.zeros(8))


class _RecordingCtx:
    """Stands in for backend.Context (no GPU): fixed results, the calls recorded."""

    def __init__(self):
        self.calls = []

    def sparse_elbo_grad(self, X, terms, noise, y, Z, jitter):
        self.calls.append(("grad", X.copy(), list(terms), noise, np.array(y), Z.copy(), jitter))
        return -10.0, -np.asarray(y) * 0.5, np.arange(1.0, len(terms) + 1.0), 0.25, 0.5

    def sparse_elbo(self, X, terms, noise, y, Z, jitter):
        self.calls.append(("value", jitter))
        return -10.0

    def logpdf_grad(self, X, terms, noise, v):
        self.calls.append(("exact",))
        return -7.0, -np.asarray(v), np.zeros(len(terms)), 0.0


def _table(N=20, seed=3):
    rng = np.random.default_rng(seed)
    return {"y": rng.normal(size=N), "x": rng.uniform(-5, 5, N), "t": rng.uniform(0, 10, N)}


def test_mcmc_model_with_inducing_inputs_calls_the_sparse_entries():
    ctx = _RecordingCtx()
    tab = _table()
    Z = np.column_stack([np.linspace(-5, 5, 4), np.linspace(0, 10, 4), np.linspace(-5, 5, 4)])  # (one column per term)
    m = M.MCMCModel("y ~| SqExp(:x) + OU(:t; l=3) + Linear(:x)", tab, ["x"], ctx=ctx, inducing=Z, jitter=1e-4)
    fx = np.linspace(0, 1, m.N)
    lp, dell, dfx = m.logdensity_and_gradient(2.5, fx)
    kind, X, terms, noise, y, Zc, jitter = ctx.calls[-1]
    assert kind == "grad" and noise == 0.1 and jitter == 1e-4 and np.array_equal(Zc, Z) and np.array_equal(y, fx)
    assert dell == 1.0 + 3.0  # terms 0 and 2 carry ℓ (fake dparam = 1, 2, 3): `tied` is unchanged
    assert np.allclose(dfx, -fx * 0.5 + (tab["y"] - fx))
    assert m.logdensity_and_gradient(1.0, fx)[1] == 3.0  # the l == 1 quirk too
    n = m.memo.calls
    m.logdensity_and_gradient(1.0, fx)
    assert m.memo.calls == n  # the same primal point: answered from the memo
    m.inducing = Z + 1e-3
    m.logdensity_and_gradient(1.0, fx)
    assert m.memo.calls == n + 1  # Z is part of the key
    m.jitter = 1e-3
    m.logdensity_and_gradient(1.0, fx)
    assert m.memo.calls == n + 2  # and jitter
    m.logdensity(1.0, fx)
    assert ctx.calls[-1] == ("value", 1e-3)
    with pytest.raises(F.ArgumentError):
        M.MCMCModel("y ~| SqExp(:x)", tab, ["x"], ctx=ctx, inducing=Z)  # two columns for a one-column design


def test_mcmc_model_without_inducing_inputs_is_unchanged():
    ctx = _RecordingCtx()
    m = M.MCMCModel("y ~| SqExp(:x)", _table(), ["x"], ctx=ctx)
    m.logdensity_and_gradient(2.0, np.zeros(m.N))
    assert ctx.calls == [("exact",)]
