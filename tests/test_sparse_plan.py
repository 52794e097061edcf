"""The sparse (inducing-point) entries on the CPU, no device: the exported symbols, the dry walk
of their three stages (gaplac_plan_check_sparse: the posterior evaluation of order Mz with
N + Ms riding rows, the launches that form S, the preloaded factorisation of order Mz with the
Ms rows riding when Ms > 0) with its two negative controls, the split rule, and the backend
switch in front of the new front-end forms.
"""
import ctypes

import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd import formula as F

SYMBOLS = ("gaplac_sparse_elbo", "gaplac_sparse_posterior_mean_var", "gaplac_sparse_split", "gaplac_plan_check_sparse")
NS = [1, 5, 127, 128, 129, 300, 513, 1023, 1024, 1025, 2051, 16384, 70000]
MZS = [1, 5, 127, 128, 129, 257, 513, 1024, 4096]
MSS = [0, 1, 3, 128, 129, 1000]


def plan(N, Mz, Ms, spw=4, short_ws=0):
    lib = _native.load()
    launches, violations = ctypes.c_int64(), ctypes.c_int64()
    msg = ctypes.create_string_buffer(256)
    rc = lib.gaplac_plan_check_sparse(N, Mz, Ms, spw, short_ws, ctypes.byref(launches), ctypes.byref(violations),
                                      msg, 256)
    return rc, launches.value, violations.value, msg.value.decode()


def split(N, Mz):
    lib = _native.load()
    chunks, rows = ctypes.c_int64(), ctypes.c_int64()
    assert lib.gaplac_sparse_split(N, Mz, ctypes.byref(chunks), ctypes.byref(rows)) == 0
    return chunks.value, rows.value


def test_the_four_symbols_are_exported():
    lib = _native.load()
    for name in SYMBOLS:
        assert name in _native.EXPORTED
        assert hasattr(lib, name)
    assert lib.gaplac_abi_version() == 1


@pytest.mark.parametrize("Ms", MSS)
@pytest.mark.parametrize("Mz", MZS)
def test_every_launch_of_the_three_stages_inside_its_workspace(Mz, Ms):
    for N in NS:
        for spw in ((1, 4, 8) if N <= 1025 else (4,)):
            rc, launches, violations, msg = plan(N, Mz, Ms, spw)
            assert rc == 0, (N, Mz, Ms, spw, rc, msg)
            assert launches > 0
            assert violations == 0, (N, Mz, Ms, spw, msg)


def test_the_walk_covers_all_three_stages():
    lib = _native.load()
    l1, v1 = ctypes.c_int64(), ctypes.c_int64()
    for N, Mz in ((300, 130), (4096, 1000), (16384, 1024)):
        # more launches than the stage-1 posterior evaluation alone, and the riding rows add their own
        assert lib.gaplac_plan_check(Mz, 2, N, 4, ctypes.byref(l1), ctypes.byref(v1), None, 0) == 0
        _, l0, _, _ = plan(N, Mz, 0)
        _, lr, _, _ = plan(N, Mz, 130)
        assert l1.value + 3 <= l0 < lr, (N, Mz, l1.value, l0, lr)


@pytest.mark.parametrize("short_ws", [1, 2])
@pytest.mark.parametrize("N,Mz,Ms", [(1, 1, 0), (1, 1, 1), (128, 128, 0), (300, 1000, 0), (1000, 300, 5),
                                     (4096, 129, 130), (2051, 5, 2)])
def test_negative_controls_report_the_short_workspace(N, Mz, Ms, short_ws):
    rc, launches, violations, msg = plan(N, Mz, Ms, 4, short_ws)
    assert rc == 0
    assert violations >= 1
    assert "touches elements" in msg


def test_bad_arguments():
    for a in ((0, 1, 0), (10, 0, 0), (10, 1, -1), (10, 1, 0, 0), (10, 1, 0, 9), (10, 1, 0, 4, 3), (10, 1, 0, 4, -1),
              (65535 * 128 + 1, 1, 0)):
        assert plan(*a)[0] == _native.E_ARG, a


@pytest.mark.parametrize("Mz", [0, 1, 5, 129, 1024, 4096])
def test_split_rule(Mz):
    lib = _native.load()
    ntb = (Mz + 128) // 128
    ntl = ntb * (ntb + 1) // 2
    for N in (0, 1, 1023, 1024, 1025, 2051, 16384, 65536, 262144, 1 << 20, 8_000_000):
        chunks, rows = split(N, Mz)
        assert (chunks, rows) == split(N, Mz)           # the same on every call
        assert rows >= 1024 and rows % 1024 == 0
        assert chunks == -(-N // rows)                  # whole chunks, the last one ragged
        assert chunks * ntl <= 8192                     # at most 1 GiB of partial tiles
    # short chunks at small Mz: two chunks and a ragged last one are reachable at N ~ 2000
    assert split(2051, 5) == (3, 1024) and split(2051, 129) == (3, 1024)
    one = ctypes.c_int64()
    assert lib.gaplac_sparse_split(-1, 1, ctypes.byref(one), ctypes.byref(one)) == _native.E_ARG
    assert lib.gaplac_sparse_split(1, -1, ctypes.byref(one), ctypes.byref(one)) == _native.E_ARG
    assert lib.gaplac_sparse_split(1, 1, None, ctypes.byref(one)) == _native.E_ARG


def test_switch_gates_the_sparse_forms(monkeypatch):
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))
    fx = AG.FiniteGP(gp, np.linspace(0, 1, 8)[:, None], 0.1)
    vfe = AG.VFE(gp(np.linspace(0, 1, 3), 1e-6))
    post = AG.posterior(vfe, fx, np.zeros(8))
    assert isinstance(post, AG.ApproxPosteriorGP)
    assert isinstance(AG.posterior(fx, np.zeros(8)), AG.PosteriorGP)  # the exact form goes where it went
    with pytest.raises(F.ArgumentError):
        AG.posterior(vfe, fx, np.zeros(7))
    monkeypatch.setenv("GAPLAC_HIP", "0")
    with pytest.raises(AG.BackendDisabled):
        AG.elbo(vfe, fx, np.zeros(8))
    with pytest.raises(AG.BackendDisabled):
        AG.dtc(vfe, fx, np.zeros(8))
    with pytest.raises(AG.BackendDisabled):
        AG.mean_and_var(post, np.linspace(0, 1, 5))
