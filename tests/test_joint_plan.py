"""The joint posterior entries (gaplac_posterior_mean_cov / _rand / _logpdf) on the CPU: the
exported symbols, the dry walk of their three stages (gaplac_plan_check_joint: the posterior
evaluation, the covariance launches against both workspaces, the preloaded factorisation of
order M, with R riding rows when R > 0) with its two negative controls, and the backend switch
in front of the new front-end forms.
"""
import ctypes

import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd import formula as F
from tests.test_plan_guard import SIZES

MS = [1, 127, 128, 129, 1000, 10300]
SYMBOLS = ("gaplac_posterior_mean_cov", "gaplac_posterior_rand", "gaplac_posterior_logpdf", "gaplac_plan_check_joint")


def plan(N, M, R, spw=4, short_ws=0):
    lib = _native.load()
    launches, violations = ctypes.c_int64(), ctypes.c_int64()
    msg = ctypes.create_string_buffer(256)
    rc = lib.gaplac_plan_check_joint(N, M, R, spw, short_ws, ctypes.byref(launches), ctypes.byref(violations), msg, 256)
    return rc, launches.value, violations.value, msg.value.decode()


def test_the_four_symbols_are_exported():
    lib = _native.load()
    for name in SYMBOLS:
        assert name in _native.EXPORTED
        assert hasattr(lib, name)
    assert lib.gaplac_abi_version() == 1


@pytest.mark.parametrize("spw", [1, 4, 8])
@pytest.mark.parametrize("R", [0, 1, 130])
@pytest.mark.parametrize("M", MS)
def test_every_launch_of_the_three_stages_inside_its_workspace(M, R, spw):
    for N in SIZES:
        rc, launches, violations, msg = plan(N, M, R, spw)
        assert rc == 0, (N, M, R, spw, rc, msg)
        assert launches > 0
        assert violations == 0, (N, M, R, spw, msg)


def test_the_walk_covers_all_three_stages():
    # more launches than the posterior evaluation alone, and the riding rows add their own
    lib = _native.load()
    l1, v1 = ctypes.c_int64(), ctypes.c_int64()
    for N, M in ((300, 130), (4096, 1000), (16384, 1024)):
        assert lib.gaplac_plan_check(N, 2, M, 4, ctypes.byref(l1), ctypes.byref(v1), None, 0) == 0
        _, l0, _, _ = plan(N, M, 0)
        _, lr, _, _ = plan(N, M, 130)
        assert l1.value + 3 <= l0 < lr, (N, M, l1.value, l0, lr)


@pytest.mark.parametrize("short_ws", [1, 2])
@pytest.mark.parametrize("N,M,R", [(1, 1, 0), (128, 128, 0), (300, 1000, 0), (300, 1000, 5), (4096, 129, 130),
                                   (300, 10300, 2)])
def test_negative_controls_report_the_short_workspace(N, M, R, short_ws):
    rc, launches, violations, msg = plan(N, M, R, 4, short_ws)
    assert rc == 0
    assert violations >= 1
    assert "touches elements" in msg


def test_bad_arguments():
    for a in ((0, 1, 0), (10, 0, 0), (10, 1, -1), (10, 1, 0, 0), (10, 1, 0, 9), (10, 1, 0, 4, 3), (10, 1, 0, 4, -1)):
        assert plan(*a)[0] == _native.E_ARG, a


def test_switch_gates_the_joint_forms(monkeypatch):
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))
    fx = AG.FiniteGP(gp, np.linspace(0, 1, 8)[:, None], 0.1)
    fpx = AG.posterior(fx, np.zeros(8))(np.linspace(0, 1, 5), 0.1)
    assert len(fpx) == 5
    monkeypatch.setenv("GAPLAC_HIP", "0")
    with pytest.raises(AG.BackendDisabled):
        AG.mean_and_cov(fpx)
    with pytest.raises(AG.BackendDisabled):
        AG.cov(fpx)
    with pytest.raises(AG.BackendDisabled):
        AG.rand(fpx, n=3)
    with pytest.raises(AG.BackendDisabled):
        AG.rand(fpx, z=np.zeros(5))
    with pytest.raises(AG.BackendDisabled):
        AG.logpdf(fpx, np.zeros(5))
    with pytest.raises(AG.BackendDisabled):
        AG.logpdf(fpx, np.zeros((5, 2)))
