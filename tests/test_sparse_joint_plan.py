"""The sparse joint entries on the CPU, no device: the exported symbols, the dry walk of their
stages (gaplac_plan_check_sparse_joint: gaplac_plan_check_sparse with Ms test points, the copy of
the a rows, the covariance launches with the mirroring pass, the third factorisation of order Ms
with R rows riding when R > 0) against all three workspaces with its three negative controls, and
the backend switch in front of the new front-end forms.
"""
import ctypes

import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd import formula as F
from tests.test_sparse_plan import MZS, NS
from tests.test_sparse_plan import plan as sparse_plan

SYMBOLS = ("gaplac_sparse_posterior_mean_cov", "gaplac_sparse_posterior_rand", "gaplac_sparse_posterior_logpdf",
           "gaplac_plan_check_sparse_joint")
MSS = [1, 3, 128, 129, 1000]
RS = [0, 1, 129]


def plan(N, Mz, Ms, R, spw=4, short_ws=0):
    lib = _native.load()
    launches, violations = ctypes.c_int64(), ctypes.c_int64()
    msg = ctypes.create_string_buffer(256)
    rc = lib.gaplac_plan_check_sparse_joint(N, Mz, Ms, R, spw, short_ws, ctypes.byref(launches),
                                            ctypes.byref(violations), msg, 256)
    return rc, launches.value, violations.value, msg.value.decode()


def test_the_four_symbols_are_exported():
    lib = _native.load()
    for name in SYMBOLS:
        assert name in _native.EXPORTED
        assert hasattr(lib, name)
    assert lib.gaplac_abi_version() == 1


@pytest.mark.parametrize("Ms", MSS)
@pytest.mark.parametrize("Mz", MZS)
def test_every_launch_inside_its_workspace(Mz, Ms):
    for N in NS:
        for spw in ((1, 4, 8) if N <= 1025 else (4,)):
            for R in RS:
                rc, launches, violations, msg = plan(N, Mz, Ms, R, spw)
                assert rc == 0, (N, Mz, Ms, R, spw, rc, msg)
                assert launches > 0
                assert violations == 0, (N, Mz, Ms, R, spw, msg)


def test_the_walk_covers_the_stages_after_the_mean():
    for N, Mz, Ms in ((300, 130, 130), (4096, 1000, 5), (16384, 1024, 1000)):
        _, l0, _, _ = sparse_plan(N, Mz, Ms)
        _, lj, _, _ = plan(N, Mz, Ms, 0)
        _, lr, _, _ = plan(N, Mz, Ms, 129)
        # the copy, the zeroing, the covariance kernel, the mirror, and a factorisation of order Ms
        assert l0 + 5 <= lj < lr, (N, Mz, Ms, l0, lj, lr)


@pytest.mark.parametrize("short_ws", [1, 2, 3])
@pytest.mark.parametrize("N,Mz,Ms,R", [(1, 1, 1, 0), (127, 5, 129, 0), (1000, 300, 5, 3), (128, 128, 128, 1),
                                       (2051, 129, 130, 129), (300, 1000, 1000, 0)])
def test_negative_controls_report_the_short_workspace(N, Mz, Ms, R, short_ws):
    rc, launches, violations, msg = plan(N, Mz, Ms, R, 4, short_ws)
    assert rc == 0
    assert violations >= 1
    assert "touches elements" in msg


def test_bad_arguments():
    for a in ((0, 1, 1, 0), (10, 0, 1, 0), (10, 1, 0, 0), (10, 1, -1, 0), (10, 1, 1, -1), (10, 1, 1, 0, 0),
              (10, 1, 1, 0, 9), (10, 1, 1, 0, 4, 4), (10, 1, 1, 0, 4, -1), (65535 * 128 + 1, 1, 1, 0),
              (10, 1, 1, 65535 * 128 + 1)):
        assert plan(*a)[0] == _native.E_ARG, a


def test_switch_gates_the_joint_sparse_forms(monkeypatch):
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))
    fx = AG.FiniteGP(gp, np.linspace(0, 1, 8)[:, None], 0.1)
    vfe = AG.VFE(gp(np.linspace(0, 1, 3), 1e-6))
    post = AG.posterior(vfe, fx, np.zeros(8))
    fpx = post(np.linspace(0, 1, 5), 0.05)
    assert isinstance(fpx, AG.FinitePosteriorGP) and len(fpx) == 5 and fpx.noise == 0.05
    exact = AG.posterior(fx, np.zeros(8))(np.linspace(0, 1, 5), 0.05)
    assert type(exact) is AG.FinitePosteriorGP              # the exact form goes where it went
    # the shape checks come before any library call
    monkeypatch.setenv("GAPLAC_HIP", "1")
    with pytest.raises(F.ArgumentError):
        AG.logpdf(fpx, np.zeros(4))
    with pytest.raises(F.ArgumentError):
        AG.rand(fpx, z=np.zeros((4, 2)))
    monkeypatch.setenv("GAPLAC_HIP", "0")
    with pytest.raises(AG.BackendDisabled):
        AG.mean_and_cov(fpx)
    with pytest.raises(AG.BackendDisabled):
        AG.cov(fpx)
    with pytest.raises(AG.BackendDisabled):
        AG.rand(fpx, z=np.zeros((5, 2)))
    with pytest.raises(AG.BackendDisabled):
        AG.rand(fpx, rng=np.random.default_rng(0))
    with pytest.raises(AG.BackendDisabled):
        AG.logpdf(fpx, np.zeros(5))
