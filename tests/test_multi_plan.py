"""The matrix forms (gaplac_logpdf_multi / _device, gaplac_rand_multi) on the CPU: the dry
walk of the logpdf_multi schedule (gaplac_plan_check mode 3: the R responses as dense extra
rows, M = R; mode 11 = the same walk against a workspace one element short), the backend
switch in front of the new front-end forms, and the three exported symbols.
"""
import ctypes

import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd import formula as F
from tests.test_plan_guard import SIZES

RS = [1, 127, 128, 129, 1000, 6144, 6145]


def plan(N, mode, M, spw=4):
    lib = _native.load()
    launches, violations = ctypes.c_int64(), ctypes.c_int64()
    msg = ctypes.create_string_buffer(256)
    rc = lib.gaplac_plan_check(N, mode, M, spw, ctypes.byref(launches), ctypes.byref(violations), msg, 256)
    return rc, launches.value, violations.value, msg.value.decode()


@pytest.mark.parametrize("spw", [1, 4, 8])
@pytest.mark.parametrize("R", RS)
def test_every_launch_of_logpdf_multi_inside_the_workspace(R, spw):
    for N in SIZES:
        rc, launches, violations, msg = plan(N, 3, R, spw)
        assert rc == 0, (N, R, spw, rc, msg)
        assert launches > 0
        assert violations == 0, (N, R, spw, msg)


def test_rows_leave_the_tail_at_49_tile_rows():
    # N = 16384: R <= 48 * 128 rides in the persistent tail beside its 80 columns; one more
    # response makes 49 tile rows, every column a super-panel with its extra-row launches
    _, l0, v0, _ = plan(16384, 0, 0)
    _, l1, v1, _ = plan(16384, 3, 6144)
    _, l2, v2, _ = plan(16384, 3, 6145)
    assert v0 == v1 == v2 == 0
    assert l0 < l1 < l2


def test_the_dry_walk_covers_the_new_launches():
    # against the posterior's walk of the same rows: the transposing launch stands where the
    # cross-covariance launch stood, the partial / finish pair where the posterior's pair stood
    for N, R in ((300, 130), (4096, 1000), (16384, 1024)):
        _, lp, _, _ = plan(N, 2, R)
        _, lm, _, _ = plan(N, 3, R)
        assert lm == lp, (N, R, lp, lm)


@pytest.mark.parametrize("N", [1, 128, 300, 4096])
def test_negative_control_short_workspace_is_reported(N):
    rc, launches, violations, msg = plan(N, 11, 64)
    assert rc == 0
    assert violations >= 1
    assert "touches elements" in msg


def test_mode_3_needs_rows():
    assert plan(10, 3, 0)[0] == _native.E_ARG
    assert plan(10, 11, 0)[0] == _native.E_ARG
    assert plan(10, 4, 1)[0] == _native.E_ARG


def test_switch_gates_the_matrix_forms(monkeypatch):
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))
    fx = AG.FiniteGP(gp, np.linspace(0, 1, 8)[:, None], 0.1)
    monkeypatch.setenv("GAPLAC_HIP", "0")
    with pytest.raises(AG.BackendDisabled):
        AG.logpdf(fx, np.zeros((8, 3)))
    with pytest.raises(AG.BackendDisabled):
        AG.rand(fx, n=3)
    with pytest.raises(AG.BackendDisabled):
        AG.rand(fx, z=np.zeros((8, 2)))
    with pytest.raises(AG.BackendDisabled):
        AG.select_formulae("y ~| SqExp(:x; l=1)", "y ~| OU(:x; l=1)", {"x": [0.0], "y": [0.0]}, responses=["y"])


def test_the_three_symbols_are_exported():
    lib = _native.load()
    for name in ("gaplac_logpdf_multi", "gaplac_logpdf_multi_device", "gaplac_rand_multi"):
        assert name in _native.EXPORTED
        assert hasattr(lib, name)
    assert lib.gaplac_abi_version() == 1
