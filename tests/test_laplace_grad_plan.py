"""gaplac_laplace_logpdf_grad on the CPU, no device: the exported symbols and the dry walk of
gaplac_plan_check_laplace_grad (one Newton step with a trial point, the final factorisation with
identity rows, the gradient's stages and ending) against the workspace and the vectors' buffer, with
both negative controls (either one element short).
"""
import ctypes

import pytest

from gaplac_amd import _native

SYMBOLS = ("gaplac_laplace_logpdf_grad", "gaplac_plan_check_laplace_grad")
SIZES = [1, 127, 128, 129, 300, 1000, 2049, 3400]


def plan(N, spw=4, short_ws=0):
    lib = _native.load()
    launches, violations = ctypes.c_int64(), ctypes.c_int64()
    msg = ctypes.create_string_buffer(256)
    rc = lib.gaplac_plan_check_laplace_grad(N, spw, short_ws, ctypes.byref(launches), ctypes.byref(violations), msg, 256)
    return rc, launches.value, violations.value, msg.value.decode()


def test_the_symbols_are_exported():
    lib = _native.load()
    for name in SYMBOLS:
        assert name in _native.EXPORTED
        assert hasattr(lib, name)


@pytest.mark.parametrize("spw", [1, 4])
@pytest.mark.parametrize("N", SIZES)
def test_every_launch_stays_inside_its_allocation(N, spw):
    rc, launches, violations, msg = plan(N, spw)
    assert rc == 0 and violations == 0, msg
    # more launches than the value's walk at the same size: the gradient's stages are walked
    lib = _native.load()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    assert lib.gaplac_plan_check_laplace(N, 0, spw, 0, ctypes.byref(a), ctypes.byref(b), None, 0) == 0
    assert launches > a.value


@pytest.mark.parametrize("N", SIZES)
def test_a_workspace_one_element_short_is_reported(N):
    rc, _, violations, msg = plan(N, short_ws=1)
    assert rc == 0 and violations >= 1
    assert "workspace" in msg


@pytest.mark.parametrize("N", SIZES)
def test_a_vector_buffer_one_element_short_is_reported(N):
    rc, _, violations, msg = plan(N, short_ws=2)
    assert rc == 0 and violations >= 1
    assert "laplace_grad" in msg  # the gradient's own launch reports it: its vectors lie last


def test_argument_errors():
    assert plan(0)[0] == _native.E_ARG
    assert plan(10, spw=0)[0] == _native.E_ARG
    assert plan(10, spw=9)[0] == _native.E_ARG
    assert plan(10, short_ws=3)[0] == _native.E_ARG
