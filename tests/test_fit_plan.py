"""The fitted posterior on the CPU, no device: the exported symbols and the dry walk of a fit
(gaplac_plan_check_fit: the create-time tile copy, z and the back-substitution, one
mean-and-variance query of M points in chunks of cap, one matrix-free mean query) against the
fit's buffer, with its negative control (the buffer one element short).
"""
import ctypes

import pytest

from gaplac_amd import _native

SYMBOLS = ("gaplac_fit_create", "gaplac_fit_destroy", "gaplac_fit_info", "gaplac_fit_alpha", "gaplac_fit_mean",
           "gaplac_fit_mean_var", "gaplac_plan_check_fit")
NS = [1, 127, 128, 129, 1000, 4096, 10239, 10240, 16384]
CAPS = [1, 128, 129, 1024]


def queries(cap):
    return [1, cap, cap + 1, 5 * cap + 3]


def plan(N, cap, M, spw=4, short_ws=0):
    lib = _native.load()
    launches, violations = ctypes.c_int64(), ctypes.c_int64()
    msg = ctypes.create_string_buffer(256)
    rc = lib.gaplac_plan_check_fit(N, cap, M, spw, short_ws, ctypes.byref(launches), ctypes.byref(violations), msg, 256)
    return rc, launches.value, violations.value, msg.value.decode()


def test_the_symbols_are_exported():
    lib = _native.load()
    for name in SYMBOLS:
        assert name in _native.EXPORTED
        assert hasattr(lib, name)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("N", NS)
def test_every_launch_of_a_fit_inside_its_buffer(N, cap):
    for M in queries(cap):
        rc, launches, violations, msg = plan(N, cap, M)
        assert rc == 0, (N, cap, M, rc, msg)
        assert launches > 0
        assert violations == 0, (N, cap, M, msg)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("N", NS)
def test_a_buffer_one_element_short_is_reported(N, cap):
    for M in queries(cap):
        rc, launches, violations, msg = plan(N, cap, M, short_ws=1)
        assert rc == 0, (N, cap, M, rc, msg)
        assert violations >= 1, (N, cap, M)
        assert "workspace" in msg


def test_other_super_panel_widths_and_the_query_chunks():
    for spw in (1, 2, 8):
        for N, cap, M in ((129, 1, 3), (1000, 129, 300), (4096, 128, 643)):
            rc, launches, violations, msg = plan(N, cap, M, spw)
            assert (rc, violations) == (0, 0), (N, cap, M, spw, msg)
    # a query in more chunks walks more launches; M = 0 walks the create-time launches alone
    counts = [plan(1000, 128, M)[1] for M in (0, 128, 129, 643)]
    assert 0 < counts[0] < counts[1] < counts[2] < counts[3]


def test_bad_arguments():
    for args in ((0, 1, 1), (5, 0, 1), (5, 1, -1)):
        assert plan(*args)[0] == _native.E_ARG
    assert plan(5, 1, 1, spw=0)[0] == _native.E_ARG
    assert plan(5, 1, 1, spw=9)[0] == _native.E_ARG
    assert plan(5, 1, 1, short_ws=2)[0] == _native.E_ARG


def test_null_handles_without_a_device():
    lib = _native.load()
    assert lib.gaplac_fit_destroy(None) == 0
    assert lib.gaplac_fit_info(None, None, None, None, None, None) == _native.E_ARG
    assert lib.gaplac_fit_alpha(None, None) == _native.E_ARG
    assert lib.gaplac_fit_mean(None, 0, None, 0, None) == _native.E_ARG
    assert lib.gaplac_fit_mean_var(None, 0, None, 0, None, None) == _native.E_ARG
    h = ctypes.c_void_p()
    assert lib.gaplac_fit_create(None, 0, 0, None, 0, 0, None, 0.0, None, 1, ctypes.byref(h)) == _native.E_ARG
    assert not h.value
