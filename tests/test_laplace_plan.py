"""The Laplace entries on the CPU, no device: the exported symbols and the dry walk of
gaplac_plan_check_laplace (one Newton step with a trial point, the final factorisation, one
posterior query of M points in its chunks) against the workspace and the vectors' buffer, with its
negative control (both one element short).
"""
import ctypes

import pytest

from gaplac_amd import _native

SYMBOLS = ("gaplac_laplace_logpdf", "gaplac_laplace_posterior_mean_var", "gaplac_plan_check_laplace")
EDGES = [127, 128, 129, 255, 256, 257, 1000, 4096, 10239, 10240, 16384]  # the padding edges and beyond
MS = [0, 1, 128, 129, 1000, 4096, 4097, 9000]


def plan(N, M, spw=4, short_ws=0):
    lib = _native.load()
    launches, violations = ctypes.c_int64(), ctypes.c_int64()
    msg = ctypes.create_string_buffer(256)
    rc = lib.gaplac_plan_check_laplace(N, M, spw, short_ws, ctypes.byref(launches), ctypes.byref(violations), msg, 256)
    return rc, launches.value, violations.value, msg.value.decode()


def test_the_symbols_are_exported():
    lib = _native.load()
    for name in SYMBOLS:
        assert name in _native.EXPORTED
        assert hasattr(lib, name)


@pytest.mark.parametrize("spw", range(1, 9))
def test_every_launch_inside_for_n_1_to_300(spw):
    for N in range(1, 301):
        for M in (0, 3) if N % 16 else (0, 1, 129):
            rc, launches, violations, msg = plan(N, M, spw)
            assert rc == 0, (N, M, spw, rc, msg)
            assert launches > 0
            assert violations == 0, (N, M, spw, msg)


@pytest.mark.parametrize("spw", [1, 4, 8])
@pytest.mark.parametrize("N", EDGES)
def test_every_launch_inside_at_the_padding_edges(N, spw):
    for M in MS:
        rc, launches, violations, msg = plan(N, M, spw)
        assert (rc, violations) == (0, 0), (N, M, spw, msg)
        assert launches > 0


@pytest.mark.parametrize("N", [1, 5, 127, 128, 129, 300, 1000, 4096])
def test_buffers_one_element_short_are_reported(N):
    for M in (0, 1, 129, 4097):
        for spw in (1, 4, 8):
            rc, launches, violations, msg = plan(N, M, spw, short_ws=1)
            assert rc == 0, (N, M, rc, msg)
            assert violations >= 1, (N, M, spw)
            assert "workspace" in msg


def test_a_posterior_query_walks_more_launches_per_chunk():
    counts = [plan(1000, M)[1] for M in (0, 1, 4097, 8193)]
    assert 0 < counts[0] < counts[1] < counts[2] < counts[3]


def test_bad_arguments():
    assert plan(0, 1)[0] == _native.E_ARG
    assert plan(5, -1)[0] == _native.E_ARG
    assert plan(5, 1, spw=0)[0] == _native.E_ARG
    assert plan(5, 1, spw=9)[0] == _native.E_ARG
    assert plan(5, 1, short_ws=2)[0] == _native.E_ARG


def test_null_context_without_a_device():
    lib = _native.load()
    q = ctypes.c_double()
    it, cv, info = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    rc = lib.gaplac_laplace_logpdf(None, 0, 0, None, 0, 0, None, 0.0, 1, 0.0, None, 10, 1e-12, None, ctypes.byref(q),
                                   None, None, ctypes.byref(it), ctypes.byref(cv), ctypes.byref(info))
    assert rc == _native.E_ARG
    assert q.value != q.value  # NaN-filled first
