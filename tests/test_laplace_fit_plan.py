"""The fitted Laplace posterior's host side, no device: the new symbols, the
dry walk of its launches (gaplac_plan_check_laplace_fit) over tile edges, chunk edges and both
negative controls, and the entries' behaviour on NULL handles."""
import ctypes
from ctypes import byref, c_double, c_int32, c_int64, c_void_p

import pytest

from gaplac_amd import _native

NEW = ("gaplac_laplace_fit_create", "gaplac_fit_mode", "gaplac_fit_laplace_info", "gaplac_fit_mean_cov",
       "gaplac_gauss_hermite", "gaplac_laplace_predict", "gaplac_plan_check_laplace_fit")
SIZES = [1, 127, 128, 129, 1000, 4096, 10239, 10240, 16384]
CAPS = [1, 128, 129, 1024]


def walk(N, cap, M, spw=4, short_ws=0):
    lib = _native.load()
    launches, violations = c_int64(-1), c_int64(-1)
    msg = ctypes.create_string_buffer(256)
    rc = lib.gaplac_plan_check_laplace_fit(N, cap, M, spw, short_ws, byref(launches), byref(violations), msg, 256)
    return rc, launches.value, violations.value, msg.value.decode()


def test_new_symbols_are_exported():
    lib = _native.load()
    for name in NEW:
        assert name in _native.EXPORTED and hasattr(lib, name), name


@pytest.mark.parametrize("N", SIZES)
def test_dry_walk_has_no_violation(N):
    for cap in CAPS:
        for M in (1, cap, cap + 1, 5 * cap + 3):
            for spw in (1, 4, 8):
                rc, launches, violations, msg = walk(N, cap, M, spw)
                assert rc == 0 and launches > 0 and violations == 0, (N, cap, M, spw, msg)


@pytest.mark.parametrize("N", SIZES)
def test_short_workspaces_are_reported(N):
    for cap in CAPS:
        for M in (1, cap, cap + 1, 5 * cap + 3):
            for short_ws, name in ((1, "fit_vectors_copy"), (2, "post_cov")):
                rc, _, violations, msg = walk(N, cap, M, 4, short_ws)
                assert rc == 0 and violations >= 1, (N, cap, M, short_ws)
                assert name in msg or "mirror" in msg, msg


def test_the_walk_counts_the_scaled_build_per_chunk():
    # M points in chunks of cap, then min(M, cap) more for the covariance: every chunk's query is the
    # same number of guard checks at one N, so the counts are linear in the number of chunks
    a = walk(300, 128, 128)[1]
    b = walk(300, 128, 256)[1]
    c = walk(300, 128, 384)[1]
    assert b - a == c - b > 0


def test_bad_arguments_are_rejected():
    E = _native.E_ARG
    assert walk(0, 128, 1)[0] == E and walk(10, 0, 1)[0] == E and walk(10, 128, -1)[0] == E
    assert walk(10, 128, 1, spw=0)[0] == E and walk(10, 128, 1, spw=9)[0] == E
    assert walk(10, 128, 1, short_ws=3)[0] == E and walk(10, 128, 1, short_ws=-1)[0] == E
    assert walk(10, 128 * 65536, 1)[0] == E
    assert walk(10, 128, 0)[0] == 0  # M = 0: the create-time launches alone


def test_null_handles():
    lib = _native.load()
    E = _native.E_ARG
    buf = (c_double * 4)()
    assert lib.gaplac_fit_mode(None, buf) == E
    lik, it, cv = c_int32(), c_int32(), c_int32()
    par, jit = c_double(), c_double()
    assert lib.gaplac_fit_laplace_info(None, byref(lik), byref(par), byref(jit), byref(it), byref(cv)) == E
    assert lib.gaplac_fit_mean_cov(None, 1, buf, 1, 0.0, buf, buf, 1) == E
    h = c_void_p(12345)
    info = c_int64()
    rc = lib.gaplac_laplace_fit_create(None, 1, 1, buf, 1, 0, None, 1e-6, _native.LIK_POISSON, 0.0, buf, 10, 1e-12,
                                       None, 128, byref(h), byref(it), byref(cv), byref(info))
    assert rc == E and not h.value
    assert lib.gaplac_laplace_fit_create(None, 1, 1, buf, 1, 0, None, 1e-6, _native.LIK_POISSON, 0.0, buf, 10, 1e-12,
                                         None, 128, None, None, None, None) == E
    assert lib.gaplac_fit_destroy(None) == 0
