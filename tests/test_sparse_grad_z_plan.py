"""gaplac_sparse_elbo_grad_z on the CPU, no device: the exported symbols and the dry walk of its
launches (gaplac_plan_check_sparse_grad_z: gaplac_plan_check_sparse_grad's walk with the product
kernel's dZ variant in the product's place, then the sum over the row tiles, the order-Mz part and
the finishing step, against the first workspace, the scratch and the buffer of dZ's partials) with
its three negative controls.
"""
import ctypes

import pytest

from gaplac_amd import _native

SHAPES = [(1, 1), (5, 129), (127, 128), (129, 127), (300, 5), (700, 127), (1000, 129), (513, 513), (2000, 257),
          (262144, 4096)]
# footprint checks the dZ walk adds: the variant's store of the partials; the sum over the row tiles
# (its reads, its store); the order-Mz part (G_uu, its store); the finishing step's store of dZ
DZ_CHECKS = 6


def plan_z(N, Mz, T=4, spw=4, short_ws=0):
    lib = _native.load()
    launches, violations = ctypes.c_int64(), ctypes.c_int64()
    msg = ctypes.create_string_buffer(256)
    rc = lib.gaplac_plan_check_sparse_grad_z(N, Mz, T, spw, short_ws, ctypes.byref(launches), ctypes.byref(violations),
                                             msg, 256)
    return rc, launches.value, violations.value, msg.value.decode()


def plan(N, Mz, spw=4, short_ws=0):
    lib = _native.load()
    launches, violations = ctypes.c_int64(), ctypes.c_int64()
    rc = lib.gaplac_plan_check_sparse_grad(N, Mz, spw, short_ws, ctypes.byref(launches), ctypes.byref(violations),
                                           None, 0)
    return rc, launches.value, violations.value


def test_the_two_symbols_are_exported():
    lib = _native.load()
    for name in ("gaplac_sparse_elbo_grad_z", "gaplac_plan_check_sparse_grad_z"):
        assert name in _native.EXPORTED
        assert hasattr(lib, name)


@pytest.mark.parametrize("N,Mz", SHAPES)
def test_every_launch_inside_its_region(N, Mz):
    for spw in ((1, 4, 8) if N <= 2000 else (4,)):
        for T in (1, 4, 16):
            rc, launches, violations, msg = plan_z(N, Mz, T, spw)
            assert rc == 0, (N, Mz, T, spw, rc, msg)
            assert violations == 0, (N, Mz, T, spw, msg)
            # gaplac_plan_check_sparse_grad's own count is what it was: the dZ walk adds the
            # footprint checks of its launches (the variant's store of the partials among them)
            rc0, l0, v0 = plan(N, Mz, spw)
            assert rc0 == 0 and v0 == 0
            assert launches == l0 + DZ_CHECKS, (N, Mz, launches, l0)


@pytest.mark.parametrize("short_ws", [1, 2, 3])
@pytest.mark.parametrize("N,Mz", [(1, 1), (128, 128), (300, 1000), (1000, 300), (2051, 5), (262144, 4096)])
def test_negative_controls_report_the_short_region(N, Mz, short_ws):
    rc, launches, violations, msg = plan_z(N, Mz, 4, 4, short_ws)
    assert rc == 0
    if short_ws == 3:  # the partials one element short: the finishing step's store of dZ leaves them
        assert violations >= 1 and "sparse_dz_finish_kernel touches elements" in msg, msg
        assert plan_z(N, Mz, 4, 4, 0)[2] == 0
    else:              # as gaplac_plan_check_sparse_grad's controls, and no fewer reports than there
        _, _, v0 = plan(N, Mz, 4, short_ws)
        assert v0 >= 2 and violations >= v0, (violations, v0)
        assert "touches elements" in msg


def test_the_product_variant_reports_a_first_workspace_too_short():
    # control 1 at a shape whose last riding row is the workspace's last element: the dZ variant's
    # footprint is the product kernel's
    rc, _, violations, _ = plan_z(2051, 5, 4, 4, 1)
    assert rc == 0 and violations >= plan(2051, 5, 4, 1)[2]


def test_bad_arguments():
    for a in ((0, 1), (10, 0), (10, 1, 0), (10, 1, 17), (10, 1, 4, 0), (10, 1, 4, 9), (10, 1, 4, 4, 4),
              (10, 1, 4, 4, -1), (65535 * 128 + 1, 1)):
        assert plan_z(*a)[0] == _native.E_ARG, a
    assert plan(10, 1, 4, 3)[0] == _native.E_ARG  # (the third control belongs to the dZ walk alone)
