"""One line per call of every host-only plan entry: rc, launches, violations, message.

    python tools/plan_table.py > table.txt        (GAPLAC_LIB_PATH picks another build)

The behaviour check of a change to the plan walks: between two builds rc and the counts must be
identical line for line; the message may differ only where a negative control (short_ws > 0) has
several violations. The grids are the plan tests' own constants. Not a golden file: launch counts
change legitimately with schedule work. No device needed.
"""
import ctypes
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaplac_amd import _native  # noqa: E402
from tests import test_fit_plan as fp, test_joint_plan as jp, test_laplace_fit_plan as lfp  # noqa: E402
from tests import test_laplace_grad_plan as lgp, test_laplace_plan as lp, test_multi_plan as mp  # noqa: E402
from tests import test_plan_guard as pg, test_sparse_grad_plan as sgp, test_sparse_grad_z_plan as sgz  # noqa: E402
from tests import test_sparse_joint_plan as sjp, test_sparse_plan as sp  # noqa: E402

SPWS = (4, 1)  # super-panel widths: the default and the narrowest (every panel column a super-panel)
# entry -> (argument tuples before spw, the short_ws values it accepts)
WALKS = {
    "laplace_fit": (itertools.product(lfp.SIZES, lfp.CAPS, lp.MS), range(3)),
    "fit": (itertools.product(fp.NS, fp.CAPS, lp.MS), range(2)),
    "laplace_grad": (((n,) for n in lgp.SIZES), range(3)),
    "laplace": (itertools.product(lp.EDGES, lp.MS), range(2)),
    "sparse": (itertools.product(sp.NS, sp.MZS, sp.MSS), range(3)),
    "sparse_grad": (sgp.SHAPES, range(3)),
    "sparse_grad_z": ((s + (t,) for s in sgz.SHAPES for t in (1, 4)), range(4)),  # T: one term, and the test's 4
    "sparse_joint": (itertools.product(sp.NS, sp.MZS, sjp.MSS, sjp.RS), range(4)),
    "joint": (itertools.product(fp.NS, jp.MS, sjp.RS), range(3)),
}


def main():
    lib = _native.load()
    launches, violations, msg = ctypes.c_int64(), ctypes.c_int64(), ctypes.create_string_buffer(256)
    tail = (ctypes.byref(launches), ctypes.byref(violations), msg, 256)

    def line(name, args, short_ws, fn, *fargs):
        launches.value = violations.value = -1
        msg.value = b""
        rc = fn(*fargs, *tail)
        print(f"{name} {args} short_ws={short_ws} rc={rc} launches={launches.value} "
              f"violations={violations.value} | {msg.value.decode()}")

    for name, (grid, shorts) in WALKS.items():
        fn = getattr(lib, "gaplac_plan_check_" + name)
        for args, spw, short_ws in itertools.product(list(grid), SPWS, shorts):
            line(name, tuple(args) + (spw,), short_ws, fn, *args, spw, short_ws)
    # the plain entry: mode 0 / 1 at every size, 2 / 3 with the joint's and the multi entries' M; + 8: short
    modes = [(0, [1]), (1, [1]), (2, jp.MS), (3, mp.RS)]
    for N, (mode, Ms), spw, short_ws in itertools.product(pg.SIZES, modes, SPWS, (0, 1)):
        for M in Ms:
            line("plain", (N, mode, M, spw), short_ws, lib.gaplac_plan_check, N, mode + 8 * short_ws, M, spw)


if __name__ == "__main__":
    main()
