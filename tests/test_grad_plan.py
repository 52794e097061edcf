"""(CPU) What the sizes of tests/test_gpu_grad_schedule.py reach in the gradient's schedule, its launch
footprints there, and the oracle's own error at those sizes.

extra_row_launches mirrors, in plain Python, the tile counts of the identity rows' launches in
factor_and_reduce (gaplac_api.hip): extra_rows_chain's rows (c1 - c) per chain step with rows = c,
extra_rows_update's rows (je - jb) with rows = the end of the super-panel applied, on s_extra and on
s_xrest. A launch of at least XR_TILE_MIN = 128 tiles runs as whole tiles (tile_syrk_kernel with the
rectangular tile_decode: strips of 8 tile rows, then the remainder rows & 7), a smaller one on
quadrants.

What the mirror guards: the sizes of the GPU test stay tied to their purpose. If someone edits a size
or a width there, the claims of that file's table fail here. It is a restatement of the host code, not
a reading of it: it cannot see a change of XR_TILE_MIN, of the schedule or of build_grad_list in the
library (the footprint walk below does run the library's own schedule).
"""
import numpy as np
import pytest

from oracle import restatement as R
from tests.backward_error import worst_ratio
from tests.test_plan_guard import plan

NB = 128
XR_TILE_MIN = 128
# (N, W) of tests/test_gpu_grad_schedule.py's table
TABLE = [(640, 1), (2049, 4), (3400, 4), (4000, 8)]


def tile_columns(N):
    return -(-(N + 1) // NB)


def superpanels(N, W):
    nt = tile_columns(N)
    return list(range(0, nt, W)) + [nt]


def extra_row_launches(N, W, serial=False):
    """[(stream, p, c or None, rows, columns)] of one gradient evaluation, in enqueue order per stream:
    "chain" (step c of super-panel p), "extra" (SP p on SP p+1's columns, s_extra), "xrest" (SP p-1 on
    the columns after SP p, s_xrest), "merged" (both updates as one launch, GAPLAC_SERIAL)."""
    spc = superpanels(N, W)
    nt, nsp = spc[-1], len(spc) - 1
    out = []
    for p in range(nsp):
        c0, c1 = spc[p], spc[p + 1]
        if not serial and p >= 1 and nt > c1:
            out.append(("xrest", p, None, c0, nt - c1))
        for c in range(c0 + 1, c1):
            out.append(("chain", p, c, c, c1 - c))
        je = nt if serial else (spc[p + 2] if p + 2 <= nsp else nt)
        if je > c1:
            out.append(("merged" if serial else "extra", p, None, c1, je - c1))
    return out


def whole(launch):
    return launch[3] * launch[4] >= XR_TILE_MIN


def cinv_supertiles(N):
    s = -(-(-(-N // NB)) // 8)
    return s * (s + 1) // 2


def test_640_spw1_reuses_both_event_parities_twice():
    spc = superpanels(640, 1)
    assert spc == [0, 1, 2, 3, 4, 5, 6]
    ls = extra_row_launches(640, 1)
    # ev_xr[(p - 1) & 1] is recorded behind every s_xrest update and waited for at p + 1 (p >= 2 in
    # factor_and_reduce); ev_xc[p & 1] behind every chain
    xr = [l[1] for l in ls if l[0] == "xrest"]
    assert xr == [1, 2, 3, 4]                      # parities 0, 1, 0, 1: each recorded twice
    assert not any(whole(l) for l in ls)           # the smallest size: quadrants only
    assert not any(l[0] == "chain" for l in ls)    # W = 1: no step inside a super-panel


def test_2049_last_superpanel_is_one_column_wide():
    spc = superpanels(2049, 4)
    assert spc == [0, 4, 8, 12, 16, 17]
    assert not any(whole(l) for l in extra_row_launches(2049, 4))
    assert cinv_supertiles(2049) == 6 and -(-2049 // NB) == 17   # the third super-row: tile row 16 alone


def test_3400_has_one_whole_tile_launch_with_a_remainder():
    spc = superpanels(3400, 4)
    assert spc == [0, 4, 8, 12, 16, 20, 24, 27] and [b - a for a, b in zip(spc[4:], spc[5:])] == [4, 4, 3]
    ls = extra_row_launches(3400, 4)
    big = [l for l in ls if whole(l)]
    assert big == [("xrest", 3, None, 12, 11)]     # 132 tiles: one strip of 8 rows and 4 more
    assert big[0][3] % 8 == 4 and big[0][3] // 8 == 1
    assert sum(1 for l in ls if not whole(l)) >= 20  # quadrant launches in the same evaluation


def test_4000_spw8_whole_tiles_and_quadrants():
    spc = superpanels(4000, 8)
    assert spc == [0, 8, 16, 24, 32]
    ls = extra_row_launches(4000, 8)
    tiles = {(l[0], l[1], l[2]): (l[3], l[4]) for l in ls}
    assert tiles[("extra", 1, None)] == (16, 8) and tiles[("extra", 2, None)] == (24, 8)
    assert tiles[("xrest", 1, None)] == (8, 16) and tiles[("xrest", 2, None)] == (16, 8)
    assert [tiles[("chain", 3, c)][0] * tiles[("chain", 3, c)][1] for c in (25, 26, 27, 28)] == [175, 156, 135, 112]
    got = sorted((l[0], l[1], l[2]) for l in ls if whole(l))
    assert got == sorted([("extra", 1, None), ("extra", 2, None), ("xrest", 1, None), ("xrest", 2, None),
                          ("chain", 3, 25), ("chain", 3, 26), ("chain", 3, 27)])
    assert not whole(("chain", 3, 28, *tiles[("chain", 3, 28)]))


def test_some_size_has_a_whole_tile_launch_with_a_partial_strip():
    """Across the table: a launch of at least 128 tiles whose row count is no multiple of 8, with
    quadrant launches in the same evaluation (3400; the 4000 chain steps 25, 26, 27 too)."""
    hits = []
    for N, W in TABLE:
        ls = extra_row_launches(N, W)
        if any(whole(l) and l[3] % 8 for l in ls) and any(not whole(l) for l in ls):
            hits.append(N)
    assert hits == [3400, 4000]


def test_serial_schedule_merges_the_updates():
    """GAPLAC_SERIAL: one update per super-panel over every later column, so launches that were
    quadrants on two streams become whole tiles (which is why test_serial_schedule compares the two)."""
    s34 = [(l[3], l[4]) for l in extra_row_launches(3400, 4, serial=True) if whole(l)]
    assert s34 == [(8, 19), (12, 15), (16, 11), (20, 7)]     # multi-stream: (12, 11) alone
    # N = 4000 in the serial context runs the default width, 4, against the default context's
    s40 = [(l[3], l[4]) for l in extra_row_launches(4000, 4, serial=True) if whole(l)]
    assert s40 == [(8, 24), (12, 20), (16, 16), (20, 12), (24, 8)]
    m40 = [(l[0], l[3], l[4]) for l in extra_row_launches(4000, 4) if whole(l)]
    assert m40 == [("xrest", 8, 20), ("xrest", 12, 16), ("xrest", 16, 12), ("xrest", 20, 8)]


def test_cinv_supertiles_wrap_the_xcd_queues():
    """build_grad_list deals super-tile s to queue s & 7: with more than 8 some queue holds a second
    one and the others are padded behind it. 3400 (m = 27) is the table's case; 4000 (m = 32) has ten
    super-tiles as well, all of them full."""
    counts = {N: cinv_supertiles(N) for N, _ in TABLE}
    assert counts == {640: 1, 2049: 6, 3400: 10, 4000: 10}
    assert [N for N in counts if counts[N] > 8] == [3400, 4000]


@pytest.mark.parametrize("N,W", TABLE)
def test_footprints_inside_the_workspace(N, W):
    """The library's own dry walk (gaplac_plan_check, mode 1 = gradient) of every launch at the table's
    sizes and widths; its short-workspace control (mode + 8) reports."""
    launches, violations, msg = plan(N, 1, 0, W)
    assert launches > 0 and violations == 0, (N, W, msg)
    _, violations, msg = plan(N, 1 + 8, 0, W)
    assert violations >= 1 and "touches elements" in msg


@pytest.mark.parametrize("N", [2049, 3400])
def test_oracle_routes_agree(N):
    """The yardstick of tests/test_gpu_grad_schedule.py at its sizes: cho_solve's C^-1 (logpdf_grad)
    against dpotri's (logpdf_grad_potri) within 1e-12 of (|ref| + scale) on dparam and dnoise and of
    max |dv| on dv, a thousandth of the 1e-9 it judges (2.5e-16 at N = 3201)."""
    from tests.test_gpu_grad_schedule import COMPOSITE, NOISE_VAR, inputs
    X, v = inputs(N, "composite")
    lp, dv, dp, dn = R.logpdf_grad(X, COMPOSITE, NOISE_VAR, v)
    lp2, dv2, dp2, dn2 = R.logpdf_grad_potri(X, COMPOSITE, NOISE_VAR, v)
    sc, scn = R.logpdf_grad_scale(X, COMPOSITE, NOISE_VAR, v)
    edp = worst_ratio(np.abs(dp2 - dp), np.abs(dp) + sc)      # (Cat: 0 of 0)
    edn = abs(dn2 - dn) / (abs(dn) + scn)
    edv = float(np.max(np.abs(dv2 - dv)) / np.max(np.abs(dv)))
    print(f"GRADPLAN oracle routes N={N}: dparam {edp:.2e}, dnoise {edn:.2e}, dv {edv:.2e}")
    assert lp2 == lp
    assert edp <= 1e-12 and edn <= 1e-12 and edv <= 1e-12
