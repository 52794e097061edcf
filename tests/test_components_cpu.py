"""The per-component posterior (gaplac_posterior_components) on the CPU: the formula lowering
with its component map and labels, the exported symbol, the backend switch in front of the new
front-end calls, and the dry walk of the entry's schedule.

The entry runs the posterior evaluation with G * M riding rows (gaplac_plan_check mode 2 at
M = G * M; mode 10 = the same walk against a workspace one element short): its two new kernels
are launched by the posterior's own launchers, behind the same footprint check and with the same
grids, so the walk is the same launch list. ROWS are the G * M values of
tests/test_gpu_components.py.
"""
import ctypes

import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd import fitplot
from gaplac_amd import formula as F
from gaplac_amd import kernels as K
from gaplac_amd._native import CAT, LINEAR, NOISE, OU, SQEXP

ROWS = [1, 3 * 77, 5 * 129, 2 * 255, 77, 257, 3 * 200, 3 * 86, 86, 3 * 2048, 3 * 2049, 4 * 129]
NS = [1, 50, 127, 128, 129, 300, 513, 700]


def plan(N, mode, M, spw=4):
    lib = _native.load()
    launches, violations = ctypes.c_int64(), ctypes.c_int64()
    msg = ctypes.create_string_buffer(256)
    rc = lib.gaplac_plan_check(N, mode, M, spw, ctypes.byref(launches), ctypes.byref(violations), msg, 256)
    return rc, launches.value, violations.value, msg.value.decode()


@pytest.mark.parametrize("rows", ROWS)
def test_every_launch_inside_the_workspace(rows):
    for N in NS:
        rc, launches, violations, msg = plan(N, 2, rows)
        assert rc == 0 and launches > 0, (N, rows, rc, msg)
        assert violations == 0, (N, rows, msg)


@pytest.mark.parametrize("rows", [1, 231, 645, 6147])
def test_negative_control_short_workspace_is_reported(rows):
    for N in (1, 129, 700):
        rc, _, violations, msg = plan(N, 10, rows)
        assert rc == 0 and violations >= 1 and "touches elements" in msg, (N, rows, msg)


def test_rows_leave_the_tail_at_49_tile_rows():
    # N = 300: 3 * 2048 rows are 48 tile rows and ride in the tail, 3 * 2049 are 49 and do not
    _, l1, v1, _ = plan(300, 2, 3 * 2048)
    _, l2, v2, _ = plan(300, 2, 3 * 2049)
    assert v1 == v2 == 0 and l1 < l2


def test_the_symbol_is_declared_and_exported():
    lib = _native.load()
    assert "gaplac_posterior_components" in _native.EXPORTED
    assert hasattr(lib, "gaplac_posterior_components")
    assert lib.gaplac_abi_version() == 1


def lowered(text, **kw):
    return K.lower_formula_components(F.parse_gp(text), **kw)


def test_a_sum_has_one_component_per_summand():
    terms, vars_, comp, labels = lowered("SqExp(:t; l=1.5) + OU(:t; l=3) + Cat(:p) + Linear(:n; c=0.5)")
    assert terms == [(SQEXP, 0, 1.5, 0), (OU, 1, 3.0, 1), (CAT, 2, 0.0, 2), (LINEAR, 3, 0.5, 3)]
    assert vars_ == ["t", "t", "p", "n"]
    assert comp == [0, 1, 2, 3]
    assert labels == ["SqExp(:t; l=1.5)", "OU(:t; l=3)", "Cat(:p)", "Linear(:n; c=0.5)"]
    # the same under the product lowering
    assert lowered("SqExp(:t; l=1.5) + OU(:t; l=3) + Cat(:p) + Linear(:n; c=0.5)", products=True)[2:] == (comp, labels)


def test_a_lone_product_is_one_component_under_both_lowerings():
    # reference lowering: kernel() turns the product into a sum (Q1): two groups, one component
    terms, _, comp, labels = lowered("SqExp(:t; l=2) * Cat(:p)")
    assert [t[3] for t in terms] == [0, 1] and comp == [0, 0]
    assert labels == ["SqExp(:t; l=2) * Cat(:p)"]
    terms, _, comp, labels = lowered("SqExp(:t; l=2) * Cat(:p)", products=True)
    assert [t[3] for t in terms] == [0, 0] and comp == [0, 0]
    assert labels == ["SqExp(:t; l=2) * Cat(:p)"]
    # a single term
    assert lowered("Cat(:p)")[2:] == ([0], ["Cat(:p)"])


def test_a_product_summand_is_one_group_and_one_component():
    terms, vars_, comp, labels = lowered("SqExp(:t) * Cat(:p) + Linear(:n) + Noise(0.7)", products=True)
    assert terms == [(SQEXP, 0, 1.0, 0), (CAT, 1, 0.0, 0), (LINEAR, 2, 0.0, 1), (NOISE, -1, 0.7, 2)]
    assert vars_ == ["t", "p", "n"]
    assert comp == [0, 0, 1, 2]
    assert labels == ["SqExp(:t) * Cat(:p)", "Linear(:n)", "Noise(0.7)"]
    with pytest.raises(RuntimeError):  # the reference lowering rejects a product inside a sum
        lowered("SqExp(:t) * Cat(:p) + Linear(:n)")


def test_a_noise_summand_is_a_component_of_its_own():
    terms, vars_, comp, labels = lowered("Cat(:p) + Noise + Linear(:n)")
    assert [t[0] for t in terms] == [CAT, NOISE, LINEAR]
    assert vars_ == ["p", "n"] and comp == [0, 1, 2]
    assert labels == ["Cat(:p)", "Noise", "Linear(:n)"]
    # hyperparameters move the terms, not the labels (the formula as written)
    terms, _, comp, labels = lowered("SqExp(:t; l=2) + Cat(:p)", hyperparams={"t": 5.0})
    assert terms[0] == (SQEXP, 0, 5.0, 0) and labels[0] == "SqExp(:t; l=2)"


def test_labels_parse_back_to_the_summands():
    text = "SqExp(:t; l=1.5) * Cat(:p) + OU(:t; l=0.25) + Linear(:n; c=2) + Noise(0.5)"
    labels = lowered(text, products=True)[3]
    assert F.parse_gp(" + ".join(labels)) == F.parse_gp(text)


def test_switch_gates_the_component_calls(monkeypatch):
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5) + Cat(:g)"))
    x = np.column_stack([np.linspace(0, 1, 8), np.arange(8.0) % 2])
    post = AG.posterior(AG.FiniteGP(gp, x, 0.1), np.zeros(8))
    monkeypatch.setenv("GAPLAC_HIP", "0")
    with pytest.raises(AG.BackendDisabled):
        post.component_mean_and_var(x, [0, 1])
    with pytest.raises(AG.BackendDisabled):
        fitplot.component_table("y ~| SqExp(:x; l=1.5) + Cat(:g)", {"x": x[:, 0], "g": x[:, 1], "y": np.zeros(8)})
