"""gaplac_posterior_components (HIP, through the C-ABI) against the CPU recipe of
tests/components_oracle.py (pinned by tests/test_components_oracle.py).

Inputs: columns as tests/joint_oracle.cols; the term set SqExp(col 0, 1.5) | OU(col 0, 3.0) |
Cat(col 1) | Linear(col 2, 0.5) | Noise 0.7 with every term its own group, and the same terms
with SqExp and Cat in one product group; observation noise 0.1.
Bars (tests/test_gpu_posterior.py's, per component): mean within 1e-9 max(1, max |mean_g|),
variance within 1e-9 max(1, kdiag_g). Across call shapes 1e-13 relative (tests/test_gpu_multi.py's
bar: the tail and the super-panel schedule may order the updates differently).
"""
from ctypes import c_int32, c_void_p

import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd import fitplot
from gaplac_amd import formula as F
from gaplac_amd import kernels as K
from gaplac_amd._native import CAT, LINEAR, NOISE, term_array
from gaplac_amd.backend import ArgumentError, Context, PosDefException
from tests import components_oracle as CO
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
SETS = {"single_groups": CO.TERMS, "product_group": CO.TERMS_PROD}


@pytest.fixture(scope="module")
def ctx():
    if not gpu_available():
        pytest.skip("no GPU")
    c = Context(0)
    yield c
    c.close()


def run(ctx, case, comp=None, G=None, terms=None):
    return ctx.posterior_components(case.X, case.terms if terms is None else terms, CO.NOISE_OBS, case.y, case.Xs,
                                    case.comp if comp is None else comp, case.G if G is None else G)


def check(ctx, case):
    mean, var = run(ctx, case)
    assert mean.shape == var.shape == (case.M, case.G)
    ok, em, ev = CO.within_bars(mean, var, case)
    print(f"N={case.N} G={case.G} M={case.M}: worst mean / bar {em:.3g}, worst var / bar {ev:.3g}")
    assert ok
    for g in range(case.G):
        tg = CO.terms_of(case.terms, case.comp, g)
        if not tg:  # the zero process: exactly +0.0
            for a in (mean[:, g], var[:, g]):
                assert np.all(a == 0.0) and not np.any(np.signbit(a))
        elif all(t[0] == NOISE for t in tg):  # a Noise component: mean exactly 0, its variance exactly
            assert np.all(mean[:, g] == 0.0) and np.all(var[:, g] == tg[0][2])
    return mean, var


# 1. sizes: odd M makes a lane's two rows straddle components; 3 * 77 = 231 and 5 * 129 = 645 put
# component boundaries inside 128-row tiles. G = 3 leaves Linear and Noise out, G = 5 makes the Noise
# term a component (the product set has four groups: its fifth component is empty).
@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("G,M", [(1, 1), (3, 77), (5, 129), (2, 255)])
@pytest.mark.parametrize("N", [1, 50, 127, 128, 129, 300, 700])
def test_sizes_against_the_oracle(ctx, N, G, M, name):
    check(ctx, CO.Case(N, G, M, SETS[name]))


# 2. one component holding every term: the same rows, schedule and row contents as the posterior
@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("N,M", [(129, 77), (700, 257)])
def test_one_component_is_the_whole_posterior_bit_for_bit(ctx, N, M, name):
    case = CO.Case(N, 1, M, SETS[name])
    assert case.comp == [0] * len(case.terms)
    mean, var = run(ctx, case)
    m, v = ctx.posterior_mean_var(case.X, case.terms, CO.NOISE_OBS, case.y, case.Xs)
    assert np.array_equal(mean[:, 0], m) and np.array_equal(var[:, 0], v)


# 3. within one call shape the rows do not see each other
def test_permutations_are_bitwise(ctx):
    case = CO.Case(513, 3, 200)
    mean, var = run(ctx, case)
    rng = np.random.default_rng(3)
    for perm in ([2, 0, 1], [1, 0, 2]):  # component g becomes component perm[g]
        comp = [perm[c] if c >= 0 else -1 for c in case.comp]
        pm, pv = run(ctx, case, comp=comp)
        assert np.array_equal(pm[:, perm], mean) and np.array_equal(pv[:, perm], var)
    rows = rng.permutation(case.M)
    pm, pv = ctx.posterior_components(case.X, case.terms, CO.NOISE_OBS, case.y, case.Xs[rows], case.comp, 3)
    assert np.array_equal(pm, mean[rows]) and np.array_equal(pv, var[rows])


# 4. across call shapes
def close13(a, b):
    return np.max(np.abs(a - b)) <= 1e-13 * max(1.0, np.max(np.abs(b)))


@pytest.fixture(scope="module")
def shape_case():
    return CO.Case(700, 3, 86)


def test_a_component_equals_its_own_single_call(ctx, shape_case):
    case = shape_case
    mean, var = check(ctx, case)
    for g in range(3):
        comp = [0 if c == g else -1 for c in case.comp]
        m1, v1 = run(ctx, case, comp=comp, G=1)
        print("component", g, "max |diff| mean", np.max(np.abs(m1[:, 0] - mean[:, g])), "var",
              np.max(np.abs(v1[:, 0] - var[:, g])))
        assert close13(m1[:, 0], mean[:, g]) and close13(v1[:, 0], var[:, g])


def test_superpanel_rows_agree_with_the_tail(shape_case, monkeypatch):
    if not gpu_available():
        pytest.skip("no GPU")
    case = shape_case
    with Context(0) as c:
        a = run(c, case)
    monkeypatch.setenv("GAPLAC_TAILK", "0")
    with Context(0) as c:
        b = run(c, case)
    print("tail vs super-panels: max |diff| mean", np.max(np.abs(a[0] - b[0])), "var", np.max(np.abs(a[1] - b[1])))
    assert close13(a[0], b[0]) and close13(a[1], b[1])


# 5. 3 * 2048 = 6144 rows are 48 tile rows, the last count that rides in the tail beside the matrix;
# 3 * 2049 = 6147 are 49, the first that does not (tests/test_gpu_multi.py's boundaries)
@pytest.mark.parametrize("M", [2048, 2049])
def test_the_tails_row_capacity(ctx, M):
    check(ctx, CO.Case(300, 3, M))


# 6. the component means add up to the posterior mean
@pytest.mark.parametrize("N,M", [(300, 129), (700, 77)])
def test_sum_rule(ctx, N, M):
    case = CO.Case(N, 5, M)
    assert sorted(case.comp) == [0, 1, 2, 3, 4]
    mean, _ = run(ctx, case)
    full, _ = ctx.posterior_mean_var(case.X, case.terms, CO.NOISE_OBS, case.y, case.Xs)
    bar = 1e-9 * max(1.0, np.sum(np.max(np.abs(mean), axis=0)))
    print("sum rule: max |diff|", np.max(np.abs(mean.sum(1) - full)), "bar", bar)
    assert np.max(np.abs(mean.sum(1) - full)) <= bar


# 7. edges
def raw(ctx, case, G, comp, mean, ldm, var, ldv, M=None, terms=None, X=None, y=None, noise=CO.NOISE_OBS):
    terms = case.terms if terms is None else terms
    Xc = np.asfortranarray(case.X if X is None else X, dtype=np.float64)
    y = np.ascontiguousarray(case.y if y is None else y, dtype=np.float64)
    Xs = np.asfortranarray(case.Xs, dtype=np.float64)
    N, D = Xc.shape
    M = Xs.shape[0] if M is None else M
    ca = (c_int32 * max(1, len(comp)))(*comp) if comp is not None else None
    p = lambda a: None if a is None else a.ctypes.data_as(c_void_p)
    return ctx.lib.gaplac_posterior_components(ctx.h, N, D, p(Xc), max(N, 1), len(terms), term_array(terms), float(noise),
                                               p(y), M, p(Xs), max(Xs.shape[0], 1), G, ca, p(mean), ldm, p(var), ldv)


def test_an_empty_component_is_exactly_zero(ctx):
    case = CO.Case(129, 4, 77, comp=[0, 2, 2, -1, 3])  # component 1 has no terms
    mean, var = check(ctx, case)
    assert np.all(mean[:, 1] == 0.0) and np.all(var[:, 1] == 0.0)
    assert not np.any(np.signbit(mean[:, 1])) and not np.any(np.signbit(var[:, 1]))


def test_no_training_points_gives_the_prior(ctx):
    case = CO.Case(0, 5, 9)
    mean, var = run(ctx, case)
    assert np.all(mean == 0.0)
    assert np.max(np.abs(var - case.kd)) <= 1e-15 * np.max(case.kd)
    assert np.all(var[:, 4] == 0.7) and np.all(var[:, :3] == 1.0)


def test_no_points_or_no_components_write_nothing(ctx):
    case = CO.Case(50, 3, 7)
    can_m, can_v = np.full((7, 3), -7.5, order="F"), np.full((7, 3), -7.5, order="F")
    assert raw(ctx, case, 3, case.comp, can_m, 7, can_v, 7, M=0) == 0
    assert raw(ctx, case, 0, [-1] * 5, can_m, 7, can_v, 7) == 0
    assert raw(ctx, case, 0, None, can_m, 7, can_v, 7) == 0
    assert np.all(can_m == -7.5) and np.all(can_v == -7.5)
    m, v = ctx.posterior_components(case.X, case.terms, CO.NOISE_OBS, case.y, case.Xs[:0], case.comp, 3)
    assert m.shape == v.shape == (0, 3)
    m, v = ctx.posterior_components(case.X, case.terms, CO.NOISE_OBS, case.y, case.Xs, [-1] * 5)
    assert m.shape == v.shape == (7, 0)
    # bad terms are reported before the early return
    with pytest.raises(ArgumentError):
        ctx.posterior_components(case.X, [(CAT, 7, 0.0, 0)], CO.NOISE_OBS, case.y, case.Xs[:0], [0], 1)


def test_outputs_are_optional_and_padding_rows_stay(ctx):
    case = CO.Case(129, 3, 77)
    mean, var = run(ctx, case)
    pm, pv = np.full((80, 3), -7.5, order="F"), np.full((79, 3), -7.5, order="F")
    assert raw(ctx, case, 3, case.comp, pm, 80, pv, 79) == 0
    assert np.array_equal(pm[:77], mean) and np.array_equal(pv[:77], var)
    assert np.all(pm[77:] == -7.5) and np.all(pv[77:] == -7.5)  # rows M .. ld-1 are the caller's
    only = np.empty((77, 3), order="F")
    assert raw(ctx, case, 3, case.comp, only, 77, None, 0) == 0 and np.array_equal(only, mean)
    assert raw(ctx, case, 3, case.comp, None, 0, only, 77) == 0 and np.array_equal(only, var)


def test_argument_errors(ctx):
    case = CO.Case(50, 3, 7)
    m, v = np.zeros((7, 3), order="F"), np.zeros((7, 3), order="F")
    # one product group in two components
    assert raw(ctx, case, 2, [0, 1, 1, -1, -1], m, 7, v, 7, terms=CO.TERMS_PROD) == _native.E_KIND
    assert raw(ctx, case, 2, [0, 0, 1, -1, -1], m, 7, v, 7, terms=CO.TERMS_PROD) == 0
    bad = [raw(ctx, case, 3, [0, 1, 3, -1, -1], m, 7, v, 7),   # an entry = G
           raw(ctx, case, 3, [0, 1, -2, -1, -1], m, 7, v, 7),  # an entry below -1
           raw(ctx, case, -1, case.comp, m, 7, v, 7),
           raw(ctx, case, 3, None, m, 7, v, 7),                # comp NULL with G > 0 and T > 0
           raw(ctx, case, 3, case.comp, m, 6, v, 7),           # ldm < M
           raw(ctx, case, 3, case.comp, m, 7, v, 6)]           # ldv < M
    assert bad == [_native.E_ARG] * len(bad)
    for rc in bad:
        with pytest.raises(ArgumentError):
            ctx._check(rc)
    assert raw(ctx, case, 3, case.comp, None, 0, None, 0) == 0  # (leading dimensions of NULL outputs are not read)
    with pytest.raises(ArgumentError):
        ctx.posterior_components(case.X, case.terms, CO.NOISE_OBS, case.y, case.Xs, [0, 1])  # len(comp) != T
    check(ctx, case)


def test_not_positive_definite_fills_nan_and_the_context_survives(ctx):
    # Linear-only, noise 0 on integer inputs: K = x x^T has rank 1 and the second pivot is exactly 0
    case = CO.Case(50, 3, 7)
    X = np.column_stack([np.zeros(8), np.zeros(8), np.arange(1.0, 9.0)])
    lin = [(LINEAR, 2, 0.0, 0)]
    m, v = np.zeros((7, 1), order="F"), np.zeros((7, 1), order="F")
    rc = raw(ctx, case, 1, [0], m, 7, v, 7, terms=lin, X=X, y=np.ones(8), noise=0.0)
    assert rc == 2 and np.all(np.isnan(m)) and np.all(np.isnan(v))
    with pytest.raises(PosDefException) as e:
        ctx.posterior_components(X, lin, 0.0, np.ones(8), case.Xs, [0])
    assert e.value.info == 2
    # the parity tests' Cat-only, noise 0 matrix (repeated levels) fails the same way
    Xc = np.repeat(np.arange(8.0), 4)[:, None] * np.ones((1, 3))
    m[:], v[:] = 0.0, 0.0
    rc = raw(ctx, case, 1, [0], m, 7, v, 7, terms=[(CAT, 0, 0.0, 0)], X=Xc, y=np.ones(32), noise=0.0)
    assert rc > 0 and np.all(np.isnan(m)) and np.all(np.isnan(v))
    check(ctx, case)  # a good call on the same context


def test_a_dirty_workspace(ctx):
    check(ctx, CO.Case(700, 5, 129))
    check(ctx, CO.Case(129, 3, 77))
    check(ctx, CO.Case(50, 2, 255))


# 8. the fitplot table on the reference's example data
def test_fitplot_component_table(ctx, tmp_path):
    import os

    import pandas as pd

    from tests.golden_io import GOLDEN
    df = pd.read_csv(os.path.join(GOLDEN, "data", "input_pair_109.tsv"), sep="\t")
    table = {c: df[c].to_numpy() for c in df.columns if c != "SampleID"}
    text = "bug ~| Cat(:PersonID) + Linear(:nutrient)"
    out = fitplot.component_table(text, table, ctx=ctx, output=str(tmp_path / "fit.tsv"))
    labels = ["Cat(:PersonID)", "Linear(:nutrient)"]
    assert list(out) == ["PersonID", "nutrient"] + [f"{l}.{s}" for l in labels for s in ("mean", "var", "partial")]
    y = np.asarray(table["bug"], dtype=np.float64)
    assert all(len(out[c]) == len(y) for c in out)
    spec = F.gp_spec(text)
    gp, vars_ = AG.make_gp(spec)
    X = AG.design_matrix(table, vars_)
    post = AG.posterior(AG.FiniteGP(gp, X, 0.1), y, ctx=ctx)
    full, _ = post.mean_and_var(X)
    means = np.column_stack([out[f"{l}.mean"] for l in labels])
    bar = 1e-9 * max(1.0, np.sum(np.max(np.abs(means), axis=0)))
    print("table: max |sum of means - posterior mean|", np.max(np.abs(means.sum(1) - full)), "bar", bar)
    assert np.max(np.abs(means.sum(1) - full)) <= bar
    assert np.array_equal(out[f"{labels[0]}.partial"], y - means[:, 1])
    assert np.array_equal(out[f"{labels[1]}.partial"], y - means[:, 0])
    for l in labels:
        assert np.all(np.isfinite(out[f"{l}.var"]))
    # the front end gives the same numbers; the file has the table's columns and rows
    terms, _, comp, _ = K.lower_formula_components(F.formula(spec))
    m2, v2 = post.component_mean_and_var(X, comp)
    assert np.array_equal(m2, means) and np.array_equal(v2[:, 0], out[f"{labels[0]}.var"])
    lines = (tmp_path / "fit.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(out) and len(lines) == len(y) + 1
    # at other points: no partial residuals
    at = {"PersonID": table["PersonID"][:5], "nutrient": np.linspace(0, 1, 5)}
    out2 = fitplot.component_table(text, table, at=at, ctx=ctx)
    assert list(out2) == ["PersonID", "nutrient"] + [f"{l}.{s}" for l in labels for s in ("mean", "var")]
    assert all(len(out2[c]) == 5 for c in out2)
