"""tests/hp_oracle.py against the numpy oracle (CPU): the rounding-error bound holds for
oracle.restatement with constants 1 on the sweeps the GPU tests use, for values and both
derivatives, and the comparison is sharp enough to see an 8-ulp error in one entry and a table
entry taken from its neighbour."""
import numpy as np
import pytest

from oracle import restatement as R
from tests import hp_oracle as H
from tests import sparse_grad_z_oracle as GZ

KINDS = [(H.SQEXP, "sqexp"), (H.OU, "ou")]
PAIRS = H.sweep_pairs()
PAIRS_D = H.sweep_pairs(overflow=False)


def numpy_entries(kind, l, x):
    X = np.asarray(x)[:, None]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        K = R.term_matrix(X, kind, 0, l)
        dl = R.term_derivative(X, kind, 0, l)
        dx = GZ.d1_term(X, X, kind, 0, l).T          # d k(x_i, x_j) / d x_j = d1 k(x_j, x_i)
    return K, dl, dx


@pytest.mark.parametrize("l,x0", H.CASES)
@pytest.mark.parametrize("kind,name", KINDS)
def test_numpy_oracle_inside_the_bound_with_constants_one(kind, name, l, x0):
    x = H.sweep_x(kind, l, x0)
    got = numpy_entries(kind, l, x)
    for which, what in enumerate(("k", "dk/dl", "dk/dxj")):
        r, at = H.worst_ratio(kind, l, x, PAIRS if which == 0 else PAIRS_D, got[which], which)
        print(f"{name} l={l} x0={x0} {what}: worst error/bound {r:.3f} at {at}")
        assert r <= 1.0, (what, r, at)
    # exact duplicates of the anchor: k exactly 1, derivatives exactly 0
    for i in (1, 2):
        assert x[i] == x[0] and got[0][i, 0] == 1.0 and got[1][i, 0] == 0.0 and got[2][i, 0] == 0.0


def test_designed_arguments_are_realised():
    """At offset 0 the pair (i, 0) has the designed argument to within a few ulps: every breakpoint
    j ln2/256 (every residue j mod 256), the tie points, both sides of the flush, an underflowing
    and an overflowing d^2."""
    for kind, _ in KINDS:
        x = H.sweep_x(kind, 1.5, 0.0)
        args = H.sweep_args()
        hit = set()
        for i, a in enumerate(args, start=1):
            got = -float(H._parts(kind, 1.5, x[i], x[0])[4])
            assert abs(got - a) <= 1e-15 * a
            q = a / H.LN2_256
            if abs(q - round(q)) < 1e-9:
                hit.add(int(round(q)) % 256)
        assert hit == set(range(256))
        assert any(745.13 < a < 745.2 for a in args) and any(a > 745.2 for a in args) and 708.39 in args
    x = H.sweep_x(H.SQEXP, 1.5, 0.0)
    with np.errstate(over="ignore", under="ignore"):
        assert np.float64(x[-2] / 1.5) ** 2 == 0.0 and x[-2] != 0.0 and np.isinf(np.float64(x[-1] / 1.5) ** 2)


def test_sees_eight_ulps_in_one_normal_entry():
    for kind, _ in KINDS:
        x = H.sweep_x(kind, 1.5, 0.0)
        K = numpy_entries(kind, 1.5, x)[0]
        i = H.BREAK0 + 100
        assert 1e-3 < K[i, 0] < 1.0
        assert H.worst_ratio(kind, 1.5, x, [(i, 0)], K)[0] <= 1.0
        for sign in (1, -1):
            Kb = K.copy()
            Kb[i, 0] += sign * 8 * np.spacing(K[i, 0])
            assert H.worst_ratio(kind, 1.5, x, [(i, 0)], Kb)[0] > 1.0
            assert H.worst_ratio(kind, 1.5, x, PAIRS, Kb)[0] > 1.0


def test_sees_a_neighbouring_table_entry_at_every_breakpoint():
    """exp at breakpoint j is 2^-(j/256): an implementation reading table entry j +- 1 is off by the
    factor 2^(1/256). Every one of the 255 breakpoint points (and the duplicate, j = 0) notices."""
    for kind, _ in KINDS:
        x = H.sweep_x(kind, 1.5, 0.0)
        K = numpy_entries(kind, 1.5, x)[0]
        for i in [1] + list(range(H.BREAK0, H.BREAK0 + 255)):
            for f in (2.0 ** (1 / 256), 2.0 ** (-1 / 256)):
                Kb = K.copy()
                Kb[i, 0] *= f
                assert H.worst_ratio(kind, 1.5, x, [(i, 0)], Kb, 0, 4, 4)[0] > 1e10


def test_cat_rule_of_the_reference_in_both_oracle_branches():
    """kappa(d2) = d2 > 0 ? 0 : 1: a NaN category has covariance 1 with everything."""
    x = np.array([1.0, np.nan, 1.0, 2.0, -0.0, 0.0, np.inf, -np.inf])
    want = np.array([[float(H.entry(H.CAT, 0.0, a, b)[0]) for b in x] for a in x])
    assert want[1].tolist() == [1.0] * 8 and want[0, 3] == 0.0 and want[4, 5] == 1.0 and want[6, 6] == 1.0
    with np.errstate(invalid="ignore"):
        assert np.array_equal(R.term_matrix(x[:, None], R.CAT, 0, 0.0, "direct"), want)
        assert np.array_equal(R.cross_term_matrix(x[:, None], x[:, None], R.CAT, 0, 0.0), want)
        fin = x[~np.isinf(x)]                        # (inf^2 - 2 inf^2 is NaN in the gemm form by its nature)
        assert np.array_equal(R.term_matrix(fin[:, None], R.CAT, 0, 0.0, "gemm"),
                              R.term_matrix(fin[:, None], R.CAT, 0, 0.0, "direct"))


def test_dense_formulas_against_the_numpy_oracle():
    """The mp.matrix formulas (N <= 3) state what oracle.restatement and the sparse oracles compute."""
    from tests import sparse_oracle as S
    X = np.array([[0.3, 1.0], [1.1, 2.0], [2.0, 1.0]])
    terms = [(H.SQEXP, 0, 1.5, 0), (H.CAT, 1, 0.0, 0), (H.OU, 0, 0.7, 1), (H.LINEAR, 0, 0.5, 2)]
    v = np.array([1.0, -0.5, 0.25])
    lp, dv, dth, dn, sth, sn = H.logpdf_grad(X.tolist(), terms, 0.3, v)
    rl, rdv, rdp, rdn = R.logpdf_grad(X, terms, 0.3, v)
    rs, rsn = R.logpdf_grad_scale(X, terms, 0.3, v)
    assert abs(float(lp) - rl) <= 1e-14 * abs(rl)
    assert np.allclose([float(t) for t in dv], rdv, rtol=1e-13, atol=0)
    assert np.allclose([float(t) for t in dth], rdp, rtol=0, atol=1e-13 * rs.max())
    assert abs(float(dn) - rdn) <= 1e-13 * rsn and np.allclose([float(t) for t in sth], rs, rtol=1e-13)
    Xs = np.array([[0.7, 2.0], [5.0, 3.0]])
    m = H.posterior_mean(X.tolist(), terms, 0.3, v, Xs.tolist())
    assert np.allclose([float(t) for t in m], R.posterior_mean_var(X, terms, 0.3, v, Xs)[0], rtol=1e-13)
    Z = np.array([[0.5, 1.0], [1.7, 2.0]])
    e = H.vfe_bound(X.tolist(), terms, 0.3, v, Z.tolist(), 1e-3)
    assert abs(float(e) - S.dense(X, terms, 0.3, v, Z, 1e-3)["elbo"]) <= 1e-12 * abs(float(e))
    dZ = H.vfe_bound_grad_z(X.tolist(), terms, 0.3, v, Z.tolist(), 1e-3, cols=[0])
    ref, scale = GZ.dense(X, terms, 0.3, v, Z, 1e-3)
    for mi in range(2):
        assert abs(float(dZ[mi][0]) - ref[mi, 0]) <= 1e-11 * (abs(ref[mi, 0]) + scale[mi, 0])
