"""The per-component recipe (tests/components_oracle.py) pinned on the CPU: against the dense
solve K_g(xs, X) solve(C, y) and kdiag_g - diag(K_g solve(C, K_g^T)), a route without any
Cholesky factor, and, with one component holding every term, against R.posterior_mean_var.

Bars: both routes are backward-stable solves with C, cond(C) <= (|K| + noise) / noise ~ 1e4 at
these sizes (kernel sums of a few hundred unit-diagonal entries, noise 0.1), so they agree to
~cond * eps ~ 1e-12 relative; 1e-10 of max(1, max |mean_g|) / max(1, kdiag_g) leaves two digits.
No GPU needed."""
import numpy as np
import pytest

from oracle import restatement as R
from tests import components_oracle as CO

N, M = 129, 77


def inputs(terms):
    rng = np.random.default_rng(11)
    return CO.cols(rng, N), CO.cols(rng, M), rng.normal(size=N)


@pytest.mark.parametrize("terms", [CO.TERMS, CO.TERMS_PROD], ids=["single_groups", "product_group"])
def test_recipe_matches_the_dense_solve(terms):
    X, Xs, y = inputs(terms)
    G = max(t[3] for t in terms) + 1
    comp = CO.comp_for(terms, G)
    mean, var, kd = CO.components(X, terms, CO.NOISE_OBS, y, Xs, comp, G)
    C = R.gram(X, terms, CO.NOISE_OBS)
    alpha = np.linalg.solve(C, y)
    for g in range(G):
        tg = CO.terms_of(terms, comp, g)
        Kg = R.cross_gram(X, Xs, tg).T  # M x N
        m_ref = Kg @ alpha
        v_ref = R.kernel_diag(Xs, tg) - np.einsum("ij,ji->i", Kg, np.linalg.solve(C, Kg.T))
        assert np.max(np.abs(mean[:, g] - m_ref)) <= 1e-10 * max(1.0, np.max(np.abs(m_ref)))
        assert np.all(np.abs(var[:, g] - v_ref) <= 1e-10 * np.maximum(1.0, kd[:, g]))
    # the Noise component: no cross-covariance, the prior variance is its own
    assert np.all(mean[:, G - 1] == 0.0) and np.all(var[:, G - 1] == 0.7)
    # the means sum to the whole posterior's mean
    full = R.posterior_mean_var(X, terms, CO.NOISE_OBS, y, Xs)[0]
    assert np.max(np.abs(mean.sum(1) - full)) <= 1e-12 * max(1.0, np.max(np.abs(full)))


def test_one_component_is_the_whole_posterior():
    X, Xs, y = inputs(CO.TERMS)
    mean, var, _ = CO.components(X, CO.TERMS, CO.NOISE_OBS, y, Xs, [0] * len(CO.TERMS), 1)
    rm, rv = R.posterior_mean_var(X, CO.TERMS, CO.NOISE_OBS, y, Xs)
    assert np.max(np.abs(mean[:, 0] - rm)) <= 1e-12 * max(1.0, np.max(np.abs(rm)))
    assert np.max(np.abs(var[:, 0] - rv)) <= 1e-12 * np.max(R.kernel_diag(Xs, CO.TERMS))


def test_left_out_terms_and_empty_components():
    X, Xs, y = inputs(CO.TERMS)
    comp = CO.comp_for(CO.TERMS, 3)
    assert comp == [0, 1, 2, -1, -1]
    mean, var, kd = CO.components(X, CO.TERMS, CO.NOISE_OBS, y, Xs, comp, 4)  # component 3 has no terms
    assert np.all(mean[:, 3] == 0.0) and np.all(var[:, 3] == 0.0) and np.all(kd[:, 3] == 0.0)
    # N = 0: the prior
    m0, v0, k0 = CO.components(np.zeros((0, 3)), CO.TERMS, CO.NOISE_OBS, np.zeros(0), Xs, comp, 3)
    assert np.all(m0 == 0.0) and np.array_equal(v0, k0) and np.all(k0[:, :3] == 1.0)
