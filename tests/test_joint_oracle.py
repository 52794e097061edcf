"""The joint-posterior recipe (tests/joint_oracle.py) pinned to scikit-learn's independent
GaussianProcessRegressor.predict(return_cov=True), as tests/test_posterior_oracle.py pins the
marginal one: mean within 1e-10 of max |mean| (>= 1), standard deviations within 1e-7; the
covariance entries take the same 1e-7 (they are at most 1 here, so an entry moves no more than
twice what a standard deviation moves). No GPU needed."""
import numpy as np
import pytest
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import RBF, Matern

from gaplac_amd._native import OU, SQEXP
from oracle import restatement as R
from tests import joint_oracle as J

N, M = 60, 40


def compare(k, terms, X, Xs, Xk, Xsk):
    rng = np.random.default_rng(8)
    y = rng.normal(size=N)
    gpr = GaussianProcessRegressor(kernel=k, alpha=0.1, optimizer=None, normalize_y=False).fit(Xk, y)
    m_ref, c_ref = gpr.predict(Xsk, return_cov=True)
    m, S = J.mean_cov(X, terms, 0.1, y, Xs, 0.0)
    assert np.max(np.abs(m - m_ref)) <= 1e-10 * max(1.0, np.max(np.abs(m_ref)))
    assert np.max(np.abs(S - c_ref)) <= 1e-7
    assert np.max(np.abs(np.sqrt(np.maximum(np.diag(S), 0)) - np.sqrt(np.maximum(np.diag(c_ref), 0)))) <= 1e-7
    assert np.array_equal(S, S.T)
    # noise_s only moves the diagonal
    S1 = J.mean_cov(X, terms, 0.1, y, Xs, 0.25)[1]
    assert np.max(np.abs(S1 - S - 0.25 * np.eye(M))) <= 1e-15 * 2
    # the marginals are the restatement's
    rm, rv = R.posterior_mean_var(X, terms, 0.1, y, Xs)
    assert np.max(np.abs(m - rm)) <= 1e-12 and np.max(np.abs(np.diag(S) - rv)) <= 1e-12


@pytest.mark.parametrize("kind,l", [(SQEXP, 1.5), (OU, 2.0)])
def test_mean_and_cov_match_sklearn(kind, l):
    rng = np.random.default_rng(3)
    X = rng.uniform(-5, 5, (N, 1))
    Xs = np.vstack([rng.uniform(-6, 6, (M - 2, 1)), X[:2]])  # two test points on training inputs
    k = RBF(length_scale=l) if kind == SQEXP else Matern(length_scale=l, nu=0.5)
    compare(k, [(kind, 0, l, 0)], X, Xs, X, Xs)


def test_sum_kernel_matches_sklearn():
    rng = np.random.default_rng(4)
    x, xs = rng.uniform(0, 10, N), rng.uniform(0, 10, M)
    compare(RBF(1.3) + Matern(3.0, nu=0.5), [(SQEXP, 0, 1.3, 0), (OU, 1, 3.0, 1)], np.column_stack([x, x]),
            np.column_stack([xs, xs]), x[:, None], xs[:, None])


def test_draws_and_logpdf_follow_the_formula():
    rng = np.random.default_rng(5)
    X, Xs = rng.uniform(-5, 5, (N, 1)), rng.uniform(-5, 5, (M, 1))
    y = rng.normal(size=N)
    m, S = J.mean_cov(X, [(SQEXP, 0, 1.5, 0)], 0.1, y, Xs, 0.1)
    Z = rng.normal(size=(M, 3))
    D = J.draws(m, S, Z)
    lp, ld, q = J.logpdf(m, S, D)
    assert np.max(np.abs(q - (Z * Z).sum(0))) <= 1e-9 * np.max((Z * Z).sum(0))
    assert abs(ld - np.linalg.slogdet(S)[1]) <= 1e-10 * abs(ld)
    Sinv = np.linalg.inv(S)
    for r in range(3):
        d = D[:, r] - m
        assert abs(lp[r] + (M * np.log(2 * np.pi) + ld + d @ Sinv @ d) / 2) <= 1e-9 * abs(lp[r])
