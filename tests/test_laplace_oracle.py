"""The numpy restatement of the Laplace approximation (tests/laplace_oracle.py) against known
answers (CPU):

- Bernoulli on SqExp(1.5), jitter 0, against scikit-learn's GaussianProcessClassifier(RBF(1.5),
  optimizer=None).log_marginal_likelihood (the same algorithm, R&W 3.1 / 5.1, stopped at 1e-10):
  1e-10 relative.
- Gaussian against the exact logpdf at noise = jitter + variance (the approximation is exact): 1e-12.
- every case: a = grad log p(y | f) at the mode within 1e-12 max(1, max |g|), and log q by a second
  route (slogdet(I + K W) through LU) within 1e-12 relative.
"""
import numpy as np
import pytest

from oracle import restatement as R
from tests import laplace_oracle as LO

SIZES = [1, 5, 127, 129, 300, 700]


@pytest.mark.parametrize("N", [50, 300, 700])
def test_bernoulli_matches_scikit_learn(N):
    from sklearn.gaussian_process import GaussianProcessClassifier
    from sklearn.gaussian_process.kernels import RBF

    X, _, y = LO.data(N, 1, "sqexp", "bernoulli")
    if len(np.unique(y)) < 2:
        pytest.fail("the recipe drew one class only")
    gpc = GaussianProcessClassifier(RBF(1.5), optimizer=None).fit(X[:, :1], y.astype(int))
    want = gpc.log_marginal_likelihood()
    got = LO.laplace(X, LO.SQEXP_TERMS, 0.0, LO.BERNOULLI, y).logq
    print(f"N={N}: oracle {got!r} scikit-learn {want!r} diff {abs(got - want):.3e}")
    assert abs(got - want) <= 1e-10 * max(1.0, abs(want))


@pytest.mark.parametrize("terms_name", ["sqexp", "composite"])
@pytest.mark.parametrize("N", SIZES)
def test_gaussian_is_exact(N, terms_name):
    c = LO.case(N, 1, terms_name, "gaussian")
    want = R.logpdf(c["X"], c["terms"], LO.JITTER + 0.1, c["y"])[0]
    res = c["res"]
    print(f"N={N} {terms_name}: iters {res.iters} diff {abs(res.logq - want):.3e}")
    assert res.converged and res.iters == 2
    assert abs(res.logq - want) <= 1e-12 * max(1.0, abs(want))


@pytest.mark.parametrize("lik_name", ["bernoulli", "poisson", "gaussian"])
@pytest.mark.parametrize("terms_name", ["sqexp", "composite"])
@pytest.mark.parametrize("N", SIZES)
def test_mode_and_second_route(N, terms_name, lik_name):
    c = LO.case(N, 1, terms_name, lik_name)
    res = c["res"]
    assert res.converged
    g = LO.lik_terms(c["lik"], c["lik_param"], c["y"], res.f)[1]
    eg = np.max(np.abs(res.a - g)) / max(1.0, np.max(np.abs(g)))
    lu = LO.logq_by_lu(res, c["lik"], c["lik_param"], c["y"])
    el = abs(res.logq - lu) / max(1.0, abs(lu))
    print(f"N={N} {terms_name} {lik_name}: iters {res.iters} halvings {res.halvings} |a - g| {eg:.3e} LU route {el:.3e}")
    assert eg <= 1e-12
    assert el <= 1e-12


def test_line_search_is_exercised_and_agrees_with_plain_newton():
    """The composite Poisson inputs take halvings; the iteration without them ends at the same log q
    (both stop where the objective's change meets tol = 1e-12 relative, and both are then polished:
    1e-11 leaves room for the two routes' rounding in sums of N = 300 terms)."""
    c = LO.case(300, 1, "composite", "poisson")
    plain = LO.laplace(c["X"], c["terms"], LO.JITTER, c["lik"], c["y"], line_search=False)
    print(f"halvings {c['res'].halvings}; iters {c['res'].iters} against {plain.iters} without")
    assert c["res"].halvings >= 1
    assert plain.converged
    assert abs(plain.logq - c["res"].logq) <= 1e-11 * max(1.0, abs(plain.logq))
