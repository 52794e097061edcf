"""The restatement of the Laplace gradient (tests/laplace_grad_oracle.py) pinned four ways, none of
them its own closed form. No GPU needed.

1. Central differences of laplace().logq in every parameter and in the jitter, within 1e-6 of the
   scale (tests/test_grad_oracle.py's bar; observed 8.2e-10).
2. scikit-learn's GaussianProcessClassifier.log_marginal_likelihood(eval_gradient=True) for
   Bernoulli with an RBF kernel, within 1e-8 of |ref| + scale (observed 1.6e-15 relative). Its
   gradient is in log l: ours times l.
3. oracle.restatement.logpdf_grad at noise = jitter + variance under the Gaussian likelihood, within
   1e-10 of the scale, the implicit parts exactly 0.
4. diag Sigma by a second route, K~_ii - |L^{-1} (sw o K~_:i)|^2, within 1e-10.
"""
import numpy as np
import pytest

from gaplac_amd._native import CAT
from oracle import restatement as R
from tests import laplace_grad_oracle as GO
from tests import laplace_oracle as LO

FD_CASES = [(N, tn, ln) for N in (60, 300) for tn in ("sqexp", "composite") for ln in ("bernoulli", "poisson", "gaussian")]


def _logq(X, terms, jitter, c):
    return LO.laplace(X, terms, jitter, c["lik"], c["y"], c["lik_param"]).logq


@pytest.mark.parametrize("N,terms_name,lik_name", FD_CASES)
def test_gradient_matches_central_differences(N, terms_name, lik_name):
    X, _, y = LO.data(N, 1, terms_name, lik_name)
    terms = LO.TERM_SETS[terms_name]
    lik, param = LO.LIKS[lik_name]
    c = dict(lik=lik, y=y, lik_param=param)
    g = GO.laplace_grad(X, terms, LO.JITTER, lik, y, param)
    worst = 0.0
    for t, (kind, col, p, grp) in enumerate(terms):
        if kind == CAT:
            assert g.dparam[t] == 0.0 and g.implicit[t] == 0.0
            continue
        h = 1e-5 * p
        tp, tm = [list(x) for x in terms], [list(x) for x in terms]
        tp[t][2] += h
        tm[t][2] -= h
        fd = (_logq(X, [tuple(x) for x in tp], LO.JITTER, c) - _logq(X, [tuple(x) for x in tm], LO.JITTER, c)) / (2 * h)
        floor = 10 * 2.2e-16 * max(1.0, abs(g.logq)) / h  # rounding of the difference
        err = abs(g.dparam[t] - fd)
        worst = max(worst, err / (abs(fd) + g.scale[t]))
        assert err <= 1e-6 * (abs(fd) + g.scale[t]) + floor, (t, g.dparam[t], fd)
    # the jitter, at a value that leaves room for a central difference
    J = 1e-3
    gj = GO.laplace_grad(X, terms, J, lik, y, param)
    h = 1e-6
    fd = (_logq(X, terms, J + h, c) - _logq(X, terms, J - h, c)) / (2 * h)
    floor = 10 * 2.2e-16 * max(1.0, abs(gj.logq)) / h
    err = abs(gj.djitter - fd)
    worst = max(worst, err / (abs(fd) + gj.scale_jitter))
    print(f"N={N} {terms_name} {lik_name}: worst error {worst:.3e} of the scale")
    assert err <= 1e-6 * (abs(fd) + gj.scale_jitter) + floor, (gj.djitter, fd)


@pytest.mark.parametrize("N", [50, 200])
def test_bernoulli_rbf_matches_scikit_learn(N):
    import sklearn.gaussian_process as gpc
    from sklearn.gaussian_process.kernels import RBF

    X, _, y = LO.data(N, 1, "sqexp", "bernoulli")
    l = 1.5
    terms = [(1, 0, l, 0)]
    g = GO.laplace_grad(X, terms, 0.0, LO.BERNOULLI, y, max_iter=200, tol=1e-14)
    m = gpc.GaussianProcessClassifier(kernel=RBF(l), optimizer=None, max_iter_predict=200).fit(X[:, :1], y)
    lml, dl = m.log_marginal_likelihood(np.log([l]), eval_gradient=True)
    ours = g.dparam[0] * l
    print(f"N={N}: lml {lml!r} ours {g.logq!r}; gradient {dl[0]!r} ours {ours!r}")
    assert abs(g.logq - lml) <= 1e-8 * max(1.0, abs(lml))
    assert abs(ours - dl[0]) <= 1e-8 * (abs(dl[0]) + g.scale[0] * l)


@pytest.mark.parametrize("N,terms_name", [(60, "sqexp"), (300, "composite")])
def test_gaussian_likelihood_is_the_exact_gradient(N, terms_name):
    X, _, y = LO.data(N, 1, terms_name, "gaussian")
    terms = LO.TERM_SETS[terms_name]
    g = GO.laplace_grad(X, terms, LO.JITTER, LO.GAUSSIAN, y, 0.1)
    lp, _, dp, dn = R.logpdf_grad(X, terms, LO.JITTER + 0.1, y)
    assert np.all(g.implicit == 0.0)
    assert abs(g.logq - lp) <= 1e-10 * max(1.0, abs(lp))
    assert np.all(np.abs(g.dparam - dp) <= 1e-10 * (np.abs(dp) + g.scale))
    assert abs(g.djitter - dn) <= 1e-10 * (abs(dn) + g.scale_jitter)


@pytest.mark.parametrize("N,terms_name,lik_name", [(60, "sqexp", "bernoulli"), (300, "composite", "poisson")])
def test_diag_sigma_by_a_second_route(N, terms_name, lik_name):
    c = GO.case(N, terms_name, lik_name)
    res, g = c["res"], c["grad"]
    first = (1.0 - g.dbinv) / res.W  # W diag Sigma = 1 - diag B^{-1}
    second = GO.diag_sigma_second_route(res)
    assert np.max(np.abs(first - second)) <= 1e-10 * max(1.0, np.max(np.abs(second)))
