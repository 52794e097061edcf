"""numpy restatement of the gradient of the Laplace log q (Rasmussen & Williams,
Algorithm 5.1) on tests/laplace_oracle.laplace and oracle.restatement.term_derivative.

With K~ = gram(X, terms, jitter), at the mode: a, f, W, sw = sqrt(W), B = I + sw K~ sw = L L^T,
R = sw B^{-1} sw, rho = (d^3 log p / df^3) / W (Bernoulli tanh(f / 2), Poisson -1, Gaussian 0):

    s2 = (1 - diag B^{-1}) rho / 2              (= diag(Sigma) d^3 log p / 2, Sigma = (K~^{-1} + W)^{-1})
    u  = s2 - R (K~ s2)                         (= (I + W K~)^{-1} s2)
    d log q / d theta_t = 1/2 sum_ij (a_i a_j - R_ij) dK~_ij/dtheta_t + sum_ij u_i dK~_ij/dtheta_t a_j
    d log q / d jitter  = 1/2 (a^T a - tr R) + u^T a

The first sum is the explicit part, the second the implicit part. (R&W print s2 with a minus: their
third derivative is that of -log p through dW/df; scikit-learn and central differences agree with
the sign here.) A term inside a product group is multiplied by the group's other terms, as in
oracle.restatement.logpdf_grad.
"""
import numpy as np
import scipy.linalg

from oracle import restatement as R
from tests import laplace_oracle as LO


def rho(lik, f):
    if lik == LO.BERNOULLI:
        return np.tanh(0.5 * f)
    if lik == LO.POISSON:
        return -np.ones_like(f)
    return np.zeros_like(f)


def term_dk(X, terms, t):
    """dK~/dtheta_t (N x N): term t's derivative times the other terms of its product group."""
    kind, col, param, group = terms[t]
    dK = R.term_derivative(X, kind, col, param)
    for s, (k2, c2, p2, g2) in enumerate(terms):
        if s != t and g2 == group:
            dK = dK * R.term_matrix(X, k2, c2, p2)
    return dK


class GradResult:
    pass


def grad_from(res, X, terms, lik):
    """The gradient at a laplace() result: a GradResult with dparam, djitter, implicit (T + 1: the
    implicit parts of dparam and djitter), the magnitudes scale (T), scale_jitter, implicit_scale
    (T + 1), and u, s2, Rm, dbinv."""
    X = np.asarray(X, dtype=np.float64)
    terms = list(terms)
    N, T = X.shape[0], len(terms)
    a, f, sw, L, K = res.a, res.f, res.sw, res.L, res.K
    Li = scipy.linalg.solve_triangular(L, np.eye(N), lower=True, check_finite=False)  # L^{-1}
    dbinv = np.sum(Li * Li, axis=0)                                                  # diag B^{-1}
    Ls = Li * sw[None, :]                                                             # L^{-1} diag(sw)
    Rm = Ls.T @ Ls
    s2 = 0.5 * (1.0 - dbinv) * rho(lik, f)
    u = s2 - Rm @ (K @ s2)
    g = GradResult()
    g.u, g.s2, g.Rm, g.dbinv = u, s2, Rm, dbinv
    g.dparam, g.implicit = np.zeros(T), np.zeros(T + 1)
    g.scale, g.implicit_scale = np.zeros(T), np.zeros(T + 1)
    E = np.outer(a, a) - Rm
    Ea = np.abs(np.outer(a, a)) + 2.0 * np.abs(np.outer(u, a)) + np.abs(Rm)
    Ua = np.abs(np.outer(u, a))
    for t in range(T):
        dK = term_dk(X, terms, t)
        g.implicit[t] = float(u @ (dK @ a))
        g.dparam[t] = 0.5 * float(np.sum(E * dK)) + g.implicit[t]
        g.scale[t] = 0.5 * float(np.sum(Ea * np.abs(dK)))
        g.implicit_scale[t] = float(np.sum(Ua * np.abs(dK)))
    g.implicit[T] = float(u @ a)
    g.djitter = 0.5 * (float(a @ a) - float(np.trace(Rm))) + g.implicit[T]
    g.scale_jitter = 0.5 * float(np.trace(Ea))
    g.implicit_scale[T] = float(np.sum(np.abs(u * a)))
    g.logq, g.res = res.logq, res
    return g


def laplace_grad(X, terms, jitter, lik, y, lik_param=0.0, **kw):
    """laplace() and the gradient at its result."""
    return grad_from(LO.laplace(X, terms, jitter, lik, y, lik_param, **kw), X, terms, lik)


def diag_sigma_second_route(res):
    """diag Sigma by its definition's other form: K~_ii - |L^{-1} (sw o K~_:i)|^2."""
    V = scipy.linalg.solve_triangular(res.L, res.sw[:, None] * res.K, lower=True, check_finite=False)
    return np.diag(res.K) - np.sum(V * V, axis=0)


_cache = {}


def case(N, terms_name, lik_name):
    """LO.case(N, 1, ...) with its gradient under "grad", computed once and shared."""
    key = (N, terms_name, lik_name)
    if key not in _cache:
        c = dict(LO.case(N, 1, terms_name, lik_name))
        c["grad"] = grad_from(c["res"], c["X"], c["terms"], c["lik"])
        _cache[key] = c
    return _cache[key]
