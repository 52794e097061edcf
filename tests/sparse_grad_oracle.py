"""CPU recipe for the gradient of the inducing-point bound (gaplac_sparse_elbo_grad), built from
oracle.restatement (no GPU). The bound is tests/sparse_oracle.py's; its gradient with respect to
y, the term parameters, the observation variance and jitter by two routes:

    woodbury: the arithmetic of include/gaplac.h: c = S^{-1} w, alpha = (y - V^T c) / noise,
              ctil = L^{-T} c, Phi = I / noise - S^{-1}, W' = L^{-T} Phi, G_uf = ctil alpha^T + W' V,
              G_uu = -(ctil ctil^T + L^{-T} (S / noise - 2 I + noise S^{-1}) L^{-1}) / 2
    dense:    C = Q + noise I at N x N, alpha = C^{-1} y, M = alpha alpha^T - C^{-1} + I / noise,
              B = (Kuu + jitter I)^{-1} Kuf, G_uf = B M, G_uu = -B M B^T / 2,
              dnoise = (alpha^T alpha - tr C^{-1}) / 2 + trace / (2 noise^2)

Both return dict(elbo, dy, dparam, dnoise, djitter, scale): scale[t] is the addend magnitude
|diag addend| + sum |G_uf o dKuf| + sum |G_uu o dKuu| a dparam entry is judged against (the
entries cancel far below it). tests/test_sparse_grad_oracle.py pins one route to the other and
the dense one to central differences of the bound.
"""
import numpy as np
import scipy.linalg

from gaplac_amd._native import CAT, LINEAR, NOISE, OU, SQEXP
from oracle import restatement as R
from tests.sparse_oracle import _mats, _tri


def cross_term_derivative(Za, Xb, kind, col, param):
    """dk_t(z_m, x_n)/dparam_t (len(Za) x len(Xb)); a NOISE term is 0 across point sets."""
    if kind in (NOISE, CAT):
        return np.zeros((len(Za), len(Xb)))
    if kind == LINEAR:
        return np.ones((len(Za), len(Xb)))
    s = 1.0 / param
    u = (s * Za[:, col])[:, None] - (s * Xb[:, col])[None, :]
    if kind == SQEXP:
        return np.exp(-(u * u) * 0.5) * (u * u) / param
    a = np.abs(u)
    return np.exp(-a) * a / param


def _diag_k(X, kind, col, param):
    if kind == NOISE:
        return np.full(len(X), float(param))
    if kind == LINEAR:
        return X[:, col] * X[:, col] + param
    return np.ones(len(X))


def derivative_blocks(X, Z, terms):
    """Per term t: (sum_n dk(x_n, x_n)/dtheta_t, dK(Z, X)/dtheta_t, dK(Z)/dtheta_t), each times
    the other terms of t's product group."""
    out = []
    for t, (kind, col, param, group) in enumerate(terms):
        dd = np.ones(len(X)) if kind in (LINEAR, NOISE) else np.zeros(len(X))
        duf = cross_term_derivative(Z, X, kind, col, param)
        duu = R.term_derivative(Z, kind, col, param)
        for s, (k2, c2, p2, g2) in enumerate(terms):
            if s != t and g2 == group:
                dd = dd * _diag_k(X, k2, c2, p2)
                duf = duf * R.cross_term_matrix(Z, X, k2, c2, p2)
                duu = duu * R.term_matrix(Z, k2, c2, p2)
        out.append((float(np.sum(dd)), duf, duu))
    return out


def _assemble(X, Z, terms, noise, Guf, Guu):
    dparam = np.zeros(len(terms))
    scale = np.zeros(len(terms))
    for t, (dd, duf, duu) in enumerate(derivative_blocks(X, Z, terms)):
        dparam[t] = -dd / (2 * noise) + float(np.sum(Guf * duf)) + float(np.sum(Guu * duu))
        scale[t] = abs(dd / (2 * noise)) + float(np.sum(np.abs(Guf * duf))) + float(np.sum(np.abs(Guu * duu)))
    return dparam, scale


def woodbury(X, terms, noise, y, Z, jitter):
    X, Z, _ = _mats(X, Z, None)
    y = np.asarray(y, dtype=np.float64)
    N, Mz = len(X), len(Z)
    L = R.cholesky_lower(Z, terms, jitter)
    V = _tri(L, R.cross_gram(Z, X, terms))
    S = noise * np.eye(Mz) + V @ V.T
    Ls = np.linalg.cholesky(S)
    u = _tri(Ls, V @ y)
    c = scipy.linalg.solve_triangular(Ls, u, lower=True, trans="T", check_finite=False)
    alpha = (y - V.T @ c) / noise
    Linv = _tri(L, np.eye(Mz))
    Lsinv = _tri(Ls, np.eye(Mz))
    Sinv = Lsinv.T @ Lsinv
    ctil = Linv.T @ c
    Phi = np.eye(Mz) / noise - Sinv
    Guf = np.outer(ctil, alpha) + (Linv.T @ Phi) @ V
    Guu = -0.5 * (np.outer(ctil, ctil) + Linv.T @ (S / noise - 2 * np.eye(Mz) + noise * Sinv) @ Linv)
    logdet = (N - Mz) * np.log(noise) + 2.0 * np.sum(np.log(np.diag(Ls)))
    quad = (float(y @ y) - float(u @ u)) / noise
    trace = float(np.sum(R.kernel_diag(X, terms) - np.sum(V * V, axis=0)))
    elbo = -((N * R.LOG2PI + logdet) + quad) / 2 - trace / (2 * noise)
    dparam, scale = _assemble(X, Z, terms, noise, Guf, Guu)
    dnoise = 0.5 * (float(alpha @ alpha) - (N - Mz + noise * np.trace(Sinv)) / noise) + trace / (2 * noise * noise)
    return dict(elbo=float(elbo), dy=-alpha, dparam=dparam, dnoise=float(dnoise), djitter=float(np.trace(Guu)),
                scale=scale)


def dense(X, terms, noise, y, Z, jitter):
    X, Z, _ = _mats(X, Z, None)
    y = np.asarray(y, dtype=np.float64)
    N, Mz = len(X), len(Z)
    Kuu = R.gram(Z, terms, jitter)
    Kuf = R.cross_gram(Z, X, terms)
    cf = scipy.linalg.cho_factor(Kuu, lower=True, check_finite=False)
    B = scipy.linalg.cho_solve(cf, Kuf, check_finite=False)
    Q = Kuf.T @ B
    C = Q + noise * np.eye(N)
    dtc, _, _ = R.logpdf_from_cov(C, y)
    cc = scipy.linalg.cho_factor(C, lower=True, check_finite=False)
    alpha = scipy.linalg.cho_solve(cc, y, check_finite=False)
    Cinv = scipy.linalg.cho_solve(cc, np.eye(N), check_finite=False)
    M = np.outer(alpha, alpha) - Cinv + np.eye(N) / noise
    Guf = B @ M
    Guu = -0.5 * Guf @ B.T
    trace = float(np.sum(R.kernel_diag(X, terms) - np.diag(Q)))
    dparam, scale = _assemble(X, Z, terms, noise, Guf, Guu)
    dnoise = 0.5 * (float(alpha @ alpha) - float(np.trace(Cinv))) + trace / (2 * noise * noise)
    return dict(elbo=float(dtc - trace / (2 * noise)), dy=-alpha, dparam=dparam, dnoise=float(dnoise),
                djitter=float(np.trace(Guu)), scale=scale)
