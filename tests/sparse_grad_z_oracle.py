"""CPU recipe for the gradient of the inducing-point bound with respect to the inducing inputs
(gaplac_sparse_elbo_grad_z), built from oracle.restatement (no GPU). With G_uf and G_uu of
tests/sparse_grad_oracle.py's two routes (recomputed here), for inducing point m and column d:

    dZ[m, d] = sum over the terms t with col_t = d of
                   sum_n  G_uf[m, n]  d1 k_t(z_m, x_n)  prod_{s != t in t's group} k_s(z_m, x_n)
               + 2 sum_m' G_uu[m, m'] d1 k_t(z_m, z_m') prod_{s != t in t's group} k_s(z_m, z_m')

d1 k(a, b), the derivative in the first argument: -k (a - b) / l^2 (SQEXP), -k sign(a - b) / l (OU,
sign(0) = 0), b (LINEAR), 0 (CAT, NOISE). woodbury() and dense() return (dZ, scale), both Mz x D:
scale holds the same sums with absolute values, the addend magnitude an entry is judged against
(the entries cancel to about 1e-8 of it).
"""
import numpy as np
import scipy.linalg

from gaplac_amd._native import LINEAR, OU, SQEXP
from oracle import restatement as R
from tests.sparse_oracle import _mats, _tri


def d1_term(Za, Xb, kind, col, param):
    """d k_t(a, b) / da for the rows a of Za and b of Xb (len(Za) x len(Xb))."""
    a, b = Za[:, col], Xb[:, col]
    if kind == LINEAR:
        return np.broadcast_to(b[None, :], (len(a), len(b))).copy()
    if kind not in (SQEXP, OU):
        return np.zeros((len(a), len(b)))
    s = 1.0 / param
    u = (s * a)[:, None] - (s * b)[None, :]
    if kind == SQEXP:
        return -np.exp(-(u * u) * 0.5) * u * s
    return -np.exp(-np.abs(u)) * np.sign(u) * s


def _assemble(X, Z, terms, Guf, Guu):
    dZ = np.zeros(Z.shape)
    scale = np.zeros(Z.shape)
    for t, (kind, col, param, group) in enumerate(terms):
        if kind not in (SQEXP, OU, LINEAR):
            continue
        duf = d1_term(Z, X, kind, col, param)
        duu = d1_term(Z, Z, kind, col, param)
        for s, (k2, c2, p2, g2) in enumerate(terms):
            if s != t and g2 == group:
                duf = duf * R.cross_term_matrix(Z, X, k2, c2, p2)
                duu = duu * R.term_matrix(Z, k2, c2, p2)
        dZ[:, col] += np.sum(Guf * duf, axis=1) + 2.0 * np.sum(Guu * duu, axis=1)
        scale[:, col] += np.sum(np.abs(Guf * duf), axis=1) + 2.0 * np.sum(np.abs(Guu * duu), axis=1)
    return dZ, scale


def woodbury(X, terms, noise, y, Z, jitter):
    X, Z, _ = _mats(X, Z, None)
    y = np.asarray(y, dtype=np.float64)
    Mz = len(Z)
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
    Guf = np.outer(ctil, alpha) + (Linv.T @ (np.eye(Mz) / noise - Sinv)) @ V
    Guu = -0.5 * (np.outer(ctil, ctil) + Linv.T @ (S / noise - 2 * np.eye(Mz) + noise * Sinv) @ Linv)
    return _assemble(X, Z, terms, Guf, Guu)


def dense(X, terms, noise, y, Z, jitter):
    X, Z, _ = _mats(X, Z, None)
    y = np.asarray(y, dtype=np.float64)
    N = len(X)
    Kuf = R.cross_gram(Z, X, terms)
    cf = scipy.linalg.cho_factor(R.gram(Z, terms, jitter), lower=True, check_finite=False)
    B = scipy.linalg.cho_solve(cf, Kuf, check_finite=False)
    cc = scipy.linalg.cho_factor(Kuf.T @ B + noise * np.eye(N), lower=True, check_finite=False)
    alpha = scipy.linalg.cho_solve(cc, y, check_finite=False)
    M = np.outer(alpha, alpha) - scipy.linalg.cho_solve(cc, np.eye(N), check_finite=False) + np.eye(N) / noise
    Guf = B @ M
    return _assemble(X, Z, terms, Guf, -0.5 * Guf @ B.T)
