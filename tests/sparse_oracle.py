"""CPU recipe for the inducing-point (VFE) approximation, built from oracle.restatement (no GPU).
AbstractGPs is not available to pin it, so the formulas of include/gaplac.h are the contract and
two independent routes to them are kept:

    dense:    Q = K(X,Z) (Kuu + jitter I)^{-1} K(Z,X) formed at N x N, C = Q + noise I factored by
              LAPACK: dtc = log N(y | 0, C), trace = sum(kdiag(X) - diag Q), elbo = dtc -
              trace / (2 noise), mean = Q(xs,X) C^{-1} y, var = kdiag(xs) - Q(xs,X) C^{-1} Q(X,xs)
    woodbury: Kuu + jitter I = L L^T, V = L^{-1} K(Z,X), S = noise I + V V^T = L_S L_S^T, u =
              L_S^{-1} V y: logdet = (N - Mz) log noise + 2 sum log diag L_S, quad = (y.y - u.u) /
              noise, mean_j = (L_S^{-1} a_j) . u, var_j = kdiag - |a_j|^2 + noise |L_S^{-1} a_j|^2

tests/test_sparse_oracle.py pins one to the other; tests/test_gpu_sparse.py compares the HIP
entries against dense for N <= 2000 and woodbury above. case() generates the inputs in the fixed
order X, Z, y, Xs.
"""
import numpy as np
import scipy.linalg

from oracle import restatement as R
from tests.joint_oracle import cols


def _mats(X, Z, Xs):
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    Z = np.asarray(Z, dtype=np.float64).reshape(len(Z), -1)
    Xs = None if Xs is None else np.asarray(Xs, dtype=np.float64).reshape(len(Xs), -1)
    return X, Z, Xs


def _tri(L, B):
    return scipy.linalg.solve_triangular(L, B, lower=True, check_finite=False)


def dense(X, terms, noise, y, Z, jitter, Xs=None):
    """dict(elbo, dtc, trace, logdet, quad[, mean, var]) by the N x N route."""
    X, Z, Xs = _mats(X, Z, Xs)
    y = np.asarray(y, dtype=np.float64)
    L = R.cholesky_lower(Z, terms, jitter)
    V = _tri(L, R.cross_gram(Z, X, terms))  # Mz x N
    Q = V.T @ V
    C = Q + noise * np.eye(len(X))
    dtc, logdet, quad = R.logpdf_from_cov(C, y)
    trace = float(np.sum(R.kernel_diag(X, terms) - np.diag(Q)))
    out = dict(elbo=dtc - trace / (2 * noise), dtc=dtc, trace=trace, logdet=logdet, quad=quad)
    if Xs is not None:
        A = _tri(L, R.cross_gram(Z, Xs, terms))  # Mz x Ms
        Qsx = A.T @ V
        cf = scipy.linalg.cho_factor(C, lower=True, check_finite=False)
        out["mean"] = Qsx @ scipy.linalg.cho_solve(cf, y, check_finite=False)
        W = _tri(np.tril(cf[0]), Qsx.T)
        out["var"] = R.kernel_diag(Xs, terms) - np.sum(W * W, axis=0)
    return out


def woodbury(X, terms, noise, y, Z, jitter, Xs=None):
    """The same dict by the Mz x Mz route (the arithmetic of the HIP entries)."""
    X, Z, Xs = _mats(X, Z, Xs)
    y = np.asarray(y, dtype=np.float64)
    N, Mz = len(X), len(Z)
    L = R.cholesky_lower(Z, terms, jitter)
    V = _tri(L, R.cross_gram(Z, X, terms))
    Ls = np.linalg.cholesky(noise * np.eye(Mz) + V @ V.T)
    u = _tri(Ls, V @ y)
    logdet = (N - Mz) * np.log(noise) + 2.0 * np.sum(np.log(np.diag(Ls)))
    quad = (float(y @ y) - float(u @ u)) / noise
    dtc = -((N * R.LOG2PI + logdet) + quad) / 2
    trace = float(np.sum(R.kernel_diag(X, terms) - np.sum(V * V, axis=0)))
    out = dict(elbo=dtc - trace / (2 * noise), dtc=dtc, trace=trace, logdet=float(logdet), quad=quad, u=u)
    if Xs is not None:
        A = _tri(L, R.cross_gram(Z, Xs, terms))
        Cj = _tri(Ls, A)
        out["mean"] = Cj.T @ u
        out["var"] = R.kernel_diag(Xs, terms) - np.sum(A * A, axis=0) + noise * np.sum(Cj * Cj, axis=0)
    return out


class Case:
    """One (N, Mz, Ms) case: inputs drawn in the fixed order X, Z, y, Xs from
    default_rng(N * 7 + Mz); the reference by `route` (default: dense up to N = 2000, woodbury
    above), computed once."""

    def __init__(self, N, Mz, Ms, terms, noise=0.1, jitter=1e-6, route=None):
        rng = np.random.default_rng(N * 7 + Mz)
        self.N, self.Mz, self.Ms, self.terms, self.noise, self.jitter = N, Mz, Ms, terms, noise, jitter
        self.X = cols(rng, N)
        self.Z = cols(rng, Mz)
        self.y = rng.normal(size=N)
        self.Xs = cols(rng, Ms)
        route = route or (dense if N <= 2000 else woodbury)
        self.ref = route(self.X, terms, noise, self.y, self.Z, jitter, self.Xs)
        self.kd = R.kernel_diag(self.Xs, terms)
