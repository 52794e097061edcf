"""CPU recipe for the joint forms of the inducing-point (VFE) posterior at test points, built on
tests/sparse_oracle.py and tests/joint_oracle.py (no GPU). AbstractGPs is not available to pin
them, so the formulas of include/gaplac.h are the contract and two independent routes are kept:

    dense:    Q = K(.,Z) (Kuu + jitter I)^{-1} K(Z,.), C = Q(X,X) + noise I factored by LAPACK:
              m = Q(xs,X) C^{-1} y, Sigma* = gram(Xs, noise_s) - Q(xs,X) C^{-1} Q(X,xs)
    woodbury: Kuu + jitter I = L L^T, V = L^{-1} K(Z,X), A = L^{-1} K(Z,Xs), S = noise I + V V^T =
              L_S L_S^T, u = L_S^{-1} V y, B = L_S^{-1} A: m = B^T u,
              Sigma* = gram(Xs, noise_s) - A^T A + noise B^T B     (the arithmetic of the HIP entries)

Draws and logpdf come from joint_oracle.draws / .logpdf on (m, Sigma*).
tests/test_sparse_joint_oracle.py pins one route to the other; tests/test_gpu_sparse_joint.py
compares the HIP entries against dense for N <= 2000 and woodbury above. Case generates the inputs
as sparse_oracle.Case does (X, Z, y, Xs from default_rng(N * 7 + Mz)), then E (Ms x 5) and
Ys = draws + 0.3 * normal from default_rng(N * 7 + Mz + 1).
"""
import numpy as np
import scipy.linalg

from oracle import restatement as R
from tests import joint_oracle as J
from tests import sparse_oracle as S


def dense(X, terms, noise, y, Z, jitter, Xs, noise_s):
    """(mean, Sigma*) by the N x N route."""
    X, Z, Xs = S._mats(X, Z, Xs)
    y = np.asarray(y, dtype=np.float64)
    L = R.cholesky_lower(Z, terms, jitter)
    V = S._tri(L, R.cross_gram(Z, X, terms))  # Mz x N
    A = S._tri(L, R.cross_gram(Z, Xs, terms))  # Mz x Ms
    C = V.T @ V + noise * np.eye(len(X))
    Qsx = A.T @ V
    cf = scipy.linalg.cho_factor(C, lower=True, check_finite=False)
    mean = Qsx @ scipy.linalg.cho_solve(cf, y, check_finite=False)
    W = S._tri(np.tril(cf[0]), Qsx.T)  # N x Ms
    return mean, R.gram(Xs, terms, noise_s) - W.T @ W


def woodbury(X, terms, noise, y, Z, jitter, Xs, noise_s):
    """(mean, Sigma*) by the Mz x Mz route."""
    X, Z, Xs = S._mats(X, Z, Xs)
    y = np.asarray(y, dtype=np.float64)
    L = R.cholesky_lower(Z, terms, jitter)
    V = S._tri(L, R.cross_gram(Z, X, terms))
    Ls = np.linalg.cholesky(noise * np.eye(len(Z)) + V @ V.T)
    u = S._tri(Ls, V @ y)
    A = S._tri(L, R.cross_gram(Z, Xs, terms))
    B = S._tri(Ls, A)
    return B.T @ u, R.gram(Xs, terms, noise_s) - A.T @ A + noise * (B.T @ B)


class Case:
    """One (N, Mz, Ms) case with its reference, computed once by `route` (default: dense up to
    N = 2000, woodbury above): mean, cov (noise_s), cov0 (noise_s = 0), and for noise_s the draws
    of E, the held-out Ys and their (logpdf, logdet, quad)."""

    def __init__(self, N, Mz, Ms, terms, noise=0.1, jitter=1e-6, noise_s=0.1, route=None, R_=5):
        base = S.Case(N, Mz, Ms, terms, noise, jitter, route=S.woodbury)
        self.N, self.Mz, self.Ms, self.terms = N, Mz, Ms, terms
        self.noise, self.jitter, self.noise_s = noise, jitter, noise_s
        self.X, self.Z, self.y, self.Xs, self.kd = base.X, base.Z, base.y, base.Xs, base.kd
        self.var = base.ref["var"]  # sparse_oracle's marginal variance (latent: noise_s = 0)
        rng = np.random.default_rng(N * 7 + Mz + 1)
        self.E = rng.normal(size=(Ms, R_))
        route = route or (dense if N <= 2000 else woodbury)
        self.mean, self.cov = route(self.X, terms, noise, self.y, self.Z, jitter, self.Xs, noise_s)
        self.cov0 = route(self.X, terms, noise, self.y, self.Z, jitter, self.Xs, 0.0)[1]
        self.draws = J.draws(self.mean, self.cov, self.E)
        self.Ys = self.draws + 0.3 * rng.normal(size=(Ms, R_))
        self.lp = J.logpdf(self.mean, self.cov, self.Ys)
