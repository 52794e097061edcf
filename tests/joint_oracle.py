"""CPU recipe for the joint posterior at test points, built from oracle.restatement (no GPU):

    L = cholesky_lower(X, terms, noise), V = L \\ K(X, Xs), z = L \\ y, m = V^T z,
    Sigma* = gram(Xs, terms, noise_s) - V^T V, L* = cholesky(Sigma*),
    draws = m + L* Z, logpdf_r = -(M log 2pi + logdet Sigma* + |L*^{-1}(Ys[:, r] - m)|^2) / 2.

tests/test_joint_oracle.py pins it to scikit-learn; tests/test_gpu_joint.py compares the HIP
entries against it. case() generates the GPU tests' inputs in the order the issue fixes.
"""
import numpy as np
import scipy.linalg

from oracle import restatement as R


def mean_cov(X, terms, noise, y, Xs, noise_s):
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    Xs = np.asarray(Xs, dtype=np.float64).reshape(len(Xs), -1)
    L = R.cholesky_lower(X, terms, noise)
    V = scipy.linalg.solve_triangular(L, R.cross_gram(X, Xs, terms), lower=True, check_finite=False)
    z = scipy.linalg.solve_triangular(L, np.asarray(y, dtype=np.float64), lower=True, check_finite=False)
    return V.T @ z, R.gram(Xs, terms, noise_s) - V.T @ V


def draws(m, S, Z):
    return m[:, None] + np.linalg.cholesky(S) @ Z


def logpdf(m, S, Ys):
    """(logpdf[R], logdet, quad[R])"""
    Ls = np.linalg.cholesky(S)
    W = scipy.linalg.solve_triangular(Ls, Ys - m[:, None], lower=True, check_finite=False)
    quad = (W * W).sum(0)
    logdet = 2.0 * np.sum(np.log(np.diag(Ls)))
    return -((len(m) * R.LOG2PI + logdet) + quad) / 2, logdet, quad


def cols(rng, n):
    # (tests/test_gpu_multi.py's cols)
    return np.column_stack([rng.uniform(0, 10, n), rng.integers(0, 40, n).astype(float), rng.normal(size=n)])


class Case:
    """One (N, M) case of the GPU tests with its reference, computed once: inputs drawn in the
    fixed order X, Xs, y, Z, then Ys = draws + 0.3 * noise, all for noise_s = 0.1; the covariance
    reference also for noise_s = 0."""

    def __init__(self, N, M, terms, noise=0.1, noise_s=0.1, R_=5):
        rng = np.random.default_rng(N * 7 + M)
        self.N, self.M, self.terms, self.noise, self.noise_s = N, M, terms, noise, noise_s
        self.X = cols(rng, N)
        self.Xs = cols(rng, M)
        self.y = rng.normal(size=N)
        self.Z = rng.normal(size=(M, R_))
        self.mean, self.cov = mean_cov(self.X, terms, noise, self.y, self.Xs, noise_s)
        self.cov0 = mean_cov(self.X, terms, noise, self.y, self.Xs, 0.0)[1]
        self.draws = draws(self.mean, self.cov, self.Z)
        self.Ys = self.draws + 0.3 * rng.normal(size=(M, R_))
        self.lp = logpdf(self.mean, self.cov, self.Ys)
        self.kd = R.kernel_diag(self.Xs, terms)
