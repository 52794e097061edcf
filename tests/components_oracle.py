"""CPU recipe for the per-component posteriors, built from oracle.restatement (no GPU):

    L = cholesky_lower(X, terms, noise), z = L \\ y, and per component g with terms_g its terms
    V = L \\ cross_gram(X, Xs, terms_g),  mean_g = V^T z,  var_g = kernel_diag(Xs, terms_g) - sum V^2.

The training covariance uses every term, the cross-covariance and the prior variance the terms
of one component. tests/test_components_oracle.py pins the recipe to a dense solve (no Cholesky)
and to R.posterior_mean_var; tests/test_gpu_components.py compares gaplac_posterior_components
against it. case() generates the GPU tests' inputs (columns as tests/joint_oracle.cols).
"""
import numpy as np
import scipy.linalg

from gaplac_amd._native import CAT, LINEAR, NOISE, OU, SQEXP
from oracle import restatement as R
from tests.joint_oracle import cols

# the issue's term set (every term its own group) and the one with a product group
TERMS = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (LINEAR, 2, 0.5, 3), (NOISE, -1, 0.7, 4)]
TERMS_PROD = [(SQEXP, 0, 1.5, 0), (CAT, 1, 0.0, 0), (OU, 0, 3.0, 1), (LINEAR, 2, 0.5, 2), (NOISE, -1, 0.7, 3)]
NOISE_OBS = 0.1


def comp_for(terms, G):
    """The issue's component maps: G = 5 (G = 4 for the product set): one component per product
    group, the Noise term the last; G = 3: the first three groups, Linear and Noise left out
    (comp = -1); G = 2: the first two groups; G = 1: every term in component 0."""
    groups = [t[3] for t in terms]
    ng = max(groups) + 1
    if G == 1:
        return [0] * len(terms)
    if G == ng:
        return list(groups)
    return [g if g < G else -1 for g in groups]


def terms_of(terms, comp, g):
    return [t for t, c in zip(terms, comp) if c == g]


def components(X, terms, noise, y, Xs, comp, G):
    """(mean[M, G], var[M, G], kdiag[M, G])"""
    X = np.asarray(X, dtype=np.float64)
    Xs = np.asarray(Xs, dtype=np.float64)
    X = X[:, None] if X.ndim == 1 else X
    Xs = Xs[:, None] if Xs.ndim == 1 else Xs
    M = Xs.shape[0]
    mean, var, kd = np.zeros((M, G)), np.zeros((M, G)), np.zeros((M, G))
    if len(X) == 0:
        for g in range(G):
            tg = terms_of(terms, comp, g)
            kd[:, g] = R.kernel_diag(Xs, tg) if tg else 0.0
        return mean, kd.copy(), kd
    L = R.cholesky_lower(X, terms, noise)
    z = scipy.linalg.solve_triangular(L, np.asarray(y, dtype=np.float64), lower=True, check_finite=False)
    for g in range(G):
        tg = terms_of(terms, comp, g)
        if not tg:
            continue  # the zero process
        V = scipy.linalg.solve_triangular(L, R.cross_gram(X, Xs, tg), lower=True, check_finite=False)
        kd[:, g] = R.kernel_diag(Xs, tg)
        mean[:, g] = V.T @ z
        var[:, g] = kd[:, g] - (V * V).sum(0)
    return mean, var, kd


class Case:
    """One (N, G, M) case with its reference, computed once: inputs drawn in the order X, Xs, y."""

    def __init__(self, N, G, M, terms=TERMS, comp=None, seed=None):
        rng = np.random.default_rng(N * 7 + G * 1000 + M if seed is None else seed)
        self.N, self.G, self.M, self.terms = N, G, M, terms
        self.comp = comp_for(terms, G) if comp is None else comp
        self.X = cols(rng, N)
        self.Xs = cols(rng, M)
        self.y = rng.normal(size=N)
        self.mean, self.var, self.kd = components(self.X, terms, NOISE_OBS, self.y, self.Xs, self.comp, G)


def within_bars(mean, var, ref):
    """The bars of tests/test_gpu_posterior.py per component: mean within 1e-9 max(1, max|mean_g|),
    variance within 1e-9 max(1, kdiag_g). Returns (ok, worst mean ratio, worst variance ratio)."""
    rm, rv, kd = ref.mean, ref.var, ref.kd
    if mean.shape[0] == 0 or mean.shape[1] == 0:
        return mean.shape == rm.shape and var.shape == rv.shape, 0.0, 0.0
    bm = 1e-9 * np.maximum(1.0, np.max(np.abs(rm), axis=0))
    em = np.max(np.abs(mean - rm) / bm[None, :])
    ev = np.max(np.abs(var - rv) / (1e-9 * np.maximum(1.0, np.abs(kd))))
    return bool(em <= 1.0 and ev <= 1.0), float(em), float(ev)
