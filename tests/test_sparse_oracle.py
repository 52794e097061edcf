"""The two CPU routes of tests/sparse_oracle.py (the dense N x N one and the Woodbury one the HIP
entries follow) agree: AbstractGPs is not available to pin elbo / dtc / posterior(VFE) directly,
so each route is the other's check. Bars: 1e-11 relative in dtc and elbo, 1e-11 of
max(1, max |mean|) in the mean and of max(1, max kdiag) in the variance; the largest
disagreements seen on these inputs are 6.7e-14, 2.9e-12 and 5.7e-16, so the
GPU bar of 1e-9 leaves more than 300x over what the reference itself is good for.
"""
import numpy as np
import pytest

from gaplac_amd._native import CAT, LINEAR, NOISE, OU, SQEXP
from oracle import restatement as R
from tests import sparse_oracle as S

COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (LINEAR, 2, 0.5, 3)]
SIZES = [(300, 1), (300, 5), (700, 127), (1000, 129), (2000, 257), (513, 513)]
BAR = 1e-11


def compare(d, w, kd):
    rel = max(abs(d[k] - w[k]) / abs(d[k]) for k in ("dtc", "elbo"))
    em = np.max(np.abs(d["mean"] - w["mean"])) / max(1.0, np.max(np.abs(d["mean"])))
    ev = np.max(np.abs(d["var"] - w["var"])) / max(1.0, np.max(kd))
    print("rel dtc/elbo", rel, "mean", em, "var", ev)
    assert rel <= BAR and em <= BAR and ev <= BAR
    for k in ("logdet", "quad", "trace"):  # (as the GPU tests judge them: against |dtc|)
        assert abs(d[k] - w[k]) <= BAR * abs(d["dtc"]), k


@pytest.mark.parametrize("jitter", [1e-6, 1e-2])
@pytest.mark.parametrize("N,Mz", SIZES)
def test_woodbury_route_matches_the_dense_route(N, Mz, jitter):
    c = S.Case(N, Mz, 64, COMPOSITE, 0.1, jitter, route=S.dense)
    w = S.woodbury(c.X, COMPOSITE, 0.1, c.y, c.Z, jitter, c.Xs)
    compare(c.ref, w, c.kd)
    assert c.ref["trace"] >= 0 and c.ref["elbo"] <= c.ref["dtc"]


def test_product_groups_and_noise_term():
    rng = np.random.default_rng(12)
    N, Mz, Ms = 260, 70, 190
    X = np.column_stack([rng.uniform(0, 5, N), rng.normal(size=N)])
    Z = np.column_stack([rng.uniform(0, 5, Mz), rng.normal(size=Mz)])
    Xs = np.column_stack([rng.uniform(0, 5, Ms), rng.normal(size=Ms)])
    terms = [(SQEXP, 0, 1.3, 0), (LINEAR, 1, 0.4, 0), (OU, 0, 2.5, 1), (NOISE, -1, 0.2, 2)]
    y = rng.normal(size=N)
    compare(S.dense(X, terms, 0.1, y, Z, 1e-6, Xs), S.woodbury(X, terms, 0.1, y, Z, 1e-6, Xs), R.kernel_diag(Xs, terms))


@pytest.mark.parametrize("N", [129, 300])
def test_inducing_points_at_the_data_are_exact(N):
    # Z = X, jitter 0: Q = K, so dtc = elbo = the exact logpdf and the posterior is the exact one
    rng = np.random.default_rng(N)
    X = S.cols(rng, N)
    y = rng.normal(size=N)
    Xs = S.cols(rng, 40)
    terms = [(OU, 0, 3.0, 0), (CAT, 1, 0.0, 1), (LINEAR, 2, 0.5, 2)]
    lp = R.logpdf(X, terms, 0.1, y)[0]
    rm, rv = R.posterior_mean_var(X, terms, 0.1, y, Xs)
    for route in (S.dense, S.woodbury):
        r = route(X, terms, 0.1, y, X, 0.0, Xs)
        assert abs(r["dtc"] - lp) <= 1e-11 * abs(lp) and abs(r["elbo"] - lp) <= 1e-10 * abs(lp)
        assert np.max(np.abs(r["mean"] - rm)) <= 1e-10 * max(1.0, np.max(np.abs(rm)))
        assert np.max(np.abs(r["var"] - rv)) <= 1e-10 * max(1.0, np.max(R.kernel_diag(Xs, terms)))
