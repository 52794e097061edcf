"""The two CPU routes of tests/sparse_joint_oracle.py (the dense N x N one and the Woodbury one
the HIP entries follow) agree on the joint forms of the inducing-point posterior: AbstractGPs is
not available to pin mean_and_cov / rand / logpdf of posterior(VFE(f(z)), fx, y)(xs, noise_s)
directly, so each route is the other's check. Bar 1e-11 (tests/test_sparse_oracle.py's): the
covariance in units of max(1, max kdiag), the mean and the draws in units of max(1, max |.|),
logpdf relative. On the sizes of tests/test_gpu_sparse_joint.py's parity test (COMPOSITE terms,
noise 0.1, noise_s 0.1, jitter 1e-6 and 1e-2) the routes differ by at most 3.0e-15 (cov), 2.8e-12
(mean), 1.9e-12 (draws) and 3.7e-14 (logpdf), and Sigma* has a condition number <= 166 there; at
noise_s = 0 its smallest eigenvalue is >= 2.5e-5 (that matrix is compared, never factored).
"""
import numpy as np
import pytest

from gaplac_amd._native import CAT, LINEAR, NOISE, OU, SQEXP
from oracle import restatement as R
from tests import joint_oracle as J
from tests import sparse_joint_oracle as SJ
from tests import sparse_oracle as S

COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (LINEAR, 2, 0.5, 3)]
SIZES = [(300, 1, 1), (300, 5, 3), (700, 127, 129), (1000, 129, 128), (513, 128, 127), (129, 129, 130),
         (2000, 257, 257), (600, 64, 513), (400, 300, 1000), (2051, 129, 130)]
BAR = 1e-11


def compare(d, w, kd):
    """d, w: Cases by the two routes on the same inputs."""
    ec = max(np.max(np.abs(d.cov - w.cov)), np.max(np.abs(d.cov0 - w.cov0))) / max(1.0, np.max(kd))
    em = np.max(np.abs(d.mean - w.mean)) / max(1.0, np.max(np.abs(d.mean)))
    ed = np.max(np.abs(d.draws - w.draws)) / max(1.0, np.max(np.abs(d.draws)))
    el = np.max(np.abs(d.lp[0] - w.lp[0]) / np.abs(d.lp[0]))
    print("cov", ec, "mean", em, "draws", ed, "rel logpdf", el)
    assert ec <= BAR and em <= BAR and ed <= BAR and el <= BAR
    assert abs(d.lp[1] - w.lp[1]) <= BAR * np.min(np.abs(d.lp[0]))          # (as the GPU tests judge them)
    assert np.all(np.abs(d.lp[2] - w.lp[2]) <= BAR * np.abs(d.lp[0]))


@pytest.mark.parametrize("jitter", [1e-6, 1e-2])
@pytest.mark.parametrize("N,Mz,Ms", SIZES)
def test_woodbury_route_matches_the_dense_route(N, Mz, Ms, jitter):
    d = SJ.Case(N, Mz, Ms, COMPOSITE, 0.1, jitter, 0.1, route=SJ.dense)
    w = SJ.Case(N, Mz, Ms, COMPOSITE, 0.1, jitter, 0.1, route=SJ.woodbury)
    assert np.array_equal(d.E, w.E) and np.array_equal(d.X, w.X)
    compare(d, w, d.kd)
    # the diagonal at noise_s = 0 is sparse_oracle's marginal variance
    ev = np.max(np.abs(np.diag(w.cov0) - w.var))
    print("max |diag cov0 - var|", ev)
    assert ev <= 1e-12


def test_product_groups_and_noise_term():
    rng = np.random.default_rng(12)
    N, Mz, Ms = 260, 70, 190
    X = np.column_stack([rng.uniform(0, 5, N), rng.normal(size=N)])
    Z = np.column_stack([rng.uniform(0, 5, Mz), rng.normal(size=Mz)])
    Xs = np.column_stack([rng.uniform(0, 5, Ms), rng.normal(size=Ms)])
    terms = [(SQEXP, 0, 1.3, 0), (LINEAR, 1, 0.4, 0), (OU, 0, 2.5, 1), (NOISE, -1, 0.2, 2)]
    y = rng.normal(size=N)
    kd = R.kernel_diag(Xs, terms)
    for noise_s in (0.0, 0.1):
        dm, dS = SJ.dense(X, terms, 0.1, y, Z, 1e-6, Xs, noise_s)
        wm, wS = SJ.woodbury(X, terms, 0.1, y, Z, 1e-6, Xs, noise_s)
        assert np.max(np.abs(dS - wS)) <= BAR * max(1.0, np.max(kd))
        assert np.max(np.abs(dm - wm)) <= BAR * max(1.0, np.max(np.abs(dm)))
    # a NOISE term counts on the diagonal of the test points' own Gram
    assert np.max(np.abs(np.diag(wS) - 0.1 - S.woodbury(X, terms, 0.1, y, Z, 1e-6, Xs)["var"])) <= 1e-12 * np.max(kd)


@pytest.mark.parametrize("N", [129, 300])
def test_inducing_points_at_the_data_are_exact(N):
    # Z = X, jitter 0: Q = K, so the approximate posterior is the exact one, jointly
    rng = np.random.default_rng(N)
    X = S.cols(rng, N)
    y = rng.normal(size=N)
    Xs = S.cols(rng, 40)
    terms = [(OU, 0, 3.0, 0), (CAT, 1, 0.0, 1), (LINEAR, 2, 0.5, 2)]
    kd = R.kernel_diag(Xs, terms)
    for noise_s in (0.0, 0.1):
        rm, rS = J.mean_cov(X, terms, 0.1, y, Xs, noise_s)
        for route in (SJ.dense, SJ.woodbury):
            m, Sg = route(X, terms, 0.1, y, X, 0.0, Xs, noise_s)
            print("mean", np.max(np.abs(m - rm)), "cov / max(1, kdiag)", np.max(np.abs(Sg - rS) / max(1.0, np.max(kd))))
            assert np.max(np.abs(m - rm)) <= 1e-10 * max(1.0, np.max(np.abs(rm)))
            assert np.max(np.abs(Sg - rS)) <= 1e-10 * max(1.0, np.max(kd))
