"""The two CPU routes to the gradient of the inducing-point bound (tests/sparse_grad_oracle.py)
pinned to each other at 1e-11 of the scales the GPU tests judge by, and the dense route pinned
to central differences of tests.sparse_oracle.woodbury's elbo: dparam, dnoise and dy at 1e-6 of
the addend magnitude (tests/test_grad_oracle.py's bar) at jitter = 1e-6, djitter at jitter = 1e-2
(at 1e-6 no step is both inside the truncation and above the rounding of the difference). No GPU
needed.
"""
import numpy as np
import pytest

from gaplac_amd._native import CAT, LINEAR, NOISE, OU, SQEXP
from tests import sparse_grad_oracle as G
from tests import sparse_oracle as S

COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (LINEAR, 2, 0.5, 3)]
PRODUCT = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 0), (CAT, 1, 0.0, 1), (LINEAR, 2, 0.5, 1), (NOISE, 0, 0.05, 2)]
SHAPES = [(300, 1, 1e-6), (5, 129, 1e-6), (129, 127, 1e-6), (300, 5, 1e-2), (700, 127, 1e-6), (1000, 129, 1e-2),
          (513, 513, 1e-2), (513, 513, 1e-6)]


def inputs(N, Mz):
    rng = np.random.default_rng(N * 7 + Mz)
    return S.cols(rng, N), S.cols(rng, Mz), rng.normal(size=N)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("terms", [COMPOSITE, PRODUCT], ids=["composite", "product"])
@pytest.mark.parametrize("N,Mz,jitter", SHAPES)
def test_the_two_routes_agree(N, Mz, jitter, terms):
    X, Z, y = inputs(N, Mz)
    w = G.woodbury(X, terms, 0.1, y, Z, jitter)
    d = G.dense(X, terms, 0.1, y, Z, jitter)
    ref = S.woodbury(X, terms, 0.1, y, Z, jitter)
    e = dict(elbo=rel(w["elbo"], ref["elbo"]), dparam=float(np.max(np.abs(w["dparam"] - d["dparam"]) / d["scale"].clip(1e-300))),
             dnoise=rel(w["dnoise"], d["dnoise"]), djitter=rel(w["djitter"], d["djitter"]),
             dy=float(np.max(np.abs(w["dy"] - d["dy"])) / np.max(np.abs(d["dy"]))))
    print(N, Mz, jitter, e)
    assert e["elbo"] <= 1e-13 and rel(d["elbo"], ref["elbo"]) <= 1e-11
    for k in ("dparam", "dnoise", "djitter", "dy"):
        assert e[k] <= 1e-11, k
    for t, term in enumerate(terms):
        if term[0] == CAT:
            assert w["dparam"][t] == 0.0 and d["dparam"][t] == 0.0


def elbo(X, terms, noise, y, Z, jitter):
    return S.woodbury(X, terms, noise, y, Z, jitter)["elbo"]


@pytest.mark.parametrize("terms", [COMPOSITE, PRODUCT], ids=["composite", "product"])
@pytest.mark.parametrize("N,Mz", [(129, 127), (300, 5), (700, 127)])
def test_dense_route_matches_central_differences(N, Mz, terms):
    X, Z, y = inputs(N, Mz)
    jitter = 1e-6
    d = G.dense(X, terms, 0.1, y, Z, jitter)
    e0 = abs(d["elbo"])
    for t, (kind, col, param, group) in enumerate(terms):
        if kind == CAT:
            continue
        h = 1e-5 * param
        tp, tm = [list(x) for x in terms], [list(x) for x in terms]
        tp[t][2] += h
        tm[t][2] -= h
        fd = (elbo(X, [tuple(x) for x in tp], 0.1, y, Z, jitter) - elbo(X, [tuple(x) for x in tm], 0.1, y, Z, jitter)) / (2 * h)
        floor = 10 * 2.2e-16 * max(1.0, e0) / h  # rounding of the difference
        print("dparam", t, d["dparam"][t], fd, abs(d["dparam"][t] - fd) / d["scale"][t])
        assert abs(d["dparam"][t] - fd) <= 1e-6 * (abs(fd) + d["scale"][t]) + floor, (t, d["dparam"][t], fd)
    h = 1e-6
    fdn = (elbo(X, terms, 0.1 + h, y, Z, jitter) - elbo(X, terms, 0.1 - h, y, Z, jitter)) / (2 * h)
    print("dnoise", d["dnoise"], fdn, rel(d["dnoise"], fdn))
    assert abs(d["dnoise"] - fdn) <= 1e-6 * abs(fdn) + 10 * 2.2e-16 * max(1.0, e0) / h
    for i in (0, N // 2):
        e = np.zeros(N)
        e[i] = 1e-6
        fdy = (elbo(X, terms, 0.1, y + e, Z, jitter) - elbo(X, terms, 0.1, y - e, Z, jitter)) / 2e-6
        print("dy", i, d["dy"][i], fdy)
        assert abs(d["dy"][i] - fdy) <= 1e-6 * max(1.0, abs(fdy)) + 10 * 2.2e-16 * max(1.0, e0) / 1e-6
    # jitter: the third derivative is large (Kuu's small eigenvalues), so the step is small and
    # the bar is what this step leaves: observed 1.3e-11 .. 6.9e-8 relative at h = jitter / 1000
    # (truncation goes with h^2: jitter / 100 left 1e-5), so 1e-6
    jitter = 1e-2
    d = G.dense(X, terms, 0.1, y, Z, jitter)
    h = jitter / 1000
    fdj = (elbo(X, terms, 0.1, y, Z, jitter + h) - elbo(X, terms, 0.1, y, Z, jitter - h)) / (2 * h)
    print("djitter", d["djitter"], fdj, rel(d["djitter"], fdj))
    assert rel(d["djitter"], fdj) <= 1e-6
