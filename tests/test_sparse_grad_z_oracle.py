"""The CPU recipe for dZ (tests/sparse_grad_z_oracle.py), pinned without a GPU: its two routes to
each other, the dense one to central differences of the bound, the exact zeros, and
vfe_fit.fit_inducing on a stand-in context whose gradient is the dense route.

Bars: the routes within 1e-11 of (|ref| + addend magnitude) per entry (observed: 6.2e-13). Central
differences of sparse_oracle.woodbury's elbo at h = 1e-5 within 1e-6 max(1, |fd|) plus the rounding
floor 10 eps |elbo| / h, the bar of tests/test_gpu_sparse_grad.py's mcmc test; the formula has no OU
term there, whose kink a step would cross (OU is pinned by the dense route only).
"""
import numpy as np
import pytest

from gaplac_amd import vfe_fit
from gaplac_amd._native import CAT, LINEAR, NOISE, OU, SQEXP
from gaplac_amd.backend import PosDefException
from tests import sparse_grad_oracle as G
from tests import sparse_grad_z_oracle as GZ
from tests import sparse_oracle as S

COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (LINEAR, 2, 0.5, 3)]
PRODUCT = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 0), (CAT, 1, 0.0, 1), (LINEAR, 2, 0.5, 1), (NOISE, 0, 0.05, 2)]
NO_OU = [(SQEXP, 0, 1.5, 0), (CAT, 1, 0.0, 1), (LINEAR, 2, 0.5, 2)]


@pytest.mark.parametrize("N,Mz,jitter,terms", [(300, 5, 1e-6, COMPOSITE), (129, 127, 1e-6, COMPOSITE),
                                               (700, 127, 1e-2, COMPOSITE), (700, 127, 1e-6, PRODUCT)])
def test_the_two_routes_agree(N, Mz, jitter, terms):
    c = S.Case(N, Mz, 1, terms, 0.1, jitter)
    dw, sw = GZ.woodbury(c.X, terms, 0.1, c.y, c.Z, jitter)
    dd, sd = GZ.dense(c.X, terms, 0.1, c.y, c.Z, jitter)
    err = np.abs(dw - dd) / (np.abs(dd) + sd).clip(1e-300)
    print("routes / (|ref| + scale)", err.max(), "cancellation", (np.abs(dd) / sd.clip(1e-300))[:, [0, 2]].min())
    assert dw.shape == dd.shape == (Mz, 3)
    assert np.all(np.abs(dw - dd) <= 1e-11 * (np.abs(dd) + sd))
    assert np.all(dw[:, 1] == 0.0) and np.all(dd[:, 1] == 0.0)  # the column only CAT reads
    assert np.all(np.abs(sw - sd) <= 1e-9 * sd)


def test_dense_route_matches_central_differences():
    N, Mz, h = 700, 127, 1e-5
    c = S.Case(N, Mz, 1, NO_OU, 0.1, 1e-6)
    dZ, _ = GZ.dense(c.X, NO_OU, 0.1, c.y, c.Z, 1e-6)
    elbo = S.woodbury(c.X, NO_OU, 0.1, c.y, c.Z, 1e-6)["elbo"]
    for m, d in ((0, 0), (17, 0), (126, 0), (3, 2), (90, 2)):
        e = np.zeros(c.Z.shape)
        e[m, d] = h
        fd = (S.woodbury(c.X, NO_OU, 0.1, c.y, c.Z + e, 1e-6)["elbo"] -
              S.woodbury(c.X, NO_OU, 0.1, c.y, c.Z - e, 1e-6)["elbo"]) / (2 * h)
        bar = 1e-6 * max(1.0, abs(fd)) + 10 * 2.2e-16 * abs(elbo) / h
        print("dZ", (m, d), dZ[m, d], fd, abs(dZ[m, d] - fd), "bar", bar)
        assert abs(dZ[m, d] - fd) <= bar


def test_unread_and_categorical_columns_are_exactly_zero():
    c = S.Case(300, 5, 1, COMPOSITE, 0.1, 1e-6)
    rng = np.random.default_rng(5)
    X4, Z4 = np.column_stack([c.X, rng.normal(size=300)]), np.column_stack([c.Z, rng.normal(size=5)])
    for route in (GZ.woodbury, GZ.dense):
        dZ, scale = route(X4, COMPOSITE, 0.1, c.y, Z4, 1e-6)
        assert dZ.shape == (5, 4)
        assert np.all(dZ[:, 1] == 0.0) and np.all(dZ[:, 3] == 0.0) and np.all(scale[:, [1, 3]] == 0.0)
        assert np.all(dZ[:, [0, 2]] != 0.0)


class _DenseCtx:
    """Stands in for backend.Context (no GPU): the dense CPU routes."""

    def __init__(self):
        self.calls = 0

    def sparse_elbo_grad(self, X, terms, noise, y, Z, jitter, wrt_z=False):
        self.calls += 1
        g = G.dense(X, terms, noise, y, Z, jitter)
        out = (g["elbo"], g["dy"], g["dparam"], g["dnoise"], g["djitter"])
        return out + (GZ.dense(X, terms, noise, y, Z, jitter)[0],) if wrt_z else out


def _fit_inputs():
    rng = np.random.default_rng(200)
    x = np.sort(rng.uniform(0, 10, 200))
    X = np.column_stack([x, rng.normal(size=200)])
    y = np.sin(x) + 0.3 * rng.normal(size=200)
    Z0 = np.column_stack([np.linspace(0.1, 0.9, 6), np.arange(6.0)])  # bunched in the left tenth
    return X, y, Z0


def test_fit_inducing_climbs_the_bound_and_moves_only_its_columns():
    X, y, Z0 = _fit_inputs()
    terms = [(SQEXP, 0, 1.0, 0)]
    ctx = _DenseCtx()
    keep = Z0.copy()
    Z, elbo, history = vfe_fit.fit_inducing(ctx, X, terms, 0.1, y, Z0, jitter=1e-6, maxiter=40)
    print("bound", history[0], "->", elbo, "in", len(history) - 1, "steps,", ctx.calls, "calls; Z", np.sort(Z[:, 0]))
    assert np.array_equal(Z0, keep)                          # the start is not written to
    assert len(history) >= 2 and all(b >= a for a, b in zip(history, history[1:]))
    assert elbo == history[-1] and elbo > history[0]
    assert np.array_equal(Z[:, 1], Z0[:, 1]) and not np.array_equal(Z[:, 0], Z0[:, 0])
    assert elbo == ctx.sparse_elbo_grad(X, terms, 0.1, y, Z, 1e-6)[0]
    # explicit columns: a column a term reads stays where it is when it is not listed
    both = [(SQEXP, 0, 1.0, 0), (LINEAR, 1, 0.5, 1)]
    assert vfe_fit.movable_columns(both, 2) == [0, 1]
    assert vfe_fit.movable_columns(COMPOSITE, 3) == [0, 2]
    Zb, eb, hb = vfe_fit.fit_inducing(ctx, X, both, 0.1, y, Z0, cols=[0], maxiter=10)
    assert np.array_equal(Zb[:, 1], Z0[:, 1]) and eb > hb[0]
    Z1, e1, h1 = vfe_fit.fit_inducing(ctx, X[:, 0], terms, 0.1, y, Z0[:, 0], maxiter=5)   # 1-D inputs
    assert Z1.shape == (6, 1) and e1 >= h1[0]
    with pytest.raises(ValueError):
        vfe_fit.fit_inducing(ctx, X, terms, 0.1, y, Z0, cols=[2])


def test_fit_inducing_survives_a_failed_trial_point():
    X, y, Z0 = _fit_inputs()
    terms = [(SQEXP, 0, 1.0, 0)]

    class Failing(_DenseCtx):
        def sparse_elbo_grad(self, *a, **k):
            if self.calls == 1:                              # the first trial point of the first line search
                self.calls += 1
                raise PosDefException(3)
            return super().sparse_elbo_grad(*a, **k)

    ctx = Failing()
    Z, elbo, history = vfe_fit.fit_inducing(ctx, X, terms, 0.1, y, Z0, maxiter=20)
    assert ctx.calls > 2 and elbo > history[0] and all(b >= a for a, b in zip(history, history[1:]))
