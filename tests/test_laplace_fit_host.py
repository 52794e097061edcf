"""laplace_fit.fit_hyperparameters and abstractgps.approx_lml_grad on the host, no device: the fit
runs against a CPU stand-in for the context built from the numpy restatement
(tests/laplace_grad_oracle.py)."""
import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd import formula as F
from gaplac_amd import laplace_fit as LF
from oracle import restatement as R
from tests import laplace_grad_oracle as GO
from tests import laplace_oracle as LO


class OracleCtx:
    """Offers laplace_logpdf_grad as backend.Context does, computed by the restatement."""

    def __init__(self):
        self.log = []  # (warm-started, converged) per call

    def laplace_logpdf_grad(self, X, terms, jitter, lik, y, lik_param=0.0, max_iter=100, tol=1e-12, a0=None):
        g = GO.laplace_grad(X, list(terms), jitter, lik, y, lik_param, max_iter=max_iter, tol=tol, a0=a0)
        g.a, g.f, g.iters, g.converged = g.res.a, g.res.f, g.res.iters, g.res.converged
        self.log.append((a0 is not None, g.converged))
        return g


def planted(N=120, l_true=0.7, seed=3):
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(0, 10, N), rng.integers(0, 4, N).astype(float)])
    K = R.gram(X, [(_native.SQEXP, 0, l_true, 0)], 1e-6)
    f = 1.5 * (np.linalg.cholesky(K) @ rng.normal(size=N))
    return X, rng.poisson(np.exp(f)).astype(np.float64)


def test_the_fit_climbs_and_recovers_the_planted_direction():
    X, y = planted()
    l0 = 4.0
    terms = [(_native.SQEXP, 0, l0, 0), (_native.CAT, 1, 0.0, 1)]
    ctx = OracleCtx()
    fitted, logq, hist = LF.fit_hyperparameters(ctx, X, terms, 1e-6, LO.POISSON, y, maxiter=30)
    assert len(hist) >= 2 and all(b >= a for a, b in zip(hist, hist[1:]))
    assert logq == hist[-1] and logq > hist[0]
    l = fitted[0][2]
    print(f"l: {l0} -> {l:.4f} (planted 0.7); log q {hist[0]:.4f} -> {logq:.4f} in {len(ctx.log)} evaluations")
    assert abs(np.log(l) - np.log(0.7)) < abs(np.log(l0) - np.log(0.7)) and l < l0
    assert fitted[1] == terms[1] and fitted[0][:2] == terms[0][:2] and fitted[0][3] == terms[0][3]
    # every evaluation but the first starts from the previous a; one from a = 0 only follows a
    # warm-started one that did not converge
    assert ctx.log[0][0] is False and sum(w for w, _ in ctx.log) >= 2
    assert all(ctx.log[i - 1] == (True, False) for i in range(1, len(ctx.log)) if not ctx.log[i][0])
    # at the fitted point the gradient in log l is small against its start
    g0 = GO.laplace_grad(X, terms, 1e-6, LO.POISSON, y).dparam[0] * l0
    g1 = GO.laplace_grad(X, fitted, 1e-6, LO.POISSON, y).dparam[0] * l
    assert abs(g1) <= 1e-3 * abs(g0)


def test_free_terms_and_the_degenerate_calls():
    X, y = planted(N=40)
    terms = [(_native.SQEXP, 0, 2.0, 0), (_native.OU, 0, 3.0, 1), (_native.LINEAR, 1, 0.5, 2)]
    assert LF.free_lengthscales(terms) == [0, 1]
    ctx = OracleCtx()
    fitted, logq, hist = LF.fit_hyperparameters(ctx, X, terms, 1e-6, LO.POISSON, y, free=[1], maxiter=5)
    assert fitted[0] == terms[0] and fitted[2] == terms[2] and fitted[1][2] != 3.0
    assert all(b >= a for a, b in zip(hist, hist[1:]))
    same, q0, h0 = LF.fit_hyperparameters(ctx, X, terms, 1e-6, LO.POISSON, y, maxiter=0)
    assert same == terms and h0 == [q0] and abs(q0 - hist[0]) <= 1e-12 * abs(q0)  # (exp(log l) rounds)
    for bad in ([2], [5], [-1], [0, 0]):
        with pytest.raises(ValueError):
            LF.fit_hyperparameters(ctx, X, terms, 1e-6, LO.POISSON, y, free=bad)


def test_approx_lml_grad_argument_errors():
    gp = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))[0]
    lfx = AG.LatentGP(gp, AG.PoissonLikelihood(), 1e-6)(np.linspace(0, 1, 8)[:, None])
    la = AG.LaplaceApproximation()
    with pytest.raises(F.ArgumentError):
        AG.approx_lml_grad("la", lfx, np.zeros(8))
    with pytest.raises(F.ArgumentError):
        AG.approx_lml_grad(la, "lfx", np.zeros(8))
    with pytest.raises(F.ArgumentError):
        AG.approx_lml_grad(la, lfx, np.zeros(7))
    with pytest.raises(F.ArgumentError):
        AG.approx_lml_grad(la, lfx, np.zeros((8, 1)))


def test_approx_lml_grad_passes_the_objects_on():
    """(lml, dparam, djitter) from the context's result, the arguments those of the objects."""
    gp = AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5) + OU(:x; l=3.0)"))[0]
    x = np.linspace(0, 5, 30)
    X = np.column_stack([x, x])
    y = np.random.default_rng(1).poisson(2.0, 30).astype(np.float64)
    lfx = AG.LatentGP(gp, AG.PoissonLikelihood(), 1e-5)(X)
    ctx = OracleCtx()
    out = AG.approx_lml_grad(AG.LaplaceApproximation(maxiter=50, tol=1e-11), lfx, y, ctx=ctx)
    ref = GO.laplace_grad(X, lfx.fx.terms, 1e-5, LO.POISSON, y, max_iter=50, tol=1e-11)
    assert out[0] == ref.logq and np.array_equal(out[1], ref.dparam) and out[2] == ref.djitter
