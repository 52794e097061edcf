"""The host side of the Laplace approximation, no device: the formula's likelihood slot, the
argument errors of the abstractgps objects, the backend switch, and where select_formulae sends a
formula whose likelihood is not Gaussian.
"""
import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd import backend
from gaplac_amd import formula as F


# ---- the formula slot -----------------------------------------------------------------------
@pytest.mark.parametrize("text,lik", [("Bernoulli", F.Bernoulli()), ("Bernoulli()", F.Bernoulli()),
                                      ("Poisson", F.Poisson()), ("Poisson()", F.Poisson()),
                                      ("  Poisson  ", F.Poisson()), ("Gaussian", F.Gaussian()),
                                      ("Gaussian()", F.Gaussian()), ("", F.Gaussian())])
def test_likelihood_slot(text, lik):
    spec = F.gp_spec(f"y : {text} ~| SqExp(:x; l=1.5) + Cat(:g)")
    assert F.likelihood(spec) == lik
    assert type(F.likelihood(spec)) is type(lik)
    assert F.response(spec) == "y"
    assert F.gp_spec("y ~| SqExp(:x)").lik == F.Gaussian()


@pytest.mark.parametrize("name", ["Gamma", "bernoulli", "poisson()", "Poisson(2)", "Binomial()", "NegativeBinomial",
                                  "Bernoulli ()", "Laplace"])
def test_every_other_name_is_undefined(name):
    with pytest.raises(F.UndefVarError):
        F.gp_spec(f"y : {name} ~| SqExp(:x)")


def test_the_likelihoods_are_distinct():
    assert F.Bernoulli() != F.Poisson() and F.Bernoulli() != F.Gaussian() and F.Poisson() != F.Gaussian()
    assert repr(F.Bernoulli()) == "Bernoulli()" and repr(F.Poisson()) == "Poisson()"
    assert isinstance(F.Bernoulli(), F.AbstractLiklihood) and isinstance(F.Poisson(), F.AbstractLiklihood)


# ---- the abstractgps objects ----------------------------------------------------------------
def _gp():
    return AG.make_gp(F.gp_spec("y ~| SqExp(:x; l=1.5)"))[0]


def _lfx(n=8, lik=None):
    return AG.LatentGP(_gp(), lik or AG.PoissonLikelihood(), 1e-6)(np.linspace(0, 1, n)[:, None])


def test_likelihood_objects():
    assert AG.BernoulliLikelihood().code == _native.LIK_BERNOULLI
    assert AG.PoissonLikelihood().code == _native.LIK_POISSON
    g = AG.GaussianLikelihood(0.1)
    assert (g.code, g.param) == (_native.LIK_GAUSSIAN, 0.1)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(F.ArgumentError):
            AG.GaussianLikelihood(bad)


def test_latent_gp_argument_errors():
    with pytest.raises(F.ArgumentError):
        AG.LatentGP("not a GP", AG.PoissonLikelihood(), 1e-6)
    with pytest.raises(F.ArgumentError):
        AG.LatentGP(_gp(), "poisson", 1e-6)
    with pytest.raises(F.ArgumentError):
        AG.LatentGP(_gp(), F.Poisson(), 1e-6)  # (the formula's tag is not a likelihood object)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(F.ArgumentError):
            AG.LatentGP(_gp(), AG.PoissonLikelihood(), bad)
    lfx = _lfx(5)
    assert len(lfx) == 5 and lfx.fx.noise == 1e-6 and isinstance(lfx.lik, AG.PoissonLikelihood)
    assert AG.LatentGP(_gp(), AG.BernoulliLikelihood()).jitter == 1e-6


def test_laplace_approximation_argument_errors():
    la = AG.LaplaceApproximation()
    assert (la.maxiter, la.tol) == (100, 1e-12)
    for bad in (0, -3, 2.5):
        with pytest.raises(F.ArgumentError):
            AG.LaplaceApproximation(maxiter=bad)
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(F.ArgumentError):
            AG.LaplaceApproximation(tol=bad)


def test_approx_lml_and_posterior_argument_errors():
    la, lfx = AG.LaplaceApproximation(), _lfx(8)
    with pytest.raises(F.ArgumentError):
        AG.approx_lml(la, lfx, np.zeros(7))
    with pytest.raises(F.ArgumentError):
        AG.approx_lml(la, lfx, np.zeros((8, 2)))
    with pytest.raises(F.ArgumentError):
        AG.approx_lml(la, lfx.fx, np.zeros(8))  # a FiniteGP is not a LatentFiniteGP
    with pytest.raises(F.ArgumentError):
        AG.approx_lml("laplace", lfx, np.zeros(8))
    with pytest.raises(F.ArgumentError):
        AG.posterior(la, lfx, np.zeros(9))
    with pytest.raises(F.ArgumentError):
        AG.posterior(la, lfx)
    post = AG.posterior(la, lfx, np.zeros(8))
    assert isinstance(post, AG.LaplacePosteriorGP) and post.prior is lfx.fx
    for name in ("mean_and_var", "mean", "var", "f_hat"):
        assert hasattr(type(post), name)


def test_the_existing_posterior_dispatches_are_intact():
    fx = AG.FiniteGP(_gp(), np.linspace(0, 1, 8)[:, None], 0.1)
    assert type(AG.posterior(fx, np.zeros(8))) is AG.PosteriorGP
    fz = AG.FiniteGP(_gp(), np.linspace(0, 1, 3)[:, None], 1e-6)
    assert type(AG.posterior(AG.VFE(fz), fx, np.zeros(8))) is AG.ApproxPosteriorGP
    with pytest.raises(F.ArgumentError):
        AG.posterior(fx)


def test_likelihood_code_names():
    assert backend.likelihood_code("Bernoulli") == _native.LIK_BERNOULLI
    assert backend.likelihood_code("poisson") == _native.LIK_POISSON
    assert backend.likelihood_code("GAUSSIAN") == _native.LIK_GAUSSIAN
    assert backend.likelihood_code(2) == 2
    with pytest.raises(backend.ArgumentError):
        backend.likelihood_code("gamma")


# ---- the gate -------------------------------------------------------------------------------
def test_switch_is_read_at_call_time(monkeypatch):
    la, lfx, y = AG.LaplaceApproximation(), _lfx(8), np.ones(8)
    table = {"y": y, "x": np.linspace(0, 1, 8)}
    monkeypatch.setenv("GAPLAC_HIP", "0")
    with pytest.raises(AG.BackendDisabled):
        AG.approx_lml(la, lfx, y)
    with pytest.raises(AG.BackendDisabled):
        AG.posterior(la, lfx, y).mean_and_var(np.zeros((2, 1)))
    with pytest.raises(AG.BackendDisabled):
        AG.posterior(la, lfx, y).f_hat
    with pytest.raises(AG.BackendDisabled):
        AG.select_formulae("y : Poisson ~| SqExp(:x)", "y : Poisson ~| OU(:x)", table)
    monkeypatch.setenv("GAPLAC_HIP", "1")
    sentinel = RuntimeError("backend reached")

    def fake_ctx():
        raise sentinel

    monkeypatch.setattr(backend, "default_context", fake_ctx)
    with pytest.raises(RuntimeError) as ei:
        AG.approx_lml(la, lfx, y)
    assert ei.value is sentinel


# ---- select_formulae's routing --------------------------------------------------------------
class FakeContext:
    """Records which entry each formula reaches."""

    def __init__(self):
        self.calls = []

    def logpdf(self, X, terms, noise, v, full=False):
        self.calls.append(("logpdf", noise, list(terms)))
        return -1.0

    def logpdf_multi(self, X, terms, noise, Y, full=False):
        self.calls.append(("logpdf_multi", noise, list(terms)))
        return np.full(Y.shape[1], -1.0)

    def laplace_logpdf(self, X, terms, jitter, lik, y, lik_param=0.0, max_iter=100, tol=1e-12, a0=None, full=False):
        self.calls.append(("laplace_logpdf", jitter, lik, max_iter, tol))
        return -3.0


def test_select_formulae_routes_by_likelihood():
    table = {"y": np.arange(6.0), "z": np.arange(6.0) % 2, "x": np.linspace(0, 1, 6)}
    c = FakeContext()
    bayes, lp1, lp2 = AG.select_formulae("y : Poisson ~| SqExp(:x)", "y : Poisson() ~| OU(:x)", table, ctx=c)
    assert (bayes, lp1, lp2) == (0.0, -3.0, -3.0)
    assert c.calls == [("laplace_logpdf", 1e-6, _native.LIK_POISSON, 100, 1e-12)] * 2
    c = FakeContext()
    AG.select_formulae("z : Bernoulli ~| SqExp(:x)", "z ~| SqExp(:x)", table, noise=0.2, ctx=c)
    assert [k[0] for k in c.calls] == ["laplace_logpdf", "logpdf"]
    assert c.calls[0][2] == _native.LIK_BERNOULLI and c.calls[1][1] == 0.2
    c = FakeContext()  # Gaussian formulas keep their call
    AG.select_formulae("y ~| SqExp(:x)", "y : Gaussian ~| OU(:x)", table, ctx=c)
    assert [k[0] for k in c.calls] == ["logpdf", "logpdf"]
    c = FakeContext()
    AG.select_formulae("y ~| SqExp(:x)", "y ~| OU(:x)", table, ctx=c, responses=["y", "z"])
    assert [k[0] for k in c.calls] == ["logpdf_multi", "logpdf_multi"]
    for f1, f2 in (("y : Poisson ~| SqExp(:x)", "y ~| OU(:x)"), ("y ~| SqExp(:x)", "z : Bernoulli ~| OU(:x)")):
        with pytest.raises(F.ArgumentError):
            AG.select_formulae(f1, f2, table, ctx=FakeContext(), responses=["y"])
