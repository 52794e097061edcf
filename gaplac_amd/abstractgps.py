"""AbstractGPs-shaped front end over the HIP backend (the drop-in boundary).

In the reference the hot path is the generic function
`Distributions.logpdf(::AbstractGPs.FiniteGP, ::AbstractVector)` (AbstractGPs 0.5.12),
reached from CLI/src/mcmc.jl:35 (`fx ~ FiniteGP(GP(k), RowVecs(X), 0.1)`) and
CLI/src/select.jl:43-50 (`logpdf(FiniteGP(gp, x, 0.1, obsdim=1), y)`). This module
mirrors that surface: GP(kernel), FiniteGP(gp, X, noise), logpdf(fx, v) — and routes the
evaluation through libgaplac_hip.so. There is no CPU fallback.

The switch: the Julia glue gates its overloads on a flag that
__init__ sets from GAPLAC_HIP at every package load; here the same variable is read at
EVERY call (hip_enabled). Off, the Julia host falls through to AbstractGPs' own method;
this twin has no such method (no CPU path in the product), so it raises BackendDisabled.
Default on here, since nothing else could answer.
"""
from __future__ import annotations

import os

import numpy as np

from . import backend
from . import formula as F
from . import kernels as K


class BackendDisabled(RuntimeError):
    """GAPLAC_HIP=0: the HIP backend is switched off (the Julia host would use AbstractGPs)."""


def hip_enabled() -> bool:
    """GAPLAC_HIP, read now (not at import): "0" turns the backend off."""
    return os.environ.get("GAPLAC_HIP", "1") != "0"


def _gate():
    if not hip_enabled():
        raise BackendDisabled("GAPLAC_HIP=0: HIP backend disabled; the Julia host falls back to AbstractGPs")


class GP:
    """Zero-mean GP with a kernel from GaPLAC.kernel (AbstractGPs.GP(k))."""

    def __init__(self, kern):
        self.kernel = kern

    def __call__(self, x, noise=0.0, obsdim=1):
        return FiniteGP(self, x, noise, obsdim=obsdim)


class FiniteGP:
    """AbstractGPs.FiniteGP(f, x, Σy): f at the rows of x (RowVecs / obsdim=1) with
    i.i.d. observation noise Σy = Diagonal(Fill(noise, N))."""

    def __init__(self, f: GP, x, noise=0.0, obsdim=1):
        X = np.asarray(x, dtype=np.float64)
        if X.ndim == 1:
            X = X[:, None]
        if obsdim == 2:
            X = X.T
        elif obsdim != 1:
            raise F.ArgumentError("obsdim must be 1 or 2")
        self.f = f
        self.x = np.asfortranarray(X)
        self.noise = float(noise)
        self.terms = K.lower(f.kernel)

    def __len__(self):
        return self.x.shape[0]


def logpdf(fx: FiniteGP, y, ctx: backend.Context | None = None, full: bool = False):
    """-(N log 2pi + logdet(C) + ||U^-T y||^2) / 2 on the GPU; raises
    backend.PosDefException(info) when C is not positive definite (cholesky check=true).
    A matrix y (N x R) is AbstractGPs' logpdf(fx, Y::AbstractMatrix): one log-density per
    column, shape (R,), from one factorisation (gaplac_logpdf_multi)."""
    _gate()
    if isinstance(fx, FinitePosteriorGP):
        # logpdf(posterior(fx, y)(xs, noise), ys): a vector gives a scalar, a matrix one value
        # per column (gaplac_posterior_logpdf)
        ys = np.asarray(y, dtype=np.float64)
        if ys.ndim == 0 or ys.ndim > 2 or ys.shape[0] != len(fx):
            raise F.ArgumentError("DimensionMismatch: length of ys does not match the test points")
        res = fx._logpdf(ys if ys.ndim == 2 else ys[:, None], ctx, full)
        if ys.ndim == 2:
            return res
        return (res[0][0], res[1], res[2][0]) if full else res[0]
    ctx = ctx or backend.default_context()
    y = np.asarray(y, dtype=np.float64)
    if y.ndim == 0 or y.shape[0] != len(fx):
        raise F.ArgumentError("DimensionMismatch: length of y does not match the FiniteGP")
    if y.ndim == 2:
        return ctx.logpdf_multi(fx.x, fx.terms, fx.noise, y, full=full)
    return ctx.logpdf(fx.x, fx.terms, fx.noise, y, full=full)


def logpdf_and_gradient(fx: FiniteGP, y, ctx: backend.Context | None = None):
    """(logpdf, dlogpdf/dy, dlogpdf/dparam per lowered term, dlogpdf/dnoise) on the GPU:
    what ForwardDiff computes through AbstractGPs.logpdf in the reference's mcmc
    (CLI/src/mcmc.jl:31-41), as one analytic evaluation (gaplac_logpdf_grad)."""
    _gate()
    ctx = ctx or backend.default_context()
    y = np.asarray(y, dtype=np.float64)
    if y.shape[0] != len(fx):
        raise F.ArgumentError("DimensionMismatch: length of y does not match the FiniteGP")
    return ctx.logpdf_grad(fx.x, fx.terms, fx.noise, y)


class PosteriorGP:
    """AbstractGPs.posterior(fx, y): the GP conditioned on observations y at fx's inputs.
    Evaluation happens per query (mean_and_var at test inputs), one gaplac_posterior_mean_var
    call each; fit() returns the same posterior with the factorisation kept."""

    def __init__(self, fx: FiniteGP, y, ctx: backend.Context | None = None):
        y = np.asarray(y, dtype=np.float64)
        if y.shape[0] != len(fx):
            raise F.ArgumentError("DimensionMismatch: length of y does not match the FiniteGP")
        self.prior = fx
        self.y = y
        self.ctx = ctx

    def _xs(self, x):
        X = np.asarray(x, dtype=np.float64)
        if X.ndim == 1:
            X = X[:, None]
        return X

    def mean_and_var(self, x):
        """AbstractGPs.mean_and_var(f::PosteriorGP, x): posterior mean and marginal variance
        (latent: no observation noise) at the rows of x."""
        _gate()
        ctx = self.ctx or backend.default_context()
        return ctx.posterior_mean_var(self.prior.x, self.prior.terms, self.prior.noise, self.y, self._xs(x))

    def component_mean_and_var(self, x, comp, G=None):
        """(mean[M, G], var[M, G]) of every component of the kernel at the rows of x: comp[t] is
        the component of lowered term t (kernels.lower_formula_components gives the map of a
        formula's summands), -1 for none. One factorisation for all of them
        (gaplac_posterior_components); nothing in AbstractGPs does this in one call."""
        _gate()
        ctx = self.ctx or backend.default_context()
        return ctx.posterior_components(self.prior.x, self.prior.terms, self.prior.noise, self.y, self._xs(x),
                                        comp, G)

    def mean(self, x):
        return self.mean_and_var(x)[0]

    def var(self, x):
        return self.mean_and_var(x)[1]

    def fit(self, cap: int = 1024):
        """The posterior factored once and kept on the device (gaplac_fit_create), as AbstractGPs'
        PosteriorGP keeps its Cholesky factor and α: a FittedPosteriorGP whose queries skip the
        factorisation. cap: the test points solved at once (larger queries run in chunks)."""
        _gate()
        ctx = self.ctx or backend.default_context()
        return FittedPosteriorGP(self, ctx.fit(self.prior.x, self.prior.terms, self.prior.noise, self.y, cap=cap))

    def __call__(self, x, noise=0.0):
        """AbstractGPs' fp(xs, σ²): the posterior at the rows of x, jointly, with observation
        variance noise there (a FiniteGP{<:PosteriorGP})."""
        return FinitePosteriorGP(self, x, noise)


class FittedPosteriorGP:
    """PosteriorGP.fit(): the same posterior behind a kept factorisation (backend.Fit). mean_and_var
    and var solve the test rows against the kept factor (gaplac_fit_mean_var); mean alone is the
    matrix-free K(xs, X) α (gaplac_fit_mean). Close it (or use it as a context manager) to free
    the device memory early."""

    def __init__(self, f: PosteriorGP, fit: "backend.Fit"):
        self.f = f
        self.prior = f.prior
        self.y = f.y
        self.handle = fit

    def mean_and_var(self, x):
        _gate()
        return self.handle.mean_var(self.f._xs(x))

    def mean(self, x):
        _gate()
        return self.handle.mean(self.f._xs(x))

    def var(self, x):
        return self.mean_and_var(x)[1]

    def close(self):
        self.handle.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class FinitePosteriorGP:
    """posterior(fx, y)(xs, noise): a finite-dimensional Gaussian with mean m and covariance
    Σ* (gaplac.h, the joint posterior entries). Every query is one library call."""

    def __init__(self, f: PosteriorGP, x, noise=0.0):
        self.f = f
        self.x = np.asfortranarray(f._xs(x))
        self.noise = float(noise)

    def __len__(self):
        return self.x.shape[0]

    def _args(self):
        pr = self.f.prior
        return pr.x, pr.terms, pr.noise, self.f.y, self.x, self.noise

    def _ctx(self, ctx):
        return ctx or self.f.ctx or backend.default_context()

    def mean_and_cov(self, ctx=None):
        _gate()
        return self._ctx(ctx).posterior_mean_cov(*self._args())

    def _rand(self, z, ctx):
        return self._ctx(ctx).posterior_rand(*self._args(), z)

    def _logpdf(self, ys, ctx, full):
        return self._ctx(ctx).posterior_logpdf(*self._args(), ys, full=full)


class VFE:
    """AbstractGPs.VFE(fz): the inducing-point approximation of Titsias with pseudo-points
    fz = f(z, jitter), a FiniteGP whose inputs are the inducing inputs and whose noise is the
    jitter."""

    def __init__(self, fz: FiniteGP):
        if not isinstance(fz, FiniteGP):
            raise F.ArgumentError("VFE takes the FiniteGP f(z, jitter) at the inducing inputs")
        self.fz = fz


def _vfe_args(vfe: VFE, fx: FiniteGP, y):
    if not isinstance(vfe, VFE) or not isinstance(fx, FiniteGP):
        raise F.ArgumentError("expected (VFE(f(z)), f(x, noise), y)")
    if vfe.fz.terms != fx.terms:
        raise F.ArgumentError("VFE: f(z) and f(x) must be the same GP")
    if vfe.fz.x.shape[1] != fx.x.shape[1]:
        raise F.ArgumentError("DimensionMismatch: inducing inputs and training inputs differ in columns")
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 1 or y.shape[0] != len(fx):
        raise F.ArgumentError("DimensionMismatch: length of y does not match the FiniteGP")
    return fx.x, fx.terms, fx.noise, y, vfe.fz.x, vfe.fz.noise


def elbo(vfe: VFE, fx: FiniteGP, y, ctx: backend.Context | None = None, full: bool = False):
    """AbstractGPs.elbo(VFE(f(z)), f(x, noise), y): the evidence lower bound (gaplac_sparse_elbo);
    full=True returns the dict elbo, dtc, trace, logdet, quad."""
    _gate()
    args = _vfe_args(vfe, fx, y)
    return (ctx or backend.default_context()).sparse_elbo(*args, full=full)


def elbo_and_gradient(vfe: VFE, fx: FiniteGP, y, ctx: backend.Context | None = None, wrt_inducing: bool = False):
    """(elbo, dy, dparam, dnoise, djitter): the bound and its gradient with respect to y, the
    lowered terms' parameters, the observation variance and the jitter of f(z, jitter), the
    inducing inputs fixed (gaplac_sparse_elbo_grad). wrt_inducing=True appends dZ, the gradient
    with respect to the inducing inputs (Mz x D, gaplac_sparse_elbo_grad_z). AbstractGPs has no
    such method: a Julia host differentiates elbo by AD."""
    _gate()
    args = _vfe_args(vfe, fx, y)
    c = ctx or backend.default_context()
    return c.sparse_elbo_grad(*args, wrt_z=True) if wrt_inducing else c.sparse_elbo_grad(*args)


def dtc(vfe: VFE, fx: FiniteGP, y, ctx: backend.Context | None = None):
    """AbstractGPs.dtc(VFE(f(z)), f(x, noise), y): log N(y | 0, Q + noise I), the bound without
    its trace term (gaplac_sparse_elbo's out_dtc)."""
    _gate()
    args = _vfe_args(vfe, fx, y)
    return (ctx or backend.default_context()).sparse_elbo(*args, full=True)["dtc"]


class ApproxPosteriorGP:
    """AbstractGPs.posterior(VFE(f(z)), f(x, noise), y): the approximate posterior. Evaluation
    happens per query, one gaplac_sparse_posterior_mean_var call each."""

    def __init__(self, vfe: VFE, fx: FiniteGP, y, ctx: backend.Context | None = None):
        self._args = _vfe_args(vfe, fx, y)
        self.approx = vfe
        self.prior = fx
        self.y = self._args[3]
        self.ctx = ctx

    def mean_and_var(self, x):
        _gate()
        X = np.asarray(x, dtype=np.float64)
        if X.ndim == 1:
            X = X[:, None]
        ctx = self.ctx or backend.default_context()
        return ctx.sparse_posterior_mean_var(*self._args, X)

    def mean(self, x):
        return self.mean_and_var(x)[0]

    def var(self, x):
        return self.mean_and_var(x)[1]

    def __call__(self, x, noise=0.0):
        """AbstractGPs' fp(xs, σ²): the approximate posterior at the rows of x, jointly, with
        observation variance noise there."""
        return FiniteApproxPosteriorGP(self, x, noise)


class FiniteApproxPosteriorGP(FinitePosteriorGP):
    """posterior(VFE(f(z)), fx, y)(xs, noise): the finite-dimensional Gaussian of the
    inducing-point posterior (gaplac.h, the sparse joint entries). A FinitePosteriorGP to
    mean_and_cov, cov, rand and logpdf: the same gate and shape checks, one library call per
    query."""

    def __init__(self, f: ApproxPosteriorGP, x, noise=0.0):
        X = np.asarray(x, dtype=np.float64)
        if X.ndim == 1:
            X = X[:, None]
        self.f = f
        self.x = np.asfortranarray(X)
        self.noise = float(noise)

    def _args(self):
        return (*self.f._args, self.x, self.noise)

    def mean_and_cov(self, ctx=None):
        _gate()
        return self._ctx(ctx).sparse_posterior_mean_cov(*self._args())

    def _rand(self, z, ctx):
        return self._ctx(ctx).sparse_posterior_rand(*self._args(), z)

    def _logpdf(self, ys, ctx, full):
        return self._ctx(ctx).sparse_posterior_logpdf(*self._args(), ys, full=full)


# ---- Laplace approximation, in the shape of ApproximateGPs.jl ----
class BernoulliLikelihood:
    """GPLikelihoods.BernoulliLikelihood() with its default logistic link: y in {0, 1}."""
    code, param = backend._native.LIK_BERNOULLI, 0.0

    def __repr__(self):
        return "BernoulliLikelihood()"


class PoissonLikelihood:
    """GPLikelihoods.PoissonLikelihood() with its default exp link: y a count."""
    code, param = backend._native.LIK_POISSON, 0.0

    def __repr__(self):
        return "PoissonLikelihood()"


class GaussianLikelihood:
    """GPLikelihoods.GaussianLikelihood(var): the approximation is then exact."""
    code = backend._native.LIK_GAUSSIAN

    def __init__(self, var):
        var = float(var)
        if not (var > 0.0) or not np.isfinite(var):
            raise F.ArgumentError(f"GaussianLikelihood: the variance {var} must be finite and > 0")
        self.param = var

    def __repr__(self):
        return f"GaussianLikelihood({self.param})"


_LIKELIHOODS = (BernoulliLikelihood, PoissonLikelihood, GaussianLikelihood)


class LatentGP:
    """AbstractGPs.LatentGP(f, lik, jitter): a GP whose values are seen through the likelihood
    lik; jitter >= 0 is added to the latent covariance's diagonal."""

    def __init__(self, f: GP, lik, jitter: float = 1e-6):
        if not isinstance(f, GP):
            raise F.ArgumentError("LatentGP takes a GP")
        if not isinstance(lik, _LIKELIHOODS):
            raise F.ArgumentError("LatentGP: lik must be a BernoulliLikelihood, PoissonLikelihood or GaussianLikelihood")
        jitter = float(jitter)
        if not (jitter >= 0.0) or not np.isfinite(jitter):
            raise F.ArgumentError(f"LatentGP: jitter {jitter} must be finite and >= 0")
        self.f, self.lik, self.jitter = f, lik, jitter

    def __call__(self, x, obsdim=1):
        return LatentFiniteGP(self, x, obsdim=obsdim)


class LatentFiniteGP:
    """lgp(x): the latent GP at the rows of x (AbstractGPs.LatentFiniteGP)."""

    def __init__(self, lgp: LatentGP, x, obsdim=1):
        self.lgp = lgp
        self.fx = FiniteGP(lgp.f, x, lgp.jitter, obsdim=obsdim)
        self.lik = lgp.lik

    def __len__(self):
        return len(self.fx)


class LaplaceApproximation:
    """ApproximateGPs.LaplaceApproximation: Newton's iteration, at most maxiter steps, stopped
    when the objective changes by no more than tol (1 + |objective|)."""

    def __init__(self, maxiter: int = 100, tol: float = 1e-12):
        if int(maxiter) != maxiter or int(maxiter) < 1:
            raise F.ArgumentError(f"LaplaceApproximation: maxiter = {maxiter} must be an integer >= 1")
        tol = float(tol)
        if not (tol > 0.0) or not np.isfinite(tol):
            raise F.ArgumentError(f"LaplaceApproximation: tol = {tol} must be finite and > 0")
        self.maxiter, self.tol = int(maxiter), tol


def _laplace_args(la, lfx, y):
    if not isinstance(la, LaplaceApproximation) or not isinstance(lfx, LatentFiniteGP):
        raise F.ArgumentError("expected (LaplaceApproximation(), LatentGP(f, lik, jitter)(x), y)")
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 1 or y.shape[0] != len(lfx):
        raise F.ArgumentError("DimensionMismatch: length of y does not match the LatentFiniteGP")
    return y


def approx_lml(la: LaplaceApproximation, lfx: LatentFiniteGP, y, ctx: backend.Context | None = None, a0=None,
               full: bool = False):
    """ApproximateGPs.approx_lml(la, lfx, y): log q(y | X) of the Laplace approximation
    (gaplac_laplace_logpdf). a0: a warm start; full=True returns the backend's LaplaceResult."""
    _gate()
    y = _laplace_args(la, lfx, y)
    fx = lfx.fx
    return (ctx or backend.default_context()).laplace_logpdf(
        fx.x, fx.terms, fx.noise, lfx.lik.code, y, lik_param=lfx.lik.param, max_iter=la.maxiter, tol=la.tol, a0=a0,
        full=full)


def approx_lml_grad(la: LaplaceApproximation, lfx: LatentFiniteGP, y, ctx: backend.Context | None = None, a0=None,
                    full: bool = False):
    """(lml, dparam, djitter): approx_lml and its gradient in every term's parameter, in the order of
    kernels.lower_formula (the order of lfx.fx.terms; l / c / a Noise term's variance, 0 for Cat), and
    in the jitter (gaplac_laplace_logpdf_grad). For a GaussianLikelihood djitter is also the
    derivative in its variance. a0: a warm start; full=True returns the backend's LaplaceGradResult."""
    _gate()
    y = _laplace_args(la, lfx, y)
    fx = lfx.fx
    res = (ctx or backend.default_context()).laplace_logpdf_grad(
        fx.x, fx.terms, fx.noise, lfx.lik.code, y, lik_param=lfx.lik.param, max_iter=la.maxiter, tol=la.tol, a0=a0)
    return res if full else (res.logq, res.dparam, res.djitter)


class LaplacePosteriorGP:
    """posterior(la, lfx, y): the Gaussian approximation of the latent posterior. The mode is found
    when f_hat (or logq) is first asked for and kept as the warm start of every query; each
    mean_and_var is one gaplac_laplace_posterior_mean_var call."""

    def __init__(self, la: LaplaceApproximation, lfx: LatentFiniteGP, y, ctx: backend.Context | None = None):
        self.y = _laplace_args(la, lfx, y)
        self.la, self.lfx, self.prior, self.ctx = la, lfx, lfx.fx, ctx
        self._res = None

    def _ctx(self):
        return self.ctx or backend.default_context()

    def _mode(self):
        if self._res is None:
            _gate()
            self._res = approx_lml(self.la, self.lfx, self.y, ctx=self._ctx(), full=True)
        return self._res

    @property
    def f_hat(self):
        """The mode of the latent posterior at the training inputs."""
        return self._mode().f

    @property
    def logq(self):
        return self._mode().logq

    def mean_and_var(self, x):
        _gate()
        X = np.asarray(x, dtype=np.float64)
        if X.ndim == 1:
            X = X[:, None]
        fx, lik = self.prior, self.lfx.lik
        a0 = self._res.a if self._res is not None and self._res.converged else None
        return self._ctx().laplace_posterior_mean_var(fx.x, fx.terms, fx.noise, lik.code, self.y, X,
                                                      lik_param=lik.param, max_iter=self.la.maxiter, tol=self.la.tol,
                                                      a0=a0)

    def mean(self, x):
        return self.mean_and_var(x)[0]

    def var(self, x):
        return self.mean_and_var(x)[1]

    def fit(self, cap: int = 1024):
        """The mode found once and the factor of B kept on the device (gaplac_laplace_fit_create):
        a FittedLaplacePosteriorGP whose queries take neither Newton steps nor a factorisation.
        cap: the test points solved at once (larger queries run in chunks)."""
        _gate()
        fx, lik = self.prior, self.lfx.lik
        a0 = self._res.a if self._res is not None and self._res.converged else None
        return FittedLaplacePosteriorGP(self, self._ctx().laplace_fit(
            fx.x, fx.terms, fx.noise, lik.code, self.y, lik_param=lik.param, max_iter=self.la.maxiter,
            tol=self.la.tol, a0=a0, cap=cap))


class FittedLaplacePosteriorGP:
    """LaplacePosteriorGP.fit(): the same latent posterior behind a kept factorisation of B
    (backend.Fit of kind "laplace"). mean_and_var and var solve the test rows against the kept
    factor, mean alone is the matrix-free K(xs, X) a, mean_and_cov the joint covariance of at most
    cap points, predict the observation-space summaries. Close it (or use it as a context manager)
    to free the device memory early."""

    def __init__(self, f: LaplacePosteriorGP, fit: "backend.Fit"):
        self.f = f
        self.prior = f.prior
        self.y = f.y
        self.handle = fit

    @staticmethod
    def _xs(x):
        X = np.asarray(x, dtype=np.float64)
        return X[:, None] if X.ndim == 1 else X

    @property
    def f_hat(self):
        """The mode of the latent posterior at the training inputs."""
        return self.handle.f_hat()

    @property
    def logq(self):
        return self.handle.logq

    def mean_and_var(self, x):
        _gate()
        return self.handle.mean_var(self._xs(x))

    def mean(self, x):
        _gate()
        return self.handle.mean(self._xs(x))

    def var(self, x):
        return self.mean_and_var(x)[1]

    def mean_and_cov(self, x, noise=0.0):
        _gate()
        return self.handle.mean_cov(self._xs(x), noise_s=noise)

    def predict(self, x, ys=None, Q: int = 32):
        """(ymean, yvar[, logp]) of the observations at the rows of x under the likelihood."""
        _gate()
        return self.handle.predict(self._xs(x), ys=ys, Q=Q)

    def close(self):
        self.handle.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def posterior(*args, ctx: backend.Context | None = None):
    """AbstractGPs.posterior(fx, y) (CLI/src/select.jl:51-52, src/plotting.jl:8), or
    posterior(VFE(f(z)), fx, y): the approximate posterior of the inducing-point approximation, or
    posterior(LaplaceApproximation(), lfx, y): the Laplace approximation of a latent GP's."""
    if args and isinstance(args[0], LaplaceApproximation):
        if len(args) not in (3, 4):
            raise F.ArgumentError("posterior(LaplaceApproximation(), lfx, y)")
        return LaplacePosteriorGP(args[0], args[1], args[2], args[3] if len(args) == 4 else ctx)
    if args and isinstance(args[0], VFE):
        if len(args) not in (3, 4):
            raise F.ArgumentError("posterior(VFE(f(z)), fx, y)")
        return ApproxPosteriorGP(args[0], args[1], args[2], args[3] if len(args) == 4 else ctx)
    if len(args) not in (2, 3):
        raise F.ArgumentError("posterior(fx, y)")
    return PosteriorGP(args[0], args[1], args[2] if len(args) == 3 else ctx)


def mean_and_var(f: PosteriorGP, x):
    """AbstractGPs.mean_and_var(pgp, xtest) (src/plotting.jl:12)."""
    return f.mean_and_var(x)


def mean_and_cov(fpx: FinitePosteriorGP, ctx: backend.Context | None = None):
    """AbstractGPs.mean_and_cov(posterior(fx, y)(xs, noise)): the mean and the full M x M
    covariance at the test points (gaplac_posterior_mean_cov)."""
    return fpx.mean_and_cov(ctx)


def cov(fpx: FinitePosteriorGP, ctx: backend.Context | None = None):
    """AbstractGPs.cov(posterior(fx, y)(xs, noise))."""
    return fpx.mean_and_cov(ctx)[1]


def rand(fx: FiniteGP, n=None, z=None, rng=None, ctx: backend.Context | None = None):
    """rand(rng, fx) = cholesky(C).U' * randn(rng, N) for the zero-mean FiniteGP
    (CLI/src/sample.jl:25). The standard-normal draws stay on the host: pass z, or an rng
    (numpy Generator) to draw it.
    With n (or a 2-D z, N x n) it is rand(rng, fx, n::Int) = cholesky(C).U' * randn(rng, N, n):
    an N x n matrix from one factorisation (gaplac_rand_multi), the draws made as
    rng.standard_normal((N, n))."""
    _gate()
    if n is not None and z is not None and (np.ndim(z) != 2 or np.shape(z)[1] != int(n)):
        raise F.ArgumentError("DimensionMismatch: z must be N x n when both n and z are given")
    if z is None:
        rng = rng if rng is not None else np.random.default_rng()
        z = rng.standard_normal(len(fx) if n is None else (len(fx), int(n)))
    if isinstance(fx, FinitePosteriorGP):
        # rand(rng, posterior(fx, y)(xs, noise)[, n]) = m + L* z (gaplac_posterior_rand)
        z = np.asarray(z, dtype=np.float64)
        if z.ndim == 0 or z.ndim > 2 or z.shape[0] != len(fx):
            raise F.ArgumentError("DimensionMismatch: z does not match the test points")
        out = fx._rand(z if z.ndim == 2 else z[:, None], ctx)
        return out if z.ndim == 2 else out[:, 0]
    ctx = ctx or backend.default_context()
    if np.ndim(z) == 2:
        return ctx.rand_multi(fx.x, fx.terms, fx.noise, z)
    return ctx.rand(fx.x, fx.terms, fx.noise, z)


def make_gp(spec: F.Spec, hyperparams=None):
    """src/interface.jl:36-41 — (GP(kern), vars), checking #vars == #kernels."""
    kern, vars_ = K.kernel(F.formula(spec), hyperparams)
    kernels = K._walk_kernel(kern)
    n_noise = sum(isinstance(k, K.IndexNoiseKernel) for k in kernels)
    if len(vars_) != len(kernels) - n_noise:
        raise RuntimeError("Something went wrong with equation parsing, number of variables should == number of kernels")
    return GP(kern), vars_


def design_matrix(table, vars_) -> np.ndarray:
    """`Matrix(df[!, vars])`: one column per formula term (duplicates allowed here; the
    reference's DataFrames selection rejects duplicates)."""
    cols = [np.asarray(table[v], dtype=np.float64) for v in vars_]
    if not cols:
        n = len(next(iter(table.values()))) if isinstance(table, dict) else len(table)
        return np.zeros((n, 0))
    return np.column_stack(cols)


def _formula_likelihood(spec: F.Spec):
    """The likelihood object of a formula's slot; None for Gaussian (the FiniteGP path)."""
    lik = F.likelihood(spec)
    if isinstance(lik, F.Bernoulli):
        return BernoulliLikelihood()
    if isinstance(lik, F.Poisson):
        return PoissonLikelihood()
    return None


def select_formulae(f1: str, f2: str, table, noise: float = 0.1, ctx: backend.Context | None = None,
                    responses=None):
    """CLI/src/select.jl:21-54 (`select --formulae`): logpdf of two formulas on the same
    data and the printed "Log2 Bayes" value, which is lp1 - lp2. Both models
    run through one batched call.
    responses: a list of column names scored in place of the formulas' own response (one
    covariate table, many responses): each formula is factored once and scored against all of
    them (two logpdf_multi calls); the three results are then arrays, one entry per name.
    A formula with `Bernoulli` or `Poisson` in its likelihood slot is scored by approx_lml (the
    Laplace approximation, jitter 1e-6) in place of logpdf; responses= takes Gaussian formulas only."""
    _gate()
    ctx = ctx or backend.default_context()
    specs = [F.gp_spec(f1), F.gp_spec(f2)]
    liks = [_formula_likelihood(s) for s in specs]
    if responses is not None and any(lk is not None for lk in liks):
        raise F.ArgumentError("select_formulae: responses= scores Gaussian formulas only")
    if any(lk is not None for lk in liks):
        # a formula whose likelihood is not Gaussian: log q of its Laplace approximation (latent
        # jitter 1e-6); a Gaussian formula beside it keeps logpdf at `noise`
        lps = []
        for s, lk in zip(specs, liks):
            gp, vars_ = make_gp(s)
            X = design_matrix(table, vars_)
            y = np.asarray(table[F.response(s)], dtype=np.float64)
            if lk is None:
                lps.append(logpdf(FiniteGP(gp, X, noise), y, ctx=ctx))
            else:
                lps.append(approx_lml(LaplaceApproximation(), LatentGP(gp, lk, 1e-6)(X), y, ctx=ctx))
        lp1, lp2 = lps
        return lp1 - lp2, lp1, lp2
    if responses is not None:
        names = list(responses)
        Y = np.column_stack([np.asarray(table[r], dtype=np.float64) for r in names]) if names else None
        lps = []
        for s in specs:
            gp, vars_ = make_gp(s)
            X = design_matrix(table, vars_)
            Ys = Y if Y is not None else np.zeros((X.shape[0], 0))
            lps.append(logpdf(FiniteGP(gp, X, noise), Ys, ctx=ctx))
        lp1, lp2 = lps
        return lp1 - lp2, lp1, lp2
    if F.response(specs[0]) != F.response(specs[1]):
        # the reference reads each response separately; keep the same data flow
        pass
    lps = []
    for s in specs:
        gp, vars_ = make_gp(s)
        X = design_matrix(table, vars_)
        y = np.asarray(table[F.response(s)], dtype=np.float64)
        lps.append(logpdf(FiniteGP(gp, X, noise), y, ctx=ctx))
    lp1, lp2 = lps
    return lp1 - lp2, lp1, lp2
