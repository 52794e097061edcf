"""Fit of the lengthscales of a latent GP under a non-Gaussian likelihood: L-BFGS-B on log q of the
Laplace approximation with the gradient of gaplac_laplace_logpdf_grad, in the
shape of vfe_fit.fit_inducing.

The only thing asked of `ctx` is laplace_logpdf_grad(X, terms, jitter, lik, y, lik_param=, a0=) with
.logq .dparam .a .converged on its result, so any object that offers it will do (tests use a CPU
stand-in built from the numpy restatement).
"""
from __future__ import annotations

import numpy as np

from . import _native
from .backend import PosDefException

LENGTHSCALE_KINDS = (_native.SQEXP, _native.OU)


def free_lengthscales(terms) -> list[int]:
    """The terms whose parameter is a lengthscale (SqExp / OU), in order."""
    return [t for t, x in enumerate(terms) if x[0] in LENGTHSCALE_KINDS]


def fit_hyperparameters(ctx, X, terms, jitter, lik, y, free=None, lik_param: float = 0.0, maxiter: int = 100):
    """Maximise log q over the lengthscales of the terms `free` (default: every SqExp / OU term),
    starting at their values in `terms`, by L-BFGS-B on the log-lengthscales (d log q / d log l =
    l d log q / d l). Every evaluation is warm-started with the previous converged evaluation's a
    (and repeated from a = 0 if it does not converge from there). Returns
    (terms, logq, history): the terms with the fitted lengthscales (everything else as given), log
    q there and log q at the start and after every accepted step (non-decreasing)."""
    from scipy.optimize import minimize  # (here, so that the package does not need scipy to import)

    terms = [tuple(t) for t in terms]
    free = free_lengthscales(terms) if free is None else [int(t) for t in free]
    for t in free:
        if t < 0 or t >= len(terms) or terms[t][0] not in LENGTHSCALE_KINDS:
            raise ValueError(f"free term {t} is not a SqExp / OU term of the {len(terms)} terms")
    if len(set(free)) != len(free):
        raise ValueError(f"free terms {free} repeat")
    seen = {}
    warm = [None]
    # A trial point at which B cannot be factored (a non-finite W) is rejected: log q counts as -inf
    # there; the line search gets a finite stand-in below every value it can accept with a zero
    # gradient (vfe_fit.fit_inducing's device), so that it backs off.
    rejected = [np.inf]

    def with_logs(v):
        out = list(terms)
        for t, lv in zip(free, v):
            kind, col, _, group = out[t]
            out[t] = (kind, col, float(np.exp(lv)), group)
        return out

    def evaluate(tt):
        try:
            res = ctx.laplace_logpdf_grad(X, tt, jitter, lik, y, lik_param=lik_param, a0=warm[0])
        except PosDefException:
            if warm[0] is None:
                raise
            res = None
        if res is None or (not res.converged and warm[0] is not None):
            # far from the previous parameters the previous a can be a start from which no step is
            # accepted, or at which W overflows (f = K a overshoots): once more from a = 0
            res = ctx.laplace_logpdf_grad(X, tt, jitter, lik, y, lik_param=lik_param, a0=None)
        if res.converged and np.all(np.isfinite(res.a)):
            warm[0] = np.array(res.a, dtype=np.float64)
        return res

    def neg_logq(v):
        key = v.tobytes()
        if key not in seen:  # (the optimiser asks for its starting point again)
            tt = with_logs(v)
            try:
                res = evaluate(tt)
            except PosDefException:
                return rejected[0], np.zeros_like(v)
            ls = np.array([tt[t][2] for t in free])
            seen[key] = (float(res.logq), -np.asarray(res.dparam, dtype=np.float64)[free] * ls)
        return -seen[key][0], seen[key][1].copy()

    if not free or maxiter <= 0:
        logq = float(evaluate(terms).logq)
        return terms, logq, [logq]
    v0 = np.log(np.array([terms[t][2] for t in free], dtype=np.float64))
    f0, _ = neg_logq(v0)
    if v0.tobytes() not in seen:  # the start itself fails: nothing to climb from
        evaluate(terms)
    rejected[0] = f0 + 10.0 * (1.0 + abs(f0))
    history = [-f0]

    def accepted(v):
        e = seen.get(np.asarray(v, dtype=np.float64).tobytes())
        if e is not None and e[0] >= history[-1]:
            history.append(e[0])

    res = minimize(neg_logq, v0, jac=True, method="L-BFGS-B", callback=accepted, options={"maxiter": int(maxiter)})
    # (res.x is the last accepted iterate: a line search that fails puts it back)
    x = np.asarray(res.x, dtype=np.float64)
    return with_logs(x), seen[x.tobytes()][0] if x.tobytes() in seen else history[-1], history
