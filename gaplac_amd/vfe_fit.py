"""Fit the inducing inputs of the VFE approximation by climbing the bound.

    Z, elbo, history = fit_inducing(ctx, X, terms, noise, y, Z0)

The only thing asked of `ctx` is sparse_elbo_grad(X, terms, noise, y, Z, jitter, wrt_z=True), so
any object with that method will do (a CPU stand-in in the tests). The kernel parameters stay
fixed: the caller has dparam from the same call and can climb in them too.
"""
from __future__ import annotations

import numpy as np

from ._native import CAT, LINEAR, OU, SQEXP
from .backend import PosDefException


def movable_columns(terms, D: int) -> list[int]:
    """Columns of Z the bound is differentiable in: read by at least one SQEXP / OU / LINEAR term
    and by no CAT term (a category has no neighbourhood to move in)."""
    moving = {int(col) for kind, col, _, _ in terms if kind in (SQEXP, OU, LINEAR)}
    fixed = {int(col) for kind, col, _, _ in terms if kind == CAT}
    return sorted(c for c in moving - fixed if 0 <= c < D)


def fit_inducing(ctx, X, terms, noise, y, Z0, jitter: float = 1e-6, cols=None, maxiter: int = 100):
    """Maximise the bound over the columns `cols` of the inducing inputs (default:
    movable_columns), starting at Z0, by L-BFGS-B on the gradient dZ of gaplac_sparse_elbo_grad_z.
    Returns (Z, elbo, history): the fitted inducing inputs (every other column as in Z0), the
    bound there and the bound at the start and after every accepted step (non-decreasing)."""
    from scipy.optimize import minimize  # (here, so that the package does not need scipy to import)

    terms = list(terms)
    Z = np.array(Z0, dtype=np.float64)
    if Z.ndim == 1:
        Z = Z[:, None]
    Mz, D = Z.shape
    cols = movable_columns(terms, D) if cols is None else [int(c) for c in cols]
    if any(c < 0 or c >= D for c in cols):
        raise ValueError(f"cols {cols} outside the {D} columns of Z")
    seen = {}
    # A trial point whose K(Z) + jitter I or S is not positive definite is rejected: the bound counts
    # as -inf there. The line search gets a finite stand-in below every value it can accept (the
    # start's bound minus ten times its size) with a zero gradient, so that its interpolation stays
    # finite and it backs off; with inf itself L-BFGS-B stops at once.
    rejected = [np.inf]

    def with_cols(v):
        Zt = Z.copy()
        Zt[:, cols] = v.reshape(Mz, len(cols))
        return Zt

    def neg_bound(v):
        key = v.tobytes()
        if key not in seen:  # (the optimiser asks for its starting point again)
            try:
                out = ctx.sparse_elbo_grad(X, terms, noise, y, with_cols(v), jitter, wrt_z=True)
            except PosDefException:
                return rejected[0], np.zeros_like(v)
            dZ = np.asarray(out[5], dtype=np.float64)
            seen[key] = (float(out[0]), -np.ascontiguousarray(dZ[:, cols]).ravel())
        return -seen[key][0], seen[key][1].copy()

    v0 = np.ascontiguousarray(Z[:, cols]).ravel()
    if v0.size == 0 or maxiter <= 0:
        elbo = float(ctx.sparse_elbo_grad(X, terms, noise, y, Z, jitter, wrt_z=True)[0])
        return Z, elbo, [elbo]
    f0, _ = neg_bound(v0)
    if v0.tobytes() not in seen:  # the start itself is not positive definite: nothing to climb from
        ctx.sparse_elbo_grad(X, terms, noise, y, Z, jitter, wrt_z=True)
    rejected[0] = f0 + 10.0 * (1.0 + abs(f0))
    history = [-f0]

    def accepted(v):
        e = seen.get(np.asarray(v, dtype=np.float64).tobytes())
        if e is not None and e[0] >= history[-1]:
            history.append(e[0])

    res = minimize(neg_bound, v0, jac=True, method="L-BFGS-B", callback=accepted, options={"maxiter": int(maxiter)})
    # (res.x is the last accepted iterate: a line search that fails puts it back)
    x = np.asarray(res.x, dtype=np.float64)
    return with_cols(x), seen[x.tobytes()][0] if x.tobytes() in seen else history[-1], history
