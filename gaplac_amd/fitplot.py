"""`fitplot` arithmetic: the posterior of every component of a fitted GP, as a table.

The reference's README names a `fitplot` command ("diagnostic plots showing the posteriors of
different components of the GP") and lists it as not yet implemented. This module computes
what such a plot shows, without plotting: for a formula k = sum_g k_g (g = the top-level
summands, kernels.lower_formula_components) and training data (X, y),

    <label>.mean = K_g(xs, X) C^-1 y
    <label>.var  = k_g(xs, xs) - K_g(xs, X) C^-1 K_g(X, xs)          C = K(X) + noise I

for all components from one factorisation (gaplac_posterior_components). At the training
rows the table also carries the partial residual of each component,

    <label>.partial = y - sum_{h != g} mean_h

the points a fit plot scatters against component g's curve.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import abstractgps as AG
from . import backend
from . import formula as F
from . import kernels as K
from .select import df_output


def component_table(formula_text: str, table, at=None, noise: float = 0.1, products: bool = False,
                    ctx: Optional[backend.Context] = None, output: Optional[str] = None):
    """Per-component posteriors of `formula_text` fitted to `table` (column name -> values).

    at: a table with the formula's variable columns, the test points; None = the training
    rows, which adds the `.partial` columns. products: the true-product lowering
    (kernels.lower_formula). Returns the table (dict of columns: the test points' variable
    columns, then `<label>.mean`, `<label>.var` [, `<label>.partial`] per component); with
    `output` (.csv / .tsv) it is also written there (select.df_output).
    """
    AG._gate()
    ctx = ctx or backend.default_context()
    spec = F.gp_spec(formula_text)
    terms, vars_, comp, labels = K.lower_formula_components(F.formula(spec), products=products)
    X = AG.design_matrix(table, vars_)
    y = np.asarray(table[F.response(spec)], dtype=np.float64)
    pts = table if at is None else at
    Xs = X if at is None else AG.design_matrix(at, vars_)
    mean, var = ctx.posterior_components(X, terms, noise, y, Xs, comp, len(labels))
    out: Dict[str, Sequence] = {}
    for v in vars_:
        if v not in out:
            out[v] = np.asarray(pts[v], dtype=np.float64)
    for g, label in enumerate(labels):
        out[f"{label}.mean"] = mean[:, g].copy()
        out[f"{label}.var"] = var[:, g].copy()
        if at is None:
            out[f"{label}.partial"] = y - np.delete(mean, g, axis=1).sum(axis=1)
    if output is not None:
        df_output(out, output)
    return out
