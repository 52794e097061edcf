"""Every output of the Laplace, joint, sparse-joint, fit and row-kernel entries at the smallest shapes that cross
a tile edge and a chunk edge, as .npy files, and their sha256.

    python tools/api_dump.py --out DIR            (GAPLAC_LIB_PATH picks another build)

The behaviour check of a host-only change: summation orders are functions of the sizes alone, so two
builds (and two runs of one) must hash identically. One error case per entry goes into errors.npy. Needs a GPU.
"""
import hashlib
import itertools
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaplac_amd import _native  # noqa: E402
from gaplac_amd.backend import ArgumentError, Context, GaplacError, PosDefException  # noqa: E402

SINGLE = [(_native.SQEXP, 0, 1.5, 0), (_native.OU, 0, 3.0, 1), (_native.CAT, 1, 0.0, 2)]
PRODUCT = [(_native.SQEXP, 0, 1.5, 0), (_native.CAT, 1, 0.0, 0), (_native.OU, 0, 3.0, 1)]
MIXED = [(_native.SQEXP, 0, 1.5, 0), (_native.LINEAR, 0, 0.5, 0), (_native.OU, 0, 3.0, 1), (_native.NOISE, 0, 0.2, 1),
         (_native.CAT, 1, 0.0, 2)]  # every branch of term_k: a LINEAR and a NOISE term inside product groups
TERM_SETS = (("single", SINGLE, (0, 1, 2)), ("product", PRODUCT, (0, 0, 2)), ("mixed", MIXED, (0, 0, 1, 1, 2)))
NS, LAP_MS, MS, RS, MZS = (129, 300), (0, 3, 129, 4097), (3, 129), (1, 129), (5, 130)  # 4097 crosses LAP_CHUNK
JITTER, NOISE, NOISE_S, CAP = 1e-6, 0.1, 0.05, 1024
ROW_NS, ROW_MS, ROW_MZS = NS + (513,), MS + (513,), MZS + (513,)  # 513: more than one 512-column chunk


def inputs(n, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(0, 10, n), rng.integers(0, 7, n).astype(float)]).reshape(n, 2)


def row_entries(ctx, rng, save):
    """The entries that sum over riding rows: posterior, components, gradient, draws, matrix forms, an exact
    fit's queries and the sparse bound, per term set. A refused call raises: every entry is in the hashes."""
    for N, (tname, terms, comp) in itertools.product(ROW_NS, TERM_SETS):
        X, y, z = inputs(N, N), rng.standard_normal(N), rng.standard_normal(N)
        tag, ex = f"rows_N{N}_{tname}", (X, terms, NOISE, y)
        save(tag + "_logpdf_grad", *ctx.logpdf_grad(*ex))
        save(tag + "_rand", ctx.rand(X, terms, NOISE, z))
        for R in RS:
            multi = (X, terms, NOISE, rng.standard_normal((N, R)))
            save(f"{tag}_R{R}_multi", *ctx.logpdf_multi(*multi, full=True), ctx.rand_multi(*multi))
        with ctx.fit(*ex, cap=CAP) as fit:
            save(tag + "_fit_alpha", fit.alpha())
            for M in ROW_MS:
                Xs = inputs(M, 2000 + M)
                save(f"{tag}_M{M}_fit", fit.mean(Xs), *fit.mean_var(Xs))
                save(f"{tag}_M{M}_mean_var", *ctx.posterior_mean_var(*ex, Xs))
                save(f"{tag}_M{M}_comp", *ctx.posterior_components(*ex, Xs, [0] * len(terms)),
                     *ctx.posterior_components(*ex, Xs, comp, G=3))
        for Mz in ROW_MZS:
            sp = (*ex, inputs(Mz, 3000 + Mz), JITTER)
            save(f"{tag}_Mz{Mz}_elbo", *ctx.sparse_elbo(*sp, full=True).values())
            save(f"{tag}_Mz{Mz}_elbo_grad", *ctx.sparse_elbo_grad(*sp), *ctx.sparse_elbo_grad(*sp, wrt_z=True))
            for M in ROW_MS:
                save(f"{tag}_Mz{Mz}_M{M}_mean_var", *ctx.sparse_posterior_mean_var(*sp, inputs(M, 2000 + M)))


def main():
    out_dir = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(out_dir, exist_ok=True)
    warnings.simplefilter("ignore", RuntimeWarning)  # (a Newton iteration cut short is a result too)
    errors = []

    def save(name, *arrays):
        for i, a in enumerate(arrays):
            np.save(os.path.join(out_dir, f"{name}.{i}.npy"), np.asarray(a))

    def refused(name, call):
        try:
            call()
            errors.append(f"{name}: no error")
        except (ArgumentError, GaplacError, PosDefException) as e:  # return code and error text in the message
            errors.append(f"{name}: {type(e).__name__}: {e}")

    rng = np.random.default_rng(7)
    with Context(0) as ctx:
        for N in (0,) + NS:
            X, y = inputs(N, N), rng.standard_normal(N)
            for lik in ("bernoulli", "poisson"):
                yl = (y > 0).astype(float) if lik == "bernoulli" else np.floor(np.exp(np.clip(y, -2, 2)))
                lap = (X, SINGLE, JITTER, lik, yl)
                tag = f"lap_N{N}_{lik}"
                r = ctx.laplace_logpdf(*lap, full=True)
                save(tag + "_logpdf", r.logq, r.f, r.a, r.iters, r.converged)
                for tname, terms, _ in TERM_SETS:
                    g = ctx.laplace_logpdf_grad(X, terms, JITTER, lik, yl)
                    save(f"{tag}_grad_{tname}", g.logq, g.f, g.a, g.dparam, g.djitter, g.implicit, g.iters)
                with ctx.laplace_fit(*lap, cap=CAP) as fit:
                    save(tag + "_fit", fit.logq, fit.logdet, fit.quad, fit.iters, fit.f_hat(), fit.alpha())
                    for M in LAP_MS:
                        Xs = inputs(M, 1000 + M)
                        save(f"{tag}_M{M}_post", *ctx.laplace_posterior_mean_var(*lap, Xs, full=True))
                        save(f"{tag}_M{M}_fit_mean_var", *fit.mean_var(Xs))
                        save(f"{tag}_M{M}_fit_mean_cov", *fit.mean_cov(Xs[:CAP], NOISE_S))
            for M in (0,) + MS if N else MS[:1]:
                Xs = inputs(M, 2000 + M)
                ex = (X, SINGLE, NOISE, y, Xs)
                save(f"exact_N{N}_M{M}_mean_cov", *ctx.posterior_mean_cov(*ex, NOISE_S))
                with ctx.fit(X, SINGLE, NOISE, y, cap=CAP) as fit:
                    save(f"exact_N{N}_M{M}_fit_mean_cov", *fit.mean_cov(Xs, NOISE_S))
                for Mz in MZS if N else MZS[:1]:
                    sp = (X, SINGLE, NOISE, y, inputs(Mz, 3000 + Mz), JITTER, Xs)
                    save(f"sparse_N{N}_Mz{Mz}_M{M}_mean_cov", *ctx.sparse_posterior_mean_cov(*sp, NOISE_S))
                    for R in RS:
                        E, Ys = rng.standard_normal((M, R)), rng.standard_normal((M, R))
                        tag = f"N{N}_M{M}_R{R}"
                        keep = save if M else (lambda *a: None)  # (an empty logpdf call writes nothing)
                        if Mz == MZS[0]:
                            save(f"exact_{tag}_rand", ctx.posterior_rand(*ex, NOISE_S, E))
                            keep(f"exact_{tag}_logpdf", *ctx.posterior_logpdf(*ex, NOISE_S, Ys, full=True))
                        save(f"sparse_Mz{Mz}_{tag}_rand", ctx.sparse_posterior_rand(*sp, NOISE_S, E))
                        keep(f"sparse_Mz{Mz}_{tag}_logpdf", *ctx.sparse_posterior_logpdf(*sp, NOISE_S, Ys, full=True))
        row_entries(ctx, rng, save)
        # one refused call per entry
        X, y, Xs, Z = inputs(5, 1), np.ones(5), inputs(3, 2), inputs(2, 3)
        E = np.zeros((3, 2))
        bad = (X, SINGLE, -1.0, "poisson", y)  # jitter < 0
        refused("laplace_logpdf", lambda: ctx.laplace_logpdf(*bad))
        refused("laplace_logpdf_grad", lambda: ctx.laplace_logpdf_grad(*bad))
        refused("laplace_posterior_mean_var", lambda: ctx.laplace_posterior_mean_var(*bad, Xs))
        refused("laplace_fit", lambda: ctx.laplace_fit(*bad))
        ex, sp = (X, SINGLE, NOISE, y, Xs), (X, SINGLE, NOISE, y, Z, JITTER, Xs)
        for name, tail in (("mean_cov", ()), ("rand", (E,)), ("logpdf", (E,))):  # noise_s < 0
            refused("posterior_" + name, lambda: getattr(ctx, "posterior_" + name)(*ex, -1.0, *tail))
            refused("sparse_posterior_" + name, lambda: getattr(ctx, "sparse_posterior_" + name)(*sp, -1.0, *tail))
        with ctx.fit(X, SINGLE, NOISE, y, cap=2) as fit:
            refused("fit_mean_cov", lambda: fit.mean_cov(Xs))  # M > cap
    save("errors", np.array(errors))
    for f in sorted(os.listdir(out_dir)):
        with open(os.path.join(out_dir, f), "rb") as fh:
            print(hashlib.sha256(fh.read()).hexdigest(), "", f)


if __name__ == "__main__":
    main()
