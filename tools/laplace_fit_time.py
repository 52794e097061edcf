"""Timing of the fitted Laplace posterior at N = 16384 with the configs[2] terms,
jitter 1e-6, under the Bernoulli and the Poisson likelihood: what the handle costs to create and
what a query costs from it, beside the calls a user had before it, all from the same rounds.

    laplace_logpdf / laplace_fit        the iteration alone / with the handle filled (create)
    lfit_mean_var_M, lfit_mean_65536    queries of the Laplace handle, M = 128 / 1024 / 4096
    lfit_mean_cov_1024                  the joint covariance of 1024 points from it
    oneshot_mean_var_M                  laplace_posterior_mean_var warm-started with a at the same M:
                                        one Newton step and the final factorisation per call
    fit_mean_var_M, fit_mean_65536      the same queries of an exact handle (gaplac_fit_create)

Needs a GPU (fails without one).

    python tools/laplace_fit_time.py [--reps 12] [--out profiles/laplace_fit_time.json] [--design]
    python tools/laplace_fit_time.py --once   (one Laplace and one exact query of 4096 points and
                                               nothing timed: the run to put under a kernel trace
                                               for the scaled build beside the unscaled one)

The data: tools/laplace_time.py's. After one warm-up call of every variant the variants alternate
in one process, `reps` rounds in a freshly shuffled order; wall time per call (every entry waits
for its result and copies it to the host), median / min / max per variant.
"""
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JITTER = 1e-6
CAP = 4096
QUERY_M = (128, 1024, 4096)
MEAN_M = 65536
COV_M = 1024
HBM_COPY_TBS = 6.29  # measured copy rate of the part


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    a = sys.argv[1:]
    reps = int(a[a.index("--reps") + 1]) if "--reps" in a else 12
    out = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "laplace_fit_time.json")
    if reps < 10:
        raise SystemExit("at least 10 repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("laplace_fit_time.py needs a GPU")
    from gaplac_amd import configs as CF
    from gaplac_amd.backend import Context

    X, v = CF.config2_inputs()
    N, D = X.shape
    terms = CF.config2_terms(1.5)
    rng = np.random.default_rng(11)
    ctx = Context(0)
    f = 0.5 * ctx.rand(X, terms, JITTER, rng.standard_normal(N))
    ys = {"bernoulli": (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-f))).astype(np.float64),
          "poisson": rng.poisson(np.exp(np.clip(f, -5.0, 3.0))).astype(np.float64)}
    Xs = X[rng.integers(0, N, MEAN_M)].copy()
    Xs[:, 0] += rng.normal(scale=0.05, size=MEAN_M)
    exact = ctx.fit(X, terms, CF.NOISE_VAR, v, cap=CAP)
    if "--once" in a:
        with ctx.laplace_fit(X, terms, JITTER, "poisson", ys["poisson"], cap=CAP) as lf:
            lf.mean_var(Xs[:4096])
            exact.mean_var(Xs[:4096])
            print(json.dumps({"N": N, "M": 4096, "iters": lf.iters, "converged": lf.converged}))
        exact.close()
        ctx.close()
        return
    fits = {lik: ctx.laplace_fit(X, terms, JITTER, lik, ys[lik], cap=CAP) for lik in ys}
    modes = {lik: fits[lik].alpha() for lik in ys}
    iters = {lik: (fits[lik].iters, fits[lik].converged) for lik in ys}

    variants = {}
    for lik in ys:
        y, lf, a0 = ys[lik], fits[lik], modes[lik]
        variants[f"{lik}:laplace_logpdf"] = lambda y=y, lik=lik: ctx.laplace_logpdf(X, terms, JITTER, lik, y)
        variants[f"{lik}:laplace_fit"] = lambda y=y, lik=lik: ctx.laplace_fit(X, terms, JITTER, lik, y, cap=128).close()
        for M in QUERY_M:
            variants[f"{lik}:lfit_mean_var_{M}"] = lambda lf=lf, M=M: lf.mean_var(Xs[:M])
            variants[f"{lik}:oneshot_mean_var_{M}"] = lambda y=y, lik=lik, a0=a0, M=M: ctx.laplace_posterior_mean_var(
                X, terms, JITTER, lik, y, Xs[:M], a0=a0)
        variants[f"{lik}:lfit_mean_{MEAN_M}"] = lambda lf=lf: lf.mean(Xs)
        variants[f"{lik}:lfit_mean_cov_{COV_M}"] = lambda lf=lf: lf.mean_cov(Xs[:COV_M])
    variants["logpdf"] = lambda: ctx.logpdf(X, terms, CF.NOISE_VAR, v)
    variants["fit_create"] = lambda: ctx.fit(X, terms, CF.NOISE_VAR, v, cap=128).close()
    for M in QUERY_M:
        variants[f"fit_mean_var_{M}"] = lambda M=M: exact.mean_var(Xs[:M])
    variants[f"fit_mean_{MEAN_M}"] = lambda: exact.mean(Xs)
    variants[f"fit_mean_cov_{COV_M}"] = lambda: exact.mean_cov(Xs[:COV_M])

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a warm-started call that did not converge would be another cost
        for fn in variants.values():  # warm-up of every shape
            fn()
        times = {k: [] for k in variants}
        order = list(variants)
        for _ in range(reps):
            rng.shuffle(order)
            for k in order:
                fn = variants[k]
                t0 = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t0) * 1e3)
    for h in list(fits.values()) + [exact]:
        h.close()
    ctx.close()
    res = {k: summary(ms) for k, ms in times.items()}
    med = {k: s["median_ms"] for k, s in res.items()}
    Np = (N + 128) // 128 * 128
    derived = {"exact_create_minus_logpdf_ms": round(med["fit_create"] - med["logpdf"], 4),
               "scaled_build_bytes_at_4096": 8 * 4096 * Np,
               "scaled_build_at_hbm_copy_rate_ms": round(8 * 4096 * Np / (HBM_COPY_TBS * 1e12) * 1e3, 4)}
    for lik in ys:
        d = {"iters": iters[lik][0], "converged": iters[lik][1],
             "create_minus_laplace_logpdf_ms": round(med[f"{lik}:laplace_fit"] - med[f"{lik}:laplace_logpdf"], 4)}
        for M in QUERY_M:
            q, o, e = med[f"{lik}:lfit_mean_var_{M}"], med[f"{lik}:oneshot_mean_var_{M}"], med[f"fit_mean_var_{M}"]
            d[f"M={M}"] = {"handle_ms": q, "oneshot_warm_ms": o, "oneshot_over_handle": round(o / q, 3),
                           "handle_cheaper": bool(q < o), "handle_minus_exact_handle_ms": round(q - e, 4)}
        derived[lik] = d
    doc = {"N": N, "terms": "configs[2], l = 1.5", "jitter": JITTER, "cap": CAP, "reps": reps, "wall_ms": res,
           "derived": derived}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc, indent=1))
    if "--design" in a:
        print("| call | median ms | min | max |")
        print("|---|---|---|---|")
        for k in variants:
            s = res[k]
            print(f"| `{k}` | {s['median_ms']:.3f} | {s['min_ms']:.3f} | {s['max_ms']:.3f} |")


if __name__ == "__main__":
    main()
