"""Timing of the Laplace gradient at N = 16384 with the configs[2] terms:
gaplac_laplace_logpdf_grad under the Bernoulli and the Poisson likelihood beside
gaplac_laplace_logpdf, gaplac_logpdf_grad and gaplac_logpdf from the same rounds. Both Laplace
entries take the same Newton steps, so call - laplace_logpdf's call is the gradient stage: the
identity rows riding in the final factorisation, the row scaling, the products by Y, the
contraction and the bilinear form. It is held against logpdf_grad - logpdf, the same stage of the
exact gradient (identity rows, alpha, contraction).

Needs a GPU (fails without one).

    python tools/laplace_grad_time.py [--reps 12] [--out profiles/laplace_grad_time.json] [--design]
    python tools/laplace_grad_time.py --once    (one Poisson gradient call and nothing else: the run
                                                 to put under a kernel trace)

The data and the rounds are tools/laplace_time.py's: a latent draw f = 0.5 L z, y = Bernoulli(sigma(f))
and y = Poisson(exp(clip(f, -5, 3))), seeded; after one warm-up call of every variant the variants
alternate in one process, `reps` rounds in a freshly shuffled order; wall time per call, median /
min / max per variant.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0  # HBM3E, spec
JITTER = 1e-6
MEAN_EVALS_PER_S = 2.5e11  # the matrix-free mean kernel, profiles/fit_time.json (fit_mean at M = 65536)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    a = sys.argv[1:]
    reps = int(a[a.index("--reps") + 1]) if "--reps" in a else 12
    out = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "laplace_grad_time.json")
    if reps < 10:
        raise SystemExit("at least 10 repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("laplace_grad_time.py needs a GPU")
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
    if "--once" in a:
        r = ctx.laplace_logpdf_grad(X, terms, JITTER, "poisson", ys["poisson"])
        print(json.dumps({"N": N, "lik": "poisson", "iters": r.iters, "converged": r.converged, "logq": r.logq,
                          "dparam": list(r.dparam), "djitter": r.djitter, "implicit": list(r.implicit)}))
        ctx.close()
        return
    iters = {}

    def value(lik):
        r = ctx.laplace_logpdf(X, terms, JITTER, lik, ys[lik], full=True)
        iters["value_" + lik] = (r.iters, r.converged)

    def grad(lik):
        r = ctx.laplace_logpdf_grad(X, terms, JITTER, lik, ys[lik])
        iters["grad_" + lik] = (r.iters, r.converged)

    variants = {
        "logpdf": lambda: ctx.logpdf(X, terms, CF.NOISE_VAR, v),
        "logpdf_grad": lambda: ctx.logpdf_grad(X, terms, CF.NOISE_VAR, v),
        "laplace_bernoulli": lambda: value("bernoulli"),
        "laplace_poisson": lambda: value("poisson"),
        "laplace_grad_bernoulli": lambda: grad("bernoulli"),
        "laplace_grad_poisson": lambda: grad("poisson"),
    }
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
    ctx.close()
    res = {k: summary(ms) for k, ms in times.items()}
    med = {k: s["median_ms"] for k, s in res.items()}
    exact_stage = med["logpdf_grad"] - med["logpdf"]
    scale_bytes = 2 * 8.0 * N * (N + 1) / 2  # Y's upper triangle read and written once
    derived = {"exact_gradient_stage_ms": round(exact_stage, 4),
               "row_scale_roofline_bytes": scale_bytes,
               "row_scale_at_hbm_spec_ms": round(scale_bytes / (HBM_TBS * 1e12) * 1e3, 4),
               "bilinear_pairs": float(N) * N,
               "bilinear_at_fit_mean_rate_ms": round(float(N) * N / MEAN_EVALS_PER_S * 1e3, 4)}
    for lik in ("bernoulli", "poisson"):
        stage = med[f"laplace_grad_{lik}"] - med[f"laplace_{lik}"]
        derived[lik] = {"iters": iters["grad_" + lik][0], "converged": iters["grad_" + lik][1],
                        "same_steps_as_value": iters["grad_" + lik] == iters["value_" + lik],
                        "gradient_stage_ms": round(stage, 4),
                        "stage_over_exact_stage": round(stage / exact_stage, 4),
                        "call_over_value_call": round(med[f"laplace_grad_{lik}"] / med[f"laplace_{lik}"], 4)}
    doc = {"N": N, "terms": "configs[2], l = 1.5", "jitter": JITTER, "reps": reps, "wall_ms": res, "derived": derived}
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
