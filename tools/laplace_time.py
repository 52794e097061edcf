"""Timing of the Laplace approximation at N = 16384 with the configs[2] terms:
gaplac_laplace_logpdf under the Bernoulli and the Poisson likelihood beside gaplac_logpdf and
gaplac_fit_create from the same rounds. A call with `iters` Newton steps factors B iters + 1 times
(the last for log q), so call ms / (iters + 1) is the cost of one step, to be held against
fit_create (a factorisation plus a back-substitution) plus the step's own parts: two matrix-free
products, the Gram, the B build and the elementwise launches.

Needs a GPU (fails without one).

    python tools/laplace_time.py [--reps 12] [--out profiles/laplace_time.json] [--design]
    python tools/laplace_time.py --once      (one Poisson call and nothing else: the run to put
                                              under a kernel trace for the B build's time)

The data: a latent draw f = 0.5 L z (gaplac_rand on the same terms), y = Bernoulli(sigma(f)) and
y = Poisson(exp(clip(f, -5, 3))), seeded. After one warm-up call of every variant the variants
alternate in one process, `reps` rounds in a freshly shuffled order; wall time per call (every
entry waits for its result and copies it to the host), median / min / max per variant.
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
GRAM_MS = 0.23             # the Gram at N = 16384


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    a = sys.argv[1:]
    reps = int(a[a.index("--reps") + 1]) if "--reps" in a else 12
    out = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "laplace_time.json")
    if reps < 10:
        raise SystemExit("at least 10 repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("laplace_time.py needs a GPU")
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
        r = ctx.laplace_logpdf(X, terms, JITTER, "poisson", ys["poisson"], full=True)
        print(json.dumps({"N": N, "lik": "poisson", "iters": r.iters, "converged": r.converged, "logq": r.logq}))
        ctx.close()
        return
    iters = {}

    def laplace(lik):
        r = ctx.laplace_logpdf(X, terms, JITTER, lik, ys[lik], full=True)
        iters[lik] = (r.iters, r.converged)

    variants = {
        "logpdf": lambda: ctx.logpdf(X, terms, CF.NOISE_VAR, v),
        "fit_create": lambda: ctx.fit(X, terms, CF.NOISE_VAR, v, cap=128).close(),
        "laplace_bernoulli": lambda: laplace("bernoulli"),
        "laplace_poisson": lambda: laplace("poisson"),
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
    product_ms = float(N) * N / MEAN_EVALS_PER_S * 1e3
    b_bytes = 2 * 8.0 * N * (N + 1) / 2
    parts = {"two_matrix_free_products_ms": round(2 * product_ms, 4), "gram_ms": GRAM_MS,
             "b_build_at_hbm_spec_ms": round(b_bytes / (HBM_TBS * 1e12) * 1e3, 4)}
    parts_sum = sum(parts.values())
    derived = {"step_parts_from_earlier_measurements": parts, "b_build_roofline_bytes": b_bytes}
    for lik in ("bernoulli", "poisson"):
        it, conv = iters[lik]
        per = med[f"laplace_{lik}"] / (it + 1)
        derived[lik] = {"iters": it, "converged": conv, "ms_per_step": round(per, 4),
                        "step_over_fit_create": round(per / med["fit_create"], 4),
                        "step_over_logpdf": round(per / med["logpdf"], 4),
                        "excess_over_fit_create_ms": round(per - med["fit_create"], 4),
                        "excess_over_parts": round((per - med["fit_create"]) / parts_sum, 4)}
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
