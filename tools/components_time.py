"""Timing of gaplac_posterior_components at N = 16384 with the configs[2]
terms: G = 4 components (SqExp, OU, Cat and the Noise term) at M = 256 and M = 1024 test points,
each against gaplac_posterior_mean_var at M' = G * M test points: the same schedule and the same
number of riding rows, differing only in the cross-covariance and the finishing launch (the
control). Needs a GPU (fails without one).

    python tools/components_time.py [--reps 10] [--out profiles/components_time.json]

After one warm-up call of every shape (the workspace grows to its largest), the variants
alternate in one process, `reps` rounds in a freshly shuffled order; wall time per call (every
entry waits for its result and copies it to the host), median / min / max per variant. The
expectation: the entry's median inside the control's own min-max spread of the same run.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G = 4
MS = (256, 1024)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    a = sys.argv[1:]
    reps = int(a[a.index("--reps") + 1]) if "--reps" in a else 10
    out = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "components_time.json")
    if reps < 10:
        raise SystemExit("at least 10 repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("components_time.py needs a GPU")
    from gaplac_amd import configs as CF
    from gaplac_amd.backend import Context

    X, v = CF.config2_inputs()
    N, D = X.shape
    terms = CF.config2_terms(1.5)
    comp = [0, 1, 2, 3]  # every term (the Noise term too) a component of its own
    rng = np.random.default_rng(7)
    Mmax = G * max(MS)
    Xs = np.column_stack([rng.uniform(0, 10, Mmax), rng.integers(0, N // 3, Mmax).astype(float)])
    ctx = Context(0)
    variants = {}
    for m in MS:
        variants[f"posterior_components_G{G}_M{m}"] = (
            lambda m=m: ctx.posterior_components(X, terms, CF.NOISE_VAR, v, Xs[:m], comp, G))
        variants[f"posterior_mean_var_M{G * m}"] = (
            lambda m=m: ctx.posterior_mean_var(X, terms, CF.NOISE_VAR, v, Xs[:G * m]))
    for f in variants.values():  # warm-up of every shape
        f()
    times = {k: [] for k in variants}
    order = list(variants)
    for _ in range(reps):
        rng.shuffle(order)
        for k in order:
            f = variants[k]
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    res = {k: summary(ms) for k, ms in times.items()}
    verdict = {}
    for m in MS:
        c, e = res[f"posterior_mean_var_M{G * m}"], res[f"posterior_components_G{G}_M{m}"]
        d = e["median_ms"] - c["median_ms"]
        verdict[f"G{G}_M{m}"] = {"excess_ms": round(d, 4), "excess_over_control": round(d / c["median_ms"], 4),
                                 "control_spread_ms": round(c["max_ms"] - c["min_ms"], 4),
                                 "median_inside_control_min_max": bool(c["min_ms"] <= e["median_ms"] <= c["max_ms"])}
    doc = {"N": N, "terms": "configs[2], l = 1.5", "G": G, "comp": comp, "reps": reps, "wall_ms": res,
           "against_posterior_mean_var_at_G_M_points": verdict}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
