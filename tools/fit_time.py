"""Timing of the fitted posterior at N = 16384 with the configs[2] terms, each
variant against the unchanged entry that does the same work with a factorisation (the control):

    fit_create             against gaplac_logpdf (the excess: tile copy + back-substitution)
    fit.mean_var at M      against gaplac_posterior_mean_var at M,  M = 128 / 1024 / 4096
    fit.mean at M          against fit.mean_var at M where both run, M = 1024 / 65536

Needs a GPU (fails without one).

    python tools/fit_time.py [--reps 12] [--out profiles/fit_time.json] [--design]

After one warm-up call of every shape (the workspaces grow to their largest, code objects load),
the variants alternate in one process, `reps` rounds in a freshly shuffled order; wall time per
call (every entry waits for its result and copies it to the host), median / min / max per
variant. The derived rates take the wall time of the call as the kernels' time, so they are
lower bounds on the kernels' rates. --design also prints the table of DESIGN.md §10.12.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F64_TFLOPS = 78.6  # MI355X FP64 matrix, spec
HBM_TBS = 8.0           # HBM3E, spec
M_VAR = (128, 1024, 4096)
M_MEAN = (1024, 65536)
CAP = 4096


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    a = sys.argv[1:]
    reps = int(a[a.index("--reps") + 1]) if "--reps" in a else 12
    out = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "fit_time.json")
    if reps < 10:
        raise SystemExit("at least 10 repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fit_time.py needs a GPU")
    from gaplac_amd import configs as CF
    from gaplac_amd.backend import Context

    X, v = CF.config2_inputs()
    N, D = X.shape
    terms = CF.config2_terms(1.5)
    rng = np.random.default_rng(7)
    Mmax = max(M_VAR + M_MEAN)
    Xs = np.column_stack([rng.uniform(0, 10, Mmax), rng.integers(0, N // 3, Mmax).astype(float)])
    ctx = Context(0)
    fit = ctx.fit(X, terms, CF.NOISE_VAR, v, cap=CAP)
    variants = {
        "logpdf": lambda: ctx.logpdf(X, terms, CF.NOISE_VAR, v),
        "fit_create": lambda: ctx.fit(X, terms, CF.NOISE_VAR, v, cap=CAP).close(),
    }
    for m in M_VAR:
        variants[f"posterior_mean_var_M{m}"] = lambda m=m: ctx.posterior_mean_var(X, terms, CF.NOISE_VAR, v, Xs[:m])
        variants[f"fit_mean_var_M{m}"] = lambda m=m: fit.mean_var(Xs[:m])
    for m in M_MEAN:
        variants[f"fit_mean_M{m}"] = lambda m=m: fit.mean(Xs[:m])
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
    fit.close()
    ctx.close()
    res = {k: summary(ms) for k, ms in times.items()}
    med = {k: s["median_ms"] for k, s in res.items()}
    Np = (N + 1 + 127) // 128 * 128
    l_bytes = 8.0 * Np * (Np + 128) / 2  # the lower tiles, read once
    excess = med["fit_create"] - med["logpdf"]
    derived = {
        "create_excess_ms": round(excess, 4),
        "create_excess_over_logpdf": round(excess / med["logpdf"], 4),
        "one_read_of_L_at_hbm_spec_ms": round(l_bytes / (HBM_TBS * 1e12) * 1e3, 4),
        "copy_and_backsub_bytes": 3 * l_bytes,  # the copy reads and writes L, the back-substitution reads it
    }
    below = {}
    for m in M_VAR:
        q, c = med[f"fit_mean_var_M{m}"], med[f"posterior_mean_var_M{m}"]
        tf = float(m) * N * N / (q * 1e-3) / 1e12
        derived[f"mean_var_M{m}"] = {"query_over_one_shot": round(q / c, 4), "rows_solve_tflops": round(tf, 3),
                                     "frac_of_fp64_peak": round(tf / PEAK_F64_TFLOPS, 4)}
        below[f"M{m}"] = bool(q < c)
    for m in M_MEAN:
        q = med[f"fit_mean_M{m}"]
        derived[f"mean_M{m}"] = {"kernel_evaluations_per_s": round(float(m) * N / (q * 1e-3), 1)}
        if f"fit_mean_var_M{m}" in med:
            derived[f"mean_M{m}"]["mean_over_mean_var"] = round(q / med[f"fit_mean_var_M{m}"], 4)
    doc = {"N": N, "terms": "configs[2], l = 1.5", "cap": CAP, "reps": reps, "wall_ms": res, "derived": derived,
           "query_median_below_one_shot_median": below}
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
