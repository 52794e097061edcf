"""Timing of the joint posterior entries at N = 16384 with the configs[2]
terms: gaplac_posterior_mean_cov at M = 128 / 1024 / 4096 and gaplac_posterior_rand at M = 1024
with R = 1 / 128, each against gaplac_posterior_mean_var at the same N and M (the unchanged
entry: the control). Needs a GPU (fails without one).

    python tools/posterior_joint_time.py [--reps 10] [--out profiles/posterior_joint_time.json]

After one warm-up call of every shape (the workspaces grow to their largest), the variants
alternate in one process, `reps` rounds in a freshly shuffled order; wall time per call (every
entry waits for its result and copies it to the host), median / min / max per variant.
post_cov_kernel alone (with the zeroing launch in front of it) is timed by the library with
hipEvents, in a second context created under GAPLAC_TAIL_TRACE (which slows the evaluation, so
no wall time is taken there); its flops are counted as N M (M + 128): 2 N 128^2 for each of
the (M/128)(M/128 + 1)/2 lower tiles, the diagonal ones as whole tiles.
"""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F64_TFLOPS = 78.6  # MI355X FP64 matrix, spec
M_COV = (128, 1024, 4096)
R_RAND = (1, 128)
M_RAND = 1024
NOISE_S = 0.1


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    a = sys.argv[1:]
    reps = int(a[a.index("--reps") + 1]) if "--reps" in a else 10
    out = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "posterior_joint_time.json")
    if reps < 10:
        raise SystemExit("at least 10 repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("posterior_joint_time.py needs a GPU")
    from gaplac_amd import configs as CF
    from gaplac_amd.backend import Context

    X, v = CF.config2_inputs()
    N, D = X.shape
    terms = CF.config2_terms(1.5)
    rng = np.random.default_rng(7)
    Mmax = max(M_COV)
    Xs = np.column_stack([rng.uniform(0, 10, Mmax), rng.integers(0, N // 3, Mmax).astype(float)])
    Z = np.asfortranarray(rng.standard_normal((M_RAND, max(R_RAND))))
    ctx = Context(0)
    variants = {}
    for m in M_COV:
        variants[f"posterior_mean_var_M{m}"] = lambda m=m: ctx.posterior_mean_var(X, terms, CF.NOISE_VAR, v, Xs[:m])
        variants[f"posterior_mean_cov_M{m}"] = (
            lambda m=m: ctx.posterior_mean_cov(X, terms, CF.NOISE_VAR, v, Xs[:m], NOISE_S))
    for r in R_RAND:
        variants[f"posterior_rand_M{M_RAND}_R{r}"] = (
            lambda r=r: ctx.posterior_rand(X, terms, CF.NOISE_VAR, v, Xs[:M_RAND], NOISE_S, Z[:, :r]))
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
    # post_cov_kernel alone: a context that traces (the switch is read at creation)
    tdir = tempfile.mkdtemp(prefix="gaplac_pc_")
    os.environ["GAPLAC_TAIL_TRACE"] = os.path.join(tdir, "trace")
    tctx = Context(0)
    del os.environ["GAPLAC_TAIL_TRACE"]
    for m in M_COV:
        tctx.posterior_mean_cov(X, terms, CF.NOISE_VAR, v, Xs[:m], NOISE_S)  # warm-up
    open(os.path.join(tdir, "trace.pc"), "w").close()
    for _ in range(reps):
        for m in M_COV:
            tctx.posterior_mean_cov(X, terms, CF.NOISE_VAR, v, Xs[:m], NOISE_S)
    tctx.close()
    kernel = {}
    for line in open(os.path.join(tdir, "trace.pc")):
        n, m, ms = line.split()
        kernel.setdefault(int(m), []).append(float(ms))
    shutil.rmtree(tdir)
    pc = {}
    for m, ms in sorted(kernel.items()):
        s = summary(ms)
        flops = float(N) * m * (m + 128.0)
        tf = flops / (s["median_ms"] * 1e-3) / 1e12
        mt = (m + 127) // 128
        s.update({"tiles": mt * (mt + 1) // 2, "flops": flops, "tflops": round(tf, 3),
                  "frac_of_fp64_peak": round(tf / PEAK_F64_TFLOPS, 4)})
        pc[f"M{m}"] = s
    excess = {}
    for m in M_COV:
        c, j = res[f"posterior_mean_var_M{m}"], res[f"posterior_mean_cov_M{m}"]
        d = j["median_ms"] - c["median_ms"]
        excess[f"mean_cov_M{m}"] = {"excess_ms": round(d, 4), "excess_over_control": round(d / c["median_ms"], 4)}
    c = res[f"posterior_mean_var_M{M_RAND}"]
    for r in R_RAND:
        d = res[f"posterior_rand_M{M_RAND}_R{r}"]["median_ms"] - c["median_ms"]
        excess[f"rand_M{M_RAND}_R{r}"] = {"excess_ms": round(d, 4), "excess_over_control": round(d / c["median_ms"], 4)}
    doc = {"N": N, "terms": "configs[2], l = 1.5", "noise_s": NOISE_S, "reps": reps, "wall_ms": res,
           "post_cov_kernel": pc, "excess_over_posterior_mean_var": excess}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
