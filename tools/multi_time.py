"""Timing of the matrix forms at N = 16384 with the configs[2] terms:
gaplac_logpdf_multi_device and gaplac_rand_multi against the single-vector entries and the
posterior, whose schedule logpdf_multi shares. Needs a GPU (fails without one).

    python tools/multi_time.py [--reps 10] [--out profiles/multi_time.json]

After one warm-up call of every shape (the workspaces grow to their largest), the variants
alternate in one process, `reps` rounds in a freshly shuffled order; wall time per call
(every entry waits for its result), median / min / max per variant. The L Z kernel alone is timed by the library with
hipEvents around its launch, in a second context created under GAPLAC_TAIL_TRACE (which slows
the evaluation, so no wall time is taken there); its flops are N (N + 1) R.
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
R_LOGPDF = (1, 128, 1024, 4096)
R_RAND = (1, 128, 1024)
M_POST = 1024


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    a = sys.argv[1:]
    reps = int(a[a.index("--reps") + 1]) if "--reps" in a else 10
    out = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "multi_time.json")
    if reps < 10:
        raise SystemExit("at least 10 repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("multi_time.py needs a GPU")
    from gaplac_amd import configs as CF
    from gaplac_amd.backend import Context

    X, v = CF.config2_inputs()
    N, D = X.shape
    terms = CF.config2_terms(1.5)
    rng = np.random.default_rng(7)
    Y = rng.standard_normal((N, max(R_LOGPDF)))
    Z = np.asfortranarray(rng.standard_normal((N, max(R_RAND))))
    Xs = np.column_stack([rng.uniform(0, 10, M_POST), rng.integers(0, N // 3, M_POST).astype(float)])
    dX = torch.tensor(X.T.copy(), device="cuda")   # (D, N) row-major = N x D column-major, ld N
    dv = torch.tensor(v, device="cuda")
    dY = torch.tensor(Y.T.copy(), device="cuda")   # N x R column-major, ld N
    torch.cuda.synchronize()
    ctx = Context(0)
    variants = {"logpdf_device": lambda: ctx.logpdf_device(N, D, dX.data_ptr(), N, terms, CF.NOISE_VAR, dv.data_ptr())}
    for r in R_LOGPDF:
        variants[f"logpdf_multi_device_R{r}"] = (
            lambda r=r: ctx.logpdf_multi_device(N, D, dX.data_ptr(), N, terms, CF.NOISE_VAR, r, dY.data_ptr(), N))
    variants[f"posterior_mean_var_M{M_POST}"] = lambda: ctx.posterior_mean_var(X, terms, CF.NOISE_VAR, v, Xs)
    variants["rand"] = lambda: ctx.rand(X, terms, CF.NOISE_VAR, Z[:, 0])
    for r in R_RAND:
        variants[f"rand_multi_R{r}"] = lambda r=r: ctx.rand_multi(X, terms, CF.NOISE_VAR, Z[:, :r])
    for f in variants.values():  # warm-up of every shape
        f()
    times = {k: [] for k in variants}
    order = list(variants)
    for _ in range(reps):
        # a new order every round: a call right after rand_multi's large host copies runs ~1.5 ms
        # slower, whichever variant it is (in a fixed order that was always logpdf_device)
        rng.shuffle(order)
        for k in order:
            f = variants[k]
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    res = {k: summary(ms) for k, ms in times.items()}
    # the L Z kernel alone: a context that traces (the switch is read at creation)
    tdir = tempfile.mkdtemp(prefix="gaplac_lz_")
    os.environ["GAPLAC_TAIL_TRACE"] = os.path.join(tdir, "trace")
    tctx = Context(0)
    del os.environ["GAPLAC_TAIL_TRACE"]
    for r in R_RAND:
        tctx.rand_multi(X, terms, CF.NOISE_VAR, Z[:, :r])  # warm-up
    open(os.path.join(tdir, "trace.lz"), "w").close()
    for _ in range(reps):
        for r in R_RAND:
            tctx.rand_multi(X, terms, CF.NOISE_VAR, Z[:, :r])
    tctx.close()
    kernel = {}
    for line in open(os.path.join(tdir, "trace.lz")):
        n, r, ms = line.split()
        kernel.setdefault(int(r), []).append(float(ms))
    shutil.rmtree(tdir)
    lz = {}
    for r, ms in sorted(kernel.items()):
        s = summary(ms)
        tf = N * (N + 1.0) * r / (s["median_ms"] * 1e-3) / 1e12
        s.update({"flops": N * (N + 1.0) * r, "tflops": round(tf, 3), "frac_of_fp64_peak": round(tf / PEAK_F64_TFLOPS, 4)})
        lz[f"R{r}"] = s
    post, single = res[f"posterior_mean_var_M{M_POST}"], res["logpdf_device"]
    spread = post["max_ms"] - post["min_ms"]
    gap = post["median_ms"] - single["median_ms"]  # the rows' fixed cost
    matvec = res["rand"]["median_ms"] - single["median_ms"]  # the mat-vec rand_multi replaces
    checks = {
        "posterior_spread_ms": round(spread, 4),
        "posterior_over_logpdf_gap_ms": round(gap, 4),
        "rand_minus_logpdf_ms": round(matvec, 4),
        "multi_R1024_within_posterior": res["logpdf_multi_device_R1024"]["median_ms"] <= post["median_ms"] + spread,
        "multi_R1_within_single_plus_gap": res["logpdf_multi_device_R1"]["median_ms"]
        <= single["median_ms"] + (single["max_ms"] - single["min_ms"]) + gap,
        "lz_R128_under_128_matvecs": lz["R128"]["median_ms"] < 128 * matvec,
    }
    doc = {"N": N, "terms": "configs[2], l = 1.5", "reps": reps, "wall_ms": res, "lz_kernel": lz, "checks": checks}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
