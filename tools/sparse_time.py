"""Timing of the inducing-point (VFE) entries with the configs[2] terms:
gaplac_sparse_elbo at N = 16384 / 65536 / 262144 x Mz = 256 / 1024 / 4096,
gaplac_sparse_posterior_mean_var at Ms = 1024 (Mz = 1024), stage 1 alone (the posterior
evaluation of order Mz with the N rows of X riding: gaplac_posterior_mean_var on (Z, jitter)) and
gaplac_logpdf at N = 16384 and 65536 in the same rounds (the unchanged entry: the control).
Needs a GPU (fails without one).

    python tools/sparse_time.py [--reps 10] [--out profiles/sparse_time.json] [--nmax 262144]

After one warm-up call of every shape (the workspaces grow to their largest), the variants
alternate in one process, `reps` rounds in a freshly shuffled order; wall time per call (every
entry waits for its result and copies it to the host), median / min / max per variant. The
stage-2 kernels alone (the row preparation, rows_syrk_kernel and rows_syrk_reduce_kernel) are
timed by the library with hipEvents, in a second context created under GAPLAC_TAIL_TRACE (which
slows the evaluation, so no wall time is taken there); their flops are counted as N Mz (Mz + 128):
2 N 128^2 for each of the (Mz/128)(Mz/128 + 1)/2 lower tiles, the diagonal ones as whole tiles.
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
NS = (16384, 65536, 262144)
MZS = (256, 1024, 4096)
N_CONTROL = (16384, 65536)
MS_POST, MZ_POST = 1024, 1024
JITTER = 1e-6


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    a = sys.argv[1:]
    reps = int(a[a.index("--reps") + 1]) if "--reps" in a else 10
    out = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "sparse_time.json")
    nmax = int(a[a.index("--nmax") + 1]) if "--nmax" in a else max(NS)
    if reps < 10:
        raise SystemExit("at least 10 repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sparse_time.py needs a GPU")
    from gaplac_amd import configs as CF
    from gaplac_amd.backend import Context

    ns = [n for n in NS if n <= nmax]
    terms = CF.config2_terms(1.5)
    data = {n: CF.config2_inputs(n) for n in ns}
    rng = np.random.default_rng(7)
    Zall = np.column_stack([rng.uniform(0, 10, max(MZS)), rng.integers(0, max(MZS), max(MZS)).astype(float)])
    Xs = np.column_stack([rng.uniform(0, 10, MS_POST), rng.integers(0, max(MZS), MS_POST).astype(float)])
    zeros = np.zeros(max(MZS))
    ctx = Context(0)
    variants = {}
    for n in ns:
        X, y = data[n]
        for mz in MZS:
            variants[f"sparse_elbo_N{n}_Mz{mz}"] = (
                lambda X=X, y=y, mz=mz: ctx.sparse_elbo(X, terms, CF.NOISE_VAR, y, Zall[:mz], JITTER))
            variants[f"stage1_N{n}_Mz{mz}"] = (
                lambda X=X, mz=mz: ctx.posterior_mean_var(Zall[:mz], terms, JITTER, zeros[:mz], X))
        variants[f"sparse_posterior_N{n}_Mz{MZ_POST}_Ms{MS_POST}"] = (
            lambda X=X, y=y: ctx.sparse_posterior_mean_var(X, terms, CF.NOISE_VAR, y, Zall[:MZ_POST], JITTER, Xs))
        if n in N_CONTROL:
            variants[f"logpdf_N{n}"] = lambda X=X, y=y: ctx.logpdf(X, terms, CF.NOISE_VAR, y)
    for f in variants.values():  # warm-up of every shape
        f()
    times = {k: [] for k in variants}
    order = list(variants)
    for i in range(reps):
        print(f"round {i + 1}/{reps}", file=sys.stderr, flush=True)
        rng.shuffle(order)
        for k in order:
            f = variants[k]
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    res = {k: summary(ms) for k, ms in times.items()}
    # the stage-2 kernels alone: a context that traces (the switch is read at creation)
    tdir = tempfile.mkdtemp(prefix="gaplac_ss_")
    os.environ["GAPLAC_TAIL_TRACE"] = os.path.join(tdir, "trace")
    tctx = Context(0)
    del os.environ["GAPLAC_TAIL_TRACE"]
    shapes = [(n, mz) for n in ns for mz in MZS]
    for n, mz in shapes:
        tctx.sparse_elbo(data[n][0], terms, CF.NOISE_VAR, data[n][1], Zall[:mz], JITTER)  # warm-up
    open(os.path.join(tdir, "trace.ss"), "w").close()
    for _ in range(reps):
        for n, mz in shapes:
            tctx.sparse_elbo(data[n][0], terms, CF.NOISE_VAR, data[n][1], Zall[:mz], JITTER)
    chunks = {(n, mz): tctx.sparse_split(n, mz) for n, mz in shapes}
    tctx.close()
    kernel = {}
    for line in open(os.path.join(tdir, "trace.ss")):
        n, mz, ms = line.split()
        kernel.setdefault((int(n), int(mz)), []).append(float(ms))
    shutil.rmtree(tdir)
    st2 = {}
    for (n, mz), ms in sorted(kernel.items()):
        s = summary(ms)
        flops = float(n) * mz * (mz + 128.0)
        tf = flops / (s["median_ms"] * 1e-3) / 1e12
        s.update({"chunks": chunks[(n, mz)][0], "chunk_rows": chunks[(n, mz)][1], "flops": flops,
                  "tflops": round(tf, 3), "frac_of_fp64_peak": round(tf / PEAK_F64_TFLOPS, 4)})
        st2[f"N{n}_Mz{mz}"] = s
    ratio = {}
    for n in ns:
        if n in N_CONTROL:
            c = res[f"logpdf_N{n}"]["median_ms"]
            for mz in MZS:
                ratio[f"N{n}_Mz{mz}"] = round(res[f"sparse_elbo_N{n}_Mz{mz}"]["median_ms"] / c, 4)
    doc = {"terms": "configs[2], l = 1.5", "jitter": JITTER, "reps": reps, "wall_ms": res, "stage2_kernels": st2,
           "sparse_elbo_over_logpdf": ratio}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
