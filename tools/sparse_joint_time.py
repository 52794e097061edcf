"""Timing of the joint forms of the inducing-point posterior with the
configs[2] terms: gaplac_sparse_posterior_mean_cov, _rand and _logpdf (R = 8 columns) at
Mz = 256 / 1024 / 4096 x Ms = 128 / 1024 / 4096, N = 16384 and 65536, and
gaplac_sparse_posterior_mean_var on the same shapes in the same rounds (the entry this work does
not touch: the control). Needs a GPU (fails without one).

    python tools/sparse_joint_time.py [--reps 10] [--out profiles/sparse_joint_time.json] [--nmax 65536]

After one warm-up call of every shape (the workspaces grow to their largest), the variants
alternate in one process, `reps` rounds in a freshly shuffled order; wall time per call (every
entry waits for its result and copies it to the host: mean_cov returns Ms^2 doubles), median /
min / max per variant. The covariance launches alone (the zeroing of the b rows' padding columns
and sparse_post_cov_kernel; taken through gaplac_sparse_posterior_rand, which has no mirroring
pass) are timed by the library with hipEvents, in a second context created under
GAPLAC_TAIL_TRACE (which slows the evaluation, so no wall time is taken there; the trace suffix is
.sj, "Mz Ms ms"); they do not depend on N, so that pass runs at the smaller N only. Their flops are counted as 2 Ms^2 roundup(Mz + 1, 128): the
lower triangle of each of the two products (A^T A and B^T B), Ms^2 roundup(Mz + 1, 128) apiece.
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
NS = (16384, 65536)
MZS = (256, 1024, 4096)
MSS = (128, 1024, 4096)
R_COLS = 8
JITTER = 1e-6
NOISE_S = 0.1


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    a = sys.argv[1:]
    reps = int(a[a.index("--reps") + 1]) if "--reps" in a else 10
    out = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "sparse_joint_time.json")
    nmax = int(a[a.index("--nmax") + 1]) if "--nmax" in a else max(NS)
    if reps < 10:
        raise SystemExit("at least 10 repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sparse_joint_time.py needs a GPU")
    from gaplac_amd import configs as CF
    from gaplac_amd.backend import Context

    ns = [n for n in NS if n <= nmax]
    terms = CF.config2_terms(1.5)
    data = {n: CF.config2_inputs(n) for n in ns}
    rng = np.random.default_rng(7)
    Zall = np.column_stack([rng.uniform(0, 10, max(MZS)), rng.integers(0, max(MZS), max(MZS)).astype(float)])
    Xsall = np.column_stack([rng.uniform(0, 10, max(MSS)), rng.integers(0, max(MZS), max(MSS)).astype(float)])
    E = rng.normal(size=(max(MSS), R_COLS))
    ctx = Context(0)
    variants = {}
    for n in ns:
        X, y = data[n]
        for mz in MZS:
            for ms in MSS:
                head = (X, terms, CF.NOISE_VAR, y, Zall[:mz], JITTER, Xsall[:ms])
                tag = f"N{n}_Mz{mz}_Ms{ms}"
                variants[f"mean_var_{tag}"] = lambda h=head: ctx.sparse_posterior_mean_var(*h)
                variants[f"mean_cov_{tag}"] = lambda h=head: ctx.sparse_posterior_mean_cov(*h, NOISE_S)
                variants[f"rand_{tag}"] = lambda h=head, ms=ms: ctx.sparse_posterior_rand(*h, NOISE_S, E[:ms])
                variants[f"logpdf_{tag}"] = lambda h=head, ms=ms: ctx.sparse_posterior_logpdf(*h, NOISE_S, E[:ms])
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
    # the covariance launches alone: a context that traces (the switch is read at creation)
    tdir = tempfile.mkdtemp(prefix="gaplac_sj_")
    os.environ["GAPLAC_TAIL_TRACE"] = os.path.join(tdir, "trace")
    tctx = Context(0)
    del os.environ["GAPLAC_TAIL_TRACE"]
    X, y = data[ns[0]]
    shapes = [(mz, ms) for mz in MZS for ms in MSS]
    for mz, ms in shapes:
        tctx.sparse_posterior_rand(X, terms, CF.NOISE_VAR, y, Zall[:mz], JITTER, Xsall[:ms], NOISE_S, E[:ms])  # warm-up
    open(os.path.join(tdir, "trace.sj"), "w").close()
    for _ in range(reps):
        for mz, ms in shapes:
            tctx.sparse_posterior_rand(X, terms, CF.NOISE_VAR, y, Zall[:mz], JITTER, Xsall[:ms], NOISE_S, E[:ms])
    tctx.close()
    kernel = {}
    for line in open(os.path.join(tdir, "trace.sj")):
        mz, ms, t = line.split()
        kernel.setdefault((int(mz), int(ms)), []).append(float(t))
    shutil.rmtree(tdir)
    cov = {}
    for (mz, ms), t in sorted(kernel.items()):
        s = summary(t)
        flops = 2.0 * ms * ms * ((mz + 128) // 128 * 128)
        tf = flops / (s["median_ms"] * 1e-3) / 1e12
        s.update({"flops": flops, "tflops": round(tf, 3), "frac_of_fp64_peak": round(tf / PEAK_F64_TFLOPS, 4)})
        cov[f"Mz{mz}_Ms{ms}"] = s
    ratio = {}
    for n in ns:
        for mz in MZS:
            for ms in MSS:
                tag = f"N{n}_Mz{mz}_Ms{ms}"
                c = res[f"mean_var_{tag}"]["median_ms"]
                ratio[tag] = {k: round(res[f"{k}_{tag}"]["median_ms"] / c, 4) for k in ("mean_cov", "rand", "logpdf")}
    doc = {"terms": "configs[2], l = 1.5", "jitter": JITTER, "noise_s": NOISE_S, "R": R_COLS, "reps": reps,
           "wall_ms": res, "covariance_launches": cov, "over_mean_var": ratio}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
