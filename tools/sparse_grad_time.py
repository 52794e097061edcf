"""Timing of gaplac_sparse_elbo_grad with the configs[2] terms at N = 16384 /
65536 / 262144 x Mz = 256 / 1024 / 4096, with gaplac_sparse_elbo at the same shapes in the same
rounds (the unchanged entry: the control). Needs a GPU (fails without one).

    python tools/sparse_grad_time.py [--reps 10] [--out profiles/sparse_grad_time.json] [--nmax 262144]

After one warm-up call of every shape (the workspaces grow to their largest), the variants
alternate in one process, `reps` rounds in a freshly shuffled order; wall time per call (every
entry waits for its result and copies it to the host), median / min / max per variant, and the
gradient-to-value ratio of the medians per shape. The product kernel alone (sparse_guf_kernel and
the reduction of its per-tile sums) is timed by the library with hipEvents, in a second context
created under GAPLAC_TAIL_TRACE (which slows the evaluation, so no wall time is taken there); its
flops are counted as 2 N Mz^2.

    python tools/sparse_grad_time.py --wrt-z [--out profiles/sparse_grad_z_time.json]

adds gaplac_sparse_elbo_grad_z to the same shuffled rounds, with
gaplac_sparse_elbo_grad, which that change does not touch, as its control; the traced context then
times the product both ways: sparse_guf_kernel with its reduction, and its dZ variant with the dZ
reductions, the order-Mz part and the finishing step. Per shape it reports what dZ adds to the call
beside the product alone, the cost of the second pass over the N rows that the fused epilogue avoids.
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
JITTER = 1e-6


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    a = sys.argv[1:]
    reps = int(a[a.index("--reps") + 1]) if "--reps" in a else 10
    out = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "sparse_grad_time.json")
    nmax = int(a[a.index("--nmax") + 1]) if "--nmax" in a else max(NS)
    wrt_z = "--wrt-z" in a
    if wrt_z and "--out" not in a:
        out = os.path.join(ROOT, "profiles", "sparse_grad_z_time.json")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sparse_grad_time.py needs a GPU")
    from gaplac_amd import configs as CF
    from gaplac_amd.backend import Context

    ns = [n for n in NS if n <= nmax]
    terms = CF.config2_terms(1.5)
    data = {n: CF.config2_inputs(n) for n in ns}
    rng = np.random.default_rng(7)
    Zall = np.column_stack([rng.uniform(0, 10, max(MZS)), rng.integers(0, max(MZS), max(MZS)).astype(float)])
    shapes = [(n, mz) for n in ns for mz in MZS]
    ctx = Context(0)
    variants = {}
    for n, mz in shapes:
        X, y = data[n]
        variants[f"sparse_elbo_grad_N{n}_Mz{mz}"] = (
            lambda X=X, y=y, mz=mz: ctx.sparse_elbo_grad(X, terms, CF.NOISE_VAR, y, Zall[:mz], JITTER))
        variants[f"sparse_elbo_N{n}_Mz{mz}"] = (
            lambda X=X, y=y, mz=mz: ctx.sparse_elbo(X, terms, CF.NOISE_VAR, y, Zall[:mz], JITTER))
        if wrt_z:
            variants[f"sparse_elbo_grad_z_N{n}_Mz{mz}"] = (
                lambda X=X, y=y, mz=mz: ctx.sparse_elbo_grad(X, terms, CF.NOISE_VAR, y, Zall[:mz], JITTER, wrt_z=True))
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
    # the product kernel alone: a context that traces (the switch is read at creation)
    tdir = tempfile.mkdtemp(prefix="gaplac_sg_")
    os.environ["GAPLAC_TAIL_TRACE"] = os.path.join(tdir, "trace")
    tctx = Context(0)
    del os.environ["GAPLAC_TAIL_TRACE"]
    def traced(**kw):
        for n, mz in shapes:
            tctx.sparse_elbo_grad(data[n][0], terms, CF.NOISE_VAR, data[n][1], Zall[:mz], JITTER, **kw)  # warm-up
        open(os.path.join(tdir, "trace.sg"), "w").close()
        for i in range(reps):
            print(f"kernel round {i + 1}/{reps} {kw}", file=sys.stderr, flush=True)
            for n, mz in shapes:
                tctx.sparse_elbo_grad(data[n][0], terms, CF.NOISE_VAR, data[n][1], Zall[:mz], JITTER, **kw)
        kernel = {}
        for line in open(os.path.join(tdir, "trace.sg")):
            n, mz, ms = line.split()
            kernel.setdefault((int(n), int(mz)), []).append(float(ms))
        prod = {}
        for (n, mz), ms in sorted(kernel.items()):
            s = summary(ms)
            flops = 2.0 * n * mz * mz
            tf = flops / (s["median_ms"] * 1e-3) / 1e12
            s.update({"flops": flops, "tflops": round(tf, 3), "frac_of_fp64_peak": round(tf / PEAK_F64_TFLOPS, 4)})
            prod[f"N{n}_Mz{mz}"] = s
        return prod

    prod = traced()
    prod_z = traced(wrt_z=True) if wrt_z else None
    tctx.close()
    shutil.rmtree(tdir)
    ratio = {f"N{n}_Mz{mz}": round(res[f"sparse_elbo_grad_N{n}_Mz{mz}"]["median_ms"] /
                                   res[f"sparse_elbo_N{n}_Mz{mz}"]["median_ms"], 4) for n, mz in shapes}
    doc = {"terms": "configs[2], l = 1.5", "jitter": JITTER, "reps": reps, "wall_ms": res, "product_kernel": prod,
           "grad_over_value": ratio}
    if wrt_z:
        doc["product_kernel_dz"] = prod_z
        added = {}
        for n, mz in shapes:
            k = f"N{n}_Mz{mz}"
            gz, g = res[f"sparse_elbo_grad_z_{k}"]["median_ms"], res[f"sparse_elbo_grad_{k}"]["median_ms"]
            added[k] = {"grad_z_minus_grad_ms": round(gz - g, 4), "grad_z_over_grad": round(gz / g, 4),
                        "product_alone_ms": prod[k]["median_ms"], "product_dz_alone_ms": prod_z[k]["median_ms"],
                        "traced_dz_minus_plain_ms": round(prod_z[k]["median_ms"] - prod[k]["median_ms"], 4)}
        doc["dz_added"] = added
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
