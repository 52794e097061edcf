"""Record tests/golden/tail_update_parent.json: the SHA-256 of the factor's lower triangle for the
single-evaluation cases of tests/test_gpu_tail_update.py, of the batch's logpdf vector and of
the gradient's outputs, with the library GAPLAC_LIB_PATH names (the control arm of
tools/build_lib_at.sh: the commit before the tail's update loop changed).

usage (on the GPU box):  GAPLAC_LIB_PATH=tools/bin/lib_parent.so python tools/record_tail_golden.py OUT.json
Run it twice and compare the files: a library that does not reproduce its own hashes gives no fixture.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_gpu_tail_update as T  # noqa: E402


def main():
    out = sys.argv[1]
    sha = {}

    def put(key, value):
        sha[key] = value
        print(f"{key} {value}", flush=True)

    ctxs = {name: T.make_ctx(env) for name, env in T.SCHEDULES.items()}
    for name, N in T.FACTOR_CASES:
        X, v = T.inputs(N)
        L, _ = ctxs[name].factor(X, T.TERMS, T.NOISE_VAR, v)
        put(f"{name}_n{N}", T.factor_sha256(L))
    X, v = T.inputs(T.BATCH_N)
    lps, info = ctxs["default"].logpdf_batch(X, T.BATCH_MODELS, T.NOISE_VAR, v)
    assert not info.any()
    put(f"batch3_n{T.BATCH_N}", T.batch_sha256(lps))
    X, v = T.inputs(T.GRAD_N)
    put(f"grad_n{T.GRAD_N}", T.grad_sha256(ctxs["default"].logpdf_grad(X, T.TERMS, T.NOISE_VAR, v)))
    for c in ctxs.values():
        c.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump({"library": "the commit before the tail's update loop changed (tools/build_lib_at.sh)",
                   "what": "SHA-256 of the column-major lower triangle of Context.factor's L; of logpdf_batch's "
                           "logpdf vector; of logpdf_grad's logpdf, dv, dparam, dnoise bytes in that order",
                   "sha256": sha}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
