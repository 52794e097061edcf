"""Record tests/golden/bulk_kloop_parent.json: the SHA-256 of the factor's lower triangle for the
whole-tile band cases of tests/test_gpu_bulk_kloop.py, with the library GAPLAC_LIB_PATH names
(the control arm of tools/build_lib_at.sh: the commit before the k-loop changed).

usage (on the GPU box):  GAPLAC_LIB_PATH=tools/bin/lib_parent.so python tools/record_kloop_golden.py OUT.json
Run it twice and compare the files: a library that does not reproduce its own hashes gives no fixture.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_gpu_bulk_kloop as T  # noqa: E402


def main():
    out = sys.argv[1]
    sha = {}
    for name, N in T.BAND_CASES:
        ctx = T.make_ctx(T.SCHEDULES[name])
        X, v = T.inputs(N)
        L, _ = ctx.factor(X, T.TERMS, T.NOISE_VAR, v)
        ctx.close()
        sha[f"{name}_n{N}"] = T.factor_sha256(L)
        print(f"{name}_n{N} {sha[f'{name}_n{N}']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump({"library": "the commit before the bulk k-loop changed (tools/build_lib_at.sh)",
                   "what": "SHA-256 of the column-major lower triangle of Context.factor's L",
                   "sha256": sha}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
