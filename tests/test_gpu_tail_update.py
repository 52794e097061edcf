"""The update loop of the persistent tail (tail_update) in both instances of
tail_kernel, at every depth and through every kind of task list, against LAPACK and the
oracle, and bitwise against the loop it replaced.

A lane of the loop holds two adjacent matrix rows per pair of 16x16 blocks and moves them
with 16-byte accesses, steps its fragment addresses in a scalar, and keeps a ring of eight
k-steps in flight whose slots are refilled right behind the MFMAs that read them. What can go
wrong is a row pair mapped to the wrong C element, a ring slot overwritten before its MFMAs
issued, the ring's fill or drain at the smallest and the largest depth, the ragged last tile
row, the 64x64 quadrant instance, and either template instance of the kernel. So:

* N = 1500 (12 tile columns) and N = 2049 (17, two live rows in the last tile) at the default
  settings: the whole matrix in the tail with the Gram inside it (tail_kernel<true>), deep
  K = 512 tasks from tile column 8 on, K = 256 paired near tiles, K = 128 whole tiles and
  quadrant tasks in the last columns;
* N = 2049 with GAPLAC_TAIL_S=12: five bulk tile columns, then a 12-column tail without the
  Gram (tail_kernel<false>, the instance the 16k evaluation runs);
* logpdf_batch of 3 models at N = 1500: batched lists have deep width 8 (K = 1024 tasks) and
  whole-tile TRSM tasks;
* one gradient evaluation at N = 1500: the extra-row tasks go through the same loop.

The single evaluations: the factor against LAPACK's on the oracle's matrix at
||L - Lr|| <= 1e-12 ||Lr||, logpdf, logdet and quad against oracle.restatement at 1e-12
relative (the bars, terms and inputs of tests/test_gpu_bulk_kloop.py). The batch returns one
logpdf per model and no factor: each logpdf against the oracle at 1e-12 relative. The gradient
at the bar of tests/test_gpu_grad.py. Bitwise: the SHA-256 of the factor's lower triangle, of
the batch's logpdf vector and of the gradient's outputs against
tests/golden/tail_update_parent.json, recorded with the library of the commit before the loop
changed (tools/record_tail_golden.py; that library reproduced its own hashes in two
recordings): every accumulator receives the same MFMAs with the same operands in the same k
order, so every output is bitwise what it was.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from gaplac_amd._native import CAT, NOISE, OU, SQEXP
from gaplac_amd.backend import Context
from oracle import restatement as R
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

# (tests/test_gpu_bulk_kloop.py's terms and inputs)
TERMS = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (NOISE, -1, 1.0, 3)]
NOISE_VAR = 0.1
SCHEDULES = {"default": {}, "tail12": {"GAPLAC_TAIL_S": "12"}}
FACTOR_CASES = [("default", 1500), ("default", 2049), ("tail12", 2049)]
BATCH_N = 1500
BATCH_MODELS = [
    TERMS,
    [(SQEXP, 0, 0.7, 0), (CAT, 1, 0.0, 1), (NOISE, -1, 0.5, 2)],
    [(OU, 0, 2.0, 0), (SQEXP, 0, 4.0, 1), (NOISE, -1, 2.0, 2)],
]
GRAD_N = 1500
GRAD_TOL = 1e-9  # tests/test_gpu_grad.py
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tail_update_parent.json")


def inputs(N):
    rng = np.random.default_rng(N)
    X = np.column_stack([rng.uniform(0, 10, N), rng.integers(0, max(1, N // 3), N).astype(float)])
    return X, rng.standard_normal(N)


def make_ctx(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def factor_sha256(L):
    """SHA-256 of the factor's lower triangle (column-major bytes, the upper triangle zeroed)."""
    return hashlib.sha256(np.asfortranarray(np.tril(L)).tobytes(order="F")).hexdigest()


def batch_sha256(lps):
    return hashlib.sha256(np.ascontiguousarray(lps, dtype=np.float64).tobytes()).hexdigest()


def grad_sha256(got):
    lp, dv, dp, dn = got
    h = hashlib.sha256()
    for a in (np.float64(lp), dv, dp, np.float64(dn)):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def reference(N):
    """(Lr, (logpdf, logdet, quad)) of the oracle at N: computed once, shared, never changed."""
    X, v = inputs(N)
    Lr = R.cholesky_lower(X, TERMS, NOISE_VAR)
    Lr.setflags(write=False)
    return Lr, R.logpdf(X, TERMS, NOISE_VAR, v)


@pytest.fixture(scope="module")
def ctxs():
    if not gpu_available():
        pytest.skip("no GPU")
    cs = {name: make_ctx(env) for name, env in SCHEDULES.items()}
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["sha256"]


@pytest.mark.parametrize("name,N", FACTOR_CASES)
def test_factor_every_task_class(ctxs, golden, name, N):
    ctx = ctxs[name]
    X, v = inputs(N)
    Lr, (rl, rd, rq) = reference(N)
    L, _ = ctx.factor(X, TERMS, NOISE_VAR, v)
    err, bar = np.linalg.norm(np.tril(L) - Lr), 1e-12 * np.linalg.norm(Lr)
    lp, ld, q = ctx.logpdf(X, TERMS, NOISE_VAR, v, full=True)
    print(f"{name} N={N}: ||L-Lr|| {err:.3e} (bar {bar:.3e}) max|L-Lr| {np.max(np.abs(np.tril(L) - Lr)):.3e} "
          f"logpdf {abs(lp - rl) / abs(rl):.2e} logdet {abs(ld - rd) / abs(rl):.2e} quad {abs(q - rq) / abs(rl):.2e}")
    assert err <= bar
    assert abs(lp - rl) <= 1e-12 * abs(rl), (lp, rl)
    assert abs(ld - rd) <= 1e-12 * abs(rl), (ld, rd)
    assert abs(q - rq) <= 1e-12 * abs(rl), (q, rq)
    assert factor_sha256(L) == golden[f"{name}_n{N}"]


def test_batch_deep8(ctxs, golden):
    X, v = inputs(BATCH_N)
    lps, info = ctxs["default"].logpdf_batch(X, BATCH_MODELS, NOISE_VAR, v)
    assert not info.any()
    for m, terms in enumerate(BATCH_MODELS):
        rl = reference(BATCH_N)[1][0] if m == 0 else R.logpdf(X, terms, NOISE_VAR, v)[0]
        print(f"batch model {m}: logpdf {abs(lps[m] - rl) / abs(rl):.2e}")
        assert abs(lps[m] - rl) <= 1e-12 * abs(rl), (m, lps[m], rl)
    assert batch_sha256(lps) == golden[f"batch3_n{BATCH_N}"]


def test_gradient_extra_rows(ctxs, golden):
    X, v = inputs(GRAD_N)
    got = ctxs["default"].logpdf_grad(X, TERMS, NOISE_VAR, v)
    lp, dv, dp, dn = got
    rlp, rdv, rdp, rdn = R.logpdf_grad(X, TERMS, NOISE_VAR, v)
    scale, scalen = R.logpdf_grad_scale(X, TERMS, NOISE_VAR, v)
    print(f"grad N={GRAD_N}: logpdf {abs(lp - rlp) / abs(rlp):.2e} dv {np.max(np.abs(dv - rdv)):.2e} "
          f"dparam {[f'{abs(dp[t] - rdp[t]) / max(abs(rdp[t]) + scale[t], 1e-300):.2e}' for t in range(len(rdp))]} "
          f"dnoise {abs(dn - rdn) / (abs(rdn) + scalen):.2e}")
    assert abs(lp - rlp) <= GRAD_TOL * abs(rlp)
    assert np.max(np.abs(dv - rdv)) <= GRAD_TOL * max(1.0, np.max(np.abs(rdv)))
    for t in range(len(rdp)):
        assert abs(dp[t] - rdp[t]) <= GRAD_TOL * (abs(rdp[t]) + scale[t]), (t, dp[t], rdp[t], scale[t])
    assert abs(dn - rdn) <= GRAD_TOL * (abs(rdn) + scalen), (dn, rdn)
    assert grad_sha256(got) == golden[f"grad_n{GRAD_N}"]
