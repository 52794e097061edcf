"""The k-loop of the bulk tile kernels (tile_mma_neg) at every depth and
through both of its front ends, against LAPACK and the oracle, and bitwise against the loop
it replaced.

The loop stages its operands in k-chunks whose addresses are stepped, not recomputed, and
meets at its one barrier per chunk ahead of the chunk's last k-step: what can go wrong is a
chunk staged from the wrong panel column, a buffer overwritten while a wave still reads it,
the first or the last chunk, and the idle waves of a diagonal tile. So:

* whole-tile bands at every depth (tile_band_kernel): GAPLAC_TAIL_S=8, GAPLAC_PAIR_M=1,
  GAPLAC_BAND_TILES_M=1 with super-panels 1, 3 and 4 tile columns wide give K = 128 (the
  fewest chunks), 384, 512 and, at the paired steps, 768 / 1024; N = 1500 and 2049 give
  diagonal tiles and a ragged last tile row;
* the triangle kernel (tile_syrk_kernel): N = 4800 without a serial tail, default and paired,
  whose trailing triangles exceed the 512 tiles below which updates run as quadrants
  (K = 512 and 1024).

Every case: the factor against LAPACK's on the oracle's matrix at the bar of
tests/test_gpu_parity.py::test_factor_and_solve_match_lapack (||L - Lr|| <= 1e-12 ||Lr||,
which bounds every entry), logpdf, logdet and quad against oracle.restatement at 1e-12
relative (the bar of tests/test_gpu_schedules.py, whose terms and inputs these are), and for
the band cases the SHA-256 of the factor's lower triangle against
tests/golden/bulk_kloop_parent.json, recorded with the library of the commit before the loop
changed (tools/record_kloop_golden.py; that library reproduced its own hashes in two
recordings): the loop feeds every accumulator the same MFMAs in the same order, so the factor
is bitwise what it was.
The settings are read when a context is created, as in tests/test_gpu_schedules.py.
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

TERMS = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (NOISE, -1, 1.0, 3)]
NOISE_VAR = 0.1
BAND_ENV = {"GAPLAC_TAIL_S": "8", "GAPLAC_PAIR_M": "1", "GAPLAC_BAND_TILES_M": "1"}
SCHEDULES = {
    "band_spw1": {**BAND_ENV, "GAPLAC_SPW": "1"},
    "band_spw3": {**BAND_ENV, "GAPLAC_SPW": "3"},
    "band_spw4": {**BAND_ENV, "GAPLAC_SPW": "4"},
    "triangle": {"GAPLAC_TAIL_S": "0"},
    "triangle_pair": {"GAPLAC_TAIL_S": "0", "GAPLAC_PAIR_M": "1"},
}
BAND_CASES = [(name, N) for name in ("band_spw1", "band_spw3", "band_spw4") for N in (1500, 2049)]
TRIANGLE_CASES = [(name, 4800) for name in ("triangle", "triangle_pair")]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bulk_kloop_parent.json")


def inputs(N):
    # (tests/test_gpu_schedules.py's inputs)
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


def check_against_oracle(ctx, N):
    X, v = inputs(N)
    Lr, (rl, rd, rq) = reference(N)
    L, _ = ctx.factor(X, TERMS, NOISE_VAR, v)
    err, bar = np.linalg.norm(np.tril(L) - Lr), 1e-12 * np.linalg.norm(Lr)
    lp, ld, q = ctx.logpdf(X, TERMS, NOISE_VAR, v, full=True)
    print(f"N={N}: ||L-Lr|| {err:.3e} (bar {bar:.3e}) max|L-Lr| {np.max(np.abs(np.tril(L) - Lr)):.3e} "
          f"logpdf {abs(lp - rl) / abs(rl):.2e} logdet {abs(ld - rd) / abs(rl):.2e} quad {abs(q - rq) / abs(rl):.2e}")
    assert err <= bar
    assert abs(lp - rl) <= 1e-12 * abs(rl), (lp, rl)
    assert abs(ld - rd) <= 1e-12 * abs(rl), (ld, rd)
    assert abs(q - rq) <= 1e-12 * abs(rl), (q, rq)
    return L


@pytest.mark.parametrize("name,N", BAND_CASES)
def test_whole_tile_bands_every_depth(ctxs, golden, name, N):
    L = check_against_oracle(ctxs[name], N)
    assert factor_sha256(L) == golden[f"{name}_n{N}"]


@pytest.mark.parametrize("name,N", TRIANGLE_CASES)
def test_triangle_kernel(ctxs, name, N):
    check_against_oracle(ctxs[name], N)
