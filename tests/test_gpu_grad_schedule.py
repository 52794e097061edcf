"""gaplac_logpdf_grad's super-panel schedule and C^-1 tiling against the gradient restatement at the
sizes where they take their other paths, with test_gpu_grad.check_grad's rule:
logpdf within 1e-9 relative, dv within 1e-9 of max |dv|, every dparam and dnoise within 1e-9 of
(|ref| + oracle.logpdf_grad_scale).

The gradient never takes the persistent tail (tail_allowed), so every tile column goes through
super-panels, the identity rows Y = L^-T on two streams of their own (s_extra, s_xrest) whose waits
alternate between two events per kind and matter from the third super-panel on. With
nt = ceil((N + 1) / 128), m = ceil(N / 128) and the super-panel width W (GAPLAC_SPW, read when a
context is created):

  N     W  nt  what it reaches (tests/test_grad_plan.py asserts these counts)
  640   1   6  six super-panels: both parities of ev_xc / ev_xr used twice, at the smallest size
  2049  4  17  five super-panels, the last one column wide; six C^-1 super-tiles, the last super-row
               holding a single tile row
  3400  4  27  seven super-panels, the last three wide; at p = 3 the s_xrest update is 12 x 11 = 132
               tiles, the only extra-row launch of at least XR_TILE_MIN = 128: tile_syrk_kernel with
               the rectangular tile_decode, one strip of 8 rows plus a remainder of 4; ten C^-1
               super-tiles, so XCD queues 0 and 1 hold two and the others are padded
  4000  8  32  K = 1024 updates; s_extra updates of 16 x 8 and 24 x 8 tiles, s_xrest updates of 8 x 16
               and 16 x 8 and the chain steps c = 25, 26, 27 as whole tiles, c = 28 (112) on quadrants

Inputs: test_gpu_grad.test_sizes_composite's (three columns; SqExp, OU, Cat, Linear, Noise; noise 0.1;
seed = N). The product-group cases take test_gpu_grad.test_product_groups' formula and its columns
(uniform, normal, 20 categories: with the composite columns its Cat factor would sit on the normal
column, all values distinct, and the group would be diagonal), seed = N.

The oracle is computed once per (N, formula) and shared by every context (a module-level cache);
its two routes agree to 1e-12 of the addends at these sizes (tests/test_grad_plan.py).
"""
import functools
import os

import numpy as np
import pytest

from gaplac_amd._native import CAT, LINEAR, NOISE, OU, SQEXP
from gaplac_amd.backend import Context
from oracle import restatement as R
from tests.backward_error import worst_ratio
from tests.conftest import gpu_available
from tests.test_gpu_grad import check_grad

pytestmark = pytest.mark.gpu

NOISE_VAR = 0.1
COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (LINEAR, 2, 0.5, 3), (NOISE, -1, 0.05, 4)]
PRODUCT = [(SQEXP, 0, 1.3, 0), (LINEAR, 1, 0.4, 0), (CAT, 2, 0.0, 0), (OU, 0, 2.5, 1), (NOISE, -1, 0.2, 2)]
FORMULAS = {"composite": COMPOSITE, "product": PRODUCT}
CONTEXTS = {
    "default": {},
    "spw1": {"GAPLAC_SPW": "1"},
    "spw8": {"GAPLAC_SPW": "8"},
    "serial": {"GAPLAC_SERIAL": "1"},
    "unfused": {"GAPLAC_GRAD_FUSED": "0"},
}
# (N, context) of the table above
TABLE = [(640, "spw1"), (2049, "default"), (3400, "default"), (4000, "spw8")]


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


@pytest.fixture(scope="module")
def ctxs():
    if not gpu_available():
        pytest.skip("no GPU")
    cs = {name: make_ctx(env) for name, env in CONTEXTS.items()}
    yield cs
    for c in cs.values():
        c.close()


@functools.lru_cache(maxsize=None)
def inputs(N, formula):
    rng = np.random.default_rng(N)
    if formula == "composite":
        X = np.column_stack([rng.uniform(0, 10, N), rng.integers(0, max(1, N // 3), N).astype(float),
                             rng.normal(size=N)])
    else:
        X = np.column_stack([rng.uniform(0, 5, N), rng.normal(size=N), rng.integers(0, 20, N).astype(float)])
    v = rng.normal(size=N)
    X.setflags(write=False)
    v.setflags(write=False)
    return X, v


@functools.lru_cache(maxsize=None)
def oracle(N, formula):
    """((logpdf, dv, dparam, dnoise), dparam's scale, dnoise's scale), computed once and left unchanged."""
    X, v = inputs(N, formula)
    ref = R.logpdf_grad(X, FORMULAS[formula], NOISE_VAR, v)
    sc, scn = R.logpdf_grad_scale(X, FORMULAS[formula], NOISE_VAR, v)
    for a in (ref[1], ref[2], sc):
        a.setflags(write=False)
    return ref, sc, scn


_gpu = {}


def gpu_grad(ctxs, cname, N, formula="composite"):
    """One evaluation per (context, N, formula), shared by the tests that compare contexts."""
    key = (cname, N, formula)
    if key not in _gpu:
        X, v = inputs(N, formula)
        _gpu[key] = ctxs[cname].logpdf_grad(X, FORMULAS[formula], NOISE_VAR, v)
    return _gpu[key]


def report(what, got, N, formula="composite"):
    """The worst figure of each output against the oracle, in units of its tolerance's reference."""
    (rlp, rdv, rdp, rdn), sc, scn = oracle(N, formula)
    lp, dv, dp, dn = got
    print(f"GRADSCHED {what} N={N} {formula}: logpdf {abs(lp - rlp) / abs(rlp):.2e}, "
          f"dv {np.max(np.abs(dv - rdv)) / max(1.0, np.max(np.abs(rdv))):.2e}, "
          f"dparam {worst_ratio(np.abs(np.asarray(dp) - rdp), np.abs(rdp) + sc):.2e}, "
          f"dnoise {abs(dn - rdn) / (abs(rdn) + scn):.2e}")


def check(what, got, N, formula="composite"):
    ref, sc, scn = oracle(N, formula)
    report(what, got, N, formula)
    check_grad(got, ref, sc, scn)


@pytest.mark.parametrize("N,cname", TABLE, ids=[f"{n}-{c}" for n, c in TABLE])
def test_schedule_against_oracle(ctxs, N, cname):
    check(cname, gpu_grad(ctxs, cname, N), N)


@pytest.mark.parametrize("N", [3400, 4000])
def test_serial_schedule(ctxs, N):
    """GAPLAC_SERIAL=1 merges the two extra-row updates of a super-panel into one launch, so a tile can
    go through another kernel (whole tile against quadrants): every tile still receives the same
    super-panels in the same order with the same k order, so the serial gradient is held to the
    oracle and to the multi-stream result (1e-10 of max |dparam| + 1 and of |dnoise| + 1,
    test_gpu_switches.test_grad_unfused's bar; logpdf and dv bitwise). Measured: all four outputs
    bitwise equal at both sizes, which is asserted."""
    got = gpu_grad(ctxs, "serial", N)
    check("serial", got, N)
    base = gpu_grad(ctxs, "default", N)
    lp, dv, dp, dn = got
    blp, bdv, bdp, bdn = base
    ddp = float(np.max(np.abs(np.asarray(dp) - np.asarray(bdp))))
    print(f"GRADSCHED serial-vs-default N={N}: max |dparam diff| {ddp:.3e} (scale {np.abs(bdp).max() + 1.0:.3e}), "
          f"|dnoise diff| {abs(dn - bdn):.3e}, logpdf equal {lp == blp}, dv equal {np.array_equal(dv, bdv)}")
    assert lp == blp
    assert np.array_equal(dv, bdv)
    assert ddp <= 1e-10 * (np.abs(bdp).max() + 1.0), (dp, bdp)
    assert abs(dn - bdn) <= 1e-10 * (abs(bdn) + 1.0), (dn, bdn)
    assert np.array_equal(dp, bdp) and dn == bdn, (dp, bdp, dn, bdn)


@pytest.mark.parametrize("N", [2049, 3400])
def test_unfused_contraction(ctxs, N):
    """GAPLAC_GRAD_FUSED=0: cinv_tile_kernel writes -C^-1 over the factor storage, grad_contract_kernel
    contracts it, over six and ten super-tiles."""
    check("unfused", gpu_grad(ctxs, "unfused", N), N)


@pytest.mark.parametrize("N", [2049, 3400])
def test_product_groups(ctxs, N):
    """A product group forces the stored -C^-1 and grad_contract_kernel's product rule in the default
    context, past one super-tile."""
    check("default", gpu_grad(ctxs, "default", N, "product"), N, "product")


def test_repeat_is_bitwise(ctxs):
    """Two evaluations at N = 3400 with a logpdf at N = 4000 (the plain layout, lda = Np, over the same
    workspace) and a gradient at N = 2049 (another tile list and C^-1 list) between them."""
    c = ctxs["default"]
    X, v = inputs(3400, "composite")
    a = c.logpdf_grad(X, COMPOSITE, NOISE_VAR, v)
    Xb, vb = inputs(4000, "composite")
    c.logpdf(Xb, COMPOSITE, NOISE_VAR, vb)
    Xc, vc = inputs(2049, "composite")
    c.logpdf_grad(Xc, COMPOSITE, NOISE_VAR, vc)
    b = c.logpdf_grad(X, COMPOSITE, NOISE_VAR, v)
    assert a[0] == b[0] and a[3] == b[3]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    check("default, after other sizes", b, 3400)


def test_row_permutation(ctxs):
    """The rows of X permuted with v: every pair (i, j) moves to another tile and another XCD queue;
    logpdf, dparam and dnoise stay within the oracle's rule and dv is permuted."""
    N = 3400
    X, v = inputs(N, "composite")
    perm = np.random.default_rng(N + 1).permutation(N)
    got = ctxs["default"].logpdf_grad(np.ascontiguousarray(X[perm]), COMPOSITE, NOISE_VAR, np.ascontiguousarray(v[perm]))
    (rlp, rdv, rdp, rdn), sc, scn = oracle(N, "composite")
    back = np.empty(N)
    back[perm] = got[1]
    report("default, rows permuted", (got[0], back, got[2], got[3]), N)
    check_grad(got, (rlp, rdv[perm], rdp, rdn), sc, scn)
