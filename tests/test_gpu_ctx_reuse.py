"""One context across the entry points, at the smallest order where the split bulk updates
are on: a plain logpdf creates the split's second stream (`s_xrest`), the
gradient and the posterior then add the extra rows' stream and use both. The schedule is a
function of (N, mode) alone, so whatever ran on a context before, every result is bitwise
that of a fresh context.

GAPLAC_TAIL_S=16, N = 6143: 48 tile columns, the super-panel phase ends at tile column 32
(the split's minimum), `pair_m` = 40 tile rows are never met (no paired deferral), and the
triangle updates of steps 0..4 are split into two band launches and a rest.
"""
import numpy as np
import pytest

from oracle import restatement as R
from tests.conftest import gpu_available
from tests.test_gpu_switches import TERMS, ctx_with, inputs

pytestmark = pytest.mark.gpu
ENV = {"GAPLAC_TAIL_S": "16"}
N, M, NOISE_VAR = 6143, 256, 0.1


def test_context_reuse_across_entry_points():
    if not gpu_available():
        pytest.skip("no GPU")
    X, v = inputs(N)
    Xs = inputs(M, seed=7)[0]
    ctxs = [ctx_with(ENV) for _ in range(4)]
    reused, f_lp, f_grad, f_post = ctxs
    try:
        lp1 = reused.logpdf(X, TERMS, NOISE_VAR, v, full=True)
        grad = reused.logpdf_grad(X, TERMS, NOISE_VAR, v)
        post = reused.posterior_mean_var(X, TERMS, NOISE_VAR, v, Xs)
        lp2 = reused.logpdf(X, TERMS, NOISE_VAR, v, full=True)

        f_lp.reset_stats()
        f_lp.set_profiling(2)
        ref_lp = f_lp.logpdf(X, TERMS, NOISE_VAR, v, full=True)
        f_lp.set_profiling(0)
        st = f_lp.stats()
        ref_grad = f_grad.logpdf_grad(X, TERMS, NOISE_VAR, v)
        ref_post = f_post.posterior_mean_var(X, TERMS, NOISE_VAR, v, Xs)

        # the split was engaged: at this size only its head launches are event-timed bands
        print("bulk_launches", st["bulk_launches"], "syrk_launches", st["syrk_launches"])
        assert st["bulk_launches"] > st["syrk_launches"] > 0, st

        assert lp1 == ref_lp, (lp1, ref_lp)
        assert lp2 == ref_lp, (lp2, ref_lp)
        assert grad[0] == ref_grad[0] and grad[3] == ref_grad[3], (grad[0], ref_grad[0], grad[3], ref_grad[3])
        assert np.array_equal(grad[1], ref_grad[1])
        assert np.array_equal(grad[2], ref_grad[2]), (grad[2], ref_grad[2])
        assert np.array_equal(post[0], ref_post[0])
        assert np.array_equal(post[1], ref_post[1])

        oracle = R.logpdf(X, TERMS, NOISE_VAR, v)[0]
        print("logpdf", ref_lp[0], "oracle", oracle, "rel", abs(ref_lp[0] - oracle) / abs(oracle))
        assert abs(ref_lp[0] - oracle) <= 1e-9 * abs(oracle), (ref_lp[0], oracle)
    finally:
        for c in ctxs:
            c.close()  # every context closes without error
