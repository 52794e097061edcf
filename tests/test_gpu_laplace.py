"""The Laplace approximation (gaplac_laplace_logpdf / _posterior_mean_var, HIP through the C-ABI)
against the numpy restatement tests/laplace_oracle.py.

Bars: log q within 1e-9 max(1, |log q|) of the oracle (the project's bar; the iteration's path
dependence is some 1e-13), the mode f within 1e-9 max(1, max |f|), the posterior under the bars of
tests/test_gpu_posterior.py (mean within 1e-9 max(1, max |mean|), variance within 1e-9 max(1,
kdiag)). The oracle polishes its mode with two further Newton steps, the library stops where the
objective's change meets tol = 1e-12; Newton's quadratic convergence puts that iterate some 1e-12
from the mode. Iterations: at most 12 (the restatement takes 1 to 7 on these inputs), Gaussian at
most 3 (the approximation is exact: one step reaches the mode, one confirms it). Identical calls
are bitwise equal.
"""
import os
import warnings

import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd import abstractgps as AG
from gaplac_amd import formula as F
from gaplac_amd.backend import ArgumentError, Context, PosDefException
from tests import laplace_oracle as LO
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
TOL = 1e-9
SIZES = [1, 5, 127, 128, 129, 300, 700, 1000]
POSTERIOR_SIZES = [(1, 1), (5, 3), (127, 129), (129, 1), (300, 1000), (700, 257)]
TERMS = ["sqexp", "composite"]
LIKS = ["bernoulli", "poisson", "gaussian"]


@pytest.fixture(scope="module")
def ctx():
    if not gpu_available():
        pytest.skip("no GPU")
    c = Context(0)
    yield c
    c.close()


def run(ctx, c, **kw):
    return ctx.laplace_logpdf(c["X"], c["terms"], LO.JITTER, c["lik"], c["y"], lik_param=c["lik_param"], full=True, **kw)


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


@pytest.mark.parametrize("lik_name", LIKS)
@pytest.mark.parametrize("terms_name", TERMS)
@pytest.mark.parametrize("N", SIZES)
def test_logq_and_mode(ctx, N, terms_name, lik_name):
    c = LO.case(N, 1, terms_name, lik_name)
    ref = c["res"]
    res = run(ctx, c)
    eq = rel(res.logq, ref.logq)
    ef = np.max(np.abs(res.f - ref.f)) / max(1.0, np.max(np.abs(ref.f)))
    ea = np.max(np.abs(res.a - ref.a)) / max(1.0, np.max(np.abs(ref.a)))
    print(f"N={N} {terms_name} {lik_name}: iters {res.iters} (oracle {ref.iters}, {ref.halvings} halvings) "
          f"log q error {eq:.3e} f error {ef:.3e} a error {ea:.3e}")
    assert eq <= TOL
    assert ef <= TOL
    assert res.converged and res.iters <= 12
    if lik_name == "gaussian":
        assert res.iters <= 3
        exact = ctx.logpdf(c["X"], c["terms"], LO.JITTER + c["lik_param"], c["y"])
        print(f"    against logpdf at the same noise: {rel(res.logq, exact):.3e}")
        assert rel(res.logq, exact) <= TOL


@pytest.mark.parametrize("terms_name,lik_name", [("composite", "bernoulli"), ("composite", "poisson"),
                                                 ("composite", "gaussian"), ("sqexp", "poisson")])
@pytest.mark.parametrize("N,M", POSTERIOR_SIZES)
def test_posterior(ctx, N, M, terms_name, lik_name):
    c = LO.case(N, M, terms_name, lik_name)
    mean, var, logq, iters, conv = ctx.laplace_posterior_mean_var(
        c["X"], c["terms"], LO.JITTER, c["lik"], c["y"], c["Xs"], lik_param=c["lik_param"], full=True)
    em = np.max(np.abs(mean - c["mean"])) / max(1.0, np.max(np.abs(c["mean"])))
    ev = np.max(np.abs(var - c["var"]) / np.maximum(1.0, np.abs(c["kdiag"])))
    print(f"N={N} M={M} {terms_name} {lik_name}: iters {iters} mean error {em:.3e} variance error {ev:.3e} "
          f"log q error {rel(logq, c['res'].logq):.3e}")
    assert conv
    assert em <= TOL
    assert ev <= TOL
    assert rel(logq, c["res"].logq) <= TOL
    # the entry without test points factors the same B by another schedule (no riding rows): the
    # bar of tests/test_gpu_schedules.py between schedules
    assert abs(logq - run(ctx, c).logq) <= 1e-12 * max(1.0, abs(logq))


# Noise terms (the diagonal the matrix-free products leave out): one as a group of its own, one
# inside a product group (SqExp * Noise: 0.3 delta_ij, since SqExp is 1 on the diagonal)
NOISE_SETS = {
    "sum": [(_native.SQEXP, 0, 1.5, 0), (_native.OU, 0, 3.0, 1), (_native.CAT, 1, 0.0, 2), (_native.NOISE, -1, 0.5, 3)],
    "product": [(_native.OU, 0, 3.0, 0), (_native.SQEXP, 0, 1.5, 1), (_native.NOISE, -1, 0.3, 1),
                (_native.LINEAR, 2, 0.5, 2), (_native.NOISE, -1, 0.2, 2)],
}


@pytest.mark.parametrize("lik_name", ["bernoulli", "poisson"])
@pytest.mark.parametrize("name", sorted(NOISE_SETS))
def test_noise_terms(ctx, name, lik_name):
    N, M = 300, 129
    terms = NOISE_SETS[name]
    X, Xs, y = LO.data(N, M, "composite", lik_name)
    lik = LO.LIKS[lik_name][0]
    ref = LO.laplace(X, terms, LO.JITTER, lik, y)
    rm, rv = LO.posterior_mean_var(ref, X, terms, Xs)
    from oracle import restatement as R

    kd = R.kernel_diag(Xs, terms)
    res = ctx.laplace_logpdf(X, terms, LO.JITTER, lik, y, full=True)
    mean, var = ctx.laplace_posterior_mean_var(X, terms, LO.JITTER, lik, y, Xs)
    ef = np.max(np.abs(res.f - ref.f)) / max(1.0, np.max(np.abs(ref.f)))
    em = np.max(np.abs(mean - rm)) / max(1.0, np.max(np.abs(rm)))
    ev = np.max(np.abs(var - rv) / np.maximum(1.0, np.abs(kd)))
    print(f"{name} {lik_name}: iters {res.iters} (oracle {ref.iters}) log q error {rel(res.logq, ref.logq):.3e} "
          f"f {ef:.3e} mean {em:.3e} variance {ev:.3e}")
    assert res.converged and res.iters <= 12
    assert rel(res.logq, ref.logq) <= TOL and ef <= TOL and em <= TOL and ev <= TOL


@pytest.mark.parametrize("terms_name,lik_name,N", [("composite", "poisson", 700), ("composite", "bernoulli", 300),
                                                   ("sqexp", "poisson", 129)])
def test_warm_start(ctx, terms_name, lik_name, N):
    c = LO.case(N, 1, terms_name, lik_name)
    cold = run(ctx, c)
    warm = run(ctx, c, a0=cold.a)
    print(f"N={N} {terms_name} {lik_name}: cold {cold.iters} steps, warm {warm.iters}; "
          f"log q differs by {abs(warm.logq - cold.logq) / abs(cold.logq):.3e}")
    assert warm.converged and warm.iters <= 2
    assert abs(warm.logq - cold.logq) <= 1e-12 * abs(cold.logq)


@pytest.mark.parametrize("lik_name", LIKS)
def test_identical_calls_are_bitwise_equal(ctx, lik_name):
    c = LO.case(700, 257, "composite", lik_name)
    r1, r2 = run(ctx, c), run(ctx, c)
    assert r1.logq == r2.logq and r1.iters == r2.iters
    assert np.array_equal(r1.f, r2.f) and np.array_equal(r1.a, r2.a)
    p = [ctx.laplace_posterior_mean_var(c["X"], c["terms"], LO.JITTER, c["lik"], c["y"], c["Xs"],
                                        lik_param=c["lik_param"]) for _ in range(2)]
    assert np.array_equal(p[0][0], p[1][0]) and np.array_equal(p[0][1], p[1][1])


def test_other_entries_between_two_laplace_calls(ctx):
    """logpdf and logpdf_grad on other data between two Laplace calls on one context change neither;
    a fit created before a Laplace call answers the same, to the bit, after it."""
    c = LO.case(300, 1000, "composite", "poisson")
    o = LO.case(129, 1, "composite", "gaussian")
    lp0 = ctx.logpdf(o["X"], o["terms"], 0.1, o["y"])
    g0 = ctx.logpdf_grad(o["X"], o["terms"], 0.1, o["y"])
    with ctx.fit(o["X"], o["terms"], 0.1, o["y"], cap=128) as fit:
        m0, v0 = fit.mean_var(c["Xs"])
        r1 = run(ctx, c)
        lp1 = ctx.logpdf(o["X"], o["terms"], 0.1, o["y"])
        g1 = ctx.logpdf_grad(o["X"], o["terms"], 0.1, o["y"])
        r2 = run(ctx, c)
        m1, v1 = fit.mean_var(c["Xs"])
    assert r1.logq == r2.logq and np.array_equal(r1.f, r2.f) and np.array_equal(r1.a, r2.a)
    assert lp0 == lp1
    assert g0[0] == g1[0] and all(np.array_equal(x, y) for x, y in zip(g0[1:3], g1[1:3])) and g0[3] == g1[3]
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)


def test_other_schedule(ctx):
    """The composite Poisson case at N = 700 on a context created under GAPLAC_TAILK=0 and
    GAPLAC_SPW=1: per-column launches in the place of the persistent tail, one-tile super-panels."""
    c = LO.case(700, 257, "composite", "poisson")
    env = {"GAPLAC_TAILK": "0", "GAPLAC_SPW": "1"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        other = Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        res = run(other, c)
        mean, var = other.laplace_posterior_mean_var(c["X"], c["terms"], LO.JITTER, c["lik"], c["y"], c["Xs"])
    finally:
        other.close()
    ref = c["res"]
    em = np.max(np.abs(mean - c["mean"])) / max(1.0, np.max(np.abs(c["mean"])))
    ev = np.max(np.abs(var - c["var"]) / np.maximum(1.0, np.abs(c["kdiag"])))
    print(f"iters {res.iters}; log q error {rel(res.logq, ref.logq):.3e} mean {em:.3e} variance {ev:.3e}")
    assert res.converged and res.iters <= 12
    assert rel(res.logq, ref.logq) <= TOL
    assert np.max(np.abs(res.f - ref.f)) / max(1.0, np.max(np.abs(ref.f))) <= TOL
    assert em <= TOL and ev <= TOL


def test_max_iter_1_is_not_an_error(ctx):
    c = LO.case(300, 1000, "composite", "poisson")
    with pytest.warns(RuntimeWarning, match="did not converge"):
        res = run(ctx, c, max_iter=1)
    assert res.converged is False and res.iters == 1
    assert np.isfinite(res.logq)
    assert np.all(np.isfinite(res.f)) and np.all(np.isfinite(res.a))
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # and the context goes on: a full run raises no warning
        assert run(ctx, c).converged


def test_argument_errors_leave_the_context_usable(ctx):
    c = LO.case(129, 1, "sqexp", "poisson")
    X, y, terms = c["X"], c["y"], c["terms"]
    good = run(ctx, c).logq

    def code(**kw):
        args = dict(X=X, terms=terms, jitter=LO.JITTER, lik=_native.LIK_POISSON, y=y)
        args.update(kw)
        with pytest.raises(ArgumentError) as e:
            ctx.laplace_logpdf(**args)
        return int(str(e.value).split("gaplac error ")[1].split(":")[0])

    half, neg, frac = y.copy(), y.copy(), y.copy()
    half[3], neg[5], frac[7] = 0.5, -1.0, 1.5
    cases = [
        (dict(lik=7), _native.E_KIND),
        (dict(jitter=-1e-6), _native.E_PARAM),
        (dict(jitter=float("nan")), _native.E_PARAM),
        (dict(tol=0.0), _native.E_PARAM),
        (dict(tol=float("inf")), _native.E_PARAM),
        (dict(tol=float("nan")), _native.E_PARAM),
        (dict(max_iter=0), _native.E_PARAM),
        (dict(lik=_native.LIK_GAUSSIAN, lik_param=0.0), _native.E_PARAM),
        (dict(lik=_native.LIK_GAUSSIAN, lik_param=-0.1), _native.E_PARAM),
        (dict(lik=_native.LIK_BERNOULLI, y=half), _native.E_PARAM),
        (dict(lik=_native.LIK_BERNOULLI, y=y + 2.0), _native.E_PARAM),
        (dict(y=neg), _native.E_PARAM),
        (dict(y=frac), _native.E_PARAM),
        (dict(terms=[(_native.SQEXP, 0, -1.0, 0)]), _native.E_PARAM),
        (dict(terms=[(_native.SQEXP, 9, 1.0, 0)]), _native.E_COL),
    ]
    for kw, want in cases:
        assert code(**kw) == want, kw
        assert run(ctx, c).logq == good, kw
    with pytest.raises(ArgumentError):
        ctx.laplace_posterior_mean_var(X, terms, LO.JITTER, "poisson", y, np.zeros((3, X.shape[1] + 1)))
    assert run(ctx, c).logq == good


def test_a_non_finite_w_is_reported_with_b_named(ctx):
    """A start whose f = K a0 overflows exp(f): W is not finite, B cannot be formed; info > 0, the
    text names B, and the context goes on."""
    c = LO.case(129, 1, "sqexp", "poisson")
    good = run(ctx, c).logq
    with pytest.raises(PosDefException) as e:
        run(ctx, c, a0=np.full(129, 1e3))
    assert e.value.info > 0
    msg = ctx.lib.gaplac_last_error(ctx.h).decode()
    assert msg.startswith("B = I + sqrt(W) K sqrt(W)") and "not finite" in msg
    assert run(ctx, c).logq == good


def test_empty_training_set(ctx):
    Xs = LO.inputs(5, 3)[1]
    X0 = np.zeros((0, Xs.shape[1]))
    res = ctx.laplace_logpdf(X0, LO.COMPOSITE, LO.JITTER, "poisson", np.zeros(0), full=True)
    assert res.logq == 0.0 and res.iters == 0 and res.converged
    mean, var = ctx.laplace_posterior_mean_var(X0, LO.COMPOSITE, LO.JITTER, "poisson", np.zeros(0), Xs)
    from oracle import restatement as R

    assert np.array_equal(mean, np.zeros(3))
    assert np.allclose(var, R.kernel_diag(Xs, LO.COMPOSITE), rtol=1e-15, atol=0)


def test_abstractgps_objects(ctx):
    c = LO.case(127, 129, "composite", "bernoulli")
    lgp = AG.LatentGP(_gp_of(c["terms"]), AG.BernoulliLikelihood(), LO.JITTER)
    la = AG.LaplaceApproximation()
    cols = [0, 0, 1, 2]
    lfx = lgp(c["X"][:, cols])
    xs = c["Xs"][:, cols]
    assert rel(AG.approx_lml(la, lfx, c["y"], ctx=ctx), c["res"].logq) <= TOL
    post = AG.posterior(la, lfx, c["y"], ctx=ctx)
    mean, var = post.mean_and_var(xs)
    assert np.max(np.abs(mean - c["mean"])) / max(1.0, np.max(np.abs(c["mean"]))) <= TOL
    assert np.max(np.abs(var - c["var"]) / np.maximum(1.0, np.abs(c["kdiag"]))) <= TOL
    assert np.max(np.abs(post.f_hat - c["res"].f)) / max(1.0, np.max(np.abs(c["res"].f))) <= TOL
    assert np.array_equal(post.mean(xs), post.mean_and_var(xs)[0])  # (now from the warm start)


def _gp_of(terms):
    """The GP of the formula that lowers to the composite set; its design matrix has one column per
    term (a twice): columns [0, 0, 1, 2] of the composite inputs."""
    assert terms == LO.COMPOSITE
    gp, vars_ = AG.make_gp(F.gp_spec("y ~| SqExp(:a; l=1.5) + OU(:a; l=3.0) + Cat(:b) + Linear(:c; c=0.5)"))
    assert vars_ == ["a", "a", "b", "c"]
    return gp


def test_select_formulae_scores_poisson_formulas_by_approx_lml(ctx):
    N = 300
    X, _, y = LO.data(N, 1, "composite", "poisson")
    table = {"y": y, "x": X[:, 0], "g": X[:, 1]}
    f1 = "y : Poisson ~| SqExp(:x; l=1.5) + Cat(:g)"
    f2 = "y : Poisson() ~| OU(:x; l=3.0)"
    bayes, lp1, lp2 = AG.select_formulae(f1, f2, table, ctx=ctx)
    D1 = np.column_stack([X[:, 0], X[:, 1]])
    o1 = LO.laplace(D1, [(1, 0, 1.5, 0), (4, 1, 0.0, 1)], 1e-6, LO.POISSON, y).logq
    o2 = LO.laplace(X[:, :1], [(2, 0, 3.0, 0)], 1e-6, LO.POISSON, y).logq
    print(f"lp1 {lp1!r} oracle {o1!r}; lp2 {lp2!r} oracle {o2!r}")
    assert rel(lp1, o1) <= TOL and rel(lp2, o2) <= TOL
    assert bayes == lp1 - lp2
    assert abs(bayes - (o1 - o2)) <= TOL * max(1.0, abs(o1), abs(o2))
    # a Gaussian formula keeps its own path and result
    g = "y ~| SqExp(:x; l=1.5)"
    assert AG.select_formulae(g, g, table, ctx=ctx)[1] == ctx.logpdf(X[:, :1], [(1, 0, 1.5, 0)], 0.1, y)
    with pytest.raises(F.ArgumentError):
        AG.select_formulae(f1, f2, table, ctx=ctx, responses=["y"])
