"""tests/laplace_hard.py pinned on the CPU, so that tests/test_gpu_laplace_hard.py can neither pass
vacuously nor fail for the oracle's sake: the reference converges and is stable under further
long-double steps, every yardstick path ends finite, the designs exercise what they are for (a
non-finite psi in a trial point, halvings on rounding noise near the mode), which cases test the
flat 1e-9 and which the bar relative to plain fp64 LAPACK is fixed, degraded iterations fail the
GPU test's bars, and the prediction oracle is the Gauss-Hermite rule it states to 1e-11 where the
probabilities are within 1e-20 of 0 and 1 and the rates 1e4.
"""
import mpmath
import numpy as np
import pytest
from numpy.polynomial.hermite import hermgauss

from tests import laplace_hard as H
from tests import laplace_oracle as LO
from tests import laplace_predict_oracle as PO

IDS = [H.case_id(k) for k in H.CASES]


def test_table():
    """The whole table: per case max W, cond(B), steps:halvings of the reference and of each path,
    and the yardstick of every output."""
    for key in H.CASES:
        c = H.case(key)
        print(H.row(c))
        print("    " + " ".join(f"{k} {v:.1e}" for k, v in c["yard"].items()))
        print("    a per path " + " ".join(f"{e['a']:.1e}" for e in c["errs"]) + "; residual per path "
              + " ".join(f"{r:.1e}" for r in c["path_res"]))


@pytest.mark.parametrize("key", H.CASES, ids=IDS)
def test_reference_and_paths(key):
    c = H.case(key)
    res = c["res"]
    assert res.converged and res.iters <= 14
    # two more long-double steps move nothing beyond 1e-11
    more = H.refine(res, c["lik"], c["y"], 2, ax=res.ax)
    moved = H.errors(dict(logq=more.logq, a=more.a, f=more.f), c)
    print(f"{H.case_id(key)}: two more steps move " + " ".join(f"{k} {v:.1e}" for k, v in moved.items())
          + f"; the reference's residual {c['ref_res']:.1e}")
    assert all(v <= 1e-11 for v in moved.values())
    # (an a rounded to fp64 leaves a residual of some |W K| ulp(a), 1e-10 at W = 1e4 and under the
    # vague intercept: the reference is three digits inside the yardstick wherever that is beyond
    # the flat bar's range)
    assert c["ref_res"] <= max(1e-10, 1e-3 * c["yard_res"])
    for path, run, out in zip(H.PATHS, c["runs"], c["outs"]):
        assert run.converged and 1 <= run.iters <= 20, path
        assert sum(h for h, _ in run.trace) == run.halvings and len(run.trace) == run.iters, path
        for k, v in out.items():
            assert np.all(np.isfinite(v)), (path, k)


@pytest.mark.parametrize("N", [129, 700])
def test_outlier_meets_a_non_finite_psi(N):
    c = H.case(("outlier", N, None))
    for path in H.PATHS[:2]:
        run = c["runs"][H.PATHS.index(path)]
        print(f"outlier-{N} {path}: (halvings, non-finite psi) per step {run.trace}")
        assert run.trace[0][1] >= 1 and run.halvings >= 10
    assert np.max(c["res"].W) > 4e3


@pytest.mark.parametrize("key", [k for k in H.CASES if k[0] == "counts" and k[2] >= 5], ids=H.case_id)
def test_counts_take_halvings_near_the_mode(key):
    """Halvings after the third step. Whether a yardstick path takes one at level 5 depends on the
    BLAS build's summation order (psi's rounding noise against the slack tol (1 + |psi|)); at tol =
    1e-14 the slack is below the noise at every level, so that run is counted with them."""
    c = H.case(key)
    late = [sum(h for h, _ in run.trace[3:]) for run in c["runs"]]
    tight = H.iterate(c, "cold 1e-14")
    late14 = sum(h for h, _ in tight.trace[3:])
    print(f"{H.case_id(key)}: halvings after the third step, per path: {late}; at tol = 1e-14: {late14} "
          f"({tight.iters} steps, converged {tight.converged})")
    assert max(late + [late14]) >= 1
    if key[2] >= 7:
        assert max(late) >= 1


def test_which_cases_test_which_bar():
    """The yardstick of a is beyond 1e-9 for counts at level >= 5 and vague(700, 1e6), below it for
    zeros, separable and outlier(129). vague(700, 1e4) sits on the edge: a full Newton step leaves a
    within cond(B) u |b|, some 5e-11, and a path whose last step is halved on psi's rounding noise
    ends 1e-8 to 6e-7 away; which of the two the four paths show depends on the labels (10 of 14
    seeds tried gave more than 1e-9) and on the BLAS build's summation order, so only the floor is
    asserted for it and the bar of the GPU test follows whatever the yardstick is."""
    for key in H.CASES:
        y = H.case(key)["yard"]
        name, N, arg = key
        if (name == "counts" and arg >= 5) or key == ("vague", 700, 1e6):
            assert y["a"] > 1e-9, key
        if key == ("vague", 700, 1e4):
            print(f"vague-700-1e4: yardstick of a {y['a']:.3e}")
            assert y["a"] > 1e-11, key
        if name in ("zeros", "separable") or key == ("outlier", 129, None):
            assert y["a"] < 1e-9, key
        if name in ("zeros", "separable"):
            assert max(y.values()) < 1e-10 and H.case(key)["yard_res"] < 1e-10, key
        assert y["var"] < 1e-10 and y["cov"] < 1e-10, key
    for N in (129, 700):
        assert np.min(H.case(("separable", N, None))["res"].W) == 0.0
        assert np.max(np.abs(H.case(("separable", N, None))["res"].f)) > 50.0
        assert np.max(H.case(("zeros", N, None))["res"].W) < 2e-3


def _sw32(K, lik, param, y, f):
    """LO.newton_step with sw rounded to float32."""
    import scipy.linalg

    _, g, W = LO.lik_terms(lik, param, y, f)
    sw = np.sqrt(W).astype(np.float32).astype(np.float64)
    L = np.linalg.cholesky(np.eye(K.shape[0]) + sw[:, None] * K * sw[None, :])
    b = W * f + g
    u = scipy.linalg.solve_triangular(L, sw * (K @ b), lower=True, check_finite=False)
    u = scipy.linalg.solve_triangular(L, u, lower=True, trans="T", check_finite=False)
    an = b - sw * u
    return an, K @ an


def _stale():
    """LO.newton_step with B (and the sw around its inverse) from the previous iterate's W."""
    import scipy.linalg

    prev = []

    def step(K, lik, param, y, f):
        _, g, W = LO.lik_terms(lik, param, y, f)
        sw = np.sqrt(prev[-1] if prev else W)
        prev.append(W)
        L = np.linalg.cholesky(np.eye(K.shape[0]) + sw[:, None] * K * sw[None, :])
        b = W * f + g
        u = scipy.linalg.solve_triangular(L, sw * (K @ b), lower=True, check_finite=False)
        u = scipy.linalg.solve_triangular(L, u, lower=True, trans="T", check_finite=False)
        an = b - sw * u
        return an, K @ an

    return step


def _row(K, lik, param, y, f):
    """LO.newton_step with row 128's sw taken from row 127 (an index off by one at a tile's edge)."""
    import scipy.linalg

    _, g, W = LO.lik_terms(lik, param, y, f)
    sw = np.sqrt(W)
    sw[128] = sw[127]
    L = np.linalg.cholesky(np.eye(K.shape[0]) + sw[:, None] * K * sw[None, :])
    b = W * f + g
    u = scipy.linalg.solve_triangular(L, sw * (K @ b), lower=True, check_finite=False)
    u = scipy.linalg.solve_triangular(L, u, lower=True, trans="T", check_finite=False)
    an = b - sw * u
    return an, K @ an


def _degraded(c, step):
    run = H.iterate(c, "cold 1e-12", step=step)
    out, _ = H.outputs(run, c["X"], c["Xs"], c["terms"], c["lik"])
    errs, resid = H.errors(out, c), H.residual(c, run.a)
    print(f"{run.iters} steps, {run.halvings} halvings, converged {run.converged}; a {errs['a']:.3e} "
          f"(yardstick {c['yard']['a']:.3e}) f {errs['f']:.3e} ({c['yard']['f']:.3e}) residual {resid:.3e} "
          f"({c['yard_res']:.3e})")
    return H.violations(c, errs), H.violations(c, {}, resid)


@pytest.mark.parametrize("name,key", [("stale", ("counts", 700, 7)), ("row", ("counts", 700, 7)),
                                      ("sw32", ("outlier", 129, None)), ("sw32", ("counts", 129, 3))])
def test_a_degraded_iteration_fails_the_bars(name, key):
    """The GPU test's assertions 2 (error bars) and 3 (residual), through the same H.violations,
    given a numpy iteration that is subtly wrong: on counts(700, 7) B from the previous iterate's W,
    or one row of B scaled by its neighbour's sw. sw rounded to float32 moves f by 1e-7 |f|, which
    the bar of counts(700, 7) (ten times LAPACK's 1.4e-8) admits: the flat bar catches it, on
    outlier(129) and counts(129, 3)."""
    c = H.case(key)
    bad_e, bad_r = _degraded(c, {"stale": _stale(), "row": _row, "sw32": _sw32}[name])
    print("\n".join(bad_e + bad_r))
    assert any(b.startswith("a:") for b in bad_e) and any(b.startswith("f:") for b in bad_e)
    assert bad_r
    # and the honest paths pass the same check
    for e, r in zip(c["errs"], c["path_res"]):
        assert H.violations(c, e, r) == []


def test_what_the_relative_bar_admits():
    """sw rounded to float32 on counts(700, 7): printed, not asserted either way. The bar there is
    LAPACK's own error, and this degradation is no worse than LAPACK."""
    c = H.case(("counts", 700, 7))
    bad_e, bad_r = _degraded(c, _sw32)
    print("beyond the bars: " + ("; ".join(bad_e + bad_r) or "nothing"))


MP = mpmath.mp.clone()  # (a context of its own, as tests/hp_oracle.py's: the global one stays as it is)
MP.dps = 40


def _rule(Q=32):
    """The Gauss-Hermite rule of order Q in 40 digits: numpy's nodes polished by Newton on H_Q,
    w = 2^(Q-1) Q! sqrt(pi) / (Q^2 H_(Q-1)(x)^2)."""
    xs, ws = [], []
    for x0 in hermgauss(Q)[0]:
        x = MP.mpf(float(x0))
        for _ in range(6):
            x -= MP.hermite(Q, x) / (2 * Q * MP.hermite(Q - 1, x))
        xs.append(x)
        ws.append(MP.mpf(2) ** (Q - 1) * MP.factorial(Q) * MP.sqrt(MP.pi) / (Q ** 2 * MP.hermite(Q - 1, x) ** 2))
    return xs, ws


def _mp_predict(lik, m, v, y, rule):
    """(ymean, yvar, logp) of one point by the rule in 40 digits."""
    m, v, y = MP.mpf(float(m)), MP.mpf(max(float(v), 0.0)), MP.mpf(float(y))
    fs = [m + MP.sqrt(2 * v) * x for x in rule[0]]
    spi = MP.sqrt(MP.pi)

    def lp(f):
        return y * f - MP.exp(f) - MP.loggamma(y + 1) if lik == LO.POISSON else y * f - MP.log1p(MP.exp(f))

    if lik == LO.POISSON:
        ymean = MP.exp(m + v / 2)
        yvar = ymean + MP.expm1(v) * ymean ** 2
    else:
        ymean = MP.fsum(w / (1 + MP.exp(-f)) for w, f in zip(rule[1], fs)) / spi
        yvar = ymean * (1 - ymean)
    logp = MP.log(MP.fsum(w * MP.exp(lp(f)) for w, f in zip(rule[1], fs)) / spi) if v > 0 else lp(m)
    return ymean, yvar, logp


@pytest.mark.parametrize("shrink", [1.0, H.SHRINK])
@pytest.mark.parametrize("key", [("separable", 129, None), ("separable", 700, None), ("counts", 129, 9),
                                 ("counts", 700, 9)], ids=H.case_id)
def test_the_prediction_oracle_on_the_hard_fits(key, shrink):
    """tests/laplace_predict_oracle.predict at the reference's latent mean and variance against the
    same rule in 40 digits, every fourth test point: within 1e-11 max(1, |ref|), two digits inside
    the library's bar (the Poisson log score sums ys f, e^f and lgamma(ys + 1), 1e5 each at these
    rates: 3 ulp of that is 4e-11 absolute, 4e-12 of a log score of -10), and the probabilities
    within 1e-13 of themselves. Under the separable labels the probabilities at the test points only
    come within 1e-9 of 0 and 1 (N = 700; the slope's posterior is that wide), so the same means are
    also predicted from the variance divided by H.SHRINK: within 1e-20 of 0 and 1."""
    c = H.case(key)
    mean, var = c["out"]["mean"], c["out"]["var"] / shrink
    ys = H.predict_ys(c)
    ym, yv, lp = PO.predict(c["lik"], mean, var, ys)
    assert np.all(np.isfinite(ym)) and np.all(np.isfinite(yv)) and np.all(np.isfinite(lp))
    rule = _rule()
    worst = dict(ymean=0.0, yvar=0.0, logp=0.0, p=0.0)
    for j in range(0, len(mean), 4):
        rm, rv, rl = _mp_predict(c["lik"], mean[j], var[j], ys[j], rule)
        for k, o, r in (("ymean", ym[j], rm), ("yvar", yv[j], rv), ("logp", lp[j], rl)):
            worst[k] = max(worst[k], float(abs(o - r) / max(1, abs(r))))
        if c["lik"] == LO.BERNOULLI:
            worst["p"] = max(worst["p"], float(abs(ym[j] - rm) / rm))
    print(f"{H.case_id(key)} var / {shrink:g}: oracle against the rule in 40 digits: {worst}; "
          f"ymean spans {np.min(ym):.3e} to {np.max(ym):.3e}, 1 - ymean down to {np.min(1 - ym):.3e}, "
          f"log score down to {np.min(lp):.3f}")
    assert max(worst["ymean"], worst["yvar"], worst["logp"]) <= 1e-11 and worst["p"] <= 1e-13
    if c["lik"] == LO.BERNOULLI:
        assert np.all((ym >= 0.0) & (ym <= 1.0)) and np.all(yv >= 0.0)
    if c["lik"] == LO.BERNOULLI and shrink > 1:
        assert np.min(ym) < 1e-20 and np.min(1.0 - ym) < 1e-20
    if c["lik"] == LO.POISSON:
        assert np.max(ym) > 5e3
