"""gaplac_laplace_logpdf_grad (HIP through the C-ABI) against the numpy restatement
tests/laplace_grad_oracle.py (pinned on the CPU by tests/test_laplace_grad_oracle.py).

Bars: log q within 1e-9 |log q| (relative); dparam[t] within 1e-9 (|ref| + scale_t), scale_t = 1/2
sum_ij (|a_i a_j| + 2 |u_i a_j| + |R_ij|) |dK_ij/dtheta_t| the size of what the gradient sums (as
tests/test_gpu_grad.py states its bar); djitter likewise. The implicit part is some 1e-7 to 5e-9 of
that scale at N >= 1000, so the total's bar cannot see an error in it: it is checked on its own,
within 1e-9 (|ref| + sum_ij |u_i| |dK_ij| |a_j|). f, a and iters are bitwise those of
laplace_logpdf on the same inputs.
"""
import ctypes
import warnings
from ctypes import byref, c_double, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from gaplac_amd import _native
from gaplac_amd.backend import ArgumentError, Context, term_array
from oracle import restatement as R
from tests import laplace_grad_oracle as GO
from tests import laplace_oracle as LO
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
TOL = 1e-9
SIZES = [1, 5, 127, 128, 129, 300, 1000]
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
    return ctx.laplace_logpdf_grad(c["X"], c["terms"], c.get("jitter", LO.JITTER), c["lik"], c["y"],
                                   lik_param=c["lik_param"], **kw)


def errors(res, g):
    """The errors in units of their bars: log q, the worst of dparam / djitter, the worst implicit part."""
    eq = abs(res.logq - g.logq) / abs(g.logq)
    T = len(g.dparam)
    ed = [abs(res.dparam[t] - g.dparam[t]) / (abs(g.dparam[t]) + g.scale[t]) for t in range(T) if g.scale[t] > 0]
    for t in range(T):
        if g.scale[t] == 0:  # (a Cat term, or a term whose derivative vanishes on these inputs)
            assert res.dparam[t] == 0.0 and res.implicit[t] == 0.0
    ed.append(abs(res.djitter - g.djitter) / (abs(g.djitter) + g.scale_jitter))
    ei = [abs(res.implicit[t] - g.implicit[t]) / (abs(g.implicit[t]) + g.implicit_scale[t])
          for t in range(T + 1) if g.implicit_scale[t] > 0]
    for t in range(T + 1):
        if g.implicit_scale[t] == 0:
            assert res.implicit[t] == 0.0
    return eq, max(ed), max(ei, default=0.0)


def check(ctx, c, g, label, res=None):
    res = res if res is not None else run(ctx, c)
    eq, ed, ei = errors(res, g)
    print(f"{label}: iters {res.iters} log q error {eq:.3e} gradient {ed:.3e} of its scale, implicit part "
          f"{ei:.3e} of its own")
    assert np.all(np.isfinite(res.dparam)) and np.isfinite(res.djitter) and np.all(np.isfinite(res.implicit))
    assert res.converged
    assert eq <= TOL and ed <= TOL and ei <= TOL
    return res


def same_mode(ctx, c, res):
    val = ctx.laplace_logpdf(c["X"], c["terms"], c.get("jitter", LO.JITTER), c["lik"], c["y"],
                             lik_param=c["lik_param"], full=True)
    assert np.array_equal(res.f, val.f) and np.array_equal(res.a, val.a)
    assert res.iters == val.iters and res.converged == val.converged
    assert abs(res.logq - val.logq) <= 1e-12 * max(1.0, abs(val.logq))  # (another schedule of the same B)


@pytest.mark.parametrize("lik_name", LIKS)
@pytest.mark.parametrize("terms_name", TERMS)
@pytest.mark.parametrize("N", SIZES)
def test_parity(ctx, N, terms_name, lik_name):
    c = GO.case(N, terms_name, lik_name)
    res = check(ctx, c, c["grad"], f"N={N} {terms_name} {lik_name}")
    same_mode(ctx, c, res)


def test_large_schedule(ctx):
    """N = 2049 (17 tile columns): five super-panels, the last one column wide, six C^{-1}
    super-tiles. (The restatement takes 6 steps and no halving on these inputs.)"""
    c = GO.case(2049, "composite", "poisson")
    res = check(ctx, c, c["grad"], "N=2049 composite poisson")
    same_mode(ctx, c, res)


PRODUCT = [(_native.SQEXP, 0, 1.5, 0), (_native.CAT, 1, 0.0, 0), (_native.OU, 0, 3.0, 1)]


@pytest.mark.parametrize("lik_name", ["bernoulli", "poisson"])
def test_product_groups(ctx, lik_name):
    """SqExp * Cat in one group plus OU: the two-launch contraction and the bilinear kernel's
    product rule."""
    X, _, y = LO.data(300, 1, "composite", lik_name)
    lik = LO.LIKS[lik_name][0]
    c = dict(X=X, y=y, terms=PRODUCT, lik=lik, lik_param=0.0)
    g = GO.laplace_grad(X, PRODUCT, LO.JITTER, lik, y)
    assert g.scale[0] > 0 and g.implicit_scale[0] > 0 and g.scale[1] == 0
    res = check(ctx, c, g, f"product groups {lik_name}")
    same_mode(ctx, c, res)


@pytest.mark.parametrize("terms_name", TERMS)
@pytest.mark.parametrize("N", [129, 1000])
def test_gaussian_known_answer(ctx, N, terms_name):
    c = GO.case(N, terms_name, "gaussian")
    res = run(ctx, c)
    lp, _, dp, dn = ctx.logpdf_grad(c["X"], c["terms"], LO.JITTER + c["lik_param"], c["y"])
    g = c["grad"]
    assert np.all(res.implicit == 0.0)
    assert abs(res.logq - lp) <= TOL * abs(lp)
    ed = np.abs(res.dparam - dp) / (np.abs(dp) + g.scale + (g.scale == 0))
    ej = abs(res.djitter - dn) / (abs(dn) + g.scale_jitter)
    print(f"N={N} {terms_name}: against logpdf_grad dparam {np.max(ed):.3e} dnoise {ej:.3e}")
    assert np.all(ed <= TOL) and ej <= TOL


def test_w_to_zero(ctx):
    """Bernoulli under a steep Linear term with separated labels: |f| reaches 38 and the smallest W
    is 0.0 in the restatement (sigma (1 - sigma) rounds to 0 there; the library's e / (1 + e)^2
    gives 2e-17), the largest 1.6e-3; the restatement converges in 15 steps. Nothing is divided
    by W, so everything stays finite and within the bars."""
    rng = np.random.default_rng(5)
    N = 200
    x = rng.uniform(20.0, 120.0, N) * np.where(rng.uniform(size=N) < 0.5, -1.0, 1.0)
    X, y = x[:, None], (x > 0).astype(np.float64)
    terms = [(_native.LINEAR, 0, 0.5, 0)]
    g = GO.laplace_grad(X, terms, LO.JITTER, LO.BERNOULLI, y)
    assert g.res.converged and np.min(g.res.W) <= 1e-12
    c = dict(X=X, y=y, terms=terms, lik=LO.BERNOULLI, lik_param=0.0)
    res = check(ctx, c, g, f"min W {np.min(g.res.W):.3e}")
    assert np.all(np.isfinite(res.f)) and np.all(np.isfinite(res.a))


def test_repeatability_and_state(ctx):
    """Two calls are bitwise equal, also with a logpdf_grad at N = 129 and a logpdf at N = 300 on the
    same context in between (the workspace changes its layout twice); both of those still match
    their restatements."""
    c = GO.case(300, "composite", "poisson")
    o = LO.case(129, 1, "composite", "gaussian")
    p = LO.case(300, 1, "sqexp", "gaussian")

    def same(r1, r2):
        return (r1.logq == r2.logq and r1.djitter == r2.djitter and np.array_equal(r1.dparam, r2.dparam)
                and np.array_equal(r1.implicit, r2.implicit) and np.array_equal(r1.f, r2.f)
                and np.array_equal(r1.a, r2.a) and r1.iters == r2.iters)

    r1, r2 = run(ctx, c), run(ctx, c)
    assert same(r1, r2)
    lp, dv, dp, dn = ctx.logpdf_grad(o["X"], o["terms"], 0.1, o["y"])
    lq = ctx.logpdf(p["X"], p["terms"], 0.1, p["y"])
    r3 = run(ctx, c)
    assert same(r1, r3)
    rlp, rdv, rdp, rdn = R.logpdf_grad(o["X"], o["terms"], 0.1, o["y"])
    sc, scn = R.logpdf_grad_scale(o["X"], o["terms"], 0.1, o["y"])
    assert abs(lp - rlp) <= TOL * max(1.0, abs(rlp))
    assert np.all(np.abs(dp - rdp) <= TOL * (np.abs(rdp) + sc)) and abs(dn - rdn) <= TOL * (abs(rdn) + scn)
    assert np.max(np.abs(dv - rdv)) <= TOL * max(1.0, np.max(np.abs(rdv)))
    rlq = R.logpdf(p["X"], p["terms"], 0.1, p["y"])[0]
    assert abs(lq - rlq) <= TOL * max(1.0, abs(rlq))


@pytest.mark.parametrize("terms_name,lik_name,N", [("composite", "poisson", 1000), ("sqexp", "bernoulli", 129)])
def test_warm_start(ctx, terms_name, lik_name, N):
    c = GO.case(N, terms_name, lik_name)
    cold = run(ctx, c)
    warm = run(ctx, c, a0=cold.a)
    assert warm.iters <= 1
    check(ctx, c, c["grad"], f"warm N={N} {terms_name} {lik_name}", res=warm)


def test_central_differences_of_the_librarys_own_log_q(ctx):
    """N = 1000, composite, Poisson: central differences of laplace_logpdf in each lengthscale (h =
    1e-5 l) and in the jitter (at 1e-3, h = 1e-6), within 1e-6 of the scale plus the rounding of the
    difference (10 ulp of log q over h), tests/test_grad_oracle.py's bar."""
    X, _, y = LO.data(1000, 1, "composite", "poisson")
    terms = LO.COMPOSITE
    J = 1e-3
    g = GO.laplace_grad(X, terms, J, LO.POISSON, y)
    res = ctx.laplace_logpdf_grad(X, terms, J, "poisson", y)

    def logq(tt, j):
        return ctx.laplace_logpdf(X, tt, j, "poisson", y)

    for t in (0, 1):
        h = 1e-5 * terms[t][2]
        tp, tm = [list(x) for x in terms], [list(x) for x in terms]
        tp[t][2] += h
        tm[t][2] -= h
        fd = (logq([tuple(x) for x in tp], J) - logq([tuple(x) for x in tm], J)) / (2 * h)
        err = abs(res.dparam[t] - fd)
        floor = 10 * 2.2e-16 * max(1.0, abs(res.logq)) / h
        print(f"term {t}: gradient {res.dparam[t]!r} difference {fd!r}: {err / (abs(fd) + g.scale[t]):.3e} of the scale")
        assert err <= 1e-6 * (abs(fd) + g.scale[t]) + floor
    h = 1e-6
    fd = (logq(terms, J + h) - logq(terms, J - h)) / (2 * h)
    err = abs(res.djitter - fd)
    print(f"jitter: gradient {res.djitter!r} difference {fd!r}: {err / (abs(fd) + g.scale_jitter):.3e} of the scale")
    assert err <= 1e-6 * (abs(fd) + g.scale_jitter) + 10 * 2.2e-16 * max(1.0, abs(res.logq)) / h


def _raw(ctx, X, terms, lik, y, max_iter=100, tol=1e-12, null=False):
    """The entry through ctypes with pre-filled outputs: (rc, logq, f, a, dparam, djitter, implicit)."""
    Xc = np.asfortranarray(X, dtype=np.float64)
    N, D = Xc.shape
    T = len(terms)
    ta = term_array(terms)
    y = np.ascontiguousarray(y, dtype=np.float64)
    logq, dj = c_double(7.0), c_double(7.0)
    f, a, dp, imp = (np.full(n, 7.0) for n in (max(N, 1), max(N, 1), max(T, 1), T + 1))
    iters, conv, info = c_int32(), c_int32(), c_int64()
    p = (lambda arr: None) if null else (lambda arr: arr.ctypes.data_as(c_void_p))
    rc = ctx.lib.gaplac_laplace_logpdf_grad(
        ctx.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), T, ta, LO.JITTER, lik, 0.0, y.ctypes.data_as(c_void_p),
        max_iter, tol, None, None if null else byref(logq), p(f), p(a), None if null else byref(iters),
        None if null else byref(conv), None if null else byref(info), p(dp), None if null else byref(dj), p(imp))
    return rc, logq.value, f[:N], a[:N], dp[:T], dj.value, imp


def test_errors_and_edges(ctx):
    c = GO.case(129, "sqexp", "poisson")
    X, y, terms = c["X"], c["y"], c["terms"]
    good = run(ctx, c)
    # error paths NaN-fill every output and leave the context usable
    for kw in (dict(lik=7), dict(tol=0.0), dict(max_iter=0), dict(y=y + 0.5)):
        args = dict(lik=_native.LIK_POISSON, y=y)
        args.update(kw)
        rc, logq, f, a, dp, dj, imp = _raw(ctx, X, terms, args["lik"], args["y"], args.get("max_iter", 100),
                                           args.get("tol", 1e-12))
        assert rc < 0
        assert np.isnan(logq) and np.isnan(dj) and np.all(np.isnan(dp)) and np.all(np.isnan(imp))
        assert np.all(np.isnan(f)) and np.all(np.isnan(a))
        again = run(ctx, c)
        assert again.logq == good.logq and np.array_equal(again.dparam, good.dparam)
    with pytest.raises(ArgumentError):
        ctx.laplace_logpdf_grad(X, [(_native.SQEXP, 0, -1.0, 0)], LO.JITTER, "poisson", y)
    # NULL outputs are accepted
    assert _raw(ctx, X, terms, _native.LIK_POISSON, y, null=True)[0] == 0
    # max_iter = 1: not converged, not an error, finite outputs, the same warning as laplace_logpdf
    with pytest.warns(RuntimeWarning, match="did not converge"):
        r1 = run(ctx, c, max_iter=1)
    assert r1.converged is False and r1.iters == 1
    assert np.isfinite(r1.logq) and np.all(np.isfinite(r1.dparam)) and np.isfinite(r1.djitter)
    assert np.all(np.isfinite(r1.implicit))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert run(ctx, c).converged
    # N = 0
    X0 = np.zeros((0, X.shape[1]))
    r0 = ctx.laplace_logpdf_grad(X0, LO.COMPOSITE, LO.JITTER, "poisson", np.zeros(0))
    assert r0.logq == 0.0 and r0.iters == 0 and r0.converged
    assert np.array_equal(r0.dparam, np.zeros(4)) and r0.djitter == 0.0 and np.array_equal(r0.implicit, np.zeros(5))


def test_abstractgps_and_the_fit_on_the_device(ctx):
    """approx_lml_grad on the objects of tests/test_gpu_laplace.py, and a short lengthscale fit on the
    device: the history climbs and the fitted point's log q is the library's own at those terms."""
    from gaplac_amd import abstractgps as AG
    from gaplac_amd import formula as F
    from gaplac_amd import laplace_fit as LF

    c = GO.case(127, "composite", "bernoulli")
    gp, _ = AG.make_gp(F.gp_spec("y ~| SqExp(:a; l=1.5) + OU(:a; l=3.0) + Cat(:b) + Linear(:c; c=0.5)"))
    lfx = AG.LatentGP(gp, AG.BernoulliLikelihood(), LO.JITTER)(c["X"][:, [0, 0, 1, 2]])
    lml, dparam, djitter = AG.approx_lml_grad(AG.LaplaceApproximation(), lfx, c["y"], ctx=ctx)
    g = c["grad"]
    assert abs(lml - g.logq) <= TOL * abs(g.logq)
    assert np.all(np.abs(dparam - g.dparam) <= TOL * (np.abs(g.dparam) + g.scale))
    assert abs(djitter - g.djitter) <= TOL * (abs(g.djitter) + g.scale_jitter)
    p = GO.case(300, "composite", "poisson")
    start = [(k, col, 2.0 * v if k in LF.LENGTHSCALE_KINDS else v, grp) for k, col, v, grp in p["terms"]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (a warm start that fails is repeated from a = 0)
        fitted, logq, hist = LF.fit_hyperparameters(ctx, p["X"], start, LO.JITTER, p["lik"], p["y"], maxiter=4)
    print(f"fit: log q {hist[0]:.6f} -> {logq:.6f} in {len(hist) - 1} accepted steps, "
          f"l = {[round(t[2], 4) for t in fitted[:2]]}")
    assert len(hist) >= 2 and all(b >= a for a, b in zip(hist, hist[1:])) and logq > hist[0]
    assert [t[:2] + t[3:] for t in fitted] == [t[:2] + t[3:] for t in start] and fitted[2:] == start[2:]
    again = ctx.laplace_logpdf(p["X"], fitted, LO.JITTER, p["lik"], p["y"])
    assert abs(again - logq) <= 1e-9 * max(1.0, abs(logq))
