"""Hard inputs for the Laplace paths: large counts, a vague intercept, outliers
whose first Newton point overflows exp, all-zero counts and separable labels, each with a reference,
a yardstick and an oracle-free residual. Infrastructure only; tests/test_laplace_hard_oracle.py pins
it on the CPU, tests/test_gpu_laplace_hard.py holds the library to it.

The reference is tests/laplace_oracle.laplace with its long-double polish, then EXTENDED more steps
of the same residual form with a itself carried in long double (refine): under the vague intercept
K's entries are 1e6, so f = K fl(a) is only determined to 1e-9 by an a rounded to fp64, and K a
cancels six digits even in long double. There the constant part of K is taken out exactly and the sum
of a formed exactly (matvec), and the reference's f is that of the unrounded a. From the result come
the posterior (posterior_mean_var), the gradient (laplace_grad_oracle.grad_from), the joint
covariance at the test points and the observation-space prediction (laplace_predict_oracle.predict).

The yardstick is the same iteration in plain fp64 LAPACK without polish along four paths: a cold
start at tol = 1e-12 (the library's default), a cold start at tol = 1e-13, and warm starts from the
reference's a rounded to float32 and from half of it. Near the mode the halving
decisions are taken on rounding noise, so one path's error is itself noisy (under the vague
intercept by three orders of magnitude from one set of labels to the next); per output the yardstick
is the largest error of the four.

Error measures, those of tests/test_gpu_laplace.py, test_gpu_laplace_grad.py and
test_gpu_laplace_fit.py: log q |d| / max(1, |ref|); a, f, mean max |d| / max(1, max |ref|); var and
the covariance entries |d| / max(1, kdiag) (the covariance: max(1, max kdiag)); dparam[t], djitter
|d| / (|ref| + scale); implicit[t] |d| / (|ref| + implicit_scale); ymean, yvar |d| / max(1, |ref|).

The residual max |g(K a) - a| / max(1, max |a|), with K a and g in long double, needs no oracle: at
the mode a = g(K a).
"""
import math

import numpy as np
import scipy.linalg

from oracle import restatement as R
from tests import laplace_grad_oracle as GO
from tests import laplace_oracle as LO
from tests import laplace_predict_oracle as PO

M = 129
COUNTS_TERMS = [(R.SQEXP, 0, 1.5, 0), (R.LINEAR, 2, 40.0, 1)]
LEVELS = [3, 5, 7, 9]
VAGUE_C = [1e4, 1e6]
NAMES = ["counts", "outlier", "separable", "vague", "zeros"]
# steps with a in long double that the reference takes after laplace()'s polish:
# tests/test_laplace_hard_oracle.py shows that two more move nothing beyond 1e-11
EXTENDED = 2
# the prediction is also checked from the latent variance divided by this (separable labels: the
# probabilities then lie within 1e-20 of 0 and 1)
SHRINK = 100.0


def _seed(name, N, extra=0):
    # What the yardstick's paths do near the mode is chance: of 14 constants tried, 4 gave
    # counts(., 5) a halving after the third step at both sizes and 10 gave vague(700, 1e4) an error
    # of a beyond 1e-9 (the others 3e-11 to 1e-10). This is the first that gave both, with one BLAS
    # build; another build's summation order draws again, so tests/test_laplace_hard_oracle.py pins
    # neither of the two.
    return 7000021 + 7919 * N + 101 * NAMES.index(name) + int(extra)


def counts(N, level):
    """Poisson counts of rate exp(level + 0.5 z), z a draw from the SqExp term: W = exp(f) to 1e4."""
    X, Xs = LO.inputs(N, M)
    rng = np.random.default_rng(_seed("counts", N, level))
    K = R.gram(X, COUNTS_TERMS[:1], LO.JITTER)
    z = np.linalg.cholesky(K + 1e-8 * np.eye(N)) @ rng.normal(size=N)
    y = rng.poisson(np.exp(level + 0.5 * z)).astype(np.float64)
    return X, Xs, COUNTS_TERMS, LO.POISSON, y


def vague(N, c):
    """Random labels under an intercept of prior variance c: every W = 1/4, B = I + K / 4."""
    X, Xs = LO.inputs(N, M)
    rng = np.random.default_rng(_seed("vague", N, np.log10(c)))
    y = (rng.uniform(size=N) < 0.5).astype(np.float64)
    return X, Xs, [(R.SQEXP, 0, 1.5, 0), (R.LINEAR, 2, float(c), 1)], LO.BERNOULLI, y


def outlier(N):
    """Counts of rate 1 with every 37th 5000: the first Newton point overflows exp (psi = -inf)."""
    X, Xs = LO.inputs(N, M)
    rng = np.random.default_rng(_seed("outlier", N))
    y = rng.poisson(1.0, size=N).astype(np.float64)
    y[::37] = 5000.0
    return X, Xs, LO.COMPOSITE, LO.POISSON, y


def zeros(N):
    """All counts zero: f near -7, W near 1e-3."""
    X, Xs = LO.inputs(N, M)
    return X, Xs, COUNTS_TERMS, LO.POISSON, np.zeros(N)


def separable(N):
    """Labels y = (x > 0) under a Linear term on a column scaled by 10: |f| to 90, W down to 0.0."""
    X, Xs = LO.inputs(N, M)
    X, Xs = X.copy(), Xs.copy()
    X[:, 2] *= 10.0
    Xs[:, 2] *= 10.0
    return X, Xs, [(R.LINEAR, 2, 0.5, 0)], LO.BERNOULLI, (X[:, 2] > 0).astype(np.float64)


DESIGNS = {"counts": counts, "vague": vague, "outlier": outlier, "zeros": zeros, "separable": separable}
CASES = ([("counts", N, lv) for N in (129, 700) for lv in LEVELS] + [("counts", 2049, 7)]
         + [("vague", N, c) for N in (129, 700) for c in VAGUE_C]
         + [(name, N, None) for name in ("outlier", "zeros", "separable") for N in (129, 700)])
PATHS = ["cold 1e-12", "cold 1e-13", "warm float32", "warm half"]


def case_id(key):
    name, N, arg = key
    return f"{name}-{N}" + ("" if arg is None else f"-{arg:g}")


def design(key):
    name, N, arg = key
    return DESIGNS[name](N) if arg is None else DESIGNS[name](N, arg)


def outputs(res, X, Xs, terms, lik):
    """Every output the library's entries return, from a laplace() result."""
    mean, var = LO.posterior_mean_var(res, X, terms, Xs)
    g = GO.grad_from(res, X, terms, lik)
    Ks = R.cross_gram(Xs, X, terms)
    V = scipy.linalg.solve_triangular(res.L, res.sw[:, None] * Ks.T, lower=True, check_finite=False)
    ymean, yvar, _ = PO.predict(lik, mean, var)
    return dict(logq=res.logq, a=res.a, f=res.f, mean=mean, var=var, dparam=g.dparam, djitter=g.djitter,
                implicit=g.implicit, cov=R.gram(Xs, terms, 0.0) - V.T @ V, ymean=ymean, yvar=yvar), g


def errors(out, c):
    """name -> error of the outputs `out` (a dict as outputs() returns, any subset of its keys)
    against the reference of case c, in the measures of the module's docstring."""
    ref, g, kd = c["out"], c["grad"], c["kdiag"]
    e = {}

    def vec(k):
        return float(np.max(np.abs(out[k] - ref[k])) / max(1.0, np.max(np.abs(ref[k]))))

    def scaled(x, r, s):
        if s == 0:  # (a Cat term: the derivative vanishes, and the result is 0.0 exactly)
            return 0.0 if x == 0.0 else np.inf
        return float(abs(x - r) / (abs(r) + s))

    if "logq" in out:
        e["logq"] = abs(out["logq"] - ref["logq"]) / max(1.0, abs(ref["logq"]))
    for k in ("a", "f", "mean"):
        if k in out:
            e[k] = vec(k)
    if "var" in out:
        e["var"] = float(np.max(np.abs(out["var"] - ref["var"]) / np.maximum(1.0, np.abs(kd))))
    if "dparam" in out:
        for t in range(len(g.dparam)):
            e[f"dparam[{t}]"] = scaled(out["dparam"][t], g.dparam[t], g.scale[t])
        e["djitter"] = scaled(out["djitter"], g.djitter, g.scale_jitter)
        for t in range(len(g.implicit)):
            e[f"implicit[{t}]"] = scaled(out["implicit"][t], g.implicit[t], g.implicit_scale[t])
    if "cov" in out:
        e["cov"] = float(np.max(np.abs(out["cov"] - ref["cov"])) / max(1.0, np.max(kd)))
    for k in ("ymean", "yvar"):
        if k in out:
            e[k] = float(np.max(np.abs(out[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))))
    return e


def split(K):
    """(K - s in long double, s): s = min K where K's entries lie in [s, 2 s] with s >= 1000 (the
    vague intercept; K - s is then exact in fp64, by Sterbenz), else 0."""
    s = float(np.min(K))
    if s < 1e3 or np.max(K) > 2.0 * s:
        return K.astype(np.longdouble), 0.0
    return (K - s).astype(np.longdouble), s


def matvec(Kx, shift, ax):
    """K a in long double for a long-double a; the constant part's s sum(a) from the exact sums of
    a's leading and trailing fp64 parts."""
    f = Kx @ ax
    if shift:
        hi = ax.astype(np.float64)
        lo = (ax - hi).astype(np.float64)
        f = f + np.longdouble(shift) * (np.longdouble(math.fsum(hi)) + np.longdouble(math.fsum(lo)))
    return f


def refine(res, lik, y, steps, ax=None):
    """`steps` Newton steps in the residual form of LO.polish_step from res.a (or the long-double
    ax), a carried in long double; returns a new Result with a and f rounded once from it, W, L and
    log q at that f, and the unrounded a as .ax."""
    K, N = res.K, res.K.shape[0]
    Kx, shift = split(K)
    yx = y.astype(np.longdouble)
    ax = res.a.astype(np.longdouble) if ax is None else ax
    for _ in range(steps):
        f = matvec(Kx, shift, ax)
        r = (LO.grad_extended(lik, 0.0, yx, f) - ax).astype(np.float64)
        sw = np.sqrt(LO.lik_terms(lik, 0.0, y, f.astype(np.float64))[2])
        L = np.linalg.cholesky(np.eye(N) + sw[:, None] * K * sw[None, :])
        u = scipy.linalg.solve_triangular(L, sw * (K @ r), lower=True, check_finite=False)
        u = scipy.linalg.solve_triangular(L, u, lower=True, trans="T", check_finite=False)
        ax = ax + (r - sw * u)
    out = LO.Result()
    out.iters, out.converged, out.halvings, out.K, out.ax = res.iters, res.converged, res.halvings, K, ax
    out.a, out.f = ax.astype(np.float64), matvec(Kx, shift, ax).astype(np.float64)
    lp, out.g, out.W = LO.lik_terms(lik, 0.0, y, out.f)
    out.sw = np.sqrt(out.W)
    out.L = np.linalg.cholesky(np.eye(N) + out.sw[:, None] * K * out.sw[None, :])
    out.logq = -0.5 * float(out.a @ out.f) + float(np.sum(lp)) - float(np.sum(np.log(np.diag(out.L))))
    return out


def residual(c, a):
    """max |g(K a) - a| / max(1, max |a|), K a and g in long double."""
    ax = np.asarray(a, dtype=np.float64).astype(np.longdouble)
    f = matvec(c["Kx"], c["shift"], ax)
    r = LO.grad_extended(c["lik"], 0.0, c["y"].astype(np.longdouble), f) - ax
    return float(np.max(np.abs(r)) / max(1.0, np.max(np.abs(a))))


def start(c, path):
    """(tol, a0) of a yardstick path."""
    a = c["res"].a
    return {"cold 1e-12": (1e-12, None), "cold 1e-13": (1e-13, None), "cold 1e-14": (1e-14, None),
            "warm float32": (1e-12, a.astype(np.float32).astype(np.float64)),
            "warm half": (1e-12, 0.5 * a)}[path]


def iterate(c, path, step=None):
    """One yardstick path on case c: laplace(polish=0), with .trace, one (halvings, trial points
    whose psi was not finite) per Newton step taken or tried, counted by wrapping LO.psi and
    LO.newton_step. `step` replaces LO.newton_step for the call's duration (the degraded
    iterations of tests/test_laplace_hard_oracle.py)."""
    tol, a0 = start(c, path)
    keep = LO.newton_step, LO.psi
    newton = step if step is not None else keep[0]
    trace = []

    def counted_step(*args):
        trace.append([])
        return newton(*args)

    def counted_psi(*args):
        v = keep[1](*args)
        if trace:
            trace[-1].append(v)
        return v

    try:
        LO.newton_step, LO.psi = counted_step, counted_psi
        r = LO.laplace(c["X"], c["terms"], LO.JITTER, c["lik"], c["y"], polish=0, tol=tol, a0=a0)
    finally:
        LO.newton_step, LO.psi = keep
    # every step's list but the last ends with the next step's psi_old
    trials = [t[:-1] for t in trace[:-1]] + trace[-1:]
    r.trace = [(len(t) - 1, sum(1 for v in t if not np.isfinite(v))) for t in trials]
    return r


def yardstick_of(c, step=None):
    """(runs, errors per path, the largest per output, residual per path) of the yardstick's paths."""
    runs = [iterate(c, p, step) for p in PATHS]
    outs = [outputs(r, c["X"], c["Xs"], c["terms"], c["lik"])[0] for r in runs]
    errs = [errors(o, c) for o in outs]
    worst = {k: max(e[k] for e in errs) for k in errs[0]}
    return runs, outs, errs, worst, [residual(c, r.a) for r in runs]


def predict_ys(c):
    """Observations at the test points to score: labels 0, 1, 0, ... (each point's unlikely label
    among them), or counts drawn at the reference's rates."""
    if c["lik"] == LO.BERNOULLI:
        return (np.arange(M) % 2).astype(np.float64)
    rng = np.random.default_rng(_seed(c["key"][0], c["key"][1], 50))
    return rng.poisson(np.exp(c["out"]["mean"])).astype(np.float64)


_cache = {}


def case(key):
    """One case computed once and shared, read-only: X, Xs, y, terms, lik, res (the reference), out
    (its outputs), grad, kdiag, Kx and shift (split(K)), runs / outs / errs / path_res (the
    yardstick's paths), yard (the yardstick per output), yard_res (its residual: the largest of the
    paths'), ref_res (the reference's)."""
    if key not in _cache:
        X, Xs, terms, lik, y = design(key)
        res = refine(LO.laplace(X, terms, LO.JITTER, lik, y), lik, y, EXTENDED)
        out, g = outputs(res, X, Xs, terms, lik)
        c = dict(key=key, X=X, Xs=Xs, y=y, terms=terms, lik=lik, lik_param=0.0, res=res, out=out, grad=g,
                 kdiag=R.kernel_diag(Xs, terms))
        c["Kx"], c["shift"] = split(res.K)
        c["ref_res"] = residual(c, res.a)
        c["runs"], c["outs"], c["errs"], c["yard"], rr = yardstick_of(c)
        c["path_res"], c["yard_res"] = rr, max(rr)
        for arr in (X, Xs, y, res.a, res.f, *[v for v in out.values() if isinstance(v, np.ndarray)]):
            arr.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def bar(yard, flat=1e-9):
    """The bar of an output whose yardstick is `yard`: the project's flat 1e-9 where the yardstick
    is below 1e-10, within a digit of the yardstick (DESIGN.md §5.2's margin) beyond."""
    return max(flat, 10.0 * yard)


def violations(c, errs, resid=None):
    """The outputs of `errs` (a dict as errors() returns) beyond their bars, and the residual
    `resid` of the same run's a where it is beyond its own; one line each, [] when all is met."""
    bad = [f"{k}: error {e:.3e} > bar {bar(c['yard'][k]):.3e} (yardstick {c['yard'][k]:.3e})"
           for k, e in errs.items() if not e <= bar(c["yard"][k])]
    if resid is not None and not resid <= bar(c["yard_res"]):
        bad.append(f"residual: {resid:.3e} > bar {bar(c['yard_res']):.3e} (yardstick {c['yard_res']:.3e})")
    return bad


def row(c):
    """One line of the table: the design, max W, cond(B), steps / halvings, the yardstick."""
    res, y = c["res"], c["yard"]
    ev = np.linalg.eigvalsh(res.L @ res.L.T)
    imp = max(v for k, v in y.items() if k.startswith("implicit"))
    dpar = max(v for k, v in y.items() if k.startswith("dparam"))
    it = "/".join(f"{r.iters}:{r.halvings}" for r in c["runs"])
    return (f"{case_id(c['key']):18s} maxW {np.max(res.W):8.2e} minW {np.min(res.W):8.2e} cond(B) {ev[-1] / ev[0]:8.2e} "
            f"ref {res.iters}:{res.halvings} paths {it:14s} a {y['a']:.1e} f {y['f']:.1e} logq {y['logq']:.1e} "
            f"mean {y['mean']:.1e} var {y['var']:.1e} cov {y['cov']:.1e} dparam {dpar:.1e} djit {y['djitter']:.1e} "
            f"impl {imp:.1e} ymean {y['ymean']:.1e} yvar {y['yvar']:.1e} resid {c['yard_res']:.1e} (ref {c['ref_res']:.1e})")
