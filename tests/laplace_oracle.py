"""numpy / scipy restatement of the Laplace approximation of DESIGN.md §10.13 (Rasmussen &
Williams, Algorithms 3.1 and 5.1), on oracle.restatement's gram / cross_gram / kernel_diag.

K = gram(X, terms, jitter). One Newton step from (a, f), f = K a, with g = grad log p, W = -hess
log p (diagonal), sw = sqrt(W):

    B = I + sw K sw,  L = chol(B),  b = W f + g,  c = K b,  a+ = b - sw B^{-1} (sw c),  f+ = K a+
    psi(a, f) = -a^T f / 2 + sum_i log p(y_i | f_i)

then (a, f) + s ((a+, f+) - (a, f)) with the first s = 1, 1/2, ... (at most 20 halvings) whose psi
is finite and >= psi_old - tol (1 + |psi_old|); stop when |psi_new - psi_old| <= tol (1 + |psi_new|)
or after max_iter steps. After meeting tol this restatement takes `polish` (two) more full Newton
steps (polish_step: the step in its residual form, the residual in extended precision), so that its
f is limited neither by tol nor by cond(B); the step count it reports is the one at which tol was
met. Then W at the last f, B factored once more, and

    log q = -a^T f / 2 + sum log p - sum_i log L_ii
    mean_j = k(xs_j, X) a,   var_j = k(xs_j, xs_j) - |L^{-1} (sw k(X, xs_j))|^2
"""
import numpy as np
import scipy.linalg
import scipy.special

from oracle import restatement as R

GAUSSIAN, BERNOULLI, POISSON = 0, 1, 2  # GAPLAC_LIK_*
LOG2PI = 1.8378770664093453


def lik_terms(lik, param, y, f):
    """(log p, g, W) per observation."""
    if lik == BERNOULLI:
        lp = y * f - np.logaddexp(0.0, f)
        pi = scipy.special.expit(f)
        return lp, y - pi, pi * (1.0 - pi)
    if lik == POISSON:
        with np.errstate(over="ignore"):
            m = np.exp(f)
        return y * f - m - scipy.special.gammaln(y + 1.0), y - m, m
    if lik == GAUSSIAN:
        r = y - f
        return -0.5 * (LOG2PI + np.log(param)) - 0.5 * r * r / param, r / param, np.full_like(f, 1.0 / param)
    raise ValueError(f"unknown likelihood {lik}")


def psi(lik, param, y, a, f):
    with np.errstate(invalid="ignore", over="ignore"):
        return -0.5 * float(a @ f) + float(np.sum(lik_terms(lik, param, y, f)[0]))


def newton_step(K, lik, param, y, f):
    """(a+, f+) of one full Newton step from f."""
    _, g, W = lik_terms(lik, param, y, f)
    sw = np.sqrt(W)
    B = np.eye(K.shape[0]) + sw[:, None] * K * sw[None, :]
    L = np.linalg.cholesky(B)
    b = W * f + g
    c = K @ b
    u = scipy.linalg.solve_triangular(L, sw * c, lower=True, check_finite=False)
    u = scipy.linalg.solve_triangular(L, u, lower=True, trans="T", check_finite=False)
    an = b - sw * u
    return an, K @ an


def grad_extended(lik, param, y, f):
    """g at an extended-precision f (np.longdouble)."""
    if lik == BERNOULLI:
        e = np.exp(-np.abs(f))
        return y - np.where(f >= 0, 1 / (1 + e), e / (1 + e))
    if lik == POISSON:
        return y - np.exp(f)
    return (y - f) / np.longdouble(param)


def polish_step(K, lik, param, y, a):
    """The same Newton step in its residual form, a+ = a + (I + W K)^{-1} (g(K a) - a), with K a and
    the residual in extended precision: the step's rounding error then scales with the (small)
    correction, not with cond(B), so the mode it ends at satisfies a = g(K a) to a few ulps.
    (I + W K)^{-1} r = r - sw B^{-1} (sw K r).  Returns (a+, f+ = K a+ rounded once)."""
    Kx = K.astype(np.longdouble)
    f = (Kx @ a.astype(np.longdouble))
    res = (grad_extended(lik, param, y.astype(np.longdouble), f) - a).astype(np.float64)
    _, _, W = lik_terms(lik, param, y, f.astype(np.float64))
    sw = np.sqrt(W)
    L = np.linalg.cholesky(np.eye(K.shape[0]) + sw[:, None] * K * sw[None, :])
    u = scipy.linalg.solve_triangular(L, sw * (K @ res), lower=True, check_finite=False)
    u = scipy.linalg.solve_triangular(L, u, lower=True, trans="T", check_finite=False)
    an = (a.astype(np.longdouble) + (res - sw * u)).astype(np.float64)
    return an, (Kx @ an.astype(np.longdouble)).astype(np.float64)


class Result:
    pass


def laplace(X, terms, jitter, lik, y, lik_param=0.0, max_iter=100, tol=1e-12, a0=None, polish=2, line_search=True):
    """The iteration; a Result with logq, f, a, iters, converged, halvings, sw, L, K."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    N = X.shape[0]
    K = R.gram(X, terms, jitter)
    a = np.zeros(N) if a0 is None else np.array(a0, dtype=np.float64)
    f = K @ a
    r = Result()
    r.iters, r.converged, r.halvings = 0, False, 0
    for _ in range(max_iter):
        psi_old = psi(lik, lik_param, y, a, f)
        an, fn = newton_step(K, lik, lik_param, y, f)
        s, ok = 1.0, False
        for _h in range(21 if line_search else 1):
            at, ft = (an, fn) if s == 1.0 else (a + s * (an - a), f + s * (fn - f))
            psi_new = psi(lik, lik_param, y, at, ft)
            if not line_search or (np.isfinite(psi_new) and psi_new >= psi_old - tol * (1.0 + abs(psi_old))):
                ok = True
                break
            s *= 0.5
            r.halvings += 1
        if not ok:
            break
        a, f = at, ft
        r.iters += 1
        if abs(psi_new - psi_old) <= tol * (1.0 + abs(psi_new)):
            r.converged = True
            break
    for _ in range(polish if r.converged else 0):
        a, f = polish_step(K, lik, lik_param, y, a)
    lp, g, W = lik_terms(lik, lik_param, y, f)
    sw = np.sqrt(W)
    L = np.linalg.cholesky(np.eye(N) + sw[:, None] * K * sw[None, :])
    r.logq = -0.5 * float(a @ f) + float(np.sum(lp)) - float(np.sum(np.log(np.diag(L))))
    r.a, r.f, r.g, r.W, r.sw, r.L, r.K = a, f, g, W, sw, L, K
    return r


def logq_by_lu(r, lik, lik_param, y):
    """log q by a second route: log p - a^T f / 2 - slogdet(I + K W) / 2 through LU."""
    sign, ld = np.linalg.slogdet(np.eye(r.K.shape[0]) + r.K * r.W[None, :])
    assert sign > 0
    return float(np.sum(lik_terms(lik, lik_param, y, r.f)[0])) - 0.5 * float(r.a @ r.f) - 0.5 * float(ld)


def posterior_mean_var(r, X, terms, Xs):
    """Latent mean and variance at the rows of Xs from a laplace() result."""
    Ks = R.cross_gram(np.asarray(Xs, dtype=np.float64), np.asarray(X, dtype=np.float64), terms)  # M x N
    V = scipy.linalg.solve_triangular(r.L, r.sw[:, None] * Ks.T, lower=True, check_finite=False)
    return Ks @ r.a, R.kernel_diag(np.asarray(Xs, dtype=np.float64), terms) - np.sum(V * V, axis=0)


# ---- the data recipe of the tests -------------------------------------------------------------
SQEXP_TERMS = [(1, 0, 1.5, 0)]                                             # SqExp(l = 1.5) on column 0
COMPOSITE = [(1, 0, 1.5, 0), (2, 0, 3.0, 1), (4, 1, 0.0, 2), (3, 2, 0.5, 3)]  # tests/test_gpu_fit.py's
TERM_SETS = {"sqexp": SQEXP_TERMS, "composite": COMPOSITE}
LIKS = {"bernoulli": (BERNOULLI, 0.0), "poisson": (POISSON, 0.0), "gaussian": (GAUSSIAN, 0.1)}
JITTER = 1e-6


def inputs(N, M):
    """(X, Xs) of tests/test_gpu_fit.composite(N, M)."""
    from tests.test_gpu_fit import composite

    X, Xs, _ = composite(N, M)
    return X, Xs


def data(N, M, terms_name, lik_name):
    """(X, Xs, y): X from test_gpu_fit.composite, a latent draw 0.5 chol(K + 1e-8 I) z under the term
    set, and y = Bernoulli(sigma(f)), Poisson(exp(clip(f, -5, 3))) or f + sqrt(0.1) eps, seeded."""
    X, Xs = inputs(N, M)
    rng = np.random.default_rng(1000 * N + 10 * sorted(TERM_SETS).index(terms_name) + sorted(LIKS).index(lik_name))
    K = R.gram(X, TERM_SETS[terms_name], JITTER)
    f = 0.5 * (np.linalg.cholesky(K + 1e-8 * np.eye(N)) @ rng.normal(size=N))
    if lik_name == "bernoulli":
        y = (rng.uniform(size=N) < scipy.special.expit(f)).astype(np.float64)
    elif lik_name == "poisson":
        y = rng.poisson(np.exp(np.clip(f, -5.0, 3.0))).astype(np.float64)
    else:
        y = f + np.sqrt(0.1) * rng.normal(size=N)
    return X, Xs, y


_cache = {}


def case(N, M, terms_name, lik_name):
    """One case computed once and shared, read-only: dict with X, Xs, y, terms, lik, lik_param, res
    (the laplace() result), mean, var, kdiag."""
    key = (N, M, terms_name, lik_name)
    if key not in _cache:
        X, Xs, y = data(N, M, terms_name, lik_name)
        terms = TERM_SETS[terms_name]
        lik, param = LIKS[lik_name]
        res = laplace(X, terms, JITTER, lik, y, param)
        mean, var = posterior_mean_var(res, X, terms, Xs)
        kd = R.kernel_diag(Xs, terms)
        for arr in (X, Xs, y, res.a, res.f, mean, var, kd):
            arr.setflags(write=False)
        _cache[key] = dict(X=X, Xs=Xs, y=y, terms=terms, lik=lik, lik_param=param, res=res, mean=mean, var=var,
                           kdiag=kd)
    return _cache[key]
