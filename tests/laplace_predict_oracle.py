"""numpy restatement of gaplac_laplace_predict on numpy's own Gauss-Hermite
rule, and the same integrals by adaptive quadrature.

With v = max(var, 0), s = sqrt(v), (x_q, w_q) = numpy.polynomial.hermite.hermgauss(Q) and f_q = mean
+ sqrt(2) s x_q:   int h(f) N(f | mean, v) df ~ pi^{-1/2} sum_q w_q h(f_q).

    gaussian   ymean = mean, yvar = v + param, logp = log N(ys; mean, v + param)
    poisson    ymean = exp(mean + v/2), yvar = ymean + expm1(v) ymean^2,
               logp = logsumexp_q[log w_q + ys f_q - e^{f_q} - lgamma(ys + 1)] - log(pi) / 2
    bernoulli  ymean = p = min(1, pi^{-1/2} sum_q w_q sigma(f_q)), yvar = p (1 - p),
               logp = logsumexp_q[log w_q + ys f_q - log(1 + e^{f_q})] - log(pi) / 2
"""
import numpy as np
import scipy.integrate
import scipy.special
from numpy.polynomial.hermite import hermgauss

GAUSSIAN, BERNOULLI, POISSON = 0, 1, 2  # GAPLAC_LIK_*
LOG2PI = 1.8378770664093453


def lik_logp(lik, y, f):
    if lik == BERNOULLI:
        return y * f - np.logaddexp(0.0, f)
    with np.errstate(over="ignore"):
        return y * f - np.exp(f) - scipy.special.gammaln(y + 1.0)


def predict(lik, mean, var, ys=None, lik_param=0.0, Q=32):
    """(ymean, yvar, logp or None), one entry per point; NaN where mean or var is not finite."""
    mean = np.asarray(mean, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    bad = ~(np.isfinite(mean) & np.isfinite(var))
    mu = np.where(bad, 0.0, mean)
    v = np.where(bad, 0.0, np.maximum(var, 0.0))
    logp = None
    if lik == GAUSSIAN:
        ymean, yvar = mu.copy(), v + lik_param
        if ys is not None:
            logp = -0.5 * (LOG2PI + np.log(yvar)) - 0.5 * (ys - mu) ** 2 / yvar
    else:
        x, w = hermgauss(Q)
        f = mu[:, None] + np.sqrt(2.0) * np.sqrt(v)[:, None] * x[None, :]
        if lik == POISSON:
            ymean = np.exp(mu + 0.5 * v)
            yvar = ymean + np.expm1(v) * ymean * ymean
        else:
            # (the rounded weights sum to sqrt(pi) (1 + 2^-52): where every sigma(f_q) is 1 the sum
            # is one ulp above 1 and p (1 - p) negative; a probability is at most 1)
            ymean = np.minimum((scipy.special.expit(f) @ w) / np.sqrt(np.pi), 1.0)
            yvar = ymean * (1.0 - ymean)
        if ys is not None:
            t = np.log(w)[None, :] + lik_logp(lik, np.asarray(ys, dtype=np.float64)[:, None], f)
            logp = scipy.special.logsumexp(t, axis=1) - 0.5 * np.log(np.pi)
            point = v == 0.0  # a point mass: the likelihood at the mean itself
            logp[point] = lik_logp(lik, np.asarray(ys, dtype=np.float64)[point], mu[point])
    out = [ymean, yvar] + ([logp] if logp is not None else [])
    for a in out:
        a[bad] = np.nan
    return ymean, yvar, logp


def logp_quad(lik, mean, var, ys):
    """log int p(ys | f) N(f | mean, var) df per point by scipy.integrate.quad (epsrel 1e-13) over
    mean +- 12 sd, the integrand scaled by its value at its largest node so nothing underflows."""
    out = np.empty(len(mean))
    for j, (m, v, y) in enumerate(zip(mean, var, ys)):
        s = np.sqrt(v)
        grid = np.linspace(m - 12 * s, m + 12 * s, 2001)
        lg = lik_logp(lik, y, grid) - 0.5 * ((grid - m) / s) ** 2
        top = np.max(lg)

        def h(f):
            return np.exp(lik_logp(lik, y, f) - 0.5 * ((f - m) / s) ** 2 - top)

        val, _ = scipy.integrate.quad(h, m - 12 * s, m + 12 * s, epsrel=1e-13, epsabs=0.0, limit=400,
                                      points=[grid[np.argmax(lg)]])
        out[j] = np.log(val) + top - 0.5 * np.log(2.0 * np.pi * v)
    return out
