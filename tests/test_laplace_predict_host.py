"""gaplac_gauss_hermite / gaplac_laplace_predict: host arithmetic of the library,
no device.

Bars. The rule against numpy's hermgauss: nodes within 1e-14 max(1, |x|), weights within 1e-13
relative. The predictions against tests/laplace_predict_oracle.predict at the same Q: 1e-12 max(1,
|value|), the project's bar between two fp64 routes to one formula (both sum Q <= 64 terms of like
sign, so their roundings differ by a few Q ulps). The restatement at Q = 32 against adaptive
quadrature: 1e-9 on each case's 40 largest-variance points (measured: at most 1.6e-11, Poisson,
composite terms, variance up to 0.55).
"""
import ctypes

import numpy as np
import pytest
import scipy.special
from numpy.polynomial.hermite import hermgauss

from gaplac_amd import _native, backend
from gaplac_amd.backend import ArgumentError
from tests import laplace_oracle as LO
from tests import laplace_predict_oracle as PO

CASES = [(t, l) for t in ("sqexp", "composite") for l in ("bernoulli", "poisson", "gaussian")]


def draw_ys(lik_name, f, seed):
    """Observations at the test points drawn as tests/laplace_oracle.data draws them."""
    rng = np.random.default_rng(seed)
    if lik_name == "bernoulli":
        return (rng.uniform(size=f.size) < scipy.special.expit(f)).astype(np.float64)
    if lik_name == "poisson":
        return rng.poisson(np.exp(np.clip(f, -5.0, 3.0))).astype(np.float64)
    return f + np.sqrt(0.1) * rng.normal(size=f.size)


def case_inputs(terms_name, lik_name):
    c = LO.case(300, 1000, terms_name, lik_name)
    ys = draw_ys(lik_name, c["mean"], 17 + CASES.index((terms_name, lik_name)))
    return c["lik"], c["lik_param"], c["mean"], c["var"], ys


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.mark.parametrize("Q", [1, 2, 20, 32, 64])
def test_gauss_hermite_matches_hermgauss(Q):
    x, w = backend.gauss_hermite(Q)
    rx, rw = hermgauss(Q)
    ex = float(np.max(np.abs(x - rx) / np.maximum(1.0, np.abs(rx))))
    ew = float(np.max(np.abs(w - rw) / rw))
    print(f"Q={Q}: nodes {ex:.3e}, weights {ew:.3e} (relative)")
    assert ex <= 1e-14 and ew <= 1e-13
    assert np.all(np.diff(x) > 0)


def test_gauss_hermite_rejects_bad_orders():
    lib = _native.load()
    buf = np.zeros(80)
    for Q in (0, 65, -3):
        assert lib.gaplac_gauss_hermite(Q, buf.ctypes.data, buf.ctypes.data) == _native.E_ARG
        with pytest.raises(ArgumentError):
            backend.gauss_hermite(Q)
    assert lib.gaplac_gauss_hermite(5, None, None) == 0  # either output may be NULL


@pytest.mark.parametrize("terms_name,lik_name", CASES)
@pytest.mark.parametrize("Q", [20, 32])
def test_predict_matches_the_restatement(terms_name, lik_name, Q):
    lik, param, mean, var, ys = case_inputs(terms_name, lik_name)
    ym, yv, lp = backend.laplace_predict(lik, mean, var, ys, lik_param=param, Q=Q)
    rm, rv, rl = PO.predict(lik, mean, var, ys, lik_param=param, Q=Q)
    errs = rel(ym, rm), rel(yv, rv), rel(lp, rl)
    print(f"{terms_name} {lik_name} Q={Q}: ymean {errs[0]:.3e} yvar {errs[1]:.3e} logp {errs[2]:.3e}")
    assert max(errs) <= 1e-12
    ym2, yv2 = backend.laplace_predict(lik, mean, var, lik_param=param, Q=Q)  # no score
    assert np.array_equal(ym2, ym) and np.array_equal(yv2, yv)


@pytest.mark.parametrize("terms_name,lik_name", [c for c in CASES if c[1] != "gaussian"])
def test_restatement_at_q32_matches_adaptive_quadrature(terms_name, lik_name):
    lik, param, mean, var, ys = case_inputs(terms_name, lik_name)
    top = np.argsort(var)[-40:]
    _, _, rl = PO.predict(lik, mean[top], var[top], ys[top], lik_param=param, Q=32)
    ref = PO.logp_quad(lik, mean[top], var[top], ys[top])
    e = rel(rl, ref)
    print(f"{terms_name} {lik_name}: Q=32 against quad {e:.3e} (largest variance {var[top].max():.3f})")
    assert e <= 1e-9


def test_edges():
    B, P, G = _native.LIK_BERNOULLI, _native.LIK_POISSON, _native.LIK_GAUSSIAN
    # var = 0: log p(ys | mean) itself; a slightly negative variance is clamped to it
    mu = np.array([-1.3, 0.0, 2.1])
    for lik, ys in ((B, np.array([1.0, 0.0, 1.0])), (P, np.array([0.0, 3.0, 7.0]))):
        for v in (0.0, -1e-14):
            ym, yv, lp = backend.laplace_predict(lik, mu, np.full(3, v), ys)
            assert np.array_equal(lp, PO.lik_logp(lik, ys, mu)) or rel(lp, PO.lik_logp(lik, ys, mu)) <= 1e-15
            rm, rv, _ = PO.predict(lik, mu, np.zeros(3), ys)
            assert rel(ym, rm) <= 1e-12 and rel(yv, rv) <= 1e-12
    # Bernoulli deep in both tails
    mu, v, ys = np.array([40.0, -40.0, 40.0, -40.0]), np.ones(4), np.array([1.0, 1.0, 0.0, 0.0])
    ym, yv, lp = backend.laplace_predict(B, mu, v, ys)
    rm, rv, rl = PO.predict(B, mu, v, ys)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(ym)) and np.all(np.isfinite(yv))
    assert max(rel(ym, rm), rel(yv, rv), rel(lp, rl)) <= 1e-12
    # Poisson with a large count
    mu, v, ys = np.array([9.0, 9.3]), np.array([0.02, 0.3]), np.array([1e4, 1e4])
    ym, yv, lp = backend.laplace_predict(P, mu, v, ys)
    rm, rv, rl = PO.predict(P, mu, v, ys)
    assert np.all(np.isfinite(lp)) and max(rel(ym, rm), rel(yv, rv), rel(lp, rl)) <= 1e-12
    # NaN in gives NaN out at that point only
    for lik, ys, par in ((B, np.array([1.0, 0.0, 1.0, 0.0]), 0.0), (P, np.array([1.0, 0.0, 2.0, 5.0]), 0.0),
                         (G, np.array([0.1, 0.2, 0.3, 0.4]), 0.1)):
        mu, v = np.array([0.3, np.nan, -0.2, 0.5]), np.array([0.2, 0.1, np.inf, 0.4])
        out = backend.laplace_predict(lik, mu, v, ys, lik_param=par)
        ref = PO.predict(lik, mu, v, ys, lik_param=par)
        for o, r in zip(out, ref):
            assert np.all(np.isnan(o[1:3])) and np.all(np.isfinite(o[[0, 3]]))
            assert rel(o[[0, 3]], r[[0, 3]]) <= 1e-12
    # ys outside the support, an unknown likelihood, a bad order
    lib = _native.load()
    one, out = np.array([0.5]), np.full(1, 7.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for lik, bad in ((B, 0.5), (B, 2.0), (P, -1.0), (P, 1.5), (P, np.inf), (G, np.nan)):
        ys = np.array([bad])
        assert lib.gaplac_laplace_predict(lik, 0.1, 1, p(one), p(one), p(ys), 32, p(out), None, None) == _native.E_PARAM
        assert np.isnan(out[0])  # NaN-filled first
        with pytest.raises(ArgumentError):
            backend.laplace_predict(lik, one, one, ys, lik_param=0.1)
    assert lib.gaplac_laplace_predict(7, 0.0, 1, p(one), p(one), None, 32, p(out), None, None) == _native.E_KIND
    assert lib.gaplac_laplace_predict(B, 0.0, 1, p(one), p(one), None, 0, p(out), None, None) == _native.E_ARG
    assert lib.gaplac_laplace_predict(B, 0.0, 1, p(one), p(one), None, 65, p(out), None, None) == _native.E_ARG
    assert lib.gaplac_laplace_predict(B, 0.0, 1, None, p(one), None, 32, p(out), None, None) == _native.E_ARG
    assert lib.gaplac_laplace_predict(B, 0.0, -1, p(one), p(one), None, 32, p(out), None, None) == _native.E_ARG
    # every output may be NULL; M = 0
    assert lib.gaplac_laplace_predict(B, 0.0, 1, p(one), p(one), p(np.array([1.0])), 32, None, None, None) == 0
    assert lib.gaplac_laplace_predict(P, 0.0, 0, None, None, None, 32, None, None, None) == 0
    ym, yv, lp = backend.laplace_predict("poisson", np.zeros(0), np.zeros(0), np.zeros(0))
    assert ym.shape == yv.shape == lp.shape == (0,)


def test_gaussian_is_closed_form():
    mu, v, ys = np.array([0.2, -1.0]), np.array([0.5, 0.0]), np.array([0.0, 1.0])
    ym, yv, lp = backend.laplace_predict("gaussian", mu, v, ys, lik_param=0.1, Q=0)  # Q ignored
    assert np.array_equal(ym, mu) and np.array_equal(yv, v + 0.1)
    ref = -0.5 * (np.log(2 * np.pi * (v + 0.1)) + (ys - mu) ** 2 / (v + 0.1))
    assert rel(lp, ref) <= 1e-15
