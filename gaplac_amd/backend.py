"""Python handle on the HIP backend: a device context and the logpdf entry points.

This is the Python mirror of the `ccall` glue a GaPLAC maintainer would add in Julia
(INTEGRATION.md); numpy arrays stand in for Julia's GC-owned column-major buffers.
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_double, c_int32, c_int64, c_void_p

import numpy as np

from . import _native
from ._native import Term, term_array


class GaplacError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"gaplac error {code}: {msg}")
        self.code = code


class PosDefException(ArithmeticError):
    """Mirror of Julia's LinearAlgebra.PosDefException(info) (cholesky check=true)."""

    def __init__(self, info: int):
        super().__init__(f"PosDefException: matrix is not positive definite; Cholesky factorization failed (info={info})")
        self.info = info


class ArgumentError(ValueError):
    """Mirror of Julia's ArgumentError for invalid kernel parameters / arguments."""


def _colmajor(X: np.ndarray) -> np.ndarray:
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    return np.asfortranarray(X)


_LIK_CODES = {"gaussian": _native.LIK_GAUSSIAN, "bernoulli": _native.LIK_BERNOULLI, "poisson": _native.LIK_POISSON}


def likelihood_code(lik) -> int:
    """GAPLAC_LIK_* of a likelihood given by name (any case) or by code; an unknown name is an
    ArgumentError, an unknown code is left to the library (GAPLAC_E_KIND)."""
    if isinstance(lik, str):
        try:
            return _LIK_CODES[lik.lower()]
        except KeyError:
            raise ArgumentError(f"unknown likelihood {lik!r}; expected one of {sorted(_LIK_CODES)}") from None
    return int(lik)


class LaplaceResult:
    """What gaplac_laplace_logpdf returns: log q, the mode f, a = K^{-1} f, the Newton steps taken
    and whether the iteration met its tolerance."""

    def __init__(self, logq: float, f: np.ndarray, a: np.ndarray, iters: int, converged: bool):
        self.logq, self.f, self.a, self.iters, self.converged = logq, f, a, iters, converged

    def __repr__(self):
        return f"LaplaceResult(logq={self.logq!r}, iters={self.iters}, converged={self.converged})"


class LaplaceGradResult(LaplaceResult):
    """What gaplac_laplace_logpdf_grad returns: a LaplaceResult with dparam (one entry per term, in
    the term's own parameter), djitter, and implicit (T + 1 values: the parts of dparam and djitter
    that come from the mode's dependence on the parameter)."""

    def __init__(self, logq, f, a, iters, converged, dparam: np.ndarray, djitter: float, implicit: np.ndarray):
        super().__init__(logq, f, a, iters, converged)
        self.dparam, self.djitter, self.implicit = dparam, djitter, implicit

    def __repr__(self):
        return (f"LaplaceGradResult(logq={self.logq!r}, dparam={self.dparam!r}, djitter={self.djitter!r}, "
                f"iters={self.iters}, converged={self.converged})")


class Context:
    """One device, one persistent workspace (gaplac_ctx)."""

    def __init__(self, device: int = 0):
        self.lib = _native.load()
        h = c_void_p()
        rc = self.lib.gaplac_ctx_create(int(device), byref(h))
        if rc != 0:
            raise GaplacError(rc, f"gaplac_ctx_create(device={device}) failed")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.gaplac_ctx_destroy(self.h)
            self.h = None

    def release(self):
        """Free the large device workspaces (gaplac_ctx_release); the next call re-allocates."""
        self._check(self.lib.gaplac_ctx_release(self.h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------------ helpers
    def _check(self, rc: int):
        if rc == 0:
            return
        if rc > 0:
            raise PosDefException(rc)
        msg = self.lib.gaplac_last_error(self.h)
        msg = msg.decode() if msg else ""
        if rc in (_native.E_PARAM, _native.E_KIND, _native.E_COL, _native.E_ARG):
            raise ArgumentError(f"gaplac error {rc}: {msg}")
        raise GaplacError(rc, msg)

    # ------------------------------------------------------------------ entries
    def logpdf(self, X, terms, noise: float, v, full: bool = False):
        """logpdf of the zero-mean FiniteGP; full=True returns (logpdf, logdet, quad)."""
        Xc = _colmajor(X)
        v = np.ascontiguousarray(v, dtype=np.float64)
        N, D = Xc.shape
        if v.shape[0] != N:
            raise ArgumentError(f"length of v ({v.shape[0]}) != N ({N})")
        terms = list(terms)  # one pass: a generator must not reach the library as T = 0
        ta = term_array(terms)
        lp, ld, q = c_double(), c_double(), c_double()
        rc = self.lib.gaplac_logpdf(
            self.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), ta, float(noise),
            v.ctypes.data_as(c_void_p), byref(lp), byref(ld), byref(q),
        )
        self._check(rc)
        return (lp.value, ld.value, q.value) if full else lp.value

    def logpdf_device(self, N: int, D: int, dX_ptr: int, ldx: int, terms, noise: float, dv_ptr: int, full=False):
        terms = list(terms)
        ta = term_array(terms)
        lp, ld, q = c_double(), c_double(), c_double()
        rc = self.lib.gaplac_logpdf_device(
            self.h, N, D, c_void_p(dX_ptr), ldx, len(terms), ta, float(noise), c_void_p(dv_ptr),
            byref(lp), byref(ld), byref(q),
        )
        self._check(rc)
        return (lp.value, ld.value, q.value) if full else lp.value

    def logpdf_batch(self, X, models, noise: float, v):
        """models: list of term lists. Returns (logpdf array, info array)."""
        Xc = _colmajor(X)
        v = np.ascontiguousarray(v, dtype=np.float64)
        N, D = Xc.shape
        offs = [0]
        flat = []
        models = [list(m) for m in models]
        for m in models:
            flat.extend(m)
            offs.append(len(flat))
        ta = term_array(flat)
        off_arr = (c_int32 * len(offs))(*offs)
        out = np.empty(len(models), dtype=np.float64)
        info = np.zeros(len(models), dtype=np.int64)
        rc = self.lib.gaplac_logpdf_batch(
            self.h, len(models), N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), off_arr, ta, float(noise),
            v.ctypes.data_as(c_void_p), out.ctypes.data_as(ctypes.POINTER(c_double)),
            info.ctypes.data_as(ctypes.POINTER(c_int64)),
        )
        self._check(rc)
        return out, info

    def logpdf_grad(self, X, terms, noise: float, v):
        """(logpdf, dv, dparam, dnoise): logpdf and its gradient with respect to v, to each
        term's parameter (l / c / variance; 0 for Cat) and to the observation variance
        (gaplac_logpdf_grad)."""
        Xc = _colmajor(X)
        v = np.ascontiguousarray(v, dtype=np.float64)
        N, D = Xc.shape
        if v.shape[0] != N:
            raise ArgumentError(f"length of v ({v.shape[0]}) != N ({N})")
        terms = list(terms)
        ta = term_array(terms)
        lp, dn = c_double(), c_double()
        dv = np.empty(N, dtype=np.float64)
        dp = np.empty(max(1, len(terms)), dtype=np.float64)
        rc = self.lib.gaplac_logpdf_grad(
            self.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), ta, float(noise),
            v.ctypes.data_as(c_void_p), byref(lp), dv.ctypes.data_as(c_void_p), dp.ctypes.data_as(c_void_p),
            byref(dn),
        )
        self._check(rc)
        return lp.value, dv, dp[: len(terms)].copy(), dn.value

    def logpdf_grad_device(self, N: int, D: int, dX_ptr: int, ldx: int, terms, noise: float, dv_ptr: int,
                           want_dv: bool = True):
        """Device-resident inputs; returns (logpdf, dv or None, dparam, dnoise)."""
        terms = list(terms)
        ta = term_array(terms)
        lp, dn = c_double(), c_double()
        dv = np.empty(N, dtype=np.float64) if want_dv else None
        dp = np.empty(max(1, len(terms)), dtype=np.float64)
        rc = self.lib.gaplac_logpdf_grad_device(
            self.h, N, D, c_void_p(dX_ptr), ldx, len(terms), ta, float(noise), c_void_p(dv_ptr), byref(lp),
            dv.ctypes.data_as(c_void_p) if want_dv else None, dp.ctypes.data_as(c_void_p), byref(dn),
        )
        self._check(rc)
        return lp.value, dv, dp[: len(terms)].copy(), dn.value

    def posterior_mean_var(self, X, terms, noise: float, y, Xs):
        """(mean, var) of the posterior of the zero-mean FiniteGP given y, at the rows of Xs
        (gaplac_posterior_mean_var)."""
        Xc = _colmajor(X)
        y = np.ascontiguousarray(y, dtype=np.float64)
        N, D = Xc.shape
        if y.shape[0] != N:
            raise ArgumentError(f"length of y ({y.shape[0]}) != N ({N})")
        Xsc = _colmajor(Xs)
        M = Xsc.shape[0]
        if Xsc.shape[1] != D:
            raise ArgumentError(f"test inputs have {Xsc.shape[1]} columns, training inputs {D}")
        terms = list(terms)
        ta = term_array(terms)
        mean = np.empty(M, dtype=np.float64)
        var = np.empty(M, dtype=np.float64)
        rc = self.lib.gaplac_posterior_mean_var(
            self.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), ta, float(noise),
            y.ctypes.data_as(c_void_p), M, Xsc.ctypes.data_as(c_void_p), max(M, 1),
            mean.ctypes.data_as(c_void_p), var.ctypes.data_as(c_void_p),
        )
        self._check(rc)
        return mean, var

    # ---- Laplace approximation (gaplac_laplace_logpdf / _posterior_mean_var) ----
    def _laplace_args(self, X, terms, jitter, lik, y, lik_param, max_iter, tol, a0):
        Xc = _colmajor(X)
        y = np.ascontiguousarray(y, dtype=np.float64)
        N, D = Xc.shape
        if y.ndim != 1 or y.shape[0] != N:
            raise ArgumentError(f"length of y ({y.shape[0] if y.ndim else 0}) != N ({N})")
        if a0 is not None:
            a0 = np.ascontiguousarray(a0, dtype=np.float64)
            if a0.shape != (N,):
                raise ArgumentError(f"a0 has shape {a0.shape}, expected ({N},)")
        terms = list(terms)
        keep = (Xc, y, a0, term_array(terms))
        args = [self.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), keep[3], float(jitter),
                likelihood_code(lik), float(lik_param), y.ctypes.data_as(c_void_p), int(max_iter), float(tol),
                a0.ctypes.data_as(c_void_p) if a0 is not None else None]
        return keep, N, D, args

    @staticmethod
    def _laplace_warn(converged: bool, iters: int):
        if not converged:
            import warnings

            warnings.warn(f"the Laplace approximation's Newton iteration did not converge in {iters} step(s); "
                          "the results are those of the last iterate", RuntimeWarning, stacklevel=3)

    def laplace_logpdf(self, X, terms, jitter: float, lik, y, lik_param: float = 0.0, max_iter: int = 100,
                       tol: float = 1e-12, a0=None, full: bool = False):
        """log q(y | X), the Laplace approximation of the marginal likelihood of a latent GP with
        covariance K(X) + jitter I under the likelihood lik ("bernoulli", "poisson", "gaussian" or a
        LIK_* code; lik_param: the Gaussian's variance). full=True returns a LaplaceResult with
        .logq .f .a .iters .converged; a (= K^{-1} f at the mode) is a warm start a0 for a later call.
        A RuntimeWarning when the iteration did not converge within max_iter steps."""
        keep, N, _, args = self._laplace_args(X, terms, jitter, lik, y, lik_param, max_iter, tol, a0)
        logq = c_double()
        f = np.empty(N, dtype=np.float64)
        a = np.empty(N, dtype=np.float64)
        iters, conv, info = c_int32(), c_int32(), c_int64()
        rc = self.lib.gaplac_laplace_logpdf(*args, byref(logq), f.ctypes.data_as(c_void_p), a.ctypes.data_as(c_void_p),
                                            byref(iters), byref(conv), byref(info))
        self._check(rc)
        self._laplace_warn(bool(conv.value), iters.value)
        if full:
            return LaplaceResult(logq.value, f, a, iters.value, bool(conv.value))
        return logq.value

    def laplace_logpdf_grad(self, X, terms, jitter: float, lik, y, lik_param: float = 0.0, max_iter: int = 100,
                            tol: float = 1e-12, a0=None) -> LaplaceGradResult:
        """log q(y | X) of laplace_logpdf and its gradient in every term's parameter (l / c / a Noise
        term's variance; 0 for Cat) and in the jitter (gaplac_laplace_logpdf_grad): a
        LaplaceGradResult with .logq .dparam .djitter .implicit .f .a .iters .converged. For the
        Gaussian likelihood djitter is also the derivative in lik_param. A RuntimeWarning when the
        iteration did not converge: the gradient is then that of the last iterate, not the exact
        derivative of the reported log q."""
        keep, N, _, args = self._laplace_args(X, terms, jitter, lik, y, lik_param, max_iter, tol, a0)
        T = args[5]
        logq, dj = c_double(), c_double()
        f = np.empty(N, dtype=np.float64)
        a = np.empty(N, dtype=np.float64)
        dp = np.empty(max(1, T), dtype=np.float64)
        imp = np.empty(T + 1, dtype=np.float64)
        iters, conv, info = c_int32(), c_int32(), c_int64()
        rc = self.lib.gaplac_laplace_logpdf_grad(
            *args, byref(logq), f.ctypes.data_as(c_void_p), a.ctypes.data_as(c_void_p), byref(iters), byref(conv),
            byref(info), dp.ctypes.data_as(c_void_p), byref(dj), imp.ctypes.data_as(c_void_p))
        self._check(rc)
        self._laplace_warn(bool(conv.value), iters.value)
        return LaplaceGradResult(logq.value, f, a, iters.value, bool(conv.value), dp[:T].copy(), dj.value, imp)

    def laplace_posterior_mean_var(self, X, terms, jitter: float, lik, y, Xs, lik_param: float = 0.0,
                                   max_iter: int = 100, tol: float = 1e-12, a0=None, full: bool = False):
        """(mean, var) of the Laplace approximation's latent posterior at the rows of Xs; full=True
        returns (mean, var, logq, iters, converged)."""
        keep, N, D, args = self._laplace_args(X, terms, jitter, lik, y, lik_param, max_iter, tol, a0)
        Xsc = _colmajor(Xs)
        M = Xsc.shape[0]
        if Xsc.shape[1] != D:
            raise ArgumentError(f"test inputs have {Xsc.shape[1]} columns, training inputs {D}")
        logq = c_double()
        mean = np.empty(M, dtype=np.float64)
        var = np.empty(M, dtype=np.float64)
        iters, conv, info = c_int32(), c_int32(), c_int64()
        rc = self.lib.gaplac_laplace_posterior_mean_var(
            *args, M, Xsc.ctypes.data_as(c_void_p), max(M, 1), byref(logq), mean.ctypes.data_as(c_void_p),
            var.ctypes.data_as(c_void_p), byref(iters), byref(conv), byref(info))
        self._check(rc)
        self._laplace_warn(bool(conv.value), iters.value)
        if full:
            return mean, var, logq.value, iters.value, bool(conv.value)
        return mean, var

    def fit(self, X, terms, noise: float, y, cap: int = 1024) -> "Fit":
        """The posterior given y, factored once and kept on the device (gaplac_fit_create): a Fit
        whose queries skip the factorisation. cap: test points solved at once."""
        Xc = _colmajor(X)
        y = np.ascontiguousarray(y, dtype=np.float64)
        N, D = Xc.shape
        if y.ndim != 1 or y.shape[0] != N:
            raise ArgumentError(f"length of y ({y.shape[0] if y.ndim else 0}) != N ({N})")
        terms = list(terms)
        ta = term_array(terms)
        h = c_void_p()
        rc = self.lib.gaplac_fit_create(
            self.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), ta, float(noise),
            y.ctypes.data_as(c_void_p), int(cap), byref(h),
        )
        self._check(rc)
        return Fit(self, h, D, noise=float(noise))

    def laplace_fit(self, X, terms, jitter: float, lik, y, lik_param: float = 0.0, max_iter: int = 100,
                    tol: float = 1e-12, a0=None, cap: int = 1024) -> "Fit":
        """The latent posterior of the Laplace approximation, its mode found once and the factor of
        B kept on the device (gaplac_laplace_fit_create): a Fit of kind "laplace" whose queries cost
        the test rows' solve, not Newton steps or a factorisation. Arguments as laplace_logpdf; cap:
        test points solved at once. A RuntimeWarning when the iteration did not converge (the Fit
        then holds the last iterate)."""
        keep, N, D, args = self._laplace_args(X, terms, jitter, lik, y, lik_param, max_iter, tol, a0)
        h = c_void_p()
        iters, conv, info = c_int32(), c_int32(), c_int64()
        rc = self.lib.gaplac_laplace_fit_create(*args, int(cap), byref(h), byref(iters), byref(conv), byref(info))
        self._check(rc)
        self._laplace_warn(bool(conv.value), iters.value)
        return Fit(self, h, D)

    def posterior_components(self, X, terms, noise: float, y, Xs, comp, G=None):
        """(mean[M, G], var[M, G]): the posterior of every component of k = sum_g k_g at the
        rows of Xs, all from one factorisation (gaplac_posterior_components). comp[t] is the
        component of term t (-1: none; equal within a product group); G defaults to
        max(comp) + 1."""
        Xc = _colmajor(X)
        y = np.ascontiguousarray(y, dtype=np.float64)
        N, D = Xc.shape
        if y.shape[0] != N:
            raise ArgumentError(f"length of y ({y.shape[0]}) != N ({N})")
        Xsc = _colmajor(Xs)
        M = Xsc.shape[0]
        if Xsc.shape[1] != D:
            raise ArgumentError(f"test inputs have {Xsc.shape[1]} columns, training inputs {D}")
        terms = list(terms)
        comp = [int(c) for c in comp]
        if len(comp) != len(terms):
            raise ArgumentError(f"comp has {len(comp)} entries for {len(terms)} terms")
        if G is None:
            G = max(comp, default=-1) + 1
        G = int(G)
        ta = term_array(terms)
        ca = (c_int32 * max(1, len(comp)))(*comp)
        mean = np.empty((M, max(G, 0)), dtype=np.float64, order="F")
        var = np.empty((M, max(G, 0)), dtype=np.float64, order="F")
        rc = self.lib.gaplac_posterior_components(
            self.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), ta, float(noise),
            y.ctypes.data_as(c_void_p), M, Xsc.ctypes.data_as(c_void_p), max(M, 1), G, ca,
            mean.ctypes.data_as(c_void_p), max(M, 1), var.ctypes.data_as(c_void_p), max(M, 1),
        )
        self._check(rc)
        return mean, var

    def rand(self, X, terms, noise: float, z):
        """L z with C = K(X) + noise I = L L^T (gaplac_rand): one draw of the FiniteGP for the
        standard-normal vector z."""
        Xc = _colmajor(X)
        z = np.ascontiguousarray(z, dtype=np.float64)
        N, D = Xc.shape
        if z.shape[0] != N:
            raise ArgumentError(f"length of z ({z.shape[0]}) != N ({N})")
        terms = list(terms)
        ta = term_array(terms)
        out = np.empty(N, dtype=np.float64)
        rc = self.lib.gaplac_rand(self.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), ta,
                                  float(noise), z.ctypes.data_as(c_void_p), out.ctypes.data_as(c_void_p))
        self._check(rc)
        return out

    def _multi_outputs(self, R: int):
        lp = np.empty(max(R, 1), dtype=np.float64)
        q = np.empty(max(R, 1), dtype=np.float64)
        return lp, c_double(0.0), q

    def logpdf_multi(self, X, terms, noise: float, Y, full: bool = False):
        """logpdf of every column of Y (N x R) under the zero-mean FiniteGP, one factorisation
        (gaplac_logpdf_multi): an array of R, or (logpdf[R], logdet, quad[R]) with full=True."""
        Xc = _colmajor(X)
        Yc = np.asarray(Y, dtype=np.float64)
        if Yc.ndim != 2:
            raise ArgumentError(f"Y must be a matrix (N x R), got {Yc.ndim} dimension(s)")
        Yc = np.asfortranarray(Yc)
        N, D = Xc.shape
        if Yc.shape[0] != N:
            raise ArgumentError(f"rows of Y ({Yc.shape[0]}) != N ({N})")
        R = Yc.shape[1]
        terms = list(terms)
        ta = term_array(terms)
        lp, ld, q = self._multi_outputs(R)
        rc = self.lib.gaplac_logpdf_multi(
            self.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), ta, float(noise),
            R, Yc.ctypes.data_as(c_void_p), max(N, 1), lp.ctypes.data_as(c_void_p), byref(ld),
            q.ctypes.data_as(c_void_p),
        )
        self._check(rc)
        return (lp[:R], ld.value, q[:R]) if full else lp[:R]

    def logpdf_multi_device(self, N: int, D: int, dX_ptr: int, ldx: int, terms, noise: float, R: int, dY_ptr: int,
                            ldy: int, full: bool = False):
        """Device-resident X (N x D, ldx) and Y (N x R, ldy); the results are host arrays."""
        terms = list(terms)
        ta = term_array(terms)
        if R < 0:
            raise ArgumentError(f"R = {R} < 0")
        lp, ld, q = self._multi_outputs(R)
        rc = self.lib.gaplac_logpdf_multi_device(
            self.h, N, D, c_void_p(dX_ptr), ldx, len(terms), ta, float(noise), R, c_void_p(dY_ptr), ldy,
            lp.ctypes.data_as(c_void_p), byref(ld), q.ctypes.data_as(c_void_p),
        )
        self._check(rc)
        return (lp[:R], ld.value, q[:R]) if full else lp[:R]

    def rand_multi(self, X, terms, noise: float, Z):
        """L Z with C = K(X) + noise I = L L^T (gaplac_rand_multi): one draw of the FiniteGP per
        column of the standard-normal matrix Z (N x R). Returns N x R (column-major)."""
        Xc = _colmajor(X)
        Zc = np.asarray(Z, dtype=np.float64)
        if Zc.ndim != 2:
            raise ArgumentError(f"Z must be a matrix (N x R), got {Zc.ndim} dimension(s)")
        Zc = np.asfortranarray(Zc)
        N, D = Xc.shape
        if Zc.shape[0] != N:
            raise ArgumentError(f"rows of Z ({Zc.shape[0]}) != N ({N})")
        R = Zc.shape[1]
        terms = list(terms)
        ta = term_array(terms)
        out = np.empty((N, R), dtype=np.float64, order="F")
        buf = out if out.size else np.empty(1)  # (an empty result still passes a valid pointer)
        rc = self.lib.gaplac_rand_multi(
            self.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), ta, float(noise),
            R, Zc.ctypes.data_as(c_void_p), max(N, 1), buf.ctypes.data_as(c_void_p), max(N, 1),
        )
        self._check(rc)
        return out

    def _joint_head(self, X, terms, noise, y, Xs, noise_s):
        """The argument head the three joint posterior entries share (after self.h)."""
        Xc = _colmajor(X)
        y = np.ascontiguousarray(y, dtype=np.float64)
        N, D = Xc.shape
        if y.ndim != 1 or y.shape[0] != N:
            raise ArgumentError(f"length of y ({y.shape[0] if y.ndim else 0}) != N ({N})")
        Xsc = _colmajor(Xs)
        M = Xsc.shape[0]
        if Xsc.shape[1] != D:
            raise ArgumentError(f"test inputs have {Xsc.shape[1]} columns, training inputs {D}")
        terms = list(terms)
        ta = term_array(terms)
        head = (N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), ta, float(noise),
                y.ctypes.data_as(c_void_p), M, Xsc.ctypes.data_as(c_void_p), max(M, 1), float(noise_s))
        return head, (Xc, y, Xsc, ta), M

    def posterior_mean_cov(self, X, terms, noise: float, y, Xs, noise_s: float = 0.0):
        """(mean, cov) of the posterior of the zero-mean FiniteGP given y, jointly at the rows of
        Xs with observation variance noise_s there (gaplac_posterior_mean_cov): cov is the full
        symmetric M x M matrix."""
        head, keep, M = self._joint_head(X, terms, noise, y, Xs, noise_s)
        mean = np.empty(M, dtype=np.float64)
        cov = np.empty((M, M), dtype=np.float64, order="F")
        mb = mean if M else np.empty(1)  # (an empty result still passes valid pointers)
        cb = cov if M else np.empty(1)
        rc = self.lib.gaplac_posterior_mean_cov(self.h, *head, mb.ctypes.data_as(c_void_p),
                                                cb.ctypes.data_as(c_void_p), max(M, 1))
        self._check(rc)
        return mean, cov

    def posterior_rand(self, X, terms, noise: float, y, Xs, noise_s: float, Z):
        """m 1^T + L* Z (gaplac_posterior_rand): one joint posterior draw at the rows of Xs per
        column of the standard-normal matrix Z (M x R). Returns M x R (column-major)."""
        head, keep, M = self._joint_head(X, terms, noise, y, Xs, noise_s)
        Zc = np.asarray(Z, dtype=np.float64)
        if Zc.ndim != 2:
            raise ArgumentError(f"Z must be a matrix (M x R), got {Zc.ndim} dimension(s)")
        Zc = np.asfortranarray(Zc)
        if Zc.shape[0] != M:
            raise ArgumentError(f"rows of Z ({Zc.shape[0]}) != M ({M})")
        R = Zc.shape[1]
        out = np.empty((M, R), dtype=np.float64, order="F")
        buf = out if out.size else np.empty(1)
        rc = self.lib.gaplac_posterior_rand(self.h, *head, R, Zc.ctypes.data_as(c_void_p), max(M, 1),
                                            buf.ctypes.data_as(c_void_p), max(M, 1))
        self._check(rc)
        return out

    def posterior_logpdf(self, X, terms, noise: float, y, Xs, noise_s: float, Ys, full: bool = False):
        """logpdf of every column of Ys (M x R) under the joint posterior at the rows of Xs
        (gaplac_posterior_logpdf): an array of R, or (logpdf[R], logdet, quad[R]) with full=True."""
        head, keep, M = self._joint_head(X, terms, noise, y, Xs, noise_s)
        Yc = np.asarray(Ys, dtype=np.float64)
        if Yc.ndim != 2:
            raise ArgumentError(f"Ys must be a matrix (M x R), got {Yc.ndim} dimension(s)")
        Yc = np.asfortranarray(Yc)
        if Yc.shape[0] != M:
            raise ArgumentError(f"rows of Ys ({Yc.shape[0]}) != M ({M})")
        R = Yc.shape[1]
        lp, ld, q = self._multi_outputs(R)
        rc = self.lib.gaplac_posterior_logpdf(self.h, *head, R, Yc.ctypes.data_as(c_void_p), max(M, 1),
                                              lp.ctypes.data_as(c_void_p), byref(ld), q.ctypes.data_as(c_void_p))
        self._check(rc)
        return (lp[:R], ld.value, q[:R]) if full else lp[:R]

    def _sparse_head(self, X, terms, noise, y, Z, jitter):
        """The argument head the two sparse entries share (after self.h)."""
        Xc = _colmajor(X)
        y = np.ascontiguousarray(y, dtype=np.float64)
        N, D = Xc.shape
        if y.ndim != 1 or y.shape[0] != N:
            raise ArgumentError(f"length of y ({y.shape[0] if y.ndim else 0}) != N ({N})")
        Zc = _colmajor(Z)
        Mz = Zc.shape[0]
        if Zc.shape[1] != D:
            raise ArgumentError(f"inducing inputs have {Zc.shape[1]} columns, training inputs {D}")
        terms = list(terms)
        ta = term_array(terms)
        head = (N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), ta, float(noise),
                y.ctypes.data_as(c_void_p), Mz, Zc.ctypes.data_as(c_void_p), max(Mz, 1), float(jitter))
        return head, (Xc, y, Zc, ta), D

    def sparse_elbo(self, X, terms, noise: float, y, Z, jitter: float = 0.0, full: bool = False):
        """The evidence lower bound of the inducing-point (VFE) approximation with inducing inputs
        Z (gaplac_sparse_elbo); full=True returns the dict elbo, dtc, trace, logdet, quad."""
        head, keep, _ = self._sparse_head(X, terms, noise, y, Z, jitter)
        out = [c_double() for _ in range(5)]
        rc = self.lib.gaplac_sparse_elbo(self.h, *head, *(byref(o) for o in out))
        self._check(rc)
        names = ("elbo", "dtc", "trace", "logdet", "quad")
        return {k: o.value for k, o in zip(names, out)} if full else out[0].value

    def sparse_elbo_grad(self, X, terms, noise: float, y, Z, jitter: float = 0.0, wrt_z: bool = False):
        """(elbo, dy, dparam, dnoise, djitter): the bound and its gradient with respect to y, the
        term parameters, the observation variance and jitter (gaplac_sparse_elbo_grad). wrt_z=True
        appends dZ, the gradient with respect to the inducing inputs, an (Mz, D) array
        (gaplac_sparse_elbo_grad_z); the other five are bitwise the same either way."""
        head, keep, D = self._sparse_head(X, terms, noise, y, Z, jitter)
        N, T = head[0], head[4]
        elbo, dnoise, djitter = c_double(), c_double(), c_double()
        dy = np.empty(N, dtype=np.float64)
        dparam = np.empty(T, dtype=np.float64)
        yb = dy if N else np.empty(1)  # (an empty result still passes valid pointers)
        pb = dparam if T else np.empty(1)
        outs = (byref(elbo), yb.ctypes.data_as(c_void_p), pb.ctypes.data_as(c_void_p), byref(dnoise), byref(djitter))
        if wrt_z:
            Mz = head[8]
            dZ = np.empty((Mz, D), dtype=np.float64, order="F")
            zb = dZ if dZ.size else np.empty(1)
            rc = self.lib.gaplac_sparse_elbo_grad_z(self.h, *head, *outs, zb.ctypes.data_as(c_void_p), max(Mz, 1))
            self._check(rc)
            return elbo.value, dy, dparam, dnoise.value, djitter.value, dZ
        rc = self.lib.gaplac_sparse_elbo_grad(self.h, *head, *outs)
        self._check(rc)
        return elbo.value, dy, dparam, dnoise.value, djitter.value

    def sparse_posterior_mean_var(self, X, terms, noise: float, y, Z, jitter: float, Xs):
        """(mean, var) of the approximate posterior given y at the rows of Xs
        (gaplac_sparse_posterior_mean_var)."""
        head, keep, D = self._sparse_head(X, terms, noise, y, Z, jitter)
        Xsc = _colmajor(Xs)
        Ms = Xsc.shape[0]
        if Xsc.shape[1] != D:
            raise ArgumentError(f"test inputs have {Xsc.shape[1]} columns, training inputs {D}")
        mean = np.empty(Ms, dtype=np.float64)
        var = np.empty(Ms, dtype=np.float64)
        mb = mean if Ms else np.empty(1)  # (an empty result still passes valid pointers)
        vb = var if Ms else np.empty(1)
        rc = self.lib.gaplac_sparse_posterior_mean_var(self.h, *head, Ms, Xsc.ctypes.data_as(c_void_p), max(Ms, 1),
                                                       mb.ctypes.data_as(c_void_p), vb.ctypes.data_as(c_void_p))
        self._check(rc)
        return mean, var

    def _sparse_joint_head(self, X, terms, noise, y, Z, jitter, Xs, noise_s):
        """The argument head the three sparse joint entries share (after self.h)."""
        head, keep, D = self._sparse_head(X, terms, noise, y, Z, jitter)
        Xsc = _colmajor(Xs)
        Ms = Xsc.shape[0]
        if Xsc.shape[1] != D:
            raise ArgumentError(f"test inputs have {Xsc.shape[1]} columns, training inputs {D}")
        head = head + (Ms, Xsc.ctypes.data_as(c_void_p), max(Ms, 1), float(noise_s))
        return head, keep + (Xsc,), Ms

    def sparse_posterior_mean_cov(self, X, terms, noise: float, y, Z, jitter: float, Xs, noise_s: float = 0.0):
        """(mean, cov) of the approximate posterior given y, jointly at the rows of Xs with
        observation variance noise_s there (gaplac_sparse_posterior_mean_cov): cov is the full
        symmetric Ms x Ms matrix."""
        head, keep, Ms = self._sparse_joint_head(X, terms, noise, y, Z, jitter, Xs, noise_s)
        mean = np.empty(Ms, dtype=np.float64)
        cov = np.empty((Ms, Ms), dtype=np.float64, order="F")
        mb = mean if Ms else np.empty(1)  # (an empty result still passes valid pointers)
        cb = cov if Ms else np.empty(1)
        rc = self.lib.gaplac_sparse_posterior_mean_cov(self.h, *head, mb.ctypes.data_as(c_void_p),
                                                       cb.ctypes.data_as(c_void_p), max(Ms, 1))
        self._check(rc)
        return mean, cov

    def sparse_posterior_rand(self, X, terms, noise: float, y, Z, jitter: float, Xs, noise_s: float, E):
        """m 1^T + L* E (gaplac_sparse_posterior_rand): one joint draw of the approximate posterior
        at the rows of Xs per column of the standard-normal matrix E (Ms x R). Returns Ms x R
        (column-major)."""
        head, keep, Ms = self._sparse_joint_head(X, terms, noise, y, Z, jitter, Xs, noise_s)
        Ec = np.asarray(E, dtype=np.float64)
        if Ec.ndim != 2:
            raise ArgumentError(f"E must be a matrix (Ms x R), got {Ec.ndim} dimension(s)")
        Ec = np.asfortranarray(Ec)
        if Ec.shape[0] != Ms:
            raise ArgumentError(f"rows of E ({Ec.shape[0]}) != Ms ({Ms})")
        R = Ec.shape[1]
        out = np.empty((Ms, R), dtype=np.float64, order="F")
        buf = out if out.size else np.empty(1)
        rc = self.lib.gaplac_sparse_posterior_rand(self.h, *head, R, Ec.ctypes.data_as(c_void_p), max(Ms, 1),
                                                   buf.ctypes.data_as(c_void_p), max(Ms, 1))
        self._check(rc)
        return out

    def sparse_posterior_logpdf(self, X, terms, noise: float, y, Z, jitter: float, Xs, noise_s: float, Ys,
                                full: bool = False):
        """logpdf of every column of Ys (Ms x R) under the joint approximate posterior at the rows
        of Xs (gaplac_sparse_posterior_logpdf): an array of R, or (logpdf[R], logdet, quad[R]) with
        full=True."""
        head, keep, Ms = self._sparse_joint_head(X, terms, noise, y, Z, jitter, Xs, noise_s)
        Yc = np.asarray(Ys, dtype=np.float64)
        if Yc.ndim != 2:
            raise ArgumentError(f"Ys must be a matrix (Ms x R), got {Yc.ndim} dimension(s)")
        Yc = np.asfortranarray(Yc)
        if Yc.shape[0] != Ms:
            raise ArgumentError(f"rows of Ys ({Yc.shape[0]}) != Ms ({Ms})")
        R = Yc.shape[1]
        lp, ld, q = self._multi_outputs(R)
        rc = self.lib.gaplac_sparse_posterior_logpdf(self.h, *head, R, Yc.ctypes.data_as(c_void_p), max(Ms, 1),
                                                     lp.ctypes.data_as(c_void_p), byref(ld),
                                                     q.ctypes.data_as(c_void_p))
        self._check(rc)
        return (lp[:R], ld.value, q[:R]) if full else lp[:R]

    def sparse_split(self, N: int, Mz: int):
        """(chunks, chunk_rows) of the product over the N rows (gaplac_sparse_split)."""
        chunks, rows = c_int64(), c_int64()
        self._check(self.lib.gaplac_sparse_split(int(N), int(Mz), byref(chunks), byref(rows)))
        return chunks.value, rows.value

    def gram(self, X, terms, noise: float = 0.0) -> np.ndarray:
        Xc = _colmajor(X)
        N, D = Xc.shape
        out = np.empty((N, N), dtype=np.float64, order="F")
        terms = list(terms)
        ta = term_array(terms)
        rc = self.lib.gaplac_gram(self.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), ta,
                                  float(noise), out.ctypes.data_as(c_void_p), max(N, 1))
        self._check(rc)
        return out

    def gram_time(self, X, terms, noise: float, v, reps: int = 5):
        """(best_ms, bytes): one plain-grid Gram launch into the workspace, timed with
        hipEvents (best of reps), and its algorithmic HBM bytes (bench.py extra.gram)."""
        Xc = _colmajor(X)
        v = np.ascontiguousarray(v, dtype=np.float64)
        N, D = Xc.shape
        terms = list(terms)
        ta = term_array(terms)
        ms, nbytes = c_double(0.0), c_double(0.0)
        rc = self.lib.gaplac_gram_time(self.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), ta,
                                       float(noise), v.ctypes.data_as(c_void_p), int(reps), byref(ms), byref(nbytes))
        self._check(rc)
        return ms.value, nbytes.value

    def factor(self, X, terms, noise: float, v):
        """(L, z): lower Cholesky factor of C and z = L^{-1} v."""
        Xc = _colmajor(X)
        v = np.ascontiguousarray(v, dtype=np.float64)
        N, D = Xc.shape
        L = np.empty((N, N), dtype=np.float64, order="F")
        z = np.empty(N, dtype=np.float64)
        terms = list(terms)
        ta = term_array(terms)
        rc = self.lib.gaplac_factor(self.h, N, D, Xc.ctypes.data_as(c_void_p), max(N, 1), len(terms), ta,
                                    float(noise), v.ctypes.data_as(c_void_p), L.ctypes.data_as(c_void_p),
                                    max(N, 1), z.ctypes.data_as(c_void_p))
        self._check(rc)
        return L, z

    def set_profiling(self, mode):
        """0/False off, 1/True per-launch device timestamps, 2 hipEvents around the bulk
        trailing-update launches (production schedule)."""
        self.lib.gaplac_set_profiling(self.h, int(mode))

    def stats(self) -> dict:
        s = _native.Stats()
        self.lib.gaplac_get_stats(self.h, byref(s))
        return {name: getattr(s, name) for name, _ in _native.Stats._fields_}

    def reset_stats(self):
        self.lib.gaplac_reset_stats(self.h)


class Fit:
    """A fitted posterior (gaplac_fit): the factor, z and alpha = C^{-1} y kept on the device by
    Context.fit. Queries cost the test rows' solve (mean_var) or a matrix-free product (mean), not
    a factorisation. Free it with close() or a with-block; a Fit outlives neither its Context's
    close() (every query then raises ArgumentError) nor its own.

    kind "laplace" (Context.laplace_fit): the latent posterior of the Laplace approximation, the
    factor that of B, alpha = grad log p(y | f) at the mode; .logq (= .logpdf), .iters, .converged,
    .lik, .lik_param, .jitter and f_hat() besides."""

    def __init__(self, ctx: Context, h: c_void_p, D: int, noise: float | None = None):
        self.ctx = ctx
        self.lib = ctx.lib
        self.h = h
        self.D = D
        self.noise = noise
        n, cap = c_int64(), c_int64()
        lp, ld, q = c_double(), c_double(), c_double()
        self.lib.gaplac_fit_info(h, byref(n), byref(cap), byref(lp), byref(ld), byref(q))
        self.N, self.cap = n.value, cap.value
        self.logpdf, self.logdet, self.quad = lp.value, ld.value, q.value
        lik, it, cv = c_int32(), c_int32(), c_int32()
        lpar, jit = c_double(), c_double()
        if self.lib.gaplac_fit_laplace_info(h, byref(lik), byref(lpar), byref(jit), byref(it), byref(cv)) == 0:
            self.kind = "laplace"
            self.lik, self.lik_param, self.jitter = lik.value, lpar.value, jit.value
            self.logq, self.iters, self.converged = self.logpdf, it.value, bool(cv.value)
        else:
            self.kind = "exact"

    def close(self):
        if getattr(self, "h", None):
            self.lib.gaplac_fit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _handle(self):
        if not getattr(self, "h", None):
            raise ArgumentError("the fit is closed")
        return self.h

    def _check(self, rc: int):
        if rc < 0 and not self.ctx.h:
            raise ArgumentError(f"gaplac error {rc}: the fit's context is closed")
        self.ctx._check(rc)

    def _xs(self, Xs):
        Xsc = _colmajor(Xs)
        if Xsc.shape[1] != self.D:
            raise ArgumentError(f"test inputs have {Xsc.shape[1]} columns, training inputs {self.D}")
        return Xsc

    def alpha(self) -> np.ndarray:
        """alpha = C^{-1} y (gaplac_fit_alpha)."""
        h = self._handle()
        out = np.empty(self.N, dtype=np.float64)
        buf = out if self.N else np.empty(1)  # (an empty result still passes a valid pointer)
        self._check(self.lib.gaplac_fit_alpha(h, buf.ctypes.data_as(c_void_p)))
        return out

    def mean(self, Xs) -> np.ndarray:
        """Posterior mean at the rows of Xs, matrix-free (gaplac_fit_mean)."""
        h = self._handle()
        Xsc = self._xs(Xs)
        M = Xsc.shape[0]
        mean = np.empty(M, dtype=np.float64)
        mb = mean if M else np.empty(1)
        self._check(self.lib.gaplac_fit_mean(h, M, Xsc.ctypes.data_as(c_void_p), max(M, 1), mb.ctypes.data_as(c_void_p)))
        return mean

    def mean_var(self, Xs):
        """(mean, var) at the rows of Xs (gaplac_fit_mean_var): the arithmetic of
        Context.posterior_mean_var without its factorisation."""
        h = self._handle()
        Xsc = self._xs(Xs)
        M = Xsc.shape[0]
        mean = np.empty(M, dtype=np.float64)
        var = np.empty(M, dtype=np.float64)
        mb = mean if M else np.empty(1)
        vb = var if M else np.empty(1)
        self._check(self.lib.gaplac_fit_mean_var(h, M, Xsc.ctypes.data_as(c_void_p), max(M, 1),
                                                 mb.ctypes.data_as(c_void_p), vb.ctypes.data_as(c_void_p)))
        return mean, var

    def f_hat(self) -> np.ndarray:
        """The mode of a Laplace fit (gaplac_fit_mode); ArgumentError for an exact fit."""
        h = self._handle()
        out = np.empty(self.N, dtype=np.float64)
        buf = out if self.N else np.empty(1)
        self._check(self.lib.gaplac_fit_mode(h, buf.ctypes.data_as(c_void_p)))
        return out

    def mean_cov(self, Xs, noise_s: float = 0.0):
        """(mean, cov) jointly at the rows of Xs, at most cap of them (gaplac_fit_mean_cov): cov =
        K(xs) + noise_s I - V^T V, the full symmetric M x M matrix."""
        h = self._handle()
        Xsc = self._xs(Xs)
        M = Xsc.shape[0]
        mean = np.empty(M, dtype=np.float64)
        cov = np.empty((M, M), dtype=np.float64, order="F")
        mb = mean if M else np.empty(1)
        cb = cov if M else np.empty(1)
        self._check(self.lib.gaplac_fit_mean_cov(h, M, Xsc.ctypes.data_as(c_void_p), max(M, 1), float(noise_s),
                                                 mb.ctypes.data_as(c_void_p), cb.ctypes.data_as(c_void_p), max(M, 1)))
        return mean, cov

    def predict(self, Xs, ys=None, Q: int = 32):
        """Observation-space predictions at the rows of Xs: (ymean, yvar), and with ys the log
        predictive density of each ys[j] as a third array. mean_var, then laplace_predict under the
        fit's likelihood; an exact fit is the Gaussian case with lik_param = its noise."""
        mean, var = self.mean_var(Xs)
        if self.kind == "laplace":
            return laplace_predict(self.lik, mean, var, ys, self.lik_param, Q)
        if self.noise is None:
            raise ArgumentError("the fit does not know its observation variance")
        return laplace_predict(_native.LIK_GAUSSIAN, mean, var, ys, self.noise, Q)


def gauss_hermite(Q: int):
    """(nodes, weights) of the physicists' Gauss-Hermite rule of order Q (gaplac_gauss_hermite),
    nodes ascending. Host arithmetic: no device is needed."""
    lib = _native.load()
    x = np.empty(max(int(Q), 1), dtype=np.float64)
    w = np.empty(max(int(Q), 1), dtype=np.float64)
    rc = lib.gaplac_gauss_hermite(int(Q), x.ctypes.data_as(c_void_p), w.ctypes.data_as(c_void_p))
    if rc != 0:
        raise ArgumentError(f"gaplac error {rc}: Q = {Q} is outside [1, 64]")
    return x, w


def laplace_predict(lik, mean, var, ys=None, lik_param: float = 0.0, Q: int = 32):
    """Observation-space predictions from a latent (mean, var) under the likelihood lik
    (gaplac_laplace_predict): (ymean, yvar), and with ys also logp, the log predictive density of
    each ys[j], by Gauss-Hermite quadrature of order Q. Host arithmetic: no device is needed."""
    lib = _native.load()
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    var = np.ascontiguousarray(var, dtype=np.float64)
    if mean.ndim != 1 or var.shape != mean.shape:
        raise ArgumentError(f"mean {mean.shape} and var {var.shape} must be vectors of one length")
    M = mean.shape[0]
    if ys is not None:
        ys = np.ascontiguousarray(ys, dtype=np.float64)
        if ys.shape != mean.shape:
            raise ArgumentError(f"ys has shape {ys.shape}, expected {mean.shape}")
    ym, yv, lp = (np.empty(max(M, 1), dtype=np.float64) for _ in range(3))
    rc = lib.gaplac_laplace_predict(
        likelihood_code(lik), float(lik_param), M, mean.ctypes.data_as(c_void_p), var.ctypes.data_as(c_void_p),
        ys.ctypes.data_as(c_void_p) if ys is not None else None, int(Q), ym.ctypes.data_as(c_void_p),
        yv.ctypes.data_as(c_void_p), lp.ctypes.data_as(c_void_p) if ys is not None else None)
    if rc != 0:
        what = {_native.E_PARAM: "a ys outside the likelihood's support (or a negative Gaussian variance)",
                _native.E_KIND: "unknown likelihood", _native.E_ARG: "bad argument (Q outside [1, 64]?)"}
        raise ArgumentError(f"gaplac error {rc}: {what.get(rc, '')}")
    if ys is None:
        return ym[:M], yv[:M]
    return ym[:M], yv[:M], lp[:M]


_default_ctx: Context | None = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx
