"""Backward error of a Cholesky factor and of the solves with it: residuals, bounds, a model, inputs.

TEST INFRASTRUCTURE ONLY (numpy, CPU). The residuals L L^T - C, L z - v and C alpha - y are formed in
np.longdouble (64-bit significand: the product of two fp64 numbers is exact in it and a sum of N of
them is rounded N times at 2^-64, 2^-11 of what is measured); the bounds are functions of the
outputs L, z, alpha alone, with constants counted from the kernel code (no free tolerance, as in
tests/test_gpu_entrywise.py). u = 2^-53, gamma_n = n u / (1 - n u).

plain_bound: gamma_{N+1} |L||L^T| (Higham, Accuracy and Stability, Thm 10.3; gamma_{N+1} |L||z| for a
substitution, Thm 8.5). It holds for every order of summation and for fused multiply-adds, as long as
a pivot is a correctly rounded sqrt and a column is divided by it.

design_bound: what the HIP factorisation may reach by its design (gaplac_kernels.hip).

 1. Pivots and in-tile columns (dpanel_t, diag2_sweep_a / _b). With y = rsq(p) (relative error e0,
    |e0| <= 2^-23), t = fl(p y), e = fma(-t, y, 1), cc = fma(e, 3/8, 1/2):
        rd = fma(y e, cc, y)  for 1/sqrt(p),      d = fma(t e, cc, t)  for sqrt(p).
    The series (1 - e)^{-1/2} = 1 + e/2 + 3/8 e^2 + 5/16 e^3 ... is cut after e^2: 5/16 |e|^3 <= 2^-67.
    t's rounding moves e by at most u (absolutely: e is t y's distance from 1), that is the results
    by u/2; the products y e, t e and cc are rounded relative to a term below 2^-22; the last fma
    rounds once. So rd = p^{-1/2} (1 + h), d = p^{1/2} (1 + h'), |h|, |h'| <= 1.5 u + 2^-66 < 2 u:
    inside one ulp, but not the u of a correctly rounded sqrt. A diagonal entry so carries
    (1 + h')^2 where Thm 10.3 has (1 + delta)^2 (one more u), and a column entry l = fl(s rd) has
    l d = s (1 + theta_4) (rd against 1/d: 3 u, the product: u) where the division has
    (1 + delta) (three more u). The longest chain is row N's; with the riding row z (row N + 1,
    same arithmetic) the constant in front of |L||L^T| and |L||z| grows from gamma_{N+1} to
    gamma_{N+3}, and by one more (gamma_{N+4}, GAMMA_EXTRA = 3) for point 2's s0 + s1.

 2. Tile rows below the diagonal tile (trsm_subst_kernel_body, tail_trsm, tail_trsm_pipe; the riding
    rows go through the same code). For the 16 x 16 diagonal sub-block b, with D = the computed
    L_bb^{-1} (dinv_diag, diag2_dinv) and s = B_b - sum_{c<b} X_c L_bc^T,
        X_b = fl(s D^T).
    s: one rounding per earlier column (every update is an fma into an fp64 accumulator, MFMA or
       VALU, and what is stored between launches is the accumulator itself) and one for the two
       partial sums s0 + s1: c_ij = sum_{k<K} l_ik l_jk (1 + theta_{K+1}) + s_j (1 + theta_{K+1}), the
       usual form, K + 1 <= N. That is point 1's gamma_{N+4} |L||L^T| and no more.
    D: column j of D solves L_bb x = e_j by substitution, 15 terms at most, each a product and a
       subtraction (2 roundings where the compiler does not fuse them, dinv_diag; 1 in diag2_dinv's
       fma), then fl(x rd) with rd against 1/d as above (4 u): (L_bb + dL_j) D_j = e_j,
       |dL_j| <= gamma_34 |L_bb|, so L_bb D = I + F with |F| <= gamma_34 |L_bb||D|.
    s D^T: four chained MFMAs of four terms, a 16-term sum however it is ordered:
       X_b = s D^T + e1, |e1| <= gamma_16 |s||D^T|.
    Together X_b L_bb^T = s (I + F)^T + e1 L_bb^T, so r = X_b L_bb^T - s obeys
        |r| <= (gamma_34 + gamma_16) |s| |D^T| |L_bb^T|,    to first order  |s| <= |X_b| |L_bb^T|,
    r = 0 for plain substitution. (gamma_34 + gamma_16) / gamma_16 = 3.125. The bound is evaluated
    with the exact inverse of the returned L_bb (inverted here in long double) in place of D and with
    |X_b||L_bb^T| in place of |s|: |D| <= |L_bb^{-1}| (1 + w) and |s| <= |X_b||L_bb^T| (1 + w) / (1 - w)
    with w = gamma_50 max_b || |L_bb^{-1}||L_bb| ||_inf, which design_terms() requires to be at most
    0.05 (a 16 x 16 sub-block of condition 1e13 would break it; the designed inputs reach 1e5):
    3.125 * 1.05^2 / 0.95 < 4 =: C_SUB. So, for row i below sub-block b and the columns J of b,
        |L L^T - C|[i, J] <= gamma_{N+4} (|L||L^T|)[i, J] + C_SUB gamma_16 (|X_b| T_b^T)[i],
        T_b = |L_bb| |L_bb^{-1}| |L_bb|,
    mirrored for the upper triangle, and for a solve L z = v,
        |L z - v|[J] <= gamma_{N+4} (|L||z|)[J] + C_SUB gamma_16 T_b |z_J|.
    The term is applied to every row below sub-block b, the rows of the same 128-tile included (they
    are swept by plain substitution in the diagonal kernels and need none of it): a superset, and
    what substitution_model, whose every panel is 16 wide, needs.

substitution_model is the numpy model of point 2: a right-looking Cholesky, 16 columns at a time,
whose panel is B @ inv(L_bb).T; it lets the CPU suite show that the plain check fails where the
design predicts and that the design check holds.

ld_logpdf and ld_logpdf_grad are the long-double references of the forward checks (logpdf; alpha,
dparam, dnoise), lapack_grad is fp64 LAPACK's gradient on a given C (the yardstick), and
alpha_forward_bound carries the design bounds forward into the gradient's alpha = Y z.
"""
import warnings

import numpy as np
import scipy.linalg

from oracle import restatement as R

SQEXP, OU, LINEAR, CAT, NOISE = 1, 2, 3, 4, 5
LD = np.longdouble
HAVE_LD = bool(np.finfo(LD).eps <= 2.0 ** -63)
if not HAVE_LD:
    warnings.warn("tests.backward_error: np.longdouble has no 64-bit significand on this platform; the "
                  "residuals are formed with mpmath (tests/hp_oracle.py) on a subset of rows only")
U = 2.0 ** -53
DB = 16            # the diagonal sub-block of the substitution
C_SUB = 4.0        # point 2
GAMMA_EXTRA = 3    # point 1: gamma_{N+1} -> gamma_{N+1+GAMMA_EXTRA}
FIXED_ROWS = (0, 15, 16, 127, 128, 129, 1023, 1024)


def gamma(n):
    return n * U / (1.0 - n * U)


def subset_rows(N, extra=54, seed=0):
    """The rows of a partial residual: FIXED_ROWS (below N), N-2, N-1 and `extra` seeded random rows."""
    rows = {r for r in FIXED_ROWS if r < N} | {max(N - 2, 0), N - 1}
    rng = np.random.default_rng(seed + N)
    rows |= set(int(r) for r in rng.choice(N, size=min(extra, N), replace=False))
    return np.array(sorted(rows))


# ------------------------------------------------------------------------------------------- products
def _mp_rows_times(Lr, Rt, sub):
    """(Lr @ Rt - sub) with 50-digit arithmetic, as fp64 (the fallback without a long double)."""
    from tests import hp_oracle as H
    out = np.empty((Lr.shape[0], Rt.shape[1]))
    for i in range(Lr.shape[0]):
        nz = np.nonzero(Lr[i])[0]
        for j in range(Rt.shape[1]):
            out[i, j] = float(H.MP.fsum(H.mpf(float(Lr[i, k])) * H.mpf(float(Rt[k, j])) for k in nz)
                              - H.mpf(float(sub[i, j])))
    return out


def _rows_times(Lr, Rt, sub):
    """Lr @ Rt - sub, the product and the difference in long double, rounded to fp64 at the end."""
    if not HAVE_LD:
        return _mp_rows_times(Lr, Rt, sub)
    return np.asarray(Lr.astype(LD) @ Rt.astype(LD) - sub.astype(LD), dtype=np.float64)


def factor_residual(L, C, rows=None):
    """(E, A) = (|L L^T - C|, |L||L^T|), all rows or the given ones (O(|rows| N^2)). Without a long
    double a complete residual is refused: pass rows (subset_rows)."""
    N = L.shape[0]
    if rows is None and not HAVE_LD:
        raise RuntimeError("no 64-bit-significand long double here: factor_residual needs rows=")
    if rows is None:
        E = np.empty((N, N))
        for r0 in range(0, N, 128):                      # L is lower triangular: row block r0 needs
            r1 = min(r0 + 128, N)                        # the first r1 columns only
            E[r0:r1] = np.abs(_rows_times(L[r0:r1, :r1], L[:, :r1].T, C[r0:r1]))
        A = np.abs(L) @ np.abs(L).T
    else:
        rows = np.asarray(rows)
        E = np.abs(_rows_times(L[rows], L.T, C[rows]))
        A = np.abs(L[rows]) @ np.abs(L).T
    return E, A


def solve_residual(L, z, v):
    """(|L z - v|, |L||z|)."""
    e = np.abs(_rows_times(L, z[:, None], v[:, None]))[:, 0]
    return e, np.abs(L) @ np.abs(z)


def spd_solve_residual(C, alpha, y, L):
    """(|C alpha - y|, |L||L^T||alpha|)."""
    e = np.abs(_rows_times(C, alpha[:, None], y[:, None]))[:, 0]
    return e, np.abs(L) @ (np.abs(L).T @ np.abs(alpha))


# --------------------------------------------------------------------------------------------- bounds
def plain_bound(A, N):
    return gamma(N + 1) * A


def _tri_inverse_ld(T):
    """Inverse of a lower triangular block by substitution in long double (mpmath without one)."""
    n = T.shape[0]
    if not HAVE_LD:
        from tests import hp_oracle as H
        Ti = H.MP.inverse(H.MP.matrix(T.tolist()))
        return np.array([[float(Ti[i, j]) for j in range(n)] for i in range(n)])
    return np.asarray(_tri_inverse_long(T.astype(LD)), dtype=np.float64)


def _tri_inverse_long(Tl):
    """The same inverse of a long-double lower triangular matrix, kept in long double."""
    n = Tl.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        rhs = -(Tl[i, :i] @ X[:i])
        rhs[i] += 1
        X[i] = rhs / Tl[i, i]
    return X


def design_terms(L, nb=DB):
    """[(j0, j1, T_b)] for the diagonal sub-blocks of L, T_b = |L_bb||L_bb^{-1}||L_bb|; raises where the
    first-order form of the bound does not hold (module docstring, w <= 0.05)."""
    out = []
    for j0 in range(0, L.shape[0], nb):
        j1 = min(j0 + nb, L.shape[0])
        Lb = np.abs(L[j0:j1, j0:j1])
        Li = np.abs(_tri_inverse_ld(L[j0:j1, j0:j1]))
        w = gamma(50) * np.max(np.sum(Li @ Lb, axis=1))
        if not w <= 0.05:
            raise ArithmeticError(f"sub-block at {j0}: gamma_50 |||L^-1||L||| = {w:.3g} > 0.05")
        out.append((j0, j1, Lb @ Li @ Lb))
    return out


def substitution_term(L, nb=DB):
    """S (N x N, symmetric): S[i, J_b] = (|L[i, J_b]| T_b^T) for the rows i below sub-block b."""
    N = L.shape[0]
    S = np.zeros((N, N))
    for j0, j1, T in design_terms(L, nb):
        S[j1:, j0:j1] = np.abs(L[j1:, j0:j1]) @ T.T
    return S + S.T


def design_bound(L, A, rows=None):
    """Bound of |L L^T - C| (all rows, or the given rows of it; A from factor_residual alike)."""
    N = L.shape[0]
    S = substitution_term(L)
    return gamma(N + 1 + GAMMA_EXTRA) * A + C_SUB * gamma(DB) * (S if rows is None else S[np.asarray(rows)])


def design_bound_solve(L, z, Az):
    """Bound of |L z - v| for the riding row (Az = |L||z| from solve_residual)."""
    N = L.shape[0]
    s = np.zeros(N)
    for j0, j1, T in design_terms(L):
        s[j0:j1] = T @ np.abs(z[j0:j1])
    return gamma(N + 1 + GAMMA_EXTRA) * Az + C_SUB * gamma(DB) * s


def design_bound_alpha(L, alpha):
    """Bound of |C alpha - y| for alpha = L^{-T} (L^{-1} y) (Higham Thm 10.4 with the additions above).
    With C = L L^T + dC, (L + dL1) z = y by the riding row and (L^T + dL2) alpha = z by plain
    back-substitution (fit_backsub_*: x = b fl(1 / l_ii), gamma_{N+2} |L^T|):
        C alpha - y = dC alpha - dL1 z - L dL2 alpha,    |z| <= (1 + gamma_{N+2}) |L^T||alpha|,
    so three plain terms (gamma_{N+4}, gamma_{N+4}, gamma_{N+2}; 3N + 13 covers them and the factor on
    |z|) and the substitution term twice: the factor's, S |alpha|, and the forward solve's,
    T |L^T||alpha| blockwise. The back-substitution has none."""
    N = L.shape[0]
    w = np.abs(L).T @ np.abs(alpha)
    s = np.zeros(N)
    for j0, j1, T in design_terms(L):
        s[j0:j1] = T @ w[j0:j1]
    return gamma(3 * N + 13) * (np.abs(L) @ w) + C_SUB * gamma(DB) * (substitution_term(L) @ np.abs(alpha) + s)


def mean_bound(L, z, alpha, noise, rows):
    """Bound of |mean_j - ((C - noise I) alpha)_j|, j in rows, for the posterior mean at the training
    points themselves, mean_j = fl(w_j . z) with w_j the riding row (L + dL_j) w_j = k_j, apart from
    the entries' own error |k_j - (C_j - noise e_j)| |alpha| (the caller adds it: the cross-covariance
    row k_j is computed apart from C, by other code). With z = (L^T + dL2) alpha (back-substitution,
    gamma_{N+2} |L^T|):
        w_j . z = (L w_j) . alpha + w_j . dL2 alpha = (k_j - dL_j w_j) . alpha + w_j . dL2 alpha,
    so
        |mean_j - k_j . alpha| <= gamma_{N+4} |w_j| . |z|                 the product (post_partial_kernel:
                                                                         a product and a sum per term on two
                                                                         accumulators of N / 2 terms, then
                                                                         the chunks: N + 4 roundings at most)
                                + (gamma_{N+4} |L||w_j| + C_SUB gamma_16 T |w_j|) . |alpha|     the riding row
                                + gamma_{N+2} |w_j| . |L^T||alpha|                              alpha's solve.
    w_j is not an output; to first order w_j = L^-1 (C_j - noise e_j) = L_j^T - noise L^-1 e_j, and the
    bound takes |w_j| <= (|L_j^T| + noise |L^-1 e_j|) (1 + 1e-6): the rest, L^-1 applied to the
    residual row of the factor and to the entries' error, is below 1e-9 of it on the designed inputs."""
    N = L.shape[0]
    Li = np.abs(scipy.linalg.solve_triangular(L, np.eye(N), lower=True, check_finite=False))
    la = np.abs(L).T @ np.abs(alpha)
    blocks = design_terms(L)
    out = np.empty(len(rows))
    for n, j in enumerate(rows):
        w = (np.abs(L[j]) + noise * Li[:, j]) * (1.0 + 1e-6)
        s = np.zeros(N)
        for j0, j1, T in blocks:
            s[j0:j1] = T @ w[j0:j1]
        out[n] = (gamma(N + 4) * (w @ np.abs(z)) + (gamma(N + 4) * (np.abs(L) @ w) + C_SUB * gamma(DB) * s) @ np.abs(alpha)
                  + gamma(N + 2) * (w @ la))
    return out


def mean_residual(C, alpha, noise, mean, rows):
    """|(C alpha)_j - noise alpha_j - mean_j| for j in rows, formed in long double."""
    sub = LD(noise) * alpha[rows].astype(LD) + mean[rows].astype(LD)
    return np.abs(_rows_times(C[rows], alpha[:, None], sub[:, None]))[:, 0]


def entry_error_term(X, term, alpha, rows, constants):
    """sum_i (B'(x_j, x_i) + B''(x_j, x_i)) |alpha_i| for j in rows: how far two implementations of the
    entries of one SqExp or OU term, each within hp_oracle.entry_bound with its own (c_e, c_u) of
    `constants`, can move a product with alpha."""
    from tests import hp_oracle as H
    kind, col, param, _ = term
    out = np.empty(len(rows))
    for n, j in enumerate(rows):
        tot = H.mpf(0)
        for i in range(X.shape[0]):
            b = sum(H.entry_bound(kind, param, X[j, col], X[i, col], c_e, c_u)[0] for c_e, c_u in constants)
            tot += b * abs(H.mpf(float(alpha[i])))
        out[n] = float(tot)
    return out


def worst_ratio(E, B):
    """max E / B (0 / 0 counts as 0, x / 0 as inf)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(E == 0.0, 0.0, E / B)
    return float(np.max(r))


# ---------------------------------------------------------------------------------------------- model
def _tri_inverse(T):
    """The explicit inverse as the kernels form it: L x = e_j by substitution, column by column, in
    fp64. It is exactly lower triangular; a general inverse (LU with pivoting) leaves rounding noise
    above the diagonal, which multiplies the large entries of a row of B into its small ones."""
    return scipy.linalg.solve_triangular(T, np.eye(T.shape[0]), lower=True, check_finite=False)


def substitution_model(C, nb=DB):
    """Right-looking Cholesky, nb columns at a time, the panel by the explicit inverse of L_bb."""
    N = C.shape[0]
    A = np.array(C, dtype=np.float64)
    L = np.zeros((N, N))
    for k in range(0, N, nb):
        e = min(k + nb, N)
        Lkk = np.linalg.cholesky(A[k:e, k:e])
        L[k:e, k:e] = Lkk
        if e < N:
            X = A[e:, k:e] @ _tri_inverse(Lkk).T
            L[e:, k:e] = X
            A[e:, e:] -= X @ X.T
    return L


def substitution_model_solve(L, v, nb=DB):
    """z = L^{-1} v the same way: z_b = inv(L_bb) (v_b - sum_{c<b} L_bc z_c)."""
    N = L.shape[0]
    z = np.zeros(N)
    for k in range(0, N, nb):
        e = min(k + nb, N)
        z[k:e] = _tri_inverse(L[k:e, k:e]) @ (v[k:e] - L[k:e, :k] @ z[:k])
    return z


# ------------------------------------------------------------------------- long-double reference logpdf
LOG2PI = LD(1.8378770664093454835606594728112352797227949472755668)


def ld_cholesky(C):
    """Lower Cholesky factor in long double (left-looking, one matrix-vector product per column)."""
    if not HAVE_LD:
        raise RuntimeError("no 64-bit-significand long double here")
    N = C.shape[0]
    Cl = C.astype(LD)
    L = np.zeros((N, N), dtype=LD)
    for j in range(N):
        col = Cl[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0:
            raise np.linalg.LinAlgError(f"pivot {j + 1} is not positive")
        d = np.sqrt(col[0])
        L[j, j] = d
        L[j + 1:, j] = col[1:] / d
    return L


SLICE_BITS, SLICES = 20, 5


def _slices(X):
    """The rows of X (long double) as SLICES fp64 matrices that add up to X within 2^-100 of each row's
    largest entry; a slice's entries are multiples of its row's grid with at most SLICE_BITS + 1
    bits, so the fp64 product of two slices over fewer than 2^11 columns is exact (Ozaki's scheme)."""
    X = np.array(X, dtype=LD)
    mx = np.max(np.abs(X), axis=1)
    e = np.ceil(np.log2(np.where(mx > 0, mx, LD(1)))).astype(np.int64)
    out = []
    for p in range(SLICES):
        g = np.ldexp(LD(1), e - SLICE_BITS * (p + 1))[:, None]
        s = np.rint(X / g) * g
        out.append(np.asarray(s, dtype=np.float64))
        X -= s
    return out


def _exact_residual(T, Sa, Sb):
    """T - A B^T for A, B given by their slices: the slice products are exact in fp64 and are taken
    off T in long double, the largest first, so that the roundings are relative to what is left."""
    assert Sa[0].shape[1] < 2 ** (52 - 2 * SLICE_BITS - 1)
    acc = np.array(T, dtype=LD)
    for t in range(SLICES):
        for p in range(t + 1):
            acc -= Sa[p] @ Sb[t - p].T
    return acc


def ld_logpdf(C, v, refine=True):
    """(logpdf, logdet, quad) of N(v | 0, C) as long doubles: a long-double factorisation M = L L^T,
    and (refine) its own backward error taken out to first order. The factor stored in long double
    leaves R = C - M of 2^-64 |L||L^T|, which cond(C) multiplies into logdet and quad: about 2^-11 of
    what fp64 LAPACK loses. With R formed exactly (_exact_residual),
        logdet C = logdet M + tr(M^-1 R) + O(|M^-1 R|^2),
        quad = a^T (2 v - C a) + (a - C^-1 v)^T C (a - C^-1 v)  for any a, here a = M^-1 v,
    and what is dropped is of second order in cond(C) N 2^-64."""
    L = ld_cholesky(C)
    N = C.shape[0]
    vl = v.astype(LD)
    Li = _tri_inverse_long(L)                         # L^-1, row by row
    z = Li @ vl
    logdet = 2 * np.sum(np.log(np.diag(L)))
    quad = z @ z
    if refine:
        S = _slices(L)
        Rm = _exact_residual(C, S, S)
        logdet = logdet + np.sum((Li @ Rm) * Li)      # tr(L^-1 R L^-T)
        a = Li.T @ z
        Sa = _slices(a[None, :])
        rho = _exact_residual(vl[:, None], _slices(C), Sa)[:, 0]            # v - C a
        av = -_exact_residual(np.zeros((1, 1)), Sa, _slices(vl[None, :]))[0, 0]
        quad = av + a @ rho
    return -(N * LOG2PI + logdet + quad) / 2, logdet, quad


# ----------------------------------------------------------------------- long-double reference gradient
def grad_derivatives(X, terms):
    """[dC/dparam_t] in fp64, as oracle.restatement.logpdf_grad forms them: term_derivative times the
    other terms of the product group."""
    terms = list(terms)
    out = []
    for t, (kind, col, param, group) in enumerate(terms):
        dK = R.term_derivative(X, kind, col, param)
        for s, (k2, c2, p2, g2) in enumerate(terms):
            if s != t and g2 == group:
                dK = dK * R.term_matrix(X, k2, c2, p2)
        out.append(dK)
    return out


def ld_logpdf_grad(C, X, terms, v, with_scale=False):
    """(alpha, dparam, dnoise) of log N(v | 0, C) in long double, C the fp64 covariance of the formula
    `terms` on the rows of X (dv = -alpha):
        alpha = C^-1 v,   dparam_t = 1/2 sum_ij (alpha_i alpha_j - C^-1_ij) dC_ij,   dnoise = 1/2 tr(...),
    with C^-1 = L^-T L^-1 from ld_cholesky and _tri_inverse_long, every product and sum in long double,
    and dC = grad_derivatives (fp64 data, taken as exact). The solve for alpha is refined to first
    order as in ld_logpdf: alpha += M^-1 (v - C alpha) with the residual formed exactly. What the
    stored factor leaves in C^-1 is cond(C) N 2^-64 of it, 2^-11 of what fp64 LAPACK loses.
    with_scale: also the magnitudes 1/2 sum (|alpha_i alpha_j| + |C^-1_ij|) |dC_ij| per parameter and
    1/2 sum_i (alpha_i^2 + |C^-1_ii|) for the noise (oracle.restatement.logpdf_grad_scale's), and
    |C^-1| (for alpha_forward_bound), as fp64."""
    L = ld_cholesky(C)
    vl = v.astype(LD)
    Li = _tri_inverse_long(L)
    alpha = Li.T @ (Li @ vl)
    rho = _exact_residual(vl[:, None], _slices(C), _slices(alpha[None, :]))[:, 0]          # v - C alpha
    alpha = alpha + Li.T @ (Li @ rho)
    Cinv = Li.T @ Li
    W = np.outer(alpha, alpha) - Cinv
    dCs = grad_derivatives(X, terms)
    half = LD(1) / 2
    dparam = np.array([half * np.sum(W * dC.astype(LD)) for dC in dCs], dtype=LD)
    dnoise = half * np.sum(np.diag(W))
    if not with_scale:
        return alpha, dparam, dnoise
    A = np.abs(np.outer(alpha, alpha)) + np.abs(Cinv)
    scale = np.array([float(half * np.sum(A * np.abs(dC).astype(LD))) for dC in dCs])
    return alpha, dparam, dnoise, scale, float(half * np.sum(np.diag(A))), np.asarray(np.abs(Cinv), dtype=np.float64)


def alpha_forward_bound(L, z, alpha, Cinv_abs):
    """Entrywise bound of |alpha_hat - C^-1 v| for the gradient's alpha_hat = fl(Y z) (alpha_partial_kernel),
    Y the identity rows carried through the factorisation (Y = L^-T), from the design bounds above, to
    first order. With L L^T = C + E, L z = v + e and a = L^-T z:  C a = v + e - E a, so
        a - C^-1 v = C^-1 (e - E a),      |E| <= design_bound,  |e| <= design_bound_solve.
    Row i of Y goes through the riding row's arithmetic with the right-hand side e_i (trsm_rows: the
    16 x 16 explicit inverses, point 2): L y_i^T = e_i + r_i with design_bound_solve's form, so
    Y = (I + R) L^-T,  |R|[i, J_b] <= gamma_{N+4} (|Y||L^T|)[i, J_b] + C_SUB gamma_16 T_b |y_i[J_b]|.
    The product is a sum of N terms however it is grouped (four accumulators per 512 columns, then
    the chunks): alpha_hat = Y z + d, |d| <= gamma_{N+4} |Y||z|. Together
        |alpha_hat - C^-1 v| <= |C^-1| (|e| + |E||a|) + |R||a| + gamma_{N+4} |Y||z|,
    evaluated with alpha_hat for a and the inverse of the returned L for Y, times 1.01 for what first
    order drops (cond(C) gamma_N of it: below 1e-3 on the designed inputs). The first term is the
    forward error any Cholesky solve is allowed (LAPACK's has gamma_{N+1} |L||L^T| for |E|); the factor's
    substitution term inside design_bound is what the explicit inverses add to it."""
    N = L.shape[0]
    a = np.abs(alpha)
    Labs = np.abs(L)
    E = design_bound(L, Labs @ Labs.T)
    e = design_bound_solve(L, z, Labs @ np.abs(z))
    Y = np.abs(_tri_inverse(L)).T
    Ra = gamma(N + 1 + GAMMA_EXTRA) * (Y @ (Labs.T @ a))
    for j0, j1, T in design_terms(L):
        Ra += C_SUB * gamma(DB) * (Y[:, j0:j1] @ (T.T @ a[j0:j1]))
    return 1.01 * (Cinv_abs @ (e + E @ a) + Ra + gamma(N + 1 + GAMMA_EXTRA) * (Y @ np.abs(z)))


def lapack_grad(C, X, terms, v):
    """(alpha, dparam, dnoise) in fp64 with oracle.restatement.logpdf_grad_potri's arithmetic (dpotrf,
    cho_solve, dpotri, vdot) on a given C. Raises numpy.linalg.LinAlgError where dpotrf finds C not
    positive definite."""
    from scipy.linalg import lapack
    U, info = lapack.dpotrf(C, lower=0, clean=1, overwrite_a=0)
    if info:
        raise np.linalg.LinAlgError(f"dpotrf info = {info}")
    alpha = scipy.linalg.cho_solve((U, False), v, check_finite=False)
    Cinv, info = lapack.dpotri(U, lower=0, overwrite_c=1)
    Cinv = np.triu(Cinv) + np.triu(Cinv, 1).T
    W = np.outer(alpha, alpha)
    W -= Cinv
    dparam = np.array([0.5 * float(np.vdot(W, dK)) for dK in grad_derivatives(X, terms)])
    return alpha, dparam, 0.5 * float(np.trace(W))


# --------------------------------------------------------------------------------------------- inputs
NOISES = (0.1, 1e-4, 1e-6, 1e-8)
SIZES = (129, 300, 700)
COMPOSITE = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 1), (CAT, 1, 0.0, 2), (NOISE, -1, 1.0, 3)]   # test_gpu_parity's


def design_points(name, N):
    """(X, terms) of one design at size N. X has two columns (the second: categories, for composite)."""
    rng = np.random.default_rng([N, sum(name.encode())])
    cats = rng.integers(0, max(1, N // 4), N).astype(float)
    if name == "unif":
        x, terms = rng.uniform(0, 10, N), [(SQEXP, 0, 1.5, 0)]
    elif name == "sorted":
        x, terms = np.sort(rng.uniform(0, 10, N)), [(SQEXP, 0, 1.5, 0)]
    elif name == "dates":
        x, terms = 2.4e6 + rng.integers(0, 400, N).astype(float), [(SQEXP, 0, 30.0, 0)]
    elif name == "ou":
        x, terms = rng.uniform(0, 10, N), [(OU, 0, 0.7, 0)]
    elif name == "composite":
        x, terms = rng.uniform(-5, 5, N), list(COMPOSITE)
    else:
        raise KeyError(name)
    return np.column_stack([x, cats]), terms


DESIGNS = ("unif", "sorted", "dates", "ou", "composite")


def model_draw(C, seed):
    """chol(C) @ randn: a draw from the model, so that quad is O(N) as for real data."""
    return np.linalg.cholesky(C) @ np.random.default_rng(seed).standard_normal(C.shape[0])


def designed_input(name, noise, N):
    X, terms = design_points(name, N)
    v = model_draw(R.gram(X, terms, noise), N + 1)
    return X, terms, noise, v


def input_ids(sizes=SIZES, noises=NOISES):
    return [(name, noise, N) for name in DESIGNS for noise in noises for N in sizes]


def input_name(key):
    name, noise, N = key
    return f"{name}-{noise:g}-{N}"


def designed_inputs(sizes=SIZES, noises=NOISES):
    """{name: (X, terms, noise, v)} of every design x noise x size."""
    return {input_name(k): designed_input(*k) for k in input_ids(sizes, noises)}
