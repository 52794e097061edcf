"""A plain 50-digit restatement of one covariance entry, and of the small dense formulas built on it.

TEST INFRASTRUCTURE ONLY (mpmath, CPU). Everything here is an exact real function of the fp64
inputs, evaluated at 50 significant digits; nothing is tuned to any implementation.

One entry. For SqExp and OU with lengthscale l the fp64 number s = fl(1/l) is taken as given (every
implementation, the reference's ScaleTransform included, starts from it), and then, in exact
arithmetic,

    u = x s,   d = u_i - u_j,   a = -d^2/2 (SqExp)  or  -|d| (OU),   k = exp(a)
    dk/dl  = k d^2 s (SqExp),  k |d| s (OU)         (the derivative in l, with 1/l read as s)
    dk/dxj = k d s   (SqExp),  k sign(d) s (OU)     (sign(0) = 0)
    Linear: k = x_i x_j + c,  dk/dc = 1,  dk/dxj = x_i
    Cat:    k = 0 if |x_i - x_j| > 0 else 1  (the reference's rule kappa(d2) = d2 > 0 ? 0.0 : 1.0:
            a NaN category has covariance 1 with everything, itself included); derivatives 0

Non-finite inputs follow IEEE rules (inf - inf = NaN, 0 inf = NaN, exp(-inf) = 0, NaN propagates).

entry_bound() is the rounding error an fp64 implementation of the reference's recipe (round u, round
d, round the argument, one exp, round each further product) may reach, with eps = 2^-53:

    B_k = k eps (c_e + |a|) + k |da/dd| eps c_u (|u_i| + |u_j|) + 2^-1075

the first term the exp's own error (c_e) and the roundings of d and of the argument (relative to |a|),
the second the roundings of the two scaled coordinates carried through a(d), the last half a
subnormal step. A derivative g = k m(d) s (m = d^2, |d|, d or sign d) has the analogous

    B_g = |g| eps (c_e + |a| + n_g) + |dg/dd| eps c_u (|u_i| + |u_j|) + 2^-1075 (1 + s + |m| s)

with n_g the roundings after the exp that the value itself does not have: the products forming g
(2 for m = sign d, 3 otherwise, m's own rounding counted) and 1 for reading 1/l as s where an
implementation divides by l. tests/test_hp_oracle.py pins that oracle.restatement stays inside
both with c_e = c_u = 1.
"""
import mpmath

SQEXP, OU, LINEAR, CAT, NOISE = 1, 2, 3, 4, 5

MP = mpmath.mp.clone()
MP.dps = 50
mpf = MP.mpf
EPS = mpf(2) ** -53
FLOOR = mpf(2) ** -1075
LOG2PI = MP.log(2 * MP.pi)


def _m(x):
    """An fp64 input as an exact 50-digit number (a 50-digit number stays: mpmath.diff's steps)."""
    return x if isinstance(x, MP.mpf) else mpf(float(x))


def _sign(d):
    return mpf(1) if d > 0 else (mpf(-1) if d < 0 else mpf(0))


def _parts(kind, param, xi, xj):
    """(s, ui, uj, d, a) of a SqExp / OU entry, exact."""
    s = mpf(1.0 / float(param))
    ui, uj = _m(xi) * s, _m(xj) * s
    d = ui - uj
    a = -(d * d) / 2 if kind == SQEXP else -abs(d)
    return s, ui, uj, d, a


def entry(kind, param, xi, xj):
    """(k, dk/dparam, dk/dxj) of one term at one pair, as 50-digit numbers."""
    if kind in (SQEXP, OU):
        s, ui, uj, d, a = _parts(kind, param, xi, xj)
        k = MP.exp(a)
        if kind == SQEXP:
            return k, k * d * d * s, k * d * s
        return k, k * abs(d) * s, (k * _sign(d) * s if not MP.isnan(d) else d)
    if kind == LINEAR:
        return _m(xi) * _m(xj) + mpf(float(param)), mpf(1), _m(xi)
    if kind == CAT:
        return (mpf(0) if abs(_m(xi) - _m(xj)) > 0 else mpf(1)), mpf(0), mpf(0)
    raise ValueError(f"no entry for term kind {kind}")


def entry_bound(kind, param, xi, xj, c_e=1, c_u=1):
    """(B_k, B_dparam, B_dxj): the rounding-error bounds of the module docstring for finite inputs.
    Linear: one rounding per operation of x_i x_j + c; its derivatives and all of Cat are exact."""
    xi, xj = float(xi), float(xj)
    if kind == LINEAR:
        p = abs(mpf(xi) * mpf(xj))
        return EPS * (2 * p + abs(mpf(float(param)))) + FLOOR, mpf(0), mpf(0)
    if kind == CAT:
        return mpf(0), mpf(0), mpf(0)
    s, ui, uj, d, a = _parts(kind, param, xi, xj)
    k = MP.exp(a)
    uu = EPS * c_u * (abs(ui) + abs(uj))
    ad = abs(d)
    if kind == SQEXP:
        bk = k * EPS * (c_e + abs(a)) + k * ad * uu + FLOOR
        g, dg, m = k * d * d * s, k * abs(2 * d - d ** 3) * s, d * d          # dk/dl
        bl = g * EPS * (c_e + abs(a) + 4) + dg * uu + FLOOR * (1 + s + m * s)
        g, dg, m = k * ad * s, k * abs(1 - d * d) * s, ad                     # dk/dxj
        bx = g * EPS * (c_e + abs(a) + 4) + dg * uu + FLOOR * (1 + s + m * s)
        return bk, bl, bx
    bk = k * EPS * (c_e + abs(a)) + k * uu + FLOOR
    g, dg, m = k * ad * s, k * abs(1 - ad) * s, ad                            # dk/dl
    bl = g * EPS * (c_e + abs(a) + 4) + dg * uu + FLOOR * (1 + s + m * s)
    g, dg, m = k * s, k * s, mpf(1)                                           # dk/dxj (off the kink)
    bx = g * EPS * (c_e + abs(a) + 3) + dg * uu + FLOOR * (1 + s + m * s)
    return bk, bl, bx


def worst_ratio(kind, param, x, pairs, got, which=0, c_e=1, c_u=1):
    """max over the pairs (i, j) of |got[i, j] - exact| / bound for the value (which = 0), dk/dparam
    (1) or dk/dxj (2) of one term on the coordinates x; returns (ratio, (i, j)) of the worst."""
    worst, at = 0.0, None
    for i, j in pairs:
        ref = entry(kind, param, x[i], x[j])[which]
        b = entry_bound(kind, param, x[i], x[j], c_e, c_u)[which]
        r = float(abs(mpf(float(got[i, j])) - ref) / b)
        if r != r:                                           # a NaN where the exact value is a number
            return r, (i, j)
        if r > worst:
            worst, at = r, (i, j)
    return worst, at


# ------------------------------------------------------------------------------------------------
# Formulas: terms = [(kind, col, param, group)], groups contiguous; a group multiplies its terms,
# groups add. X rows are points. A NOISE term is its variance on the diagonal of a Gram, 0 across.
# ------------------------------------------------------------------------------------------------
def formula_entry(terms, xa, xb, same_point=False):
    """(k, [dk/dparam_t], [dk/dxb[col] per column as dict]) of the whole formula at rows xa, xb."""
    terms = list(terms)
    vals = []
    for kind, col, param, group in terms:
        if kind == NOISE:
            vals.append((mpf(float(param)) if same_point else mpf(0), mpf(1) if same_point else mpf(0), mpf(0)))
        else:
            vals.append(entry(kind, param, xa[col], xb[col]))
    k, dparam, dx = mpf(0), [mpf(0)] * len(terms), {}
    for t, (kind, col, param, group) in enumerate(terms):
        others = mpf(1)
        for s2, t2 in enumerate(terms):
            if s2 != t and t2[3] == group:
                others *= vals[s2][0]
        dparam[t] = vals[t][1] * others
        if kind != NOISE:
            dx[col] = dx.get(col, mpf(0)) + vals[t][2] * others
        if t == 0 or terms[t - 1][3] != group:
            k += vals[t][0] * others
    return k, dparam, dx


def gram(X, terms, noise=0.0):
    n = len(X)
    C = MP.matrix(n, n)
    for i in range(n):
        for j in range(n):
            C[i, j] = formula_entry(terms, X[i], X[j], i == j)[0]
        C[i, i] += mpf(float(noise))
    return C


def cross(Xa, Xb, terms):
    K = MP.matrix(len(Xa), len(Xb))
    for i in range(len(Xa)):
        for j in range(len(Xb)):
            K[i, j] = formula_entry(terms, Xa[i], Xb[j])[0]
    return K


def _vec(v):
    return MP.matrix([mpf(float(t)) for t in v])


def logpdf_of(C, v):
    """log N(v | 0, C) by determinant and inverse."""
    v = _vec(v)
    quad = (v.T * MP.inverse(C) * v)[0]
    return -(len(v) * LOG2PI + MP.log(MP.det(C)) + quad) / 2


def logpdf(X, terms, noise, v):
    return logpdf_of(gram(X, terms, noise), v)


def grad_from(C, dCs, v):
    """From the covariance C, the matrices dC/dtheta and v: (dv, [dtheta], dnoise, [scale_theta],
    scale_noise) with dv = -alpha, dtheta = 1/2 sum W o dC, W = alpha alpha^T - C^-1, dnoise =
    1/2 tr W, and the scales the same sums over |alpha alpha^T| + |C^-1| and |dC| (the magnitudes
    oracle.restatement.logpdf_grad_scale states)."""
    n = C.rows
    v = _vec(v)
    Ci = MP.inverse(C)
    al = Ci * v
    half = mpf(1) / 2
    W = lambda i, j: al[i] * al[j] - Ci[i, j]
    A = lambda i, j: abs(al[i] * al[j]) + abs(Ci[i, j])
    rng = [(i, j) for i in range(n) for j in range(n)]
    dth = [half * sum(W(i, j) * dC[i, j] for i, j in rng) for dC in dCs]
    sth = [half * sum(A(i, j) * abs(dC[i, j]) for i, j in rng) for dC in dCs]
    return -al, dth, half * sum(W(i, i) for i in range(n)), sth, half * sum(A(i, i) for i in range(n))


def grad_matrices(X, terms, noise):
    """(C, [dC/dparam_t]) of the formula on the rows of X."""
    n, T = len(X), len(list(terms))
    C = MP.matrix(n, n)
    dCs = [MP.matrix(n, n) for _ in range(T)]
    for i in range(n):
        for j in range(n):
            k, dp, _ = formula_entry(terms, X[i], X[j], i == j)
            C[i, j] = k
            for t in range(T):
                dCs[t][i, j] = dp[t]
        C[i, i] += mpf(float(noise))
    return C, dCs


def logpdf_grad(X, terms, noise, v):
    C, dCs = grad_matrices(X, terms, noise)
    return (logpdf_of(C, v),) + grad_from(C, dCs, v)


def posterior_mean(X, terms, noise, y, Xs):
    return cross(Xs, X, terms) * (MP.inverse(gram(X, terms, noise)) * _vec(y))


def vfe_bound(X, terms, noise, y, Z, jitter):
    """elbo = log N(y | 0, Q + noise I) - sum(kdiag(X) - diag Q) / (2 noise),
    Q = K(X, Z) (K(Z, Z) + jitter I)^-1 K(Z, X) (a NOISE term counts in kdiag and in K(Z, Z))."""
    Kuf = cross(Z, X, terms)
    Q = Kuf.T * MP.inverse(gram(Z, terms, jitter)) * Kuf
    n = len(X)
    tr = sum(formula_entry(terms, X[i], X[i], True)[0] - Q[i, i] for i in range(n))
    C = Q.copy()
    for i in range(n):
        C[i, i] += mpf(float(noise))
    return logpdf_of(C, y) - tr / (2 * mpf(float(noise)))


def vfe_bound_grad_z(X, terms, noise, y, Z, jitter, cols=None):
    """d elbo / dZ[m][c] by mpmath.diff at full precision, for the columns `cols` (default: all;
    a column only Cat reads is a step function: leave it out). Entries not asked for are None."""
    Z = [[mpf(float(t)) for t in row] for row in Z]
    out = [[None] * len(Z[0]) for _ in Z]
    for m in range(len(Z)):
        for c in (range(len(Z[0])) if cols is None else cols):
            def f(z, m=m, c=c):
                Zm = [list(r) for r in Z]
                Zm[m][c] = z
                return vfe_bound(X, terms, noise, y, Zm, jitter)
            out[m][c] = MP.diff(f, Z[m][c])
    return out


# ------------------------------------------------------------------------------------------------
# The sweeps tests/test_hp_oracle.py and tests/test_gpu_entrywise.py share: 300 points, point 0 the
# anchor x0 and x_i = x0 + l d_i with d_i chosen so that the exp argument of the pair (i, 0) is
# -A_i (d = sqrt(2 A) for SqExp, A for OU), as nearly as x's grid at x0 allows.
# ------------------------------------------------------------------------------------------------
LN2_256 = 0.6931471805599453 / 256
CASES = [(1.5, 0.0), (30.0, 2.4e6), (0.01, -3.0), (100.0, 1e3)]         # (l, offset x0)
N_SWEEP = 300
BREAK0 = 3                                                              # point of breakpoint j = 1


def sweep_args():
    """The 299 magnitudes A_i, i = 1..299: two exact duplicates of the anchor (A = 0); the 255
    breakpoints (j + 256 (j mod 3)) ln2/256, j = 1..255, every table entry at a normal-range result
    and three binades; the specials; 30 tie points (n + 1/2) ln2/256."""
    special = [1e-17, 36.7, 708.39, 720.0, 740.0, 744.0, 745.13, 745.19, 745.21, 1e4]
    ties = [(37 * n + 0.5) * LN2_256 for n in range(1, 31)]
    args = [0.0, 0.0] + [(j + 256 * (j % 3)) * LN2_256 for j in range(1, 256)] + special + ties
    assert len(args) == N_SWEEP - 3
    return args


def sweep_x(kind, l, x0):
    """The 300 coordinates (numpy-free: a list of floats). The last two points are set through d:
    d = 1e-170 (d^2 underflows) and d = 1e200 (d^2 overflows)."""
    import math
    d = [math.sqrt(2 * a) if kind == SQEXP else a for a in sweep_args()] + [1e-170, 1e200]
    return [x0] + [x0 + l * t for t in d]


def sweep_pairs(overflow=True):
    """The anchor's column (every designed argument), and a lattice of other pairs in the first
    tile column (rows from the diagonal, the full and the padded tile). overflow=False leaves out
    the last point, whose d^2 overflows: there k = 0 in every arithmetic, but the derivative recipe
    k d^2 / l is 0 * inf = NaN in fp64, in the reference's arithmetic as in any other, while the
    exact value is a number far below 2^-1075. The derivative checks leave that point out."""
    n = N_SWEEP if overflow else N_SWEEP - 1
    return [(i, 0) for i in range(n)] + [(i, j) for i in range(1, n, 7) for j in range(1, 128, 9)]
