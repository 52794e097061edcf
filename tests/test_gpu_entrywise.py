"""Covariance entries of the HIP paths, one by one, against tests/hp_oracle.py (50 digits).

Every check is |got - exact| <= B with hp_oracle.entry_bound's B (no free tolerance), on the sweeps
of hp_oracle.sweep_x: the 256 table breakpoints, tie points, duplicates, the subnormal range, both
sides of the flush at -745.2, an underflowing and an overflowing d^2, at lengthscales and offsets
like real tables' (dates: l = 30, offset 2.4e6).

Constants (all <= 4), from the kernel code:

  table exp, c_e = 4.  exp_nonpos claims to be within 1 ulp of the library exp, which is itself within
      1 ulp of exp: 2 ulps of the result, and an ulp is at most 2 eps of its number.
  library exp (term_k, term_dk, term_d2: cross-covariances, product groups), c_e = 2: 1 ulp.
  OU, and SqExp outside the Gram kernel, c_u = 1: u = fl(s x), d = fl(u_i - u_j), the argument
      fl(d d) / 2 or |d|: the reference's recipe, operation by operation.
  SqExp in the Gram kernel, c_u = 4.  The coordinates are scaled by sc = fl(s fl(1/sqrt 2)) so that the
      argument is -fl(d' d'): sc = (s / sqrt 2)(1 + t), |t| <= 2 eps, common to both coordinates, so it
      moves the argument by 4 eps |a|; with d' rounding (2 eps |a|) and the square's (eps |a|) that is
      7 eps |a| besides the two coordinate roundings eps |d| (|u_i| + |u_j|) =: eps |d| U. The bound
      offers eps |a| + c_u eps |d| U and |d| U >= d^2 = 2 |a|, so c_u = 4 covers 7 |a| + |d| U.

Derivative outputs (logpdf_grad at N = 2, noise 3) are judged the same way: the exact closed form
evaluated at the covariance entry moved to either end of its bound, plus A |dC| bounds of the
derivative entries, plus C_F eps of the output's magnitude (oracle.restatement.logpdf_grad_scale's:
the sum of |alpha alpha^T| + |C^-1| against |dC|). C_F = 64: C = [[4, k], [k, 4]] has condition number
at most 5/3, and fewer than 40 roundings lie between the entries and an output (factor 3, two solves
4, the inverse 6 per entry, W 3, products and sums 6, the reductions' partial sums); 40 * 5/3 < 64.
Each of those roundings is fl(x) = x (1 + t) + h with |t| <= eps and, where x falls in the subnormal
range, |h| <= 2^-1075; every later factor (alpha, C^-1, k, dk, 1/l <= 2/3) is below 1 here, so the h's
add up to at most C_F 2^-1075 in an output: a derivative near 1e-320 cannot be closer than a
subnormal step. (The first version of this test left the h's out and failed on exactly the outputs
below 1e-315, by up to 40 of its tolerances, that is by less than one subnormal step.)

dZ of the sparse bound (N = 3, Mz = 2) is judged against mpmath.diff with 4x the error that
tests/sparse_grad_z_oracle.py itself has on the same cases (DZ_ORACLE_ERR per kind, pinned on the CPU by
test_dz_numpy_oracle_error_is_as_stated), relative to |ref| + the addend magnitude.

Each test prints its worst error/bound ratio before it asserts (DESIGN.md §5.1 lists them).
"""
import functools
import os

import numpy as np
import pytest

from gaplac_amd._native import CAT, LINEAR, OU, SQEXP
from gaplac_amd.backend import Context
from tests import hp_oracle as H
from tests import sparse_grad_z_oracle as GZ
from tests.conftest import gpu_available

gpu = pytest.mark.gpu
C_E_TABLE, C_E_LIBM = 4, 2
C_U = {(SQEXP, "gram"): 4, (OU, "gram"): 1, (SQEXP, "plain"): 1, (OU, "plain"): 1}
C_F = 64
KINDS = [(SQEXP, "sqexp"), (OU, "ou")]
PAIRS = H.sweep_pairs()
SUBNORMAL = 2.0 ** -1022
# worst |numpy dense route - mpmath.diff| / (|ref| + addends) over dz_cases(kind), measured on the CPU:
# 1.202e-11 (SqExp) and 5.561e-12 (OU), both at l = 30, offset 2.4e6, where a scaled coordinate is 8e4
# and its rounding alone moves d by 1e-11 (at offset 0 the route is within 3.5e-16)
DZ_ORACLE_ERR = {SQEXP: 1.21e-11, OU: 5.57e-12}


def env_context(**env):
    """A context created under the given environment switches (read at creation)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    if not gpu_available():
        pytest.skip("no GPU")
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_launch_pair():
    if not gpu_available():
        pytest.skip("no GPU")
    c = env_context(GAPLAC_TAIL_S="0")
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_unfused():
    if not gpu_available():
        pytest.skip("no GPU")
    c = env_context(GAPLAC_GRAD_FUSED="0")
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def sweep(kind, l, x0):
    return np.array(H.sweep_x(kind, l, x0))


@functools.lru_cache(maxsize=None)
def column_ref(kind, l, x0, c_e, c_u):
    """(exact, bound) of k(x_i, x_0) for the 300 sweep points, as two lists of 50-digit numbers."""
    x = sweep(kind, l, x0)
    return ([H.entry(kind, l, t, x[0])[0] for t in x], [H.entry_bound(kind, l, t, x[0], c_e, c_u)[0] for t in x])


def column_ratio(got, kind, l, x0, c_e, c_u, extra=None):
    """Worst |got[i] - k(x_i, x_0)| / bound over the column; extra[i] is added to the bound."""
    ref, b = column_ref(kind, l, x0, c_e, c_u)
    worst, at = 0.0, None
    for i in range(len(ref)):
        r = float(abs(H.mpf(float(got[i])) - ref[i]) / (b[i] + (H.mpf(float(extra[i])) if extra is not None else 0)))
        if r != r:
            return r, i
        if r > worst:
            worst, at = r, i
    return worst, at


_gram_cols = {}


def gram_column(ctx, kind, l, x0):
    """Column 0 of the stand-alone Gram of one term on the sweep, built once per case."""
    key = (kind, l, x0)
    if key not in _gram_cols:
        _gram_cols[key] = ctx.gram(sweep(kind, l, x0), [(kind, 0, l, 0)])
    return _gram_cols[key]


# ------------------------------------------------------------------------------------ stand-alone Gram
@gpu
@pytest.mark.parametrize("l,x0", H.CASES)
@pytest.mark.parametrize("kind,name", KINDS)
def test_gram_single_term(ctx, kind, name, l, x0):
    x = sweep(kind, l, x0)
    G = gram_column(ctx, kind, l, x0)
    r, at = H.worst_ratio(kind, l, x, PAIRS, G, 0, C_E_TABLE, C_U[kind, "gram"])
    r1, _ = H.worst_ratio(kind, l, x, PAIRS, G, 0, 1, 1)
    normal = [(i, j) for i, j in PAIRS if G[i, j] >= SUBNORMAL]
    rn, _ = H.worst_ratio(kind, l, x, normal, G, 0, C_E_TABLE, C_U[kind, "gram"])
    rn1, _ = H.worst_ratio(kind, l, x, normal, G, 0, 1, 1)
    print(f"ENTRYWISE gram {name} l={l} x0={x0}: worst error/bound {r:.3f} at {at} (with constants 1: {r1:.3f}); "
          f"normal-range results alone {rn:.3f} (with constants 1: {rn1:.3f})")
    assert r <= 1.0, (r, at)
    assert np.array_equal(G, G.T)
    assert np.all(G[[1, 2], 0] == 1.0) and np.all(np.diag(G) == 1.0)       # exact duplicates, the diagonal
    assert G[299, 0] == 0.0 and not np.signbit(G[299, 0])                    # d^2 overflows: +0
    ref = column_ref(kind, l, x0, C_E_TABLE, C_U[kind, "gram"])[0]
    hit = [i for i in range(300) if float(ref[i]) >= SUBNORMAL and float(ref[i]) < 1.0]
    sub = [i for i in range(300) if 0.0 < float(ref[i]) < SUBNORMAL]
    assert len(hit) >= 255 and len(sub) >= 4                                 # normal and subnormal results seen


@gpu
def test_gram_linear_term(ctx):
    x = sweep(OU, 1.5, 0.0).copy()
    x[299] = 1e150                                                           # (products stay finite)
    G = ctx.gram(x, [(LINEAR, 0, 0.5, 0)])
    r, at = H.worst_ratio(LINEAR, 0.5, x, PAIRS, G)
    print(f"ENTRYWISE gram linear: worst error/bound {r:.3f} at {at}")
    assert r <= 1.0, (r, at)


@gpu
def test_gram_product_group_of_three(ctx):
    """SqExp * OU * Linear in one group, the first group: GM_PR_FIRST, GM_PR and GM_PR_LAST0. The
    bound is the factors' bounds carried through the two products, each rounded once (and possibly
    into the subnormal range): ((B1 k2 + B2 k1 + eps k1 k2 + floor) |k3| + B3 k1 k2 + eps |k| + floor)."""
    x = sweep(OU, 1.5, 0.0).copy()
    x[299] = 1e150
    terms = [(SQEXP, 0, 1.5, 0), (OU, 0, 3.0, 0), (LINEAR, 0, 0.5, 0)]
    G = ctx.gram(x, terms)
    cs = [(C_E_TABLE, C_U[SQEXP, "gram"]), (C_E_TABLE, C_U[OU, "gram"]), (1, 1)]
    worst, at = 0.0, None
    for i, j in PAIRS:
        k = [H.entry(t[0], t[2], x[i], x[j])[0] for t in terms]
        b = [H.entry_bound(t[0], t[2], x[i], x[j], *c)[0] for t, c in zip(terms, cs)]
        p12 = k[0] * k[1]
        bound = ((b[0] * k[1] + b[1] * k[0] + H.EPS * p12 + H.FLOOR) * abs(k[2]) + b[2] * p12
                 + H.EPS * abs(p12 * k[2]) + H.FLOOR) * (1 + H.mpf(10) ** -10)
        r = float(abs(H.mpf(float(G[i, j])) - p12 * k[2]) / bound)
        assert r == r, (i, j)
        if r > worst:
            worst, at = r, (i, j)
    print(f"ENTRYWISE gram product group: worst error/bound {worst:.3f} at {at}")
    assert worst <= 1.0, (worst, at)
    assert np.array_equal(G, G.T)


# ------------------------------------------------------------------------- the Gram an evaluation builds
def check_factor_column(c, G, kind, name, l, x0, what):
    """noise 3: C_00 = 4, L_00 = 2 exactly, L[i, 0] = C[i, 0] / 2, so k(x_i, x_0) = 2 L[i, 0]. Halving
    is exact down to the normal range; a subnormal k with an odd last bit is rounded by it, by
    design of the test (not of the kernel), so below 2^-1021 the two columns may differ by one
    subnormal step (2^-1074) and that step is added to the bound there. Everywhere else: bitwise."""
    x = sweep(kind, l, x0)
    L, z = c.factor(x, [(kind, 0, l, 0)], 3.0, np.ones(len(x)))
    assert L[0, 0] == 2.0
    col = 2.0 * L[:, 0]
    col[0] -= 3.0                                                            # (C_00 - noise = k_00 = 1)
    small = np.abs(G[:, 0]) < 2.0 ** -1021
    extra = np.where(small, 2.0 ** -1074, 0.0)
    r, at = column_ratio(col, kind, l, x0, C_E_TABLE, C_U[kind, "gram"], extra)
    print(f"ENTRYWISE factor[{what}] {name} l={l} x0={x0}: worst error/bound {r:.3f} at {at}")
    assert r <= 1.0, (r, at)
    assert np.array_equal(col[~small], G[~small, 0])
    assert np.all(np.abs(col[small] - G[small, 0]) <= 2.0 ** -1074)
    return col


@gpu
@pytest.mark.parametrize("l,x0", H.CASES)
@pytest.mark.parametrize("kind,name", KINDS)
def test_gram_inside_an_evaluation(ctx, ctx_launch_pair, kind, name, l, x0):
    G = gram_column(ctx, kind, l, x0)
    a = check_factor_column(ctx, G, kind, name, l, x0, "in-tail")
    b = check_factor_column(ctx_launch_pair, G, kind, name, l, x0, "launch pair")
    assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------ cross-covariance
@gpu
@pytest.mark.parametrize("l,x0", H.CASES)
@pytest.mark.parametrize("kind,name", KINDS)
def test_cross_covariance(ctx, kind, name, l, x0):
    """N = 1, noise 0, y = 1: C = 1, alpha = 1, and the mean at xs_j is k(xs_j, x_0) itself."""
    x = sweep(kind, l, x0)
    mean, var = ctx.posterior_mean_var(x[:1, None], [(kind, 0, l, 0)], 0.0, np.ones(1), x[:, None])
    r, at = column_ratio(mean, kind, l, x0, C_E_LIBM, C_U[kind, "plain"])
    print(f"ENTRYWISE cross {name} l={l} x0={x0}: worst error/bound {r:.3f} at {at}")
    assert r <= 1.0, (r, at)
    assert np.all(mean[[0, 1, 2]] == 1.0) and mean[299] == 0.0
    assert np.all((var >= 0.0) & (var <= 1.0)) and np.all(var[[0, 1, 2]] == 0.0)


# ----------------------------------------------------------------------------------------- derivatives
D_IDX = sorted(set(range(1, 258, 8)) | set(range(258, 268)) | {268, 280, 298})   # 46 arguments, no d^2 overflow
D_CASES = [(1.5, 0.0), (30.0, 2.4e6)]
V2 = np.array([1.0, -0.5])


def grad_terms(kind, l, path):
    """default / unfused: one term (table exp); product: the term times an OU term (library exp)."""
    return [(kind, 0, l, 0), (OU, 0, 2.0 * l, 0)] if path == "product" else [(kind, 0, l, 0)]


def grad_reference(terms, path, xa, xb):
    """Exact outputs of logpdf_grad on the points (xa, xb) with noise 3 and v = V2, and for each its
    tolerance (module docstring): [(exact, tol)] for dv_0, dv_1, dparam_t..., dnoise."""
    c_e = C_E_LIBM if path == "product" else C_E_TABLE
    X = [[xa], [xb]]
    C, dCs = H.grad_matrices(X, terms, 3.0)
    vals = [H.entry(t[0], t[2], xb, xa) for t in terms]
    bnds = [H.entry_bound(t[0], t[2], xb, xa, c_e, 1) for t in terms]
    # bounds of the off-diagonal entry of C and of every dC (first order, 1 + 1e-10 for the rest)
    if len(terms) == 1:
        bK, bdK = bnds[0][0], [bnds[0][1]]
    else:
        (k1, g1, _), (k2, g2, _) = vals
        (b1, bg1, _), (b2, bg2, _) = bnds
        bK = b1 * k2 + b2 * k1 + H.EPS * k1 * k2 + H.FLOOR
        bdK = [bg1 * k2 + b2 * abs(g1) + H.EPS * abs(g1) * k2 + H.FLOOR,
               bg2 * k1 + b1 * abs(g2) + H.EPS * abs(g2) * k1 + H.FLOOR]

    def outputs(Cm):
        dv, dth, dn, sth, sn = H.grad_from(Cm, dCs, V2)
        Ci = H.MP.inverse(Cm)
        al = Ci * H._vec(V2)
        sv = [sum(abs(Ci[i, j]) * abs(H.mpf(float(V2[j]))) for j in range(2)) for i in range(2)]
        a01 = abs(al[0] * al[1]) + abs(Ci[0, 1])
        return [dv[0], dv[1]] + dth + [dn], sv + sth + [sn], a01

    q, scale, a01 = outputs(C)
    moved = []
    for sgn in (1, -1):
        Cm = C.copy()
        Cm[0, 1] += sgn * bK
        Cm[1, 0] += sgn * bK
        moved.append(outputs(Cm)[0])
    out = []
    for n in range(len(q)):
        tol = C_F * (H.EPS * scale[n] + H.FLOOR) + max(abs(m[n] - q[n]) for m in moved)
        if 2 <= n < 2 + len(terms):
            tol += a01 * bdK[n - 2]
        out.append((q[n], tol * (1 + H.mpf(10) ** -10)))
    return out


def check_grad_path(c, path, kind, name):
    worst, at = 0.0, None
    for l, x0 in D_CASES:
        x = sweep(kind, l, x0)
        terms = grad_terms(kind, l, path)
        for i in D_IDX:
            lp, dv, dp, dn = c.logpdf_grad(np.array([[x[0]], [x[i]]]), terms, 3.0, V2)
            got = [dv[0], dv[1]] + list(dp) + [dn]
            ref = grad_reference(tuple(terms), path, float(x[0]), float(x[i]))
            for n, (g, (q, tol)) in enumerate(zip(got, ref)):
                assert np.isfinite(g), (l, x0, i, n)
                r = float(abs(H.mpf(float(g)) - q) / tol) if tol > 0 else (0.0 if float(q) == g else np.inf)
                if r > worst:
                    worst, at = r, (l, x0, i, n)
            if x[i] == x[0]:                                                # a duplicate: dC/dl is exactly 0
                assert dp[0] == 0.0
    print(f"ENTRYWISE grad[{path}] {name}: worst error/tolerance {worst:.3f} at {at}")
    assert worst <= 1.0, (worst, at)


@gpu
@pytest.mark.parametrize("kind,name", KINDS)
def test_grad_fused(ctx, kind, name):
    check_grad_path(ctx, "default", kind, name)


@gpu
@pytest.mark.parametrize("kind,name", KINDS)
def test_grad_unfused(ctx_unfused, kind, name):
    check_grad_path(ctx_unfused, "unfused", kind, name)


@gpu
@pytest.mark.parametrize("kind,name", KINDS)
def test_grad_product_group(ctx, kind, name):
    check_grad_path(ctx, "product", kind, name)


# --------------------------------------------------------------------------------------------------- dZ
DZ_IDX = [H.BREAK0, H.BREAK0 + 100, H.BREAK0 + 254, 258, 259, 260, 263, 265, 266, 267, 268, 290]
Y3 = np.array([1.0, -0.5, 0.25])


def dz_cases(kind):
    """(X, Z, terms): Z_0 is the anchor and X_0 the sweep point, so the pair (Z_0, X_0) has the
    designed argument; the other points keep both matrices well conditioned. A point that
    coincides with the anchor is left out for OU (its kink: no derivative to compare)."""
    for l, x0 in D_CASES:
        x = sweep(kind, l, x0)
        for i in DZ_IDX:
            if kind == OU and x[i] == x[0]:
                continue
            X = np.array([[x[i]], [x0 + 0.5 * l], [x0 - 0.8 * l]])
            Z = np.array([[x0], [x0 + 1.3 * l]])
            yield (l, x0, i), X, Z, [(kind, 0, l, 0)]


@functools.lru_cache(maxsize=None)
def dz_reference(kind):
    out = []
    for key, X, Z, terms in dz_cases(kind):
        ref = H.vfe_bound_grad_z(X.tolist(), terms, 0.3, Y3, Z.tolist(), 1e-3)
        _, scale = GZ.dense(X, terms, 0.3, Y3, Z, 1e-3)
        out.append((key, X, Z, terms, np.array([[float(t) for t in row] for row in ref]), scale))
    return out


def dz_error(dZ, ref, scale):
    return float(np.max(np.abs(dZ - ref) / (np.abs(ref) + scale)))


@pytest.mark.parametrize("kind,name", KINDS)
def test_dz_numpy_oracle_error_is_as_stated(kind, name):
    """(CPU) The numpy dense route against mpmath.diff on the GPU test's cases: within DZ_ORACLE_ERR."""
    worst = max(dz_error(GZ.dense(X, terms, 0.3, Y3, Z, 1e-3)[0], ref, scale)
                for key, X, Z, terms, ref, scale in dz_reference(kind))
    print(f"ENTRYWISE dZ numpy oracle {name}: worst error {worst:.3e}")
    assert 0.9 * DZ_ORACLE_ERR[kind] <= worst <= DZ_ORACLE_ERR[kind]


@gpu
@pytest.mark.parametrize("kind,name", KINDS)
def test_dz_against_mpmath_diff(ctx, kind, name):
    worst, at = 0.0, None
    for key, X, Z, terms, ref, scale in dz_reference(kind):
        got = ctx.sparse_elbo_grad(X, terms, 0.3, Y3, Z, 1e-3, wrt_z=True)
        assert np.all(np.isfinite(got[5]))
        e = dz_error(got[5], ref, scale)
        print(f"ENTRYWISE dZ {name} case {key}: error {e:.3e}")
        if e > worst:
            worst, at = e, key
    print(f"ENTRYWISE dZ {name}: worst error {worst:.3e} at {at} (allowed {4 * DZ_ORACLE_ERR[kind]:.2e})")
    assert worst <= 4 * DZ_ORACLE_ERR[kind], (worst, at)


# ------------------------------------------------------------------- non-finite and signed-zero inputs
SPECIALS = [np.nan, np.inf, -np.inf, -0.0]
TERMS1 = {"sqexp": (SQEXP, 0, 1.5, 0), "ou": (OU, 0, 1.5, 0), "linear": (LINEAR, 0, 0.5, 0), "cat": (CAT, 0, 0.0, 0)}


def same_entry(got, kind, param, xi, xj, c_e):
    """got is the IEEE value of the exact rule: NaN where it is NaN, the same infinity, and a finite
    value within its bound (0 and 1 exactly: their bounds are below an ulp)."""
    ref = H.entry(kind, param, xi, xj)[0]
    if H.MP.isnan(ref):
        return bool(np.isnan(got))
    if H.MP.isinf(ref):
        return got == float(ref)
    if kind in (SQEXP, OU) and not (np.isfinite(xi) and np.isfinite(xj)):
        return got == float(ref)                                             # exp(-inf) = 0 exactly
    return bool(abs(H.mpf(float(got)) - ref) <= H.entry_bound(kind, param, xi, xj, c_e, 1)[0])


@gpu
@pytest.mark.parametrize("special", SPECIALS, ids=["nan", "inf", "-inf", "-0.0"])
@pytest.mark.parametrize("name", sorted(TERMS1))
def test_special_inputs_gram(ctx, name, special):
    term = TERMS1[name]
    x = np.array([1.0, special, 2.0, 1.0, 0.0, special])
    G = ctx.gram(x, [term])
    bad = [(i, j, G[i, j]) for i in range(6) for j in range(6)
           if not same_entry(G[i, j], term[0], term[2], x[i], x[j], C_E_TABLE)]
    assert not bad, bad
    if name == "cat" and np.isnan(special):
        assert np.all(G[1] == 1.0) and np.all(G[:, 1] == 1.0)               # the reference's rule, diagonal included
    if special == 0.0:                                                       # -0.0 is 0.0 to every kind
        assert np.array_equal(G, ctx.gram(np.where(x == 0.0, 0.0, x), [term]))


@gpu
@pytest.mark.parametrize("special", SPECIALS, ids=["nan", "inf", "-inf", "-0.0"])
@pytest.mark.parametrize("name", sorted(TERMS1))
def test_special_inputs_cross_covariance_and_prior(ctx, name, special):
    term = TERMS1[name]
    kind, param = term[0], term[2]
    xs = np.array([special, 1.0, 2.0, -0.0])
    # N = 1 at the finite point 1: C = k(1, 1) (1, or 1.5 for Linear), mean_j = k(xs_j, 1) / C
    mean, var = ctx.posterior_mean_var(np.ones((1, 1)), [term], 0.0, np.ones(1), xs[:, None])
    c00 = float(H.entry(kind, param, 1.0, 1.0)[0])
    for j in range(4):
        ref = H.entry(kind, param, xs[j], 1.0)[0]
        if H.MP.isnan(ref):
            assert np.isnan(mean[j]), (j, mean[j])
        elif H.MP.isinf(ref):
            assert mean[j] == float(ref)
        else:
            b = H.entry_bound(kind, param, xs[j], 1.0, C_E_LIBM, 1)[0] if np.isfinite(xs[j]) else 0
            assert abs(H.mpf(float(mean[j])) - ref / c00) <= b / c00 + 4 * H.EPS * abs(ref / c00), (j, mean[j])
    # N = 1 at the special point itself (Cat: k(NaN, NaN) = 1, a positive definite 1 x 1 matrix)
    if name == "cat":
        mean, var = ctx.posterior_mean_var(np.full((1, 1), special), [term], 0.0, np.ones(1), xs[:, None])
        want = [float(H.entry(kind, param, t, special)[0]) for t in xs]
        assert mean.tolist() == want and var.tolist() == [1.0 - w * w for w in want]
    # N = 0: the prior, mean 0 and var = k(xs_j, xs_j)
    mean, var = ctx.posterior_mean_var(np.zeros((0, 1)), [term], 0.0, np.zeros(0), xs[:, None])
    assert np.all(mean == 0.0)
    for j in range(4):
        ref = H.entry(kind, param, xs[j], xs[j])[0]
        if H.MP.isnan(ref):
            assert np.isnan(var[j]), (j, var[j])
        else:
            assert var[j] == float(ref), (j, var[j])
