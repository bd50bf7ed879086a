"""An independent reference for two loop-closure passes: the RANSAC scores of csrc/kt_match.hip (match_ransac, match_best; DESIGN.md 4.8 f)
and the sums of one reducing registration pass of csrc/kt_loop.hip (loop_nearest<true, true>, loop_fold; DESIGN.md 4.6 c).  Written from
DESIGN.md and the header comments of the two files; it imports nothing from the package or the oracle (numpy and the standard library only).

DRAWS.  r_k = fmix32(seed + 0x9E3779B9 * (3 h + k + 1)) mod 2^32 (murmur3's finaliser); the k-th index is r_k modulo the number of indices not
drawn yet, taken as a rank among those: the rank is raised by one for every earlier index it has reached, the smaller one first.

THREE-POINT FIT.  The float32 inputs are rationals.  fit_many() runs the triad construction in fixed point on Python integers at Q = 256
fractional bits (77 digits): every operation (product, quotient, integer square root, all rounded down) errs by at most 2^-256 in absolute
terms, and the construction amplifies an error by at most kappa^2 (kappa below; <= 400 wherever the result is used), so R and t carry more
than 60 correct digits (tests/test_loop_kernel_reference.py holds a sample against mpmath at 80 digits).  They are returned rounded to
double once, next to n1 / n3 of both sides.

INLIER COUNTS: the margin.  u = 2^-53.  The kernel's match_fit3 in double, first-order bounds, vectors in the 2-norm:
  a, b            differences of float32 values in double: relative error u
  n1 = |a|        3 roundings under the root, one for it: relative error <= 3 u;  e1 = a / n1: absolute error <= 5 u
  c = e1 x b      per component (5 u + u) (|e1_i b_j| + |e1_k b_l|) + u |c_i|: absolute error <= 16 u |b|
  n3 = |c|        relative error <= (16 |b| / n3 + 3) u;  e3 = c / n3: absolute error <= (32 |b| / n3 + 4) u
  e2 = e3 x e1    absolute error <= (32 |b| / n3 + 12) u
so every triad vector errs by at most (32 kappa + 12) u with kappa = max(|a|, |b|) / min(n1, n3) >= 1, the fit's condition (about |p| / n3),
taken as the larger of the two sides.  R = (e1 e1^T + e2 e2^T) + e3 e3^T: three products of two such vectors and two additions per entry,
|dR| <= 3 (2 (32 kappa + 12)) u + 5 u <= 272 kappa u.  c = ((p0 + p1) + p2) / 3: relative error 3 u.  t = c_old - R c_new:
|dt| <= |dR| |c_new|_1 + 8 u (|c_old|_1 + |c_new|_1).  The moved point P = ((r0 x + r1 y) + r2 z) + t of match_inlier:
|dP| <= |dR| (|p|_1 + |c_new|_1) + 16 u (|p|_1 + |c_old|_1 + |c_new|_1).  This reference evaluates the same expression in double from the
many-digit transform rounded once, which errs by less than the last term again.  Hence, for hypothesis h and match j, the kernel's point and
this reference's differ by at most
        dP(h, j) = 320 kappa_h u (|p_j|_1 + 2 (|c_old|_1 + |c_new|_1))            (FIT_C = 320: "a few tens of u" per vector, times the condition)
in every coordinate.  What follows from it, with (X, Y, Z) this reference's point:
  * |Z| <= dP: the sign of the kernel's Z is not known -> undecided.
  * otherwise |X_k / Z_k - X / Z| <= dP (1 + |X / Z|) / (|Z| - dP), so du = (fx X) / Z + cx - u_old errs by at most
    dU = fx dP (1 + |X / Z|) / (|Z| - dP) + 8 u (|fx X / Z| + |cx| + |u_old|), dv likewise, and err^2 = du^2 + dv^2 by at most
    dE = 2 (|du| dU + |dv| dV) + dU^2 + dV^2 + 4 u err^2.  |err^2 - thr^2| <= dE -> undecided.  (Relative to thr^2 this is the margin
    320 kappa u times the projection's own factor 2 fx |p| (1 + |X / Z|) / (|Z| thr): at fx = 525, Z = 1 m, thr = 2 px about 1e-9 kappa.)
  * the gate: the kernel's n1 errs by 3 u, its n3 by (16 kappa + 3) u relatively.  A norm within (16 kappa + 8) u of 1e-3 leaves the whole
    hypothesis undecided (lo = 0, hi = m); a norm certainly below 1e-3 gives lo = hi = 0.
  * a hypothesis with a norm below 1 cm (kappa in the hundreds and beyond: the bound says nothing useful) is undecided as a whole, lo = 0, hi = m;
    the numpy restatement is its only witness.
lo = the matches certainly in, hi = lo + the undecided ones.  The margin is derived above, not measured; the tests cap the share of hypotheses
with hi != lo at 1 % per case, so it cannot hide a wrong score.

exact_counts() is for transforms that ARE rationals (the lattice case: a signed axis permutation and a dyadic translation): Fraction
arithmetic, no margin; the caller shows that the kernel's arithmetic is exact there.

ICP SUMS.  icp_pass(): the moved point is float32(((m0 x + m1 y) + m2 z) + m3) in double, which numpy reproduces operation for operation; the
nearest target is the lowest-index minimum of the float32 (dx dx + dy dy) + dz dz.  Each of the 16 terms (s, t, s_a t_b, d2) is a float32 value or
the product of two: exact in double.  Their sums are taken in integers (every term is a multiple of 2^-SCALE), so `exact` has no error at all and
the only error a kernel can add is that of its own summation."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
M32 = 0xFFFFFFFF
GATE = 1e-3              # metres, the double the kernel compares with
ILL = 1e-2               # below this norm a hypothesis is left to the restatement
FIT_C = 320.0
Q = 256
ONE = 1 << Q
SCALE = 400              # icp_pass: every term must be a multiple of 2^-SCALE


# ---------------------------------------------------------------------------------------------------------------------------------
# draws
# ---------------------------------------------------------------------------------------------------------------------------------
def fmix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def draw(seed, h, m):
    """The three match indices of hypothesis h among m >= 3 matches (Python integers)."""
    taken = []
    for k in range(3):
        r = fmix32((seed & M32) + 0x9E3779B9 * (3 * h + k + 1)) % (m - k)
        for t in sorted(taken):          # r is a rank among the indices not taken yet
            if r >= t:
                r += 1
        taken.append(r)
    return tuple(taken)


def draws(seed, n_hyp, m):
    """draw() for h = 0 .. n_hyp - 1 at once: int64 [n_hyp, 3]"""
    h = np.arange(n_hyp, dtype=np.uint64)
    out = np.zeros((n_hyp, 3), np.int64)
    for k in range(3):
        x = (np.uint64(seed & M32) + np.uint64(0x9E3779B9) * (np.uint64(3) * h + np.uint64(k + 1))) & np.uint64(M32)
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x85EBCA6B)) & np.uint64(M32)
        x ^= x >> np.uint64(13)
        x = (x * np.uint64(0xC2B2AE35)) & np.uint64(M32)
        x ^= x >> np.uint64(16)
        r = (x % np.uint64(m - k)).astype(np.int64)
        if k == 1:
            r += r >= out[:, 0]
        if k == 2:
            r += r >= np.minimum(out[:, 0], out[:, 1])
            r += r >= np.maximum(out[:, 0], out[:, 1])
        out[:, k] = r
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the three-point fit in fixed point
# ---------------------------------------------------------------------------------------------------------------------------------
_to_int = np.frompyfunc(lambda v: int(v) << (Q - 160), 1, 1)
_isqrt = np.frompyfunc(lambda v: math.isqrt(v << Q), 1, 1)
_to_float = np.frompyfunc(lambda v: v / ONE, 1, 1)       # int / int: correctly rounded


def _fixed(a):
    """float32 values (held in any float array) as integers at 2^-Q, exactly"""
    a = np.asarray(a, np.float64)
    assert np.isfinite(a).all() and (a == a.astype(np.float32)).all() and (np.abs(a) < 2.0 ** 60).all()
    return _to_int(np.ldexp(a, 160))                      # 2^-149 is float32's finest bit: an integer-valued double


def _mul(a, b):
    return (a * b) >> Q


def _div(a, b):
    return (a << Q) // b


def _flt(a):
    return _to_float(a).astype(np.float64)


def _nonzero(n):
    out = n.copy()
    out[n == 0] = ONE
    return out


def _triads(p0, p1, p2):
    """[n, 3] object arrays -> e (three [n, 3]), centroid, n1, n3 (objects), |b| (float); zero norms give zero vectors"""
    a, b = p1 - p0, p2 - p0
    dot = lambda v, w: _mul(v[:, 0], w[:, 0]) + _mul(v[:, 1], w[:, 1]) + _mul(v[:, 2], w[:, 2])
    cross = lambda v, w: np.stack([_mul(v[:, 1], w[:, 2]) - _mul(v[:, 2], w[:, 1]), _mul(v[:, 2], w[:, 0]) - _mul(v[:, 0], w[:, 2]),
                                   _mul(v[:, 0], w[:, 1]) - _mul(v[:, 1], w[:, 0])], axis=1)
    n1 = _isqrt(dot(a, a))
    d1 = _nonzero(n1)
    e1 = np.stack([_div(a[:, k], d1) for k in range(3)], axis=1)
    c = cross(e1, b)
    n3 = _isqrt(dot(c, c))
    d3 = _nonzero(n3)
    e3 = np.stack([_div(c[:, k], d3) for k in range(3)], axis=1)
    e2 = cross(e3, e1)
    cen = np.stack([((p0[:, k] + p1[:, k]) + p2[:, k]) // 3 for k in range(3)], axis=1)
    return (e1, e2, e3), cen, n1, n3, _flt(_isqrt(dot(b, b)))


def fit_many(Pn, Po, tri):
    """The rigid T (new -> old) through the pairs tri[h] of the float32 point lists Pn / Po, for every hypothesis h.  dict of float64 arrays:
    R [n, 3, 3], t [n, 3] (the many-digit values rounded once), n1n, n3n, n1o, n3o, kappa, cn1, co1 (1-norms of the centroids) [n]"""
    tri = np.asarray(tri, np.int64)
    Fn, Fo = _fixed(Pn), _fixed(Po)
    en, cn, n1n, n3n, bn = _triads(Fn[tri[:, 0]], Fn[tri[:, 1]], Fn[tri[:, 2]])
    eo, co, n1o, n3o, bo = _triads(Fo[tri[:, 0]], Fo[tri[:, 1]], Fo[tri[:, 2]])
    R = np.empty((len(tri), 3, 3), object)
    for a in range(3):
        for b in range(3):
            R[:, a, b] = _mul(eo[0][:, a], en[0][:, b]) + _mul(eo[1][:, a], en[1][:, b]) + _mul(eo[2][:, a], en[2][:, b])
    t = np.stack([co[:, a] - (_mul(R[:, a, 0], cn[:, 0]) + _mul(R[:, a, 1], cn[:, 1]) + _mul(R[:, a, 2], cn[:, 2])) for a in range(3)], axis=1)
    out = dict(R=_flt(R.reshape(-1)).reshape(-1, 3, 3), t=_flt(t.reshape(-1)).reshape(-1, 3), n1n=_flt(n1n), n3n=_flt(n3n), n1o=_flt(n1o), n3o=_flt(n3o))
    nmin = np.minimum(np.minimum(out["n1n"], out["n3n"]), np.minimum(out["n1o"], out["n3o"]))
    with np.errstate(divide="ignore"):
        out["kappa"] = np.maximum(np.maximum(out["n1n"], bn), np.maximum(out["n1o"], bo)) / nmin
    out["nmin"] = nmin
    out["cn1"], out["co1"] = np.abs(_flt(cn.reshape(-1)).reshape(-1, 3)).sum(axis=1), np.abs(_flt(co.reshape(-1)).reshape(-1, 3)).sum(axis=1)
    return out


def fit_mpmath(pn3, po3, dps=80):
    """One fit with mpmath at `dps` digits, for the cross-check of fit_many: (R 3x3, t 3, (n1n, n3n, n1o, n3o)) as mpf"""
    from mpmath import mp, mpf
    mp.dps = dps

    def triad(p):
        p = [[mpf(float(v)) for v in q] for q in p]
        a, b = [p[1][k] - p[0][k] for k in range(3)], [p[2][k] - p[0][k] for k in range(3)]
        cr = lambda v, w: [v[1] * w[2] - v[2] * w[1], v[2] * w[0] - v[0] * w[2], v[0] * w[1] - v[1] * w[0]]
        n1 = mp.sqrt(sum(v * v for v in a))
        e1 = [v / n1 for v in a]
        c = cr(e1, b)
        n3 = mp.sqrt(sum(v * v for v in c))
        e3 = [v / n3 for v in c]
        return (e1, cr(e3, e1), e3), [(p[0][k] + p[1][k] + p[2][k]) / 3 for k in range(3)], n1, n3

    en, cn, n1n, n3n = triad(pn3)
    eo, co, n1o, n3o = triad(po3)
    R = [[sum(eo[k][a] * en[k][b] for k in range(3)) for b in range(3)] for a in range(3)]
    return R, [co[a] - sum(R[a][b] * cn[b] for b in range(3)) for a in range(3)], (n1n, n3n, n1o, n3o)


# ---------------------------------------------------------------------------------------------------------------------------------
# inlier counts
# ---------------------------------------------------------------------------------------------------------------------------------
def inlier_bounds(fit, Pn, uv_old, fx, fy, cx, cy, reproj_px, chunk=1 << 21):
    """(lo, hi) int64 [n_hyp]: the matches certainly inside, and those plus the undecided ones (the module docstring derives the margin).
    fx .. reproj_px are the float32 values the kernel receives."""
    Pn = np.asarray(Pn, np.float32).astype(np.float64).reshape(-1, 3)
    uv = np.asarray(uv_old, np.float64).reshape(-1, 2)
    fx, fy, cx, cy, thr = (float(np.float32(v)) for v in (fx, fy, cx, cy, reproj_px))
    thr2 = thr * thr
    n, m = len(fit["R"]), len(Pn)
    lo, hi = np.zeros(n, np.int64), np.zeros(n, np.int64)
    kappa, nmin = fit["kappa"], fit["nmin"]
    gate_m = GATE * (16.0 * np.where(np.isfinite(kappa), kappa, 1.0) + 8.0) * U
    degenerate = nmin < GATE - gate_m
    whole = ~degenerate & (nmin < ILL)                      # at the gate, or too ill-conditioned for the bound
    hi[whole] = m
    use = np.flatnonzero(~degenerate & ~whole)
    p1 = np.abs(Pn).sum(axis=1)[None, :]
    x, y, z = Pn[:, 0][None, :], Pn[:, 1][None, :], Pn[:, 2][None, :]
    step = max(1, chunk // max(m, 1))
    for i0 in range(0, len(use), step):
        h = use[i0:i0 + step]
        R, t = fit["R"][h], fit["t"][h]
        X, Y, Z = (((R[:, a, 0:1] * x + R[:, a, 1:2] * y) + R[:, a, 2:3] * z) + t[:, a:a + 1] for a in range(3))
        dP = FIT_C * U * kappa[h][:, None] * (p1 + 2.0 * (fit["cn1"][h] + fit["co1"][h])[:, None])
        z_in, z_out = Z > dP, Z < -dP
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            den = np.abs(Z) - dP
            pu, pv = (fx * X) / Z, (fy * Y) / Z
            du, dv = (pu + cx) - uv[:, 0][None, :], (pv + cy) - uv[:, 1][None, :]
            dU = fx * dP * (1.0 + np.abs(X / Z)) / den + 8.0 * U * (np.abs(pu) + abs(cx) + np.abs(uv[:, 0])[None, :])
            dV = fy * dP * (1.0 + np.abs(Y / Z)) / den + 8.0 * U * (np.abs(pv) + abs(cy) + np.abs(uv[:, 1])[None, :])
            e2 = du * du + dv * dv
            dE = 2.0 * (np.abs(du) * dU + np.abs(dv) * dV) + dU * dU + dV * dV + 4.0 * U * e2
            inside = z_in & (e2 < thr2 - dE)
            outside = z_out | (z_in & (e2 > thr2 + dE))
        lo[h] = inside.sum(axis=1)
        hi[h] = lo[h] + (~inside & ~outside).sum(axis=1)
    return lo, hi


def exact_counts(R, t, Pn, uv_old, fx, fy, cx, cy, reproj_px):
    """The score of ONE rational transform (R 3x3, t 3 of Fractions or integers) in Fraction arithmetic: Z > 0 and du^2 + dv^2 <= thr^2."""
    fx, fy, cx, cy, thr = (Fraction(float(np.float32(v))) for v in (fx, fy, cx, cy, reproj_px))
    count = 0
    for p, (uo, vo) in zip(np.asarray(Pn, np.float32).reshape(-1, 3), np.asarray(uv_old).reshape(-1, 2)):
        p = [Fraction(float(v)) for v in p]
        X, Y, Z = (sum(Fraction(R[a][b]) * p[b] for b in range(3)) + Fraction(t[a]) for a in range(3))
        if Z > 0:
            du, dv = fx * X / Z + cx - int(uo), fy * Y / Z + cy - int(vo)
            count += du * du + dv * dv <= thr * thr
    return count


# ---------------------------------------------------------------------------------------------------------------------------------
# one reducing registration pass
# ---------------------------------------------------------------------------------------------------------------------------------
def icp_pass(src, dst, M):
    """dict(index uint32 [ns], exact = the 16 sums as Fractions, abs_sum = the 16 sums of |term| as Fractions, terms float64 [ns, 16])"""
    S = np.asarray(src, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(dst, np.float32).reshape(-1, 3)
    M = np.asarray(M, np.float64).reshape(-1)[:12].reshape(3, 4)
    P = np.stack([((M[a, 0] * S[:, 0] + M[a, 1] * S[:, 1]) + M[a, 2] * S[:, 2]) + M[a, 3] for a in range(3)], axis=1).astype(np.float32)
    idx, d2 = np.zeros(len(P), np.uint32), np.zeros(len(P), np.float32)
    step = max(1, (1 << 21) // len(T))
    for i0 in range(0, len(P), step):
        q = P[i0:i0 + step]
        dx, dy, dz = q[:, 0:1] - T[None, :, 0], q[:, 1:2] - T[None, :, 1], q[:, 2:3] - T[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        best = d.min(axis=1)
        idx[i0:i0 + step] = (d == best[:, None]).argmax(axis=1)          # the first index at the minimum
        d2[i0:i0 + step] = best
    s, t = P.astype(np.float64), T[idx].astype(np.float64)
    terms = np.concatenate([s, t, (s[:, :, None] * t[:, None, :]).reshape(-1, 9), d2.astype(np.float64)[:, None]], axis=1)
    scaled = np.ldexp(terms, SCALE)
    assert np.isfinite(scaled).all() and (scaled == np.rint(scaled)).all()
    exact = [Fraction(sum(int(v) for v in scaled[:, k]), 1 << SCALE) for k in range(16)]
    abs_sum = [Fraction(sum(abs(int(v)) for v in scaled[:, k]), 1 << SCALE) for k in range(16)]
    return dict(index=idx, exact=exact, abs_sum=abs_sum, terms=terms)
