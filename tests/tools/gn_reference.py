"""An independent reference for the Gauss-Newton tail (6x6 solve, rotation vector -> matrix, pose composition, K R K^-1, 3x3 inverse,
quaternion -> matrix), written from the published algorithms and the reference's host sources (ICPOdometry.cpp:68-186,
RGBDOdometry.cpp:213-231, 328-373, OdometryProvider.h:54-68, GroundTruthOdometry.cpp:42-74, KintinuousTracker.cpp:244-256).
It imports nothing from the package or the oracle.  Two layers:

  layer 1  exact / many-digit VALUES: A x = b over fractions.Fraction (doubles are rationals), exp([r]x) by mpmath at 100 digits,
           the 4x4 compositions, the inverse of a 3x3 matrix, K R K^-1, quaternion -> matrix in rationals;
  layer 2  the DECISIONS of Eigen's unblocked, diagonally pivoted LDL^T (Eigen/src/Cholesky/LDLT.h, 3.2.x after 3.2.0) run in exact
           arithmetic: the pivot order (largest remaining |diagonal|, first maximum wins), which entries of D fall under
           max|D| * eps and are dropped by solve(), the d == 0 guard on the column scaling -- and the x that follows from them.

mpmath is needed by rodrigues_mp() alone (imported there); everything else is the standard library, so a test that reads recorded
rotation matrices can run where mpmath is absent, and rodrigues_series() gives exp([r]x) for moderate angles in rationals (held against the
mpmath values by tests/test_gn_reference.py)."""
from fractions import Fraction as F

DBL_EPS = F(1, 2 ** 52)
DBL_MAX = F((2 ** 53 - 1) * 2 ** 971)
NEAR = F(1, 2 ** 40)      # a comparison closer than this (relative) is "within rounding of its threshold"


def frac(v):
    """The exact rational value of a float (or of a (hi, lo) pair of floats)."""
    if isinstance(v, F):
        return v
    if isinstance(v, (tuple, list)):
        return F(float(v[0])) + F(float(v[1]))
    return F(float(v))


def fmat(a, rows, cols):
    return [[frac(a[i][j]) for j in range(cols)] for i in range(rows)]


def hilo(v):
    """A rational or mpmath value as two floats whose sum carries ~106 bits."""
    if isinstance(v, F):
        hi = v.numerator / v.denominator   # int / int: correctly rounded
        lo = v - F(hi)
        return hi, lo.numerator / lo.denominator
    hi = float(v)
    return hi, float(v - hi)


# ---------------------------------------------------------------------------------------------------------------------------------
# layer 1
# ---------------------------------------------------------------------------------------------------------------------------------
def gauss_solve(A, B):
    """Exact solution X of A X = B (B: n x m) by Gauss-Jordan elimination over the rationals; None when A is singular."""
    n = len(A)
    M = [list(A[i]) + list(B[i]) for i in range(n)]
    for c in range(n):
        p = next((r for r in range(c, n) if M[r][c] != 0), None)
        if p is None:
            return None
        M[c], M[p] = M[p], M[c]
        inv = 1 / M[c][c]
        M[c] = [v * inv for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    return [row[n:] for row in M]


def solve_with_condition(A, b):
    """(x, kappa_inf(A)) exactly, or (None, None) for a singular A."""
    n = len(A)
    X = gauss_solve(A, [[b[i]] + [F(int(i == j)) for j in range(n)] for i in range(n)])
    if X is None:
        return None, None
    norm = lambda M: max(sum(abs(v) for v in row) for row in M)
    return [row[0] for row in X], norm(A) * norm([row[1:] for row in X])


def backward_error(A, x, b):
    """Normwise backward error |A x - b|_inf / (|A|_inf |x|_inf + |b|_inf), in rationals."""
    n = len(A)
    res = max(abs(sum(A[i][j] * x[j] for j in range(n)) - b[i]) for i in range(n))
    den = max(sum(abs(v) for v in row) for row in A) * max(abs(v) for v in x) + max(abs(v) for v in b)
    return res / den if den != 0 else F(0)


def matmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def transpose(A):
    return [list(r) for r in zip(*A)]


def inverse(A):
    return gauss_solve(A, [[F(int(i == j)) for j in range(len(A))] for i in range(len(A))])


def rigid(R, t):
    """[R | t; 0 0 0 1]"""
    return [list(R[i]) + [t[i]] for i in range(3)] + [[F(0), F(0), F(0), F(1)]]


def rodrigues_mp(r, digits=100):
    """exp([r]x) of a rotation vector given as three floats: a 3x3 list of mpmath numbers good to ~digits."""
    import mpmath
    with mpmath.workdps(digits):
        v = [mpmath.mpf(float(c)) for c in r]
        th2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
        if th2 == 0:
            return [[mpmath.mpf(int(i == j)) for j in range(3)] for i in range(3)]
        th = mpmath.sqrt(th2)
        a = mpmath.sin(th) / th                       # sin(theta) / theta
        h = mpmath.sin(th / 2)
        b = 2 * h * h / th2                           # (1 - cos(theta)) / theta^2 without the cancellation
        c = mpmath.cos(th)
        K = [[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]
        return [[c * int(i == j) + b * v[i] * v[j] + a * K[i][j] for j in range(3)] for i in range(3)]


def rodrigues_series(r, terms=40):
    """exp([r]x) over the rationals, for use where mpmath is absent: R = cos I + ((1 - cos) / theta^2) r r^T + (sin / theta) [r]x, and
    all three coefficients are power series in theta^2 = r . r, so no square root is taken.  r: three rationals with theta^2 <= 16, where
    the remainder after 40 terms is below 16^40 / 81! < 1e-70."""
    th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    assert th2 <= 16
    a = b = F(0)            # sin(theta) / theta = sum (-th2)^n / (2n + 1)!,  (1 - cos(theta)) / theta^2 = sum (-th2)^n / (2n + 2)!
    power, fact = F(1), 1   # (-th2)^n, (2n)!
    for n in range(terms):
        fact1 = fact * (2 * n + 1)
        fact2 = fact1 * (2 * n + 2)
        a += power / fact1
        b += power / fact2
        power, fact = power * -th2, fact2
    c = 1 - th2 * b
    K = [[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]
    return [[c * int(i == j) + b * r[i] * r[j] + a * K[i][j] for j in range(3)] for i in range(3)]


def compose(increments, start=None):
    """resultRt after `resultRt = currRt * resultRt` for every currRt = [R | t] of the list, in order (ICPOdometry.cpp:142-144)."""
    T = start if start is not None else [[F(int(i == j)) for j in range(4)] for i in range(4)]
    for R, t in increments:
        T = matmul(rigid(R, t), T)
    return T


def pose_from_increment(T, Rprev, tprev):
    """ICPOdometry.cpp:146-178: T_curr = [Rprev | tprev] * inverse([R | t]) with the Isometry3f inverse [R^T | -R^T t]."""
    R = [row[:3] for row in T[:3]]
    t = [T[i][3] for i in range(3)]
    Rt = transpose(R)
    tinv = [-sum(Rt[i][k] * t[k] for k in range(3)) for i in range(3)]
    Rc = matmul(Rprev, Rt)
    tc = [sum(Rprev[i][k] * tinv[k] for k in range(3)) + tprev[i] for i in range(3)]
    return Rc, tc


def pose_term_scale(T, Rprev, tprev):
    """The magnitude of the largest term of the sums that form Rcurr and tcurr (all products expanded)."""
    sR = max(abs(Rprev[i][k] * T[j][k]) for i in range(3) for j in range(3) for k in range(3))
    st = max([abs(Rprev[i][k] * T[j][k] * T[j][3]) for i in range(3) for j in range(3) for k in range(3)] + [abs(v) for v in tprev])
    return sR, st


def krk(T, fx, fy, cx, cy):
    """RGBDOdometry.cpp:213-231: Rt = resultRt^-1 (a general 4x4 inverse there), K R K^-1 and K t.  Also the largest terms."""
    K = [[fx, F(0), cx], [F(0), fy, cy], [F(0), F(0), F(1)]]
    Ti = inverse(T)
    R = [row[:3] for row in Ti[:3]]
    t = [[Ti[i][3]] for i in range(3)]
    Kinv = inverse(K)
    KRK = matmul(matmul(K, R), Kinv)
    Kt = [row[0] for row in matmul(K, t)]
    sK = [[max(abs(K[i][p] * R[p][q] * Kinv[q][j]) for p in range(3) for q in range(3)) for j in range(3)] for i in range(3)]
    st = [max(abs(K[i][p] * t[p][0]) for p in range(3)) for i in range(3)]
    return KRK, Kt, sK, st


def inverse33_with_scale(m):
    """Inverse of a 3x3 matrix and, per element, the magnitude that the rounding errors of the cofactor form (Eigen's
    compute_inverse_size3: cofactor / determinant) are relative to: the larger product of the cofactor, and the cofactor times the
    largest term of the determinant's sum over the determinant, both over |det|."""
    inv = inverse(m)
    cof = lambda i, j: (m[(i + 1) % 3][(j + 1) % 3] * m[(i + 2) % 3][(j + 2) % 3], m[(i + 1) % 3][(j + 2) % 3] * m[(i + 2) % 3][(j + 1) % 3])
    det = sum((cof(i, 0)[0] - cof(i, 0)[1]) * m[i][0] for i in range(3))
    dterm = max(abs((cof(i, 0)[0] - cof(i, 0)[1]) * m[i][0]) for i in range(3))
    scale = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            a, b = cof(j, i)    # element (i, j) of the inverse is cofactor (j, i) / det
            scale[i][j] = max(abs(a), abs(b), abs(a - b) * dterm / abs(det)) / abs(det)
    return inv, scale


def quat_matrix(qx, qy, qz, qw):
    """Eigen's Quaternion::toRotationMatrix (no normalisation: KintinuousTracker.cpp:244-256 rotates by the quaternion as read)."""
    return [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
            [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
            [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]]


def ground_truth_pose(A, B, last):
    """GroundTruthOdometry.cpp:56-72 on 4x4 rationals: last * M^-1 * (A^-1 * B) * M, A^-1 as the Isometry3f inverse
    [R^T | -R^T t].  Returns the 4x4 product and the magnitude of its largest expanded term per element."""
    M = [[F(v) for v in row] for row in ([0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1])]
    Ra = transpose([row[:3] for row in A[:3]])
    Ai = rigid(Ra, [-sum(Ra[i][k] * A[k][3] for k in range(3)) for i in range(3)])
    Mi = inverse(M)
    LM = matmul(last, Mi)
    out = matmul(matmul(LM, matmul(Ai, B)), M)
    r4 = range(4)
    scale = [[max(abs(LM[i][a] * Ai[a][c] * B[c][e] * M[e][j]) for a in r4 for c in r4 for e in r4) for j in r4] for i in r4]
    return out, scale


# ---------------------------------------------------------------------------------------------------------------------------------
# layer 2: Eigen's LDLT<Matrix<double, 6, 6>>::compute() and solve() in exact arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def _near(a, b):
    return a != b and abs(a - b) <= NEAR * max(abs(a), abs(b))


def ldlt_eigen(A, b):
    """Returns a dict: order (the original index standing at each pivot position), transpositions, D, dropped (per pivot position),
    dropped_vars (per original unknown), x, undecidable (a pivot comparison or a |d| > tol test within 2^-40 relative of equality),
    min_pivot_ratio (min |D| / max |D|, 0 for an all-zero D)."""
    n = len(A)
    M = [list(row) for row in A]
    order = list(range(n))
    trans = []
    undecidable = False
    for k in range(n):
        # the largest remaining diagonal magnitude; maxCoeff keeps the FIRST maximum
        p, big = k, abs(M[k][k])
        for i in range(k + 1, n):
            v = abs(M[i][i])
            undecidable |= _near(v, big)
            if v > big:
                p, big = i, v
        for i in range(k, n):
            undecidable |= _near(abs(M[i][i]), big)
        trans.append(p)
        if p != k:
            M[k], M[p] = M[p], M[k]
            for row in M:
                row[k], row[p] = row[p], row[k]
            order[k], order[p] = order[p], order[k]
        # left-looking step: d_k = a_kk - sum_j l_kj^2 d_j, the column below it likewise, scaled by d_k unless that is zero
        d = M[k][k] - sum(M[k][j] * M[k][j] * M[j][j] for j in range(k))
        M[k][k] = d
        for i in range(k + 1, n):
            s = M[i][k] - sum(M[i][j] * M[k][j] * M[j][j] for j in range(k))
            M[i][k] = s / d if d != 0 else s
    D = [M[i][i] for i in range(n)]
    y = list(b)
    for k in range(n):
        if trans[k] != k:
            y[k], y[trans[k]] = y[trans[k]], y[k]
    for i in range(n):
        y[i] -= sum(M[i][j] * y[j] for j in range(i))
    maxd = max(abs(v) for v in D)
    tol = max(maxd * DBL_EPS, 1 / DBL_MAX)
    dropped = []
    for i in range(n):
        undecidable |= _near(abs(D[i]), tol)
        keep = abs(D[i]) > tol
        dropped.append(not keep)
        y[i] = y[i] / D[i] if keep else F(0)
    for i in range(n - 1, -1, -1):
        y[i] -= sum(M[j][i] * y[j] for j in range(i + 1, n))
    for k in range(n - 1, -1, -1):
        if trans[k] != k:
            y[k], y[trans[k]] = y[trans[k]], y[k]
    dropped_vars = [False] * n
    for pos in range(n):
        dropped_vars[order[pos]] = dropped[pos]
    return {"order": order, "transpositions": trans, "D": D, "dropped": dropped, "dropped_vars": dropped_vars, "x": y,
            "undecidable": bool(undecidable), "min_pivot_ratio": (min(abs(v) for v in D) / maxd) if maxd != 0 else F(0)}
