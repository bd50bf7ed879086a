"""The checks and bars that tests/test_gn_reference.py (oracle C and host ABI, on the CPU) and tests/test_gpu_solve.py (both device forms)
apply against tests/tools/gn_reference.py through the table tests/golden/gn_cases_v1.npz.  The bars are stated in the docstring of
tests/test_gn_reference.py; u = 2^-53.  Needs numpy and the standard library only."""
import os
import sys
from fractions import Fraction as F

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import gn_reference as G  # noqa: E402

TABLE_PATH = os.path.join(ROOT, "tests", "golden", "gn_cases_v1.npz")

U = 2.0 ** -53
UF = 2.0 ** -24
LAPACK_FWD, LAPACK_BWD = 1.70, 1.19          # numpy.linalg.solve on classes 1 and 5 of the table, units of kappa_inf u and of u
C_FWD, C_BWD = 8 * LAPACK_FWD, 8 * LAPACK_BWD
DENORMAL_ATOL = 16 * 2.0 ** -1074
EPS2 = F(1, 2 ** 104)                        # DBL_EPSILON^2


def table():
    with np.load(TABLE_PATH) as z:
        return {k: z[k] for k in z.files}


def _fr(a):
    return [G.frac(float(v)) for v in np.asarray(a, np.float64).reshape(-1)]


def _mat(a, n, m):
    v = _fr(a)
    return [v[i * m:(i + 1) * m] for i in range(n)]


def _hl(a):
    """(..., 2) hi / lo pairs -> a flat list of rationals"""
    a = np.asarray(a, np.float64).reshape(-1, 2)
    return [F(float(h)) + F(float(l)) for h, l in a]


def solve_error_units(T, i, x):
    """Forward error in units of kappa_inf u |x|_inf and backward error in units of u of a computed solution of system i (classes 1, 5).
    Returns (fwd, bwd, scale): scale = |x_exact|_inf; fwd is None where x_exact == 0 or sits in the denormals."""
    xe = _hl(T["s_x"][i])
    xf = _fr(x)
    scale = max(abs(v) for v in xe)
    err = max(abs(a - b) for a, b in zip(xf, xe))
    A, b = _mat(T["s_A"][i], 6, 6), _fr(T["s_b"][i])
    bwd = float(G.backward_error(A, xf, b) / F(U)) if any(v != 0 for v in xf) else 0.0
    if scale == 0:
        assert err == 0, (i, x)
        return None, bwd, 0.0
    if float(scale) < 1e-290:
        assert float(err) <= C_FWD * float(T["s_kappa"][i]) * U * float(scale) + DENORMAL_ATOL, (i, x)
        return None, None, float(scale)   # a right-hand side in the denormals: A x rounds at 2^-1074, relative measures do not apply
    return float(err / scale) / (float(T["s_kappa"][i]) * U), bwd, float(scale)


def check_solve_values(T, i, x, what):
    fwd, bwd, _ = solve_error_units(T, i, x)
    assert np.all(np.isfinite(x)), (what, i)
    if fwd is not None:
        assert fwd <= C_FWD, (what, i, int(T["s_cls"][i]), int(T["s_kind"][i]), "forward error", fwd, "x kappa u; kappa", float(T["s_kappa"][i]))
    if bwd is not None:
        assert bwd <= C_BWD, (what, i, int(T["s_cls"][i]), int(T["s_kind"][i]), "backward error", bwd, "u")
    return fwd, bwd


def check_solve_decisions(T, i, x, what, unknowns=range(6)):
    """Classes 2-4: the computed x (its entries `unknowns`) shows layer 2's pivot order and dropped set: an unknown that layer 2 leaves
    exactly 0 (a zero row, a dropped decoupled pivot) is exactly 0, and x agrees with layer 2's x -- except in class 4 where layer 2's factor
    has a pivot below 1e-8 max|D| (no accuracy is claimed there; the exact zeros still show the drops).  Returns False for an undecidable
    case, which is skipped."""
    cls = int(T["s_cls"][i])
    if T["s_undec"][i]:
        return False
    x2 = np.array([float(v) for v in _hl(T["s_x"][i])])
    compare = not (cls == 4 and not T["s_minpiv"][i] >= 1e-8)
    tol = (1e-6 if cls == 4 else 1e-9) * np.abs(x2).max()
    decoupled = [k for k in range(6) if not np.any(np.delete(T["s_A"][i][k], k))]
    for k in unknowns:
        if compare:
            assert abs(x[k] - x2[k]) <= tol, (what, i, cls, int(T["s_kind"][i]), k, x, x2, list(T["s_order"][i]), list(T["s_drop"][i]))
        if x2[k] == 0.0 and (T["s_zero"][i][k] or k in decoupled or not np.any(x2)):
            assert x[k] == 0.0, (what, i, cls, int(T["s_kind"][i]), k, x, list(T["s_drop"][i]))
        elif k in decoupled and not T["s_drop"][i][k]:      # a kept decoupled pivot: x = b / d, one rounding
            assert abs(x[k] - x2[k]) <= 4 * U * abs(x2[k]), (what, i, cls, k, x, x2)
    return True


def rotation_bar(r):
    theta = float(np.sqrt(float(sum(v * v for v in _fr(r)))))
    return 8 * U * max(1.0, theta if theta >= 10 else 1.0), theta


def check_rotation(T, row, R, what):
    """R (3x3 doubles) against the mpmath value of exp([r]x) for row `row` of the rotation table.  Returns the worst error in units of u."""
    r = T["r_vec"][row]
    bar, theta = rotation_bar(r)
    Rf = _fr(R)
    want = _hl(T["r_R"][row])
    err = max(abs(a - b) for a, b in zip(Rf, want))
    assert float(err) <= bar, (what, row, int(T["r_band"][row]), theta, float(err) / U, "u; bar", bar / U)
    M = [Rf[0:3], Rf[3:6], Rf[6:9]]
    orth = max(abs(v - int(i == j)) for i, rowv in enumerate(G.matmul(M, G.transpose(M))) for j, v in enumerate(rowv))
    assert float(orth) <= 16 * U, (what, row, theta, float(orth) / U)
    th2 = sum(v * v for v in _fr(r))
    if th2 < EPS2 * (1 - G.NEAR):
        assert np.array_equal(np.asarray(R, np.float64).reshape(3, 3), np.eye(3)), (what, row, R)
    return float(err) / U


def exact_increment(T, row):
    w = _hl(T["r_R"][row])
    return [w[0:3], w[3:6], w[6:9]], _fr(T["r_t"][row])


def check_step(T, row, T_in, rt_out, Rc, tc, prev, what, k=1, T_exact=None):
    """One `resultRt = [R | t] resultRt` and the float pose that follows.  T_in: the 4x4 doubles that went in; with T_exact (the exact product
    of the chain so far, k compositions) the accumulated bar is applied against it instead."""
    R, t = exact_increment(T, row)
    want = T_exact if T_exact is not None else G.matmul(G.rigid(R, t), _mat(T_in, 4, 4))
    got = _mat(rt_out, 4, 4)
    tnorm = float(np.sqrt(float(sum(want[i][3] ** 2 for i in range(3)))))
    bar = k * 16 * U * max(1.0, tnorm)
    _, theta = rotation_bar(T["r_vec"][row])
    assert theta < 10
    err = max(abs(got[i][j] - want[i][j]) for i in range(4) for j in range(4))
    assert float(err) <= bar, (what, row, k, float(err) / U, "u; bar", bar / U)
    # the float part, from the float inputs the code itself formed: float(resultRt), Rprev, tprev
    Tf = _mat(np.asarray(rt_out, np.float64).astype(np.float32), 4, 4)
    Rp, tp = _mat(prev[:9], 3, 3), _fr(prev[9:])
    Rw, tw = G.pose_from_increment(Tf, Rp, tp)
    sR, st = G.pose_term_scale(Tf, Rp, tp)
    eR = max(abs(a - b) for a, b in zip(_fr(Rc), [v for rowv in Rw for v in rowv]))
    et = max(abs(a - b) for a, b in zip(_fr(tc), tw))
    assert float(eR) <= 8 * UF * float(sR), (what, row, "Rcurr", float(eR) / UF / float(sR))
    assert float(et) <= 8 * UF * float(st), (what, row, "tcurr", float(et) / UF / float(st))
    return float(err) / U, float(eR) / UF / float(sR), float(et) / UF / float(st)


def host_chain(T, c, pose_update):
    """The chain c through pose_update(x, resultRt, Rprev, tprev) -> (resultRt', Rcurr, tcurr); yields what check_step needs per step."""
    state = np.eye(4)
    exact = None
    prev = T["c_prev"][c]
    for k in range(int(T["c_len"][c])):
        row = int(T["c_start"][c]) + k
        x = np.r_[T["r_t"][row], T["r_vec"][row]]
        new, Rc, tc = pose_update(x, state, prev[:9], prev[9:])
        R, t = exact_increment(T, row)
        exact = G.compose([(R, t)], exact)
        yield row, k + 1, state, new, Rc, tc, prev, exact
        state = new
