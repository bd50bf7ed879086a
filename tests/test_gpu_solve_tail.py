"""The lane-parallel Gauss-Newton tail (kt_solve_and_update_wave) where it no longer spells the serial form out: one sincos() for the
separate cos() and sin() of cv::Rodrigues, and a pivot order read from ballots of the lanes' ranks.  Both device forms run on the same
input through kt_debug_solve_check (one wave per case) and must agree in every bit of resultRt, Rcurr and tcurr (a NaN is a NaN).

Angles.  A rotation vector goes in as b over an identity A through the joint combination b_rgbd + 10 b_icp, as in
tests/test_gpu_solve.py, which forms a double from two floats.  Two floats carry 48 bits, so not every double can be formed that way
(k pi / 4 plus one ulp cannot): where the wanted double has no such pair, the unknown is formed as b / d over a diagonal A instead -- one
correctly rounded division in either form, searched over d on the host until fl(b / d) IS the wanted double.  Either way the test knows
the double the device forms, and that double is what the reference is evaluated at.  theta runs over 0, the two sides of DBL_EPSILON,
1e-12 ... 1e-2, k pi / 4 (k = 1 ... 16) with 0, +-1 and +-2 ulps added, powers of two through the large-argument reduction and on to
2^240 (b is a float: from 2^127 on the whole system is scaled by 2^-120, which reaches 2^247), +-infinity and NaN; each along +-x, +-y,
+-z and along two directions of mixed signs.  Finite results also meet the bars of tests/tools/gn_checks.py (check_rotation, check_step)
against mpmath at 100 digits.

Pivot orders.  All 4683 weak orderings of six diagonal entries (the 720 strict orders, and every multiplicity pattern of ties -- 2+1+1+1+1,
2+2+1+1, 3+3, ... 6 -- in every position and in every order of the tied groups) on a diagonally dominant system, once with a positive
diagonal and once with signs (the pivot is chosen by magnitude: +v ties with -v)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from kintinuous_amd import abi

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
BIG = 2.0 ** -120      # the scale of the whole system where the unknown is 2^127 or more (b is a float)

# the case layout and the helpers of tests/test_gpu_solve.py
CASE = np.dtype([("packed", np.float32, 32), ("packed2", np.float32, 32), ("resultRt", np.float64, 16), ("posef", np.float32, 12),
                 ("joint", np.int32), ("pad", np.int32, 3)])


def _slot(i, j):   # reduce.cu:401-418: rows i = 0..5, columns j = i..6
    return i * 7 - (i * (i - 1)) // 2 + (j - i)


def _pack(A, b):
    out = np.zeros(32, np.float32)
    for i in range(6):
        for j in range(i, 6):
            out[_slot(i, j)] = A[i, j]
        out[_slot(i, 6)] = b[i]
    return out


def _rot(rng, scale):
    w = rng.normal(size=3) * scale
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th ** 2) * (K @ K)


def _gn_checks():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "gn_checks.py")
    spec = importlib.util.spec_from_file_location("gn_checks", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(cs):
    ctx = abi.Ctx(0)
    layout = (C.c_int * 5)()
    abi._chk(abi.lib().kt_debug_solve_check(ctx.h, 0, None, None, None, layout))
    size, o_rt, o_R, o_t, case_size = list(layout)
    assert case_size == CASE.itemsize
    n = len(cs)
    out = {"serial": np.zeros((n, size), np.uint8), "wave": np.zeros((n, size), np.uint8)}
    abi._chk(abi.lib().kt_debug_solve_check(ctx.h, n, cs.ctypes.data_as(C.c_void_p), out["serial"].ctypes.data_as(C.c_void_p),
                                            out["wave"].ctypes.data_as(C.c_void_p), layout))
    ctx.close()
    return {f: (o[:, o_rt:o_rt + 128].copy().view(np.float64).reshape(n, 4, 4), o[:, o_R:o_R + 36].copy().view(np.float32).reshape(n, 3, 3),
                o[:, o_t:o_t + 12].copy().view(np.float32).reshape(n, 3)) for f, o in out.items()}


def _assert_same_bits(res, label):
    for name, a, b in zip(("resultRt", "Rcurr", "tcurr"), res["serial"], res["wave"]):
        bits = np.uint64 if a.dtype == np.float64 else np.uint32
        same = (np.isnan(a) & np.isnan(b)) | (a.view(bits) == b.view(bits))
        bad = np.nonzero(~np.all(same.reshape(len(a), -1), axis=1))[0]
        assert bad.size == 0, (name, len(bad), [label(int(k)) for k in bad[:5]], a[bad[0]], b[bad[0]])


# ---------------------------------------------------------------------------------------------------------------------------------
# angles
# ---------------------------------------------------------------------------------------------------------------------------------
def _two_float(v):
    """(b1, b2) with b1 + 10 b2 == v in double arithmetic, or None"""
    with np.errstate(over="ignore", invalid="ignore"):
        b1 = np.float32(v)
        if not np.isfinite(v):
            return b1, np.float32(0)
        if not np.isfinite(b1):
            return None
        b2 = np.float32((v - np.float64(b1)) / 10.0)
        return (b1, b2) if np.float64(b1) + 10.0 * np.float64(b2) == v else None


def _nearest_two_float(v):
    b1 = np.float32(v)
    b2 = np.float32((v - np.float64(b1)) / 10.0)
    return b1, b2


def _by_division(v, rng):
    """(d, b1, b2): a float d in [1, 2) and two floats with fl((b1 + 10 b2) / d) == v"""
    for _ in range(4000):
        d = np.float32(1.0 + rng.integers(1, 2 ** 23) * 2.0 ** -23)
        b1, b2 = _nearest_two_float(v * np.float64(d))
        if (np.float64(b1) + 10.0 * np.float64(b2)) / np.float64(d) == v:
            return d, b1, b2
    raise AssertionError(("no b / d forms", v))


def _thetas():
    th = [0.0, np.nextafter(EPS, 0.0), EPS, np.nextafter(EPS, 1.0)]
    th += [10.0 ** -e for e in range(12, 1, -1)]
    for k in range(1, 17):
        base = k * np.pi / 4
        seq = [base]
        for _ in range(2):
            seq = [np.nextafter(seq[0], 0.0)] + seq + [np.nextafter(seq[-1], np.inf)]
        th += seq
    th += [2.0 ** k for k in list(range(0, 72)) + [100, 126, 127, 128, 200, 240]]      # (b is a float: 2^247 is the largest unknown b / 2^-120 forms)
    th += [np.inf, -np.inf, np.nan]
    return [float(v) for v in th]


DIRECTIONS = [("+x", (1, 0, 0)), ("-x", (-1, 0, 0)), ("+y", (0, 1, 0)), ("-y", (0, -1, 0)), ("+z", (0, 0, 1)), ("-z", (0, 0, -1)),
              ("mixed a", (2 / 7, -3 / 7, 6 / 7)), ("mixed b", (-4 / 9, 7 / 9, -4 / 9))]


def _angle_cases():
    rng = np.random.default_rng(20250117)
    eye12 = np.r_[np.eye(3).reshape(9), np.zeros(3)].astype(np.float32)
    state = np.eye(4)
    state[:3, :3] = _rot(rng, 0.05)
    state[:3, 3] = rng.normal(size=3) * 0.05
    prev = np.r_[_rot(rng, 1.0).astype(np.float32).reshape(9), (rng.normal(size=3) * 3).astype(np.float32)].astype(np.float32)
    t_inc = np.array([0.0078125, -0.015625, 0.01171875])       # floats: exact in b
    recs, what = [], []
    for theta in _thetas():
        for dname, dvec in DIRECTIONS:
            axis = sum(1 for c in dvec if c != 0) == 1
            big = np.isfinite(theta) and theta >= 2.0 ** 127
            diag = np.full(6, BIG if big else 1.0, np.float32)
            b1, b2 = np.zeros(6, np.float32), np.zeros(6, np.float32)
            x = np.zeros(6)
            if not big:
                b1[:3] = t_inc
                x[:3] = t_inc
            for k, c in enumerate(dvec):
                if c == 0:
                    continue
                with np.errstate(invalid="ignore", over="ignore"):
                    v = np.float64(theta) * np.float64(c)
                    pair = _two_float(v * np.float64(diag[3 + k]))
                    if pair is None and axis:
                        diag[3 + k], b1[3 + k], b2[3 + k] = _by_division(v, rng)
                    else:
                        b1[3 + k], b2[3 + k] = pair if pair is not None else _nearest_two_float(v * np.float64(diag[3 + k]))
                    x[3 + k] = (np.float64(b1[3 + k]) + 10.0 * np.float64(b2[3 + k])) / np.float64(diag[3 + k])   # what either form computes
                assert not axis or x[3 + k] == v or np.isnan(v), (theta, dname)
            for st, pv in ((np.eye(4), eye12), (state, prev)):
                c = np.zeros((), CASE)
                c["packed"], c["packed2"], c["joint"] = _pack(np.diag(diag), b1), _pack(np.zeros((6, 6)), b2), 1
                c["resultRt"], c["posef"] = st.reshape(16), pv
                recs.append(c)
                what.append((theta, dname, x.copy(), st, pv))
    return np.array(recs, CASE), what


@pytest.fixture(scope="module")
def angle_run():
    cs, what = _angle_cases()
    assert 2000 < len(cs) < 6000
    return what, _run(cs)


def test_one_sincos_gives_the_bits_of_cos_and_sin(angle_run):
    what, res = angle_run
    _assert_same_bits(res, lambda k: what[k][:2])
    rt = res["serial"][0]
    finite = np.all(np.isfinite(rt.reshape(len(rt), -1)), axis=1)
    theta = np.array([w[0] for w in what])
    # the comparison is not NaN against NaN where it matters, and the NaN cases are NaNs
    assert np.all(finite[np.isfinite(theta) & (theta < 1e150)]) and not np.any(finite[~np.isfinite(theta)])
    # the increments were formed as intended: resultRt's translation over the identity state IS x[0:3], and a rotation about +z by pi / 2
    # has R[0][1] = -1 (the quadrant and the sign of the shared reduction)
    for k, w in enumerate(what):
        if w[1] == "+z" and w[0] == 2 * np.pi / 4 and np.array_equal(w[3], np.eye(4)):
            assert abs(rt[k, 0, 1] + 1.0) < 1e-15 and abs(rt[k, 1, 0] - 1.0) < 1e-15 and abs(rt[k, 0, 0]) < 1e-15
            assert np.array_equal(rt[k, :3, 3], w[2][:3])
            break
    else:
        raise AssertionError("no quarter turn about +z in the table")


def test_finite_angles_meet_the_bars_of_the_reference(angle_run):
    import mpmath
    gn = _gn_checks()
    what, res = angle_run
    rows = [k for k, w in enumerate(what) if np.all(np.isfinite(w[2])) and np.all(np.isfinite(res["serial"][0][k]))]
    assert len(rows) > 0.8 * len(what)
    T = {"r_vec": np.array([what[k][2][3:] for k in rows]), "r_t": np.array([what[k][2][:3] for k in rows]),
         "r_band": np.zeros(len(rows), np.int32), "r_R": np.zeros((len(rows), 9, 2))}
    with mpmath.workdps(100):
        for row, k in enumerate(rows):
            R = gn.G.rodrigues_mp(what[k][2][3:])
            for e, v in enumerate(v for line in R for v in line):
                hi = float(v)
                T["r_R"][row, e] = hi, float(v - mpmath.mpf(hi))
    worst = {"rot": 0.0, "rt": 0.0, "Rcurr": 0.0, "tcurr": 0.0}
    steps = 0
    for form, (rt, Rc, tc) in res.items():
        for row, k in enumerate(rows):
            theta, dname, x, state, prev = what[k]
            bar, th = gn.rotation_bar(x[3:])
            if np.array_equal(state, np.eye(4)):
                worst["rot"] = max(worst["rot"], gn.check_rotation(T, row, rt[k, :3, :3], (form, theta, dname)) * 8 * gn.U / bar)
            if th < 10:
                e = gn.check_step(T, row, state, rt[k], Rc[k], tc[k], prev, (form, theta, dname))
                worst["rt"], worst["Rcurr"], worst["tcurr"] = max(worst["rt"], e[0]), max(worst["Rcurr"], e[1]), max(worst["tcurr"], e[2])
                steps += 1
    print("worst, in units of the bars' u (rot: of 8 u max(1, theta)):", {k: round(v, 3) for k, v in worst.items()}, "steps checked:", steps)
    assert steps > 1000


# ---------------------------------------------------------------------------------------------------------------------------------
# pivot orders
# ---------------------------------------------------------------------------------------------------------------------------------
def _weak_orderings():
    """every assignment of levels 0 .. m - 1 (each used) to six positions: 4683 of them, 720 with m == 6"""
    out = [p for p in itertools.product(range(6), repeat=6) if set(p) == set(range(max(p) + 1))]
    assert len(out) == 4683 and sum(1 for p in out if max(p) == 5) == 720
    return out


def _pivot_cases():
    rng = np.random.default_rng(20250118)
    levels = np.array([1.5, 2.25, 3.0, 4.5, 7.0, 11.0], np.float32)
    orders = _weak_orderings()
    patterns = {tuple(sorted(np.bincount(p).tolist(), reverse=True)) for p in orders}
    assert len(patterns) == 11            # the partitions of 6: 1+1+1+1+1+1, 2+1+1+1+1, 2+2+1+1, 2+2+2, 3+1+1+1, 3+2+1, 3+3, 4+1+1, 4+2, 5+1, 6
    recs, what = [], []
    for signed in (False, True):
        for p in orders:
            off = (rng.uniform(-0.05, 0.05, size=(6, 6))).astype(np.float32)
            A = np.triu(off, 1) + np.triu(off, 1).T          # row sums of |off-diagonal| <= 0.25 < 1.5: diagonally dominant
            d = levels[list(p)].copy()
            if signed:
                d *= rng.choice(np.array([-1, 1], np.float32), size=6)
            A[np.arange(6), np.arange(6)] = d
            b = rng.normal(size=6).astype(np.float32) * np.float32(0.01)
            c = np.zeros((), CASE)
            c["packed"] = _pack(A.astype(np.float32), b)
            T = np.eye(4)
            T[:3, :3] = _rot(rng, 0.05); T[:3, 3] = rng.normal(size=3) * 0.05
            c["resultRt"] = T.reshape(16)
            c["posef"][:9] = _rot(rng, 1.0).astype(np.float32).reshape(9)
            c["posef"][9:] = (rng.normal(size=3) * 3).astype(np.float32)
            recs.append(c)
            what.append((signed, p))
    return np.array(recs, CASE), what


def test_every_pivot_order_and_every_tie_pattern():
    cs, what = _pivot_cases()
    res = _run(cs)
    _assert_same_bits(res, lambda k: what[k])
    rt = res["serial"][0]
    assert np.all(np.isfinite(rt)) and np.any(rt[:, :3, 3] != 0)
