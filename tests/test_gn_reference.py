"""The Gauss-Newton tail -- the 6x6 solve (Eigen's pivoted LDL^T restated), cv::Rodrigues restated, the resultRt composition, the float pose
update, K R K^-1, the 3x3 float inverse, the trajectory poses -- against tests/tools/gn_reference.py: exact rational values, mpmath rotation
matrices and Eigen's decisions taken in exact arithmetic.  The oracle's C functions and the kt_host_* ABI are the same restatement typed
twice and are otherwise compared with each other only; a slip they share is caught here.

The table is tests/golden/gn_cases_v1.npz (tests/golden/make_gn_cases.py).  The checks themselves live in tests/tools/gn_checks.py, shared with
tests/test_gpu_solve.py, which puts both device forms through the same table with the same bars.

Bars.  u = 2^-53.
  solve, classes 1 and 5 (SPD): forward error <= C_FWD kappa_inf(A) u, normwise backward error <= C_BWD u, both evaluated in rationals.  C is
      8 x the largest constant LAPACK (numpy.linalg.solve) shows on the same table: measured 1.70 (forward) and 1.19 (backward), hence
      C_FWD = 13.6, C_BWD = 9.52  (test_lapack_constants_are_the_measured_ones re-measures).
  decisions, classes 2-4: x against layer 2's x -- classes 2 and 3 to 1e-9 of |x|_inf (their regular part is a J^T J of >= 60 unit-normal
      rows or diagonally dominant: rounding moves x by ~1e-15, another pivot order or drop set by O(1)), unknowns of zero rows exactly 0;
      class 4 to 1e-6 where layer 2's factor has no pivot below 1e-8 max|D|.
  Rodrigues: 8 u per element for theta < 10, 8 u theta beyond; R R^T - I below 16 u; exactly I below the theta < DBL_EPSILON branch.
  resultRt after k compositions: k 16 u max(1, |t|);  Rcurr, tcurr, krkinv, kt, mat33_inverse, trajectory / ground-truth poses:
      8 2^-24 x the largest term of the sum that forms the element, against the rational value of the same float inputs."""
import importlib.util
import os
from fractions import Fraction as F

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


K = _load("gn_checks", os.path.join(ROOT, "tests", "tools", "gn_checks.py"))
G = K.G
TABLE_PATH = K.TABLE_PATH
U = K.U
UF = K.UF
LAPACK_FWD = K.LAPACK_FWD
LAPACK_BWD = K.LAPACK_BWD
C_FWD = K.C_FWD
C_BWD = K.C_BWD
table = K.table
_fr = K._fr
_mat = K._mat
_hl = K._hl
solve_error_units = K.solve_error_units
check_solve_values = K.check_solve_values
check_solve_decisions = K.check_solve_decisions
rotation_bar = K.rotation_bar
check_rotation = K.check_rotation
exact_increment = K.exact_increment
check_step = K.check_step
host_chain = K.host_chain


# ---------------------------------------------------------------------------------------------------------------------------------
# the forms that run on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _forms(oracle_mod):
    from kintinuous_amd import abi
    return {"oracle": (oracle_mod.ldlt_solve6, oracle_mod.rodrigues, oracle_mod.mat33_inverse),
            "host ABI": (abi.host_ldlt_solve6, abi.host_rodrigues, abi.host_mat33_inverse)}


def test_table_covers_every_class():
    """Every class of the issue is populated, per kind; the share of systems whose decisions sit within rounding of a threshold is at most
    2 % per class; classes 1 and 5 are SPD with nothing dropped; kappa_inf of class 1 spans 1e0 .. 1e14."""
    T = table()
    cls, kind = T["s_cls"], T["s_kind"]
    kinds = {1: 4, 2: 7, 3: 4, 4: 3, 5: 5}
    for c, nk in kinds.items():
        m = cls == c
        assert m.sum() >= 200, (c, int(m.sum()))
        assert set(kind[m].tolist()) == set(range(nk)), (c, set(kind[m].tolist()))
        assert T["s_undec"][m].mean() <= 0.02, (c, float(T["s_undec"][m].mean()))
    spd = (cls == 1) | (cls == 5)
    assert T["s_spd"][spd].all() and T["s_nonsing"][spd].all() and not T["s_drop"][spd].any()
    k1 = T["s_kappa"][cls == 1]
    for lo, hi in ((1, 1e2), (1e2, 1e5), (1e5, 1e8), (1e8, 1e11), (1e11, 1e14)):
        assert ((k1 >= lo) & (k1 < hi)).sum() >= 5, (lo, hi, int(((k1 >= lo) & (k1 < hi)).sum()))
    sing = (cls == 2) & (kind < 6)
    assert not T["s_nonsing"][sing].any() and T["s_drop"][sing].any(axis=1).all()
    rank = 6 - T["s_drop"][sing].sum(axis=1)
    assert set(rank.tolist()) == set(range(6))                                     # all zero, rank 1 .. 5
    tiny = (cls == 2) & (kind == 6)                                                # a nonzero pivot under / over max|D| eps
    assert T["s_nonsing"][tiny].all() and (T["s_drop"][tiny].sum(axis=1) == 1).sum() >= 10 and (T["s_drop"][tiny].sum(axis=1) == 0).sum() >= 10
    assert (~T["s_spd"][cls == 4]).all()
    assert (T["s_minpiv"][(cls == 4) & (kind < 2)] >= 1e-8).mean() > 0.9            # the 1e-6 comparison is made on nearly all of kinds 0, 1
    far = np.nonzero((cls == 4) & (kind == 2))[0]                                   # max|D| far above the first pivot, a pivot in between
    assert len(far) >= 40 and T["s_f32"][far].all()
    between = 0
    for i in far:
        l2 = G.ldlt_eigen(G.fmat(T["s_A"][i], 6, 6), [G.frac(v) for v in T["s_b"][i]])
        d0, dmax = abs(l2["D"][0]), max(abs(d) for d in l2["D"])
        assert dmax > 1000 * d0
        between += sum(1 for d, dr in zip(l2["D"], l2["dropped"]) if dr and abs(d) > G.DBL_EPS * d0 * 8)
    assert between >= 15          # dropped under max|D| eps, yet well above eps times the first pivot
    t3 = T["s_A"][(cls == 3) & (kind == 2)]
    assert all((np.diag(A) > 0).any() and (np.diag(A) < 0).any() for A in t3)       # ties between a positive and a negative diagonal
    assert T["s_drop"][(cls == 3) & (kind == 3)].sum(axis=1).min() == 1             # a tie decides which duplicate is dropped
    k5 = T["s_A"][(cls == 5)]
    mags = np.log10(np.abs(k5).reshape(len(k5), -1).max(axis=1))
    assert mags.min() < -150 and mags.max() > 150
    b5 = np.abs(T["s_b"][cls == 5])
    assert ((b5 > 0) & (b5 < 2.3e-308)).any() and (b5.max(axis=1) == 0).any()
    # every device-eligible system is float32-representable and has its partner
    e = T["s_f32"]
    assert np.array_equal(T["s_A"][e].astype(np.float32).astype(np.float64), T["s_A"][e])
    assert np.array_equal(T["s_b"][e].astype(np.float32).astype(np.float64), T["s_b"][e])
    assert (T["s_pair"][e] >= 0).all() and np.array_equal(T["s_pair"][T["s_pair"][e]], np.nonzero(e)[0])
    # class 6: 45 vectors per theta band, a third of them along a coordinate axis; class 7: three chains of every length 1 .. 19
    n6 = int(T["n6"])
    assert np.bincount(T["r_band"][:n6], minlength=7).tolist() == [45] * 7
    assert ((T["r_vec"][:n6] != 0).sum(axis=1) <= 1).sum() >= 7 * 15
    th = np.linalg.norm(T["r_vec"][:n6], axis=1)
    eps = 2.0 ** -52
    assert (th[T["r_band"][:n6] == 0] < eps).sum() >= 10 and (th[T["r_band"][:n6] == 0] >= eps).sum() >= 10
    assert np.abs(th[T["r_band"][:n6] == 3] - np.pi).max() < 1e-9 and th.max() > 5e5
    assert np.bincount(T["c_len"], minlength=20).tolist() == [0] + [3] * 19
    assert np.linalg.norm(T["c_prev"][:, 9:], axis=1).max() > 9 and len(T["k_T"]) == len(T["m_in"]) == len(T["q_pose7"]) == len(T["g_pose"]) == 200
    assert (T["q_pose7"][:, 6] < 0).sum() >= 100 and (np.abs(np.linalg.norm(T["q_pose7"][:, 3:], axis=1) - 1) > 0.1).sum() >= 100


def test_table_is_what_the_script_generates():
    """The committed file cannot drift from make_gn_cases.py: the inputs are regenerated in full, the expected values for a sample."""
    pytest.importorskip("mpmath")
    mk = _load("make_gn_cases", os.path.join(ROOT, "tests", "golden", "make_gn_cases.py"))
    T = table()
    g = mk.inputs()
    for k, v in g.items():
        assert np.array_equal(np.asarray(v), T[k]), k
    for i in range(0, len(T["s_cls"]), 17):
        e = mk.expected_solve(T["s_A"][i], T["s_b"][i])
        for name in ("x", "kappa", "order", "drop", "undec", "nonsing", "minpiv", "spd"):
            assert np.array_equal(np.asarray(e[name]).astype(T["s_" + name].dtype), T["s_" + name][i]), (i, name)
    for row in range(0, len(T["r_vec"]), 13):
        assert np.array_equal(mk.expected_rotation(T["r_vec"][row]), T["r_R"][row]), row


def _lapack_units(T):
    fw = bw = 0.0
    for i in np.nonzero((T["s_cls"] == 1) | (T["s_cls"] == 5))[0]:
        f, b, _ = solve_error_units(T, i, np.linalg.solve(T["s_A"][i], T["s_b"][i]))
        fw, bw = max(fw, f or 0.0), max(bw, b or 0.0)
    return fw, bw


def test_lapack_constants_are_the_measured_ones():
    """C_FWD and C_BWD are 8 x what an unrelated double-precision solver shows on the same table (numpy.linalg.solve: LAPACK's
    partial-pivot LU).  The literals above are the measurement rounded up to two decimals."""
    fw, bw = _lapack_units(table())
    print(f"LAPACK on classes 1 and 5: forward {fw:.3f} kappa_inf u, backward {bw:.3f} u")
    assert 0.5 * LAPACK_FWD <= fw <= LAPACK_FWD and 0.5 * LAPACK_BWD <= bw <= LAPACK_BWD, (fw, bw)


@pytest.mark.parametrize("form", ["oracle", "host ABI"])
def test_solve_values_against_exact_solutions(oracle_mod, form):
    """Classes 1 and 5."""
    solve = _forms(oracle_mod)[form][0]
    T = table()
    worst = [0.0, 0.0]
    for i in np.nonzero((T["s_cls"] == 1) | (T["s_cls"] == 5))[0]:
        f, b = check_solve_values(T, i, solve(T["s_A"][i], T["s_b"][i]), form)
        worst = [max(worst[0], f or 0.0), max(worst[1], b or 0.0)]
    print(f"{form}: forward {worst[0]:.3f} kappa_inf u (bar {C_FWD}), backward {worst[1]:.3f} u (bar {C_BWD})")


@pytest.mark.parametrize("form", ["oracle", "host ABI"])
def test_solve_decisions_against_exact_ldlt(oracle_mod, form):
    """Classes 2-4: singular, tied and indefinite systems follow the pivot order and the dropped set of Eigen's algorithm in exact arithmetic."""
    solve = _forms(oracle_mod)[form][0]
    T = table()
    for c in (2, 3, 4):
        idx = np.nonzero(T["s_cls"] == c)[0]
        checked = sum(check_solve_decisions(T, i, solve(T["s_A"][i], T["s_b"][i]), form) for i in idx)
        assert checked >= (0.9 if c == 4 else 0.98) * len(idx), (c, checked, len(idx))


@pytest.mark.parametrize("form", ["oracle", "host ABI"])
def test_rodrigues_against_mpmath_values(oracle_mod, form):
    """Class 6 and every increment of class 7."""
    rod = _forms(oracle_mod)[form][1]
    T = table()
    worst = {}
    for row in range(len(T["r_vec"])):
        e = check_rotation(T, row, rod(T["r_vec"][row]), form)
        _, theta = rotation_bar(T["r_vec"][row])
        b = int(T["r_band"][row])
        worst[b] = max(worst.get(b, 0.0), e / max(1.0, theta if theta >= 10 else 1.0))
    print(form, "worst error per band in units of u max(1, theta >= 10):", {k: round(v, 2) for k, v in sorted(worst.items())})


def test_pose_update_chains_against_exact_products():
    """Class 7: kt_host_pose_update composed 1 .. 19 times (the oracle's copy is static; the trackers' bit-equality tests tie it to this one)."""
    from kintinuous_amd import abi
    T = table()
    worst = np.zeros(3)
    for c in range(len(T["c_len"])):
        for row, k, state, new, Rc, tc, prev, exact in host_chain(T, c, abi.host_pose_update):
            worst = np.maximum(worst, check_step(T, row, state, new, Rc, tc, prev, "host ABI chain", k=k, T_exact=exact))
    print("worst: resultRt %.2f u (bar 16 k max(1, |t|)), Rcurr %.2f, tcurr %.2f x 2^-24 largest term (bar 8)" % tuple(worst))


def check_krk(Tm, intr, krkinv, kt, what):
    KRK, Kt, sK, st = G.krk(_mat(Tm, 4, 4), *[G.frac(float(v)) for v in intr])
    for i in range(3):
        for j in range(3):
            assert abs(F(float(krkinv[i][j])) - KRK[i][j]) <= F(8 * UF) * sK[i][j], (what, i, j, krkinv, intr)
        assert abs(F(float(kt[i])) - Kt[i]) <= F(8 * UF) * st[i], (what, i, kt, intr)


def test_krk_against_rationals():
    from kintinuous_amd import abi
    T = table()
    for Tm, intr in zip(T["k_T"], T["k_intr"]):
        krkinv, kt = abi.host_compute_krk(Tm, *intr)
        check_krk(Tm, intr, krkinv, kt, "host ABI")


@pytest.mark.parametrize("form", ["oracle", "host ABI"])
def test_mat33_inverse_against_rationals(oracle_mod, form):
    inv = _forms(oracle_mod)[form][2]
    worst = 0.0
    for m in table()["m_in"]:
        want, scale = G.inverse33_with_scale(_mat(m, 3, 3))
        got = inv(m.reshape(3, 3))
        for i in range(3):
            for j in range(3):
                e = abs(F(float(got[i][j])) - want[i][j]) / scale[i][j]
                worst = max(worst, float(e) / UF)
                assert e <= F(8 * UF), (form, m, i, j, float(e) / UF)
    print(form, "mat33_inverse worst %.2f x 2^-24 largest term (bar 8)" % worst)


def test_trajectory_and_ground_truth_poses_against_rationals():
    from kintinuous_amd import abi
    T = table()
    worst = [0.0, 0.0]
    for p in T["q_pose7"]:
        got = abi.host_trajectory_pose(p)
        q = _fr(p[3:])
        want = G.quat_matrix(*q)
        assert np.array_equal(got[9:], p[:3])
        for i in range(3):
            for j in range(3):
                scale = max(F(1) if i == j else F(0), 2 * max(abs(a * b) for a in q for b in q))   # the terms are 1 and 2 q_a q_b
                e = abs(F(float(got[i * 3 + j])) - want[i][j]) / scale
                worst[0] = max(worst[0], float(e) / UF)
                assert e <= F(8 * UF), ("trajectory_pose", p, i, j, float(e) / UF)
    for A, B, last in T["g_pose"]:
        R, t = abi.host_ground_truth_pose(A, B, last[:9], last[9:])
        m4 = lambda P: G.rigid(_mat(P[:9], 3, 3), _fr(P[9:]))
        want, scale = G.ground_truth_pose(m4(A), m4(B), m4(last))
        got = G.rigid(_mat(R, 3, 3), _fr(t))
        for i in range(3):
            for j in range(4):
                e = abs(got[i][j] - want[i][j]) / scale[i][j]
                worst[1] = max(worst[1], float(e) / UF)
                assert e <= F(8 * UF), ("ground_truth_pose", i, j, float(e) / UF)
    print("worst: trajectory_pose %.2f, ground_truth_pose %.2f x 2^-24 largest term (bar 8)" % tuple(worst))


def test_rational_rodrigues_series_equals_the_mpmath_values():
    """gn_reference.rodrigues_series (what the GPU end-to-end test uses where mpmath is absent) against the recorded mpmath matrices."""
    T = table()
    n = 0
    for row in range(len(T["r_vec"])):
        r = _fr(T["r_vec"][row])
        if sum(v * v for v in r) > 16:
            continue
        got = [v for rowv in G.rodrigues_series(r) for v in rowv]
        assert max(abs(a - b) for a, b in zip(got, _hl(T["r_R"][row]))) <= F(1, 2 ** 100), row
        n += 1
    assert n > 700
