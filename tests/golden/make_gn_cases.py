"""Generates tests/golden/gn_cases_v1.npz: the seeded case table of the Gauss-Newton tail (6x6 solve, rotation vector -> matrix, pose
update, K R K^-1, 3x3 inverse, trajectory poses) and what tests/tools/gn_reference.py says about it -- exact solutions and the decisions of
Eigen's pivoted LDL^T over the rationals, rotation matrices by mpmath at 100 digits, as (hi, lo) pairs of doubles.  The file holds numbers
only.  tests/test_gn_reference.py regenerates a sample where mpmath is importable and compares; tests/test_gpu_solve.py reads the file alone.
Run:  python tests/golden/make_gn_cases.py        (needs mpmath)

Every system of classes 1-5 that may go to the device is float32-representable (the kernels receive the 29 packed float sums); every
rotation vector / translation is a double of the form float + 10 * float, which the joint combination b_rgbd + 10 b_icp of the debug hook
forms exactly from two float32 numbers over an identity matrix.
"""
import itertools
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import gn_reference as G  # noqa: E402

SEED = 20261016
PATH = os.path.join(HERE, "gn_cases_v1.npz")
CLASSES = {1: "float32 J^T J, kappa 1e0 .. 1e14", 2: "exactly singular", 3: "ties on the diagonal", 4: "symmetric indefinite",
           5: "badly scaled A, denormal / zero b", 6: "rotation vectors", 7: "pose updates"}
SWAP = [3, 4, 5, 0, 1, 2]   # the partner of a device-eligible system: its unknowns with the halves exchanged (see test_gpu_solve.py)
# theta bands of class 6
BANDS = {0: "[0, 4 eps)", 1: "1e-8 .. 1e-3", 2: "around pi / 2", 3: "within 1e-9 of pi", 4: "around 2 pi", 5: "1e3 .. 1e6", 6: "generic"}
INTRINSICS = [(w / 640.0 * 525.0 / 2 ** l, w / 640.0 * 525.0 / 2 ** l, (w / 2 - 0.5) / 2 ** l, (w * 0.375 - 0.5) / 2 ** l) for w in (640, 1280) for l in range(4)]


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def two_float(v):
    """The double float32(v) + 10 * float32((v - float32(v)) / 10) next to v, and its two float32 parts."""
    v = np.asarray(v, np.float64)
    b1 = v.astype(np.float32)
    b2 = ((v - b1.astype(np.float64)) / 10.0).astype(np.float32)
    return b1.astype(np.float64) + 10.0 * b2.astype(np.float64), b1, b2


def jtj32(J, r):
    """float32(J^T J), float32(J^T r) of float32 J, r -- every sum exactly rounded (math.fsum), so the table does not depend on a BLAS."""
    J, r = J.astype(np.float64), r.astype(np.float64)
    A = np.zeros((6, 6))
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = math.fsum((J[:, i] * J[:, j]).tolist())
    b = np.array([math.fsum((J[:, i] * r).tolist()) for i in range(6)])
    return f32(A), f32(b)


def _layer2(A, b):
    return G.ldlt_eigen(G.fmat(A, 6, 6), [G.frac(v) for v in b])


def _spd(A, b):
    l2 = _layer2(A, b)
    return all(d > 0 for d in l2["D"]) and not any(l2["dropped"]) and not l2["undecidable"]


def _generic(rng, m_lo=30, m_hi=400, colscale=None, neardep=False):
    m = int(rng.integers(m_lo, m_hi))
    J = rng.normal(size=(m, 6))
    if neardep:   # two nearly dependent columns: a planar wall / a corridor barely constrains one translation and one rotation
        a, c = rng.choice(6, size=2, replace=False)
        J[:, a] = J[:, c] * rng.uniform(0.5, 2.0) + 10.0 ** rng.uniform(-3, -1) * rng.normal(size=m)
    if colscale is not None:
        J = J * colscale
    J = J.astype(np.float32)
    r = (rng.normal(size=m) * 10.0 ** rng.uniform(-4, 0)).astype(np.float32)
    return jtj32(J, r)


def solve_cases(rng):
    """Classes 1-5: a list of dicts cls, kind, A, b, f32 (may go to the device), zero (unknowns whose row and column are zero)."""
    out = []

    def add(cls, kind, A, b, f32ok=True, zero=None):
        out.append({"cls": cls, "kind": kind, "A": np.array(A, np.float64), "b": np.array(b, np.float64), "f32": f32ok,
                    "zero": np.zeros(6, bool) if zero is None else np.array(zero, bool)})

    # ---- class 1: kind = 0 plain, 1 columns scaled, 2 nearly dependent columns, 3 both
    k = 0
    while k < 150:
        span = [0.0, 1.0, 2.0, 3.0, 3.5][k % 5]
        near = k % 3 == 2
        A, b = _generic(rng, colscale=10.0 ** rng.uniform(-span, span, 6) if span else None, neardep=near)
        if not _spd(A, b):
            continue
        add(1, (1 if span else 0) + (2 if near else 0), A, b)
        k += 1
    # ---- class 2: exactly singular systems whose elimination is exact in double as well: zero rows / columns and duplicated (or negated)
    # unknowns around a well-conditioned block of rank r.  kind = r (0: all zero)
    for k in range(150):
        r = k % 6
        B, bb = _generic(rng, m_lo=60)
        S = list(rng.choice(6, size=r, replace=False))
        src, sgn = {}, {}
        for v in range(6):
            if v in S:
                src[v], sgn[v] = v, 1.0
            elif r > 0 and rng.random() < 0.6:
                src[v], sgn[v] = int(rng.choice(S)), (-1.0 if rng.random() < 0.3 else 1.0)
            else:
                src[v], sgn[v] = None, 0.0
        A, b = np.zeros((6, 6)), np.zeros(6)
        for u in range(6):
            for v in range(6):
                if src[u] is not None and src[v] is not None:
                    A[u, v] = sgn[u] * sgn[v] * B[src[u], src[v]]
            if src[u] is not None:
                b[u] = sgn[u] * bb[src[u]]
        if k % 3 == 1:      # an inconsistent right-hand side on the dependent unknowns (the dropped pivots must swallow it)
            for u in range(6):
                if u not in S:
                    b[u] = f32(b[u] + rng.normal())
        add(2, r, A, b, zero=[src[v] is None for v in range(6)])
    # kind 6: a decoupled unknown whose pivot is nonzero but below max|D| eps (solve() drops it: x = 0, not b / d), or small and above it (kept);
    # in every second case it is unknown 0, so that a threshold taken from A[0][0] shows
    for k in range(30):
        B, bb = _generic(rng, m_lo=60)
        v = 0 if k % 2 == 0 else int(rng.integers(1, 6))
        A, b = B.copy(), bb.copy()
        A[v, :] = 0
        A[:, v] = 0
        A[v, v] = f32(np.abs(B).max() * 10.0 ** (-rng.uniform(17, 30) if k % 3 else -rng.uniform(8, 14)))
        b[v] = f32(A[v, v] * rng.normal())
        add(2, 6, A, b)
    # ---- class 3: ties.  kind 0: every arrangement of the diagonal (3, 3, 5, 1, 3, 5) (test_gpu_solve kind 1); 1: all equal (its kind 2);
    # 2: equal magnitudes with mixed signs; 3: a duplicated (or negated) unknown at every pair of positions -- the tie decides which is dropped
    def offdiag(scale):
        M = rng.uniform(-scale, scale, (6, 6))
        return f32(np.triu(M, 1) + np.triu(M, 1).T)
    arrangements = sorted(set(itertools.permutations([3.0, 3.0, 5.0, 1.0, 3.0, 5.0])))
    assert len(arrangements) == 60
    for d in arrangements:
        A = offdiag(0.15)
        A[np.arange(6), np.arange(6)] = d
        add(3, 0, A, f32(rng.normal(size=6)))
    for _ in range(12):
        A = offdiag(1.0)
        A[np.arange(6), np.arange(6)] = 7.0
        add(3, 1, A, f32(rng.normal(size=6)))
    for bits in range(1, 63, 2):
        s = np.array([-1.0 if (bits >> i) & 1 else 1.0 for i in range(6)])
        A = offdiag(0.15)
        A[np.arange(6), np.arange(6)] = s * (7.0 if bits % 4 == 1 else np.array(arrangements[bits % 60])[0:6])
        add(3, 2, A, f32(rng.normal(size=6)))
    for (i, j) in itertools.combinations(range(6), 2):
        for rep in range(2):
            B, bb = _generic(rng, m_lo=60)
            s = -1.0 if rep else 1.0
            A, b = B.copy(), bb.copy()
            A[j, :] = s * B[i, :]
            A[:, j] = s * B[:, i]
            A[j, j] = B[i, i]
            A[i, j] = A[j, i] = s * B[i, i]
            b[j] = s * bb[i]
            add(3, 3, A, b)
    # ---- class 4: symmetric indefinite.  kind 0: test_gpu_solve kind 6; 1: random symmetric
    k = 0
    while k < 150:
        if k % 2 == 0:
            A, b = _generic(rng, colscale=10.0 ** rng.uniform(-2, 2))
            A = f32(A - 0.5 * np.diag(np.diag(A)))
            A[2, 2] = -A[2, 2]
        else:
            M = rng.normal(size=(6, 6)) * 10.0 ** rng.uniform(-2, 2)
            A, b = f32(np.triu(M) + np.triu(M, 1).T), f32(rng.normal(size=6))
        if _layer2(A, b)["undecidable"]:
            continue
        add(4, k % 2, A, b)
        k += 1
    # kind 2: max|D| far above the FIRST pivot.  All diagonals are of order 1 and one off-diagonal pair is 100, so D starts near 1 and holds
    # an entry near -1e4; a decoupled unknown has a diagonal between eps |D[0]| and eps max|D| (dropped: x = 0 -- a threshold taken from
    # the first pivot, as in Eigen 3.2.0's early stop, keeps it), above both (kept) or below both (dropped).  A generator of its own, so
    # that the kinds added later leave the rest of the table as it was.
    rng2 = np.random.default_rng(SEED + 1)
    for k in range(30):
        p, q, v = (int(i) for i in rng2.choice(6, size=3, replace=False))
        A = f32(np.triu(rng2.uniform(-0.05, 0.05, (6, 6)), 1))
        A = A + A.T
        A[np.arange(6), np.arange(6)] = f32(rng2.uniform(0.3, 1.0, 6) * rng2.choice([-1.0, 1.0], 6))
        A[p, q] = A[q, p] = f32(100.0 * rng2.uniform(0.8, 1.2))
        A[v, :] = 0
        A[:, v] = 0
        A[v, v] = f32(10.0 ** [-rng2.uniform(13.0, 14.5), -rng2.uniform(13.0, 14.5), -rng2.uniform(6, 9), -rng2.uniform(18, 25)][k % 4])
        b = f32(rng2.normal(size=6))
        b[v] = f32(A[v, v] * rng2.normal())
        assert not _layer2(A, b)["undecidable"]
        add(4, 2, A, b)
    # ---- class 5: kind 0: float32(A 10^k), |k| <= 30; 1: A 10^k in double, |k| <= 200 (host only); 2: float32-denormal b; 3: double-denormal b
    # (host only); 4: b == 0 or with zero entries
    k = 0
    while k < 150:
        kind = k % 5
        A, b = _generic(rng, m_lo=60)
        f32ok = kind not in (1, 3)
        if kind == 0:
            e = int(rng.integers(-30, 31))
            A, b = f32(A * 10.0 ** e), f32(b * 10.0 ** int(rng.integers(-20, 21)))
        elif kind == 1:
            A, b = A * 10.0 ** int(rng.integers(-200, 201)), b * 10.0 ** int(rng.integers(-100, 101))
        elif kind == 2:
            b = f32(b * 1e-41 / np.abs(b).max())
        elif kind == 3:
            b = b * 1e-310 / np.abs(b).max()
        else:
            b = np.zeros(6) if k % 2 else b * (rng.random(6) < 0.5)
        if not (np.all(np.isfinite(A)) and _spd(A, b if np.any(b) else np.ones(6))):
            continue
        add(5, kind, A, b, f32ok)
        k += 1
    # partners: the same system with the halves of the unknowns exchanged, a case of its own
    n = len(out)
    for c in out:
        c["pair"] = -1
    for idx in range(n):
        c = out[idx]
        if c["f32"]:
            c["pair"] = len(out)
            out.append({"cls": c["cls"], "kind": c["kind"], "A": c["A"][SWAP][:, SWAP].copy(), "b": c["b"][SWAP].copy(), "f32": True,
                        "zero": c["zero"][SWAP].copy(), "pair": idx})
    return out


def _axis(rng, k):
    if k % 3 == 0:
        a = np.zeros(3)
        a[(k // 3) % 3] = -1.0 if (k // 9) % 2 else 1.0
        return a
    a = rng.normal(size=3)
    return a / np.linalg.norm(a)


def _theta(rng, band, k):
    eps = 2.0 ** -52
    if band == 0:
        return [0.0, eps, np.nextafter(eps, 0), np.nextafter(eps, 1), eps * rng.uniform(0, 1), eps * rng.uniform(1, 4), eps * rng.uniform(0, 4)][k % 7]
    if band == 1:
        return 10.0 ** rng.uniform(-8, -3)
    if band == 2:
        return math.pi / 2 + (rng.uniform(-0.1, 0.1) if k % 2 else rng.uniform(-1e-9, 1e-9))
    if band == 3:
        return math.pi + rng.uniform(-1e-9, 1e-9)
    if band == 4:
        return 2 * math.pi + (rng.uniform(-0.01, 0.01) if k % 2 else rng.uniform(-1e-9, 1e-9))
    if band == 5:
        return 10.0 ** rng.uniform(3, 6)
    return rng.uniform(0.01, 3.0)


def _rotation(rng, angle):
    """A rotation matrix in double from numpy's own sin / cos: an INPUT (a previous pose, an increment for K R K^-1), not a reference value."""
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def inputs(seed=SEED):
    rng = np.random.default_rng(seed)
    g = {}
    sc = solve_cases(rng)
    g["s_cls"] = np.array([c["cls"] for c in sc], np.int8)
    g["s_kind"] = np.array([c["kind"] for c in sc], np.int8)
    g["s_A"] = np.array([c["A"] for c in sc], np.float64)
    g["s_b"] = np.array([c["b"] for c in sc], np.float64)
    g["s_f32"] = np.array([c["f32"] for c in sc], bool)
    g["s_zero"] = np.array([c["zero"] for c in sc], bool)
    g["s_pair"] = np.array([c["pair"] for c in sc], np.int32)
    # class 6: rows [0, n6) of the rotation table; class 7: chains of 1 .. 19 increments, rows [n6, ...)
    rv, rt, band = [], [], []
    for b_ in range(7):
        for k in range(45):
            rv.append(two_float(_axis(rng, k) * _theta(rng, b_, k))[0])
            rt.append(two_float(rng.normal(size=3) * 10.0 ** rng.uniform(-6, 1))[0])
            band.append(b_)
    g["c_start"], g["c_len"] = [], []
    for rep in range(3):
        for n in range(1, 20):
            g["c_start"].append(len(rv))
            g["c_len"].append(n)
            for k in range(n):
                b_ = [1, 6, 1, 0, 1, 2, 1, 3, 6, 4][(k + rep + n) % 10]
                th = _theta(rng, b_, k) * (0.1 if b_ == 6 else 1.0)
                rv.append(two_float(_axis(rng, k + rep) * th)[0])
                tv = rng.normal(size=3)
                rt.append(two_float(tv / np.linalg.norm(tv) * 10.0 ** rng.uniform(-6, 1))[0])
                band.append(b_)
    g["r_vec"], g["r_t"], g["r_band"] = np.array(rv), np.array(rt), np.array(band, np.int8)
    g["n6"] = np.int32(7 * 45)
    g["c_start"], g["c_len"] = np.array(g["c_start"], np.int32), np.array(g["c_len"], np.int32)
    nc = len(g["c_len"])
    prev = np.zeros((nc, 12), np.float32)
    for c in range(nc):
        prev[c, :9] = _rotation(rng, rng.uniform(0, math.pi)).astype(np.float32).reshape(9)
        tv = rng.normal(size=3)
        prev[c, 9:] = (tv / np.linalg.norm(tv) * rng.uniform(0, 10)).astype(np.float32)
    g["c_prev"] = prev
    # K R K^-1 / K t: rigid increments in double, the four pyramid levels' intrinsics at 640x480 and 1280x960
    kT, kI = [], []
    for k in range(200):
        T = np.eye(4)
        T[:3, :3] = _rotation(rng, 10.0 ** rng.uniform(-6, 0) if k % 4 else rng.uniform(0, math.pi))
        T[:3, 3] = rng.normal(size=3) * 10.0 ** rng.uniform(-6, 0.5)
        kT.append(T.reshape(16))
        kI.append(INTRINSICS[k % 8])
    g["k_T"], g["k_intr"] = np.array(kT), np.array(kI, np.float64)
    # 3x3 float inverse: rotations that have drifted off SO(3) by 1e-4
    g["m_in"] = np.array([(_rotation(rng, rng.uniform(0, math.pi)) + rng.normal(size=(3, 3)) * 1e-4).reshape(9) for _ in range(200)], np.float32)
    # trajectory lines {t, q}: non-unit and negative-w quaternions; ground-truth triples (previous stamp, current stamp, last pose)
    q = rng.normal(size=(200, 4))
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (200, 1))
    q[::2, 3] = -np.abs(q[::2, 3])
    q[::5] /= np.linalg.norm(q[::5], axis=1, keepdims=True)
    g["q_pose7"] = np.concatenate([rng.uniform(-10, 10, (200, 3)), q], axis=1).astype(np.float32)
    gt = np.zeros((200, 3, 12), np.float32)
    for k in range(200):
        for s in range(3):
            qq = rng.normal(size=4)
            qq = qq / np.linalg.norm(qq) * (1.0 if s == 2 or k % 2 else rng.uniform(0.9, 1.1))
            x, y, z, w = qq
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
            gt[k, s, :9], gt[k, s, 9:] = R.reshape(9), rng.uniform(-10, 10, 3)
    g["g_pose"] = gt
    return g


def expected_solve(A, b):
    """Layers 1 and 2 for one system: x (hi, lo) -- the exact solution wherever nothing is dropped --, kappa_inf, the pivot order, the
    dropped unknowns, the undecidable flag, whether A is nonsingular, min |D| / max |D|, whether D > 0 throughout."""
    Af, bf = G.fmat(A, 6, 6), [G.frac(v) for v in b]
    l2 = G.ldlt_eigen(Af, bf)
    x, kappa = G.solve_with_condition(Af, bf)
    if x is not None and not any(l2["dropped"]):
        assert x == l2["x"]        # the two layers agree where the answer is a number
    return {"x": np.array([G.hilo(v) for v in l2["x"]]), "kappa": float(kappa) if kappa is not None else np.inf,
            "order": np.array(l2["order"], np.int8), "drop": np.array(l2["dropped_vars"], bool), "undec": l2["undecidable"],
            "nonsing": x is not None, "minpiv": float(l2["min_pivot_ratio"]), "spd": all(d > 0 for d in l2["D"])}


def expected_rotation(r):
    return np.array([G.hilo(v) for row in G.rodrigues_mp(r) for v in row])


def expected(g):
    e = {}
    rows = [expected_solve(A, b) for A, b in zip(g["s_A"], g["s_b"])]
    for name, ty in (("x", np.float64), ("kappa", np.float64), ("order", np.int8), ("drop", bool), ("undec", bool), ("nonsing", bool),
                     ("minpiv", np.float64), ("spd", bool)):
        e["s_" + name] = np.array([r[name] for r in rows], ty)
    e["r_R"] = np.array([expected_rotation(r) for r in g["r_vec"]])
    return e


def main():
    g = inputs()
    e = expected(g)
    for c in range(1, 6):
        m = g["s_cls"] == c
        share = float(e["s_undec"][m].mean())
        print(f"class {c} ({CLASSES[c]}): {int(m.sum())} systems, {int((m & g['s_f32']).sum())} device-eligible, undecidable {share:.3%}")
        assert share <= 0.02
    m = (g["s_cls"] == 1) | (g["s_cls"] == 5)
    assert e["s_spd"][m].all() and not e["s_drop"][m].any()
    np.savez_compressed(PATH, **g, **e)
    print(PATH, os.path.getsize(PATH), "bytes;", len(g["s_cls"]), "systems,", len(g["r_vec"]), "rotations")


if __name__ == "__main__":
    main()
