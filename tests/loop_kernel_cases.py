"""The synthetic lists of tests/test_gpu_loop_kernels.py (GPU) and tests/test_loop_kernel_reference.py (CPU): match lists for the RANSAC
kernels and cloud pairs for one reducing registration pass, with what tests/tools/loop_reference.py says about them.  Inputs and
reference values use nothing from the package (restated_scores alone calls its numpy restatement): the CPU file shows with them that the GPU
file's expectations can be met before a GPU is involved."""
import functools
import importlib.util
import math
import os
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REF = _load("loop_reference", os.path.join(ROOT, "tests", "tools", "loop_reference.py"))

F = np.float32
INTR = (525.5, 531.25, 319.5, 239.5)          # fx, fy, cx, cy: float32 values
REPROJ = 2.0
GRID_M = (0, 2, 3, 4, 64, 1023, 1024, 1025, 2049, 4096)
GRID_H = (1, 63, 64, 65, 500)
CAP = 0.01                                    # the share of hypotheses the reference may leave undecided, per case


def _rodrigues(w):
    th = float(np.linalg.norm(w))
    k = np.asarray(w, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def _project(P, intr=INTR):
    fx, fy, cx, cy = intr
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], axis=1)
    return np.clip(np.nan_to_num(uv, nan=0.0, posinf=1e6, neginf=-1e6), -1e6, 1e6)


def _frustum_points(rng, n):
    fx, fy, cx, cy = INTR
    z = rng.uniform(0.5, 4.0, n)
    return np.stack([(rng.uniform(0, 640, n) - cx) * z / fx, (rng.uniform(0, 480, n) - cy) * z / fy, z], axis=1)


def match_list(m, seed, first_inlier=0, noise=True, outliers=True, n_behind=5):
    """m matches under a seeded rigid motion of points 0.5 - 4 m in front of the new camera: 60 % inliers (2 mm on the old point, 0.3 px and the
    pixel grid on the old pixel), the others replaced by random points, a handful behind the old camera (Z <= 0 after the true motion; their
    pixel is the mirrored projection, so that only the Z test rejects them).  Matches below first_inlier are all outliers.
    Returns (m_uv int32 [m, 4] = old u, old v, new u, new v; m_pn, m_po float32 [m, 3])."""
    rng = np.random.default_rng(seed)
    pn = _frustum_points(rng, m)
    behind = rng.choice(m, min(n_behind, m // 12), replace=False) if m else np.zeros(0, np.int64)
    pn[behind, 2] = -rng.uniform(0.3, 1.0, len(behind))
    pn = pn.astype(F)
    R, t = _rodrigues(np.array([0.05, -0.09, 0.04])), np.array([0.21, -0.13, 0.08])
    true = pn.astype(np.float64) @ R.T + t
    po = true + (rng.normal(0, 0.002, (m, 3)) if noise else 0.0)
    uv_old = _project(true) + (rng.normal(0, 0.3, (m, 2)) if noise else 0.0)
    if outliers:
        out = np.zeros(m, bool)
        out[rng.permutation(m)[: m - int(round(0.6 * m))]] = True
        out[:first_inlier] = True
        out[behind] = False
        rnd = _frustum_points(rng, m)
        po[out], uv_old[out] = rnd[out], _project(rnd)[out]
    uv = np.concatenate([np.rint(uv_old), np.rint(_project(pn.astype(np.float64)))], axis=1).astype(np.int32)
    return uv, pn, po.astype(F)


# ---------------------------------------------------------------------------------------------------------------------------------
# the RANSAC cases: name -> dict(uv, pn, po, seed, n_hyp, intr, reproj)
# ---------------------------------------------------------------------------------------------------------------------------------
def _ties_case():
    """64 noise-free matches: every non-degenerate hypothesis scores 64.  The triples of hypotheses 0 and 1 hold a repeated point (n1 = 0 and
    n3 = 0), so the winner is hypothesis 2."""
    m, n_hyp = 64, 130
    for seed in range(1, 1000):
        tri = REF.draws(seed, n_hyp, m)
        if len(set(tri[:3].ravel().tolist())) == 9:
            break
    uv, pn, po = match_list(m, 4242, noise=False, outliers=False, n_behind=0)
    for a in (uv, pn, po):
        a[tri[0, 1]] = a[tri[0, 0]]                          # hypothesis 0: p1 = p0
        a[tri[1, 2]] = a[tri[1, 0]]                          # hypothesis 1: p2 = p0
    return dict(uv=uv, pn=pn, po=po, seed=seed, n_hyp=n_hyp)


def _collinear_case():
    """every point of both frames on a line parallel to the x axis: c = e1 x b is exactly zero for every triple"""
    m = 1025
    rng = np.random.default_rng(9)
    x = rng.uniform(-2, 2, m).astype(F)
    pn = np.stack([x, np.full(m, 0.25, F), np.full(m, 2.0, F)], axis=1)
    po = np.stack([(x + F(0.5)).astype(F), np.full(m, -0.125, F), np.full(m, 2.5, F)], axis=1)
    uv = np.concatenate([np.rint(_project(po.astype(np.float64))), np.rint(_project(pn.astype(np.float64)))], axis=1).astype(np.int32)
    return dict(uv=uv, pn=pn, po=po, seed=3, n_hyp=65)


@functools.lru_cache(maxsize=None)
def ransac_case(name):
    if name == "ties":
        c = _ties_case()
    elif name == "collinear":
        c = _collinear_case()
    elif name == "lattice":
        c = lattice_case()
    elif name == "second_tile":                               # every inlier at index >= 1024
        uv, pn, po = match_list(2049, 2049_1, first_inlier=1024)
        c = dict(uv=uv, pn=pn, po=po, seed=11, n_hyp=130)
    elif name == "m64_h65536":
        uv, pn, po = match_list(64, 64_2)
        c = dict(uv=uv, pn=pn, po=po, seed=5, n_hyp=65536)
    else:
        m = int(name[1:])
        assert name == f"m{m}" and m in GRID_M
        uv, pn, po = match_list(m, 1000 + m, outliers=m > 4)   # (3 or 4 matches with an outlier among them score 0 under every triple: all inliers there)
        c = dict(uv=uv, pn=pn, po=po, seed=7 + m, n_hyp=max(GRID_H))
    c.setdefault("intr", INTR)
    c.setdefault("reproj", REPROJ)
    for a in (c["uv"], c["pn"], c["po"]):
        a.setflags(write=False)
    return c


RANSAC_CASES = tuple(f"m{m}" for m in GRID_M) + ("m64_h65536", "second_tile", "ties", "collinear", "lattice")


@functools.lru_cache(maxsize=None)
def ransac_bounds(name):
    """(lo, hi, fit) of the case's n_hyp hypotheses from the independent reference (hypothesis h does not depend on n_hyp: a prefix serves a
    smaller count).  The lattice case is exact: lo = hi = its integer expectation."""
    c = ransac_case(name)
    m, n = len(c["pn"]), c["n_hyp"]
    if name == "lattice":
        e = lattice_expected()
        return e, e, None
    if m < 3:
        z = np.zeros(n, np.int64)
        return z, z, None
    fit = REF.fit_many(c["pn"], c["po"], REF.draws(c["seed"], n, m))
    lo, hi = REF.inlier_bounds(fit, c["pn"], c["uv"][:, :2], *c["intr"], c["reproj"])
    return lo, hi, fit


@functools.lru_cache(maxsize=None)
def restated_scores(name):
    """The score of every hypothesis of a case from the numpy restatement (kintinuous_amd/loop_match_ref.py: draw_triples, fit_triples,
    reprojection_inliers) -- the one function of this module that calls the package."""
    from kintinuous_amd import loop_match_ref as lm
    c = ransac_case(name)
    m, n = len(c["pn"]), c["n_hyp"]
    out = np.zeros(n, np.int64)
    if m < 3:
        return out
    step = max(1, (1 << 21) // m)
    tri = lm.draw_triples(c["seed"], n, m)
    for h0 in range(0, n, step):
        R, t, deg = lm.fit_triples(c["pn"], c["po"], tri[h0:h0 + step])
        inl = lm.reprojection_inliers(R, t, c["pn"], c["uv"][:, :2], *c["intr"], c["reproj"])
        out[h0:h0 + step] = np.where(deg, 0, inl.sum(axis=1))
    return out


def expected_best(score):
    """{the lowest index of the maximum, the maximum}"""
    return [int(np.argmax(score)), int(np.max(score))]


# ---------------------------------------------------------------------------------------------------------------------------------
# the exact lattice
# ---------------------------------------------------------------------------------------------------------------------------------
LATTICE_INTR = (512.0, 520.0, 320.0, 240.0)
LATTICE_REPROJ = 5.0                                          # thr^2 = 25 = 3^2 + 4^2
# two motions new -> old, a quarter turn about z either way and a dyadic translation, in eighths of a metre: old = P p + t
LATTICE_MOTIONS = {"A": (((0, -1, 0), (1, 0, 0), (0, 0, 1)), (2, -4, 4)), "B": (((0, 1, 0), (-1, 0, 0), (0, 0, 1)), (-4, 2, 4))}


def _lattice_motion_of(h):
    return "B" if h % 3 == 1 else "A"


def _move8(name, p8):
    P, t = LATTICE_MOTIONS[name]
    return [sum(P[a][b] * p8[b] for b in range(3)) + t[a] for a in range(3)]


@functools.lru_cache(maxsize=None)
def lattice_case():
    """1500 matches on multiples of 1/8 m, 24 hypotheses whose 72 indices are distinct (the seed is searched for that).  The triple of
    hypothesis h is p0, p0 + d along one axis, p0 + (e, f) in the plane of that axis and the other of x / y, with d + e and f multiples of
    3/8: n1 = d and n3 = |f| are exact roots, e1 / e2 / e3 are signed unit axes, the centroid is a lattice point, R is the signed permutation
    and t the dyadic translation of the motion the old points were made with (A, or B for h = 1 mod 3).  z + 1/2 is 1, 2 or 4 m, so the
    projection divides by a power of two; fx, fy, cx, cy are integers.  Every operation of match_fit3 and match_inlier is then exact in
    double and the scores are integer arithmetic (lattice_expected).  Old pixels sit at integer offsets from the projection under A, so many
    pairs land exactly on du^2 + dv^2 = 25 -- (3, 4), (-4, 3), (5, 0), (0, -5) are planted on both sides of index 1024 -- ; one pair is the
    float32 neighbour of a (5, 0) pair just outside, one just inside; one pair has Z = 0, one Z < 0."""
    m, n_hyp = 1500, 24
    for seed in range(1, 100000):
        tri = REF.draws(seed, n_hyp, m)
        if len(set(tri.ravel().tolist())) == 3 * n_hyp:
            break
    rng = np.random.default_rng(77)
    fx, fy, cx, cy = (int(v) for v in LATTICE_INTR)
    pn8 = np.stack([rng.integers(-16, 17, m), rng.integers(-16, 17, m), rng.choice([4, 12, 28], m)], axis=1)
    off = rng.integers(-6, 7, (m, 2))
    off[rng.random(m) < 0.5] = 0
    for h in range(n_hyp):                                    # the triples
        base = np.array([rng.integers(-12, 9), rng.integers(-12, 9), rng.choice([4, 12, 28])])
        d, e, f = int(rng.choice([4, 8, 16])), 0, 3 * int(rng.choice([-4, -2, 1, 3]))
        e = int(rng.choice([k for k in range(-8, 9) if (d + k) % 3 == 0]))
        along = (np.array([d, 0, 0]), np.array([e, f, 0])) if h % 2 == 0 else (np.array([0, d, 0]), np.array([f, e, 0]))
        pn8[tri[h, 0]], pn8[tri[h, 1]], pn8[tri[h, 2]] = base, base + along[0], base + along[1]
        off[tri[h]] = 0
    free = [j for j in range(m) if j not in set(tri.ravel().tolist())]
    low, high = [j for j in free if j < 1024], [j for j in free if j >= 1024]
    planted = low[:6] + high[:6]
    for j, o in zip(planted, [(3, 4), (-4, 3), (5, 0), (0, -5), (5, 0), (5, 0)] * 2):
        pn8[j] = (rng.integers(-16, 17), 8 + int(rng.integers(0, 8)), 4)    # Z = 1 m: integer pixels; 1 <= y < 2: a float32 step of 2^-23
        off[j] = o
    motion = np.array(["A"] * m)
    motion[[tri[h, k] for h in range(n_hyp) for k in range(3) if _lattice_motion_of(h) == "B"]] = "B"
    pn8[low[6]], pn8[high[6]] = (3, -5, -4), (-7, 2, -12)     # Z = 0 and Z = -1 m under both motions
    po8 = np.array([_move8(motion[j], pn8[j].tolist()) for j in range(m)])
    rnd = rng.random(m) < 0.3                                   # random old points on the lattice, away from the triples and the planted pairs
    rnd[tri.ravel()] = False
    rnd[planted + [low[6], high[6]]] = False
    po8[rnd] = np.stack([rng.integers(-16, 17, m), rng.integers(-16, 17, m), rng.choice([8, 16, 32], m)], axis=1)[rnd]
    # the old pixel: the projection of the old point under its own motion, rounded down, minus the offset (du = offset + a dyadic fraction)
    uv_old = np.zeros((m, 2), np.int64)
    for j in range(m):
        X, Y, Z = (int(v) for v in po8[j])
        Z = Z if Z > 0 else 8
        uv_old[j] = (math.floor(Fraction(fx * X, Z) + cx) - off[j, 0], math.floor(Fraction(fy * Y, Z) + cy) - off[j, 1])
    pn = (pn8 / 8.0).astype(F)
    po = (po8 / 8.0).astype(F)
    for j, toward in ((planted[4], -np.inf), (planted[5], np.inf), (planted[10], -np.inf), (planted[11], np.inf)):
        pn[j, 1] = np.nextafter(pn[j, 1], F(toward))          # X = -y + 1/4 under A: y one step down puts du one step beyond 5, one step up inside
    uv = np.concatenate([uv_old, uv_old[:, ::-1] + 40], axis=1).astype(np.int32)
    return dict(uv=uv, pn=pn, po=po, seed=seed, n_hyp=n_hyp, intr=LATTICE_INTR, reproj=LATTICE_REPROJ, tri=tri, planted=tuple(planted),
                behind=(low[6], high[6]))


@functools.lru_cache(maxsize=None)
def lattice_scores_by_motion():
    """The score of motion A and of motion B over the lattice list, in integers: coordinates in units of 2^-26 m (a float32 with 1 <= |y| < 2
    is a multiple of 2^-23), du = (fx X + (cx - u_old) Z) / Z, so a pair is in when Z > 0 and
    (fx X + (cx - u_old) Z)^2 + (fy Y + (cy - v_old) Z)^2 <= thr^2 Z^2."""
    c = lattice_case()
    fx, fy, cx, cy = (int(v) for v in LATTICE_INTR)
    thr2 = int(LATTICE_REPROJ) ** 2
    unit = 1 << 26
    out = {}
    for name, (P, t8) in LATTICE_MOTIONS.items():
        count = 0
        for p, (uo, vo) in zip(c["pn"], c["uv"][:, :2]):
            q = [int(float(v) * unit) for v in p]
            assert all(q[k] == float(p[k]) * unit for k in range(3))
            X, Y, Z = (sum(P[a][b] * q[b] for b in range(3)) + t8[a] * (unit // 8) for a in range(3))
            if Z > 0:
                au, av = fx * X + (cx - int(uo)) * Z, fy * Y + (cy - int(vo)) * Z
                count += au * au + av * av <= thr2 * Z * Z
        out[name] = count
    return out


def lattice_expected():
    s = lattice_scores_by_motion()
    return np.array([s[_lattice_motion_of(h)] for h in range(lattice_case()["n_hyp"])], np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the registration pass: name -> (src, dst, M)
# ---------------------------------------------------------------------------------------------------------------------------------
ICP_CASES = {"1x1": (1, 1), "63x1023": (63, 1023), "64x1024": (64, 1024), "65x1025": (65, 1025), "777x3001": (777, 3001), "4097x1025": (4097, 1025),
             "1x3001": (1, 3001), "65x3001_far_last": (65, 3001)}


@functools.lru_cache(maxsize=None)
def icp_case(name):
    """Clouds 2 - 4 m from the origin (the centring of the host's rigid fit never sees the sums: they are large against their spread), a seeded
    small motion M, targets duplicated across the 1024-point tile boundary with sources that land on them, and in `far_last` the one live
    lane of the second wave far from everything else."""
    ns, nt = ICP_CASES[name]
    rng = np.random.default_rng(ns * 10007 + nt)
    dst = rng.uniform([-1.0, -1.0, 2.0], [1.0, 1.0, 4.0], (nt, 3)).astype(F)
    if nt > 1024:
        dst[1024] = dst[1023]
    if nt > 2900:
        dst[1500] = dst[1023]
        dst[100] = dst[2900]
    M = np.concatenate([_rodrigues(np.array([0.02, -0.03, 0.04])), np.array([[0.03], [-0.02], [0.025]])], axis=1)
    pick = rng.integers(0, nt, ns)
    if nt > 1024:
        pick[0] = 1024
    if nt > 2900 and ns > 1:
        pick[1] = 2900
    near = dst[pick].astype(np.float64) + rng.normal(0, 0.02, (ns, 3))
    near[:2] = dst[pick[:2]].astype(np.float64) + rng.normal(0, 1e-4, (min(ns, 2), 3))
    src = ((near - M[:, 3]) @ M[:, :3]).astype(F)             # M^-1: the sources land near their targets
    if name.endswith("far_last"):
        src[64] = (30.0, -20.0, 50.0)
    src.setflags(write=False)
    dst.setflags(write=False)
    return src, dst, M


@functools.lru_cache(maxsize=None)
def icp_reference(name):
    src, dst, M = icp_case(name)
    return REF.icp_pass(src, dst, M)


def sum_errors(got16, ref):
    """per sum: (|got - exact|, u * sum |term|) as Fractions"""
    u = Fraction(1, 2 ** 53)
    return [(abs(Fraction(float(got16[k])) - ref["exact"][k]), u * ref["abs_sum"][k]) for k in range(16)]
