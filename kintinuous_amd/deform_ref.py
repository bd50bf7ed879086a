"""numpy restatement of the deformation-graph stage (csrc/kt_deform.hip; include/kt_abi.h and DESIGN.md 4.11 state it): the same algorithm in
the same operation order -- the weights' window, float distances and (distance, index) order, the rows of the energy term by term, every
entry of the normal matrix summed as rotation rows, then regularisation rows by (owner, slot), then constraints by index, the right-looking
banded L D L^T with the forward substitution riding along, the lane / wave / workgroup fold of the error sums.  The stage uses + - * / and
sqrt alone, so nothing is left to differ from the device.  Needs no GPU.

The state is (M, 12): A column-major (x[3 c + r] = A(r, c)), then b -- the reference's column order.
"""
from __future__ import annotations

import numpy as np

from .pose_graph_ref import fold_lanes

CONVERGED, MAX_STEPS, INSIGNIFICANT, SINGULAR = 0, 1, 2, 3      # kt_deform_status
PIVOT_MIN = 1e-12                                  # a pivot at or below this share of its diagonal entry of J^T J: singular
LOOKBACK = 20
BAND = 12 * LOOKBACK
SQ_REG = float(np.sqrt(10.0))
SQ_CON = 10.0
DEFAULTS = {"significant_error": 0.1, "delta_tol": 1e-2, "error_tol": 1e-3, "change_tol": 1e-5, "max_steps": 10}
BLOCK = 256


def sample_nodes(positions, pose_dist):
    """initialiseGraphPoses' loop (DeformationGraph.cpp:62-73): pose 0, then every pose farther than pose_dist (float norm) from the last kept"""
    p = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    keep = [0]
    for i in range(1, len(p)):
        d = p[keep[-1]] - p[i]
        if np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) > np.float32(pose_dist):
            keep.append(i)
    return np.array(keep, dtype=np.int64)


def neighbours(M):
    """connectGraphSeq, k = 4: (M, 4)"""
    nb = np.zeros((M, 4), dtype=np.int64)
    for i in range(M):
        if i < 2 or i >= M - 2:
            base = 0 if i < 2 else M - 5
            nb[i] = [n for n in range(base, base + 5) if n != i]
        else:
            nb[i] = [i - 1, i + 1, i - 2, i + 2]
    return nb


class Graph:
    def __init__(self, node_pos, node_time):
        self.gf = np.ascontiguousarray(node_pos, dtype=np.float32).reshape(-1, 3)
        self.gd = self.gf.astype(np.float64)
        self.gt = np.ascontiguousarray(node_time, dtype=np.uint64).reshape(-1)
        self.M = len(self.gf)
        assert self.M >= 5 and (self.gt[1:] > self.gt[:-1]).all()
        self.nb = neighbours(self.M)


def identity(M):
    x = np.zeros((M, 12))
    x[:, [0, 4, 8]] = 1.0
    return x


# ---- weights ------------------------------------------------------------------------------------------------------------------------------
def weights(g: Graph, pos, times):
    """weightVerticesSeq for vertices (n, 3) float32 with uint64 times -> idx (n, 4) int32 ascending, w (n, 4) float64"""
    p = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(times, dtype=np.uint64).reshape(-1)
    n, M = len(p), g.M
    if n == 0:
        return np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float64)
    lo = np.searchsorted(g.gt, t, side="left")
    a = np.abs((g.gt[np.clip(lo - 1, 0, M - 1)] - t).view(np.int64))       # wrapping unsigned difference read as signed
    b = np.abs((g.gt[np.clip(lo, 0, M - 1)] - t).view(np.int64))
    found = np.where(lo == 0, 0, np.where(lo == M, M - 1, np.where(a <= b, lo - 1, lo)))
    first = np.maximum(0, found - (LOOKBACK - 1))
    last = np.minimum(M - 1, first + (LOOKBACK - 1))
    W = LOOKBACK
    cand = first[:, None] + np.arange(W)[None, :]
    valid = cand <= last[:, None]
    candc = np.minimum(cand, M - 1)
    d = g.gf[candc] - p[:, None, :]
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])          # float32 throughout
    dist = np.where(np.isnan(dist), np.float32(np.inf), dist)
    key_i = np.where(valid, cand, np.iinfo(np.int64).max)
    dist = np.where(valid, dist, np.float32(np.inf))
    order = np.lexsort((key_i, dist), axis=-1)[:, :5]                       # by distance, then index
    bi = np.take_along_axis(cand, order, 1)
    bd = np.take_along_axis(dist, order, 1)
    dmax = bd[:, 4].astype(np.float64)
    pd = p.astype(np.float64)
    with np.errstate(all="ignore"):
        e = pd[:, None, :] - g.gd[bi[:, :4]]
        dd = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
        u = 1.0 - dd / dmax[:, None]
        ws = u * u
        s = ((ws[:, 0] + ws[:, 1]) + ws[:, 2]) + ws[:, 3]
        flat = (s == 0.0) | ~np.isfinite(s)
        ws = np.where(flat[:, None], 0.25, ws / s[:, None])
    o = np.argsort(bi[:, :4], axis=1, kind="stable")
    return np.take_along_axis(bi[:, :4], o, 1).astype(np.int32), np.take_along_axis(ws, o, 1)


# ---- the position of a vertex and the apply pass --------------------------------------------------------------------------------------------
def position(g: Graph, x, p, idx, w):
    """sum_i w_i (A_i (p - g_i) + g_i + b_i), nodes in ascending order; p (n, 3) float64"""
    o = np.zeros((len(p), 3))
    for s in range(4):
        xs, gs = x[idx[:, s]], g.gd[idx[:, s]]
        d = p - gs
        for r in range(3):
            t = (xs[:, r] * d[:, 0] + xs[:, 3 + r] * d[:, 1]) + xs[:, 6 + r] * d[:, 2]
            t = t + gs[:, r]
            t = t + xs[:, 9 + r]
            o[:, r] = o[:, r] + w[:, s] * t
    return o


def normal_mats(x):
    """A^-T of every node, (M, 3, 3): the cofactors and one division"""
    a00, a10, a20, a01, a11, a21, a02, a12, a22 = (x[:, k] for k in range(9))
    c = np.stack([a11 * a22 - a12 * a21, a12 * a20 - a10 * a22, a10 * a21 - a11 * a20,
                  a02 * a21 - a01 * a22, a00 * a22 - a02 * a20, a01 * a20 - a00 * a21,
                  a01 * a12 - a02 * a11, a02 * a10 - a00 * a12, a00 * a11 - a01 * a10], -1)
    det = (a00 * c[:, 0] + a01 * c[:, 1]) + a02 * c[:, 2]
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        return (c * inv[:, None]).reshape(-1, 3, 3)


def apply_points(g: Graph, x, points, idx, w):
    """applyGraphToVertices on a copy of abi.NPOINT_DTYPE points"""
    out = np.array(points, copy=True).reshape(-1)
    if len(out) == 0:
        return out
    p = out["xyz"].astype(np.float64)
    nn = out["normal"].astype(np.float64)
    with np.errstate(all="ignore"):
        o = position(g, x, p, idx, w)
        Nm = normal_mats(x)
        m = np.zeros((len(out), 3))
        for s in range(4):
            N = Nm[idx[:, s]]
            for r in range(3):
                t = (N[:, r, 0] * nn[:, 0] + N[:, r, 1] * nn[:, 1]) + N[:, r, 2] * nn[:, 2]
                m[:, r] = m[:, r] + w[:, s] * t
        ln = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        ok = (ln > 0.0) & (ln < np.inf)
        newn = (m / np.where(ok, ln, 1.0)[:, None]).astype(np.float32)
        out["xyz"] = o.astype(np.float32)
    out["normal"] = np.where(ok[:, None], newn, out["normal"])
    return out


def apply(g: Graph, x, points, times):
    """kt_deform_apply: weights, then apply"""
    pts = np.asarray(points).reshape(-1)
    idx, w = weights(g, pts["xyz"], times)
    return apply_points(g, x, pts, idx, w)


def apply_mesh(g: Graph, x, vertices, span_first, span_time):
    """kt_deform_apply_mesh on a copy of abi.MESH_VERTEX_DTYPE vertices: vertices [span_first[s], span_first[s + 1]) carry span_time[s]; the
    position is what apply gives a point there with that time, rounded to float32; rgb is copied"""
    out = np.array(vertices, copy=True).reshape(-1)
    first = np.ascontiguousarray(span_first, dtype=np.int64).reshape(-1)
    t = np.ascontiguousarray(span_time, dtype=np.uint64).reshape(-1)
    assert len(first) == len(t) + 1 and first[0] == 0 and first[-1] == len(out) and (first[1:] >= first[:-1]).all()
    if len(out) == 0:
        return out
    times = np.repeat(t, first[1:] - first[:-1])
    idx, w = weights(g, out["xyz"], times)
    with np.errstate(all="ignore"):
        out["xyz"] = position(g, x, out["xyz"].astype(np.float64), idx, w).astype(np.float32)
    return out


# ---- the energy -------------------------------------------------------------------------------------------------------------------------------
def jrot(A):
    """the six E_rot rows of one node over its nine rotation unknowns (sparseJacobian): (6, 9)"""
    J = np.zeros((6, 9))
    c0, c1, c2 = A[0:3], A[3:6], A[6:9]
    J[0, 0:3], J[0, 3:6] = c1, c0
    J[1, 0:3], J[1, 6:9] = c2, c0
    J[2, 3:6], J[2, 6:9] = c2, c1
    J[3, 0:3], J[4, 3:6], J[5, 6:9] = 2.0 * c0, 2.0 * c1, 2.0 * c2
    return J


def residuals(g: Graph, x, con):
    """rrot (M, 6), rreg (M, 4, 3), rcon (L, 3), error -- the error folded per workgroup of 256 nodes / constraints, nodes first"""
    M = g.M
    A = x
    rrot = np.stack([(A[:, 0] * A[:, 3] + A[:, 1] * A[:, 4]) + A[:, 2] * A[:, 5],
                     (A[:, 0] * A[:, 6] + A[:, 1] * A[:, 7]) + A[:, 2] * A[:, 8],
                     (A[:, 3] * A[:, 6] + A[:, 4] * A[:, 7]) + A[:, 5] * A[:, 8],
                     ((A[:, 0] * A[:, 0] + A[:, 1] * A[:, 1]) + A[:, 2] * A[:, 2]) - 1.0,
                     ((A[:, 3] * A[:, 3] + A[:, 4] * A[:, 4]) + A[:, 5] * A[:, 5]) - 1.0,
                     ((A[:, 6] * A[:, 6] + A[:, 7] * A[:, 7]) + A[:, 8] * A[:, 8]) - 1.0], -1)
    en = np.zeros(M)
    for e in range(6):
        en = en + rrot[:, e] * rrot[:, e]
    rreg = np.zeros((M, 4, 3))
    for k in range(4):
        n = g.nb[:, k]
        gn, gj, bn = g.gd[n], g.gd, x[n, 9:12]
        e = gn - gj
        for r in range(3):
            t = (A[:, r] * e[:, 0] + A[:, 3 + r] * e[:, 1]) + A[:, 6 + r] * e[:, 2]
            t = t + gj[:, r]
            t = t + A[:, 9 + r]
            res = (t - (gn[:, r] + bn[:, r])) * SQ_REG
            rreg[:, k, r] = res
            en = en + res * res
    e_nodes = 0.0
    for b0 in range(0, M, BLOCK):
        e_nodes = e_nodes + fold_lanes(en[b0:b0 + BLOCK, None])[0]
    L = len(con["idx"])
    rcon = np.zeros((L, 3))
    e_con = 0.0
    if L:
        o = position(g, x, con["src"], con["idx"], con["w"])
        ec = np.zeros(L)
        for r in range(3):
            rcon[:, r] = (o[:, r] - con["target"][:, r]) * SQ_CON
            ec = ec + rcon[:, r] * rcon[:, r]
        for b0 in range(0, L, BLOCK):
            e_con = e_con + fold_lanes(ec[b0:b0 + BLOCK, None])[0]
    return rrot, rreg, rcon, e_nodes, e_con


_P_A = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3])      # unknown p of a node = column a of [A | b] ...
_P_R = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2])      # ... row r
_SAME_R = (_P_R[:, None] == _P_R[None, :]).astype(np.float64)


def _vreg(gj, gn):
    return np.array([(gn[0] - gj[0]) * SQ_REG, (gn[1] - gj[1]) * SQ_REG, (gn[2] - gj[2]) * SQ_REG, SQ_REG])


_VNEG = np.array([0.0, 0.0, 0.0, -SQ_REG])


def _vcon(s, gi, w):
    return np.array([((s[0] - gi[0]) * w) * SQ_CON, ((s[1] - gi[1]) * w) * SQ_CON, ((s[2] - gi[2]) * w) * SQ_CON, w * SQ_CON])


def _expand(vi, vj):
    """the 12 x 12 block of a term that couples unknowns of equal row r: vi[a(p)] vj[a(q)]"""
    return np.outer(vi[_P_A], vj[_P_A]) * _SAME_R


def normal_equations(g: Graph, x, con, rrot, rreg, rcon):
    """H = J^T J (dense, lower blocks filled) and rhs = -J^T r; every entry: rotation rows, regularisation rows by (owner, slot), constraints
    by index"""
    M = g.M
    n = 12 * M
    H, grad = np.zeros((n, n)), np.zeros(n)
    for j in range(M):
        J = jrot(x[j])
        blk, gj = np.zeros((9, 9)), np.zeros(9)
        for row in range(6):
            blk = blk + np.outer(J[row], J[row])
            gj = gj + J[row] * rrot[j, row]
        H[12 * j:12 * j + 9, 12 * j:12 * j + 9] += blk
        grad[12 * j:12 * j + 9] += gj
    for m in range(M):
        for k in range(4):
            nn = int(g.nb[m, k])
            v = _vreg(g.gd[m], g.gd[nn])
            res = rreg[m, k][_P_R]
            H[12 * m:12 * m + 12, 12 * m:12 * m + 12] += _expand(v, v)
            H[12 * nn:12 * nn + 12, 12 * nn:12 * nn + 12] += _expand(_VNEG, _VNEG)
            hi, lo, vh, vl = (nn, m, _VNEG, v) if nn > m else (m, nn, v, _VNEG)
            H[12 * hi:12 * hi + 12, 12 * lo:12 * lo + 12] += _expand(vh, vl)
            grad[12 * m:12 * m + 12] += v[_P_A] * res
            grad[12 * nn:12 * nn + 12] += _VNEG[_P_A] * res
    for l in range(len(con["idx"])):
        ids, ws, s = con["idx"][l], con["w"][l], con["src"][l]
        vs = [_vcon(s, g.gd[ids[a]], ws[a]) for a in range(4)]
        res = rcon[l][_P_R]
        for a in range(4):
            grad[12 * ids[a]:12 * ids[a] + 12] += vs[a][_P_A] * res
            for b in range(a + 1):                     # ids ascending: block (ids[a], ids[b]) is in the lower triangle
                H[12 * ids[a]:12 * ids[a] + 12, 12 * ids[b]:12 * ids[b] + 12] += _expand(vs[a], vs[b])
    return H, -grad


def band_solve(H, y):
    """the right-looking banded L D L^T on the lower triangle (half-bandwidth 239), the forward substitution riding along, the diagonal, the
    backward substitution.  H is overwritten; returns delta, or None when a pivot is not finite or not above PIVOT_MIN of the diagonal entry
    it started from."""
    n = len(y)
    y = y.copy()
    diag0 = np.diagonal(H).copy()
    singular = False
    for j in range(n):
        w = min(BAND - 1, n - 1 - j)
        with np.errstate(all="ignore"):
            singular = singular or not (H[j, j] > PIVOT_MIN * diag0[j] and H[j, j] < np.inf)
        a = H[j + 1:j + 1 + w, j].copy()
        lc = a / H[j, j]
        H[j + 1:j + 1 + w, j] = lc
        y[j + 1:j + 1 + w] = y[j + 1:j + 1 + w] - lc * y[j]
        H[j + 1:j + 1 + w, j + 1:j + 1 + w] -= lc[:, None] * a[None, :]
    if singular:
        return None
    y = y / np.diagonal(H)
    for j in range(n - 1, 0, -1):
        i0 = max(0, j - (BAND - 1))
        y[i0:j] = y[i0:j] - H[j, i0:j] * y[j]
    return y


def constraints(g: Graph, src_pos, src_time, target):
    src = np.ascontiguousarray(src_pos, dtype=np.float32).reshape(-1, 3)
    idx, w = weights(g, src, src_time)
    return {"src": src.astype(np.float64), "idx": idx.astype(np.int64), "w": w, "target": np.ascontiguousarray(target, dtype=np.float64).reshape(-1, 3)}


def optimise(g: Graph, src_pos=(), src_time=(), target=(), params=None):
    """kt_deform_optimise, from the identity state.  Returns state (M, 12), error_start, error_end, constraint_error, steps, status and the
    trace: [(|delta|, error, |error - lastError|, error)] per step taken -- the quantities of the stop rule."""
    p = dict(DEFAULTS)
    p.update(params or {})
    con = constraints(g, src_pos, src_time, target)
    L = len(con["idx"])
    x = identity(g.M)
    rrot, rreg, rcon, e_nodes, e_con = residuals(g, x, con)
    err = e_nodes + e_con
    error_start = error_end = last = err
    ce = float(np.sqrt(e_con)) / L if L else 0.0
    trace = []
    if L == 0 or ce < p["significant_error"]:
        return x, error_start, error_end, ce, 0, INSIGNIFICANT, trace
    steps, status = 0, MAX_STEPS
    for step in range(1, p["max_steps"] + 1):
        H, rhs = normal_equations(g, x, con, rrot, rreg, rcon)
        with np.errstate(all="ignore"):
            delta = band_solve(H, rhs)
        if delta is None:                                  # the state stays the one before this step
            status = SINGULAR
            break
        x = (x.reshape(-1) + delta).reshape(-1, 12)
        sq = delta * delta
        d2 = 0.0
        for b0 in range(0, len(sq), BLOCK):
            d2 = d2 + fold_lanes(sq[b0:b0 + BLOCK, None])[0]
        rrot, rreg, rcon, e_nodes, e_con = residuals(g, x, con)
        err = e_nodes + e_con
        steps, error_end = step, err
        dn = float(np.sqrt(d2))
        trace.append((dn, err, abs(err - last), err))
        if dn < p["delta_tol"] or err < p["error_tol"] or abs(err - last) < p["change_tol"] * err:
            status = CONVERGED
            break
        last = err
    return x, error_start, error_end, ce, steps, status, trace
