"""numpy restatement of the pose-graph stage (csrc/kt_posegraph.hip; include/kt_abi.h and DESIGN.md 4.10 state it): the same algorithm in the
same operation order -- the scan tree of the pose composition, the loops visited in index order, the lane / wave / workgroup fold of the
pair reduction, the right-looking LDLT.  Products and sums are written out term by term (numpy's matmul would pick its own order); what is
left to differ from the device is the last bit of sin, cos, atan2 and sqrt.  Needs no GPU.

Conventions: a pose is (R, t) with R (..., 3, 3) and t (..., 3); a tangent vector is [v; w] (translation first); Exp([v; w]) =
[Exp_SO3(w) | v], which agrees with SE(3)'s exponential to first order (all a Gauss-Newton step asks of a retraction).
"""
from __future__ import annotations

import numpy as np

CONVERGED, MAX_STEPS = 0, 1          # KT_POSE_GRAPH_CONVERGED, KT_POSE_GRAPH_MAX_STEPS
MAX_STEPS_N = 20
DELTA_TOL = 1e-9
CHI2_SCALE = 1000.0                  # every factor of the reference has covariance 1e-3 I
BLOCK = 256                          # lanes of a workgroup: the scan's block and the pair reduction's stride


# ---- ordered small products -------------------------------------------------------------------------------------------------------------
def mm(A, B):
    """(..., n, p) x (..., p, m): every entry the sum over the inner index in ascending order"""
    acc = A[..., :, 0, None] * B[..., None, 0, :]
    for c in range(1, A.shape[-1]):
        acc = acc + A[..., :, c, None] * B[..., None, c, :]
    return acc


def mv(A, x):
    acc = A[..., :, 0] * x[..., None, 0]
    for c in range(1, A.shape[-1]):
        acc = acc + A[..., :, c] * x[..., None, c]
    return acc


def tr(A):
    return np.swapaxes(A, -1, -2)


def se3_mul(Ra, ta, Rb, tb):
    return mm(Ra, Rb), mv(Ra, tb) + ta


def se3_inv(R, t):
    Rt = tr(R)
    return Rt, -mv(Rt, t)


def hat(w):
    z = np.zeros_like(w[..., 0])
    return np.stack([np.stack([z, -w[..., 2], w[..., 1]], -1), np.stack([w[..., 2], z, -w[..., 0]], -1), np.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def so3_exp(w):
    """Rodrigues: I + A [w]x + B [w]x^2, A = sin(th) / th, B = (1 - cos(th)) / th^2 (their series below th = 1e-4)"""
    th2 = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
    th = np.sqrt(th2)
    small = th < 1e-4
    ths = np.where(small, 1.0, th)
    A = np.where(small, 1.0 - th2 / 6.0, np.sin(ths) / ths)
    B = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(ths)) / (ths * ths))
    K = hat(w)
    return np.eye(3) + A[..., None, None] * K + B[..., None, None] * mm(K, K)


def so3_log(R):
    """the rotation vector of R for angles away from pi: a = vee(R - R^T) / 2, s = |a| = sin, c = (tr - 1) / 2, th = atan2(s, c)"""
    a = np.stack([(R[..., 2, 1] - R[..., 1, 2]) * 0.5, (R[..., 0, 2] - R[..., 2, 0]) * 0.5, (R[..., 1, 0] - R[..., 0, 1]) * 0.5], -1)
    s = np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])
    c = (((R[..., 0, 0] + R[..., 1, 1]) + R[..., 2, 2]) - 1.0) * 0.5
    small = s < 1e-5
    f = np.where(small, 1.0 + s * s / 6.0, np.arctan2(s, c) / np.where(small, 1.0, s))
    return a * f[..., None]


def so3_jr_inv(phi):
    """d Log(R Exp(w)) / dw at w = 0, R = Exp(phi): I + [phi]x / 2 + c2 [phi]x^2"""
    th2 = (phi[..., 0] * phi[..., 0] + phi[..., 1] * phi[..., 1]) + phi[..., 2] * phi[..., 2]
    th = np.sqrt(th2)
    small = th < 1e-2
    ths = np.where(small, 1.0, th)
    c2 = np.where(small, (1.0 / 12.0 + th2 / 720.0) + th2 * th2 / 30240.0, 1.0 / (ths * ths) - (1.0 + np.cos(ths)) / ((2.0 * ths) * np.sin(ths)))
    K = hat(phi)
    return np.eye(3) + 0.5 * K + c2[..., None, None] * mm(K, K)


def residual(R, t):
    """r = [trans(E); Log_SO3(rot(E))]"""
    return np.concatenate([t, so3_log(R)], -1)


def jr(R, phi):
    """Jr(E): d r(E Exp(xi)) / d xi at 0 = [[R_E, 0], [0, Jr_SO3^-1(phi)]]"""
    J = np.zeros(R.shape[:-2] + (6, 6))
    J[..., :3, :3] = R
    J[..., 3:, 3:] = so3_jr_inv(phi)
    return J


def adjoint(R, t):
    """Ad(P) on [v; w]: [[R, [t]x R], [0, R]]"""
    A = np.zeros(R.shape[:-2] + (6, 6))
    A[..., :3, :3] = R
    A[..., :3, 3:] = mm(hat(t), R)
    A[..., 3:, 3:] = R
    return A


def ldlt6_inverse(H):
    """the inverse of symmetric positive definite 6x6 blocks through an unpivoted L D L^T, column by column, then six solves"""
    n = H.shape[-1]
    L = np.zeros_like(H)
    d = np.zeros(H.shape[:-1])
    for j in range(n):
        s = H[..., j, j]
        for p in range(j):
            s = s - (L[..., j, p] * L[..., j, p]) * d[..., p]
        d[..., j] = s
        L[..., j, j] = 1.0
        for i in range(j + 1, n):
            s2 = H[..., i, j]
            for p in range(j):
                s2 = s2 - (L[..., i, p] * L[..., j, p]) * d[..., p]
            L[..., i, j] = s2 / d[..., j]
    inv = np.zeros_like(H)
    for c in range(n):
        y = np.zeros(H.shape[:-1])
        for i in range(n):
            s = np.full(H.shape[:-2], 1.0 if i == c else 0.0)
            for p in range(i):
                s = s - L[..., i, p] * y[..., p]
            y[..., i] = s
        y = y / d
        for i in range(n - 1, -1, -1):
            s = y[..., i]
            for p in range(i + 1, n):
                s = s - L[..., p, i] * y[..., p]
            y[..., i] = s
        inv[..., :, c] = y
    return inv


# ---- the measurement ----------------------------------------------------------------------------------------------------------------------
def quat_rotation(R):
    """the rotation of R's normalised quaternion (w, x, y, z), taken from the largest of {trace, R00, R11, R22} (Shepperd)"""
    R = np.asarray(R, dtype=np.float64)
    t = (R[0, 0] + R[1, 1]) + R[2, 2]
    if t >= R[0, 0] and t >= R[1, 1] and t >= R[2, 2]:
        q = np.array([1.0 + t, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        q = np.array([R[2, 1] - R[1, 2], ((1.0 + R[0, 0]) - R[1, 1]) - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif R[1, 1] >= R[2, 2]:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], ((1.0 - R[0, 0]) + R[1, 1]) - R[2, 2], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], ((1.0 - R[0, 0]) - R[1, 1]) + R[2, 2]])
    q = q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    w, x, y, z = q
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def measurement(prev16, curr16):
    """kt_host_pose_graph_measurement: Z = prev^-1 curr of two float poses, rotations re-made from their normalised quaternions, in double"""
    P = np.asarray(prev16, dtype=np.float32).reshape(4, 4).astype(np.float64)
    Cm = np.asarray(curr16, dtype=np.float32).reshape(4, 4).astype(np.float64)
    Rp, Rc = quat_rotation(P[:3, :3]), quat_rotation(Cm[:3, :3])
    Ri, ti = se3_inv(Rp, P[:3, 3])
    R, t = se3_mul(Ri, ti, Rc, Cm[:3, 3])
    Z = np.eye(4)
    Z[:3, :3], Z[:3, 3] = R, t
    return Z


# ---- the stage ----------------------------------------------------------------------------------------------------------------------------
def compose(Re, te):
    """inclusive scan of SE(3) products over elements e_0 .. e_{n-1}: Hillis-Steele inside blocks of 256 (the tail padded with identities),
    one workgroup over the block totals (a serial run per lane, Hillis-Steele over the lanes), then base x local"""
    n = Re.shape[0]
    nb = (n + BLOCK - 1) // BLOCK
    R = np.tile(np.eye(3), (nb * BLOCK, 1, 1))
    t = np.zeros((nb * BLOCK, 3))
    R[:n], t[:n] = Re, te
    R, t = R.reshape(nb, BLOCK, 3, 3), t.reshape(nb, BLOCK, 3)
    off = 1
    while off < BLOCK:
        Rn, tn = se3_mul(R[:, :-off], t[:, :-off], R[:, off:], t[:, off:])
        R, t = np.concatenate([R[:, :off], Rn], 1), np.concatenate([t[:, :off], tn], 1)
        off <<= 1
    if nb > 1:
        totR, tott = R[:, BLOCK - 1], t[:, BLOCK - 1]
        per = (nb + BLOCK - 1) // BLOCK
        sR, st = np.tile(np.eye(3), (BLOCK, 1, 1)), np.zeros((BLOCK, 3))
        for lane in range(BLOCK):
            for i in range(lane * per, min(nb, (lane + 1) * per)):
                sR[lane], st[lane] = se3_mul(sR[lane], st[lane], totR[i], tott[i])
        off = 1
        while off < BLOCK:
            Rn, tn = se3_mul(sR[:-off], st[:-off], sR[off:], st[off:])
            sR, st = np.concatenate([sR[:off], Rn], 0), np.concatenate([st[:off], tn], 0)
            off <<= 1
        baseR, baset = np.empty((nb, 3, 3)), np.empty((nb, 3))
        for lane in range(BLOCK):
            bR, bt = (np.eye(3), np.zeros(3)) if lane == 0 else (sR[lane - 1], st[lane - 1])
            for i in range(lane * per, min(nb, (lane + 1) * per)):
                baseR[i], baset[i] = bR, bt
                bR, bt = se3_mul(bR, bt, totR[i], tott[i])
        R, t = se3_mul(baseR[:, None], baset[:, None], R, t)
    return R.reshape(-1, 3, 3)[:n], t.reshape(-1, 3)[:n]


def fold_lanes(rows):
    """sum of rows (cnt, w) the way a workgroup of 256 lanes does it: lane t takes rows t, t + 256, ... in order, kt_wave_sum's xor butterfly
    inside every wave, then the four waves in order"""
    cnt, w = rows.shape
    lanes = np.zeros((BLOCK, w))
    for c in range(0, cnt, BLOCK):
        m = min(BLOCK, cnt - c)
        lanes[:m] = lanes[:m] + rows[c:c + m]
    v = lanes.reshape(BLOCK // 64, 64, w)
    idx = np.arange(64)
    off = 32
    while off > 0:
        v = v + v[:, idx ^ off]
        off >>= 1
    out = v[0, 0]
    for k in range(1, BLOCK // 64):
        out = out + v[k, 0]
    return out


def normalise_loops(loop_a, loop_b, loop_Z):
    """every loop as (i, j, Z) with i < j: a swapped pair takes the rigid inverse of its measurement"""
    li, lj, ZR, Zt = [], [], [], []
    for a, b, Z in zip(loop_a, loop_b, loop_Z):
        Z = np.asarray(Z, dtype=np.float64).reshape(4, 4)
        R, t = Z[:3, :3], Z[:3, 3]
        if a > b:
            a, b = b, a
            R, t = se3_inv(R, t)
        li.append(int(a)); lj.append(int(b)); ZR.append(R); Zt.append(t)
    L = len(li)
    return np.array(li, dtype=np.int64), np.array(lj, dtype=np.int64), np.array(ZR).reshape(L, 3, 3), np.array(Zt).reshape(L, 3)


class State:
    pass


def evaluate(s):
    """launches 1 and 2 of a step: poses, the loops' and the nodes' residuals and blocks, the cost"""
    N, L = s.N, s.L
    s.TR, s.Tt = compose(s.DR, s.Dt)
    if L:
        iR, it = se3_inv(s.TR[s.li], s.Tt[s.li])
        R, t = se3_mul(iR, it, s.TR[s.lj], s.Tt[s.lj])
        ER, Et = se3_mul(s.ZiR, s.Zit, R, t)
        s.rl = residual(ER, Et)
        s.Jl = jr(ER, s.rl[..., 3:])
        jR, jt = se3_inv(s.TR[s.lj], s.Tt[s.lj])
        s.B = mm(s.Jl, adjoint(jR, jt))                     # A_lk = B_l Ad(T_k)
        s.q = mv(tr(s.B), s.rl)
        cl = np.zeros(L)
        for c in range(6):
            cl = cl + s.rl[:, c] * s.rl[:, c]
    k = np.arange(1, N)
    ER, Et = se3_mul(s.CiR, s.Cit, s.DR[1:], s.Dt[1:])
    r = residual(ER, Et)
    J = jr(ER, r[..., 3:])
    s.Hinv = ldlt6_inverse(mm(tr(J), J))
    g = mv(tr(J), r)
    sq = np.zeros((N - 1, 6))
    for l in range(L):
        cover = (s.li[l] < k) & (k <= s.lj[l])
        sq[cover] = sq[cover] + s.q[l]
    s.Ad = adjoint(s.TR[1:], s.Tt[1:])
    b = -(g + mv(tr(s.Ad), sq))
    s.u = mv(s.Hinv, b)
    s.G = mm(mm(s.Ad, s.Hinv), tr(s.Ad)).reshape(N - 1, 36)
    s.h = mv(s.Ad, s.u)
    ck = np.zeros(N - 1)
    for c in range(6):
        ck = ck + r[:, c] * r[:, c]
    # the cost: a partial per workgroup of 256 nodes (index k - 1), the partials and then the loops in order
    cost = 0.0
    for b0 in range(0, N - 1, BLOCK):
        cost = cost + fold_lanes(ck[b0:b0 + BLOCK, None])[0]
    for l in range(L):
        cost = cost + cl[l]
    return cost


def step(s):
    """launches 3 - 5: S and v, the dense LDLT, the update; returns max |delta|_inf"""
    N, L = s.N, s.L
    n = 6 * L
    S, v = np.zeros((n, n)), np.zeros(n)
    for l in range(L):
        for m in range(l, L):
            lo, hi = max(s.li[l], s.li[m]) + 1, min(s.lj[l], s.lj[m])     # nodes k in [lo, hi]; row k - 1 of the per-node arrays
            M = fold_lanes(s.G[lo - 1:hi]).reshape(6, 6) if lo <= hi else np.zeros((6, 6))
            blk = mm(mm(s.B[l], M), tr(s.B[m]))
            if l == m:
                blk = blk + np.eye(6)
                v[6 * l:6 * l + 6] = mv(s.B[l], fold_lanes(s.h[lo - 1:hi]))
            S[6 * l:6 * l + 6, 6 * m:6 * m + 6] = blk              # the solve reads the lower triangle: a diagonal block entry by entry,
            if l != m:                                             # an off-diagonal one as its mirror
                S[6 * m:6 * m + 6, 6 * l:6 * l + 6] = blk.T
    d = np.zeros(n)
    y = v.copy()
    for j in range(n):                                   # right-looking: column j, then the trailing block
        d[j] = S[j, j]
        a = S[j + 1:, j].copy()
        lcol = a / d[j]
        S[j + 1:, j] = lcol
        S[j + 1:, j + 1:] = S[j + 1:, j + 1:] - lcol[:, None] * a[None, :]
    for j in range(n):
        y[j + 1:] = y[j + 1:] - S[j + 1:, j] * y[j]
    y = y / d
    for j in range(n - 1, -1, -1):
        y[:j] = y[:j] - S[j, :j] * y[j]
    z = mv(tr(s.B), y.reshape(L, 6))
    k = np.arange(1, N)
    sz = np.zeros((N - 1, 6))
    for l in range(L):
        cover = (s.li[l] < k) & (k <= s.lj[l])
        sz[cover] = sz[cover] + z[l]
    delta = s.u - mv(s.Hinv, mv(tr(s.Ad), sz))
    s.DR[1:], s.Dt[1:] = mm(s.DR[1:], so3_exp(delta[:, 3:])), mv(s.DR[1:], delta[:, :3]) + s.Dt[1:]
    return float(np.max(np.abs(delta)))


def optimise(T0, chain_Z, loop_a=(), loop_b=(), loop_Z=()):
    """kt_pose_graph_optimise.  T0 (4, 4); chain_Z (N - 1, 4, 4); loops as the ABI takes them.
    Returns poses (N, 4, 4), chi2_start, chi2_end, steps, status, and max |delta| of every step taken."""
    T0 = np.asarray(T0, dtype=np.float64).reshape(4, 4)
    chain_Z = np.asarray(chain_Z, dtype=np.float64).reshape(-1, 4, 4)
    s = State()
    s.N, s.L = chain_Z.shape[0] + 1, len(loop_a)
    # the solver works relative to node 0 (element 0 of the scan is the identity): the adjoints' entries grow with the distance from the frame's
    # origin, so the frame sits where the trajectory starts; T_0 is multiplied back in at the end and node 0 keeps the caller's bits
    s.DR = np.concatenate([np.eye(3)[None], chain_Z[:, :3, :3]], 0).copy()
    s.Dt = np.concatenate([np.zeros((1, 3)), chain_Z[:, :3, 3]], 0).copy()

    def poses():
        P = np.tile(np.eye(4), (s.N, 1, 1))
        P[:, :3, :3], P[:, :3, 3] = se3_mul(T0[:3, :3], T0[:3, 3], s.TR, s.Tt)
        P[0] = T0
        return P

    if s.L == 0:                                         # nothing to optimise: the start, after a zero step
        s.TR, s.Tt = compose(s.DR, s.Dt)
        cost = 0.0
        if s.N > 1:
            s.li = s.lj = np.zeros(0, dtype=np.int64)
            s.CiR, s.Cit = se3_inv(chain_Z[:, :3, :3], chain_Z[:, :3, 3])
            cost = evaluate(s)
        return poses(), CHI2_SCALE * cost, CHI2_SCALE * cost, 0, CONVERGED, []
    s.li, s.lj, ZR, Zt = normalise_loops(loop_a, loop_b, loop_Z)
    s.ZiR, s.Zit = se3_inv(ZR, Zt)
    s.CiR, s.Cit = se3_inv(chain_Z[:, :3, :3], chain_Z[:, :3, 3])
    cost = evaluate(s)
    chi2_start = chi2_end = CHI2_SCALE * cost
    steps, status, deltas = 0, MAX_STEPS, []
    for it in range(1, MAX_STEPS_N + 1):
        md = step(s)
        chi2_end = CHI2_SCALE * evaluate(s)
        steps = it
        deltas.append(md)
        if md < DELTA_TOL:
            status = CONVERGED
            break
    return poses(), chi2_start, chi2_end, steps, status, deltas
