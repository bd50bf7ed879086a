"""The Gauss-Newton tail of the reduction kernels in its two device forms: one thread (the restatement of Eigen's LDLT / cv::Rodrigues /
the Isometry3f update that the oracle shares, csrc/kt_track.hpp) against the lane-parallel form the kernels run
(kt_solve_and_update_wave).  Every output bit must agree, also where the pivot order hangs on ties, for singular and indefinite systems,
zeros and NaNs."""
import ctypes as C

import numpy as np
import pytest

from kintinuous_amd import abi

pytestmark = pytest.mark.gpu

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
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th ** 2) * (K @ K) if th > 0 else np.eye(3)


def _cases(n, seed):
    rng = np.random.default_rng(seed)
    cs = np.zeros(n, CASE)
    for k in range(n):
        kind = k % 12
        m = int(rng.integers(3, 400))
        J = rng.normal(size=(m, 6)).astype(np.float32) * np.float32(10.0 ** rng.uniform(-2, 2))
        r = rng.normal(size=m).astype(np.float32) * np.float32(10.0 ** rng.uniform(-4, 0))
        A = (J.T @ J).astype(np.float32)
        b = (J.T @ r).astype(np.float32)
        if kind == 1:     # ties on the diagonal: the pivot order is decided by the swap history
            d = rng.permutation(np.array([3.0, 3.0, 5.0, 1.0, 3.0, 5.0], np.float32))
            A = (A * np.float32(1e-3)).astype(np.float32)
            A[np.arange(6), np.arange(6)] = d
        elif kind == 2:   # all diagonal entries equal
            A[np.arange(6), np.arange(6)] = np.float32(7.0)
        elif kind == 3:   # rank deficient: rows / columns of zeros (no correspondences constrain them)
            z = rng.choice(6, size=int(rng.integers(1, 5)), replace=False)
            A[z, :] = 0; A[:, z] = 0; b[z] = 0
        elif kind == 4:   # nothing at all
            A[:] = 0; b[:] = 0
        elif kind == 5:   # rank 1 / rank 2
            J2 = J[: int(rng.integers(1, 3))]
            A = (J2.T @ J2).astype(np.float32); b = (J2.T @ r[: len(J2)]).astype(np.float32)
        elif kind == 6:   # indefinite
            A = (A - np.float32(0.5) * np.diag(np.diag(A))).astype(np.float32)
            A[2, 2] = -A[2, 2]
        elif kind == 7:   # a NaN / an infinity somewhere
            A[int(rng.integers(6)), int(rng.integers(6))] = np.float32(np.nan if k % 2 else np.inf)
            A = np.triu(A) + np.triu(A, 1).T
        elif kind == 8:   # a tiny increment: Rodrigues' theta < eps branch
            b = (b * np.float32(1e-30)).astype(np.float32)
        elif kind == 9:   # a huge increment: the large-argument path of sin / cos
            b = (b * np.float32(1e6)).astype(np.float32)
        cs[k]["packed"] = _pack(A, b)
        if kind == 10 or kind == 11:   # the joint RGB-D + ICP combination
            J3 = rng.normal(size=(m, 6)).astype(np.float32)
            cs[k]["packed2"] = _pack((J3.T @ J3).astype(np.float32), (J3.T @ r).astype(np.float32))
            cs[k]["joint"] = 1
        T = np.eye(4)
        T[:3, :3] = _rot(rng, 0.05); T[:3, 3] = rng.normal(size=3) * 0.05
        cs[k]["resultRt"] = T.reshape(16)
        cs[k]["posef"][:9] = _rot(rng, 1.0).astype(np.float32).reshape(9)
        cs[k]["posef"][9:] = (rng.normal(size=3) * 3).astype(np.float32)
    return cs


def test_lane_parallel_tail_equals_the_serial_one():
    ctx = abi.Ctx(0)
    layout = (C.c_int * 5)()
    abi._chk(abi.lib().kt_debug_solve_check(ctx.h, 0, None, None, None, layout))
    size, o_rt, o_R, o_t, case_size = list(layout)
    assert case_size == CASE.itemsize
    n = 6000
    cs = _cases(n, 20240924)
    ser = np.zeros((n, size), np.uint8)
    wav = np.zeros((n, size), np.uint8)
    abi._chk(abi.lib().kt_debug_solve_check(ctx.h, n, cs.ctypes.data_as(C.c_void_p), ser.ctypes.data_as(C.c_void_p), wav.ctypes.data_as(C.c_void_p), layout))
    fields = {"resultRt": (o_rt, 128), "Rcurr": (o_R, 36), "tcurr": (o_t, 12)}
    # the serial form did something (not a buffer of zeros), and the two agree in every byte of every output
    assert np.any(ser[:, o_rt:o_rt + 128] != 0)
    for name, (off, nb) in fields.items():
        ty = np.float64 if name == "resultRt" else np.float32
        a, b = ser[:, off:off + nb].copy().view(ty), wav[:, off:off + nb].copy().view(ty)
        # a NaN is a NaN (its sign and payload are not the reference's either: x86 and gfx950 differ there); everything else bit for bit
        same = (np.isnan(a) & np.isnan(b)) | (a.view(np.uint64 if ty is np.float64 else np.uint32) == b.view(np.uint64 if ty is np.float64 else np.uint32))
        bad = np.nonzero(~np.all(same, axis=1))[0]
        assert bad.size == 0, (name, bad[:10], [int(k) % 12 for k in bad[:10]], a[bad[0]], b[bad[0]])
    # healthy systems produce finite poses (the comparison above is not NaN against NaN throughout)
    healthy = [k for k in range(n) if k % 12 == 0]
    assert np.all(np.isfinite(ser[healthy][:, o_rt:o_rt + 128].copy().view(np.float64)))
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# Both device forms against the independent reference (tests/tools/gn_reference.py through the table tests/golden/gn_cases_v1.npz): the
# checks and bars are those of tests/test_gn_reference.py (tests/tools/gn_checks.py).  The hook returns resultRt, Rcurr and tcurr, not x: a system goes in with
# resultRt = I, so that the translation column of the new resultRt IS x[0:3] (1 * x + 0 * R, exact); its partner in the table -- the same
# system with the halves of the unknowns exchanged -- shows the other three.  A rotation vector / translation goes in as b over an
# identity A through the joint combination b_rgbd + 10 b_icp, which forms the table's doubles exactly from two floats each.
# ---------------------------------------------------------------------------------------------------------------------------------
def _gn_checks():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "gn_checks.py")
    spec = importlib.util.spec_from_file_location("gn_checks", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _two_float(v):
    b1 = np.asarray(v, np.float64).astype(np.float32)
    b2 = ((v - b1.astype(np.float64)) / 10.0).astype(np.float32)
    assert np.array_equal(b1.astype(np.float64) + 10.0 * b2.astype(np.float64), v)
    return b1, b2


def _device_table(T, gn):
    from kintinuous_amd import abi
    recs, what = [], []          # what: ("solve", system) | ("rot", row, resultRt in, prev pose)
    eye12 = np.r_[np.eye(3).reshape(9), np.zeros(3)].astype(np.float32)

    def increment(row, state, prev):
        c = np.zeros((), CASE)
        b1, b2 = _two_float(np.r_[T["r_t"][row], T["r_vec"][row]])
        c["packed"], c["packed2"], c["joint"] = _pack(np.eye(6), b1), _pack(np.zeros((6, 6)), b2), 1
        c["resultRt"], c["posef"] = np.asarray(state, np.float64).reshape(16), prev
        recs.append(c)
        what.append(("rot", row, np.array(state, np.float64), prev))

    for i in np.nonzero(T["s_f32"])[0]:
        c = np.zeros((), CASE)
        c["packed"], c["resultRt"], c["posef"] = _pack(T["s_A"][i], T["s_b"][i]), np.eye(4).reshape(16), eye12
        recs.append(c)
        what.append(("solve", int(i)))
    for row in range(int(T["n6"])):
        increment(row, np.eye(4), T["c_prev"][row % len(T["c_prev"])])
    for c in range(len(T["c_len"])):   # every step of a chain from the state the host ABI reached before it
        for row, k, state, new, Rc, tc, prev, exact in gn.host_chain(T, c, abi.host_pose_update):
            increment(row, state, prev)
    return np.array(recs, CASE), what


def _check_against_reference(T, gn, what, res):
    from kintinuous_amd import abi
    # the two forms agree in every bit on the whole table (nothing in it is a NaN)
    for a, b in zip(res["serial"], res["wave"]):
        assert np.all(np.isfinite(a)) and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    where = {w[1]: k for k, w in enumerate(what) if w[0] == "solve"}
    SWAP = [3, 4, 5, 0, 1, 2]
    eps = 2.0 ** -52
    for form, (rt, Rc, tc) in res.items():
        worst = {"fwd": 0.0, "bwd": 0.0, "rot": 0.0, "rt": 0.0, "Rcurr": 0.0, "tcurr": 0.0}
        decided = {2: [0, 0], 3: [0, 0], 4: [0, 0]}
        below = 0
        for k, w in enumerate(what):
            if w[0] == "solve":
                i = w[1]
                cls, pair = int(T["s_cls"][i]), int(T["s_pair"][i])
                x3 = rt[k, :3, 3]
                if cls in (1, 5):
                    if i < pair:     # the whole x from the system and its partner (no ties: the same pivots on the same numbers)
                        assert np.array_equal(T["s_x"][pair], T["s_x"][i][SWAP])
                        f, b = gn.check_solve_values(T, i, np.r_[x3, rt[where[pair], :3, 3]], form)
                        worst["fwd"], worst["bwd"] = max(worst["fwd"], f or 0.0), max(worst["bwd"], b or 0.0)
                else:
                    decided[cls][1] += 1
                    decided[cls][0] += int(gn.check_solve_decisions(T, i, np.r_[x3, np.zeros(3)], form, unknowns=range(3)))
                # below the theta < DBL_EPSILON branch no libm call is made: the device and the host ABI may not differ in any bit
                x = abi.host_ldlt_solve6(T["s_A"][i], T["s_b"][i])
                if np.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]) < eps:
                    hrt, hR, ht = abi.host_pose_update(x, np.eye(4), np.eye(3), np.zeros(3))
                    assert np.array_equal(hrt.view(np.uint64), rt[k].view(np.uint64)) and np.array_equal(hR.view(np.uint32), Rc[k].view(np.uint32)) \
                        and np.array_equal(ht.view(np.uint32), tc[k].view(np.uint32)), (form, i, x, hrt, rt[k])
                    below += 1
            else:
                _, row, state, prev = w
                worst["rot"] = max(worst["rot"], gn.check_rotation(T, row, rt[k, :3, :3], form) * 8 * gn.U / gn.rotation_bar(T["r_vec"][row])[0]) \
                    if np.array_equal(state, np.eye(4)) else worst["rot"]
                r = T["r_vec"][row]
                if gn.rotation_bar(r)[1] < 10:
                    e = gn.check_step(T, row, state, rt[k], Rc[k], tc[k], prev, form)
                    worst["rt"], worst["Rcurr"], worst["tcurr"] = max(worst["rt"], e[0]), max(worst["Rcurr"], e[1]), max(worst["tcurr"], e[2])
                if np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) < eps:
                    hrt, hR, ht = abi.host_pose_update(np.r_[T["r_t"][row], r], state, prev[:9], prev[9:])
                    assert np.array_equal(hrt.view(np.uint64), rt[k].view(np.uint64)) and np.array_equal(hR.view(np.uint32), Rc[k].view(np.uint32)) \
                        and np.array_equal(ht.view(np.uint32), tc[k].view(np.uint32)), (form, row, hrt, rt[k])
                    below += 1
        print(form, "worst:", {k: round(v, 3) for k, v in worst.items()}, "decided:", decided, "bit-compared below the branch:", below)
        for cls, (done, total) in decided.items():
            assert done >= (0.9 if cls == 4 else 0.98) * total, (form, cls, done, total)
        assert below >= 50


def test_both_device_forms_against_the_independent_reference():
    gn = _gn_checks()
    from kintinuous_amd import abi
    T = gn.table()
    cs, what = _device_table(T, gn)
    n = len(cs)
    assert 2000 < n < 6000
    ctx = abi.Ctx(0)
    layout = (C.c_int * 5)()
    abi._chk(abi.lib().kt_debug_solve_check(ctx.h, 0, None, None, None, layout))
    size, o_rt, o_R, o_t, case_size = list(layout)
    assert case_size == CASE.itemsize
    out = {"serial": np.zeros((n, size), np.uint8), "wave": np.zeros((n, size), np.uint8)}
    abi._chk(abi.lib().kt_debug_solve_check(ctx.h, n, cs.ctypes.data_as(C.c_void_p), out["serial"].ctypes.data_as(C.c_void_p),
                                            out["wave"].ctypes.data_as(C.c_void_p), layout))
    ctx.close()
    res = {f: (o[:, o_rt:o_rt + 128].copy().view(np.float64).reshape(n, 4, 4), o[:, o_R:o_R + 36].copy().view(np.float32).reshape(n, 3, 3),
               o[:, o_t:o_t + 12].copy().view(np.float32).reshape(n, 3)) for f, o in out.items()}
    _check_against_reference(T, gn, what, res)


def _frame_maps(oracle, cam, depth, level):
    from oracle.oracle import OIntr
    d = oracle.bilateral_filter(depth)
    for _ in range(level):
        d = oracle.pyr_down(d)
    v = oracle.create_vmap(OIntr(cam.fx, cam.fy, cam.cx, cam.cy).level(level), d)
    return v, oracle.create_nmap(v)


def test_icp_track_against_an_exact_rerun_of_its_gauss_newton_loop(ctx, oracle_mod, small_scene):
    """The tail as the tracking kernels run it -- the real 29 sums unpacked, 19 compositions onto the device's own resultRt, the level
    schedule (10, 5, 4, 0) -- and not through the debug hook.  kt_icp_track's pose is reproduced bit for bit by the stepwise loop
    (kt_icp_step + host ABI), so the A, b of every iteration are the device's own; each is solved exactly over the rationals, turned
    into a rotation by the rational series and composed exactly.  Only the tail is under test: the final pose must sit within the float
    bar (8 x 2^-24 x the largest term) of the exact chain's, plus what the double part may have accumulated -- per iteration the forward
    bar C_FWD kappa_inf u |x|_inf of the solve, and 16 k u max(1, |t|) for the k compositions -- which is also asserted on the way, on x
    and on resultRt."""
    from fractions import Fraction as F
    from kintinuous_amd import abi
    from kintinuous_amd.abi import Intr
    from tests.conftest import random_rotation
    gn = _gn_checks()
    G = gn.G
    cam, frames, traj = small_scene
    schedule = (10, 5, 4, 0)
    t0 = np.array([3, 3, 3], np.float32)
    Rprev = random_rotation(np.random.default_rng(5), 0.02)
    cur, prev = [], []
    for l in range(4):
        vc, nc = _frame_maps(oracle_mod, cam, frames[1][0], l)
        v0, n0 = _frame_maps(oracle_mod, cam, frames[0][0], l)
        vg, ng = oracle_mod.transform_maps(v0, n0, Rprev, t0)
        cur.append((ctx.upload(vc), ctx.upload(nc)))
        prev.append((ctx.upload(vg), ctx.upload(ng)))
    dist, ang = 0.10, float(np.float32(np.sin(np.float32(20.0) * np.float32(3.14159254) / np.float32(180.0))))
    gi = Intr(cam.fx, cam.fy, cam.cx, cam.cy)
    Rc, tc, _, _ = ctx.icp_track([c[0] for c in cur], [c[1] for c in cur], [p[0] for p in prev], [p[1] for p in prev], cam.cols, cam.rows, gi, Rprev, t0,
                                 schedule, dist, ang)
    R, t = Rprev.copy(), t0.copy()
    Rprev_inv = abi.host_mat33_inverse(Rprev)
    rt = np.eye(4)
    exact = None
    slack, k = 0.0, 0           # what the double part may have accumulated on an element of resultRt
    rnd = lambda v: G.frac(G.hilo(v))
    for l in (3, 2, 1, 0):
        for _ in range(schedule[l]):
            A, b, _ = ctx.icp_step(R, t, cur[l][0], cur[l][1], Rprev_inv, t0, gi.level(l), prev[l][0], prev[l][1], cam.cols >> l, cam.rows >> l, dist, ang)
            x = abi.host_ldlt_solve6(A.astype(np.float64), b.astype(np.float64))
            rt, R, t = abi.host_pose_update(x, rt, Rprev, t0)
            k += 1
            Af, bf = G.fmat(A.astype(np.float64), 6, 6), [G.frac(float(v)) for v in b]
            l2 = G.ldlt_eigen(Af, bf)
            xe, kappa = G.solve_with_condition(Af, bf)
            assert xe is not None and not any(l2["dropped"]) and not l2["undecidable"] and xe == l2["x"]
            xnorm = float(max(abs(v) for v in xe))
            fwd = gn.C_FWD * float(kappa) * gn.U * xnorm
            assert max(abs(G.frac(float(a)) - e) for a, e in zip(x, xe)) <= fwd, (k, x, float(kappa))
            xe = [rnd(v) for v in xe]
            Re = [[rnd(v) for v in row] for row in G.rodrigues_series(xe[3:])]
            exact = G.compose([(Re, xe[:3])], exact)
            tnorm = float(np.sqrt(float(sum(exact[i][3] ** 2 for i in range(3)))))
            slack += 2 * fwd * (1 + tnorm)          # x off by fwd moves [R | t] by that much and the product by (1 + |t|) times it
            bar = slack + k * 16 * gn.U * max(1.0, tnorm)
            err = max(abs(G.frac(float(rt[i][j])) - exact[i][j]) for i in range(4) for j in range(4))
            print("iteration %d: kappa_inf %.3g, |x| %.3g, resultRt off by %.2f u (bar %.1f u)" % (k, float(kappa), xnorm, float(err) / gn.U, bar / gn.U))
            assert float(err) <= bar, (k, float(err), bar)
    assert k == 19
    # the loop above IS the device's: the same pose in every bit
    assert np.array_equal(Rc.view(np.uint32), np.asarray(R, np.float32).view(np.uint32)) and np.array_equal(tc.view(np.uint32), np.asarray(t, np.float32).view(np.uint32))
    Rp, tp = gn._mat(Rprev, 3, 3), gn._fr(t0)
    Rw, tw = G.pose_from_increment(exact, Rp, tp)
    sR, st = G.pose_term_scale(exact, Rp, tp)
    eR = max(abs(a - b) for a, b in zip(gn._fr(Rc), [v for row in Rw for v in row]))
    et = max(abs(a - b) for a, b in zip(gn._fr(tc), tw))
    print("final pose: Rcurr off by %.2f, tcurr by %.2f x 2^-24 x the largest term (bar 8); double part at most %.3g" % (
        float(eR) / gn.UF / float(sR), float(et) / gn.UF / float(st), bar))
    assert float(eR) <= 8 * gn.UF * float(sR) + 4 * bar * (1 + tnorm), (float(eR), float(sR))
    assert float(et) <= 8 * gn.UF * float(st) + 4 * bar * (1 + tnorm), (float(et), float(st))
    assert np.abs(tc - t0).max() > 1e-5        # it did track something
