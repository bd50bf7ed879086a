"""The numpy restatement of the pose-graph stage (kintinuous_amd/pose_graph_ref.py) against independent references; no GPU.

  - an independent optimiser in the ABSOLUTE parametrisation (6 unknowns per node, node 0 left out, scipy rotation vectors,
    scipy.optimize.least_squares with all three tolerances at their smallest) from the same start: pose entries and chi2;
  - the same cost's stationarity at the restatement's result, for every case (an extra: it also reaches the 4097-node cases);
  - two results that need no optimiser: no loops -> the chain's composition; exact measurements -> the ground truth;
  - the measurement function against mpmath at 50 digits, and the library's against the restatement's;
  - the derivative blocks Jr and A_lk against central differences of the residual in mpmath.

THE BOUND.  G = the largest pose-entry difference between the restatement and the independent optimiser, measured per case (both are
float64 minimisers of one cost stopped at different points, so G measures the conditioning of the cases):
    n2_neighbours 2.1e-13, n3_same_pair_twice 6.8e-11, n63_full 1.6e-11, n64_a_below_b 2.1e-11, n65_spans 1.8e-12,
    n65_contradiction 7.8e-11, n257_two 7.3e-11, n257_l64 5.3e-10, n1025_l7 6.4e-11 (8 s, the slowest).
The independent optimiser gets its sparse finite-difference Jacobian and solves its trust-region steps by LSMR with that solver's own
tolerances at rounding level too; every case with N <= 1025 runs in the suite.  BOUND = 10 G = 5.3e-9 (floor 1e-9), in
tests/pose_graph_cases.py, for pose entries and (relative above 1) for chi2; tests/test_gpu_pose_graph.py holds the device to it as well.

ABOVE 65536 NODES the carry scan gives every lane a serial run of per = ceil(ceil(N / 256) / 256) >= 2 block totals; neither optimiser above
gets there, so the large cases (pc.LARGE, not in pc.NAMES) have references of their own: the chain-only ones a serial left-to-right product
in np.longdouble at EVERY node, the one with loops the ground truth under exact measurements.  E = the largest pose-entry difference
between compose() and the long-double product, measured per case:
    n65536_chain (per 1) 9.0e-14, n65537_chain (per 2) 1.0e-13, n131073_chain (per 3) 1.3e-13; chi2 of all three exactly 0.0.
Asserted: max(10 E, 1e-12), i.e. 1e-12, the floor being test_no_loops_gives_the_composition's bound.  n65537_l7: chi2 551.756 ->
0.166328 in 4 steps, max |delta| 6.5e-3, 1.9e-6, 4.8e-8, 4.2e-10 (none within a factor of two of 1e-9); exact measurements: the truth within
8.2e-13 after 1 step.  n65_step_limit (pc.STEP_LIMIT): 20 steps, KT_POSE_GRAPH_MAX_STEPS, chi2 16138.9 -> 5752.81, max |delta| 0.97 ... 6.2e-5.
"""
import functools

import mpmath as mp
import numpy as np
import pytest
from scipy.optimize import least_squares
from scipy.sparse import csr_matrix
from scipy.sparse.linalg import spsolve
from scipy.spatial.transform import Rotation

import pose_graph_cases as pc
from kintinuous_amd import pose_graph_ref as ref

BOUND, chi2_bound = pc.BOUND, pc.chi2_bound
IN_SUITE = [n for n in pc.INDEPENDENT if len(pc.case(n)["loop_a"])]
WITH_LOOPS = [n for n in pc.NAMES if len(pc.case(n)["loop_a"])]


# ---- the independent cost: absolute poses, scipy rotation vectors ----------------------------------------------------------------------
class Independent:
    def __init__(self, c):
        self.N = N = c["N"]
        self.ei = np.concatenate([np.arange(0, N - 1), np.minimum(c["loop_a"], c["loop_b"])]).astype(int)
        self.ej = np.concatenate([np.arange(1, N), np.maximum(c["loop_a"], c["loop_b"])]).astype(int)
        Z = np.concatenate([c["chain_Z"], np.array([z if a < b else pc.inv(z) for a, b, z in zip(c["loop_a"], c["loop_b"], c["loop_Z"])]).reshape(-1, 4, 4)])
        self.ZRi = np.swapaxes(Z[:, :3, :3], 1, 2)
        self.Zti = -np.einsum("eij,ej->ei", self.ZRi, Z[:, :3, 3])
        self.R0, self.t0 = c["T0"][:3, :3], c["T0"][:3, 3]

    def unpack(self, x):
        x = x.reshape(self.N - 1, 6)
        return np.concatenate([self.R0[None], Rotation.from_rotvec(x[:, 3:]).as_matrix()]), np.concatenate([self.t0[None], x[:, :3]])

    def pack(self, poses):
        return np.concatenate([poses[1:, :3, 3], Rotation.from_matrix(poses[1:, :3, :3]).as_rotvec()], 1).ravel()

    def poses(self, x):
        R, t = self.unpack(x)
        P = np.tile(np.eye(4), (self.N, 1, 1))
        P[:, :3, :3], P[:, :3, 3] = R, t
        return P

    def fun(self, x):
        R, t = self.unpack(x)
        Rij = np.einsum("eki,ekj->eij", R[self.ei], R[self.ej])
        tij = np.einsum("eki,ek->ei", R[self.ei], t[self.ej] - t[self.ei])
        RE = np.einsum("eij,ejk->eik", self.ZRi, Rij)
        tE = np.einsum("eij,ej->ei", self.ZRi, tij) + self.Zti
        return np.concatenate([tE, Rotation.from_matrix(RE).as_rotvec()], 1).ravel()

    def jacobian(self, x, h=1e-6):
        """sparse central differences: nodes that share no edge are perturbed together"""
        N, E = self.N, len(self.ei)
        adj = [set() for _ in range(N)]
        for a, b in zip(self.ei, self.ej):
            adj[a].add(b); adj[b].add(a)
        colour = -np.ones(N, dtype=int)
        for n in range(1, N):
            used = {colour[m] for m in adj[n]} | {colour[k] for m in adj[n] for k in adj[m] if k != n}
            colour[n] = next(c for c in range(N) if c not in used)
        rows, cols, vals = [], [], []
        for col in range(colour.max() + 1):
            nodes = np.nonzero(colour == col)[0]
            for comp in range(6):
                d = np.zeros((N - 1, 6))
                d[nodes - 1, comp] = h
                diff = ((self.fun(x + d.ravel()) - self.fun(x - d.ravel())) / (2 * h)).reshape(E, 6)
                for n in nodes:
                    for e in np.nonzero((self.ei == n) | (self.ej == n))[0]:
                        rows.extend(range(6 * e, 6 * e + 6)); cols.extend([6 * (n - 1) + comp] * 6); vals.extend(diff[e])
        return csr_matrix((vals, (rows, cols)), shape=(6 * E, 6 * (N - 1)))


def independent_optimum(c):
    ind = Independent(c)
    start = ref.optimise(c["T0"], c["chain_Z"])[0]                       # the composition of the chain
    eps = np.finfo(np.float64).eps
    # the Jacobian is sparse (central differences, nodes that share no edge perturbed together), so the trust-region steps go through LSMR;
    # its own tolerances are set to rounding as well, or every step would be solved to 1e-6 only
    res = least_squares(ind.fun, ind.pack(start), jac=ind.jacobian, tr_solver="lsmr", tr_options={"atol": 1e-15, "btol": 1e-15, "maxiter": 20000},
                        ftol=eps, xtol=eps, gtol=eps, method="trf")
    return ind.poses(res.x), 1000.0 * 2.0 * res.cost


@pytest.mark.parametrize("name", IN_SUITE)
def test_against_independent_optimiser(name):
    c = pc.case(name)
    poses, chi2_start, chi2_end, steps, status, deltas = pc.restated(name)
    want, want_chi2 = independent_optimum(c)
    G = np.abs(poses - want).max()
    print(name, "G %.3e" % G, "chi2", chi2_end, want_chi2, "steps", steps, "last delta %.2e" % deltas[-1])
    assert status == ref.CONVERGED and 1 <= steps < ref.MAX_STEPS_N
    assert G <= BOUND
    assert abs(chi2_end - want_chi2) <= chi2_bound(want_chi2)
    assert chi2_end <= chi2_start


@pytest.mark.parametrize("name", WITH_LOOPS)
def test_stationary_in_the_absolute_parametrisation(name):
    """the Gauss-Newton step of the INDEPENDENT cost at the restatement's result: how far that cost's minimiser is from it"""
    c = pc.case(name)
    poses, _, chi2_end, steps, status, _ = pc.restated(name)
    ind = Independent(c)
    x = ind.pack(poses)
    r = ind.fun(x)
    J = ind.jacobian(x)
    dx = spsolve((J.T @ J).tocsc(), -(J.T @ r))
    print(name, "chi2 %.6g" % chi2_end, "independent chi2 %.6g" % (1000.0 * r @ r), "Newton step %.3e" % np.abs(dx).max(), "steps", steps)
    assert status == ref.CONVERGED
    assert abs(1000.0 * r @ r - chi2_end) <= 1e-9 * max(1.0, chi2_end)      # the same cost, evaluated by other code
    assert np.abs(dx).max() <= BOUND


def test_contradiction_is_rejected_by_the_threshold():
    _, chi2_start, chi2_end, _, status, _ = pc.restated(pc.CONTRADICTION)
    assert status == ref.CONVERGED and chi2_end >= 10.0
    for name in WITH_LOOPS:
        if name not in (pc.CONTRADICTION, "n257_l64"):                      # (64 random loops of 2 degrees / 2 cm over 257 poses do not agree to chi2 < 10)
            assert pc.restated(name)[2] < 10.0, name


def test_few_cases_stop_near_the_bound():
    """the device may take one step more or fewer only where the restatement's last max |delta| lies within a factor of two of 1e-9"""
    close = [n for n in WITH_LOOPS if 0.5e-9 <= pc.restated(n)[5][-1] <= 2e-9]
    print(close)
    assert len(close) * 10 <= len(pc.NAMES)


@pytest.mark.parametrize("name", [n for n in pc.NAMES if not len(pc.case(n)["loop_a"])])
def test_no_loops_gives_the_composition(name):
    c = pc.case(name)
    poses, chi2_start, chi2_end, steps, status, deltas = pc.restated(name)
    want = [c["T0"]]
    for Z in c["chain_Z"]:
        want.append(want[-1] @ Z)
    assert np.abs(poses - np.array(want)).max() <= 1e-12                    # 256 products of entries below 3, rounding 1e-16 each
    assert (steps, status, deltas) == (0, ref.CONVERGED, []) and chi2_start == chi2_end and 0.0 <= chi2_end < 1e-20


@pytest.mark.parametrize("name", ["n2_neighbours", "n3_same_pair_twice", "n65_spans", "n257_two", "n1025_l7"])
def test_exact_measurements_give_the_truth(name):
    c = pc.noise_free(name)
    poses, chi2_start, chi2_end, steps, status, _ = ref.optimise(c["T0"], c["chain_Z"], c["loop_a"], c["loop_b"], c["loop_Z"])
    print(name, np.abs(poses - c["truth"]).max(), chi2_start, chi2_end, steps)
    assert status == ref.CONVERGED and steps <= 2
    assert np.abs(poses - c["truth"]).max() <= 1e-11                        # 1024 products, rounding 1e-16 each, entries below 3
    assert chi2_end < 1e-18


# ---- above 65536 nodes (the carry scan's serial runs) and at the step limit: pc.LARGE and pc.STEP_LIMIT ---------------------------------
@functools.lru_cache(maxsize=None)
def _serial_long_double(name):
    """T_0 Z_1 ... Z_k for every k, left to right in np.longdouble (64 bits of mantissa): no scan tree, no blocks"""
    c = pc.case(name)
    Z = c["chain_Z"].astype(np.longdouble)
    want = np.empty((c["N"], 4, 4), dtype=np.longdouble)
    want[0] = acc = c["T0"].astype(np.longdouble)
    for k in range(c["N"] - 1):
        want[k + 1] = acc = acc @ Z[k]
    return want


# E per case, measured (see the module docstring); what is asserted is 10 E with the floor of test_no_loops_gives_the_composition
E_MEASURED = {"n65536_chain": 9.1e-14, "n65537_chain": 1.1e-13, "n131073_chain": 1.3e-13}
assert sorted(E_MEASURED) == sorted(pc.LARGE_CHAINS)


@pytest.mark.parametrize("name", pc.LARGE_CHAINS)
def test_large_chain_against_a_serial_long_double_product(name):
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("np.longdouble has %d mantissa bits here, no more than a double's: it cannot referee a double product" % np.finfo(np.longdouble).nmant)
    poses = pc.restated(name)[0]
    diff = np.abs(poses - _serial_long_double(name)).reshape(len(poses), -1).max(1)
    nb = -(-len(poses) // ref.BLOCK)
    print(name, "E %.3e" % diff.max(), "at node", int(diff.argmax()), "nb", nb, "per", -(-nb // ref.BLOCK))
    assert float(diff.max()) <= max(10 * E_MEASURED[name], 1e-12)


@pytest.mark.parametrize("name", pc.LARGE_CHAINS)
def test_large_chain_result(name):
    c = pc.case(name)
    poses, chi2_start, chi2_end, steps, status, deltas = pc.restated(name)
    print(name, "chi2", chi2_end)
    assert (steps, status, deltas) == (0, ref.CONVERGED, []) and chi2_start == chi2_end
    assert 0.0 <= chi2_end < 1e-20 * c["N"] / 257                           # test_no_loops_gives_the_composition's bound per node; measured: 0.0
    assert np.array_equal(poses[0], c["T0"]) and (poses[:, 3] == [0.0, 0.0, 0.0, 1.0]).all()


def test_large_generator_draws_the_same_curve():
    """the vectorised truth is the loop's truth up to the rounding of a cross product and a norm"""
    assert np.abs(pc.truth_large(1025) - pc.truth(1025)).max() <= 4 * np.finfo(np.float64).eps * 2.0
    c = pc.case(pc.LARGE_LOOPS)
    assert c["chain_Z"].shape == (65536, 4, 4) and len(c["loop_a"]) == 7
    R = c["chain_Z"][:, :3, :3]
    assert np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() < 1e-14 and (c["chain_Z"][:, 3] == [0.0, 0.0, 0.0, 1.0]).all()
    assert not set(pc.LARGE) & set(pc.NAMES) and pc.STEP_LIMIT not in pc.NAMES


def test_large_loops_result_and_seed_rule():
    """n65537_l7 converges, and NO step's max |delta| lies within a factor of two of the stopping bound: the device, whose deltas differ from
    these in the last digits, takes the same steps.  Measured: chi2 551.756 -> 0.166328, deltas 6.5e-3, 1.9e-6, 4.8e-8, 4.2e-10"""
    _, chi2_start, chi2_end, steps, status, deltas = pc.restated(pc.LARGE_LOOPS)
    print(pc.LARGE_LOOPS, "chi2", chi2_start, chi2_end, "steps", steps, "deltas", deltas)
    assert status == ref.CONVERGED and steps == len(deltas) and chi2_end <= chi2_start
    assert not [d for d in deltas if 0.5e-9 <= d <= 2e-9]


def test_large_loops_exact_measurements_give_the_truth():
    """the anchor of the large case that does not pass through the restatement's optimum"""
    c = pc.noise_free(pc.LARGE_LOOPS)
    poses, chi2_start, chi2_end, steps, status, _ = ref.optimise(c["T0"], c["chain_Z"], c["loop_a"], c["loop_b"], c["loop_Z"])
    print(pc.LARGE_LOOPS, np.abs(poses - c["truth"]).max(), chi2_start, chi2_end, steps)
    assert status == ref.CONVERGED and steps <= 2
    # 65536 products, each adding at most 3 roundings of 1.1e-16 on entries below 4.3: 9e-11 at worst (measured 8.2e-13)
    assert np.abs(poses - c["truth"]).max() <= pc.EXACT_BOUND_LARGE


def test_step_limit_is_reached():
    """n65_step_limit: 20 steps, not converged, and nowhere near converging by chance -- the iteration contracts at a steady rate.
    Measured: chi2 16138.9 -> 5752.81, max |delta| 0.97, 0.118, 0.075, ... 9.6e-5, 6.2e-5"""
    _, chi2_start, chi2_end, steps, status, deltas = pc.restated(pc.STEP_LIMIT)
    print(pc.STEP_LIMIT, "chi2", chi2_start, chi2_end, "deltas", deltas)
    assert (steps, status, len(deltas)) == (ref.MAX_STEPS_N, ref.MAX_STEPS, 20) and ref.MAX_STEPS_N == 20
    assert chi2_end < chi2_start
    assert min(deltas) > 1e-6
    assert all(deltas[k] < deltas[k - 1] for k in range(2, 20))             # falling from the third step on


# ---- mpmath ------------------------------------------------------------------------------------------------------------------------------
mp.mp.dps = 50


def _mp(M):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(M)])


def _mp_quat_rotation(R):
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t >= R[0, 0] and t >= R[1, 1] and t >= R[2, 2]:
        q = [1 + t, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]
    elif R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        q = [R[2, 1] - R[1, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]]
    elif R[1, 1] >= R[2, 2]:
        q = [R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1 - R[0, 0] + R[1, 1] - R[2, 2], R[1, 2] + R[2, 1]]
    else:
        q = [R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1 - R[0, 0] - R[1, 1] + R[2, 2]]
    n = mp.sqrt(sum(v * v for v in q))
    w, x, y, z = [v / n for v in q]
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _mp_measurement(prev, curr):
    P, Cm = _mp(prev), _mp(curr)
    Rp, Rc = _mp_quat_rotation(P[:3, :3]), _mp_quat_rotation(Cm[:3, :3])
    R = Rp.T * Rc
    t = Rp.T * (Cm[:3, 3] - P[:3, 3])
    return np.array([[float(R[i, j]) for j in range(3)] + [float(t[i])] for i in range(3)] + [[0.0, 0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def _pose_pairs():
    rng = np.random.default_rng(5)
    pairs = []
    for k in range(200):
        P = []
        for _ in range(2):
            T = pc.exp(rng.uniform(-3, 3, 3), Rotation.random(random_state=rng).as_rotvec())
            if k % 2:
                T[:3, :3] += rng.uniform(-1e-6, 1e-6, (3, 3))               # a float pose that drifted off orthonormal
            P.append(T.astype(np.float32))
        pairs.append(tuple(P))
    return pairs


def test_measurement_against_mpmath():
    worst = 0.0
    for prev, curr in _pose_pairs():
        Z = ref.measurement(prev, curr)
        worst = max(worst, np.abs(Z - _mp_measurement(prev, curr)).max())
        assert abs(np.linalg.det(Z[:3, :3]) - 1.0) < 1e-14 and np.abs(Z[:3, :3] @ Z[:3, :3].T - np.eye(3)).max() < 1e-14
    print("worst entry error", worst)
    assert worst <= 64 * np.finfo(np.float64).eps * 8.0                      # a few dozen roundings on entries below 8


def test_library_measurement_equals_restatement():
    from kintinuous_amd import abi, build
    build.build()
    for prev, curr in _pose_pairs():
        assert abi.host_pose_graph_measurement(prev, curr).tobytes() == ref.measurement(prev, curr).tobytes()


def _mp_hat(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _mp_exp(xi):
    w = xi[3:]
    th = mp.sqrt(sum(v * v for v in w))
    K = _mp_hat(w)
    R = mp.eye(3) + (mp.sin(th) / th) * K + ((1 - mp.cos(th)) / th ** 2) * K * K if th else mp.eye(3)
    T = mp.eye(4)
    T[:3, :3] = R
    for i in range(3):
        T[i, 3] = xi[i]
    return T


def _mp_residual(E):
    a = [(E[2, 1] - E[1, 2]) / 2, (E[0, 2] - E[2, 0]) / 2, (E[1, 0] - E[0, 1]) / 2]
    s = mp.sqrt(sum(v * v for v in a))
    th = mp.atan2(s, (E[0, 0] + E[1, 1] + E[2, 2] - 1) / 2)
    f = th / s if s else mp.mpf(1)
    return [E[0, 3], E[1, 3], E[2, 3]] + [v * f for v in a]


def _mp_inv(T):
    out = mp.eye(4)
    out[:3, :3] = T[:3, :3].T
    t = -(T[:3, :3].T * T[:3, 3])
    for i in range(3):
        out[i, 3] = t[i]
    return out


def _central(f):
    """d f(xi) / d xi at 0 by central differences at h = 1e-20 in 50 digits: exact to 1e-30"""
    h = mp.mpf(10) ** -20
    J = np.zeros((6, 6))
    for c in range(6):
        xi = [mp.mpf(0)] * 6
        xi[c] = h
        plus = f(xi)
        xi[c] = -h
        minus = f(xi)
        J[:, c] = [float((p - m) / (2 * h)) for p, m in zip(plus, minus)]
    return J


def test_derivative_blocks_against_central_differences():
    rng = np.random.default_rng(9)
    worst = 0.0
    for angle in (0.0, 1e-9, 1e-5, 5e-3, 0.02, 0.3, 2.0):                  # across the series' and the closed forms' ranges
        axis = rng.standard_normal(3)
        E = pc.exp(rng.uniform(-0.3, 0.3, 3), axis / np.linalg.norm(axis) * angle)
        r = ref.residual(E[:3, :3], E[:3, 3])
        Jr = ref.jr(E[:3, :3], r[3:])
        Em = _mp(E)
        worst = max(worst, np.abs(Jr - _central(lambda xi: _mp_residual(Em * _mp_exp(xi)))).max())
        # A_lk = Jr(E_l) Ad(T_j^-1 T_k) = B_l Ad(T_k): a loop (i, j, Z) with E_l = E, perturbed at a node k inside its span
        Ti, Tk, Tj = (pc.exp(rng.uniform(-3, 3, 3), Rotation.random(random_state=rng).as_rotvec()) for _ in range(3))
        Z = pc.inv(Ti) @ Tj @ pc.inv(E)
        jR, jt = ref.se3_inv(Tj[:3, :3], Tj[:3, 3])
        El_R, El_t = ref.se3_mul(*ref.se3_inv(Z[:3, :3], Z[:3, 3]), *ref.se3_mul(*ref.se3_inv(Ti[:3, :3], Ti[:3, 3]), Tj[:3, :3], Tj[:3, 3]))
        rl = ref.residual(El_R, El_t)
        A = ref.mm(ref.mm(ref.jr(El_R, rl[3:]), ref.adjoint(jR, jt)), ref.adjoint(Tk[:3, :3], Tk[:3, 3]))
        Zi, Tii, Tkm, Pkj = _mp_inv(_mp(Z)), _mp_inv(_mp(Ti)), _mp(Tk), _mp_inv(_mp(Tk)) * _mp(Tj)
        worst = max(worst, np.abs(A - _central(lambda xi: _mp_residual(Zi * Tii * Tkm * _mp_exp(xi) * Pkj))).max())
    print("worst derivative error", worst)
    # Jr's second-order coefficient is a difference of two terms of size 1 / theta^2 above theta = 1e-2: 1e-16 * 1e4 relative; the
    # adjoints carry levers of up to 6 m twice
    assert worst <= 1e-9
