"""CPU.  What tests/test_gpu_loop_kernels.py expects of the RANSAC kernels and of the reducing registration pass, shown to be satisfiable
without a GPU: the independent reference (tests/tools/loop_reference.py: draws, a many-digit three-point fit, inlier counts with a derived
margin, exact sums) against the numpy restatement (kintinuous_amd/loop_match_ref.py, loop_icp_ref.py) on every case of
tests/loop_kernel_cases.py.

The restatement's sums are numpy's pairwise sums of a contiguous vector of n doubles: blocks of at most 128 elements go through 8
accumulators of at most 16 additions each, 3 levels combine the accumulators and at most 7 left-over elements follow one by one -- 26
additions deep -- and above 128 elements the vector is halved recursively, ceil(log2(n / 128)) further levels.  Its bound is therefore
(26 + max(0, ceil(log2(n / 128)))) u sum |term|, first order, against (6 + nw) u sum |term| for the kernels."""
import math

import numpy as np
import pytest

import loop_kernel_cases as K

REF = K.REF


_restated_scores = K.restated_scores


def test_draws():
    """distinct, below m, equal to the restatement's, for m = 3 .. 8 and every m of the cases, h < 4096; the scalar form agrees"""
    from kintinuous_amd import loop_match_ref as lm
    ms = sorted(set(range(3, 9)) | {len(K.ransac_case(n)["pn"]) for n in K.RANSAC_CASES if len(K.ransac_case(n)["pn"]) >= 3})
    for m in ms:
        for seed in (1, 0xFFFFFFF0, K.ransac_case("ties")["seed"]):
            tri = REF.draws(seed, 4096, m)
            assert tri.min() >= 0 and tri.max() < m
            assert (tri[:, 0] != tri[:, 1]).all() and (tri[:, 0] != tri[:, 2]).all() and (tri[:, 1] != tri[:, 2]).all()
            assert np.array_equal(tri, lm.draw_triples(seed, 4096, m))
            for h in list(range(0, 4096, 97 if m > 8 else 1)):
                assert REF.draw(seed, h, m) == tuple(tri[h])
    tri = REF.draws(1, 4096, 5)                                # for small m every index is drawn, in every position
    assert all(set(tri[:, k].tolist()) == set(range(5)) for k in range(3))


def test_fixed_point_fit_against_mpmath():
    """the fixed-point fit carries more than 60 digits (mpmath at 80 digits, 40 hypotheses of a noisy list)"""
    import mpmath
    c = K.ransac_case("m1025")
    tri = REF.draws(c["seed"], 40, len(c["pn"]))
    Fn, Fo = REF._fixed(c["pn"]), REF._fixed(c["po"])
    en, cn, n1n, n3n, _ = REF._triads(Fn[tri[:, 0]], Fn[tri[:, 1]], Fn[tri[:, 2]])
    fit = REF.fit_many(c["pn"], c["po"], tri)
    for h in range(40):
        R, t, norms = REF.fit_mpmath(c["pn"][tri[h]], c["po"][tri[h]])
        assert abs(mpmath.mpf(int(n1n[h])) / REF.ONE - norms[0]) < mpmath.mpf(10) ** -60
        assert abs(mpmath.mpf(int(n3n[h])) / REF.ONE - norms[1]) < mpmath.mpf(10) ** -60
        for a in range(3):
            assert fit["t"][h, a] == float(t[a])
            for b in range(3):
                assert fit["R"][h, a, b] == float(R[a][b])
        assert fit["n1o"][h] == float(norms[2]) and fit["n3o"][h] == float(norms[3])


@pytest.mark.parametrize("name", K.RANSAC_CASES)
def test_scores_within_reference(name):
    """the restatement's score of every hypothesis lies in the reference's [lo, hi], and at most 1 % of the hypotheses are undecided"""
    lo, hi, _ = K.ransac_bounds(name)
    got = _restated_scores(name)
    assert ((lo <= got) & (got <= hi)).all(), np.flatnonzero((got < lo) | (got > hi))[:10]
    for n in sorted(set(K.GRID_H) | {len(lo)}):
        if n <= len(lo):
            assert (hi[:n] != lo[:n]).sum() <= K.CAP * n, (n, np.flatnonzero(hi[:n] != lo[:n]))


def test_case_conditions():
    """the lists hold what they are meant to hold"""
    for name in K.RANSAC_CASES:
        c = K.ransac_case(name)
        assert c["uv"].shape == (len(c["pn"]), 4) and c["pn"].dtype == np.float32 and c["po"].dtype == np.float32
    for m in (64, 1023, 1024, 1025, 2049, 4096):
        lo, hi, _ = K.ransac_bounds(f"m{m}")
        c = K.ransac_case(f"m{m}")
        assert 2 <= (c["pn"][:, 2] <= 0).sum() <= 5                               # a handful behind the camera
        assert lo.max() >= 0.5 * m and (lo == 0).sum() < len(lo)                   # some hypothesis finds the motion
        assert np.abs(c["uv"][:, :2] - c["uv"][:, 2:]).max(axis=1).min() >= 3      # old and new pixels are apart (the new ones must not be read)
    lo, hi, _ = K.ransac_bounds("second_tile")
    assert lo.max() >= 0.5 * 1025 and np.array_equal(lo, hi)
    first = K.ransac_case("second_tile")
    sub = {k: (v[:1024] if k in ("uv", "pn", "po") else v) for k, v in first.items()}
    fit = REF.fit_many(first["pn"], first["po"], REF.draws(first["seed"], first["n_hyp"], 2049))
    lo1, hi1 = REF.inlier_bounds(fit, sub["pn"], sub["uv"][:, :2], *first["intr"], first["reproj"])
    assert hi1.max() <= 8                                                          # the first tile alone scores about 0
    lo, hi, _ = K.ransac_bounds("ties")
    assert np.array_equal(lo, hi) and lo[0] == 0 and lo[1] == 0 and lo[2] == 64 and (lo == 64).sum() >= 50 and K.expected_best(lo) == [2, 64]
    lo, hi, _ = K.ransac_bounds("collinear")
    assert not lo.any() and not hi.any()


def test_lattice_expectation():
    """the integer expectation of the lattice case equals the reference's rational count for both motions; the many-digit fit of every
    hypothesis IS its motion (R a signed permutation, t dyadic, exact roots); the pairs planted on the threshold are counted, the float32
    neighbour outside is not, the one inside is, Z = 0 and Z < 0 are not"""
    c = K.lattice_case()
    by_motion = K.lattice_scores_by_motion()
    for name, (P, t8) in K.LATTICE_MOTIONS.items():
        assert by_motion[name] == REF.exact_counts(P, [v / 8.0 for v in t8], c["pn"], c["uv"][:, :2], *c["intr"], c["reproj"])
    fit = REF.fit_many(c["pn"], c["po"], c["tri"])
    for h in range(c["n_hyp"]):
        P, t8 = K.LATTICE_MOTIONS[K._lattice_motion_of(h)]
        assert np.array_equal(fit["R"][h], np.array(P, np.float64)) and np.array_equal(fit["t"][h], np.array(t8) / 8.0)
        assert all(float(fit[k][h]) * 8 == round(float(fit[k][h]) * 8) for k in ("n1n", "n3n", "n1o", "n3o"))
    assert np.array_equal(c["tri"], REF.draws(c["seed"], c["n_hyp"], len(c["pn"]))) and len(set(c["tri"].ravel().tolist())) == 3 * c["n_hyp"]
    assert by_motion["A"] != by_motion["B"] and min(by_motion.values()) >= 3
    # one pair at a time under motion A
    P, t8 = K.LATTICE_MOTIONS["A"]
    one = lambda j: REF.exact_counts(P, [v / 8.0 for v in t8], c["pn"][j:j + 1], c["uv"][j:j + 1, :2], *c["intr"], c["reproj"])
    pl = c["planted"]
    assert [one(j) for j in pl] == [1, 1, 1, 1, 0, 1] * 2 and min(pl[6:]) >= 1024 and max(pl[:6]) < 1024
    assert [one(j) for j in c["behind"]] == [0, 0]
    x = c["pn"].astype(np.float64)
    assert (x[c["behind"][0], 2] + 0.5 == 0.0) and (x[c["behind"][1], 2] + 0.5 < 0.0)
    on = 0                                                     # how many pairs sit exactly on the threshold under A
    for j in range(len(x)):
        X, Y, Z = -x[j, 1] + 0.25, x[j, 0] - 0.5, x[j, 2] + 0.5
        if Z > 0:
            du, dv = 512.0 * X / Z + 320.0 - c["uv"][j, 0], 520.0 * Y / Z + 240.0 - c["uv"][j, 1]
            on += du * du + dv * dv == 25.0
    assert on >= 8, on


@pytest.mark.parametrize("name", list(K.ICP_CASES))
def test_icp_sums_of_the_restatement(name):
    """the restatement's correspondences equal the reference's and its pairwise sums meet the bound stated above"""
    from kintinuous_amd import loop_icp_ref as li
    src, dst, M = K.icp_case(name)
    ref = K.icp_reference(name)
    M4 = np.concatenate([M, [[0.0, 0.0, 0.0, 1.0]]])
    Sk = li.transform_points(M4, src)
    idx, d2 = li.nearest(Sk, dst)
    assert np.array_equal(idx, ref["index"])
    s, t = Sk.astype(np.float64), dst[idx].astype(np.float64)
    terms = np.concatenate([s, t, (s[:, :, None] * t[:, None, :]).reshape(-1, 9), d2.astype(np.float64)[:, None]], axis=1)
    assert np.array_equal(terms, ref["terms"])
    got = [float(np.ascontiguousarray(terms[:, k]).sum()) for k in range(16)]
    n = len(src)
    depth = 26 + max(0, math.ceil(math.log2(n / 128.0)))
    for k, (err, unit) in enumerate(K.sum_errors(got, ref)):
        assert err <= depth * unit, (k, float(err), float(unit))
    if len(dst) > 1024:
        assert ref["index"][0] == 1023                         # the duplicate across the tile boundary: the lower index
    if name.endswith("far_last"):
        assert ref["terms"][64, 15] > 100.0 * ref["terms"][:64, 15].sum()
