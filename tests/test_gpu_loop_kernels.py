"""GPU.  Two loop-closure passes at kernel level, on synthetic lists at the kernels' own edges (tests/loop_kernel_cases.py) instead of frames:
match_ransac + match_best (csrc/kt_match.hip) through kt_debug_match_ransac, and one reducing registration pass, loop_nearest<true, true> +
loop_fold (csrc/kt_loop.hip), through kt_debug_loop_pass (csrc/kt_debug.h: both hooks launch the product's kernels with the product's shapes).

RANSAC: the score of EVERY hypothesis equals the numpy restatement's and lies in the [lo, hi] of the independent reference
(tests/tools/loop_reference.py: a many-digit fit, a derived margin; tests/test_loop_kernel_reference.py caps the undecided hypotheses at 1 % per
case on the CPU); the winner is {the lowest index of the maximum, the maximum}.

Registration pass: the correspondences equal the reference's; every one of the 16 sums satisfies
        |got - exact| <= (6 + nw) u sum |term|,   u = 2^-53, nw = ceil(ns / 64)
where `exact` is the integer sum of the terms (each is a float32 value or the product of two: exact in double, so summation is the only
source of error).  Derivation, first order in u: a wave's 64 terms meet in an xor-butterfly of 6 levels, so every term passes through 6
additions, each of relative error u: the partial errs by at most 6 u sum |term of the wave|.  loop_fold adds the nw partials one after the
other starting from 0: at most nw further additions on the path of any term, nw u sum |term| in all.  Dead lanes contribute exact zeros."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import loop_kernel_cases as K

pytestmark = pytest.mark.gpu


def _run_ransac(ctx, name, n_hyp):
    from kintinuous_amd import abi
    c = K.ransac_case(name)
    return ctx.debug_match_ransac(c["uv"], c["pn"], c["po"], n_hyp, c["seed"], abi.Intr(*c["intr"]), c["reproj"])


def _check_ransac(ctx, name, n_hyp):
    c = K.ransac_case(name)
    m = len(c["pn"])
    score, best = _run_ransac(ctx, name, n_hyp)
    want = K.restated_scores(name)[:n_hyp]
    lo, hi, _ = K.ransac_bounds(name)
    lo, hi = lo[:n_hyp], hi[:n_hyp]
    print(f"{name} n_hyp={n_hyp}: m={m} max score {score.max()} best {best.tolist()} differing from the restatement {(score != want).sum()} "
          f"below lo {(score < lo).sum()} above hi {(score > hi).sum()} undecided hypotheses {(lo != hi).sum()}")
    assert np.array_equal(score, want), np.flatnonzero(score != want)[:10]
    assert ((lo <= score) & (score <= hi)).all(), np.flatnonzero((score < lo) | (score > hi))[:10]
    assert best.tolist() == K.expected_best(score) == K.expected_best(want)
    if m < 3:
        assert not score.any() and best.tolist() == [0, 0]
    return score, best


@pytest.mark.parametrize("n_hyp", K.GRID_H)
@pytest.mark.parametrize("m", K.GRID_M)
def test_ransac_scores(ctx, m, n_hyp):
    """the tile edges of the match list (1024 per LDS tile) crossed with the wave edges of the hypotheses"""
    _check_ransac(ctx, f"m{m}", n_hyp)


def test_ransac_65536_hypotheses(ctx):
    """KT_MATCH_MAX_HYP hypotheses: 1024 waves, 1024 strided steps per lane of match_best"""
    _check_ransac(ctx, "m64_h65536", 65536)


def test_ransac_second_tile(ctx):
    """every inlier at index >= 1024: a kernel that reads the first tile alone scores about 0 (test_case_conditions: at most 8)"""
    score, best = _check_ransac(ctx, "second_tile", 130)
    assert best[1] >= 512


def test_ransac_exact_lattice(ctx):
    """every operation exact: the scores are the integer arithmetic of loop_kernel_cases.lattice_scores_by_motion -- pairs exactly on
    du^2 + dv^2 == thr^2 count, the float32 neighbour outside does not, Z == 0 does not"""
    score, best = _check_ransac(ctx, "lattice", K.lattice_case()["n_hyp"])
    assert np.array_equal(score, K.lattice_expected())


def test_ransac_ties(ctx):
    """many hypotheses score m; 0 and 1 are degenerate (a repeated point), so the winner is hypothesis 2"""
    score, best = _check_ransac(ctx, "ties", 130)
    assert score[0] == 0 and score[1] == 0 and (score == 64).sum() >= 50 and best.tolist() == [2, 64]


def test_ransac_all_degenerate(ctx):
    score, best = _check_ransac(ctx, "collinear", 65)
    assert not score.any() and best.tolist() == [0, 0]


def test_ransac_hook_arguments(ctx, ktlib):
    from kintinuous_amd import abi
    c = K.ransac_case("m4")
    intr = abi.Intr(*c["intr"])
    out, best = np.zeros(4, np.int32), np.zeros(2, np.int32)
    call = lambda m, n: ktlib.kt_debug_match_ransac(ctx.h, c["uv"].ctypes.data, c["pn"].ctypes.data, c["po"].ctypes.data, m, n, 1, C.byref(intr), 2.0,
                                                    out.ctypes.data, best.ctypes.data)
    assert call(4, 4) == abi.KT_OK
    assert call(-1, 4) == 2 and call(4097, 4) == 2 and call(4, 0) == 2 and call(4, 65537) == 2


def _check_sums(name, sums, ref, nw):
    worst = Fraction(0)
    for k, (err, unit) in enumerate(K.sum_errors(sums, ref)):
        worst = max(worst, err / unit if unit else Fraction(0))
        assert err <= (6 + nw) * unit, (name, k, float(err), float(unit), nw)
    return float(worst)


@pytest.mark.parametrize("name", list(K.ICP_CASES))
def test_loop_pass(ctx, name):
    """indices, the 16 sums against the exact sums under the derived bound, and the changed flag: 1 on the first pass, 0 on an immediate
    second pass, 1 again after one entry of the last (partial) wave is altered, and after one entry of wave 0 is"""
    src, dst, M = K.icp_case(name)
    ref = K.icp_reference(name)
    ns, nw = len(src), math.ceil(len(src) / 64)
    sums, idx = ctx.debug_loop_pass(src, dst, M, np.full(ns, 0xFFFFFFFF, np.uint32))
    assert np.array_equal(idx, ref["index"]), np.flatnonzero(idx != ref["index"])[:10]
    worst = _check_sums(name, sums, ref, nw)
    print(f"{name}: ns={ns} nt={len(dst)} nw={nw} worst |got - exact| / (u sum|term|) = {worst:.3f} of {6 + nw}")
    assert sums[16] == 1.0
    sums2, idx2 = ctx.debug_loop_pass(src, dst, M, idx)
    assert sums2[16] == 0.0 and np.array_equal(idx2, ref["index"]) and sums2[:16].tobytes() == sums[:16].tobytes()
    for entry in (ns - 1, 0):
        prev = ref["index"].copy()
        prev[entry] ^= 1
        sums3, idx3 = ctx.debug_loop_pass(src, dst, M, prev)
        assert sums3[16] == 1.0, entry
        assert np.array_equal(idx3, ref["index"]) and sums3[:16].tobytes() == sums[:16].tobytes()


def test_loop_pass_hook_arguments(ctx, ktlib):
    from kintinuous_amd import abi
    src, dst, M = K.icp_case("1x1")
    M12 = np.ascontiguousarray(M.reshape(-1))
    prev, sums = np.zeros(1, np.uint32), np.zeros(17)
    call = lambda ns, nt: ktlib.kt_debug_loop_pass(ctx.h, src.ctypes.data, ns, dst.ctypes.data, nt, M12.ctypes.data, prev.ctypes.data, sums.ctypes.data)
    assert call(1, 1) == abi.KT_OK and call(0, 1) == 2 and call(1, 0) == 2
