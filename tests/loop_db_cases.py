"""Shared by tests/test_loop_db_ref.py (CPU) and tests/test_gpu_loop_db.py: the ten-frame scenario of the loop-closure candidate source
and the descriptor sets of its score tests.

The scenario walks loop_match_cases' textured room at 160x120: frame 0 is pose A, frames 1 - 8 turn away to the side wall and back
(yaw 20, 40, 60, 80, 60, 40, 20, 8 degrees about y, 0.5 degrees about x, a few centimetres of travel), frame 9 is pose B -- a few degrees
from frame 0, the loop to close."""
import functools

import numpy as np

import loop_icp_cases as lc
import loop_match_cases as mc

COLS, ROWS = 160, 120
YAWS = (20, 40, 60, 80, 60, 40, 20, 8)
# what the restatement gives (computed on the CPU, tests/test_loop_db_ref.py asserts them)
KEYPOINTS = (455, 434, 422, 262, 133, 251, 420, 475, 502, 461)
SCORES_9 = (367, 216, 114, 4, 4, 6, 78, 199, 282)
DETECT = dict(dislocal=3, consistency=1)


def poses():
    out = [lc.POSE_A]
    for k, yaw in enumerate(YAWS):
        out.append(lc._pose(lc._rot([0, 1, 0], np.radians(float(yaw))) @ lc._rot([1, 0, 0], np.radians(0.5)), np.array([0.025 * k, 0.0, -0.015 * k])))
    out.append(lc.POSE_B)
    return out


@functools.lru_cache(maxsize=None)
def frames():
    """[(depth uint16 [ROWS, COLS], rgb24 [ROWS, COLS, 3])] of the ten frames"""
    from kintinuous_amd import synth
    cam = mc._camera(COLS, ROWS)
    out = []
    for T in poses():
        depth, _ = synth.render(synth.Scene("room"), cam, T[:3, :3], T[:3, 3])
        out.append((depth, mc.texture(depth, cam, T)))
    return out


def camera():
    return mc._camera(COLS, ROWS)


@functools.lru_cache(maxsize=None)
def descriptors():
    """the restatement's descriptors of the ten frames, default match parameters"""
    from kintinuous_amd import loop_match_ref as mref
    return [mref.frame_keypoints(rgb, depth, mref.Params())[2] for depth, rgb in frames()]


@functools.lru_cache(maxsize=None)
def restated():
    """the restatement's ten results (loop_db_ref.Result) with DETECT"""
    from kintinuous_amd import loop_db_ref as ref
    db = ref.Database(max_entries=12)
    prm = ref.DetectParams(**DETECT)
    return [db.detect_descriptors(d, prm) for d in descriptors()]


def random_descriptors(rng, n):
    return rng.integers(0, 2 ** 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)


def flip(desc, rng, k):
    """a copy of one descriptor with k distinct bits flipped"""
    out = np.array(desc, np.uint32).copy()
    for b in rng.choice(256, size=k, replace=False):
        out[b // 32] ^= np.uint32(1) << np.uint32(b % 32)
    return out


def planted_entry(rng, query, n, max_hamming=64, base=None):
    """n descriptors (n >= 1) built around a query set so that every branch of the rule is taken: random ones (far from everything), exact
    duplicates of query descriptors (twice: d1 = d2 = 0), a tie at d1 (two descriptors at the same distance), pairs on both sides of the
    4 / 5 ratio boundary (d1 = 40, d2 = 50: rejected, 5 * 40 = 4 * 50; d2 = 51: accepted) and one at max_hamming and one past it.
    base: the n descriptors to plant into (default: random ones)"""
    e = random_descriptors(rng, n) if base is None else np.array(base, np.uint32).copy()
    nq = len(query)
    if nq == 0:
        return e
    slots = iter(rng.permutation(n))

    def put(d):
        j = next(slots, None)
        if j is not None:
            e[j] = d

    q = iter(rng.permutation(nq))
    i = next(q, None)
    if i is not None:                       # an exact duplicate, twice
        put(query[i]); put(query[i])
    i = next(q, None)
    if i is not None:                       # a tie at d1
        put(flip(query[i], rng, 10)); put(flip(query[i], rng, 10))
    i = next(q, None)
    if i is not None:                       # on the ratio boundary: rejected
        put(flip(query[i], rng, 40)); put(flip(query[i], rng, 50))
    i = next(q, None)
    if i is not None:                       # just inside it: accepted
        put(flip(query[i], rng, 40)); put(flip(query[i], rng, 51))
    i = next(q, None)
    if i is not None:                       # at max_hamming (accepted: the second neighbour is a random descriptor, about 128 bits off)
        put(flip(query[i], rng, max_hamming))
    i = next(q, None)
    if i is not None:                       # one past it
        put(flip(query[i], rng, max_hamming + 1))
    return e


def brute_scores(query, entries, max_hamming=64, ratio_num=4, ratio_den=5):
    """counts from loop_match_cases.brute_match, the independent matcher"""
    out = []
    for e in entries:
        if len(query) == 0 or len(e) == 0:
            out.append(0)
            continue
        idx, _, _ = mc.brute_match(query, e, max_hamming, ratio_num, ratio_den)
        out.append(int((idx >= 0).sum()))
    return np.array(out, np.int32)
