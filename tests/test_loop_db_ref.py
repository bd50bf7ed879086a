"""The loop-closure candidate source without a GPU: the restatement's scores against an independent matcher, the library's
host selection (kt_host_loop_db_select) against the restatement's on hand-made score arrays, and the ten-frame scenario's recorded values."""
import numpy as np
import pytest

import loop_db_cases as dc
from kintinuous_amd import loop_db_ref as ref
from kintinuous_amd import loop_match_ref as mref


# ---- scores ------------------------------------------------------------------------------------------------------------------------
def test_scores_equal_independent_matcher():
    rng = np.random.default_rng(11)
    query = dc.random_descriptors(rng, 70)
    entries = [np.zeros((0, 8), np.uint32), dc.planted_entry(rng, query, 1), dc.planted_entry(rng, query, 2), dc.planted_entry(rng, query, 40),
               dc.planted_entry(rng, query, 150), query.copy()]
    got = ref.scores(query, entries)
    want = dc.brute_scores(query, entries)
    print("scores", got.tolist(), want.tolist())
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    assert got[0] == 0                      # an empty entry
    assert got[5] == len(query)             # every descriptor finds itself at distance 0, the rest about 128 bits off
    assert 0 < got[4] < len(query)          # the planted cases are taken on both sides of the rule
    assert ref.scores(np.zeros((0, 8), np.uint32), entries).tolist() == [0] * len(entries)   # an empty query


def test_score_planted_cases_one_by_one():
    """every planted case on its own: a query of ONE descriptor against an entry that holds just the case"""
    rng = np.random.default_rng(5)
    q = dc.random_descriptors(rng, 1)
    far = dc.random_descriptors(rng, 1)
    cases = {
        "duplicate twice (d1 = d2 = 0: 0 < 0 fails)": ([q[0], q[0]], 0),
        "duplicate once + far": ([q[0], far[0]], 1),
        "tie at d1 (5 * 10 < 4 * 10 fails)": ([dc.flip(q[0], rng, 10), dc.flip(q[0], rng, 10)], 0),
        "ratio boundary (5 * 40 == 4 * 50)": ([dc.flip(q[0], rng, 40), dc.flip(q[0], rng, 50)], 0),
        "inside the ratio (5 * 40 < 4 * 51)": ([dc.flip(q[0], rng, 40), dc.flip(q[0], rng, 51)], 1),
        "one descriptor at max_hamming (d2 = 257)": ([dc.flip(q[0], rng, 64)], 1),
        "one descriptor past max_hamming": ([dc.flip(q[0], rng, 65)], 0),
        "one descriptor, a duplicate": ([q[0]], 1),
    }
    for name, (entry, want) in cases.items():
        e = np.array(entry, np.uint32)
        assert ref.score(q, e) == want, name
        assert dc.brute_scores(q, [e])[0] == want, name


# ---- selection ---------------------------------------------------------------------------------------------------------------------
def _z(n, **at):
    s = [0] * n
    for k, v in at.items():
        s[int(k[1:])] = v
    return s


# (name, scores, previous island, parameters, expected (status, candidate, candidate_score, reference, first, last, island score))
P = dict(dislocal=2, max_gap=3)
SELECT_CASES = [
    ("empty", [], None, {}, (ref.EMPTY, -1, 0, 0, -1, -1, 0)),
    ("low reference", _z(10, e0=100, e9=39), None, P, (ref.LOW_REFERENCE, -1, 0, 39, -1, -1, 0)),
    ("reference exactly min_score", _z(10, e0=100, e9=40), (0, 0), P, (ref.DETECTED, 0, 100, 40, 0, 0, 100)),
    ("no candidate", _z(10, e0=39, e9=50), (0, 0), P, (ref.NO_CANDIDATE, -1, 0, 50, -1, -1, 0)),
    ("no previous island", _z(10, e0=100, e9=50), None, P, (ref.NOT_CONSISTENT, -1, 100, 50, 0, 0, 100)),
    ("consistency off", _z(10, e0=100, e9=50), None, dict(P, consistency=0), (ref.DETECTED, 0, 100, 50, 0, 0, 100)),
    ("two islands of equal sum: the lowest first id", _z(20, e0=60, e1=60, e8=70, e9=50, e19=50), (0, 0), P, (ref.DETECTED, 0, 60, 50, 0, 1, 120)),
    ("the later island wins when larger", _z(20, e0=60, e1=60, e8=70, e9=51, e19=50), (8, 9), P, (ref.DETECTED, 8, 70, 50, 8, 9, 121)),
    ("equal s inside an island: the lowest id", _z(20, e2=50, e3=80, e4=80, e19=50), (3, 3), P, (ref.DETECTED, 3, 80, 50, 2, 4, 210)),
    ("a gap of exactly max_gap joins", _z(20, e2=50, e5=60, e19=50), (2, 2), P, (ref.DETECTED, 5, 60, 50, 2, 5, 110)),
    ("a gap of max_gap + 1 splits", _z(20, e2=50, e6=60, e19=50), (2, 2), P, (ref.DETECTED, 6, 60, 50, 6, 6, 60)),
    ("an entry exactly at newest - dislocal", _z(10, e7=90, e9=50), (7, 7), P, (ref.DETECTED, 7, 90, 50, 7, 7, 90)),
    ("an entry above newest - dislocal", _z(10, e8=90, e9=50), (7, 7), P, (ref.NO_CANDIDATE, -1, 0, 50, -1, -1, 0)),
    ("dislocal past the oldest entry", _z(3, e0=90, e2=50), (0, 0), dict(P, dislocal=3), (ref.NO_CANDIDATE, -1, 0, 50, -1, -1, 0)),
    ("alpha exactly met (10 * 30 == 3 * 100)", _z(10, e0=30, e9=100), (0, 0), dict(P, min_score=20), (ref.DETECTED, 0, 30, 100, 0, 0, 30)),
    ("alpha missed by one", _z(10, e0=29, e9=100), (0, 0), dict(P, min_score=20), (ref.NO_CANDIDATE, -1, 0, 100, -1, -1, 0)),
    ("min_score exactly met", _z(10, e0=40, e9=41), (0, 0), P, (ref.DETECTED, 0, 40, 41, 0, 0, 40)),
    # the ranges are the islands widened by max_gap on BOTH sides: islands 2 * max_gap apart still share an id, one more does not
    ("consistency ranges touch", _z(30, e10=60, e11=60, e29=50), (2, 4), P, (ref.DETECTED, 10, 60, 50, 10, 11, 120)),
    ("consistency ranges miss by one", _z(30, e10=60, e11=60, e29=50), (2, 3), P, (ref.NOT_CONSISTENT, -1, 60, 50, 10, 11, 120)),
    ("consistency ranges touch from above", _z(30, e10=60, e11=60, e29=50), (17, 20), P, (ref.DETECTED, 10, 60, 50, 10, 11, 120)),
    ("consistency ranges miss from above", _z(30, e10=60, e11=60, e29=50), (18, 20), P, (ref.NOT_CONSISTENT, -1, 60, 50, 10, 11, 120)),
    ("max_gap 0: touching means the same id", _z(30, e10=60, e29=50), (10, 10), dict(P, max_gap=0), (ref.DETECTED, 10, 60, 50, 10, 10, 60)),
    ("max_gap 0: a neighbour misses", _z(30, e10=60, e29=50), (11, 11), dict(P, max_gap=0), (ref.NOT_CONSISTENT, -1, 60, 50, 10, 10, 60)),
]


@pytest.mark.parametrize("case", SELECT_CASES, ids=[c[0] for c in SELECT_CASES])
def test_select_restatement_by_hand(case):
    """the expected tuples are worked out by hand from the definition"""
    _, scores, prev, kw, want = case
    r = ref.select(scores, prev, ref.DetectParams(**kw))
    assert (r.status, r.candidate, r.candidate_score, r.reference_score, r.island_first, r.island_last, r.island_score) == want
    assert r.entry == len(scores) and r.n_keypoints == 0


@pytest.mark.parametrize("case", SELECT_CASES, ids=[c[0] for c in SELECT_CASES])
def test_host_select_equals_restatement(case):
    from kintinuous_amd import abi
    _, scores, prev, kw, _ = case
    got = abi.host_loop_db_select(scores, prev, abi.loop_db_detect_params(**kw))
    assert got.fields() == ref.select(scores, prev, ref.DetectParams(**kw)).fields()
    if prev is None:                        # "none" may also be spelled first < 0
        assert abi.host_loop_db_select(scores, (-1, -1), abi.loop_db_detect_params(**kw)).fields() == got.fields()


def test_host_select_random_equals_restatement():
    from kintinuous_amd import abi
    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(400):
        n = int(rng.integers(0, 40))
        scores = np.where(rng.random(n) < 0.35, rng.integers(30, 120, n), rng.integers(0, 45, n)).astype(np.int32)
        kw = dict(dislocal=int(rng.integers(0, 6)), max_gap=int(rng.integers(0, 4)), consistency=int(rng.integers(0, 2)), min_score=int(rng.integers(20, 60)))
        prev = None if rng.random() < 0.3 else tuple(sorted(int(v) for v in rng.integers(0, 40, 2)))
        want = ref.select(scores, prev, ref.DetectParams(**kw))
        assert abi.host_loop_db_select(scores, prev, abi.loop_db_detect_params(**kw)).fields() == want.fields()
        seen.add(want.status)
    assert seen == {ref.EMPTY, ref.LOW_REFERENCE, ref.NO_CANDIDATE, ref.NOT_CONSISTENT, ref.DETECTED}


def test_defaults_and_bad_parameters():
    from kintinuous_amd import abi
    p, d = abi.loop_db_detect_params(), ref.DetectParams()
    assert (p.dislocal, p.alpha_num, p.alpha_den, p.min_score, p.max_gap, p.consistency) == (20, 3, 10, 40, 3, 1)
    assert (d.dislocal, d.alpha_num, d.alpha_den, d.min_score, d.max_gap, d.consistency) == (20, 3, 10, 40, 3, 1)
    for kw in (dict(alpha_den=0), dict(dislocal=-1), dict(max_gap=-1), dict(consistency=2), dict(min_score=-1)):
        with pytest.raises(abi.KtError):
            abi.host_loop_db_select([50, 50], None, abi.loop_db_detect_params(**kw))


# ---- the scenario ------------------------------------------------------------------------------------------------------------------
def test_scenario_recorded_values():
    desc = dc.descriptors()
    assert tuple(len(d) for d in desc) == dc.KEYPOINTS
    assert tuple(ref.scores(desc[9], desc[:9]).tolist()) == dc.SCORES_9
    res = dc.restated()
    for r in res:
        print(r.entry, ref.STATUS_NAMES[r.status], r.fields())
    assert [r.entry for r in res] == list(range(10)) and tuple(r.n_keypoints for r in res) == dc.KEYPOINTS
    assert all(r.status != ref.DETECTED and r.candidate == -1 for r in res[:5])
    assert res[0].status == ref.EMPTY
    assert res[5].status == ref.NOT_CONSISTENT and (res[5].island_first, res[5].island_last) == (1, 1)
    assert [(r.status, r.candidate) for r in res[6:]] == [(ref.DETECTED, 2), (ref.DETECTED, 1), (ref.DETECTED, 1), (ref.DETECTED, 0)]
    assert (res[9].reference_score, res[9].island_first, res[9].island_last, res[9].island_score, res[9].candidate_score) == (282, 0, 2, 697, 367)


def test_database_capacity_and_reset():
    rng = np.random.default_rng(2)
    db = ref.Database(max_entries=2)
    a, b = dc.random_descriptors(rng, 5), dc.random_descriptors(rng, 7)
    assert db.add_descriptors(a) == 0 and db.detect_descriptors(b).entry == 1
    with pytest.raises(OverflowError):
        db.add_descriptors(a)
    with pytest.raises(OverflowError):
        db.detect_descriptors(a)
    assert len(db.entries) == 2
    db.reset()
    assert db.detect_descriptors(a).status == ref.EMPTY and db.prev_island is None
