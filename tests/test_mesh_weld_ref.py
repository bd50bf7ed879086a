"""CPU: the weld pass's restatement (kintinuous_amd/mesh_weld_ref.py) against a brute-force weld on Python dicts and lists, the edge key
of the mesh restatement, and the split-box property: two boxes that share a cell plane, welded by key, are the one-box mesh."""
import numpy as np
import pytest

import mesh_weld_cases as cases
from conftest import random_volume_state
from kintinuous_amd import mesh_ref, mesh_weld_ref


def _ref(case):
    v, k, tri, first, times, gap = case
    return mesh_weld_ref.weld(v, k, tri, first, times, gap)


@pytest.mark.parametrize("n", [n for n in cases.SIZES if n <= 4099])
def test_random_lists_against_brute_force(n):
    for seed, spans, gap in ((n, 6, 10), (n + 1, 9, 0), (n + 2, 5, cases.NO_GATE), (n + 3, 40, 30)):
        case = cases.random_case(seed, n, spans, gap)
        got, want = _ref(case), cases.brute_weld(*case)
        cases.same(got, want)
        if n >= 257 and gap:
            assert 0 < len(got[0]) < n                  # something welded, something kept
        if n >= 257 and gap == 10:
            assert len(got[0]) > len(np.unique(case[1]))    # ... and the gate cut some group


def test_chains_and_gate_edges():
    kept = []
    for case in cases.chain_cases():
        got, want = _ref(case), cases.brute_weld(*case)
        cases.same(got, want)
        kept.append(len(got[0]))
    # key 7 at vertices 0, 3, 5 (times t0, t1, t2), keys 3 and 9 twice, key 1 once; max_gap 10, so a gap of exactly 10 welds
    #            (0,10,20) (0,10,30) (0,20,30) (0,20,40) (40,20,0) (10,0,10) (0,11,1)
    assert kept[:7] == [5, 6, 7, 8, 8, 4, 6]
    assert kept[7] == 2                        # inside one span nothing is cut, even at max_gap 0
    assert kept[8:] == [3, 1, 1]               # times 0 and 2^64 - 2: cut below that gap, welded at it and without a gate


def test_empty_and_errors():
    e = np.zeros(0, mesh_ref.MESH_VERTEX_DTYPE)
    v, k, t, f = mesh_weld_ref.weld(e, [], np.zeros((0, 3), np.uint32), [0, 0, 0], [5, 6])
    assert len(v) == 0 and len(k) == 0 and len(t) == 0 and f.tolist() == [0, 0, 0]
    assert mesh_weld_ref.weld(e, [], np.zeros((0, 3), np.uint32), [0], [])[3].tolist() == [0]
    one = np.zeros(2, mesh_ref.MESH_VERTEX_DTYPE)
    for first, times in (([1, 2], [0]), ([0, 1], [0]), ([0, 2, 1, 2], [0, 1, 2]), ([0, 2], [0, 1]), ([0], [])):
        with pytest.raises(ValueError):
            mesh_weld_ref.weld(one, [1, 2], np.zeros((0, 3), np.uint32), first, times)
    with pytest.raises(ValueError):
        mesh_weld_ref.weld(one, [1, 1 << 62], np.zeros((0, 3), np.uint32), [0, 2], [0])


def _keyed(vol, col, vs, wrap, lo, hi, real, N):
    v, t, info = mesh_ref.extract_mesh(vol, col, vs, wrap, lo, hi, real, N, info=True)
    return v, t, mesh_weld_ref.edge_keys(info["owner"], info["axis"], real)


def _volumes():
    N = 32
    yield "sphere", cases.sphere_volume(N), (3.0, 3.0, 3.0), (0, 0, 0), (0, 0, 0), N
    yield "random", random_volume_state(np.random.default_rng(11), N, True), (4.5, 5.0, 6.0), (5, 31, 17), (-40, 3 * N + 5, -7), N


@pytest.mark.parametrize("name", ["sphere", "random"])
def test_split_box_welds_to_the_one_box_mesh(name):
    (vol, col), vs, wrap, real, N = next(x[1:] for x in _volumes() if x[0] == name)
    dups = {}
    for axis, cut in cases.SPLITS:
        whole, a, b = cases.split_boxes(N, axis, cut)
        one = _keyed(vol, col, vs, wrap, *whole, real, N)
        parts = [_keyed(vol, col, vs, wrap, *box, real, N) for box in (a, b)]
        for v, t, k in [one] + parts:
            assert (np.diff(k.astype(np.int64)) > 0).all()       # strictly increasing within a mesh
            g, ax = mesh_weld_ref.key_fields(k)
            assert np.array_equal(mesh_weld_ref.edge_keys(g - np.array(real), ax, real), k) and (k >> np.uint64(62) == 0).all()
        v, k, t, first, times = cases.concat(*parts)
        welded = mesh_weld_ref.weld(v, k, t, first, times)
        cases.same(welded, cases.brute_weld(v, k, t, first, times, cases.NO_GATE))
        cases.check_split(one, welded)
        dups[(axis, cut)] = len(v) - len(welded[0])
        assert welded[3].tolist() == [0, len(parts[0][0]), len(welded[0])]   # the earlier box keeps all of its vertices
        if name == "sphere":
            assert cases.closed(welded[2])
            assert cases.closed(t) == (dups[(axis, cut)] == 0)
    if name == "sphere":
        assert all(dups[(axis, 15)] > 0 and dups[(axis, 1)] == 0 and dups[(axis, 30)] == 0 for axis in range(3)), dups
    else:
        assert all(d > 0 for d in dups.values()), dups
