"""GPU: a refused allocation in each of the seven passes over the -m mesh (kt_mesh_weld, _simplify, _normals, _components, _holes, _smooth,
_render): kt_group::grow promises that a failure leaves the group empty, the host forms that a failed call writes nothing.
kt_debug_fail_allocation refuses the k-th owner request on the host (no HIP call fails, no kernel runs in a failing state).  For every k
up to the number of requests that create plus one host-form call make: exactly one of the two reports KT_ERR_NOMEM, a failed call leaves
the caller's canaries alone, an object that exists then answers an unarmed call with the restatement's bytes, and close() gives everything
back.  One small input: mesh_holes_cases.random_case(4, 257) under a two-span table, so that every group of every pass is reached (weld
keys from a small pool at times that the gate looks at, a 16 x 12 camera in front of the patch)."""
import ctypes as C
import gc

import numpy as np
import pytest

import mesh_holes_cases as hc
from kintinuous_amd import abi, mesh_components_ref, mesh_holes_ref, mesh_normals_ref, mesh_render_ref, mesh_simplify_ref, mesh_smooth_ref, mesh_weld_ref
from mesh_weld_cases import same

pytestmark = pytest.mark.gpu

V = abi.MESH_VERTEX_DTYPE
CANARY = 0xA5


def _canary(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = CANARY
    return a


def _p(a):
    return a.ctypes.data


def _mesh():
    v, tri, _ = hc.random_case(4, 257)
    n = len(v)
    return np.ascontiguousarray(v), np.ascontiguousarray(tri), np.array([0, n // 2, n], np.uintp)


# Every pass below: (the abi class, call, want).  call(handle) -> (status, [(output array as the call left it, its bytes before the call or
# None for the canary)], the result cut to its counts, comparable to want); want: the restatement's answer.
def _weld():
    v, tri, first = _mesh()
    n, rng = len(v), np.random.default_rng(9)
    keys = rng.integers(0, 1 << 62, n // 3, dtype=np.uint64)[rng.integers(0, n // 3, n)]
    times, gap = np.array([5, 25], np.uint64), 10
    wv, wk, wt, wf = mesh_weld_ref.weld(v, keys, tri, first, times, gap)

    def call(h):
        vo, ko, t, fo, n_out = _canary(n, V), _canary(n, np.uint64), tri.copy(), _canary(3, np.uintp), C.c_size_t(0)
        s = abi.lib().kt_mesh_weld(h, _p(v), _p(keys), n, _p(t), len(tri), _p(first), _p(times), 2, gap, _p(vo), _p(ko), n, _p(fo), C.byref(n_out))
        return s, [(vo, None), (ko, None), (t, tri), (fo, None)], (vo[:n_out.value], ko[:n_out.value], t, fo.astype(np.int64))
    return abi.MeshWeld, call, (wv, wk, wt, np.asarray(wf, np.int64))


def _mesh_for_mesh(cls, name, ref, arg, extra_word, stats_cls, caps=None):
    """the four passes that give a mesh for a mesh under a span table: simplify (no word per vertex, no stats), components, holes"""
    v, tri, first = _mesh()
    n, m = len(v), len(tri)
    vcap, tcap = caps(n, m) if caps else (n, m)
    want = ref(v, tri, first, arg)
    want = (want[0], want[1], np.asarray(want[2], np.int64)) + tuple(want[3:])

    def call(h):
        vo, to, fo = _canary(vcap, V), _canary((tcap, 3), np.uint32), _canary(3, np.uintp)
        lo = _canary(n, np.uint32) if extra_word else None
        stats = stats_cls.untouched() if stats_cls else None
        n_out, m_out = C.c_size_t(0), C.c_size_t(0)
        tail = ([_p(lo)] if extra_word else []) + [_p(fo), C.byref(n_out), C.byref(m_out)] + ([C.addressof(stats)] if stats_cls else [])
        s = getattr(abi.lib(), name)(h, _p(v), n, _p(tri), m, _p(first), 2, arg, _p(vo), vcap, _p(to), tcap, *tail)
        got = (vo[:n_out.value], to[:m_out.value], fo.astype(np.int64)) + ((lo,) if extra_word else ()) + ((stats.as_tuple(),) if stats_cls else ())
        return s, [(vo, None), (to, None), (fo, None)] + ([(lo, None)] if extra_word else []), got
    return cls, call, want


def _simplify():
    return _mesh_for_mesh(abi.MeshSimplify, "kt_mesh_simplify", mesh_simplify_ref.simplify, 0.25, False, None)


def _components():
    return _mesh_for_mesh(abi.MeshComponents, "kt_mesh_components", mesh_components_ref.components, 3, True, abi.MeshComponentStats)


def _holes():
    return _mesh_for_mesh(abi.MeshHoles, "kt_mesh_holes", mesh_holes_ref.holes, 8, True, abi.MeshHoleStats, abi.MeshHoles.most)


def _normals():
    v, tri, _ = _mesh()
    n = len(v)
    wn, wz = mesh_normals_ref.normals(v, tri)

    def call(h):
        out, n_zero = _canary(n, abi.MESH_NORMAL_DTYPE), C.c_size_t(0)
        s = abi.lib().kt_mesh_normals(h, _p(v), n, _p(tri), len(tri), _p(out), C.byref(n_zero))
        return s, [(out, None)], (out, n_zero.value)
    return abi.MeshNormals, call, (np.ascontiguousarray(wn).view(abi.MESH_NORMAL_DTYPE).reshape(-1), wz)


def _smooth():
    v, tri, _ = _mesh()
    n = len(v)
    wv, ws = mesh_smooth_ref.smooth(v, tri, 2, abi.MeshSmooth.LAMBDA, abi.MeshSmooth.MU, 1)

    def call(h):
        out, stats = _canary(n, V), abi.MeshSmoothStats.untouched()
        s = abi.lib().kt_mesh_smooth(h, _p(v), n, _p(tri), len(tri), 2, abi.MeshSmooth.LAMBDA, abi.MeshSmooth.MU, 1, _p(out), C.addressof(stats))
        return s, [(out, None)], (out, stats.as_tuple())
    return abi.MeshSmooth, call, (wv, tuple(ws))


def _render():
    v, tri, _ = _mesh()
    cols, rows, intr, near = 16, 12, (8.0, 8.0, 12.0, 6.0), abi.MeshRender.NEAR
    R, t = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)   # half a metre in front of the patch in z = 0.5: it fills the image
    want = mesh_render_ref.render(v, tri, intr, cols, rows, R, t, near)
    assert want[4][0] > 0 and want[4][3] > 0
    k = abi.Intr(*intr)

    def call(h):
        planes = [_canary((rows, cols), np.uint32), _canary((rows, cols), np.uint16), _canary((rows, cols, 3), np.uint8), _canary((rows, cols, 3), np.uint8)]
        stats = abi.MeshRenderStats.untouched()
        s = abi.lib().kt_mesh_render(h, _p(v), len(v), _p(tri), len(tri), C.addressof(k), cols, rows, _p(R), _p(t), near, *[_p(a) for a in planes],
                                     C.addressof(stats))
        return s, [(a, None) for a in planes], tuple(planes) + (stats.as_tuple(),)
    return abi.MeshRender, call, tuple(want[:4]) + (tuple(want[4]),)


PASSES = {"weld": _weld, "simplify": _simplify, "normals": _normals, "components": _components, "holes": _holes, "smooth": _smooth, "render": _render}


def _equal(got, want):
    assert len(got) == len(want)
    arrays = [k for k, w in enumerate(want) if isinstance(w, np.ndarray)]
    same([got[k] for k in arrays], [want[k] for k in arrays])
    for k in set(range(len(want))) - set(arrays):          # counts and stats
        assert np.array_equal(np.asarray(got[k], np.int64), np.asarray(want[k], np.int64)), (k, got[k], want[k])


def _untouched(outs):
    for a, before in outs:
        assert (a.view(np.uint8) == CANARY).all() if before is None else np.array_equal(a, before)


@pytest.mark.parametrize("name", sorted(PASSES))
def test_every_request_refused_once(ctx, name):
    cls, call, want = PASSES[name]()

    def create_and_call():
        """-> (the object or None, [status of create, status of the call when it could be made], the call's outputs)"""
        try:
            w = cls(ctx)
        except abi.KtError as e:
            return None, [e.status], None
        s, outs, got = call(w.h)
        return w, [abi.KT_OK, s], (outs, got)

    ctx.sync()
    gc.collect()
    base = abi.live_allocations()
    w, st, (outs, got) = create_and_call()
    assert st == [abi.KT_OK, abi.KT_OK]
    _equal(got, want)
    n = sum(abi.live_allocations()) - sum(base)
    assert n >= 6, n                       # the result words, a workspace and a staging at the least
    w.close()
    assert abi.live_allocations() == base

    try:
        for k in range(1, n + 1):
            abi.fail_allocation(k)
            w, st, res = create_and_call()
            abi.fail_allocation(-1)
            assert st.count(abi.KT_ERR_NOMEM) == 1 and st.count(abi.KT_OK) == len(st) - 1, (k, st)
            if w is not None:
                _untouched(res[0])         # the call failed: nothing of the caller's is written
                s, _, got = call(w.h)      # the object is whole: groups that failed are empty and grow again
                assert s == abi.KT_OK, k
                _equal(got, want)
                w.close()
            assert abi.live_allocations() == base, k
    finally:
        abi.fail_allocation(-1)
