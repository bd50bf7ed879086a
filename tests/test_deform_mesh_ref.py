"""CPU.  deform_ref.apply_mesh, the restatement of kt_deform_apply_mesh: it holds no arithmetic of its own, so on the meshes
of tests/deform_mesh_cases.py its positions are, bit for bit, those deform_ref.apply gives the same positions as 48-byte points with the
spans' times expanded to one per point; rgb is copied; empty spans and an empty mesh are accepted.  And the `mesh` lines that the driver's
-m -df run adds to <prefix>.deform go through the tests' parser and back."""
import numpy as np
import pytest

import deform_cases as dc
import deform_mesh_cases as mc

# the 257-node graph's restated state takes the restatement's dense optimise: the GPU module shares it with tests/test_gpu_deform.py
CPU_NAMES = [n for n in mc.NAMES if not n.startswith("m257")]


@pytest.mark.parametrize("name", CPU_NAMES)
def test_apply_mesh_is_apply_on_points(name):
    from kintinuous_amd import deform_ref as ref
    c = mc.case(name)
    g, x = dc.graph(c["graph"]), dc.restated(c["graph"])[0]
    got = mc.restated(name)
    want = ref.apply(g, x, mc.as_points(c["vertices"]), mc.expanded_times(c))
    assert got.dtype == c["vertices"].dtype and len(got) == len(c["vertices"]) > 0
    assert got["xyz"].tobytes() == want["xyz"].tobytes()
    assert got["rgb"].tobytes() == c["vertices"]["rgb"].tobytes()
    assert np.abs(got["xyz"] - c["vertices"]["xyz"]).max() > 1e-3          # the state is not the identity: something moved
    assert np.isfinite(got["xyz"]).all()


def test_cases_hold_the_edges():
    """the tables are what the module's docstring says: sizes around the 256 lanes, empty spans at both ends and inside, every time edge"""
    c = mc.case("m257_n4099_c300-mixed")
    sizes = np.diff(c["span_first"].astype(np.int64)).tolist()
    assert sizes == mc.MIXED_SIZES and {0, 1, 255, 256, 257} == set(sizes) and sizes[0] == sizes[-1] == sizes[5] == 0
    nt = dc.case("m257_n4099_c300")["node_time"]
    found = [mc.nearest_node(nt, t) for t, s in zip(c["span_time"], sizes) if s]
    assert found == [0, 256, 128, 128, 18, 19, 20, 238, 255]
    assert int(c["span_time"][2]) < int(nt[0]) and int(c["span_time"][3]) > int(nt[-1])
    v = c["vertices"]
    for e in mc.RGB_EDGES:
        assert (v["rgb"] == e).any()
    assert (v["xyz"][int(c["span_first"][3])] == dc.case("m257_n4099_c300")["node_pos"][256]).all()
    o = mc.case("octa-mixed")
    lo = int(o["span_first"][3])
    d = np.linalg.norm(dc.case("octa")["node_pos"][:5].astype(np.float64) - o["vertices"]["xyz"][lo + 1].astype(np.float64), axis=1)
    assert (d == 1.0).all()
    assert np.diff(mc.case("m5_n1_c3-one4099")["span_first"].astype(np.int64)).tolist() == [4099]


def test_empty_spans_and_empty_mesh():
    from kintinuous_amd import abi, deform_ref as ref
    g, x = dc.graph("m20_n64_c7"), dc.restated("m20_n64_c7")[0]
    none = np.zeros(0, abi.MESH_VERTEX_DTYPE)
    assert len(ref.apply_mesh(g, x, none, [0], [])) == 0                            # no span at all
    assert len(ref.apply_mesh(g, x, none, [0, 0, 0], [dc.T0, dc.T0 + 7])) == 0      # spans, all empty
    # a 65-node graph, where the window depends on the time, with a state of its own: nothing here needs an optimum
    g, c = dc.graph("m65_n63_c300"), mc.case("m20_n64_c7-mixed")
    x = ref.identity(g.M) + 0.01 * np.random.default_rng(5).standard_normal((g.M, 12))
    v = c["vertices"][:5]
    t = [dc.T0 + 3 * dc.DT, dc.T0 + 60 * dc.DT]
    a = ref.apply_mesh(g, x, v, [0, 2, 5], t)
    b = ref.apply_mesh(g, x, v, [0, 0, 2, 2, 2, 5, 5], [1, t[0], 2, 3, t[1], 4])     # empty spans change nothing
    assert a.tobytes() == b.tobytes()
    assert a["xyz"].tobytes() != ref.apply_mesh(g, x, v, [0, 2, 5], t[::-1])["xyz"].tobytes()   # the span's time is what is used
    for bad in ([1, 5], [0, 3, 2, 5], [0, 4]):                                    # not from 0, decreasing, not to n
        with pytest.raises(AssertionError):
            ref.apply_mesh(g, x, v, bad, [dc.T0] * (len(bad) - 1))
    assert v.tobytes() == c["vertices"][:5].tobytes()                             # the input is left alone


def test_mesh_lines_round_trip():
    spans = [(1000, 0), (4000, 137), (18446744073709551615, 4099)]
    text = "\n".join(["pose 1000 0x1p+0 0x1.8p+1 -0x1p-3 0x0p+0 0x1p+0 0x1p+1", "node 1000 0x1p+0 0x1.8p+1 -0x1p-3", "slice 1000 12"] +
                     [mc.mesh_line(t, n) for t, n in spans] + ["result 9 12 converged 3 0x1p+4 0x1p-2 0x1p-1"]) + "\n"
    d = mc.deform_file(text)
    assert d["mesh"] == spans and d["slice"] == [(1000, 12)] and d["result"][:4] == (9, 12, "converged", 3)
    assert d["pose"] == [(1000, 1.0, 3.0, -0.125, 0.0, 1.0, 2.0)] and d["node"] == [(1000, 1.0, 3.0, -0.125)]
    assert [mc.mesh_line(*m) for m in d["mesh"]] == text.splitlines()[3:6]
    assert mc.deform_file(text.replace(mc.mesh_line(*spans[1]) + "\n", ""))["mesh"] == [spans[0], spans[2]]
    assert mc.deform_file("result 4 0 insignificant 0 0x0p+0 0x0p+0 0x0p+0\n")["mesh"] == []          # a run without -m
