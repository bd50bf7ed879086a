"""CPU: the mesh stage's case table (kintinuous_amd/mc_table.py -> kt_mc_table.hpp) and its numpy restatement
(kintinuous_amd/mesh_ref.py) on analytic signed-distance fields, and the PLY writer kt_host_save_ply (no GPU needed)."""
import os
from collections import Counter

import numpy as np
import pytest

from kintinuous_amd import mc_table, mesh_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_ply(path):
    """(vertices MESH-like: xyz float32 [n, 3] + rgb uint8 [n, 3] as a structured array, triangles int64 [m, 3]) of a binary
    little-endian PLY with the layout kt_host_save_ply writes"""
    with open(path, "rb") as f:
        data = f.read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
    props = [l.split()[-1] for l in lines if l.startswith("property") and "list" not in l]
    assert props == ["x", "y", "z", "red", "green", "blue"]
    assert "property list uchar int vertex_indices" in lines
    vd = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])
    v = np.frombuffer(body, vd, nv)
    fd = np.dtype([("n", "u1"), ("idx", "<i4", 3)])
    f = np.frombuffer(body, fd, nf, offset=nv * vd.itemsize)
    assert len(body) == nv * vd.itemsize + nf * fd.itemsize
    assert (f["n"] == 3).all()
    return v, f["idx"].astype(np.int64)


def _edge_pts(case, e):
    b, a = mc_table.EDGES[e]
    c0, c1 = mc_table.corner_pos(b), mc_table.corner_pos(b | (1 << a))
    return (c0 + c1) / 2.0, ((c1 - c0) if (case >> b) & 1 else (c0 - c1))


def test_header_is_the_generated_table():
    with open(mc_table.HEADER) as f:
        text = f.read()
    assert text == mc_table.header_text()
    tri, ntri = mc_table.parse_header(text)
    t2, n2 = mc_table.build_table()
    assert np.array_equal(tri, t2) and np.array_equal(ntri, n2)


def test_case_counts():
    tri, ntri = mc_table.build_table()
    assert ntri[0] == 0 and ntri[255] == 0
    assert int((ntri > 0).sum()) == 254 and int(ntri.max()) == mc_table.MAX_TRIS == 5
    assert dict(Counter(ntri.tolist())) == {0: 2, 1: 16, 2: 50, 3: 80, 4: 76, 5: 32}


def test_every_crossed_edge_used_and_boundary_is_the_face_segments():
    tri, ntri = mc_table.build_table()
    for case in range(256):
        crossed = {e for e, (b, a) in enumerate(mc_table.EDGES) if ((case >> b) & 1) != ((case >> (b | (1 << a))) & 1)}
        used = {int(e) for t in tri[case, :ntri[case]] for e in t}
        assert used == crossed, case
        # boundary edges (used by one triangle of the case) == the face segments, with their direction
        directed = Counter()
        for t in tri[case, :ntri[case]]:
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                directed[(int(a), int(b))] += 1
        undirected = Counter()
        for (a, b), n in directed.items():
            undirected[(min(a, b), max(a, b))] += n
        boundary = {(a, b) for (a, b) in directed if undirected[(min(a, b), max(a, b))] == 1}
        segs = {s for f in mc_table.FACES for s in mc_table.face_segments(case, f)}
        assert boundary == segs, case
        # interior diagonals: once in each direction
        for (a, b), n in directed.items():
            if undirected[(min(a, b), max(a, b))] != 1:
                assert n == 1 and directed[(b, a)] == 1, case


def test_faces_agree_between_neighbours():
    """For each face and each of its 16 sign patterns, every case sharing the pattern yields the same segments there."""
    for face in mc_table.FACES:
        _, _, cyc, _ = face
        seen = {}
        for case in range(256):
            pat = tuple((case >> c) & 1 for c in cyc)
            segs = frozenset(mc_table.face_segments(case, face))
            assert seen.setdefault(pat, segs) == segs
        assert len(seen) == 16
        # the neighbour across the face sees the same segments on its own opposite face (same edges, opposite direction)
        ax, side, _, _ = face
        opp = [f for f in mc_table.FACES if f[0] == ax and f[1] != side][0]
        for case in range(256):
            mirror = 0
            for c in range(8):
                if (case >> c) & 1:
                    mirror |= 1 << (c ^ (1 << ax))
            a = {tuple(sorted(mc_table.EDGES[e][1] for e in s)) for s in mc_table.face_segments(case, face)}
            b = {tuple(sorted(mc_table.EDGES[e][1] for e in s)) for s in mc_table.face_segments(mirror, opp)}
            assert a == b


def test_winding_points_outside():
    tri, ntri = mc_table.build_table()
    for case in range(1, 255):
        for loop in mc_table.case_loops(case):
            area, out = np.zeros(3), np.zeros(3)
            for i in range(1, len(loop) - 1):
                p0, p1, p2 = (_edge_pts(case, e)[0] for e in (loop[0], loop[i], loop[i + 1]))
                n = np.cross(p1 - p0, p2 - p0)
                d = sum(_edge_pts(case, e)[1] for e in (loop[0], loop[i], loop[i + 1]))
                assert np.dot(n, d) >= 0, case
                area += n
            for e in loop:
                out += _edge_pts(case, e)[1]
            assert np.dot(area, out) > 0, case


def _sdf_volume(fn, N, trunc=5.0):
    z, y, x = np.mgrid[0:N, 0:N, 0:N].astype(np.float64)
    r = fn(x, y, z)
    vol = np.clip(np.round(r / trunc * 32767), -32767, 32767).astype(np.int16)
    col = np.zeros((N, N, N, 4), np.uint8)
    col[..., 0] = 200
    col[..., 3] = 1
    return vol, col


def _topology(t):
    tt = t.astype(np.int64)
    d = np.concatenate([tt[:, [0, 1]], tt[:, [1, 2]], tt[:, [2, 0]]])
    u, cnt = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    closed = bool((cnt == 2).all() and len(np.unique(d, axis=0)) == len(d))
    return closed, len(u)


def _mesh(vol, col, N, wrap=(0, 0, 0)):
    """the mesh of a volume given in LOGICAL coordinates, stored under `wrap` (logical l lives at storage (l + wrap) % N)"""
    sh = (wrap[2], wrap[1], wrap[0])
    vol, col = np.roll(vol, sh, axis=(0, 1, 2)), np.roll(col, sh, axis=(0, 1, 2))
    return mesh_ref.extract_mesh(vol, col, (N / 16.0,) * 3, wrap, (0, 0, 0), (N - 1,) * 3, (0, 0, 0), N)


def test_sphere_closed_and_outward():
    N = 48
    c = np.array([23.3, 24.1, 22.7])
    vol, col = _sdf_volume(lambda x, y, z: np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - 14.2, N)
    v, t = _mesh(vol, col, N)
    closed, ne = _topology(t)
    assert closed and len(v) - ne + len(t) == 2
    cell = (N / 16.0) / N
    p = v["xyz"].astype(np.float64) / cell + N / 2 - 0.5         # back to voxel coordinates
    rad = np.sqrt(((p - c) ** 2).sum(axis=1))
    assert np.abs(rad - 14.2).max() < 1.0
    tri = p[t.astype(np.int64)]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert ((n * (tri.mean(axis=1) - c)).sum(axis=1) > 0).all()
    assert (v["rgb"] == (200 | (1 << 24))).all()


def test_torus_genus_one():
    N = 48
    R, r = 13.0, 5.5
    vol, col = _sdf_volume(lambda x, y, z: np.sqrt((np.sqrt((x - 23.6) ** 2 + (y - 24.3) ** 2) - R) ** 2 + (z - 23.9) ** 2) - r, N)
    v, t = _mesh(vol, col, N, wrap=(7, 0, 40))
    closed, ne = _topology(t)
    assert closed and len(v) - ne + len(t) == 0


def test_touching_spheres_ambiguous_faces_closed():
    """Two spheres 0.1 voxel apart along the cube diagonal: the gap crosses cell faces with alternating signs (ambiguous faces, on
    every face orientation); the mesh stays closed."""
    N = 40
    a = np.array([13.23, 13.61, 14.17])
    b = a + np.ones(3) / np.sqrt(3.0) * 13.7
    fn = lambda x, y, z: np.minimum(np.sqrt((x - a[0]) ** 2 + (y - a[1]) ** 2 + (z - a[2]) ** 2) - 6.8,
                                    np.sqrt((x - b[0]) ** 2 + (y - b[1]) ** 2 + (z - b[2]) ** 2) - 6.8)
    vol, col = _sdf_volume(fn, N, trunc=3.0)
    v, t = _mesh(vol, col, N)
    closed, ne = _topology(t)
    assert closed and len(v) - ne + len(t) in (2, 4)   # one or two components after quantisation
    F = vol < 0
    amb = 0
    for ax in range(3):
        G = np.moveaxis(F, ax, 0)
        amb += int(((G[:, :-1, :-1] == G[:, 1:, 1:]) & (G[:, :-1, 1:] == G[:, 1:, :-1]) & (G[:, :-1, :-1] != G[:, :-1, 1:])).sum())
    assert amb >= 10


def test_fma32_is_correctly_rounded():
    rng = np.random.default_rng(3)
    a = rng.standard_normal(100000).astype(np.float32)
    b = rng.standard_normal(100000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.uniform(-1e-6, 1e-6, 100000))).astype(np.float32)
    got = mesh_ref.fma32(a, b, c)
    from fractions import Fraction
    for i in range(0, 100000, 997):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        # the float32 nearest to the exact value (ties to even): compare with neighbours
        g = got[i]
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        d = abs(Fraction(float(g)) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact)


def test_ply_round_trip(tmp_path):
    from kintinuous_amd import abi
    rng = np.random.default_rng(5)
    meshes = []
    for n in (7, 0, 12):
        v = np.zeros(n, abi.MESH_VERTEX_DTYPE)
        v["xyz"] = rng.standard_normal((n, 3)).astype(np.float32)
        v["rgb"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        t = rng.integers(0, max(n, 1), (2 * n, 3)).astype(np.uint32)
        meshes.append((v, t))
    path = str(tmp_path / "m.ply")
    abi.save_ply(path, meshes)
    pv, pt = read_ply(path)
    v = np.concatenate([m[0] for m in meshes])
    assert np.array_equal(pv["xyz"], v["xyz"])
    assert np.array_equal(pv["rgb"][:, 0], ((v["rgb"] >> 16) & 255).astype(np.uint8))
    assert np.array_equal(pv["rgb"][:, 1], ((v["rgb"] >> 8) & 255).astype(np.uint8))
    assert np.array_equal(pv["rgb"][:, 2], (v["rgb"] & 255).astype(np.uint8))
    off = np.cumsum([0] + [len(m[0]) for m in meshes])
    want = np.concatenate([m[1].astype(np.int64) + off[i] for i, m in enumerate(meshes)])
    assert np.array_equal(pt, want)
    with pytest.raises(abi.KtError):   # an index past the vertices is refused
        abi.save_ply(path, [(meshes[0][0], np.array([[0, 1, 7]], np.uint32))])
