/*
 * MeshGenerator -- the -m output of the reference (backend/MeshGenerator.h, MeshGenerator::save, backend/MeshGenerator.cpp:37-188)
 * on this path: NOT its greedy-projection triangulation of the processed cloud, but the marching-cubes meshes the tracker's mesh
 * stage (kt_tracker_enable_mesh_stage) built on the GPU for every slab that left the volume and for the final volume.  save()
 * concatenates them in slice order, the triangle indices offset by the vertices before them (the shape of the reference's merge,
 * :82-137), and writes <prefix>.ply (kt_host_save_ply): two neighbouring slabs each keep their own vertex on the edges of the plane
 * between them.
 * collect() is that concatenation alone, with one span per slice that has a mesh: its first vertex and the slice's time
 * (kt_tracker_slice_pose's ts, the utime its processedCloud is deformed with) -- the span table of kt_deform_apply_mesh, which the
 * driver's -df deforms the vertices with before it writes <prefix>_def.ply over the same triangles.
 * With the tracker's keys on (kt_tracker_enable_mesh_keys) collect() also gathers every vertex's voxel-edge key, and weld() merges the
 * vertices that share one (kt_mesh_weld): the seams close, and the mesh keeps its shape as a span table for kt_deform_apply_mesh.  What
 * stays open: a seam edge whose sign change sits on another edge at the later time, and the one-cell gap where the cleared plane was
 * never fused again.
 * simplify() coarsens the mesh, welded or not, by vertex clustering (kt_mesh_simplify): the vertices of one span in one cubic cell become
 * their mean and the collapsed triangles go; the result is again a mesh with a span table.  Its quadric form (kt_mesh_simplify_quadric) puts
 * the merged vertex at the minimiser of the error quadrics of the triangles that touch its cluster instead, so edges and corners stay sharp.
 * dropSmallComponents() removes the connected pieces of the mesh, welded or not, that have fewer triangles than a threshold
 * (kt_mesh_components): the floating speckle a marching-cubes mesh of a real TSDF is surrounded by; the result is again a mesh with a span
 * table, which simplify() then takes.
 * fillSmallHoles() reports the open boundaries of the mesh and closes its simple loops of a few edges with a fan each (kt_mesh_holes): the
 * pinhole cracks the weld leaves.  The long one-cell gap between two slabs is two long rims: reported, not closed.
 * smooth() low-pass filters the vertex positions over the mesh's own edges (kt_mesh_smooth, Taubin's lambda|mu filter): the voxel-scale
 * staircase and the depth noise of the surface go, its size stays; the triangles and the span table are untouched.
 * render() draws any of these meshes from a camera pose (kt_mesh_render, a software rasteriser): a depth image in the format of -ppm's, the
 * vertex colours, and a flat-shaded view; the reference shows its mesh through OpenGL, which is out of scope.
 * normals() gives any of these meshes a normal per vertex from its own triangles (kt_mesh_normals), which write()'s second form puts
 * into the file: what the reference's .ply carries because it meshes a PointXYZRGBNormal cloud.
 */
#ifndef MESHGENERATOR_H_
#define MESHGENERATOR_H_

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "internal.h"

class MeshGenerator
{
  public:
    // the -m mesh as arrays; spanFirst has one entry more than spanTime: span s = vertices [spanFirst[s], spanFirst[s + 1])
    struct Mesh {
        std::vector<kt_mesh_vertex> vertices;
        std::vector<uint32_t> triangles;
        std::vector<size_t> spanFirst;
        std::vector<uint64_t> spanTime;
        std::vector<uint64_t> keys;   // one per vertex, or empty: some slice was meshed without keys
    };

    // the meshes of every slice of tracker t in slice order; false on failure
    static bool collect(kt_tracker* t, Mesh& m)
    {
        const int n = kt_tracker_num_slices(t);
        if (n < 0) return false;
        std::vector<kt_mesh_vertex>& v = m.vertices;
        std::vector<uint32_t>& tri = m.triangles;
        v.clear(); tri.clear(); m.spanFirst.clear(); m.spanTime.clear(); m.keys.clear();
        bool keyed = true;
        for (int i = 0; i < n; ++i) {
            long long nv = 0, nt = 0;
            if (kt_tracker_slice_mesh_info(t, i, &nv, &nt) != KT_OK) return false;
            if (nv < 0) continue;   // taken while the stage was off
            float R[9], cam[3];
            uint64_t ts = 0;
            if (kt_tracker_slice_pose(t, i, R, cam, &ts) != KT_OK) return false;
            const size_t v0 = v.size(), t0 = tri.size();
            m.spanFirst.push_back(v0);
            m.spanTime.push_back(ts);
            v.resize(v0 + (size_t)nv);
            tri.resize(t0 + 3 * (size_t)nt);
            if (kt_tracker_slice_mesh(t, i, v.data() + v0, tri.data() + t0) != KT_OK) {
                std::fprintf(stderr, "slice %d: %s\n", i, kt_last_error());
                return false;
            }
            for (size_t k = t0; k < tri.size(); ++k) tri[k] += (uint32_t)v0;
            if (keyed) {
                m.keys.resize(v.size());
                keyed = kt_tracker_slice_mesh_keys(t, i, m.keys.data() + v0) == KT_OK;   // KT_ERR_STATE: meshed without keys
            }
        }
        if (!keyed) m.keys.clear();
        m.spanFirst.push_back(v.size());
        return true;
    }

    // welds the vertices of m that share a key, in place: vertices, keys, triangles and spanFirst become the welded mesh's (spanTime
    // stays).  maxGap: spans whose times differ by more do not weld (UINT64_MAX: no gate).  false on failure, m untouched
    static bool weld(kt_ctx* ctx, Mesh& m, uint64_t maxGap)
    {
        if (m.keys.size() != m.vertices.size()) { std::fprintf(stderr, "weld: the mesh has no keys\n"); return false; }
        const size_t n = m.vertices.size();
        Rebuilt r(m, n, 0);
        r.tri = m.triangles;   // renumbered in place: a weld drops no triangle
        r.mOut = m.triangles.size() / 3;
        std::vector<uint64_t> k(n);
        if (!withPass("weld", kt_mesh_weld_create, kt_mesh_weld_destroy, ctx, [&](kt_mesh_welder* w) {
                return kt_mesh_weld(w, m.vertices.data(), m.keys.data(), n, r.tri.data(), r.mOut, m.spanFirst.data(), m.spanTime.data(), (int)m.spanTime.size(), maxGap,
                                    r.v.data(), k.data(), n, r.first.data(), &r.nOut);
            }))
            return false;
        r.commit(m);
        k.resize(m.vertices.size());
        m.keys.swap(k);
        return true;
    }

    // merges the vertices of m that share a cell of edge `cell` metres and a span, in place: vertices, triangles and spanFirst become the
    // simplified mesh's (spanTime stays); keys are cleared, because edge keys name no cluster.  false on failure, m untouched
    static bool simplify(kt_ctx* ctx, Mesh& m, float cell) { return simplifyBody(ctx, m, cell, 0, 0); }

    // the quadric form of simplify(): a merged vertex goes to the minimiser of its cluster's error quadrics, pulled towards the mean by
    // `bias` (2^-20 to 1), where that lies in the cluster's cell, and to the mean otherwise.  placed: how many did
    static bool simplify(kt_ctx* ctx, Mesh& m, float cell, float bias, size_t& placed) { return simplifyBody(ctx, m, cell, &bias, &placed); }

    // how many clusters of simplify() at `cell` have more than one member (counted on the host by the key rule of kt_mesh_simplify: one
    // cell of one span): what `placed` of the quadric form is out of
    static size_t mergedClusters(const Mesh& m, float cell)
    {
        const double inv = 1.0 / (double)cell;
        std::vector<std::array<long long, 4> > key(m.vertices.size());
        for (size_t s = 0; s < m.spanTime.size(); ++s)
            for (size_t i = m.spanFirst[s]; i < m.spanFirst[s + 1]; ++i) {
                const float x[3] = {m.vertices[i].x, m.vertices[i].y, m.vertices[i].z};
                key[i][0] = (long long)s;
                for (int a = 0; a < 3; ++a) key[i][a + 1] = (long long)std::floor((double)x[a] * inv);
            }
        std::sort(key.begin(), key.end());
        size_t merged = 0;
        for (size_t i = 0, j; i < key.size(); i = j) {
            for (j = i + 1; j < key.size() && key[j] == key[i]; ++j) {}
            merged += j - i > 1;
        }
        return merged;
    }

    // drops the connected components of m that have fewer than minTriangles triangles (kt_mesh_components), in place: vertices, triangles
    // and spanFirst become the filtered mesh's (spanTime stays); keys are cleared, as simplify() clears them: nothing after the weld reads
    // them.  false on failure, m and stats untouched
    static bool dropSmallComponents(kt_ctx* ctx, Mesh& m, uint32_t minTriangles, kt_mesh_component_stats& stats)
    {
        const size_t n = m.vertices.size(), nt = m.triangles.size() / 3;
        Rebuilt r(m, n, nt);
        kt_mesh_component_stats st = {0, 0, 0};
        if (!withPass("components", kt_mesh_components_create, kt_mesh_components_destroy, ctx, [&](kt_mesh_component_pass* w) {
                return kt_mesh_components(w, m.vertices.data(), n, m.triangles.data(), nt, m.spanFirst.data(), (int)m.spanTime.size(), minTriangles, r.v.data(), n,
                                          r.tri.data(), nt, 0, r.first.data(), &r.nOut, &r.mOut, &st);
            }))
            return false;
        r.commit(m);
        stats = st;
        return true;
    }

    // finds the open boundaries of m and closes its simple loops of at most maxEdges edges with a fan around their centre (kt_mesh_holes),
    // in place: vertices, triangles and spanFirst become the filled mesh's (spanTime stays); keys are cleared, as simplify() clears them.
    // loopOut: one word per INPUT vertex (kt_abi.h).  maxEdges below 3 only reports.  false on failure, m, stats and loopOut untouched
    static bool fillSmallHoles(kt_ctx* ctx, Mesh& m, uint32_t maxEdges, kt_mesh_hole_stats& stats, std::vector<uint32_t>* loopOut = 0)
    {
        const size_t n = m.vertices.size(), nt = m.triangles.size() / 3;
        const size_t vcap = n + n / 3, tcap = nt + (n < 3 * nt ? n : 3 * nt);   // the most a call can give
        Rebuilt r(m, vcap, tcap);
        std::vector<uint32_t> loops(n);
        kt_mesh_hole_stats st = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (!withPass("holes", kt_mesh_holes_create, kt_mesh_holes_destroy, ctx, [&](kt_mesh_hole_pass* w) {
                return kt_mesh_holes(w, m.vertices.data(), n, m.triangles.data(), nt, m.spanFirst.data(), (int)m.spanTime.size(), maxEdges, r.v.data(), vcap, r.tri.data(),
                                     tcap, loops.data(), r.first.data(), &r.nOut, &r.mOut, &st);
            }))
            return false;
        r.commit(m);
        stats = st;
        if (loopOut) loopOut->swap(loops);
        return true;
    }

    // smooths the vertex positions of m over its own edges with `steps` steps of Taubin's lambda|mu filter (kt_mesh_smooth), in place:
    // mode 0 pins the rim vertices, mode 1 moves them along the rim.  Triangles, spanFirst and spanTime stay: no vertex is added, dropped
    // or renumbered; keys are cleared, because a smoothed vertex no longer lies on its voxel edge.  false on failure, m and stats untouched
    static bool smooth(kt_ctx* ctx, Mesh& m, int steps, float lambda, float mu, int mode, kt_mesh_smooth_stats& stats)
    {
        std::vector<kt_mesh_vertex> v(m.vertices.size());
        kt_mesh_smooth_stats st = {0, 0, 0};
        if (!withPass("smooth", kt_mesh_smooth_create, kt_mesh_smooth_destroy, ctx, [&](kt_mesh_smooth_pass* w) {
                return kt_mesh_smooth(w, m.vertices.data(), m.vertices.size(), m.triangles.data(), m.triangles.size() / 3, steps, lambda, mu, mode, v.data(), &st);
            }))
            return false;
        m.vertices.swap(v); m.keys.clear();
        stats = st;
        return true;
    }

    // the images of one view of m (kt_mesh_render)
    struct View {
        std::vector<uint16_t> depth;   // millimetres, 0 where no triangle covers the pixel
        std::vector<uint8_t> color;    // rgb24: the vertex colours, interpolated
        std::vector<uint8_t> model;    // rgb24: flat shading, the light at the camera
        kt_mesh_render_stats stats;
    };

    // renders m from the camera (R camera-to-world row-major, t its centre, both in the frame of m's vertices, as kt_tracker_get_pose and
    // the dense poses give them) at cols x rows with the intrinsics intr; triangles with a vertex nearer than `near` metres are dropped
    // whole.  false on failure, view untouched
    static bool render(kt_ctx* ctx, const Mesh& m, const kt_intr& intr, int cols, int rows, const float R[9], const float t[3], float near, View& view)
    {
        const size_t pixels = cols > 0 && rows > 0 ? (size_t)cols * (size_t)rows : 0;
        View v = View();   // (the stats at zero)
        v.depth.resize(pixels); v.color.resize(3 * pixels); v.model.resize(3 * pixels);
        if (!withPass("render", kt_mesh_render_create, kt_mesh_render_destroy, ctx, [&](kt_mesh_render_pass* w) {
                return kt_mesh_render(w, m.vertices.data(), m.vertices.size(), m.triangles.data(), m.triangles.size() / 3, &intr, cols, rows, R, t, near, 0, v.depth.data(),
                                      v.color.data(), v.model.data(), &v.stats);
            }))
            return false;
        view.depth.swap(v.depth); view.color.swap(v.color); view.model.swap(v.model);
        view.stats = v.stats;
        return true;
    }

    // returns the number of triangles written, -1 on failure
    static long long write(const Mesh& m, const std::string& path)
    {
        if (kt_host_save_ply(path.c_str(), m.vertices.data(), m.vertices.size(), m.triangles.data(), m.triangles.size() / 3) != KT_OK) {
            std::fprintf(stderr, "%s\n", kt_last_error());
            return -1;
        }
        return (long long)(m.triangles.size() / 3);
    }

    // the area-weighted vertex normals of m from its own triangles (kt_mesh_normals); nZero: the vertices left at (0, 0, 0).  false on
    // failure, normals untouched
    static bool normals(kt_ctx* ctx, const Mesh& m, std::vector<kt_mesh_normal>& normals, size_t& nZero)
    {
        std::vector<kt_mesh_normal> out(m.vertices.size());
        size_t zero = 0;
        if (!withPass("normals", kt_mesh_normals_create, kt_mesh_normals_destroy, ctx, [&](kt_mesh_normal_pass* w) {
                return kt_mesh_normals(w, m.vertices.data(), m.vertices.size(), m.triangles.data(), m.triangles.size() / 3, out.data(), &zero);
            }))
            return false;
        normals.swap(out); nZero = zero;
        return true;
    }

    // the mesh with a normal per vertex (kt_host_save_ply_normals); returns the number of triangles written, -1 on failure
    static long long write(const Mesh& m, const std::vector<kt_mesh_normal>& normals, const std::string& path)
    {
        if (normals.size() != m.vertices.size()) { std::fprintf(stderr, "%s: %zu normals for %zu vertices\n", path.c_str(), normals.size(), m.vertices.size()); return -1; }
        if (kt_host_save_ply_normals(path.c_str(), m.vertices.data(), normals.data(), m.vertices.size(), m.triangles.data(), m.triangles.size() / 3) != KT_OK) {
            std::fprintf(stderr, "%s\n", kt_last_error());
            return -1;
        }
        return (long long)(m.triangles.size() / 3);
    }

    // the meshes of every slice of tracker t; returns the number of triangles written, -1 on failure
    static long long save(kt_tracker* t, const std::string& path)
    {
        Mesh m;
        return collect(t, m) ? write(m, path) : -1;
    }

  private:
    // what every pass wrapper above does around its call: the pass created on ctx, `call` run on it, `<name>: <kt_last_error()>` printed
    // when either fails, the pass destroyed.  The wrapper commits its outputs only when this returns true
    template <class Pass, class Call>
    static bool withPass(const char* name, int (*create)(kt_ctx*, void*, Pass**), int (*destroy)(Pass*), kt_ctx* ctx, Call call)
    {
        Pass* w = 0;
        int s = create(ctx, 0, &w);
        if (s == KT_OK) s = call(w);
        if (s != KT_OK) std::fprintf(stderr, "%s: %s\n", name, kt_last_error());
        if (w) destroy(w);
        return s == KT_OK;
    }

    // the outputs of a pass that rebuilds the mesh, sized for the most a call can give (vcap vertices, tcap triangles), and their commit
    // into m: vertices, triangles and spanFirst become the pass's (spanTime stays), keys are cleared
    struct Rebuilt {
        std::vector<kt_mesh_vertex> v;
        std::vector<uint32_t> tri;
        std::vector<size_t> first;
        size_t nOut, mOut;
        Rebuilt(const Mesh& m, size_t vcap, size_t tcap) : v(vcap), tri(3 * tcap), first(m.spanFirst.size()), nOut(0), mOut(0) {}
        void commit(Mesh& m)
        {
            v.resize(nOut); tri.resize(3 * mOut);
            m.vertices.swap(v); m.triangles.swap(tri); m.spanFirst.swap(first); m.keys.clear();
        }
    };

    static bool simplifyBody(kt_ctx* ctx, Mesh& m, float cell, const float* bias, size_t* placed)
    {
        const size_t n = m.vertices.size(), nt = m.triangles.size() / 3;
        Rebuilt r(m, n, nt);
        size_t nPlaced = 0;
        if (!withPass("simplify", kt_mesh_simplify_create, kt_mesh_simplify_destroy, ctx, [&](kt_mesh_simplifier* w) {
                return bias ? kt_mesh_simplify_quadric(w, m.vertices.data(), n, m.triangles.data(), nt, m.spanFirst.data(), (int)m.spanTime.size(), cell, *bias, r.v.data(),
                                                       n, r.tri.data(), nt, r.first.data(), &r.nOut, &r.mOut, &nPlaced)
                            : kt_mesh_simplify(w, m.vertices.data(), n, m.triangles.data(), nt, m.spanFirst.data(), (int)m.spanTime.size(), cell, r.v.data(), n, r.tri.data(),
                                               nt, r.first.data(), &r.nOut, &r.mOut);
            }))
            return false;
        r.commit(m);
        if (placed) *placed = nPlaced;
        return true;
    }
};

#endif /* MESHGENERATOR_H_ */
