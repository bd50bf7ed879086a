/*
 * MeshChain -- the driver's side of the -m mesh and its post-passes: the meshes of the stages of MeshStages.h, the one runner every stage
 * goes through, the part of each stage that is its own, the writer every .ply goes through (-mn) and the view of the newest mesh (-mv).
 * Which stage runs, on which mesh, and which mesh is the newest is decided in MeshStages.h alone.
 */
#ifndef MESHCHAIN_H_
#define MESHCHAIN_H_

#include <cstdio>
#include <string>
#include <vector>

#include "LinearAlgebra.h"
#include "MeshGenerator.h"
#include "MeshStages.h"
#include "Resolution.h"

// `body` on a context of its own on `gpu`, as every stage, the view and the normals of a file run; `<flag>: <error>` when there is none.
// Returns body's result
template <class Body>
bool onOwnContext(int gpu, const char* flag, Body body)
{
    kt_ctx* ctx = 0;
    if (kt_ctx_create(gpu, &ctx) != KT_OK) { std::fprintf(stderr, "%s: %s\n", flag, kt_last_error()); return false; }
    const bool ok = body(ctx);
    kt_ctx_destroy(ctx);
    return ok;
}

// Every .ply this run writes goes through MeshWriter::write, so -mn is one switch.  With it on, the normals are taken from the mesh as
// it is written (MeshGenerator::normals, on a context of its own; a deformed mesh after its deformation), the file gets 27-byte vertex
// rows, and <prefix>.normals gains one line `<file name> <vertices> <triangles> <zero normals>`.  A failed normals call writes that file
// without normals, as without -mn, and sets `failed`: the driver then ends with its failure status.
struct MeshWriter {
    bool normals;       // -mn
    int gpu;
    std::string list;   // <prefix>.normals
    bool started, failed;

    // returns the number of triangles written, -1 on failure
    long long write(const MeshGenerator::Mesh& m, const std::string& path)
    {
        if (!normals) return MeshGenerator::write(m, path);
        std::vector<kt_mesh_normal> nrm;
        size_t nZero = 0;
        if (!onOwnContext(gpu, "-mn", [&](kt_ctx* ctx) { return MeshGenerator::normals(ctx, m, nrm, nZero); })) {
            std::fprintf(stderr, "no normals for %s: written without them\n", path.c_str());
            failed = true;
            return MeshGenerator::write(m, path);
        }
        const long long tris = MeshGenerator::write(m, nrm, path);
        if (tris < 0) return tris;
        FILE* f = std::fopen(list.c_str(), started ? "a" : "w");
        if (!f) { std::fprintf(stderr, "cannot write %s\n", list.c_str()); failed = true; return tris; }
        started = true;
        std::fprintf(f, "%s %zu %lld %zu\n", path.substr(path.find_last_of('/') + 1).c_str(), m.vertices.size(), tris, nZero);
        std::fclose(f);
        return tris;
    }
};

// What a stage has of its own: the call into MeshGenerator, and the lines only it writes
struct MeshStage {
    typedef MeshGenerator::Mesh Mesh;
    virtual ~MeshStage() {}
    virtual bool writesPly() const { return true; }
    // m holds a copy of the stage's input: the pass, in place
    virtual bool run(kt_ctx* ctx, Mesh& m) = 0;
    // the sidecar's `result` line and whatever follows it into f, and the stage's line on stdout; `name` is the file the stage wrote
    virtual void report(FILE* f, const std::string& name, const Mesh& in, const Mesh& out, long long tris) = 0;
};

struct MeshChain : MeshStageOrder {
    MeshGenerator::Mesh mesh[MESH_STAGES];   // kept for -mv and for -df, which deforms every one that was produced

    // Stage k >= 1 on the mesh the order gives it: <prefix><stem>.ply through the writer unless the stage only reports, and
    // <prefix><sidecar>: the `span utime first_in first_out` lines of the input's spans where the stage has them, then the stage's own
    void run(int k, MeshStage& body, int gpu, MeshWriter& writer, const std::string& prefix)
    {
        const MeshStageRule& rule = meshStageRules[k];
        const MeshGenerator::Mesh& in = mesh[newest(k)];
        MeshGenerator::Mesh& out = mesh[k];
        const bool writes = body.writesPly();
        record(k, false, writes);   // (until it is through)
        const bool ok = onOwnContext(gpu, rule.flag, [&](kt_ctx* ctx) {
            out = in;
            if (body.run(ctx, out)) return true;
            std::fprintf(stderr, rule.cannot, prefix.c_str());
            return false;
        });
        if (!ok) return;
        const std::string ply = prefix + rule.stem + ".ply";
        const long long tris = writes ? writer.write(out, ply) : (long long)(out.triangles.size() / 3);
        FILE* f = tris < 0 ? 0 : std::fopen((prefix + rule.sidecar).c_str(), "w");
        if (!f) { std::fprintf(stderr, "cannot write %s / %s%s\n", ply.c_str(), prefix.c_str(), rule.sidecar); return; }
        for (size_t s = 0; rule.spans && s < in.spanTime.size(); ++s)
            std::fprintf(f, "span %llu %zu %zu\n", (unsigned long long)in.spanTime[s], in.spanFirst[s], out.spanFirst[s]);
        body.report(f, writes ? ply : prefix + rule.sidecar, in, out, tris);
        std::fclose(f);
        record(k, true, writes);
    }
};

// -mw: the vertices that share a voxel-edge key merged (MeshGenerator::weld).  .weld: `result n_in n_out triangles`.
// gapSeconds < 0: no gate; otherwise slabs whose times (microseconds) differ by more stay apart.
struct WeldStage : MeshStage {
    double gapSeconds = -1.0;   // -mwg
    bool run(kt_ctx* ctx, Mesh& m) { return MeshGenerator::weld(ctx, m, gapSeconds < 0.0 ? UINT64_MAX : (uint64_t)(gapSeconds * 1e6)); }
    void report(FILE* f, const std::string& name, const Mesh& in, const Mesh& out, long long tris)
    {
        std::fprintf(f, "result %zu %zu %lld\n", in.vertices.size(), out.vertices.size(), tris);
        std::printf("mesh %s: %zu of %zu vertices, %lld triangles\n", name.c_str(), out.vertices.size(), in.vertices.size(), tris);
    }
};

// -mc: without the connected components of fewer than minTriangles triangles (MeshGenerator::dropSmallComponents).
// .comp: `result n_in n_out m_in m_out components kept largest`.
struct ComponentStage : MeshStage {
    long long minTriangles = 0;   // -mc: 1 to 2^32 - 1
    kt_mesh_component_stats stats = {0, 0, 0};
    bool run(kt_ctx* ctx, Mesh& m) { return MeshGenerator::dropSmallComponents(ctx, m, (uint32_t)minTriangles, stats); }
    void report(FILE* f, const std::string& name, const Mesh& in, const Mesh& out, long long tris)
    {
        std::fprintf(f, "result %zu %zu %zu %lld %llu %llu %llu\n", in.vertices.size(), out.vertices.size(), in.triangles.size() / 3, tris,
                     (unsigned long long)stats.components, (unsigned long long)stats.kept_components, (unsigned long long)stats.largest);
        std::printf("mesh %s: %zu of %zu vertices, %lld of %zu triangles, %llu of %llu components of at least %u triangles, the largest of %llu\n", name.c_str(),
                    out.vertices.size(), in.vertices.size(), tris, in.triangles.size() / 3, (unsigned long long)stats.kept_components, (unsigned long long)stats.components,
                    (uint32_t)minTriangles, (unsigned long long)stats.largest);
    }
};

// -mh: the open boundaries of the mesh reported, and with maxEdges > 0 its simple loops of at most maxEdges edges closed by a fan each
// (MeshGenerator::fillSmallHoles); -mh 0 writes no .ply.  .holes: one `loop label edges filled` line per simple loop, ascending by label,
// made here from the pass's loop_out and fill triangles, and `result n_in n_out m_in m_out` with the nine stats in the order of
// kt_mesh_hole_stats.
struct HoleStage : MeshStage {
    long long maxEdges = 0;   // -mh: 0 to 256
    kt_mesh_hole_stats st = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> loopOut;
    bool writesPly() const { return maxEdges > 0; }
    bool run(kt_ctx* ctx, Mesh& m) { return MeshGenerator::fillSmallHoles(ctx, m, (uint32_t)maxEdges, st, &loopOut); }
    void report(FILE* f, const std::string& name, const Mesh& in, const Mesh& out, long long tris)
    {
        // a loop's vertices carry its label, the smallest of them: edges[label] = their number.  Whether a loop was filled is read off the
        // pass's own output, so the fill rule is stated nowhere here: a fill triangle (behind the input's) is (b, a, centre) with a on the loop,
        // and input vertex v of span s sits at v + (first_out[s] - first_in[s])
        const size_t nIn = in.vertices.size(), mIn = in.triangles.size() / 3;
        std::vector<uint32_t> edges(nIn, 0), inputOf(out.vertices.size(), 0xffffffffu);
        std::vector<char> wasFilled(nIn, 0);
        for (size_t v = 0; v < loopOut.size(); ++v)
            if (loopOut[v] < 0xfffffffeu) edges[loopOut[v]] += 1;
        for (size_t s = 0; s < in.spanTime.size(); ++s)
            for (size_t v = in.spanFirst[s]; v < in.spanFirst[s + 1]; ++v) inputOf[v + (out.spanFirst[s] - in.spanFirst[s])] = (uint32_t)v;
        for (size_t t = mIn; t < out.triangles.size() / 3; ++t) wasFilled[loopOut[inputOf[out.triangles[3 * t + 1]]]] = 1;
        for (size_t l = 0; l < edges.size(); ++l)
            if (edges[l]) std::fprintf(f, "loop %zu %u %d\n", l, edges[l], (int)wasFilled[l]);
        std::fprintf(f, "result %zu %zu %zu %lld %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", nIn, out.vertices.size(), mIn, tris, (unsigned long long)st.boundary_edges,
                     (unsigned long long)st.nonmanifold_edges, (unsigned long long)st.degenerate_triangles, (unsigned long long)st.loops, (unsigned long long)st.open_components,
                     (unsigned long long)st.filled, (unsigned long long)st.longest, (unsigned long long)st.new_vertices, (unsigned long long)st.new_triangles);
        std::printf("mesh %s: %llu boundary edges in %llu loops (the longest of %llu) and %llu open components, %llu non-manifold edges; %llu loops of at most %u edges filled, "
                    "%zu vertices, %lld triangles\n", name.c_str(), (unsigned long long)st.boundary_edges, (unsigned long long)st.loops, (unsigned long long)st.longest,
                    (unsigned long long)st.open_components, (unsigned long long)st.nonmanifold_edges, (unsigned long long)st.filled, (uint32_t)maxEdges, out.vertices.size(), tris);
    }
};

// -mt: the vertex positions smoothed by `steps` steps of Taubin's lambda|mu filter at lambda = 0.5, mu = -0.53 (MeshGenerator::smooth);
// mode 0 pins the rims, mode 1 (-mtb) moves them along the rim.  .smooth: `result n m steps lambda mu mode rim moved edges`, the factors
// as hex floats, the last three kt_mesh_smooth_stats.
struct SmoothStage : MeshStage {
    long long steps = 0;   // -mt: 0 to 64
    bool rim = false;      // -mtb
    const float lambda = 0.5f, mu = -0.53f;
    kt_mesh_smooth_stats st = {0, 0, 0};
    bool run(kt_ctx* ctx, Mesh& m) { return MeshGenerator::smooth(ctx, m, (int)steps, lambda, mu, rim ? 1 : 0, st); }
    void report(FILE* f, const std::string& name, const Mesh&, const Mesh& out, long long tris)
    {
        std::fprintf(f, "result %zu %lld %d %a %a %d %llu %llu %llu\n", out.vertices.size(), tris, (int)steps, (double)lambda, (double)mu, rim ? 1 : 0,
                     (unsigned long long)st.rim_vertices, (unsigned long long)st.moved_vertices, (unsigned long long)st.unique_edges);
        std::printf("mesh %s: %d steps, %llu of %zu vertices moved over %llu edges, %llu rim vertices %s, %lld triangles\n", name.c_str(), (int)steps,
                    (unsigned long long)st.moved_vertices, out.vertices.size(), (unsigned long long)st.unique_edges, (unsigned long long)st.rim_vertices,
                    rim ? "moved along the rim" : "pinned", tris);
    }
};

// -ms: coarsened by vertex clustering at a cell of `cell` metres (MeshGenerator::simplify).  .simp: `result n_in n_out m_in m_out cell`.
// With -msq (quadric) the merged vertices come from the quadric form at `bias`, and a last line `quadric bias placed clusters` follows:
// how many of the clusters of more than one member sit at their quadrics' minimiser.
struct SimplifyStage : MeshStage {
    float cell = 0.0f;         // -ms: metres; the edge of the clustering cells
    bool quadric = false;      // -msq
    float bias = 0.015625f;    // -msb: the pull towards the mean
    size_t placed = 0;
    bool run(kt_ctx* ctx, Mesh& m) { return quadric ? MeshGenerator::simplify(ctx, m, cell, bias, placed) : MeshGenerator::simplify(ctx, m, cell); }
    void report(FILE* f, const std::string& name, const Mesh& in, const Mesh& out, long long tris)
    {
        std::fprintf(f, "result %zu %zu %zu %lld %a\n", in.vertices.size(), out.vertices.size(), in.triangles.size() / 3, tris, (double)cell);
        if (quadric) {
            const size_t merged = MeshGenerator::mergedClusters(in, cell);   // the clusters of more than one member: those the quadric form can place
            std::fprintf(f, "quadric %a %zu %zu\n", (double)bias, placed, merged);
            std::printf("mesh %s: %zu of %zu merged vertices at their quadrics' minimiser (bias %g)\n", name.c_str(), placed, merged, (double)bias);
        }
        std::printf("mesh %s: %zu of %zu vertices, %lld of %zu triangles\n", name.c_str(), out.vertices.size(), in.vertices.size(), tris, in.triangles.size() / 3);
    }
};

// -mv: `mesh`, which the run wrote as <prefix><stem>.ply, rendered from `pose` (a dense pose: [R | camera centre], in the frame of the mesh's
// vertices) moved `back` metres against its viewing axis, at the run's resolution and intrinsics with near = 0.05 m (MeshGenerator::render,
// on a context of its own): <prefix><stem>_view_depth.pgm (16-bit big-endian millimetres, as -ppm's), _view_color.ppm, _view_model.ppm, and
// <prefix><viewStem>.view, one `name value` line each: the file viewed, the frame, the number of dense poses, back and near, R (row-major)
// and t as hex floats, and the four kt_mesh_render_stats.
inline bool viewMesh(int gpu, const MeshGenerator::Mesh& mesh, const Intr& intr, const kt::Matrix4f& pose, long long frame, size_t poses, float back, const std::string& prefix,
                     const std::string& stem, const std::string& viewStem)
{
    const float near = 0.05f;
    float R[9], t[3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = pose(r, c);
    for (int r = 0; r < 3; ++r) t[r] = pose(r, 3) - back * R[3 * r + 2];
    const kt_intr k = {intr.fx, intr.fy, intr.cx, intr.cy};
    const int cols = Resolution::get().cols(), rows = Resolution::get().rows();
    MeshGenerator::View view;
    const bool ok = onOwnContext(gpu, "-mv", [&](kt_ctx* ctx) {
        if (MeshGenerator::render(ctx, mesh, k, cols, rows, R, t, near, view)) return true;
        std::fprintf(stderr, "cannot render the mesh of %s%s.ply\n", prefix.c_str(), stem.c_str());
        return false;
    });
    if (!ok) return false;
    const std::string base = prefix + stem + "_view";
    FILE* f = std::fopen((base + "_depth.pgm").c_str(), "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s_depth.pgm\n", base.c_str()); return false; }
    std::fprintf(f, "P5\n%d %d\n65535\n", cols, rows);
    for (size_t i = 0; i < view.depth.size(); ++i) {
        const unsigned char be[2] = {(unsigned char)(view.depth[i] >> 8), (unsigned char)(view.depth[i] & 255)};
        std::fwrite(be, 1, 2, f);
    }
    std::fclose(f);
    const char* names[2] = {"_color.ppm", "_model.ppm"};
    for (int n = 0; n < 2; ++n) {
        f = std::fopen((base + names[n]).c_str(), "wb");
        if (!f) { std::fprintf(stderr, "cannot write %s%s\n", base.c_str(), names[n]); return false; }
        const std::vector<uint8_t>& img = n == 0 ? view.color : view.model;
        std::fprintf(f, "P6\n%d %d\n255\n", cols, rows);
        std::fwrite(img.data(), 1, img.size(), f);
        std::fclose(f);
    }
    f = std::fopen((prefix + viewStem + ".view").c_str(), "w");
    if (!f) { std::fprintf(stderr, "cannot write %s%s.view\n", prefix.c_str(), viewStem.c_str()); return false; }
    const std::string file = prefix + stem + ".ply";
    std::fprintf(f, "file %s\nframe %lld\nposes %zu\nback %a\nnear %a\nR", file.substr(file.find_last_of('/') + 1).c_str(), frame, poses, (double)back, (double)near);
    for (int a = 0; a < 9; ++a) std::fprintf(f, " %a", (double)R[a]);
    std::fprintf(f, "\nt %a %a %a\n", (double)t[0], (double)t[1], (double)t[2]);
    std::fprintf(f, "drawn_triangles %llu\nclipped_triangles %llu\ndegenerate_triangles %llu\ncovered_pixels %llu\n", (unsigned long long)view.stats.drawn_triangles,
                 (unsigned long long)view.stats.clipped_triangles, (unsigned long long)view.stats.degenerate_triangles, (unsigned long long)view.stats.covered_pixels);
    std::fclose(f);
    std::printf("view %s_*: %s.ply from dense pose %lld of %zu, %.3f m back: %llu triangles drawn, %llu clipped, %llu degenerate, %llu of %d pixels covered\n", base.c_str(),
                (prefix + stem).c_str(), frame, poses, (double)back, (unsigned long long)view.stats.drawn_triangles, (unsigned long long)view.stats.clipped_triangles,
                (unsigned long long)view.stats.degenerate_triangles, (unsigned long long)view.stats.covered_pixels, cols * rows);
    return true;
}

#endif /* MESHCHAIN_H_ */
