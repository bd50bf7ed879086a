// kintinuous_hip -- headless driver of the tracking + fusion path over a .klg log: the part of the reference's
// `Kintinuous -l log.klg [-c calib] [-s size] [-t shift] [-r|-ri] [-fod] [-sm] ...` run (src/Kintinuous.cpp,
// MainController.cpp:73-170) that ends at the CloudSlices and the .poses file.  Extra options: -n <N>, -w/-h, -o <prefix>,
// -ops (compose every frame from the internal.h operators instead of the device-resident tracker), -pcd (run the CloudSliceProcessor thread
// behind the tracker and save <prefix>.pcd the way CloudSliceProcessor::save does), -ppm (write the model views), -m (marching-cubes
// meshes of the slabs and the final volume into <prefix>.ply), -mw [-mwg <seconds>] (with -m: the slab seams welded by voxel-edge key,
// <prefix>_weld.ply and <prefix>.weld; -mwg keeps slabs further apart in time than that unwelded; with -df also <prefix>_weld_def.ply),
// -ms <metres> (with -m: the mesh, welded with -mw, coarsened by vertex clustering, <prefix>_simp.ply and <prefix>.simp; with -df also
// <prefix>_simp_def.ply), -mc <triangles> (with -m: the mesh, welded with -mw, without its connected pieces of fewer triangles than that,
// <prefix>_comp.ply and <prefix>.comp; -ms then coarsens this mesh; with -df also <prefix>_comp_def.ply), -mn (with -m: every .ply of the run carries a normal per vertex, taken on the GPU from that file's own
// triangles, and <prefix>.normals lists the files), -mv [-mvf <i>] [-mvb <metres>] (with -m: the last mesh the run writes, rendered on the GPU
// from the last dense pose or pose i, that far back along its viewing axis: <stem>_view_depth.pgm, _view_color.ppm, _view_model.ppm and
// <prefix>.view; with -df also the deformed twin from the optimised pose), -pg [-it <thresh>] (with -v <vocab> -lc: the pose graph over the accepted
// loop constraints, <prefix>.graph and <prefix>_opt.poses), -df [-dg <poseDist>] (with -pg and -pcd: the map deformed onto the optimised
// trajectory, <prefix>_def.pcd and <prefix>.deform, with -m also the mesh, <prefix>_def.ply; -ds <error> moves the 0.1 gate below which
// nothing is deformed).
#include <zlib.h>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <map>
#include <string>
#include <thread>

#include "CloudSliceProcessor.h"
#include "DeformationGraph.h"
#include "MeshGenerator.h"
#include "iSAMInterface.h"
#include "PlaceRecognition.h"
#include "TrackerInterface.h"

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
        kt_ctx* nctx = 0;
        bool ok = kt_ctx_create(gpu, &nctx) == KT_OK;
        if (!ok) std::fprintf(stderr, "-mn: %s\n", kt_last_error());
        else {
            ok = MeshGenerator::normals(nctx, m, nrm, nZero);
            kt_ctx_destroy(nctx);
        }
        if (!ok) {
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

static Intr loadCalibration(const std::string& file, int width, int height)
{
    // MainController.cpp:121-150: a calibration file holds "fx fy cx cy"; the default is 528 / 528 / 320 / 240 at VGA
    Intr k(528.0f * width / 640.0f, 528.0f * height / 480.0f, 320.0f * width / 640.0f, 240.0f * height / 480.0f);
    if (file.size()) {
        std::ifstream f(file.c_str());
        double fx, fy, cx, cy;
        if (f >> fx >> fy >> cx >> cy) k = Intr((float)fx, (float)fy, (float)cx, (float)cy);
        else { std::fprintf(stderr, "cannot read calibration %s\n", file.c_str()); std::exit(1); }
    }
    return k;
}

// -pcdraw (debug): every extracted slice as the tracker produced it, appended into one binary PCD in pcl::PointXYZRGB field order
// (x y z rgb) -- the input of the slice processor, for comparing extraction paths point by point
static bool writeRawPcd(const std::string& file, const std::vector<CloudSlice*>& slices)
{
    size_t n = 0;
    for (size_t i = 0; i < slices.size(); ++i) n += slices[i]->cloud->size();
    FILE* f = std::fopen(file.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
                    "WIDTH %zu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %zu\nDATA binary\n", n, n);
    for (size_t i = 0; i < slices.size(); ++i)
        for (size_t k = 0; k < slices[i]->cloud->size(); ++k) {
            const unsigned char* p = reinterpret_cast<const unsigned char*>(&(*slices[i]->cloud)[k]);
            std::fwrite(p, 1, 12, f);        // x y z
            std::fwrite(p + 16, 1, 4, f);    // b g r a
        }
    return std::fclose(f) == 0;
}

// -ppm: the reference's live views of the final model, without a window: <prefix>_model.ppm (shaded), <prefix>_color.ppm (fused
// colour), <prefix>_depth.pgm (16-bit millimetres)
static void writeViews(KintinuousTracker* fe, const std::string& prefix)
{
    fe->getImage();
    fe->getModelDepth();
    const int rows = Resolution::get().rows(), cols = Resolution::get().cols();
    std::vector<PixelRGB> img;
    int c;
    const char* names[2] = {"_model.ppm", "_color.ppm"};
    for (int k = 0; k < 2; ++k) {
        (k == 0 ? fe->modelSurface : fe->modelColor).download(img, c);
        FILE* f = std::fopen((prefix + names[k]).c_str(), "wb");
        if (!f) continue;
        std::fprintf(f, "P6\n%d %d\n255\n", cols, rows);
        std::fwrite(img.data(), 3, img.size(), f);
        std::fclose(f);
    }
    FILE* f = std::fopen((prefix + "_depth.pgm").c_str(), "wb");
    if (!f) return;
    std::fprintf(f, "P5\n%d %d\n65535\n", cols, rows);
    for (size_t i = 0; i < fe->modelDepthHost.size(); ++i) {
        const unsigned char be[2] = {(unsigned char)(fe->modelDepthHost[i] >> 8), (unsigned char)(fe->modelDepthHost[i] & 255)};
        std::fwrite(be, 1, 2, f);
    }
    std::fclose(f);
}

// -rank R -world W -comm <file> [-gk K]: one process per GPU, each on its own log; after the last frame the ranks exchange their K most
// recent dense poses (default 1: the final pose) with the path's single collective (kt_pose_gather: one RCCL all-gather over xGMI).
// EVERY rank contributes the same K -- a collective with unequal counts hangs -- so K comes from the command line, not from the length
// of the rank's own log, and a rank whose log gave fewer than K poses fails BEFORE it joins the communicator.  Rank 0 writes the
// 128-byte RCCL id to <file> (atomically, via rename); the other ranks wait for it.  A watchdog ends the process if the rendezvous or
// the gather does not complete (a rank that died leaves the others inside RCCL for ever): KT_COMM_TIMEOUT_S, default 120.
static bool gatherPoses(KintinuousTracker* fe, int rank, int world, const std::string& idFile, int k)
{
    const int have = kt_tracker_num_poses(fe->handle());
    if (k < 1 || have < k) {
        std::fprintf(stderr, "rank %d: %d dense poses, the gather needs %d from every rank (-gk)\n", rank, have, k);
        return false;
    }
    std::atomic<bool> done(false);
    const char* to = std::getenv("KT_COMM_TIMEOUT_S");
    const int timeout_s = to ? std::atoi(to) : 120;
    std::thread watchdog([&done, timeout_s, rank]() {
        for (int waited = 0; waited < timeout_s * 10 && !done; ++waited) std::this_thread::sleep_for(std::chrono::milliseconds(100));
        if (!done) {
            std::fprintf(stderr, "rank %d: pose gather did not complete within %d s (another rank missing?)\n", rank, timeout_s);
            std::_Exit(3);
        }
    });
    struct Join { std::atomic<bool>& d; std::thread& t; ~Join() { d = true; t.join(); } } join{done, watchdog};
    unsigned char id[KT_COMM_ID_BYTES];
    if (rank == 0) {
        ktSafeCall(kt_comm_unique_id(id));
        FILE* f = std::fopen((idFile + ".tmp").c_str(), "wb");
        if (!f || std::fwrite(id, 1, sizeof(id), f) != sizeof(id) || std::fclose(f) != 0) return false;
        if (std::rename((idFile + ".tmp").c_str(), idFile.c_str()) != 0) return false;
    } else {
        for (;;) {   // (bounded by the watchdog)
            FILE* f = std::fopen(idFile.c_str(), "rb");
            if (f) {
                const size_t got = std::fread(id, 1, sizeof(id), f);
                std::fclose(f);
                if (got == sizeof(id)) break;
            }
            std::this_thread::sleep_for(std::chrono::milliseconds(10));
        }
    }
    kt_comm* comm = 0;
    ktSafeCall(kt_comm_init(kt::device::context(), rank, world, id, &comm));
    std::vector<float> all((size_t)world * k * 16);
    ktSafeCall(kt_pose_gather(comm, fe->handle(), k, all.data()));
    ktSafeCall(kt_comm_destroy(comm));
    for (int r = 0; r < world; ++r) {
        const float* p = &all[((size_t)r * k + (k - 1)) * 16];
        std::printf("rank %d sees stream %d: last camera %.6f %.6f %.6f (%d poses gathered, %zu bytes)\n", rank, r, p[3], p[7], p[11], k,
                    all.size() * sizeof(float));
    }
    return true;
}

// -pg: the dense pose graph over the accepted constraints (Deformation::addCameraCamera without -fl, then addCameraLoop's rule for every
// constraint in order: add it and optimise; it stays when chi2 < thresh, otherwise it is removed and the graph optimised again,
// Deformation.cpp:250-256, 336-340).  The graph holds at most 64 loops: a 65th constraint next to 64 kept ones ends the run with an error.  Writes <prefix>_opt.poses in the format of <prefix>.poses (every node in time order, the first
// frame included, which .poses leaves out) and <prefix>.graph, one line per
// constraint: time1 time2 chi2 kept|rejected steps (chi2 as a hex float, both of the optimisation with the constraint in).
static bool optimisePoseGraph(kt_ctx* ctx, KintinuousTracker* fe, const std::vector<LoopClosureConstraint>& constraints, double thresh, const std::string& prefix,
                              std::vector<char>& keptOut, std::vector<std::pair<uint64_t, kt::Matrix4f> >& posesOut)
{
    FILE *g = 0, *f = 0;
    try {
        iSAMInterface iSAM(ctx);
        const std::vector<KintinuousTracker::DensePose>& dense = fe->densePoseGraph;
        for (size_t i = 1; i < dense.size(); ++i) {
            float Rp[9], tp[3], Rc[9], tc[3];
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) { Rp[3 * r + c] = dense[i - 1].pose(r, c); Rc[3 * r + c] = dense[i].pose(r, c); }
                tp[r] = dense[i - 1].pose(r, 3); tc[r] = dense[i].pose(r, 3);
            }
            iSAM.addCameraCameraConstraint(dense[i - 1].timestamp, dense[i].timestamp, Rp, tp, Rc, tc);
        }
        g = std::fopen((prefix + ".graph").c_str(), "w");
        if (!g) { std::fprintf(stderr, "cannot write %s.graph\n", prefix.c_str()); return false; }
        size_t kept = 0;
        for (size_t i = 0; i < constraints.size(); ++i) {
            const LoopClosureConstraint& c = constraints[i];
            const iSAMInterface::Factor f = iSAM.addLoopConstraint(c.time1, c.time2, c.icpTrans);
            const double chi2 = iSAM.optimise();
            const int steps = iSAM.lastStepCount();
            const bool stays = chi2 < thresh;
            if (!stays) { iSAM.removeFactor(f); iSAM.optimise(); }
            kept += stays;
            keptOut.push_back(stays ? 1 : 0);
            std::fprintf(g, "%llu %llu %a %s %d\n", (unsigned long long)c.time1, (unsigned long long)c.time2, chi2, stays ? "kept" : "rejected", steps);
        }
        std::fclose(g);
        g = 0;
        std::vector<std::pair<uint64_t, kt::Matrix4f> > poses;
        iSAM.getCameraPoses(poses);
        posesOut = poses;
        f = std::fopen((prefix + "_opt.poses").c_str(), "w");
        if (!f) { std::fprintf(stderr, "cannot write %s_opt.poses\n", prefix.c_str()); return false; }
        for (size_t i = 0; i < poses.size(); ++i) {   // KintinuousTracker::outputPose's line
            const kt::Matrix4f& P = poses[i].second;
            kt::Matrix3f R;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) R(r, c) = P(r, c);
            const kt::Quaternionf q(R);
            std::fprintf(f, "%.6f %g %g %g %g %g %g %g\n", (double)poses[i].first / 1000000.0, P(0, 3), P(1, 3), P(2, 3), q.x, q.y, q.z, q.w);
        }
        std::fclose(f);
        f = 0;
        std::printf("pose graph %s.graph: %zu nodes, %zu of %zu constraints kept\n", prefix.c_str(), iSAM.numNodes(), kept, constraints.size());
        return true;
    } catch (const std::exception& e) {
        if (g) std::fclose(g);   // (the lines written so far stay: every constraint before the one that failed)
        if (f) std::fclose(f);
        std::fprintf(stderr, "-pg: %s\n", e.what());
        return false;
    }
}

// -df: the map deformed onto the optimised trajectory (Deformation::addCameraLoop's last step, Deformation.cpp:192-231, 258-334, once, after
// the final pose graph).  Nodes are sampled from the ORIGINAL dense poses (one per node time of the pose graph, in time order).
// Constraints: every camera position, original -> optimised, at its time; for every KEPT loop each inliers1Proj point at time1 and each
// inliers2Proj point at time2, the source the point through the original pose of that time (rounded to float, as the reference's point
// pool holds it), the target the same point through the optimised pose.  The graph is applied to every slice's processedCloud with the
// slice's utime and the slices are saved through CloudSliceProcessor::save as <prefix>_def.pcd; nothing is applied when the status is
// insignificant or singular, or with fewer than five nodes.  <prefix>.deform holds the stage's inputs, floats in hex: `pose time x y z X Y Z`
// (original and optimised camera position), `node time x y z`, `con time sx sy sz tx ty tz`, `slice utime points`, `result ...`.
// With -m the mesh of <prefix>.ply goes the same way (mesh non-null): one `mesh utime vertices` line per span of MeshGenerator::collect
// ahead of the result line, the vertices through applyGraphToMesh under the same rule, and <prefix>_def.ply over the same triangles.
// With -mw the welded mesh (welded non-null, its span table the weld's) goes through applyGraphToMesh as well, into <prefix>_weld_def.ply.
// With -ms the simplified mesh (simplified non-null, its span table the simplification's) likewise, into <prefix>_simp_def.ply.
// With -mc the filtered mesh (filtered non-null, its span table the component pass's) likewise, into <prefix>_comp_def.ply.
// With -mh the filled mesh (holeFilled non-null, its span table the hole pass's) likewise, into <prefix>_fill_def.ply.
// With -mt the smoothed mesh (smoothed non-null, its span table its input's) likewise, into <prefix>_smooth_def.ply.
static bool deformMap(kt_ctx* ctx, KintinuousTracker* fe, const std::vector<LoopClosureConstraint>& constraints, const std::vector<char>& kept,
                      const std::vector<std::pair<uint64_t, kt::Matrix4f> >& optimised, float poseDist, double gate, CloudSliceProcessor& sliceProcessor, MeshGenerator::Mesh* mesh,
                      MeshGenerator::Mesh* welded, MeshGenerator::Mesh* filtered, MeshGenerator::Mesh* holeFilled, MeshGenerator::Mesh* smoothed, MeshGenerator::Mesh* simplified,
                      MeshWriter& writer, const std::string& prefix)
{
    FILE* f = 0;
    try {
        std::map<uint64_t, kt::Matrix4f> original, corrected;
        for (size_t i = 0; i < fe->densePoseGraph.size(); ++i)
            if (!original.count(fe->densePoseGraph[i].timestamp)) original[fe->densePoseGraph[i].timestamp] = fe->densePoseGraph[i].pose;
        std::vector<float> pos;
        std::vector<uint64_t> times;
        for (size_t i = 0; i < optimised.size(); ++i) {
            const uint64_t t = optimised[i].first;
            if (!original.count(t)) continue;
            corrected[t] = optimised[i].second;
            for (int a = 0; a < 3; ++a) pos.push_back(original[t](a, 3));
            times.push_back(t);
        }
        f = std::fopen((prefix + ".deform").c_str(), "w");
        if (!f) { std::fprintf(stderr, "cannot write %s.deform\n", prefix.c_str()); return false; }
        DeformationGraph graph(ctx);
        const int nodes = graph.initialiseGraphPoses(pos.data(), times.data(), times.size(), poseDist);
        int id = 0;
        for (size_t i = 0; i < times.size(); ++i) {
            const kt::Matrix4f& C = corrected[times[i]];
            const double target[3] = {(double)C(0, 3), (double)C(1, 3), (double)C(2, 3)};
            graph.addConstraint(id++, &pos[3 * i], times[i], target);
            std::fprintf(f, "pose %llu %a %a %a %a %a %a\n", (unsigned long long)times[i], (double)pos[3 * i], (double)pos[3 * i + 1], (double)pos[3 * i + 2], target[0],
                         target[1], target[2]);
        }
        for (size_t l = 0; l < constraints.size() && l < kept.size(); ++l) {
            if (!kept[l]) continue;
            for (int side = 0; side < 2; ++side) {
                const uint64_t t = side ? constraints[l].time2 : constraints[l].time1;
                const std::vector<LoopClosureVector3d>& pts = side ? constraints[l].inliers2Proj : constraints[l].inliers1Proj;
                if (!original.count(t) || !corrected.count(t)) continue;
                const kt::Matrix4f &O = original[t], &C = corrected[t];
                for (size_t j = 0; j < pts.size(); ++j) {
                    const double p[3] = {pts[j].x, pts[j].y, pts[j].z};
                    float src[3];
                    double target[3];
                    for (int r = 0; r < 3; ++r) {
                        src[r] = (float)((((double)O(r, 0) * p[0] + (double)O(r, 1) * p[1]) + (double)O(r, 2) * p[2]) + (double)O(r, 3));
                        target[r] = (((double)C(r, 0) * p[0] + (double)C(r, 1) * p[1]) + (double)C(r, 2) * p[2]) + (double)C(r, 3);
                    }
                    graph.addConstraint(id++, src, t, target);
                }
            }
        }
        const char* statusText[] = {"converged", "max-steps", "insignificant", "singular"};
        kt_deform_result r = {0.0, 0.0, 0.0, 0, KT_DEFORM_INSIGNIFICANT};
        if (graph.initialised()) {
            for (size_t i = 0; i < graph.getGraph().size(); ++i) {
                const GraphNode& g = graph.getGraph()[i];
                std::fprintf(f, "node %llu %a %a %a\n", (unsigned long long)g.time, g.position[0], g.position[1], g.position[2]);
            }
            kt_deform_params params = {gate, 1e-2, 1e-3, 1e-5, 10, 0};   // optimiseGraphSparse's, the gate by -ds
            r = graph.optimiseGraphSparse(&params);
        }
        for (size_t k = 0; k < graph.numConstraints(); ++k)
            std::fprintf(f, "con %llu %a %a %a %a %a %a\n", (unsigned long long)graph.constraintTimes()[k], (double)graph.constraintSources()[3 * k],
                         (double)graph.constraintSources()[3 * k + 1], (double)graph.constraintSources()[3 * k + 2], graph.constraintTargets()[3 * k],
                         graph.constraintTargets()[3 * k + 1], graph.constraintTargets()[3 * k + 2]);
        const bool apply = graph.initialised() && (r.status == KT_DEFORM_CONVERGED || r.status == KT_DEFORM_MAX_STEPS);
        ThreadDataPack& pack = ThreadDataPack::get();
        const int latest = pack.latestPoseId.getValue();
        for (int i = 1; i < latest; ++i) {
            CloudSlice* s = pack.cloudSlices.at(i);
            std::fprintf(f, "slice %llu %zu\n", (unsigned long long)s->utime, s->processedCloud->size());
            if (apply && s->processedCloud->size()) {
                const std::vector<uint64_t> t(s->processedCloud->size(), s->utime);
                graph.applyGraphToVertices(s->processedCloud->data(), t.data(), t.size());
            }
        }
        if (mesh) {
            for (size_t k = 0; k < mesh->spanTime.size(); ++k)
                std::fprintf(f, "mesh %llu %zu\n", (unsigned long long)mesh->spanTime[k], mesh->spanFirst[k + 1] - mesh->spanFirst[k]);
            if (apply && mesh->vertices.size())
                graph.applyGraphToMesh(mesh->vertices.data(), mesh->vertices.size(), mesh->spanFirst.data(), mesh->spanTime.data(), (int)mesh->spanTime.size());
        }
        if (welded && apply && welded->vertices.size())
            graph.applyGraphToMesh(welded->vertices.data(), welded->vertices.size(), welded->spanFirst.data(), welded->spanTime.data(), (int)welded->spanTime.size());
        if (filtered && apply && filtered->vertices.size())
            graph.applyGraphToMesh(filtered->vertices.data(), filtered->vertices.size(), filtered->spanFirst.data(), filtered->spanTime.data(), (int)filtered->spanTime.size());
        if (holeFilled && apply && holeFilled->vertices.size())
            graph.applyGraphToMesh(holeFilled->vertices.data(), holeFilled->vertices.size(), holeFilled->spanFirst.data(), holeFilled->spanTime.data(), (int)holeFilled->spanTime.size());
        if (smoothed && apply && smoothed->vertices.size())
            graph.applyGraphToMesh(smoothed->vertices.data(), smoothed->vertices.size(), smoothed->spanFirst.data(), smoothed->spanTime.data(), (int)smoothed->spanTime.size());
        if (simplified && apply && simplified->vertices.size())
            graph.applyGraphToMesh(simplified->vertices.data(), simplified->vertices.size(), simplified->spanFirst.data(), simplified->spanTime.data(),
                                   (int)simplified->spanTime.size());
        std::fprintf(f, "result %d %zu %s %d %a %a %a\n", nodes, graph.numConstraints(), statusText[r.status], r.steps, r.error_start, r.error_end, r.constraint_error);
        std::fclose(f);
        f = 0;
        if (sliceProcessor.save(prefix + "_def.pcd") < 0) { std::fprintf(stderr, "cannot write %s_def.pcd\n", prefix.c_str()); return false; }
        if (mesh) {
            const long long tris = writer.write(*mesh, prefix + "_def.ply");
            if (tris < 0) { std::fprintf(stderr, "cannot write %s_def.ply\n", prefix.c_str()); return false; }
            std::printf("mesh %s_def.ply: %lld triangles\n", prefix.c_str(), tris);
        }
        if (welded) {
            const long long tris = writer.write(*welded, prefix + "_weld_def.ply");
            if (tris < 0) { std::fprintf(stderr, "cannot write %s_weld_def.ply\n", prefix.c_str()); return false; }
            std::printf("mesh %s_weld_def.ply: %lld triangles\n", prefix.c_str(), tris);
        }
        if (filtered) {
            const long long tris = writer.write(*filtered, prefix + "_comp_def.ply");
            if (tris < 0) { std::fprintf(stderr, "cannot write %s_comp_def.ply\n", prefix.c_str()); return false; }
            std::printf("mesh %s_comp_def.ply: %lld triangles\n", prefix.c_str(), tris);
        }
        if (holeFilled) {
            const long long tris = writer.write(*holeFilled, prefix + "_fill_def.ply");
            if (tris < 0) { std::fprintf(stderr, "cannot write %s_fill_def.ply\n", prefix.c_str()); return false; }
            std::printf("mesh %s_fill_def.ply: %lld triangles\n", prefix.c_str(), tris);
        }
        if (smoothed) {
            const long long tris = writer.write(*smoothed, prefix + "_smooth_def.ply");
            if (tris < 0) { std::fprintf(stderr, "cannot write %s_smooth_def.ply\n", prefix.c_str()); return false; }
            std::printf("mesh %s_smooth_def.ply: %lld triangles\n", prefix.c_str(), tris);
        }
        if (simplified) {
            const long long tris = writer.write(*simplified, prefix + "_simp_def.ply");
            if (tris < 0) { std::fprintf(stderr, "cannot write %s_simp_def.ply\n", prefix.c_str()); return false; }
            std::printf("mesh %s_simp_def.ply: %lld triangles\n", prefix.c_str(), tris);
        }
        std::printf("deformation %s_def.pcd: %d nodes%s, %zu constraints, status %s, steps %d, error %g -> %g\n", prefix.c_str(), nodes,
                    graph.initialised() ? "" : " (fewer than 5: not deformed)", graph.numConstraints(), statusText[r.status], r.steps, r.error_start, r.error_end);
        return true;
    } catch (const std::exception& e) {
        if (f) std::fclose(f);
        std::fprintf(stderr, "-df: %s\n", e.what());
        return false;
    }
}

// -mw: the -m mesh with the vertices that share a voxel-edge key merged (MeshGenerator::weld, on a context of its own) as
// <prefix>_weld.ply, and <prefix>.weld: one `span utime first_in first_out` line per span of the mesh and `result n_in n_out triangles`.
// gapSeconds < 0: no gate; otherwise slabs whose times (microseconds) differ by more stay apart.
static bool weldMesh(int gpu, const MeshGenerator::Mesh& mesh, double gapSeconds, MeshGenerator::Mesh& welded, MeshWriter& writer, const std::string& prefix)
{
    kt_ctx* wctx = 0;
    if (kt_ctx_create(gpu, &wctx) != KT_OK) { std::fprintf(stderr, "-mw: %s\n", kt_last_error()); return false; }
    welded = mesh;
    const uint64_t gap = gapSeconds < 0.0 ? UINT64_MAX : (uint64_t)(gapSeconds * 1e6);
    const bool ok = MeshGenerator::weld(wctx, welded, gap);
    kt_ctx_destroy(wctx);
    if (!ok) { std::fprintf(stderr, "cannot weld %s.ply\n", prefix.c_str()); return false; }
    const long long tris = writer.write(welded, prefix + "_weld.ply");
    FILE* f = tris < 0 ? 0 : std::fopen((prefix + ".weld").c_str(), "w");
    if (!f) { std::fprintf(stderr, "cannot write %s_weld.ply / %s.weld\n", prefix.c_str(), prefix.c_str()); return false; }
    for (size_t s = 0; s < mesh.spanTime.size(); ++s)
        std::fprintf(f, "span %llu %zu %zu\n", (unsigned long long)mesh.spanTime[s], mesh.spanFirst[s], welded.spanFirst[s]);
    std::fprintf(f, "result %zu %zu %lld\n", mesh.vertices.size(), welded.vertices.size(), tris);
    std::fclose(f);
    std::printf("mesh %s_weld.ply: %zu of %zu vertices, %lld triangles\n", prefix.c_str(), welded.vertices.size(), mesh.vertices.size(), tris);
    return true;
}

// -mc: the mesh (the welded one with -mw) without its connected components of fewer than minTriangles triangles
// (MeshGenerator::dropSmallComponents, on a context of its own) as <prefix>_comp.ply, and <prefix>.comp: one `span utime first_in first_out`
// line per span of the mesh and `result n_in n_out m_in m_out components kept largest`.
static bool componentsMesh(int gpu, const MeshGenerator::Mesh& mesh, uint32_t minTriangles, MeshGenerator::Mesh& filtered, MeshWriter& writer, const std::string& prefix)
{
    kt_ctx* cctx = 0;
    if (kt_ctx_create(gpu, &cctx) != KT_OK) { std::fprintf(stderr, "-mc: %s\n", kt_last_error()); return false; }
    filtered = mesh;
    kt_mesh_component_stats stats = {0, 0, 0};
    const bool ok = MeshGenerator::dropSmallComponents(cctx, filtered, minTriangles, stats);
    kt_ctx_destroy(cctx);
    if (!ok) { std::fprintf(stderr, "cannot filter the components of the mesh of %s\n", prefix.c_str()); return false; }
    const long long tris = writer.write(filtered, prefix + "_comp.ply");
    FILE* f = tris < 0 ? 0 : std::fopen((prefix + ".comp").c_str(), "w");
    if (!f) { std::fprintf(stderr, "cannot write %s_comp.ply / %s.comp\n", prefix.c_str(), prefix.c_str()); return false; }
    for (size_t s = 0; s < mesh.spanTime.size(); ++s)
        std::fprintf(f, "span %llu %zu %zu\n", (unsigned long long)mesh.spanTime[s], mesh.spanFirst[s], filtered.spanFirst[s]);
    std::fprintf(f, "result %zu %zu %zu %lld %llu %llu %llu\n", mesh.vertices.size(), filtered.vertices.size(), mesh.triangles.size() / 3, tris,
                 (unsigned long long)stats.components, (unsigned long long)stats.kept_components, (unsigned long long)stats.largest);
    std::fclose(f);
    std::printf("mesh %s_comp.ply: %zu of %zu vertices, %lld of %zu triangles, %llu of %llu components of at least %u triangles, the largest of %llu\n", prefix.c_str(),
                filtered.vertices.size(), mesh.vertices.size(), tris, mesh.triangles.size() / 3, (unsigned long long)stats.kept_components,
                (unsigned long long)stats.components, minTriangles, (unsigned long long)stats.largest);
    return true;
}

// -mh: the open boundaries of the mesh (the filtered one with -mc, else the welded one with -mw) in <prefix>.holes, and with maxEdges > 0 the
// mesh with its simple loops of at most maxEdges edges closed by a fan each (MeshGenerator::fillSmallHoles, on a context of its own) as
// <prefix>_fill.ply.  <prefix>.holes: one `span utime first_in first_out` line per span of the mesh, one `loop label edges filled` line per
// simple loop, ascending by label, made here from the pass's loop_out and fill triangles, and `result n_in n_out m_in m_out` with the nine stats in the order of
// kt_mesh_hole_stats.  Returns false on failure; wrote: whether _fill.ply exists
static bool holesMesh(int gpu, const MeshGenerator::Mesh& mesh, uint32_t maxEdges, MeshGenerator::Mesh& filled, bool& wrote, MeshWriter& writer, const std::string& prefix)
{
    wrote = false;
    kt_ctx* hctx = 0;
    if (kt_ctx_create(gpu, &hctx) != KT_OK) { std::fprintf(stderr, "-mh: %s\n", kt_last_error()); return false; }
    filled = mesh;
    kt_mesh_hole_stats st = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> loopOut;
    const bool ok = MeshGenerator::fillSmallHoles(hctx, filled, maxEdges, st, &loopOut);
    kt_ctx_destroy(hctx);
    if (!ok) { std::fprintf(stderr, "cannot find the boundaries of the mesh of %s\n", prefix.c_str()); return false; }
    long long tris = (long long)(filled.triangles.size() / 3);
    if (maxEdges > 0) tris = writer.write(filled, prefix + "_fill.ply");
    FILE* f = tris < 0 ? 0 : std::fopen((prefix + ".holes").c_str(), "w");
    if (!f) { std::fprintf(stderr, "cannot write %s_fill.ply / %s.holes\n", prefix.c_str(), prefix.c_str()); return false; }
    for (size_t s = 0; s < mesh.spanTime.size(); ++s)
        std::fprintf(f, "span %llu %zu %zu\n", (unsigned long long)mesh.spanTime[s], mesh.spanFirst[s], filled.spanFirst[s]);
    // a loop's vertices carry its label, the smallest of them: edges[label] = their number.  Whether a loop was filled is read off the
    // pass's own output, so the fill rule is stated nowhere here: a fill triangle (behind the input's) is (b, a, centre) with a on the loop,
    // and input vertex v of span s sits at v + (first_out[s] - first_in[s])
    const size_t nIn = mesh.vertices.size(), mIn = mesh.triangles.size() / 3;
    std::vector<uint32_t> edges(nIn, 0), inputOf(filled.vertices.size(), 0xffffffffu);
    std::vector<char> wasFilled(nIn, 0);
    for (size_t v = 0; v < loopOut.size(); ++v)
        if (loopOut[v] < 0xfffffffeu) edges[loopOut[v]] += 1;
    for (size_t s = 0; s < mesh.spanTime.size(); ++s)
        for (size_t v = mesh.spanFirst[s]; v < mesh.spanFirst[s + 1]; ++v) inputOf[v + (filled.spanFirst[s] - mesh.spanFirst[s])] = (uint32_t)v;
    for (size_t t = mIn; t < filled.triangles.size() / 3; ++t) wasFilled[loopOut[inputOf[filled.triangles[3 * t + 1]]]] = 1;
    for (size_t l = 0; l < edges.size(); ++l)
        if (edges[l]) std::fprintf(f, "loop %zu %u %d\n", l, edges[l], (int)wasFilled[l]);
    std::fprintf(f, "result %zu %zu %zu %lld %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", mesh.vertices.size(), filled.vertices.size(), mesh.triangles.size() / 3, tris,
                 (unsigned long long)st.boundary_edges, (unsigned long long)st.nonmanifold_edges, (unsigned long long)st.degenerate_triangles, (unsigned long long)st.loops,
                 (unsigned long long)st.open_components, (unsigned long long)st.filled, (unsigned long long)st.longest, (unsigned long long)st.new_vertices,
                 (unsigned long long)st.new_triangles);
    std::fclose(f);
    wrote = maxEdges > 0;
    std::printf("mesh %s%s: %llu boundary edges in %llu loops (the longest of %llu) and %llu open components, %llu non-manifold edges; %llu loops of at most %u edges filled, "
                "%zu vertices, %lld triangles\n", prefix.c_str(), wrote ? "_fill.ply" : ".holes", (unsigned long long)st.boundary_edges, (unsigned long long)st.loops,
                (unsigned long long)st.longest, (unsigned long long)st.open_components, (unsigned long long)st.nonmanifold_edges, (unsigned long long)st.filled, maxEdges,
                filled.vertices.size(), tris);
    return true;
}

// -mt: the newest mesh that exists (the filled one with -mh, else the filtered one with -mc, else the welded one with -mw, else the collected
// one) with its vertex positions smoothed by `steps` steps of Taubin's lambda|mu filter at lambda = 0.5, mu = -0.53 (MeshGenerator::smooth,
// on a context of its own) as <prefix>_smooth.ply, and <prefix>.smooth: `result n m steps lambda mu mode rim moved edges`, the factors as
// hex floats, the last three kt_mesh_smooth_stats.  mode 0 pins the rims, mode 1 (-mtb) moves them along the rim.
static bool smoothMesh(int gpu, const MeshGenerator::Mesh& mesh, int steps, int mode, MeshGenerator::Mesh& smoothed, MeshWriter& writer, const std::string& prefix)
{
    const float lambda = 0.5f, mu = -0.53f;
    kt_ctx* tctx = 0;
    if (kt_ctx_create(gpu, &tctx) != KT_OK) { std::fprintf(stderr, "-mt: %s\n", kt_last_error()); return false; }
    smoothed = mesh;
    kt_mesh_smooth_stats st = {0, 0, 0};
    const bool ok = MeshGenerator::smooth(tctx, smoothed, steps, lambda, mu, mode, st);
    kt_ctx_destroy(tctx);
    if (!ok) { std::fprintf(stderr, "cannot smooth the mesh of %s\n", prefix.c_str()); return false; }
    const long long tris = writer.write(smoothed, prefix + "_smooth.ply");
    FILE* f = tris < 0 ? 0 : std::fopen((prefix + ".smooth").c_str(), "w");
    if (!f) { std::fprintf(stderr, "cannot write %s_smooth.ply / %s.smooth\n", prefix.c_str(), prefix.c_str()); return false; }
    std::fprintf(f, "result %zu %lld %d %a %a %d %llu %llu %llu\n", smoothed.vertices.size(), tris, steps, (double)lambda, (double)mu, mode, (unsigned long long)st.rim_vertices,
                 (unsigned long long)st.moved_vertices, (unsigned long long)st.unique_edges);
    std::fclose(f);
    std::printf("mesh %s_smooth.ply: %d steps, %llu of %zu vertices moved over %llu edges, %llu rim vertices %s, %lld triangles\n", prefix.c_str(), steps,
                (unsigned long long)st.moved_vertices, smoothed.vertices.size(), (unsigned long long)st.unique_edges, (unsigned long long)st.rim_vertices,
                mode ? "moved along the rim" : "pinned", tris);
    return true;
}

// -ms: the mesh (the smoothed one with -mt, else the filled one with -mh, else the filtered one with -mc, else the welded one with -mw) coarsened by vertex clustering at a cell of `cell` metres (MeshGenerator::simplify, on a
// context of its own) as <prefix>_simp.ply, and <prefix>.simp: one `span utime first_in first_out` line per span of the mesh and
// `result n_in n_out m_in m_out cell`.  With -msq (quadric) the merged vertices come from the quadric form at `bias`, and a last line
// `quadric bias placed clusters` follows: how many of the clusters of more than one member sit at their quadrics' minimiser.
static bool simplifyMesh(int gpu, const MeshGenerator::Mesh& mesh, float cell, bool quadric, float bias, MeshGenerator::Mesh& simplified, MeshWriter& writer,
                         const std::string& prefix)
{
    kt_ctx* sctx = 0;
    if (kt_ctx_create(gpu, &sctx) != KT_OK) { std::fprintf(stderr, "-ms: %s\n", kt_last_error()); return false; }
    simplified = mesh;
    size_t placed = 0;
    const bool ok = quadric ? MeshGenerator::simplify(sctx, simplified, cell, bias, placed) : MeshGenerator::simplify(sctx, simplified, cell);
    kt_ctx_destroy(sctx);
    if (!ok) { std::fprintf(stderr, "cannot simplify the mesh of %s\n", prefix.c_str()); return false; }
    const long long tris = writer.write(simplified, prefix + "_simp.ply");
    FILE* f = tris < 0 ? 0 : std::fopen((prefix + ".simp").c_str(), "w");
    if (!f) { std::fprintf(stderr, "cannot write %s_simp.ply / %s.simp\n", prefix.c_str(), prefix.c_str()); return false; }
    for (size_t s = 0; s < mesh.spanTime.size(); ++s)
        std::fprintf(f, "span %llu %zu %zu\n", (unsigned long long)mesh.spanTime[s], mesh.spanFirst[s], simplified.spanFirst[s]);
    std::fprintf(f, "result %zu %zu %zu %lld %a\n", mesh.vertices.size(), simplified.vertices.size(), mesh.triangles.size() / 3, tris, (double)cell);
    size_t merged = 0;   // the clusters of more than one member: those the quadric form can place
    if (quadric) {
        merged = MeshGenerator::mergedClusters(mesh, cell);
        std::fprintf(f, "quadric %a %zu %zu\n", (double)bias, placed, merged);
    }
    std::fclose(f);
    if (quadric) std::printf("mesh %s_simp.ply: %zu of %zu merged vertices at their quadrics' minimiser (bias %g)\n", prefix.c_str(), placed, merged, (double)bias);
    std::printf("mesh %s_simp.ply: %zu of %zu vertices, %lld of %zu triangles\n", prefix.c_str(), simplified.vertices.size(), mesh.vertices.size(), tris,
                mesh.triangles.size() / 3);
    return true;
}

// -mv: `mesh`, which the run wrote as <prefix><stem>.ply, rendered from `pose` (a dense pose: [R | camera centre], in the frame of the mesh's
// vertices) moved `back` metres against its viewing axis, at the run's resolution and intrinsics with near = 0.05 m (MeshGenerator::render,
// on a context of its own): <prefix><stem>_view_depth.pgm (16-bit big-endian millimetres, as -ppm's), _view_color.ppm, _view_model.ppm, and
// <prefix><viewStem>.view, one `name value` line each: the file viewed, the frame, the number of dense poses, back and near, R (row-major)
// and t as hex floats, and the four kt_mesh_render_stats.
static bool viewMesh(int gpu, const MeshGenerator::Mesh& mesh, const Intr& intr, const kt::Matrix4f& pose, long long frame, size_t poses, float back, const std::string& prefix,
                     const std::string& stem, const std::string& viewStem)
{
    const float near = 0.05f;
    float R[9], t[3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = pose(r, c);
    for (int r = 0; r < 3; ++r) t[r] = pose(r, 3) - back * R[3 * r + 2];
    const kt_intr k = {intr.fx, intr.fy, intr.cx, intr.cy};
    const int cols = Resolution::get().cols(), rows = Resolution::get().rows();
    kt_ctx* vctx = 0;
    if (kt_ctx_create(gpu, &vctx) != KT_OK) { std::fprintf(stderr, "-mv: %s\n", kt_last_error()); return false; }
    MeshGenerator::View view;
    const bool ok = MeshGenerator::render(vctx, mesh, k, cols, rows, R, t, near, view);
    kt_ctx_destroy(vctx);
    if (!ok) { std::fprintf(stderr, "cannot render the mesh of %s%s.ply\n", prefix.c_str(), stem.c_str()); return false; }
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

int main(int argc, char** argv)
{
    const ConfigArgs& args = ConfigArgs::get(argc, argv);
    if (args.help || args.logFile.empty()) { ConfigArgs::usage(argv[0]); return args.help ? 0 : 1; }
    bool ops = false, pcd = false, pcdraw = false, ppm = false, noStage = false, loops = false, poseGraph = false, deform = false, weld = false;
    float simplifyCell = 0.0f;  // -ms: metres; the edge of the clustering cells (absent: no simplification)
    bool simplify = false;
    bool quadric = false, quadricBiasGiven = false;   // -msq: the merged vertices at their quadrics' minimiser; -msb: the pull towards the mean
    float quadricBias = 0.015625f;
    bool components = false;    // -mc: the connected pieces of fewer than minComponent triangles leave the mesh
    long long minComponent = 0;
    bool holes = false;         // -mh: the boundaries of the mesh are reported, its loops of at most holeEdges edges closed
    long long holeEdges = 0;
    bool smooth = false, smoothRim = false;   // -mt: the mesh is smoothed with smoothSteps steps; -mtb: its rim vertices move along the rim
    long long smoothSteps = 0;
    bool view = false;          // -mv: the last mesh of the chain is rendered from dense pose viewFrame (-mvf; -1: the last), viewBack metres back (-mvb)
    long long viewFrame = -1;
    bool viewFrameGiven = false;
    float viewBack = 0.0f;
    bool normals = false;       // -mn: every .ply carries vertex normals
    double weldGap = -1.0;      // -mwg: seconds; slabs whose times lie further apart are not welded (default: no gate)
    float poseDist = 0.8f;      // -dg: the deformation graph's node spacing (the reference's default)
    double deformGate = 0.1;    // -ds: the constraint error below which nothing is deformed (the reference's 0.1)
    double isamThresh = 10.0;   // -it (ConfigArgs.h:127 of the reference): a loop stays when chi2 < isamThresh
    int rank = 0, world = 0, gatherCount = 1, loopDislocal = -1, loopConsistency = -1;
    std::string commFile;
    for (int i = 1; i < argc; ++i) {
        ops = ops || std::string(argv[i]) == "-ops";
        pcd = pcd || std::string(argv[i]) == "-pcd";
        pcdraw = pcdraw || std::string(argv[i]) == "-pcdraw";
        noStage = noStage || std::string(argv[i]) == "-nostage";   // debug: the slice processor thread calls kt_slice_process itself
        ppm = ppm || std::string(argv[i]) == "-ppm";
        loops = loops || std::string(argv[i]) == "-lc";
        poseGraph = poseGraph || std::string(argv[i]) == "-pg";
        deform = deform || std::string(argv[i]) == "-df";
        weld = weld || std::string(argv[i]) == "-mw";
        normals = normals || std::string(argv[i]) == "-mn";
        if (i + 1 < argc && std::string(argv[i]) == "-mwg") weldGap = std::atof(argv[i + 1]);
        if (i + 1 < argc && std::string(argv[i]) == "-ms") { simplify = true; simplifyCell = (float)std::atof(argv[i + 1]); }
        quadric = quadric || std::string(argv[i]) == "-msq";
        if (i + 1 < argc && std::string(argv[i]) == "-msb") { quadricBiasGiven = true; quadricBias = (float)std::atof(argv[i + 1]); }
        if (i + 1 < argc && std::string(argv[i]) == "-mc") { components = true; minComponent = std::atoll(argv[i + 1]); }
        if (i + 1 < argc && std::string(argv[i]) == "-mh") { holes = true; holeEdges = std::atoll(argv[i + 1]); }
        if (i + 1 < argc && std::string(argv[i]) == "-mt") { smooth = true; smoothSteps = std::atoll(argv[i + 1]); }
        smoothRim = smoothRim || std::string(argv[i]) == "-mtb";
        view = view || std::string(argv[i]) == "-mv";
        if (i + 1 < argc && std::string(argv[i]) == "-mvf") { viewFrameGiven = true; viewFrame = std::atoll(argv[i + 1]); }
        if (i + 1 < argc && std::string(argv[i]) == "-mvb") viewBack = (float)std::atof(argv[i + 1]);
        if (i + 1 < argc && std::string(argv[i]) == "-dg") poseDist = (float)std::atof(argv[i + 1]);
        if (i + 1 < argc && std::string(argv[i]) == "-ds") deformGate = std::atof(argv[i + 1]);
        if (i + 1 < argc && std::string(argv[i]) == "-it") isamThresh = std::atof(argv[i + 1]);
        if (i + 1 < argc && std::string(argv[i]) == "-rank") rank = std::atoi(argv[i + 1]);
        if (i + 1 < argc && std::string(argv[i]) == "-world") world = std::atoi(argv[i + 1]);
        if (i + 1 < argc && std::string(argv[i]) == "-comm") commFile = argv[i + 1];
        if (i + 1 < argc && std::string(argv[i]) == "-gk") gatherCount = std::atoi(argv[i + 1]);
        if (i + 1 < argc && std::string(argv[i]) == "-dl") loopDislocal = std::atoi(argv[i + 1]);      // -lc: as loop_tool -all's
        if (i + 1 < argc && std::string(argv[i]) == "-k") loopConsistency = std::atoi(argv[i + 1]);
    }

    Resolution::get(args.width, args.height);
    Volume::get(args.volumeSize, args.volumeResolution);
    const Intr intr = loadCalibration(args.calibrationFile, args.width, args.height);

    // -gj: the reader defers JPEG colour only for a consumer that makes the pixels: the device-resident tracker's frame slots
    if (args.gpuJpeg && ops) std::fprintf(stderr, "-gj ignored with -ops (the operator path takes host frames)\n");
    RawLogReader log(args.logFile, args.decodeThreads, args.gpuJpeg && !ops);
    TrackerInterface tracker(&log, intr, ops);
    if (args.extractOverlap) tracker.enableOverlap();  // MainController.cpp:187-190

    // -pcd: the backend's first thread runs next to the tracker, as in MainController (CloudSliceProcessor.cpp): it takes every slice
    // at the moment the tracker hands it over and fills its processedCloud on the GPU, on a context and stream of its own
    ThreadDataPack& pack = ThreadDataPack::get();
    pack.assignFrontend(tracker.getFrontend());
    // the slice stage itself runs on the device behind every extraction (the operator path hands raw slices to the processor instead)
    if (pcd && !ops && !noStage) tracker.getFrontend()->enableSliceStage(args.weightCull);
    // -m: the mesh stage behind every slab (MainController.cpp:113-116 starts the reference's MeshGenerator thread here)
    if (args.generateMesh && !ops) tracker.getFrontend()->enableMeshStage();
    if (args.generateMesh && ops) std::fprintf(stderr, "-m ignored with -ops (the mesh stage runs on the device-resident path)\n");
    if (weld && !(args.generateMesh && !ops)) {
        std::fprintf(stderr, "-mw ignored without -m (it welds the seams of the -m mesh)\n");
        weld = false;
    }
    if (weld) tracker.getFrontend()->enableMeshKeys();
    if (simplify && !(args.generateMesh && !ops)) {
        std::fprintf(stderr, "-ms ignored without -m (it simplifies the -m mesh)\n");
        simplify = false;
    }
    if (quadric && !simplify) {
        std::fprintf(stderr, "-msq ignored without -ms (it places the vertices that -ms merges)\n");
        quadric = false;
    }
    if (quadricBiasGiven && !simplify) std::fprintf(stderr, "-msb ignored without -ms (it is the bias of -ms -msq)\n");
    else if (quadricBiasGiven && !quadric) std::fprintf(stderr, "-msb ignored without -msq (it is the bias of -ms -msq)\n");
    if (components && !(args.generateMesh && !ops)) {
        std::fprintf(stderr, "-mc ignored without -m (it drops the small pieces of the -m mesh)\n");
        components = false;
    }
    if (components && (minComponent < 1 || minComponent > 0xffffffffll)) {
        std::fprintf(stderr, "-mc ignored: it takes a number of triangles from 1 to 2^32 - 1\n");
        components = false;
    }
    if (holes && !(args.generateMesh && !ops)) {
        std::fprintf(stderr, "-mh ignored without -m (it reports the boundaries of the -m mesh and fills its small holes)\n");
        holes = false;
    }
    if (holes && (holeEdges < 0 || holeEdges > 256)) {
        std::fprintf(stderr, "-mh ignored: it takes a number of edges from 0 to 256\n");
        holes = false;
    }
    if (holes && !weld) std::fprintf(stderr, "-mh without -mw: every slab seam will show as a boundary\n");
    if (smooth && !(args.generateMesh && !ops)) {
        std::fprintf(stderr, "-mt ignored without -m (it smooths the -m mesh)\n");
        smooth = false;
    }
    if (smooth && (smoothSteps < 0 || smoothSteps > 64)) {
        std::fprintf(stderr, "-mt ignored: it takes a number of steps from 0 to 64\n");
        smooth = false;
    }
    if (smoothRim && !smooth) {
        std::fprintf(stderr, "-mtb ignored without -mt (it lets the rims of the smoothed mesh move)\n");
        smoothRim = false;
    }
    if (view && !(args.generateMesh && !ops)) {
        std::fprintf(stderr, "-mv ignored without -m (it renders the -m mesh)\n");
        view = false;
    }
    if ((viewFrameGiven || viewBack != 0.0f) && !view) std::fprintf(stderr, "-mvf and -mvb ignored without -mv (they place its camera)\n");
    if (view && viewFrameGiven && viewFrame < 0) {   // (the upper end is known only once the log has been tracked)
        std::fprintf(stderr, "-mvf takes the index of a dense pose, from 0\n");
        return 1;
    }
    if (view && !(std::fabs(viewBack) < 8192.0f)) {
        std::fprintf(stderr, "-mvb takes a distance in metres below 8192\n");
        return 1;
    }
    if (normals && !(args.generateMesh && !ops)) {
        std::fprintf(stderr, "-mn ignored without -m (it gives the -m mesh vertex normals)\n");
        normals = false;
    }
    MeshWriter writer = {normals, args.gpu, args.saveFile + ".normals", false, false};
    CloudSliceProcessor sliceProcessor;
    pack.limit.assignValue(false);   // the GUI's 30 Hz throttle (ThreadDataPack::limit) off: play the log as fast as it tracks
    // Components run as in MainController::mainLoop (MainController.cpp:142-150): ThreadObject::start on a thread each.  Without -pcd no
    // slice processor runs; it is then marked finished up front, the way MainController::setup marks absent components (:121-141), so
    // that the tracker's end-of-log hand-shake (TrackerInterface.cpp:66-69) has nothing to wait for.
    std::thread sliceThread;
    if (pcd) sliceThread = std::thread(&ThreadObject::start, static_cast<ThreadObject*>(&sliceProcessor));
    else pack.cloudSliceProcessorFinished.assignValue(true);

    const auto t0 = std::chrono::steady_clock::now();
    std::thread trackerThread(&ThreadObject::start, static_cast<ThreadObject*>(&tracker));
    trackerThread.join();
    const int frames = tracker.getCurrentFrame();
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    pack.trackerFinished.assignValue(true);
    if (pcd) sliceThread.join();   // the slices are the processor's until it has ended (it rewrites slice->cloud in place)

    KintinuousTracker* fe = tracker.getFrontend();
    // -pcdraw is the extraction as the tracker produced it: only meaningful without -pcd, whose processor down-samples slice->cloud in place
    if (pcdraw && !pcd && !writeRawPcd(args.saveFile + ".raw.pcd", fe->getCloudSlices())) std::fprintf(stderr, "cannot write %s.raw.pcd\n", args.saveFile.c_str());
    if (pcdraw && pcd) std::fprintf(stderr, "-pcdraw ignored with -pcd (the slice processor rewrites the slices in place)\n");
    size_t points = 0;   // with -pcd: the down-sampled slices (the processor has ended); without: the raw extraction
    for (size_t i = 0; i < fe->getCloudSlices().size(); ++i) points += fe->getCloudSlices()[i]->cloud->size();
    if (pcd && (!pack.cloudSliceProcessorFinished.getValue() || sliceProcessor.save() < 0)) std::fprintf(stderr, "cannot write %s.pcd\n", args.saveFile.c_str());
    if (ppm) writeViews(fe, args.saveFile);
    MeshGenerator::Mesh mesh;   // kept for -df, which deforms its vertices into <prefix>_def.ply
    bool haveMesh = false;
    if (args.generateMesh && !ops) {   // MainController.cpp:247-249: meshGenerator->save()
        haveMesh = MeshGenerator::collect(fe->handle(), mesh);
        const long long tris = haveMesh ? writer.write(mesh, args.saveFile + ".ply") : -1;
        if (tris < 0) { std::fprintf(stderr, "cannot write %s.ply\n", args.saveFile.c_str()); haveMesh = false; }
        else std::printf("mesh %s.ply: %lld triangles\n", args.saveFile.c_str(), tris);
    }
    MeshGenerator::Mesh welded;   // -mw: the same mesh with its slab seams welded, <prefix>_weld.ply; -df deforms it too
    bool haveWelded = false;
    if (weld && haveMesh) haveWelded = weldMesh(args.gpu, mesh, weldGap, welded, writer, args.saveFile);
    MeshGenerator::Mesh filtered;   // -mc: the welded mesh (with -mw) or the collected one without its small pieces, <prefix>_comp.ply; -df deforms it too
    bool haveFiltered = false;
    if (components && haveMesh && (haveWelded || !weld)) haveFiltered = componentsMesh(args.gpu, haveWelded ? welded : mesh, (uint32_t)minComponent, filtered, writer, args.saveFile);
    MeshGenerator::Mesh holeFilled;   // -mh: the filtered mesh (with -mc), else the welded one (with -mw), else the collected one, its small holes closed, <prefix>_fill.ply; -df deforms it too
    bool haveHoles = false, haveHoleFilled = false;   // the pass ran; it wrote _fill.ply (-mh 0 only reports)
    if (holes && haveMesh && (haveWelded || !weld) && (haveFiltered || !components))
        haveHoles = holesMesh(args.gpu, haveFiltered ? filtered : haveWelded ? welded : mesh, (uint32_t)holeEdges, holeFilled, haveHoleFilled, writer, args.saveFile);
    MeshGenerator::Mesh smoothed;   // -mt: the newest of the meshes above, its vertex positions smoothed, <prefix>_smooth.ply; -df deforms it too
    bool haveSmoothed = false, smoothFailed = false;
    if (smooth && haveMesh && (haveWelded || !weld) && (haveFiltered || !components) && (haveHoles || !holes)) {
        haveSmoothed = smoothMesh(args.gpu, haveHoleFilled ? holeFilled : haveFiltered ? filtered : haveWelded ? welded : mesh, (int)smoothSteps, smoothRim ? 1 : 0, smoothed, writer,
                                  args.saveFile);
        smoothFailed = !haveSmoothed;
    }
    MeshGenerator::Mesh simplified;   // -ms: the smoothed mesh (with -mt), else the filled mesh (with -mh), else the filtered mesh (with -mc), else the welded one (with -mw), else the collected one, coarsened, <prefix>_simp.ply; -df deforms it too
    bool haveSimplified = false;
    if (simplify && haveMesh && (haveWelded || !weld) && (haveFiltered || !components) && (haveHoles || !holes) && (haveSmoothed || !smooth))
        haveSimplified = simplifyMesh(args.gpu, haveSmoothed ? smoothed : haveHoleFilled ? holeFilled : haveFiltered ? filtered : haveWelded ? welded : mesh, simplifyCell, quadric, quadricBias, simplified, writer, args.saveFile);
    // -mv: the mesh the run wrote last, from a dense pose (whose frame is the vertices': the deformation's nodes are these positions)
    MeshGenerator::Mesh* viewed = haveSimplified ? &simplified : haveSmoothed ? &smoothed : haveHoleFilled ? &holeFilled : haveFiltered ? &filtered : haveWelded ? &welded : haveMesh ? &mesh : 0;
    const std::string viewStem = haveSimplified ? "_simp" : haveSmoothed ? "_smooth" : haveHoleFilled ? "_fill" : haveFiltered ? "_comp" : haveWelded ? "_weld" : "";
    bool viewFailed = false, haveView = false;
    if (view && viewed) {
        const size_t poses = fe->densePoseGraph.size();
        if (!viewFrameGiven) viewFrame = (long long)poses - 1;
        if (viewFrame < 0 || (size_t)viewFrame >= poses) {
            std::fprintf(stderr, "-mvf %lld: the run has %zu dense poses; no view was written\n", viewFrame, poses);
            viewFailed = true;
        } else {
            haveView = viewMesh(args.gpu, *viewed, intr, fe->densePoseGraph[(size_t)viewFrame].pose, viewFrame, poses, viewBack, args.saveFile, viewStem, "");
            viewFailed = !haveView;
        }
    }
    if (args.vocabFile.size()) {   // the place-recognition tap's samples as stored (-v): count and a checksum over their bytes
        unsigned long crc = crc32(0L, Z_NULL, 0);
        const int samples = fe->placeRecognitionId.getValue();
        for (int i = 0; i < samples; ++i) {
            const PlaceRecognitionInput& s = fe->placeRecognitionBuffer[i];
            crc = crc32(crc, reinterpret_cast<const Bytef*>(s.rgbImage), (uInt)s.imageSize);
            crc = crc32(crc, reinterpret_cast<const Bytef*>(s.depthMap), (uInt)s.depthSize);
            const unsigned char flags[2] = {(unsigned char)s.isCompressed, (unsigned char)s.imageIsRaw};
            crc = crc32(crc, flags, 2);
        }
        std::printf("place recognition samples %d  crc %08lx\n", samples, crc);
    }
    if (poseGraph && !(loops && args.vocabFile.size())) std::fprintf(stderr, "-pg ignored without -v <vocab> -lc (it optimises over the accepted loop constraints)\n");
    if (deform && !(poseGraph && loops && args.vocabFile.size() && pcd)) {
        std::fprintf(stderr, "-df ignored without -v <vocab> -lc -pg -pcd (it deforms the saved map onto the optimised trajectory)\n");
        deform = false;
    }
    if (loops && args.vocabFile.empty()) std::fprintf(stderr, "-lc ignored without -v (the place-recognition tap takes the samples)\n");
    if (loops && args.vocabFile.size()) {   // PlaceRecognition over the tap's samples, on a context of its own: <prefix>.loops
        kt_ctx* lctx = 0;
        if (kt_ctx_create(args.gpu, &lctx) != KT_OK) { std::fprintf(stderr, "-lc: %s\n", kt_last_error()); return 1; }
        bool ok;
        size_t accepted = 0;
        {
            const kt_intr li = {intr.fx, intr.fy, intr.cx, intr.cy};
            const int samples = fe->placeRecognitionId.getValue();
            kt_loop_db_detect_params dp;
            kt_loop_db_detect_params_default(&dp);
            if (loopDislocal >= 0) dp.dislocal = loopDislocal;
            if (loopConsistency >= 0) dp.consistency = loopConsistency;
            PlaceRecognition pr(lctx, li, Volume::get().getVoxelSizeMeters().x, &dp, samples > 1000 ? samples : 1000);
            ok = pr.process(fe->placeRecognitionBuffer, samples) && pr.saveLoops(args.saveFile + ".loops");
            accepted = pr.constraints.size();
            for (size_t i = 0; i < pr.samples.size(); ++i)
                std::printf("loop sample %zu; time %llu; status %s; candidate %d\n", i, (unsigned long long)fe->placeRecognitionBuffer[i].utime,
                            placeRecognitionStatusText(pr.samples[i].detection.status), pr.samples[i].detection.candidate);
            std::vector<char> kept;
            std::vector<std::pair<uint64_t, kt::Matrix4f> > optimised;
            if (ok && poseGraph && !optimisePoseGraph(lctx, fe, pr.constraints, isamThresh, args.saveFile, kept, optimised)) { kt_ctx_destroy(lctx); return 1; }
            if (ok && poseGraph && deform && !deformMap(lctx, fe, pr.constraints, kept, optimised, poseDist, deformGate, sliceProcessor, haveMesh ? &mesh : 0, haveWelded ? &welded : 0, haveFiltered ? &filtered : 0, haveHoleFilled ? &holeFilled : 0, haveSmoothed ? &smoothed : 0, haveSimplified ? &simplified : 0, writer, args.saveFile)) { kt_ctx_destroy(lctx); return 1; }
            if (ok && poseGraph && deform && haveView) {   // -mv with -df: the deformed twin (deformMap moved the vertices in place) from the optimised pose of the same frame
                const uint64_t stamp = fe->densePoseGraph[(size_t)viewFrame].timestamp;
                size_t at = optimised.size();
                for (size_t i = 0; i < optimised.size() && at == optimised.size(); ++i)
                    if (optimised[i].first == stamp) at = i;
                if (at == optimised.size()) { std::fprintf(stderr, "-mv: the pose graph has no node at the time of dense pose %lld; no deformed view was written\n", viewFrame); viewFailed = true; }
                else if (!viewMesh(args.gpu, *viewed, intr, optimised[at].second, viewFrame, fe->densePoseGraph.size(), viewBack, args.saveFile, viewStem + "_def", "_def")) viewFailed = true;
            }
        }
        kt_ctx_destroy(lctx);
        if (!ok) { std::fprintf(stderr, "cannot write %s.loops\n", args.saveFile.c_str()); return 1; }
        std::printf("loops %s.loops: %zu accepted constraints\n", args.saveFile.c_str(), accepted);
    }
    {   // the first frame's host copy (firstRgbImage, what the GUI and the backend show first)
        const unsigned char* first = fe->firstRgbImage.getValue();
        if (first) std::printf("first image crc %08lx\n", crc32(0L, first, (uInt)Resolution::get().numPixels() * 3));
    }
    const kt::Vector3f cam = fe->getCurrentGlobalCamera();
    std::printf("frames %d  slices %zu  points %zu  last camera %.6f %.6f %.6f  %.1f frames/s (incl. file I/O and uploads)  path %s\n", frames,
                fe->getCloudSlices().size(), points, cam(0), cam(1), cam(2), frames / sec, ops ? "operators" : "device-resident");
    if (world > 0 && !ops) {
        if (commFile.empty() || !gatherPoses(fe, rank, world, commFile, gatherCount)) { std::fprintf(stderr, "pose gather failed (-comm <file> shared by all ranks)\n"); return 1; }
    }
    return writer.failed || smoothFailed || viewFailed ? 1 : 0;
}
