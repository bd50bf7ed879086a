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
#include <functional>
#include <map>
#include <string>
#include <thread>

#include "CloudSliceProcessor.h"
#include "DeformationGraph.h"
#include "MeshChain.h"
#include "iSAMInterface.h"
#include "PlaceRecognition.h"
#include "TrackerInterface.h"

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
// With -m every mesh the chain produced goes the same way, in stage order: its vertices through applyGraphToMesh under the same rule with
// its own span table (a stage's is its pass's, the smoothed mesh's its input's), and <prefix><stem>_def.ply over the same triangles.  The
// collected mesh also gives one `mesh utime vertices` line per span of MeshGenerator::collect ahead of the result line.
static bool deformMap(kt_ctx* ctx, KintinuousTracker* fe, const std::vector<LoopClosureConstraint>& constraints, const std::vector<char>& kept,
                      const std::vector<std::pair<uint64_t, kt::Matrix4f> >& optimised, float poseDist, double gate, CloudSliceProcessor& sliceProcessor, MeshChain& chain,
                      MeshWriter& writer, const std::string& prefix)
{
    const std::vector<int> produced = chain.produced();
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
        for (size_t i = 0; i < produced.size(); ++i) {
            MeshGenerator::Mesh& m = chain.mesh[produced[i]];
            for (size_t k = 0; produced[i] == MESH_COLLECT && k < m.spanTime.size(); ++k)
                std::fprintf(f, "mesh %llu %zu\n", (unsigned long long)m.spanTime[k], m.spanFirst[k + 1] - m.spanFirst[k]);
            if (apply && m.vertices.size()) graph.applyGraphToMesh(m.vertices.data(), m.vertices.size(), m.spanFirst.data(), m.spanTime.data(), (int)m.spanTime.size());
        }
        std::fprintf(f, "result %d %zu %s %d %a %a %a\n", nodes, graph.numConstraints(), statusText[r.status], r.steps, r.error_start, r.error_end, r.constraint_error);
        std::fclose(f);
        f = 0;
        if (sliceProcessor.save(prefix + "_def.pcd") < 0) { std::fprintf(stderr, "cannot write %s_def.pcd\n", prefix.c_str()); return false; }
        for (size_t i = 0; i < produced.size(); ++i) {
            const std::string ply = prefix + meshStageRules[produced[i]].stem + "_def.ply";
            const long long tris = writer.write(chain.mesh[produced[i]], ply);
            if (tris < 0) { std::fprintf(stderr, "cannot write %s\n", ply.c_str()); return false; }
            std::printf("mesh %s: %lld triangles\n", ply.c_str(), tris);
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

int main(int argc, char** argv)
{
    const ConfigArgs& args = ConfigArgs::get(argc, argv);
    if (args.help || args.logFile.empty()) { ConfigArgs::usage(argv[0]); return args.help ? 0 : 1; }
    bool ops = false, pcd = false, pcdraw = false, ppm = false, noStage = false, loops = false, poseGraph = false, deform = false;
    MeshChain chain;            // the -m mesh and its post-passes: a stage's flag sets its `requested`, the validation below may take it back
    bool &weld = chain.stage[MESH_WELD].requested, &components = chain.stage[MESH_COMP].requested, &holes = chain.stage[MESH_FILL].requested;
    bool &smooth = chain.stage[MESH_SMOOTH].requested, &simplify = chain.stage[MESH_SIMP].requested;
    WeldStage weldStage;             // what each stage takes from the command line is the stage's own
    ComponentStage componentStage;
    HoleStage holeStage;
    SmoothStage smoothStage;
    SimplifyStage simplifyStage;
    bool quadricBiasGiven = false;   // -msb
    bool view = false;          // -mv: the last mesh of the chain is rendered from dense pose viewFrame (-mvf; -1: the last), viewBack metres back (-mvb)
    long long viewFrame = -1;
    bool viewFrameGiven = false;
    float viewBack = 0.0f;
    bool normals = false;       // -mn: every .ply carries vertex normals
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
        if (i + 1 < argc && std::string(argv[i]) == "-mwg") weldStage.gapSeconds = std::atof(argv[i + 1]);
        if (i + 1 < argc && std::string(argv[i]) == "-ms") { simplify = true; simplifyStage.cell = (float)std::atof(argv[i + 1]); }
        simplifyStage.quadric = simplifyStage.quadric || std::string(argv[i]) == "-msq";
        if (i + 1 < argc && std::string(argv[i]) == "-msb") { quadricBiasGiven = true; simplifyStage.bias = (float)std::atof(argv[i + 1]); }
        if (i + 1 < argc && std::string(argv[i]) == "-mc") { components = true; componentStage.minTriangles = std::atoll(argv[i + 1]); }
        if (i + 1 < argc && std::string(argv[i]) == "-mh") { holes = true; holeStage.maxEdges = std::atoll(argv[i + 1]); }
        if (i + 1 < argc && std::string(argv[i]) == "-mt") { smooth = true; smoothStage.steps = std::atoll(argv[i + 1]); }
        smoothStage.rim = smoothStage.rim || std::string(argv[i]) == "-mtb";
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
    const bool meshStage = args.generateMesh && !ops;
    if (meshStage) tracker.getFrontend()->enableMeshStage();
    if (args.generateMesh && ops) std::fprintf(stderr, "-m ignored with -ops (the mesh stage runs on the device-resident path)\n");
    // the flags that work on the -m mesh, in the order their messages come: without the mesh stage each is ignored; then the flag's own checks
    const auto ignore = [](bool& given, const char* why) { std::fprintf(stderr, "%s\n", why); given = false; };
    const struct { const char* flag; bool* given; const char* does; std::function<void()> own; } onTheMesh[] = {
        {"-mw", &weld, "welds the seams of the -m mesh", {}},
        {"-ms", &simplify, "simplifies the -m mesh", [&]() {
             if (simplifyStage.quadric && !simplify) ignore(simplifyStage.quadric, "-msq ignored without -ms (it places the vertices that -ms merges)");
             if (quadricBiasGiven && !simplify) std::fprintf(stderr, "-msb ignored without -ms (it is the bias of -ms -msq)\n");
             else if (quadricBiasGiven && !simplifyStage.quadric) std::fprintf(stderr, "-msb ignored without -msq (it is the bias of -ms -msq)\n");
         }},
        {"-mc", &components, "drops the small pieces of the -m mesh", [&]() {
             const long long least = componentStage.minTriangles;
             if (components && (least < 1 || least > 0xffffffffll)) ignore(components, "-mc ignored: it takes a number of triangles from 1 to 2^32 - 1");
         }},
        {"-mh", &holes, "reports the boundaries of the -m mesh and fills its small holes", [&]() {
             if (holes && (holeStage.maxEdges < 0 || holeStage.maxEdges > 256)) ignore(holes, "-mh ignored: it takes a number of edges from 0 to 256");
             if (holes && !weld) std::fprintf(stderr, "-mh without -mw: every slab seam will show as a boundary\n");
         }},
        {"-mt", &smooth, "smooths the -m mesh", [&]() {
             if (smooth && (smoothStage.steps < 0 || smoothStage.steps > 64)) ignore(smooth, "-mt ignored: it takes a number of steps from 0 to 64");
             if (smoothStage.rim && !smooth) ignore(smoothStage.rim, "-mtb ignored without -mt (it lets the rims of the smoothed mesh move)");
         }},
        {"-mv", &view, "renders the -m mesh", [&]() {
             if ((viewFrameGiven || viewBack != 0.0f) && !view) std::fprintf(stderr, "-mvf and -mvb ignored without -mv (they place its camera)\n");
         }},
        {"-mn", &normals, "gives the -m mesh vertex normals", {}},
    };
    for (const auto& o : onTheMesh) {
        if (*o.given && !meshStage) ignore(*o.given, (std::string(o.flag) + " ignored without -m (it " + o.does + ")").c_str());
        if (o.own) o.own();
    }
    if (weld) tracker.getFrontend()->enableMeshKeys();
    // (the upper end of -mvf is known only once the log has been tracked)
    if (view && viewFrameGiven && viewFrame < 0) { std::fprintf(stderr, "-mvf takes the index of a dense pose, from 0\n"); return 1; }
    if (view && !(std::fabs(viewBack) < 8192.0f)) { std::fprintf(stderr, "-mvb takes a distance in metres below 8192\n"); return 1; }
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
    if (meshStage) {   // MainController.cpp:247-249: meshGenerator->save()
        bool ok = MeshGenerator::collect(fe->handle(), chain.mesh[MESH_COLLECT]);
        const long long tris = ok ? writer.write(chain.mesh[MESH_COLLECT], args.saveFile + ".ply") : -1;
        if (tris < 0) { std::fprintf(stderr, "cannot write %s.ply\n", args.saveFile.c_str()); ok = false; }
        else std::printf("mesh %s.ply: %lld triangles\n", args.saveFile.c_str(), tris);
        chain.record(MESH_COLLECT, ok, true);
    }
    MeshStage* const stages[MESH_STAGES] = {0, &weldStage, &componentStage, &holeStage, &smoothStage, &simplifyStage};
    for (int k = 1; k < MESH_STAGES; ++k)
        if (chain.mayRun(k)) chain.run(k, *stages[k], args.gpu, writer, args.saveFile);
    // -mv: the mesh the run wrote last, from a dense pose (whose frame is the vertices': the deformation's nodes are these positions)
    const int newest = chain.newest();
    const std::string viewStem = newest < 0 ? "" : meshStageRules[newest].stem;
    bool viewFailed = false, haveView = false;
    if (view && newest >= 0) {
        const size_t poses = fe->densePoseGraph.size();
        if (!viewFrameGiven) viewFrame = (long long)poses - 1;
        if (viewFrame < 0 || (size_t)viewFrame >= poses) {
            std::fprintf(stderr, "-mvf %lld: the run has %zu dense poses; no view was written\n", viewFrame, poses);
            viewFailed = true;
        } else {
            haveView = viewMesh(args.gpu, chain.mesh[newest], intr, fe->densePoseGraph[(size_t)viewFrame].pose, viewFrame, poses, viewBack, args.saveFile, viewStem, "");
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
            if (ok && poseGraph && deform && !deformMap(lctx, fe, pr.constraints, kept, optimised, poseDist, deformGate, sliceProcessor, chain, writer, args.saveFile)) { kt_ctx_destroy(lctx); return 1; }
            if (ok && poseGraph && deform && haveView) {   // -mv with -df: the deformed twin (deformMap moved the vertices in place) from the optimised pose of the same frame
                const uint64_t stamp = fe->densePoseGraph[(size_t)viewFrame].timestamp;
                size_t at = optimised.size();
                for (size_t i = 0; i < optimised.size() && at == optimised.size(); ++i)
                    if (optimised[i].first == stamp) at = i;
                if (at == optimised.size()) { std::fprintf(stderr, "-mv: the pose graph has no node at the time of dense pose %lld; no deformed view was written\n", viewFrame); viewFailed = true; }
                else if (!viewMesh(args.gpu, chain.mesh[newest], intr, optimised[at].second, viewFrame, fe->densePoseGraph.size(), viewBack, args.saveFile, viewStem + "_def", "_def")) viewFailed = true;
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
    return writer.failed || chain.failed() || viewFailed ? 1 : 0;
}
