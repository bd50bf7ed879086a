/*
 * iSAMInterface -- the reference's class of that name (backend/iSAMInterface.h, iSAMInterface.cpp) as a shell over kt_pose_graph
 * (include/kt_abi.h): the dense pose graph that Deformation::addCameraCamera / addCameraLoop fill
 * (backend/Deformation.cpp:130-346) and batch-optimise after every loop.  NOT iSAM: every optimise() is one kt_pose_graph_optimise
 * call from the composition of the chain, which is what batch_optimization() asks for.
 *   nodes      one per camera time, numbered by first appearance.  The first node is FIXED at the first pose it is given (the reference
 *              puts a prior on it instead).
 *   chain      addCameraCameraConstraint(time1, time2, ...) adds the node of time2 behind the node of time1 with the measurement
 *              prev^-1 curr (kt_host_pose_graph_measurement).  As in iSAMInterface.cpp:53 a call with time1 > time2 or a repeated pair is
 *              ignored; so is time1 == time2 (the reference would add an edge from a node to itself, which constrains nothing).  The
 *              solver's graph is a chain: time1 must name the newest node and time2 a new one, anything else throws.  An ignored pair
 *              with time1 == time2 leaves the chain whole (the node stays the newest); one with time1 > time2 adds no node for time2, so the
 *              next call that starts from time2 throws -- the reference carries on there with a node that no factor ties to the rest, which
 *              its solver cannot place either.  A log whose dense poses go back in time does not make a pose graph.
 *   loops      addLoopConstraint(time1, time2, constraint) adds the measurement of T(time1)^-1 T(time2) and returns a handle;
 *              removeFactor(handle) takes that loop out again.  A time that names no node throws (the reference asserts).  At most 64
 *              loops are in the graph at a time.
 *   poses      getCameraPose / getCameraPoses / getCameraPositions return poses in the WORLD basis, the one the constraints were given
 *              in.  There is no iSAM basis here: the reference rotates every pose into iSAM's axes on the way in (transformation2isam)
 *              and back on the way out, this class never leaves the world's.  They reflect the graph as it is: a getter after a change
 *              optimises first.
 * Float row-major arrays serve callers without Eigen; the Eigen overloads below go through host/EigenAdapters.h.
 */
#ifndef ISAMINTERFACE_H_
#define ISAMINTERFACE_H_

#include <stdint.h>

#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/kt_abi.h"
#include "EigenAdapters.h"

class iSAMInterface
{
  public:
    typedef int Factor;   // a loop's handle (the reference: isam::Pose3d_Pose3d_Factor*)

    explicit iSAMInterface(kt_ctx* ctx) : ctx(ctx), pg(0), pgNodes(0), dirty(true), lastChi2(0.0), lastSteps(0), lastStatus(KT_POSE_GRAPH_CONVERGED) {}
    ~iSAMInterface() { if (pg) kt_pose_graph_destroy(pg); }
    iSAMInterface(const iSAMInterface&) = delete;
    iSAMInterface& operator=(const iSAMInterface&) = delete;

    void addCameraCameraConstraint(uint64_t time1, uint64_t time2, const float Rprev[9], const float tprev[3], const float Rcurr[9], const float tcurr[3])
    {
        const std::pair<uint64_t, uint64_t> constraint(time1, time2);
        if (time1 >= time2 || cameraCameraConstraints[constraint]) return;
        float prev[16], curr[16];
        pose16(Rprev, tprev, prev);
        pose16(Rcurr, tcurr, curr);
        if (times.empty()) {   // the first node, fixed where it is: prev^-1 prev' of the measurement function is the pose itself against identity
            const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            check(kt_host_pose_graph_measurement(identity, prev, T0), "kt_host_pose_graph_measurement");
            node[time1] = 0;
            times.push_back(time1);
        }
        if (times.back() != time1 || node.count(time2)) throw std::runtime_error("iSAMInterface: the camera-camera constraints must form a chain");
        cameraCameraConstraints[constraint] = true;
        double Z[16];
        check(kt_host_pose_graph_measurement(prev, curr, Z), "kt_host_pose_graph_measurement");
        chainZ.insert(chainZ.end(), Z, Z + 16);
        node[time2] = (int)times.size();
        times.push_back(time2);
        dirty = true;
    }

    Factor addLoopConstraint(uint64_t time1, uint64_t time2, const double loopConstraint[16])
    {
        if (!node.count(time1) || !node.count(time2) || node[time1] == node[time2]) throw std::runtime_error("iSAMInterface: a loop constraint between unknown camera times");
        Loop l;
        l.a = node[time1]; l.b = node[time2]; l.active = true;
        for (int k = 0; k < 16; ++k) l.Z[k] = loopConstraint[k];
        loops.push_back(l);
        dirty = true;
        return (Factor)loops.size() - 1;
    }
    Factor addLoopConstraint(uint64_t time1, uint64_t time2, const float loopConstraint[16])   // LoopClosureConstraint::icpTrans
    {
        // through the measurement function against identity: widened, the rotation re-made from its normalised quaternion
        const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        double Z[16];
        check(kt_host_pose_graph_measurement(identity, loopConstraint, Z), "kt_host_pose_graph_measurement");
        return addLoopConstraint(time1, time2, Z);
    }

    void removeFactor(Factor factor)
    {
        if (factor < 0 || factor >= (Factor)loops.size()) throw std::runtime_error("iSAMInterface: no such factor");
        dirty = dirty || loops[factor].active;
        loops[factor].active = false;
    }

    // batch_optimization() + chi2(): 1000 x the sum of squared residuals (every factor has covariance 1e-3 I)
    double optimise()
    {
        const int n = (int)times.size();
        if (n == 0) { lastChi2 = 0.0; dirty = false; return 0.0; }
        std::vector<int> a, b;
        std::vector<double> Z;
        for (size_t i = 0; i < loops.size(); ++i)
            if (loops[i].active) { a.push_back(loops[i].a); b.push_back(loops[i].b); Z.insert(Z.end(), loops[i].Z, loops[i].Z + 16); }
        if (!pg || pgNodes < n) {
            if (pg) { kt_pose_graph_destroy(pg); pg = 0; }
            int cap = 1024;
            while (cap < n) cap *= 2;
            check(kt_pose_graph_create(ctx, cap, MAX_LOOPS, 0, &pg), "kt_pose_graph_create");
            pgNodes = cap;
        }
        poses.resize((size_t)n * 16);
        kt_pose_graph_result r;
        check(kt_pose_graph_optimise(pg, n, T0, chainZ.data(), (int)a.size(), a.data(), b.data(), Z.data(), poses.data(), &r), "kt_pose_graph_optimise");
        lastChi2 = r.chi2_end; lastSteps = r.steps; lastStatus = r.status;
        dirty = false;
        return lastChi2;
    }
    int lastStepCount() const { return lastSteps; }
    int lastStatusCode() const { return lastStatus; }

    // the pose of a camera time in the WORLD basis (row-major 4x4, rounded to float)
    kt::Matrix4f getCameraPose(uint64_t time)
    {
        if (!node.count(time)) throw std::runtime_error("iSAMInterface: unknown camera time");
        if (dirty) optimise();
        return poseOf(node[time]);
    }
    // every camera in time order (the reference walks a std::map keyed by time)
    void getCameraPoses(std::vector<std::pair<uint64_t, kt::Matrix4f> >& out)
    {
        if (dirty) optimise();
        for (std::map<uint64_t, int>::const_iterator it = node.begin(); it != node.end(); ++it) out.push_back(std::make_pair(it->first, poseOf(it->second)));
    }
    void getCameraPositions(std::vector<std::pair<uint64_t, kt::Vector3f> >& out)
    {
        if (dirty) optimise();
        for (std::map<uint64_t, int>::const_iterator it = node.begin(); it != node.end(); ++it) {
            const double* p = &poses[(size_t)it->second * 16];
            out.push_back(std::make_pair(it->first, kt::Vector3f((float)p[3], (float)p[7], (float)p[11])));
        }
    }
    // the optimised poses in double, node order (row-major 4x4 each)
    const std::vector<double>& getPosesDouble()
    {
        if (dirty) optimise();
        return poses;
    }
    size_t numNodes() const { return times.size(); }

#ifdef KT_HAVE_EIGEN
    void addCameraCameraConstraint(uint64_t time1, uint64_t time2, const kt::EigenMatrix3fRM& Rprev, const Eigen::Vector3f& tprev, const kt::EigenMatrix3fRM& Rcurr,
                                   const Eigen::Vector3f& tcurr)
    {
        addCameraCameraConstraint(time1, time2, kt::fromEigen(Rprev).data(), kt::fromEigen(tprev).data(), kt::fromEigen(Rcurr).data(), kt::fromEigen(tcurr).data());
    }
    Eigen::Matrix4f getCameraPoseEigen(uint64_t time) { return kt::toEigen(getCameraPose(time)); }
#endif

    static const int MAX_LOOPS = 64;

  private:
    struct Loop { int a, b; double Z[16]; bool active; };

    static void pose16(const float R[9], const float t[3], float out[16])
    {
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) out[4 * i + j] = R[3 * i + j];
            out[4 * i + 3] = t[i];
        }
        out[12] = out[13] = out[14] = 0.0f; out[15] = 1.0f;
    }
    static void check(int status, const char* what)
    {
        if (status != KT_OK) throw std::runtime_error(std::string("iSAMInterface: ") + what + ": " + kt_last_error());
    }
    kt::Matrix4f poseOf(int k) const
    {
        kt::Matrix4f m;
        for (int e = 0; e < 16; ++e) m.m[e] = (float)poses[(size_t)k * 16 + e];
        return m;
    }

    kt_ctx* ctx;
    kt_pose_graph* pg;
    int pgNodes;
    bool dirty;
    double lastChi2;
    int lastSteps, lastStatus;
    double T0[16];
    std::vector<uint64_t> times;          // node -> time
    std::map<uint64_t, int> node;         // time -> node
    std::vector<double> chainZ;           // 16 per chain edge
    std::vector<Loop> loops;
    std::vector<double> poses;            // the last optimisation's, 16 per node
    std::map<std::pair<uint64_t, uint64_t>, bool> cameraCameraConstraints;
};

#endif /* ISAMINTERFACE_H_ */
