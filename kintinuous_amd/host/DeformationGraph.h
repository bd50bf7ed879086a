/*
 * DeformationGraph -- the reference's class of that name (backend/DeformationGraph.h, DeformationGraph.cpp) as a shell over kt_deform
 * (include/kt_abi.h): the graph that Deformation::addCameraLoop builds over the camera poses, constrains and solves
 * (backend/Deformation.cpp:258-334).  NOT a port: the energy, the graph, the weights and the constants are the reference's, the solver
 * is the library's banded Gauss-Newton on the GPU.
 *   initialiseGraphPoses   samples the nodes from camera positions in time order (DeformationGraph.cpp:62-73: pose 0, then every pose
 *                          farther than poseDist, float norm, from the last kept one) and sets the graph.  Fewer than five nodes make no
 *                          graph: it returns the count and initialised() stays false.
 *   addConstraint          a vertex id, the vertex (position and time: there is no vertex pool here, a constraint carries its source) and
 *                          its target; a constraint with an id already present REPLACES that one (DeformationGraph.cpp:679-693).
 *   clearConstraints, optimiseGraphSparse (kt_deform_optimise from the identity state; the result struct says what became of it),
 *   applyGraphToVertices   in place on PointXYZRGBNormal points with a time each (kt_deform_apply),
 *   applyGraphToMesh       in place on the -m mesh's vertices in spans of one time each (kt_deform_apply_mesh); colours stay,
 *   getGraph               the nodes: id, position, rotation (column-major, as Eigen stores it) and translation after the last optimise.
 */
#ifndef DEFORMATIONGRAPH_H_
#define DEFORMATIONGRAPH_H_

#include <stdint.h>

#include <cmath>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/kt_abi.h"
#include "internal.h"

struct GraphNode {
    int id;
    uint64_t time;
    double position[3], rotation[9], translation[3];   // rotation column-major
};

class DeformationGraph
{
  public:
    explicit DeformationGraph(kt_ctx* ctx) : ctx(ctx), dg(0), capNodes(0), capConstraints(0), isInitialised(false) {}
    ~DeformationGraph() { if (dg) kt_deform_destroy(dg); }
    DeformationGraph(const DeformationGraph&) = delete;
    DeformationGraph& operator=(const DeformationGraph&) = delete;

    static const int MAX_NODES = 4096;

    // positions: n x 3 floats in time order, times: n.  Returns the number of nodes sampled
    int initialiseGraphPoses(const float* positions, const uint64_t* times, size_t n, float poseDist)
    {
        graph.clear();
        nodePos.clear();
        nodeTime.clear();
        isInitialised = false;
        for (size_t i = 0; i < n; ++i) {
            if (i > 0) {
                const float* last = &nodePos[nodePos.size() - 3];
                const float dx = last[0] - positions[3 * i], dy = last[1] - positions[3 * i + 1], dz = last[2] - positions[3 * i + 2];
                if (!(std::sqrt((dx * dx + dy * dy) + dz * dz) > poseDist)) continue;
            }
            nodePos.insert(nodePos.end(), positions + 3 * i, positions + 3 * i + 3);
            nodeTime.push_back(times[i]);
        }
        const int M = (int)nodeTime.size();
        if (M < 5) return M;
        if (M > MAX_NODES) throw std::runtime_error("DeformationGraph: more than 4096 nodes (raise poseDist)");
        reserve(M, capConstraints);
        check(kt_deform_set_graph(dg, M, nodePos.data(), nodeTime.data()), "kt_deform_set_graph");
        isInitialised = true;
        std::vector<double> identity((size_t)M * 12, 0.0);
        for (int i = 0; i < M; ++i) identity[12 * i] = identity[12 * i + 4] = identity[12 * i + 8] = 1.0;
        fillGraph(identity);
        return M;
    }
    bool initialised() const { return isInitialised; }

    void addConstraint(int vertexId, const float vertex[3], uint64_t vertexTime, const double target[3])
    {
        std::map<int, size_t>::const_iterator it = constraintOf.find(vertexId);
        size_t k;
        if (it != constraintOf.end()) k = it->second;
        else {
            k = srcTime.size();
            constraintOf[vertexId] = k;
            srcPos.resize(3 * (k + 1));
            srcTime.resize(k + 1);
            targets.resize(3 * (k + 1));
        }
        for (int a = 0; a < 3; ++a) { srcPos[3 * k + a] = vertex[a]; targets[3 * k + a] = target[a]; }
        srcTime[k] = vertexTime;
    }
    void clearConstraints() { constraintOf.clear(); srcPos.clear(); srcTime.clear(); targets.clear(); }
    size_t numConstraints() const { return srcTime.size(); }
    const std::vector<float>& constraintSources() const { return srcPos; }
    const std::vector<uint64_t>& constraintTimes() const { return srcTime; }
    const std::vector<double>& constraintTargets() const { return targets; }

    kt_deform_result optimiseGraphSparse(const kt_deform_params* params = 0)
    {
        if (!isInitialised) throw std::runtime_error("DeformationGraph: not initialised");
        const int M = (int)nodeTime.size();
        if ((int)srcTime.size() > capConstraints) {   // a larger object: the graph is set again on it
            reserve(M, (int)srcTime.size());
            check(kt_deform_set_graph(dg, M, nodePos.data(), nodeTime.data()), "kt_deform_set_graph");
        }
        std::vector<double> state((size_t)M * 12);
        kt_deform_result r;
        check(kt_deform_optimise(dg, (int)srcTime.size(), srcPos.data(), srcTime.data(), targets.data(), params, state.data(), &r), "kt_deform_optimise");
        fillGraph(state);
        return r;
    }

    void applyGraphToVertices(PointXYZRGBNormal* vertices, const uint64_t* vertexTimes, size_t n)
    {
        if (!isInitialised) throw std::runtime_error("DeformationGraph: not initialised");
        static_assert(sizeof(PointXYZRGBNormal) == sizeof(kt_point_xyzrgbnormal), "vertex layout");
        check(kt_deform_apply(dg, reinterpret_cast<kt_point_xyzrgbnormal*>(vertices), vertexTimes, n), "kt_deform_apply");
    }

    // vertices [spanFirst[s], spanFirst[s + 1]) carry spanTime[s]: MeshGenerator::collect's table
    void applyGraphToMesh(kt_mesh_vertex* vertices, size_t n, const size_t* spanFirst, const uint64_t* spanTime, int nSpans)
    {
        if (!isInitialised) throw std::runtime_error("DeformationGraph: not initialised");
        check(kt_deform_apply_mesh(dg, vertices, n, spanFirst, spanTime, nSpans), "kt_deform_apply_mesh");
    }

    std::vector<GraphNode>& getGraph() { return graph; }

  private:
    static void check(int status, const char* what)
    {
        if (status != KT_OK) throw std::runtime_error(std::string("DeformationGraph: ") + what + ": " + kt_last_error());
    }
    // an object for at least this many nodes and constraints (it only ever grows; a new object has no graph)
    void reserve(int nodes, int constraints)
    {
        if (dg && nodes <= capNodes && constraints <= capConstraints) return;
        int cn = capNodes > 64 ? capNodes : 64, cc = capConstraints > 1024 ? capConstraints : 1024;
        while (cn < nodes) cn *= 2;
        while (cc < constraints) cc *= 2;
        if (cn > MAX_NODES) cn = MAX_NODES;
        if (dg) { kt_deform_destroy(dg); dg = 0; }
        check(kt_deform_create(ctx, cn, cc, 0, &dg), "kt_deform_create");
        capNodes = cn; capConstraints = cc;
    }
    void fillGraph(const std::vector<double>& state)
    {
        graph.resize(nodeTime.size());
        for (size_t i = 0; i < graph.size(); ++i) {
            GraphNode& g = graph[i];
            g.id = (int)i;
            g.time = nodeTime[i];
            for (int a = 0; a < 3; ++a) { g.position[a] = (double)nodePos[3 * i + a]; g.translation[a] = state[12 * i + 9 + a]; }
            for (int a = 0; a < 9; ++a) g.rotation[a] = state[12 * i + a];
        }
    }

    kt_ctx* ctx;
    kt_deform* dg;
    int capNodes, capConstraints;
    bool isInitialised;
    std::vector<float> nodePos, srcPos;
    std::vector<uint64_t> nodeTime, srcTime;
    std::vector<double> targets;
    std::map<int, size_t> constraintOf;   // vertex id -> its constraint
    std::vector<GraphNode> graph;
};

#endif /* DEFORMATIONGRAPH_H_ */
