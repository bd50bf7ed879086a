/*
 * MeshStages -- the chain of the -m mesh and its post-passes as data, and the rules that order it.  Only indices and flags, no mesh and no
 * library call, so that tests/stubs/mesh_chain_check.cpp walks every outcome on the CPU; MeshChain.h puts the meshes and the runner on top.
 */
#ifndef MESHSTAGES_H_
#define MESHSTAGES_H_

#include <vector>

enum { MESH_COLLECT, MESH_WELD, MESH_COMP, MESH_FILL, MESH_SMOOTH, MESH_SIMP, MESH_STAGES };

// A new stage is an entry here, a body in MeshChain.h and a flag in main().  The stage writes <prefix><stem>.ply and <prefix><sidecar>;
// spans: the sidecar opens with the `span utime first_in first_out` lines; cannot: what stderr says, with the prefix, when its pass fails.
// failureSetsExitStatus is inherited: of the five passes only a failed -mt has ever ended the driver with status 1.  Kept as found.
static const struct MeshStageRule { const char *flag, *stem, *sidecar; bool spans; const char* cannot; bool failureSetsExitStatus; } meshStageRules[MESH_STAGES] = {
    {"-m", "", 0, false, 0, false},   // the collected mesh, <prefix>.ply
    {"-mw", "_weld", ".weld", true, "cannot weld %s.ply\n", false},
    {"-mc", "_comp", ".comp", true, "cannot filter the components of the mesh of %s\n", false},
    {"-mh", "_fill", ".holes", true, "cannot find the boundaries of the mesh of %s\n", false},
    {"-mt", "_smooth", ".smooth", false, "cannot smooth the mesh of %s\n", true},
    {"-ms", "_simp", ".simp", true, "cannot simplify the mesh of %s\n", false},
};

struct MeshStageOrder {
    // requested: after the command line's validation; ran: it ran and succeeded; failed: it ran and failed; produced: its mesh exists and
    // its .ply was written (-mh 0 runs and produces nothing: it only reports)
    struct Stage { bool requested, ran, failed, produced; } stage[MESH_STAGES];

    MeshStageOrder() : stage() {}

    void record(int k, bool ok, bool producesMesh)
    {
        stage[k].ran = ok;
        stage[k].failed = !ok;
        stage[k].produced = ok && producesMesh;
    }

    // stage k >= 1 runs when it is requested, stage 0 produced a mesh, and every earlier REQUESTED stage ran
    bool mayRun(int k) const
    {
        bool may = k >= 1 && stage[k].requested && stage[MESH_COLLECT].produced;
        for (int j = 1; j < k; ++j) may = may && (stage[j].ran || !stage[j].requested);
        return may;
    }

    // the latest stage before `before` that produced a mesh, -1: none.  newest(k) is the input of stage k; newest() is what -mv views
    int newest(int before = MESH_STAGES) const
    {
        int k = before - 1;
        while (k >= 0 && !stage[k].produced) --k;
        return k;
    }

    // every stage that produced a mesh, in stage order: what -df deforms and writes as <prefix><stem>_def.ply
    std::vector<int> produced() const
    {
        std::vector<int> all;
        for (int k = 0; k < MESH_STAGES; ++k)
            if (stage[k].produced) all.push_back(k);
        return all;
    }

    // the chain's part of the exit status
    bool failed() const
    {
        bool any = false;
        for (int k = 0; k < MESH_STAGES; ++k) any = any || (stage[k].failed && meshStageRules[k].failureSetsExitStatus);
        return any;
    }
};

#endif /* MESHSTAGES_H_ */
