// host/MeshStages.h alone (no GPU, no library): every outcome of the chain of the -m mesh, one row each, for tests/test_host_logic.py to
// compare with its own statement of the rules.  A case is the set of requested stages, whether stage 0 produced its mesh, and what each
// requested stage would do if it ran: s(ucceed), f(ail), and for -mh also r(eport only: -mh 0, which runs and produces nothing).
// Row: `<requested bits, stage 1 first> <stage 0> <outcomes> ran=<k<input ...> view=<stem|none> def=<stems> exit=<0|1>`, stems in quotes.
#include <cstdio>
#include <string>

#include "MeshStages.h"

int main()
{
    int rows = 0;
    for (int req = 0; req < 32; ++req)
        for (int stage0 = 0; stage0 < 2; ++stage0) {
            int choices[MESH_STAGES], cases = 1;
            for (int k = 1; k < MESH_STAGES; ++k) cases *= choices[k] = !(req >> (k - 1) & 1) ? 1 : k == MESH_FILL ? 3 : 2;
            for (int c = 0; c < cases; ++c) {
                MeshStageOrder chain;
                std::string bits, outcomes, ran, def;
                chain.record(MESH_COLLECT, stage0 != 0, true);
                for (int k = 1, rest = c; k < MESH_STAGES; rest /= choices[k], ++k) {
                    chain.stage[k].requested = req >> (k - 1) & 1;
                    const char outcome = chain.stage[k].requested ? "sfr"[rest % choices[k]] : '-';
                    bits += chain.stage[k].requested ? '1' : '0';
                    outcomes += outcome;
                    if (!chain.mayRun(k)) continue;
                    ran += " " + std::to_string(k) + "<" + std::to_string(chain.newest(k));
                    chain.record(k, outcome != 'f', outcome != 'r');
                }
                const std::vector<int> produced = chain.produced();
                for (size_t i = 0; i < produced.size(); ++i) def += std::string(" \"") + meshStageRules[produced[i]].stem + "\"";
                const int newest = chain.newest();
                const std::string view = newest < 0 ? "none" : std::string("\"") + meshStageRules[newest].stem + "\"";
                std::printf("%s %d %s ran=%s view=%s def=%s exit=%d\n", bits.c_str(), stage0, outcomes.c_str(), ran.c_str(), view.c_str(), def.c_str(), (int)chain.failed());
                ++rows;
            }
        }
    std::printf("mesh chain ok: %d rows\n", rows);
    return 0;
}
