/*
 * MeshGenerator -- the -m output of the reference (backend/MeshGenerator.h, MeshGenerator::save, backend/MeshGenerator.cpp:37-188)
 * on this path: NOT its greedy-projection triangulation of the processed cloud, but the marching-cubes meshes the tracker's mesh
 * stage (kt_tracker_enable_mesh_stage) built on the GPU for every slab that left the volume and for the final volume.  save()
 * concatenates them in slice order, the triangle indices offset by the vertices before them (the shape of the reference's merge,
 * :82-137), and writes <prefix>.ply (kt_host_save_ply).  Slab seams are not welded.
 */
#ifndef MESHGENERATOR_H_
#define MESHGENERATOR_H_

#include <cstdio>
#include <string>
#include <vector>

#include "internal.h"

class MeshGenerator
{
  public:
    // the meshes of every slice of tracker t; returns the number of triangles written, -1 on failure
    static long long save(kt_tracker* t, const std::string& path)
    {
        const int n = kt_tracker_num_slices(t);
        if (n < 0) return -1;
        std::vector<kt_mesh_vertex> v;
        std::vector<uint32_t> tri;
        for (int i = 0; i < n; ++i) {
            long long nv = 0, nt = 0;
            if (kt_tracker_slice_mesh_info(t, i, &nv, &nt) != KT_OK) return -1;
            if (nv < 0) continue;   // taken while the stage was off
            const size_t v0 = v.size(), t0 = tri.size();
            v.resize(v0 + (size_t)nv);
            tri.resize(t0 + 3 * (size_t)nt);
            if (kt_tracker_slice_mesh(t, i, v.data() + v0, tri.data() + t0) != KT_OK) {
                std::fprintf(stderr, "slice %d: %s\n", i, kt_last_error());
                return -1;
            }
            for (size_t k = t0; k < tri.size(); ++k) tri[k] += (uint32_t)v0;
        }
        if (kt_host_save_ply(path.c_str(), v.data(), v.size(), tri.data(), tri.size() / 3) != KT_OK) {
            std::fprintf(stderr, "%s\n", kt_last_error());
            return -1;
        }
        return (long long)(tri.size() / 3);
    }
};

#endif /* MESHGENERATOR_H_ */
