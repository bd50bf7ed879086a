// tests/stubs/loop_icp_check.cpp -- host/LoopConstraintICP.h through a compiler and once through the GPU, against the stand-in Eigen
// headers of this directory (tests/test_gpu_loop_icp.py::test_shell).  Input file: int32 cols, rows; float32 fx, fy, cx, cy, voxel;
// float32 bootstrap[16] row-major; uint16 frame1[rows * cols], frame2[rows * cols].  Prints the transform and the score as hex floats.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "LoopConstraintICP.h"

#ifndef KT_HAVE_EIGEN
#error "the Eigen stand-ins were not found"
#endif

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int dims[2];
    float par[5], boot[16];
    if (std::fread(dims, 4, 2, f) != 2 || std::fread(par, 4, 5, f) != 5 || std::fread(boot, 4, 16, f) != 16) return 2;
    const size_t n = (size_t)dims[0] * dims[1];
    std::vector<unsigned short> f1(n), f2(n);
    if (std::fread(f1.data(), 2, n, f) != n || std::fread(f2.data(), 2, n, f) != n) return 2;
    std::fclose(f);
    Resolution::get(dims[0], dims[1]);
    kt_ctx* ctx = nullptr;
    if (kt_ctx_create(0, &ctx) != KT_OK) { std::fprintf(stderr, "%s\n", kt_last_error()); return 1; }
    kt_intr intr = {par[0], par[1], par[2], par[3]};
    LoopConstraintICP icp(ctx, intr, par[4]);
    Eigen::Matrix4f bootstrap;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) bootstrap(i, j) = boot[4 * i + j];
    float score = 0.0f;
    const Eigen::Matrix4f d = icp.icpDepthFrames(bootstrap, f1.data(), f2.data(), score);
    std::printf("transform");
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) std::printf(" %a", (double)d(i, j));
    std::printf("\nscore %a\ninfo %d %d %d %d\n", (double)score, icp.info.n_source, icp.info.n_target, icp.info.iterations, icp.info.converged);
    kt_ctx_destroy(ctx);
    return 0;
}
