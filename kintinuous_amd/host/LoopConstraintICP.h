/*
 * LoopConstraintICP -- the dense registration of a loop-closure candidate: PlaceRecognition::icpDepthFrames
 * (backend/PlaceRecognition.cpp:238-276, the "LoopConstraint" stage of processLoopClosureDetection) on the GPU, with the reference's
 * signature.  It takes the place of depthCamera->convertToXYZPointCloud, the two pcl::VoxelGrid filters at 2.5 voxel sizes,
 * pcl::transformPointCloud by the bootstrap, pcl::IterativeClosestPointNonLinear::align and getFitnessScore: one call of
 * kt_loop_icp_depth_frames (include/kt_abi.h states the stage and where it differs from PCL's Levenberg-Marquardt ICP).
 * Constructed from the intrinsics and the voxel size (Volume::get().getVoxelSizeMeters(), a cube's single edge); the image size is
 * Resolution's.
 */
#ifndef LOOPCONSTRAINTICP_H_
#define LOOPCONSTRAINTICP_H_

#include <cstdio>
#include <limits>

#include "EigenAdapters.h"
#include "Resolution.h"
#include "internal.h"

class LoopConstraintICP
{
  public:
    LoopConstraintICP(kt_ctx* ctx, const kt_intr& intr, float voxelSizeMeters, float maxDist = 4.0f, int maxIterations = 10)
        : ctx(ctx), intr(intr), leaf(2.5f * voxelSizeMeters), maxDist(maxDist), maxIterations(maxIterations) {}

    // row-major float[16] form: returns false on a library error (kt_last_error), transform = bootstrap and score = +inf then
    bool icpDepthFrames(const float bootstrap[16], const unsigned short* frame1, const unsigned short* frame2, float transform[16], float& score)
    {
        const int s = kt_loop_icp_depth_frames(ctx, frame1, frame2, Resolution::get().width(), Resolution::get().height(), &intr, bootstrap, leaf, maxDist,
                                               maxIterations, transform, &score, &info);
        if (s == KT_OK) return true;
        std::fprintf(stderr, "LoopConstraintICP: %s\n", kt_last_error());
        for (int k = 0; k < 16; ++k) transform[k] = bootstrap[k];
        score = std::numeric_limits<float>::infinity();
        return false;
    }

#ifdef KT_HAVE_EIGEN
    // the reference's signature (PlaceRecognition.h:52)
    Eigen::Matrix4f icpDepthFrames(Eigen::Matrix4f& bootstrap, unsigned short* frame1, unsigned short* frame2, float& score)
    {
        float b[16], m[16];
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) b[4 * i + j] = bootstrap(i, j);
        icpDepthFrames(b, frame1, frame2, m, score);
        kt::Matrix4f r;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) r(i, j) = m[4 * i + j];
        return kt::toEigen(r);
    }
#endif

    kt_loop_icp_info info;   // of the last call: cloud sizes, iterations, converged

  private:
    kt_ctx* ctx;
    kt_intr intr;
    float leaf, maxDist;
    int maxIterations;
};

#endif /* LOOPCONSTRAINTICP_H_ */
