/*
 * LoopClosureBootstrap -- the relative pose of a loop-closure candidate from its two frames: what Surf3DTools::calculate3dPointsSURF,
 * Surf3DTools::surfMatch3D (backend/Surf3DTools.h:67-270) and PNPSolver::getRelativePose (backend/PNPSolver.cpp:32-97) produce together
 * in PlaceRecognition::processLoopClosureDetection, in one call of kt_loop_match_frames.  NOT a port of SURF or of cv::solvePnPRansac:
 * include/kt_abi.h states the stage (FAST-9 + BRIEF-256, a Hamming ratio test with a cross-check, a three-point rigid RANSAC scored by
 * reprojection at the reference's 500 hypotheses and 2 px).  The image size is Resolution's.
 */
#ifndef LOOPCLOSUREBOOTSTRAP_H_
#define LOOPCLOSUREBOOTSTRAP_H_

#include <cstdio>
#include <utility>
#include <vector>

#include "EigenAdapters.h"
#include "Resolution.h"
#include "internal.h"

class LoopClosureBootstrap
{
  public:
    LoopClosureBootstrap(kt_ctx* ctx, const kt_intr& intr, float maxDist = 4.0f) : ctx(ctx), intr(intr)
    {
        kt_loop_match_params_default(&params);
        params.max_dist = maxDist;
        info = kt_loop_match_info();
    }

    // pose = T (row-major, new camera -> old camera, the reference's isam::Pose3d), bootstrap = its inverse as float (what icpDepthFrames
    // takes); inliers = integer pixel pairs, new first (PNPSolver.cpp:90-96).  false on a library error: identities, no inliers.
    bool getRelativePose(float pose[16], float bootstrap[16], std::vector<std::pair<int2, int2> >& inliers, const unsigned char* rgbOld,
                         const unsigned short* depthOld, const unsigned char* rgbNew, const unsigned short* depthNew)
    {
        matches.assign((size_t)params.max_keypoints * 4, 0);
        flags.assign((size_t)params.max_keypoints, 0);
        inliers.clear();
        const int s = kt_loop_match_frames(ctx, rgbOld, depthOld, rgbNew, depthNew, Resolution::get().width(), Resolution::get().height(), &intr, &params, pose,
                                           bootstrap, matches.data(), flags.data(), (size_t)params.max_keypoints, &info);
        if (s != KT_OK) {
            std::fprintf(stderr, "LoopClosureBootstrap: %s\n", kt_last_error());
            for (int k = 0; k < 16; ++k) pose[k] = bootstrap[k] = (k % 5 == 0) ? 1.0f : 0.0f;
            info = kt_loop_match_info();
            return false;
        }
        for (int m = 0; m < info.n_matches; ++m) {
            if (!flags[m]) continue;
            const int2 fresh = {matches[4 * m + 2], matches[4 * m + 3]}, old = {matches[4 * m], matches[4 * m + 1]};
            inliers.push_back(std::pair<int2, int2>(fresh, old));
        }
        return true;
    }

#ifdef KT_HAVE_EIGEN
    // the pose as the reference assembles it (PlaceRecognition.cpp:183-186)
    bool getRelativePose(Eigen::Matrix4d& T, std::vector<std::pair<int2, int2> >& inliers, const unsigned char* rgbOld, const unsigned short* depthOld,
                         const unsigned char* rgbNew, const unsigned short* depthNew)
    {
        float p[16], b[16];
        const bool ok = getRelativePose(p, b, inliers, rgbOld, depthOld, rgbNew, depthNew);
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) T(i, j) = p[4 * i + j];
        return ok;
    }
#endif

    kt_loop_match_params params;   // the stage's parameters (defaults: kt_loop_match_params_default)
    kt_loop_match_info info;       // of the last call: keypoints, matches, inliers, the winning hypothesis

  private:
    kt_ctx* ctx;
    kt_intr intr;
    std::vector<int32_t> matches;
    std::vector<uint8_t> flags;
};

#endif /* LOOPCLOSUREBOOTSTRAP_H_ */
