/*
 * LoopClosureDetection -- PlaceRecognition::processLoopClosureDetection (backend/PlaceRecognition.cpp:114-236) for one candidate pair,
 * with the reference's gates in the reference's order: fewer than 40 matches (:152), an inlier share of at most inlierRatio (:179,
 * -il = 0.35, ConfigArgs.h:119), LoopConstraintICP::icpDepthFrames with the bootstrap, a score of 0.01 or more (:196), then
 * DepthCamera::projectInlierMatches (backend/DepthCamera.cpp:66-93) and the LoopClosureConstraint record.  Which old frame to try (DBoW
 * retrieval: host/PlaceRecognition.h) and what becomes of an accepted constraint (the pose graph: host/iSAMInterface.h; the map
 * deformation is not built) are outside this class.
 */
#ifndef LOOPCLOSUREDETECTION_H_
#define LOOPCLOSUREDETECTION_H_

#include <limits>
#include <utility>
#include <vector>

#include "LoopClosureBootstrap.h"
#include "LoopConstraintICP.h"
#include "PlaceRecognitionInput.h"

struct LoopClosureVector3d { double x, y, z; };

struct LoopClosureConstraint {   // backend/LoopClosureConstraint.h
    uint64_t time1, time2;       // the new frame's utime, the old frame's
    float icpTrans[16];          // row-major
    std::vector<LoopClosureVector3d> inliers1Proj, inliers2Proj;   // the inliers' 3D points in the new and in the old frame
    uint64_t lagTime;
};

enum LoopClosureResult {
    LOOP_ACCEPTED = 0,           // "accepted!"
    LOOP_TOO_FEW_MATCHES,        // (the reference returns without a message)
    LOOP_REJECTED_INLIERS,       // "rejected on inlier percentage"
    LOOP_REJECTED_ICP_SCORE,     // "rejected on ICP score"
    LOOP_ERROR
};

inline const char* loopClosureResultText(LoopClosureResult r)
{
    switch (r) {
        case LOOP_ACCEPTED: return "accepted";
        case LOOP_TOO_FEW_MATCHES: return "rejected on match count";
        case LOOP_REJECTED_INLIERS: return "rejected on inlier percentage";
        case LOOP_REJECTED_ICP_SCORE: return "rejected on ICP score";
        default: return "error";
    }
}

class LoopClosureDetection
{
  public:
    LoopClosureDetection(kt_ctx* ctx, const kt_intr& intr, float voxelSizeMeters, float inlierRatio = 0.35f)
        : bootstrap(ctx, intr), icp(ctx, intr, voxelSizeMeters), intr(intr), inlierRatio(inlierRatio), matches(0), inlierCount(0),
          score(std::numeric_limits<float>::infinity())
    {
    }

    // DepthCamera::projectInlierMatches as written there: float depths, the products in double (the intrinsics are the kt_intr floats)
    void projectInlierMatches(const std::vector<std::pair<int2, int2> >& inliers, std::vector<LoopClosureVector3d>& inl1, std::vector<LoopClosureVector3d>& inl2,
                              const unsigned short* depth1, const unsigned short* depth2) const
    {
        const int width = Resolution::get().width();
        const double fx = intr.fx, fy = intr.fy, cx = intr.cx, cy = intr.cy;
        for (size_t i = 0; i < inliers.size(); ++i) {
            const float depthFirst = (float)depth1[inliers[i].first.y * width + inliers[i].first.x] / 1000.f;
            const float depthSecond = (float)depth2[inliers[i].second.y * width + inliers[i].second.x] / 1000.f;
            if (!depthFirst || !depthSecond) continue;
            const LoopClosureVector3d a = {depthFirst * (inliers[i].first.x - cx) * (1 / fx), depthFirst * (inliers[i].first.y - cy) * (1 / fy), depthFirst};
            const LoopClosureVector3d b = {depthSecond * (inliers[i].second.x - cx) * (1 / fx), depthSecond * (inliers[i].second.y - cy) * (1 / fy), depthSecond};
            inl1.push_back(a);
            inl2.push_back(b);
        }
    }

    // raw frames (rgb24 and uint16 millimetres of Resolution's size)
    LoopClosureResult processLoopClosureDetection(const unsigned char* rgbOld, const unsigned short* depthOld, uint64_t utimeOld, const unsigned char* rgbNew,
                                                  const unsigned short* depthNew, uint64_t utimeNew, uint64_t lagTimeNew, LoopClosureConstraint& out)
    {
        float pose[16], boot[16];
        std::vector<std::pair<int2, int2> > inliers;
        score = std::numeric_limits<float>::infinity();
        matches = inlierCount = 0;
        if (!bootstrap.getRelativePose(pose, boot, inliers, rgbOld, depthOld, rgbNew, depthNew)) return LOOP_ERROR;
        matches = bootstrap.info.n_matches;
        inlierCount = (int)inliers.size();
        if (matches < 40) return LOOP_TOO_FEW_MATCHES;
        if (!(float(inliers.size()) / matches > inlierRatio)) return LOOP_REJECTED_INLIERS;
        if (!icp.icpDepthFrames(boot, depthOld, depthNew, out.icpTrans, score)) return LOOP_ERROR;
        if (!(score < 0.01)) return LOOP_REJECTED_ICP_SCORE;
        out.time1 = utimeNew;
        out.time2 = utimeOld;
        out.lagTime = lagTimeNew;
        out.inliers1Proj.clear();
        out.inliers2Proj.clear();
        projectInlierMatches(inliers, out.inliers1Proj, out.inliers2Proj, depthNew, depthOld);
        return LOOP_ACCEPTED;
    }

    // two samples of the place-recognition buffer; compressed ones are unpacked first, as the reference does (:132-141)
    LoopClosureResult processLoopClosureDetection(PlaceRecognitionInput& oldFrame, PlaceRecognitionInput& newFrame, LoopClosureConstraint& out)
    {
        const size_t n = (size_t)Resolution::get().numPixels();
        std::vector<unsigned char> rgbO, rgbN;
        std::vector<unsigned short> depO, depN;
        const unsigned char *ro = oldFrame.rgbImage, *rn = newFrame.rgbImage;
        const unsigned short *dO = oldFrame.depthMap, *dN = newFrame.depthMap;
        if (oldFrame.isCompressed) {
            rgbO.resize(n * 3); depO.resize(n);
            oldFrame.decompressImgTo(rgbO.data()); oldFrame.decompressDepthTo((unsigned char*)depO.data());
            ro = rgbO.data(); dO = depO.data();
        }
        if (newFrame.isCompressed) {
            rgbN.resize(n * 3); depN.resize(n);
            newFrame.decompressImgTo(rgbN.data()); newFrame.decompressDepthTo((unsigned char*)depN.data());
            rn = rgbN.data(); dN = depN.data();
        }
        return processLoopClosureDetection(ro, dO, oldFrame.utime, rn, dN, newFrame.utime, newFrame.lagTime, out);
    }

    LoopClosureBootstrap bootstrap;
    LoopConstraintICP icp;
    int matchCount() const { return matches; }
    int inliersCount() const { return inlierCount; }
    float icpScore() const { return score; }   // +inf when a gate before the registration rejected the pair

  private:
    kt_intr intr;
    float inlierRatio;
    int matches, inlierCount;
    float score;
};

#endif /* LOOPCLOSUREDETECTION_H_ */
