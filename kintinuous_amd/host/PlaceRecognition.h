/*
 * PlaceRecognition -- the reference's backend thread of that name (backend/PlaceRecognition.cpp:51-112) as a walk over the tracker's
 * placeRecognitionBuffer: every sample goes through the candidate source (the reference: dbowInterface->detectLoop(), a DLoopDetector
 * over SURF words; here kt_loop_db_detect, a database of the bootstrap's descriptors -- include/kt_abi.h), and a detected
 * candidate through LoopClosureDetection::processLoopClosureDetection(buffer[candidate], buffer[current]).  Accepted constraints are
 * collected.  The database's entry ids are the buffer's indices: the walk starts at 0 and skips nothing.
 * DIVERGENCE: the reference skips a sample when less than loopThrottle seconds of wall clock have passed since the last accepted loop
 * (:64-66); that gate makes the result depend on timing and is not built.  What becomes of a constraint is outside this class: the
 * pose graph is host/iSAMInterface.h (kintinuous_hip -pg), the map deformation is not built.
 */
#ifndef PLACERECOGNITION_H_
#define PLACERECOGNITION_H_

#include <cstdio>
#include <string>
#include <vector>

#include "LoopClosureDetection.h"

inline const char* placeRecognitionStatusText(int status)
{
    switch (status) {
        case KT_LOOP_DB_EMPTY: return "EMPTY";
        case KT_LOOP_DB_LOW_REFERENCE: return "LOW_REFERENCE";
        case KT_LOOP_DB_NO_CANDIDATE: return "NO_CANDIDATE";
        case KT_LOOP_DB_NOT_CONSISTENT: return "NOT_CONSISTENT";
        case KT_LOOP_DB_DETECTED: return "DETECTED";
        default: return "?";
    }
}

class PlaceRecognition
{
  public:
    struct Sample {
        kt_loop_db_result detection;
        bool tried;                  // a candidate was detected and went through the geometric check
        LoopClosureResult verdict;   // ... with this outcome
        int matches, inliers;
        float icpScore;
        int constraint;              // index into `constraints` when accepted, else -1
    };

    // maxEntries: DBowInterfaceSurf.cpp:45 makes room for 1000 images
    PlaceRecognition(kt_ctx* ctx, const kt_intr& intr, float voxelSizeMeters, const kt_loop_db_detect_params* detect = 0, int maxEntries = 1000)
        : detection(ctx, intr, voxelSizeMeters), db(0)
    {
        kt_loop_match_params mp;
        kt_loop_match_params_default(&mp);
        kt_loop_db_detect_params_default(&detectParams);
        if (detect) detectParams = *detect;
        if (kt_loop_db_create(ctx, maxEntries, &mp, 0, &db) != KT_OK) { std::fprintf(stderr, "PlaceRecognition: %s\n", kt_last_error()); db = 0; }
    }
    ~PlaceRecognition() { kt_loop_db_destroy(db); }

    // sample `current` of the buffer (the database holds samples 0 .. current - 1); false on a library error
    bool processSample(PlaceRecognitionInput* buffer, int current, Sample& out)
    {
        out.tried = false; out.verdict = LOOP_ERROR; out.matches = out.inliers = 0; out.constraint = -1;
        out.icpScore = std::numeric_limits<float>::infinity();
        if (!db || kt_loop_db_size(db) != current) { std::fprintf(stderr, "PlaceRecognition: sample %d out of order\n", current); return false; }
        PlaceRecognitionInput& s = buffer[current];
        const size_t n = (size_t)Resolution::get().numPixels();
        const unsigned char* rgb = s.rgbImage;
        const unsigned short* depth = s.depthMap;
        if (s.isCompressed) {   // unpacked the way LoopClosureDetection does it (PlaceRecognition.cpp:132-141)
            rgbScratch.resize(n * 3); depthScratch.resize(n);
            s.decompressImgTo(rgbScratch.data()); s.decompressDepthTo((unsigned char*)depthScratch.data());
            rgb = rgbScratch.data(); depth = depthScratch.data();
        }
        if (kt_loop_db_detect(db, rgb, depth, Resolution::get().cols(), Resolution::get().rows(), &detectParams, &out.detection) != KT_OK) {
            std::fprintf(stderr, "PlaceRecognition: %s\n", kt_last_error());
            return false;
        }
        if (out.detection.status != KT_LOOP_DB_DETECTED) return true;
        LoopClosureConstraint c;
        c.time1 = c.time2 = c.lagTime = 0;
        for (int k = 0; k < 16; ++k) c.icpTrans[k] = 0.0f;
        out.tried = true;
        out.verdict = detection.processLoopClosureDetection(buffer[out.detection.candidate], s, c);
        out.matches = detection.matchCount(); out.inliers = detection.inliersCount(); out.icpScore = detection.icpScore();
        if (out.verdict == LOOP_ERROR) return false;
        if (out.verdict == LOOP_ACCEPTED) { out.constraint = (int)constraints.size(); constraints.push_back(c); accepted.push_back(out); }
        return true;
    }

    // placeRecognitionBuffer[0 .. count) in order
    bool process(PlaceRecognitionInput* buffer, int count)
    {
        for (int i = kt_loop_db_size(db); i < count; ++i) {
            Sample s;
            if (!processSample(buffer, i, s)) return false;
            samples.push_back(s);
        }
        return true;
    }

    // the fields loop_tool prints for one pair, without a line end
    static void printPair(FILE* f, const Sample& s, const LoopClosureConstraint& c)
    {
        std::fprintf(f, "matches %d; inliers %d; share %.4f; score %a; verdict %s; times %llu %llu; projected %zu; constraint", s.matches, s.inliers,
                     s.matches ? (double)s.inliers / s.matches : 0.0, (double)s.icpScore, loopClosureResultText(s.verdict), (unsigned long long)c.time1,
                     (unsigned long long)c.time2, c.inliers1Proj.size());
        for (int k = 0; k < 16; ++k) std::fprintf(f, " %a", (double)c.icpTrans[k]);
    }

    // one text line per accepted constraint: time1 time2 matches inliers score + the 16 entries of icpTrans, floats in hex
    bool saveLoops(const std::string& path) const
    {
        FILE* f = std::fopen(path.c_str(), "w");
        if (!f) return false;
        for (size_t i = 0; i < constraints.size(); ++i) {
            const LoopClosureConstraint& c = constraints[i];
            std::fprintf(f, "%llu %llu %d %d %a", (unsigned long long)c.time1, (unsigned long long)c.time2, accepted[i].matches, accepted[i].inliers, (double)accepted[i].icpScore);
            for (int k = 0; k < 16; ++k) std::fprintf(f, " %a", (double)c.icpTrans[k]);
            std::fprintf(f, "\n");
        }
        return std::fclose(f) == 0;
    }

    LoopClosureDetection detection;
    kt_loop_db_detect_params detectParams;
    std::vector<Sample> samples;                      // of process()
    std::vector<LoopClosureConstraint> constraints;   // the accepted ones, in sample order
    std::vector<Sample> accepted;                     // ... and their samples

  private:
    kt_loop_db* db;
    std::vector<unsigned char> rgbScratch;
    std::vector<unsigned short> depthScratch;
    PlaceRecognition(const PlaceRecognition&);
    PlaceRecognition& operator=(const PlaceRecognition&);
};

#endif /* PLACERECOGNITION_H_ */
