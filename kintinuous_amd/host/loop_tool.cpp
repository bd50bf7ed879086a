// loop_tool -- one loop-closure candidate through the whole dense stage: reads frames I (old) and J (new) of a .klg log with
// RawLogReader and runs LoopClosureDetection::processLoopClosureDetection (bootstrap on the GPU, gates, registration, projected inliers).
//     loop_tool -l log.klg -a I -b J [-w W -h H] [-n N -s size -c calib] [-f]
// Prints one line: "matches M; inliers N; share S; score <hex float>; verdict <text>; times <new> <old>; projected P; constraint <16 hex
// floats>".  Exit code 0 for accept or reject, non-zero for an error (a frame the log does not deliver, a library error).
//     loop_tool -l log.klg -all [-every K] [-dl dislocal] [-k 0|1] [-w W -h H] [-n N -s size -c calib] [-f]
// The whole log through PlaceRecognition: every K-th frame is a sample (default 1), -dl / -k replace the candidate source's dislocal and
// consistency.  One line per sample: "sample I; status S; candidate C; score X; reference R; island F L", and for a sample whose
// candidate went through the geometric check the fields of the -a / -b line behind it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "LoopClosureDetection.h"
#include "PlaceRecognition.h"
#include "RawLogReader.h"
#include "Volume.h"

static PlaceRecognitionInput* sample(const RawLogReader& log, size_t n)
{
    unsigned char* rgb = new unsigned char[n * 3];
    unsigned short* depth = new unsigned short[n];
    std::memcpy(rgb, log.decompressedImage, n * 3);
    std::memcpy(depth, log.decompressedDepth, n * 2);
    return new PlaceRecognitionInput(rgb, (int)(n * 3), depth, (int)(n * 2), false, (uint64_t)log.timestamp, 0, kt::Vector3f(), kt::Matrix3f());
}

// -all: every `every`-th frame of the log is a sample of a place-recognition buffer, walked by PlaceRecognition
static int runAll(RawLogReader& log, size_t n, int gpu, const kt_intr& intr, int every, int dislocal, int consistency)
{
    const int capacity = 3000;   // KintinuousTracker::PR_BUFFER_SIZE
    PlaceRecognitionInput* buffer = new PlaceRecognitionInput[capacity];
    int count = 0, frame = 0;
    bool ok = true;
    for (int k = 0; count < capacity && log.grabNext(ok, frame) && ok; ++k) {
        if (k % every) continue;
        if (!log.decompressedImage) { std::fprintf(stderr, "frame %d without a colour image\n", k); delete[] buffer; return 3; }
        PlaceRecognitionInput& s = buffer[count++];
        s.rgbImage = new unsigned char[n * 3];
        s.depthMap = new unsigned short[n];
        std::memcpy(s.rgbImage, log.decompressedImage, n * 3);
        std::memcpy(s.depthMap, log.decompressedDepth, n * 2);
        s.imageSize = (int)(n * 3); s.depthSize = (int)(n * 2); s.utime = (uint64_t)log.timestamp;
    }
    kt_ctx* ctx = 0;
    if (kt_ctx_create(gpu, &ctx) != KT_OK) { std::fprintf(stderr, "%s\n", kt_last_error()); delete[] buffer; return 1; }
    int rc = 0;
    {
        kt_loop_db_detect_params dp;
        kt_loop_db_detect_params_default(&dp);
        if (dislocal >= 0) dp.dislocal = dislocal;
        if (consistency >= 0) dp.consistency = consistency;
        PlaceRecognition pr(ctx, intr, Volume::get().getVoxelSizeMeters().x, &dp, count > 0 ? count : 1);
        for (int i = 0; i < count && rc == 0; ++i) {
            PlaceRecognition::Sample s;
            if (!pr.processSample(buffer, i, s)) { rc = 1; break; }
            const kt_loop_db_result& d = s.detection;
            std::printf("sample %d; status %s; candidate %d; score %d; reference %d; island %d %d", i, placeRecognitionStatusText(d.status), d.candidate, d.candidate_score,
                        d.reference_score, d.island_first, d.island_last);
            if (s.tried) {
                LoopClosureConstraint none;
                none.time1 = none.time2 = none.lagTime = 0;
                for (int k = 0; k < 16; ++k) none.icpTrans[k] = 0.0f;
                std::printf("; ");
                PlaceRecognition::printPair(stdout, s, s.constraint >= 0 ? pr.constraints[s.constraint] : none);
            }
            std::printf("\n");
        }
    }
    delete[] buffer;
    kt_ctx_destroy(ctx);
    return rc;
}

int main(int argc, char** argv)
{
    const ConfigArgs& args = ConfigArgs::get(argc, argv);
    int a = -1, b = -1, every = 1, dislocal = -1, consistency = -1;
    bool all = false;
    for (int i = 1; i < argc; ++i) {
        all = all || std::strcmp(argv[i], "-all") == 0;
        if (i + 1 >= argc) continue;
        if (std::strcmp(argv[i], "-a") == 0) a = std::atoi(argv[i + 1]);
        if (std::strcmp(argv[i], "-b") == 0) b = std::atoi(argv[i + 1]);
        if (std::strcmp(argv[i], "-every") == 0) every = std::atoi(argv[i + 1]);
        if (std::strcmp(argv[i], "-dl") == 0) dislocal = std::atoi(argv[i + 1]);
        if (std::strcmp(argv[i], "-k") == 0) consistency = std::atoi(argv[i + 1]);
    }
    if (all && (args.logFile.empty() || every < 1)) { std::fprintf(stderr, "usage: %s -l log.klg -all [-every K] [-dl dislocal] [-k 0|1] [-w W -h H] [-n N -s size -c calib]\n", argv[0]); return 2; }
    if (!all && (args.logFile.empty() || a < 0 || b < 0 || a == b)) { std::fprintf(stderr, "usage: %s -l log.klg -a I -b J [-w W -h H] [-n N -s size -c calib]\n", argv[0]); return 2; }
    Resolution::get(args.width, args.height);
    Volume::get(args.volumeSize, args.volumeResolution);
    kt_intr intr = {528.0f * args.width / 640.0f, 528.0f * args.height / 480.0f, 320.0f * args.width / 640.0f, 240.0f * args.height / 480.0f};
    if (args.calibrationFile.size()) {
        std::ifstream f(args.calibrationFile.c_str());
        double fx, fy, cx, cy;
        if (!(f >> fx >> fy >> cx >> cy)) { std::fprintf(stderr, "cannot read calibration %s\n", args.calibrationFile.c_str()); return 2; }
        intr.fx = (float)fx; intr.fy = (float)fy; intr.cx = (float)cx; intr.cy = (float)cy;
    }
    RawLogReader log(args.logFile);
    const size_t n = (size_t)Resolution::get().numPixels();
    if (all) return runAll(log, n, args.gpu, intr, every, dislocal, consistency);
    PlaceRecognitionInput *oldFrame = 0, *newFrame = 0;
    bool ok = true;
    int frame = 0;
    for (int k = 0; (!oldFrame || !newFrame) && log.grabNext(ok, frame) && ok; ++k) {
        if (!log.decompressedImage) { std::fprintf(stderr, "frame %d without a colour image\n", k); return 3; }
        if (k == a) oldFrame = sample(log, n);
        if (k == b) newFrame = sample(log, n);
    }
    if (!oldFrame || !newFrame) { std::fprintf(stderr, "the log does not deliver frames %d and %d\n", a, b); return 3; }
    kt_ctx* ctx = 0;
    if (kt_ctx_create(args.gpu, &ctx) != KT_OK) { std::fprintf(stderr, "%s\n", kt_last_error()); return 1; }
    int rc = 0;
    {
        LoopClosureDetection detection(ctx, intr, Volume::get().getVoxelSizeMeters().x);
        LoopClosureConstraint c;
        c.time1 = c.time2 = c.lagTime = 0;
        for (int k = 0; k < 16; ++k) c.icpTrans[k] = 0.0f;
        const LoopClosureResult r = detection.processLoopClosureDetection(*oldFrame, *newFrame, c);
        const int m = detection.matchCount(), in = detection.inliersCount();
        std::printf("matches %d; inliers %d; share %.4f; score %a; verdict %s; times %llu %llu; projected %zu; constraint", m, in, m ? (double)in / m : 0.0,
                    (double)detection.icpScore(), loopClosureResultText(r), (unsigned long long)c.time1, (unsigned long long)c.time2, c.inliers1Proj.size());
        for (int k = 0; k < 16; ++k) std::printf(" %a", (double)c.icpTrans[k]);
        std::printf("\n");
        if (r == LOOP_ERROR) rc = 1;
    }
    delete oldFrame;
    delete newFrame;
    kt_ctx_destroy(ctx);
    return rc;
}
