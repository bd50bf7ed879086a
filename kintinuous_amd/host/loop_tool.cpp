// loop_tool -- one loop-closure candidate through the whole dense stage: reads frames I (old) and J (new) of a .klg log with
// RawLogReader and runs LoopClosureDetection::processLoopClosureDetection (bootstrap on the GPU, gates, registration, projected inliers).
//     loop_tool -l log.klg -a I -b J [-w W -h H] [-n N -s size -c calib] [-f]
// Prints one line: "matches M; inliers N; share S; score <hex float>; verdict <text>; times <new> <old>; projected P; constraint <16 hex
// floats>".  Exit code 0 for accept or reject, non-zero for an error (a frame the log does not deliver, a library error).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "LoopClosureDetection.h"
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

int main(int argc, char** argv)
{
    const ConfigArgs& args = ConfigArgs::get(argc, argv);
    int a = -1, b = -1;
    for (int i = 1; i + 1 < argc; ++i) {
        if (std::strcmp(argv[i], "-a") == 0) a = std::atoi(argv[i + 1]);
        if (std::strcmp(argv[i], "-b") == 0) b = std::atoi(argv[i + 1]);
    }
    if (args.logFile.empty() || a < 0 || b < 0 || a == b) { std::fprintf(stderr, "usage: %s -l log.klg -a I -b J [-w W -h H] [-n N -s size -c calib]\n", argv[0]); return 2; }
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
