// ConfigArgs.h -- the command-line options of the reference that reach the tracking + fusion path
// (utils/ConfigArgs.h:36-75, 111-200).  Options of the GUI / backend (-v, -m, -od, -il, ...) are accepted and ignored so
// reference command lines keep working.  Additions: -n <N> volume resolution (the reference's compile-time VOL),
// -w/-h image size, -o <prefix> output prefix (the reference derives saveFile from the log name).
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

class ConfigArgs {
  public:
    static const ConfigArgs& get(int argc = 0, char** argv = 0)
    {
        static const ConfigArgs instance(argc, argv);
        return instance;
    }

    static void usage(const std::string argv0)
    {
        std::fprintf(stderr,
                     "Usage: %s [Options]\n"
                     "  -l <log.klg>   log file (raw or zlib depth, raw or JPEG colour)\n"
                     "  -dt <threads>  decode the log ahead on this many threads (compressed logs: ~5 ms of inflate + JPEG per VGA frame; default: hardware threads / 4, at most 8; 0 = inside the read call)\n"
                     "  -gj            JPEG colour: decode only the entropy stage on the decode threads, reconstruct the pixels on the GPU (default off)\n"
                     "  -c <calib>     calibration file: fx fy cx cy\n"
                     "  -s <metres>    volume size (default 6)\n"
                     "  -t <voxels>    voxel shift threshold (default 14)\n"
                     "  -g <gpu>       device\n"
                     "  -n <N>         volume resolution (default 512)\n"
                     "  -r | -ri       RGB-D odometry | RGB-D + ICP odometry\n"
                     "  -v <vocab>     loop-closure vocabulary: sample frames into placeRecognitionBuffer (the DBoW backend itself is not part of this path)\n"
                     "  -lc            with -v: after the log, run PlaceRecognition (candidate database + geometric check) over the samples and write <prefix>.loops\n"
                     "                 ([-dl dislocal] [-k 0|1]: the candidate source's dislocal and consistency, as for loop_tool -all)\n"
                     "  -p <file>      ground-truth odometry from a trajectory file (lines utime,x,y,z,qx,qy,qz,qw)\n"
                     "  -fod           fast odometry,  -sm static mode,  -d dynamic cube,  -dc no colour angle weight,  -no no overlap\n"
                     "  -f             flip colours (RGB <-> BGR)\n"
                     "  -tum           write poses with timestamps in seconds (TUM format; the .poses default)\n"
                     "  -o <prefix>    output prefix (default: the log name)\n"
                     "  -cw <weight>   weight cull of the slice processor (default 8),  -nos do not keep overlapping points in the saved cloud\n"
                     "  -pcdraw        debug: the extracted slices as they are into <prefix>.raw.pcd (binary, x y z rgb)\n"
                     "  -pcd           run the CloudSliceProcessor stage behind the tracker and save <prefix>.pcd as the reference does\n"
                     "                 (binary pcl::PointXYZRGBNormal: x y z rgb normal_x normal_y normal_z curvature)\n"
                     "  -m             mesh every slab that leaves the volume and the final volume on the GPU and write <prefix>.ply\n"
                     "                 (binary PLY, x y z red green blue + triangles; marching cubes of the TSDF, NOT the reference's\n"
                     "                 greedy-projection triangulation of the processed cloud, so the file differs from the reference's)\n"
                     "  -mw            with -m: weld the slab seams by voxel-edge key on the GPU and write <prefix>_weld.ply and <prefix>.weld\n"
                     "                 (-mwg <seconds>: slabs further apart in time than that stay unwelded; with -df also <prefix>_weld_def.ply)\n"
                     "  -ms <metres>   with -m: merge the mesh vertices of one slab in one cubic cell of that edge on the GPU (the welded mesh with -mw)\n"
                     "                 and write <prefix>_simp.ply and <prefix>.simp (with -df also <prefix>_simp_def.ply)\n"
                     "  -msq           with -ms: put every merged vertex at the minimiser of its triangles' error quadrics where that lies in its cell\n"
                     "                 (else at the mean, as without -msq): edges and corners stay sharp; <prefix>.simp gains a `quadric` line\n"
                     "                 (-msb <bias>: the pull towards the mean, 2^-20 to 1, default 0.015625)\n"
                     "  -mc <triangles> with -m: drop the connected pieces of the mesh that have fewer triangles than that on the GPU (the welded mesh\n"
                     "                 with -mw) and write <prefix>_comp.ply and <prefix>.comp; -ms then takes this mesh (with -df also <prefix>_comp_def.ply)\n"
                     "  -mh <edges>    with -m: report the open boundaries of the mesh (after -mw and -mc) on the GPU in <prefix>.holes and close its simple\n"
                     "                 loops of at most that many edges (0 to 256; 0 only reports) with a fan each in <prefix>_fill.ply; -ms then takes this\n"
                     "                 mesh (with -df also <prefix>_fill_def.ply)\n"
                     "  -mt <steps>    with -m: smooth the vertex positions of the mesh (after -mw, -mc and -mh) on the GPU with that many steps (0 to 64) of\n"
                     "                 Taubin's lambda|mu filter (0.5, -0.53), the rims pinned, and write <prefix>_smooth.ply and <prefix>.smooth; -ms then\n"
                     "                 takes this mesh (with -df also <prefix>_smooth_def.ply); -mtb: the rim vertices move along their rim\n"
                     "  -mn            with -m: give every .ply of the run a normal per vertex (x y z nx ny nz red green blue), area-weighted from\n"
                     "                 that file's own triangles on the GPU, and list the files in <prefix>.normals\n"
                     "  -mv            with -m: render the last mesh the run writes (<prefix>.ply, or the last of _weld, _comp, _fill, _smooth, _simp) on the\n"
                     "                 GPU from the last dense pose at the run's resolution and intrinsics (near 0.05 m) and write <stem>_view_depth.pgm\n"
                     "                 (16-bit big-endian mm), <stem>_view_color.ppm, <stem>_view_model.ppm and <prefix>.view (pose, file, counts);\n"
                     "                 -mvf <i>: from dense pose i; -mvb <metres>: the camera that far back along its viewing axis; with -df also the\n"
                     "                 deformed twin from the optimised pose of that frame: <stem>_def_view_* and <prefix>_def.view\n"
                     "  -ppm           write the final model views: <prefix>_model.ppm, _color.ppm, _depth.pgm\n"
                     "  -rank R -world W -comm <file> [-gk K]   one process per GPU (-g): gather every rank's K most recent dense poses at the end (RCCL; default 1)\n",
                     argv0.c_str());
    }

    std::string calibrationFile, logFile, trajectoryFile, saveFile, vocabFile;
    int gpu, voxelShift, volumeResolution, width, height, totalNumFrames, weightCull, decodeThreads;
    float volumeSize;
    bool staticMode, dynamicCube, flipColors, extractOverlap, saveOverlap, useRGBD, useRGBDICP, disableColorAngleWeight, fastOdometry, help;
    bool generateMesh;   // -m (ConfigArgs.h:151 of the reference)
    bool gpuJpeg;        // -gj, shell only: RawLogReader defers the pixel half of JPEG colour to its consumer

  private:
    static bool flag(int argc, char** argv, const char* name)
    {
        for (int i = 1; i < argc; ++i)
            if (std::strcmp(argv[i], name) == 0) return true;
        return false;
    }
    static const char* value(int argc, char** argv, const char* name)
    {
        for (int i = 1; i + 1 < argc; ++i)
            if (std::strcmp(argv[i], name) == 0) return argv[i + 1];
        return 0;
    }

    ConfigArgs(int argc, char** argv)
        : gpu(0), voxelShift(14), volumeResolution(512), width(640), height(480), totalNumFrames(0), weightCull(8), decodeThreads(-1), volumeSize(6.0f)
    {
        const char* v;
        if ((v = value(argc, argv, "-c"))) calibrationFile = v;
        if ((v = value(argc, argv, "-l"))) logFile = v;
        if ((v = value(argc, argv, "-p"))) trajectoryFile = v;
        if ((v = value(argc, argv, "-v"))) vocabFile = v;   // a DBoW vocabulary switches the place-recognition tap on (ConfigArgs.h:121)
        if ((v = value(argc, argv, "-g"))) gpu = std::atoi(v);
        if ((v = value(argc, argv, "-t"))) voxelShift = std::atoi(v);
        if ((v = value(argc, argv, "-n"))) volumeResolution = std::atoi(v);
        if ((v = value(argc, argv, "-w"))) width = std::atoi(v);
        if ((v = value(argc, argv, "-h"))) height = std::atoi(v);
        if ((v = value(argc, argv, "-s"))) volumeSize = (float)std::atof(v);
        if ((v = value(argc, argv, "-fl"))) totalNumFrames = std::atoi(v);
        if ((v = value(argc, argv, "-dt"))) decodeThreads = std::atoi(v);   // shell only: RawLogReader decode-ahead
        if ((v = value(argc, argv, "-cw"))) weightCull = std::atoi(v);   // ConfigArgs.h:118 (default 8)
        staticMode = flag(argc, argv, "-sm");
        dynamicCube = flag(argc, argv, "-d");
        flipColors = flag(argc, argv, "-f");
        extractOverlap = !flag(argc, argv, "-no");
        saveOverlap = !flag(argc, argv, "-nos");   // ConfigArgs.h:153
        useRGBD = flag(argc, argv, "-r");
        useRGBDICP = flag(argc, argv, "-ri");
        disableColorAngleWeight = flag(argc, argv, "-dc");
        fastOdometry = flag(argc, argv, "-fod");
        generateMesh = flag(argc, argv, "-m");
        gpuJpeg = flag(argc, argv, "-gj");
        help = flag(argc, argv, "--help");
        if (useRGBDICP) useRGBD = false;  // ConfigArgs.h: -ri wins over -r
        if ((v = value(argc, argv, "-o"))) saveFile = v;
        else saveFile = logFile;
    }
};
