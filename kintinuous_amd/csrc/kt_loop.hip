// kt_loop.hip -- the dense registration behind a loop-closure candidate: PlaceRecognition::icpDepthFrames (backend/PlaceRecognition.cpp:
// 238-276, the TICK("LoopConstraint") stage of processLoopClosureDetection) on the GPU.  The reference turns both depth frames into
// pcl::PointXYZ clouds (DepthCamera::convertToXYZPointCloud, backend/DepthCamera.cpp:143-163), down-samples both with a pcl::VoxelGrid at
// 2.5 voxel sizes, moves the first by the PnP bootstrap, aligns it to the second with pcl::IterativeClosestPointNonLinear and takes
// getFitnessScore().  This is NOT a port of PCL's ICP: that class minimises the point-to-point error with Levenberg-Marquardt (cminpack);
// the same least-squares step has a closed form, which is what runs here (DESIGN.md 4.6 defines the stage so that it can be restated bit
// for bit: kintinuous_amd/loop_icp_ref.py is that restatement).
//   cloud      one wave per image column counts its kept pixels, one workgroup scans the columns, one wave per column writes its points
//              behind the columns before it: the reference's order (column outer, row inner), which is the summation order of the grid.
//              Intrinsics are the kt_intr floats (the reference mixes double intrinsics into the float product).
//   grid       kt_slice.hip's VoxelGrid (kt_slice_grid_device) on points of zero colour, on the context's slice workspace.
//   iteration  loop_nearest: a wave owns 64 source points, moves them by the accumulated transform M (double product, rounded once per
//              coordinate), streams the target cloud through LDS in tiles -- every lane reads the same address, a broadcast -- and keeps
//              (best d^2, best index), d^2 = (dx * dx + dy * dy) + dz * dz in float, strict `<` over ascending indices: ties go to the
//              lowest index.  No distance cap (PCL's default).  The wave then folds its 16 double terms (sum s, sum t, sum s t^T, sum
//              d^2) with a butterfly of fixed shape and writes one partial; loop_fold adds the partials in index order, one lane per term.
//              No atomics: the sums do not depend on scheduling.  The host solves the rigid fit (kt_host_rigid_fit) and M <- dM M.
//              M travels to the kernel as an argument; 16 doubles and a "correspondences changed" word come back per iteration.
// Stops after max_iterations updates, or at the first pass whose correspondences equal the previous pass's (a fixed point: that pass
// updates nothing and its d^2 are the score's).
#include "kt_internal.hpp"
#include "kt_wave.hpp"

#include <math.h>
#include <string.h>
#include <algorithm>

#define KT_LOOP_TILE 1024   // target points per LDS tile (12 KB)
#define KT_LOOP_TERMS 16    // 3 + 3 + 9 sums of the point-to-point problem, and sum d^2

namespace {

struct Xform { double m[12]; };   // rows 0..2 of the row-major 4x4

__device__ __forceinline__ bool loop_kept(unsigned short d, float max_mm) { return d != 0 && (float)d < max_mm; }

// kept pixels of every column: one wave per column, lanes stride over the rows
__global__ __launch_bounds__(64) void loop_col_count(const unsigned short* __restrict__ depth, int cols, int rows, float max_mm, unsigned int* __restrict__ count)
{
    const int u = blockIdx.x, lane = threadIdx.x;
    unsigned int n = 0;
    for (int v0 = 0; v0 < rows; v0 += 64) {
        const int v = v0 + lane;
        const bool k = v < rows && loop_kept(depth[(size_t)v * cols + u], max_mm);
        n += (unsigned int)__popcll(__ballot(k));
    }
    if (lane == 0) count[u] = n;
}

// the kept pixels of a column as points (kt_unproject_mm), behind the columns before it; colour and weight zero
__global__ __launch_bounds__(64) void loop_col_emit(const unsigned short* __restrict__ depth, int cols, int rows, float max_mm, kt_intr intr,
                                                    const unsigned int* __restrict__ offset, kt_point_xyzrgb* __restrict__ out)
{
    const int u = blockIdx.x, lane = threadIdx.x;
    unsigned int base = offset[u];
    for (int v0 = 0; v0 < rows; v0 += 64) {
        const int v = v0 + lane;
        const unsigned short d = v < rows ? depth[(size_t)v * cols + u] : (unsigned short)0;
        const bool k = v < rows && loop_kept(d, max_mm);
        const unsigned long long m = __ballot(k);
        if (k) {
            const f3 q = kt_unproject_mm(u, v, d, intr);
            kt_point_xyzrgb p;
            p.x = q.x; p.y = q.y; p.z = q.z;
            p.pad0 = 1.0f;
            p.b = p.g = p.r = p.a = 0;
            p.pad1[0] = p.pad1[1] = p.pad1[2] = 0;
            out[base + kt_wave_rank(m, lane)] = p;   // (base + rank < the scan's total <= cols * rows)
        }
        base += (unsigned int)__popcll(m);
    }
}

// the grid's centroids (6 floats per leaf) as a packed xyz cloud; the leaf count next to it
__global__ __launch_bounds__(256) void loop_take_xyz(const float* __restrict__ cen, const unsigned int* __restrict__ leaves, unsigned int cap,
                                                     float* __restrict__ xyz, unsigned int* __restrict__ n_out)
{
    const unsigned int n = min(*leaves, cap);
    for (unsigned int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        xyz[3 * (size_t)i] = cen[6 * (size_t)i]; xyz[3 * (size_t)i + 1] = cen[6 * (size_t)i + 1]; xyz[3 * (size_t)i + 2] = cen[6 * (size_t)i + 2];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = n;
}

// One wave per 64 source points.  XFORM: move the point by M first.  REDUCE: compare with the previous pass's correspondences and
// write the wave's partial {16 sums, changed}.  out_index / out_d2 may be null when REDUCE (prev holds the indices then).
template <bool XFORM, bool REDUCE>
__global__ __launch_bounds__(64) void loop_nearest(const float* __restrict__ src, int n_src, const float* __restrict__ dst, int n_dst, Xform M,
                                                   unsigned int* __restrict__ out_index, float* __restrict__ out_d2, unsigned int* __restrict__ prev,
                                                   double* __restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) float tx[KT_LOOP_TILE], ty[KT_LOOP_TILE], tz[KT_LOOP_TILE];
    const int lane = threadIdx.x, i = blockIdx.x * 64 + lane;
    const bool live = i < n_src;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (live) {
        px = src[3 * (size_t)i]; py = src[3 * (size_t)i + 1]; pz = src[3 * (size_t)i + 2];
        if (XFORM) {
            const double x = px, y = py, z = pz;
            px = (float)(((M.m[0] * x + M.m[1] * y) + M.m[2] * z) + M.m[3]);
            py = (float)(((M.m[4] * x + M.m[5] * y) + M.m[6] * z) + M.m[7]);
            pz = (float)(((M.m[8] * x + M.m[9] * y) + M.m[10] * z) + M.m[11]);
        }
    }
    float best = __builtin_inff();
    unsigned int bi = 0;
    for (int j0 = 0; j0 < n_dst; j0 += KT_LOOP_TILE) {
        const int nt = min(KT_LOOP_TILE, n_dst - j0);
        __syncthreads();   // the previous tile has been read by every lane
        for (int j = lane; j < nt; j += 64) {
            tx[j] = dst[3 * (size_t)(j0 + j)]; ty[j] = dst[3 * (size_t)(j0 + j) + 1]; tz[j] = dst[3 * (size_t)(j0 + j) + 2];
        }
        __syncthreads();
        int j = 0;
        for (; j + 4 <= nt; j += 4) {
            const float4 x4 = *(const float4*)&tx[j], y4 = *(const float4*)&ty[j], z4 = *(const float4*)&tz[j];
            const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, ys[4] = {y4.x, y4.y, y4.z, y4.w}, zs[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float dx = px - xs[q], dy = py - ys[q], dz = pz - zs[q];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < best) { best = d2; bi = (unsigned int)(j0 + j + q); }
            }
        }
        for (; j < nt; ++j) {
            const float dx = px - tx[j], dy = py - ty[j], dz = pz - tz[j];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < best) { best = d2; bi = (unsigned int)(j0 + j); }
        }
    }
    if (live && out_index) out_index[i] = bi;
    if (live && out_d2) out_d2[i] = best;
    if (!REDUCE) return;
    bool changed = false;
    double term[KT_LOOP_TERMS];
#pragma unroll
    for (int k = 0; k < KT_LOOP_TERMS; ++k) term[k] = 0.0;
    if (live) {
        changed = prev[i] != bi;
        prev[i] = bi;
        const double s[3] = {px, py, pz}, t[3] = {dst[3 * (size_t)bi], dst[3 * (size_t)bi + 1], dst[3 * (size_t)bi + 2]};
        kt_rigid_terms(s, t, term);
        term[15] = (double)best;
    }
    const bool any = __any(changed);
#pragma unroll
    for (int k = 0; k < KT_LOOP_TERMS; ++k) term[k] = kt_wave_sum(term[k]);
    if (lane == 0) {
        double* o = partial + (size_t)blockIdx.x * (KT_LOOP_TERMS + 1);
#pragma unroll
        for (int k = 0; k < KT_LOOP_TERMS; ++k) o[k] = term[k];
        o[KT_LOOP_TERMS] = any ? 1.0 : 0.0;
    }
}

// the partials in index order, one lane per term (lane 16: the changed flags)
__global__ __launch_bounds__(64) void loop_fold(const double* __restrict__ partial, int n_partial, double* __restrict__ out)
{
    const int k = threadIdx.x;
    if (k > KT_LOOP_TERMS) return;
    double s = 0.0;
    for (int p = 0; p < n_partial; ++p) s += partial[(size_t)p * (KT_LOOP_TERMS + 1) + k];
    out[k] = s;
}

}  // namespace

struct kt_loop_ws {
    kt_mem mem;
    size_t pix_cap, pt_cap, col_cap;
    unsigned short* depth;        // one frame, pix_cap pixels
    unsigned int* col;            // per-column counts / offsets, col_cap
    float* cloud[2];              // S and T, pt_cap points of 3 floats
    unsigned int* n_cloud;        // device: {n_S, n_T}
    unsigned int* index;          // correspondences of the previous pass (or kt_cloud_nearest's output), pt_cap
    float* d2;                    // pt_cap
    double* partial;              // (pt_cap / 64 + 1) x 17
    double* sums;                 // device, 17
    double* sums_host;            // pinned, 17
    unsigned int* n_host;         // pinned, 2
};

int kt_loop_ws_destroy(kt_loop_ws* w)
{
    if (w) w->mem.release();
    delete w;
    return KT_OK;
}

static int loop_ws_alloc(kt_loop_ws* w)
{
    kt_mem& m = w->mem;
    KT_TRY(m.device(&w->depth, w->pix_cap)); KT_TRY(m.device(&w->col, w->col_cap));
    KT_TRY(m.device(&w->cloud[0], w->pt_cap * 3)); KT_TRY(m.device(&w->cloud[1], w->pt_cap * 3));
    KT_TRY(m.device(&w->n_cloud, 2)); KT_TRY(m.device(&w->index, w->pt_cap)); KT_TRY(m.device(&w->d2, w->pt_cap));
    KT_TRY(m.device(&w->partial, (w->pt_cap / 64 + 1) * (KT_LOOP_TERMS + 1))); KT_TRY(m.device(&w->sums, KT_LOOP_TERMS + 1));
    KT_TRY(m.pinned(&w->sums_host, KT_LOOP_TERMS + 1));
    return m.pinned(&w->n_host, 2);
}

// the context's workspace, for frames of `pixels` pixels / `cols` columns and clouds of up to `points` points.  Grown when needed: the stream is drained, every
// buffer released and allocated again at the larger of its old and its requested capacity.  A failure leaves the context without a workspace (the next call starts afresh).
static int loop_ws_reserve(kt_ctx* c, size_t pixels, size_t cols, size_t points, kt_loop_ws** out)
{
    kt_loop_ws* w = c->loop_ws;
    if (w && w->pix_cap >= pixels && w->col_cap >= cols && w->pt_cap >= points) { *out = w; return KT_OK; }
    KT_HIP(hipStreamSynchronize(c->stream));
    if (!w) c->loop_ws = w = new kt_loop_ws();
    w->mem.release();
    w->pix_cap = std::max({w->pix_cap, pixels, (size_t)1}); w->col_cap = std::max({w->col_cap, cols, (size_t)1}); w->pt_cap = std::max({w->pt_cap, points, (size_t)1});
    const int s = loop_ws_alloc(w);
    if (s != KT_OK) { (void)kt_loop_ws_destroy(w); c->loop_ws = nullptr; return s; }
    *out = w;
    return KT_OK;
}

// steps a + b for one host frame, enqueued: cloud[which] and n_cloud[which] on the device
static int loop_frame_to_grid(kt_ctx* c, kt_loop_ws* w, const uint16_t* frame, int cols, int rows, const kt_intr* intr, float leaf, float max_dist, int which)
{
    const size_t pixels = (size_t)cols * rows;
    kt_slice_ws* sw = nullptr;
    KT_TRY(kt_slice_ws_of_ctx(c, pixels, &sw));
    hipStream_t st = c->stream;
    const float max_mm = max_dist * 1000.0f;
    KT_HIP(hipMemcpyAsync(w->depth, frame, pixels * sizeof(unsigned short), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(loop_col_count, dim3(cols), dim3(64), 0, st, w->depth, cols, rows, max_mm, w->col);
    hipLaunchKernelGGL(kt_scan_runs_kernel<1>, dim3(1), dim3(256), 0, st, w->col, cols, kt_slice_ws_input_count(sw));
    hipLaunchKernelGGL(loop_col_emit, dim3(cols), dim3(64), 0, st, w->depth, cols, rows, max_mm, *intr, w->col, kt_slice_ws_input(sw));
    KT_LAUNCH_CHECK();
    KT_TRY(kt_slice_grid_device(sw, kt_slice_ws_input(sw), kt_slice_ws_input_count(sw), pixels, 0, leaf));
    const int nb = kt_div_up((int)pixels, 256);
    hipLaunchKernelGGL(loop_take_xyz, dim3(nb < 1024 ? nb : 1024), dim3(256), 0, st, kt_slice_ws_centroids(sw), kt_slice_ws_leaves_dev(sw), (unsigned int)pixels,
                       w->cloud[which], w->n_cloud + which);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

static bool loop_frame_args(const uint16_t* frame, int cols, int rows, const kt_intr* intr, float leaf, float max_dist)
{
    return frame && cols > 0 && rows > 0 && (long long)cols * rows < (1 << 30) && intr && intr->fx != 0.0f && intr->fy != 0.0f && leaf > 0.0f && max_dist > 0.0f;
}

extern "C" int kt_depth_to_cloud_grid(kt_ctx* c, const uint16_t* frame, int cols, int rows, const kt_intr* intr, float leaf, float max_dist,
                                      float* out_xyz, size_t capacity, size_t* n_out)
{
    KT_ARG(c && n_out && loop_frame_args(frame, cols, rows, intr, leaf, max_dist) && (out_xyz || capacity == 0));
    *n_out = 0;
    const size_t pixels = (size_t)cols * rows;
    kt_loop_ws* w = nullptr;
    KT_TRY(loop_ws_reserve(c, pixels, (size_t)cols, pixels, &w));
    KT_TRY(loop_frame_to_grid(c, w, frame, cols, rows, intr, leaf, max_dist, 0));
    KT_HIP(hipMemcpyAsync(w->n_host, w->n_cloud, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    KT_HIP(hipStreamSynchronize(c->stream));
    const size_t n = w->n_host[0];
    *n_out = n;
    if (n > capacity) { kt_set_error("kt_depth_to_cloud_grid: %zu points, capacity %zu", n, capacity); return KT_ERR_CAPACITY; }
    if (n) {
        KT_HIP(hipMemcpyAsync(out_xyz, w->cloud[0], n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        KT_HIP(hipStreamSynchronize(c->stream));
    }
    return KT_OK;
}

extern "C" int kt_cloud_nearest(kt_ctx* c, const float* src_xyz, size_t n_src, const float* dst_xyz, size_t n_dst, uint32_t* out_index, float* out_d2)
{
    KT_ARG(c && src_xyz && dst_xyz && out_index && out_d2 && n_src > 0 && n_dst > 0 && n_src < (1u << 30) && n_dst < (1u << 30));
    kt_loop_ws* w = nullptr;
    KT_TRY(loop_ws_reserve(c, 0, 0, n_src > n_dst ? n_src : n_dst, &w));
    hipStream_t st = c->stream;
    KT_HIP(hipMemcpyAsync(w->cloud[0], src_xyz, n_src * 3 * sizeof(float), hipMemcpyHostToDevice, st));
    KT_HIP(hipMemcpyAsync(w->cloud[1], dst_xyz, n_dst * 3 * sizeof(float), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((loop_nearest<false, false>), dim3(kt_div_up((int)n_src, 64)), dim3(64), 0, st, w->cloud[0], (int)n_src, w->cloud[1], (int)n_dst, Xform(),
                       w->index, w->d2, (unsigned int*)nullptr, (double*)nullptr);
    KT_LAUNCH_CHECK();
    KT_HIP(hipMemcpyAsync(out_index, w->index, n_src * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KT_HIP(hipMemcpyAsync(out_d2, w->d2, n_src * sizeof(float), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    return KT_OK;
}

// one pass over cloud[0] (ns points) and cloud[1] (nt points): correspondences under rows 0..2 of M, their sums and whether they differ from
// w->index (which then holds them) -> sums_host
static int loop_pass(kt_ctx* c, kt_loop_ws* w, int ns, int nt, const double* M)
{
    hipStream_t st = c->stream;
    const int nw = kt_div_up(ns, 64);
    Xform X;
    for (int k = 0; k < 12; ++k) X.m[k] = M[k];
    hipLaunchKernelGGL((loop_nearest<true, true>), dim3(nw), dim3(64), 0, st, w->cloud[0], ns, w->cloud[1], nt, X, (unsigned int*)nullptr, (float*)nullptr,
                       w->index, w->partial);
    hipLaunchKernelGGL(loop_fold, dim3(1), dim3(64), 0, st, w->partial, nw, w->sums);
    KT_LAUNCH_CHECK();
    KT_HIP(hipMemcpyAsync(w->sums_host, w->sums, (KT_LOOP_TERMS + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    return KT_OK;
}

// test hook (kt_debug.h): one pass on the caller's clouds and previous correspondences
extern "C" int kt_debug_loop_pass(kt_ctx* c, const float* src_xyz, size_t n_src, const float* dst_xyz, size_t n_dst, const double M[12], uint32_t* prev,
                                  double out_sums[17])
{
    KT_ARG(c && src_xyz && dst_xyz && M && prev && out_sums && n_src > 0 && n_dst > 0 && n_src < (1u << 30) && n_dst < (1u << 30));
    kt_loop_ws* w = nullptr;
    KT_TRY(loop_ws_reserve(c, 0, 0, n_src > n_dst ? n_src : n_dst, &w));
    hipStream_t st = c->stream;
    KT_HIP(hipMemcpyAsync(w->cloud[0], src_xyz, n_src * 3 * sizeof(float), hipMemcpyHostToDevice, st));
    KT_HIP(hipMemcpyAsync(w->cloud[1], dst_xyz, n_dst * 3 * sizeof(float), hipMemcpyHostToDevice, st));
    KT_HIP(hipMemcpyAsync(w->index, prev, n_src * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    KT_TRY(loop_pass(c, w, (int)n_src, (int)n_dst, M));
    KT_HIP(hipMemcpyAsync(prev, w->index, n_src * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    memcpy(out_sums, w->sums_host, KT_LOOP_TERMS * sizeof(double));
    out_sums[KT_LOOP_TERMS] = w->sums_host[KT_LOOP_TERMS] == 0.0 ? 0.0 : 1.0;   // (the word counts the waves that saw a change; the stage tests it against 0 as here)
    return KT_OK;
}

extern "C" int kt_loop_icp_depth_frames(kt_ctx* c, const uint16_t* frame1, const uint16_t* frame2, int cols, int rows, const kt_intr* intr,
                                        const float bootstrap[16], float leaf, float max_dist, int max_iterations, float out_transform[16],
                                        float* out_score, kt_loop_icp_info* out_info)
{
    KT_ARG(c && bootstrap && out_transform && out_score && out_info && max_iterations >= 0 && loop_frame_args(frame1, cols, rows, intr, leaf, max_dist) && frame2);
    const size_t pixels = (size_t)cols * rows;
    kt_loop_ws* w = nullptr;
    KT_TRY(loop_ws_reserve(c, pixels, (size_t)cols, pixels, &w));
    hipStream_t st = c->stream;
    KT_TRY(loop_frame_to_grid(c, w, frame1, cols, rows, intr, leaf, max_dist, 0));
    KT_TRY(loop_frame_to_grid(c, w, frame2, cols, rows, intr, leaf, max_dist, 1));
    KT_HIP(hipMemcpyAsync(w->n_host, w->n_cloud, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    KT_HIP(hipMemsetAsync(w->index, 0xff, w->pt_cap * sizeof(unsigned int), st));   // no previous pass: every correspondence counts as changed
    KT_HIP(hipStreamSynchronize(st));
    const int ns = (int)w->n_host[0], nt = (int)w->n_host[1];
    memset(out_info, 0, sizeof(*out_info));
    out_info->n_source = ns; out_info->n_target = nt;
    for (int k = 0; k < 16; ++k) out_transform[k] = bootstrap[k];
    *out_score = __builtin_inff();
    if (ns == 0 || nt == 0) return KT_OK;
    double M[16];
    for (int k = 0; k < 16; ++k) M[k] = (double)bootstrap[k];
    bool scored = false;
    auto pass = [&]() -> int { return loop_pass(c, w, ns, nt, M); };
    for (int it = 0; it < max_iterations; ++it) {
        KT_TRY(pass());
        if (w->sums_host[KT_LOOP_TERMS] == 0.0) { out_info->converged = 1; scored = true; break; }   // the fixed point: M stays, this pass's d^2 are the score's
        double dM[16], Mn[16];
        KT_TRY(kt_host_rigid_fit(w->sums_host, (double)ns, dM));
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) Mn[4 * a + b] = ((dM[4 * a] * M[b] + dM[4 * a + 1] * M[4 + b]) + dM[4 * a + 2] * M[8 + b]) + dM[4 * a + 3] * M[12 + b];
        memcpy(M, Mn, sizeof(M));
        out_info->iterations = it + 1;
    }
    if (!scored) KT_TRY(pass());
    *out_score = (float)(w->sums_host[15] / (double)ns);
    for (int k = 0; k < 16; ++k) out_transform[k] = (float)M[k];
    return KT_OK;
}
