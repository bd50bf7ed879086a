// kt_match.hip -- the bootstrap of a loop-closure candidate: the dense half of PlaceRecognition::processLoopClosureDetection before
// icpDepthFrames (backend/PlaceRecognition.cpp:114-188) on the GPU.  The reference takes SURF keypoints and descriptors of both frames
// (DBowInterfaceSurf), lifts them to 3D and matches them with a ratio test (Surf3DTools.h:67-270) and runs cv::solvePnPRansac at 500
// iterations / 2 px (PNPSolver.cpp:32-97).  This is NOT a port of SURF or of OpenCV's PnP: it is a defined stage with the same inputs,
// outputs and gates (include/kt_abi.h and DESIGN.md 4.8 state it; kintinuous_amd/loop_match_ref.py restates it bit for bit).
//   frame      rgb + depth travel in ONE copy per frame (a pinned staging buffer).  kt_bgr_to_intensity, then one lane per pixel: the
//              FAST-9 score, the 5x5 box sum, non-maximum suppression + margin + depth with a histogram of the surviving scores
//              (integer atomics: counts do not depend on their order).  One workgroup finds the cut score; one wave per image row
//              counts the corners above and at the cut, one workgroup scans the rows, one wave per row writes (score, raster index)
//              keys by ballot / popcount -- above the cut all of them, at the cut the first ones in raster order.  One workgroup
//              sorts the keys (a bitonic network of fixed shape in LDS); one lane per keypoint builds its descriptor and 3D point.
//   nearest    a wave owns 64 query descriptors and streams the other frame's descriptors through LDS in tiles (every lane reads the
//              same address: a broadcast), __popcll on four 64-bit words, strict `<` over ascending indices: ties to the lowest index.
//   accept     one wave walks the new keypoints in order: ratio test, cross-check, ballot / popcount compaction of the match list.
//   ransac     one lane per hypothesis: three match indices from a counter hash, the rigid fit through them in double, then the
//              matches stream through LDS in tiles and the lane counts its reprojection inliers.  One wave folds (score, index) with
//              a butterfly of fixed shape: the highest score, ties to the lowest hypothesis.  No atomics.
// The host refits over the winner's inliers (kt_host_rigid_fit) and scores once more.
#include "kt_internal.hpp"
#include "kt_wave.hpp"

#include <math.h>
#include <string.h>
#include <algorithm>

#define KT_BRIEF_STORAGE __constant__ const
#include "kt_brief_table.hpp"

#define KT_MATCH_BINS 4096                        // scores are at most 16 * 255 = 4080
#define KT_MATCH_MARGIN (KT_BRIEF_REACH + 2)      // the descriptor's reach plus the radius of the 5x5 box
#define KT_MATCH_RANSAC_TILE 1024                 // matches per LDS tile (20 KB)
#define KT_MATCH_EPS 1e-3                         // a degenerate triple: |p1 - p0| or the distance of p2 from that line below 1 mm
#define KT_MATCH_MAX_HYP 65536

namespace {

struct Rigid { double R[9], t[3]; };

// ---- shared by the RANSAC kernel and the host's refit (double, no contraction: the same bits on both sides) ----
__host__ __device__ inline unsigned int match_hash(unsigned int seed, unsigned int h, unsigned int k)
{
    unsigned int x = seed + 0x9E3779B9u * (3u * h + k + 1u);
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;   // murmur3 fmix32
    return x;
}

// three distinct indices below m (m >= 3), distinct by skipping
__host__ __device__ inline void match_draw(unsigned int seed, unsigned int h, unsigned int m, unsigned int idx[3])
{
    const unsigned int i0 = match_hash(seed, h, 0) % m;
    unsigned int i1 = match_hash(seed, h, 1) % (m - 1u);
    i1 += i1 >= i0 ? 1u : 0u;
    unsigned int i2 = match_hash(seed, h, 2) % (m - 2u);
    const unsigned int lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    i2 += i2 >= lo ? 1u : 0u;
    i2 += i2 >= hi ? 1u : 0u;
    idx[0] = i0; idx[1] = i1; idx[2] = i2;
}

// e = {e1, e2, e3}, cen = the centroid; false for a degenerate triple
__host__ __device__ inline bool match_triad(const float* p0, const float* p1, const float* p2, double e[9], double cen[3])
{
    const double a[3] = {(double)p1[0] - (double)p0[0], (double)p1[1] - (double)p0[1], (double)p1[2] - (double)p0[2]};
    const double b[3] = {(double)p2[0] - (double)p0[0], (double)p2[1] - (double)p0[1], (double)p2[2] - (double)p0[2]};
    const double n1 = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    if (!(n1 >= KT_MATCH_EPS)) return false;
    e[0] = a[0] / n1; e[1] = a[1] / n1; e[2] = a[2] / n1;
    const double c[3] = {e[1] * b[2] - e[2] * b[1], e[2] * b[0] - e[0] * b[2], e[0] * b[1] - e[1] * b[0]};
    const double n3 = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    if (!(n3 >= KT_MATCH_EPS)) return false;
    e[6] = c[0] / n3; e[7] = c[1] / n3; e[8] = c[2] / n3;
    e[3] = e[7] * e[2] - e[8] * e[1]; e[4] = e[8] * e[0] - e[6] * e[2]; e[5] = e[6] * e[1] - e[7] * e[0];
    for (int k = 0; k < 3; ++k) cen[k] = (((double)p0[k] + (double)p1[k]) + (double)p2[k]) / 3.0;
    return true;
}

// T (new -> old) through the three pairs idx of the match arrays pn / po (3 floats per match)
__host__ __device__ inline bool match_fit3(const float* pn, const float* po, const unsigned int idx[3], Rigid* T)
{
    double en[9], eo[9], cn[3], co[3];
    if (!match_triad(pn + 3 * (size_t)idx[0], pn + 3 * (size_t)idx[1], pn + 3 * (size_t)idx[2], en, cn)) return false;
    if (!match_triad(po + 3 * (size_t)idx[0], po + 3 * (size_t)idx[1], po + 3 * (size_t)idx[2], eo, co)) return false;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) T->R[3 * a + b] = (eo[a] * en[b] + eo[3 + a] * en[3 + b]) + eo[6 + a] * en[6 + b];
    for (int a = 0; a < 3; ++a) T->t[a] = co[a] - ((T->R[3 * a] * cn[0] + T->R[3 * a + 1] * cn[1]) + T->R[3 * a + 2] * cn[2]);
    return true;
}

struct Proj { double fx, fy, cx, cy, thr2; };

__host__ __device__ inline bool match_inlier(const Rigid& T, float xf, float yf, float zf, int uo, int vo, const Proj& P)
{
    const double x = xf, y = yf, z = zf;
    const double X = ((T.R[0] * x + T.R[1] * y) + T.R[2] * z) + T.t[0];
    const double Y = ((T.R[3] * x + T.R[4] * y) + T.R[5] * z) + T.t[1];
    const double Z = ((T.R[6] * x + T.R[7] * y) + T.R[8] * z) + T.t[2];
    if (!(Z > 0.0)) return false;
    const double du = ((P.fx * X) / Z + P.cx) - (double)uo, dv = ((P.fy * Y) / Z + P.cy) - (double)vo;
    return (du * du + dv * dv) <= P.thr2;
}

// ---- the frame: scores, box sum, suppression, selection ----
__constant__ const signed char match_ring[16][2] = {{0, -3}, {1, -3}, {2, -2}, {3, -1}, {3, 0}, {3, 1}, {2, 2}, {1, 3},
                                                    {0, 3}, {-1, 3}, {-2, 2}, {-3, 1}, {-3, 0}, {-3, -1}, {-2, -2}, {-1, -3}};

// a run of 9 set bits in the ring mask, the ring taken as a circle
__device__ __forceinline__ bool match_run9(unsigned int m)
{
    const unsigned int d = m | (m << 16);
    unsigned int r = d & (d >> 1);
    r &= r >> 2;
    r &= r >> 4;       // bit i: bits i .. i + 7 set
    r &= d >> 8;       // ... and bit i + 8
    return (r & 0xFFFFu) != 0u;
}

// one lane per pixel: the FAST-9 score (0: no corner, or within 3 pixels of a border) and the 5x5 box sum (0 where the window leaves the image)
__global__ __launch_bounds__(256) void match_score_box(const unsigned char* __restrict__ I, int cols, int rows, int t, unsigned short* __restrict__ score,
                                                       unsigned short* __restrict__ box)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cols * rows) return;
    const int v = i / cols, u = i - v * cols;
    int s = 0;
    if (u >= 3 && v >= 3 && u < cols - 3 && v < rows - 3) {
        const int c = I[i];
        unsigned int bright = 0, dark = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int r = I[(v + match_ring[k][1]) * cols + (u + match_ring[k][0])];
            bright |= (r > c + t ? 1u : 0u) << k;
            dark |= (r < c - t ? 1u : 0u) << k;
            const int a = (r > c ? r - c : c - r) - t;
            s += a > 0 ? a : 0;
        }
        if (!match_run9(bright) && !match_run9(dark)) s = 0;
    }
    score[i] = (unsigned short)s;
    int b = 0;
    if (u >= 2 && v >= 2 && u < cols - 2 && v < rows - 2) {
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) b += I[(v + dy) * cols + (u + dx)];
    }
    box[i] = (unsigned short)b;
}

// non-maximum suppression on the scores of all corners, then the margin and the depth rule; kept = the score of a surviving corner or 0
__global__ __launch_bounds__(256) void match_nms_hist(const unsigned short* __restrict__ score, const unsigned short* __restrict__ depth, int cols, int rows,
                                                      float max_mm, unsigned short* __restrict__ kept, unsigned int* __restrict__ hist)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cols * rows) return;
    const int v = i / cols, u = i - v * cols;
    const int s = score[i];
    bool keep = s > 0 && u >= KT_MATCH_MARGIN && v >= KT_MATCH_MARGIN && u < cols - KT_MATCH_MARGIN && v < rows - KT_MATCH_MARGIN;
    if (keep) {   // (the margin keeps all eight neighbours inside the image)
        const unsigned short d = depth[i];
        keep = d != 0 && (float)d < max_mm;
        const unsigned short* up = score + i - cols;
        const unsigned short* dn = score + i + cols;
        keep = keep && s > up[-1] && s > up[0] && s > up[1] && s > score[i - 1] && s >= score[i + 1] && s >= dn[-1] && s >= dn[0] && s >= dn[1];
    }
    kept[i] = keep ? (unsigned short)s : (unsigned short)0;
    if (keep) atomicAdd(&hist[s], 1u);
}

// cut = {c, above, take, n}: c the highest score with (corners of score >= c) >= K, or 0 when all fit; above = corners of score > c;
// take = how many corners of score == c are kept; n = above + take.  Thread j owns the 16 bins from 4095 - 16 j downwards.
__global__ __launch_bounds__(256) void match_cut(const unsigned int* __restrict__ hist, unsigned int K, unsigned int* __restrict__ cut)
{
    __shared__ unsigned int sh[256];
    const int top = KT_MATCH_BINS - 1 - 16 * (int)threadIdx.x;
    unsigned int own[16], s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { own[k] = hist[top - k]; s += own[k]; }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned int add = threadIdx.x >= off ? sh[threadIdx.x - off] : 0u;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    const unsigned int incl = sh[threadIdx.x], total = sh[255];
    unsigned int before = incl - s;
    if (before < K && incl >= K) {   // exactly one thread, when total >= K
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (before < K && before + own[k] >= K) { cut[0] = (unsigned int)(top - k); cut[1] = before; cut[2] = K - before; cut[3] = K; }
            before += own[k];
        }
    }
    if (threadIdx.x == 0 && total < K) { cut[0] = 0u; cut[1] = total; cut[2] = 0u; cut[3] = total; }
}

// corners above / at the cut in every row: one wave per row
__global__ __launch_bounds__(64) void match_row_count(const unsigned short* __restrict__ kept, int cols, const unsigned int* __restrict__ cut, uint2* __restrict__ count)
{
    const int v = blockIdx.x, lane = threadIdx.x;
    const unsigned int c = cut[0];
    unsigned int na = 0, ne = 0;
    for (int u0 = 0; u0 < cols; u0 += 64) {
        const int u = u0 + lane;
        const unsigned int s = u < cols ? kept[(size_t)v * cols + u] : 0u;
        na += (unsigned int)__popcll(__ballot(s > c));
        ne += (unsigned int)__popcll(__ballot(s != 0u && s == c));
    }
    if (lane == 0) count[v] = make_uint2(na, ne);
}

// keys (0xFFFF - score) << 32 | raster index: the corners above the cut in raster order, then the first `take` corners at the cut
__global__ __launch_bounds__(64) void match_row_emit(const unsigned short* __restrict__ kept, int cols, const unsigned int* __restrict__ cut,
                                                     const uint2* __restrict__ offset, unsigned long long* __restrict__ keys)
{
    const int v = blockIdx.x, lane = threadIdx.x;
    const unsigned int c = cut[0], above = cut[1], take = cut[2];
    unsigned int ba = offset[v].x, be = offset[v].y;
    for (int u0 = 0; u0 < cols; u0 += 64) {
        const int u = u0 + lane;
        const unsigned int s = u < cols ? kept[(size_t)v * cols + u] : 0u;
        const bool isa = s > c, ise = s != 0u && s == c;
        const unsigned long long ma = __ballot(isa), me = __ballot(ise);
        const unsigned long long key = ((unsigned long long)(0xFFFFu - s) << 32) | (unsigned int)(v * cols + u);
        if (isa) {
            const unsigned int slot = ba + kt_wave_rank(ma, lane);
            if (slot < KT_MATCH_MAX_KP) keys[slot] = key;   // (slot < above < K <= KT_MATCH_MAX_KP by the cut's construction)
        }
        if (ise) {
            const unsigned int rank = be + kt_wave_rank(me, lane);
            if (rank < take && above + rank < KT_MATCH_MAX_KP) keys[above + rank] = key;
        }
        ba += (unsigned int)__popcll(ma);
        be += (unsigned int)__popcll(me);
    }
}

// one workgroup sorts the n keys ascending (a bitonic network over `padded`, a power of two >= n, the tail filled with all ones) and
// writes the keypoints: (u, v), score
__global__ __launch_bounds__(1024) void match_sort(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cut, int padded, int cols,
                                                   int* __restrict__ uv, int* __restrict__ score)
{
    __shared__ unsigned long long sh[KT_MATCH_MAX_KP];
    const int n = (int)min(cut[3], (unsigned int)KT_MATCH_MAX_KP);
    for (int i = threadIdx.x; i < padded; i += 1024) sh[i] = i < n ? keys[i] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= padded; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < padded; i += 1024) {
                const int p = i ^ j;
                if (p > i) {
                    const unsigned long long a = sh[i], b = sh[p];
                    if ((a > b) == ((i & k) == 0)) { sh[i] = b; sh[p] = a; }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < n; i += 1024) {
        const unsigned long long key = sh[i];
        const int idx = (int)(unsigned int)key, v = idx / cols;
        uv[2 * i] = idx - v * cols; uv[2 * i + 1] = v;
        score[i] = 0xFFFF - (int)(key >> 32);
    }
}

// one lane per keypoint: the BRIEF-256 words on the box sum, and the 3D point (kt_unproject_mm)
__global__ __launch_bounds__(64) void match_describe(const unsigned short* __restrict__ box, const unsigned short* __restrict__ depth, int cols,
                                                     const unsigned int* __restrict__ cut, const int* __restrict__ uv, kt_intr intr,
                                                     unsigned int* __restrict__ desc, float* __restrict__ xyz)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= (int)min(cut[3], (unsigned int)KT_MATCH_MAX_KP)) return;
    const int u = uv[2 * i], v = uv[2 * i + 1];
    const unsigned short* c = box + (size_t)v * cols + u;   // (the margin keeps every offset inside the box sum's valid area)
    for (int w = 0; w < 8; ++w) {
        unsigned int word = 0;
#pragma unroll 8
        for (int b = 0; b < 32; ++b) {
            const int k = 32 * w + b;
            const unsigned int sa = c[kt_brief_table[k][1] * cols + kt_brief_table[k][0]], sb = c[kt_brief_table[k][3] * cols + kt_brief_table[k][2]];
            word |= (sa < sb ? 1u : 0u) << b;
        }
        desc[8 * (size_t)i + w] = word;
    }
    const f3 p = kt_unproject_mm(u, v, depth[(size_t)v * cols + u], intr);
    xyz[3 * (size_t)i] = p.x; xyz[3 * (size_t)i + 1] = p.y; xyz[3 * (size_t)i + 2] = p.z;
}

// ---- matching ----
// One wave per 64 query descriptors against n_db descriptors (counts from device words when given).  idx = the lowest index at the
// smallest distance d1; d2 = the second smallest, duplicates counted.
__global__ __launch_bounds__(64) void match_nearest(const unsigned int* __restrict__ q, const unsigned int* __restrict__ nq_dev, int nq_arg,
                                                    const unsigned int* __restrict__ db, const unsigned int* __restrict__ ndb_dev, int ndb_arg,
                                                    int* __restrict__ out_idx, int* __restrict__ out_d1, int* __restrict__ out_d2)
{
    __shared__ __attribute__((aligned(16))) unsigned long long tile[KT_MATCH_DESC_TILE * 4];
    const int nq = nq_dev ? (int)min(*nq_dev, (unsigned int)KT_MATCH_MAX_KP) : nq_arg, ndb = ndb_dev ? (int)min(*ndb_dev, (unsigned int)KT_MATCH_MAX_KP) : ndb_arg;
    if ((int)blockIdx.x * 64 >= nq) return;   // wave-uniform
    const int lane = threadIdx.x, i = blockIdx.x * 64 + lane;
    const bool live = i < nq;
    unsigned long long a[4] = {0, 0, 0, 0};
    if (live) {
        const uint4 lo = *(const uint4*)(q + 8 * (size_t)i), hi = *(const uint4*)(q + 8 * (size_t)i + 4);
        a[0] = lo.x | ((unsigned long long)lo.y << 32); a[1] = lo.z | ((unsigned long long)lo.w << 32);
        a[2] = hi.x | ((unsigned long long)hi.y << 32); a[3] = hi.z | ((unsigned long long)hi.w << 32);
    }
    int d1 = KT_MATCH_NO_SECOND, d2 = KT_MATCH_NO_SECOND, bi = 0;
    const unsigned long long* db64 = (const unsigned long long*)db;
    for (int j0 = 0; j0 < ndb; j0 += KT_MATCH_DESC_TILE) {
        const int nt = min(KT_MATCH_DESC_TILE, ndb - j0);
        __syncthreads();   // the previous tile has been read by every lane
        for (int k = lane; k < nt * 4; k += 64) tile[k] = db64[4 * (size_t)j0 + k];
        __syncthreads();
        for (int j = 0; j < nt; ++j) {
            const ulonglong2 b0 = *(const ulonglong2*)&tile[4 * j], b1 = *(const ulonglong2*)&tile[4 * j + 2];
            const int d = (__popcll(a[0] ^ b0.x) + __popcll(a[1] ^ b0.y)) + (__popcll(a[2] ^ b1.x) + __popcll(a[3] ^ b1.y));
            if (d < d1) { d2 = d1; d1 = d; bi = j0 + j; }
            else if (d < d2) d2 = d;
        }
    }
    if (live) {
        out_idx[i] = bi; out_d1[i] = d1;
        if (out_d2) out_d2[i] = d2;
    }
}

typedef kt_accept_rule AcceptRule;   // (kt_wave.hpp: the candidate database counts by the same rule)
__device__ __forceinline__ bool match_accept(int d1, int d2, AcceptRule r) { return kt_match_accept(d1, d2, r); }

// kt_descriptor_match's output: the index, or -1 where the ratio test fails
__global__ __launch_bounds__(256) void match_apply_rule(int* __restrict__ idx, const int* __restrict__ d1, const int* __restrict__ d2, int n, AcceptRule rule)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && !match_accept(d1[i], d2[i], rule)) idx[i] = -1;
}

// One wave walks the new keypoints in order: accepted and cross-checked pairs are appended by ballot / popcount.  Per match: the pixels
// (old u, old v, new u, new v) and both 3D points.  head = {n_kp_old, n_kp_new, n_matches}.
__global__ __launch_bounds__(64) void match_pairs(const int* __restrict__ fwd_idx, const int* __restrict__ fwd_d1, const int* __restrict__ fwd_d2,
                                                  const int* __restrict__ back_idx, const unsigned int* __restrict__ cut_old, const unsigned int* __restrict__ cut_new,
                                                  AcceptRule rule, const int* __restrict__ uv_old, const int* __restrict__ uv_new, const float* __restrict__ xyz_old,
                                                  const float* __restrict__ xyz_new, int* __restrict__ m_uv, float* __restrict__ m_pn, float* __restrict__ m_po,
                                                  int* __restrict__ head)
{
    const int lane = threadIdx.x;
    const int n_old = (int)min(cut_old[3], (unsigned int)KT_MATCH_MAX_KP), n_new = (int)min(cut_new[3], (unsigned int)KT_MATCH_MAX_KP);
    unsigned int base = 0;
    if (n_old > 0)
        for (int i0 = 0; i0 < n_new; i0 += 64) {
            const int i = i0 + lane;
            bool ok = false;
            int j = 0;
            if (i < n_new) {
                j = fwd_idx[i];
                ok = match_accept(fwd_d1[i], fwd_d2[i], rule) && back_idx[j] == i;
            }
            const unsigned long long m = __ballot(ok);
            if (ok) {
                const unsigned int s = base + kt_wave_rank(m, lane);   // (s < n_new <= KT_MATCH_MAX_KP)
                m_uv[4 * s] = uv_old[2 * j]; m_uv[4 * s + 1] = uv_old[2 * j + 1]; m_uv[4 * s + 2] = uv_new[2 * i]; m_uv[4 * s + 3] = uv_new[2 * i + 1];
                for (int k = 0; k < 3; ++k) { m_pn[3 * s + k] = xyz_new[3 * i + k]; m_po[3 * s + k] = xyz_old[3 * j + k]; }
            }
            base += (unsigned int)__popcll(m);
        }
    if (lane == 0) { head[0] = n_old; head[1] = n_new; head[2] = (int)base; }
}

// ---- RANSAC ----
// one lane per hypothesis; the matches stream through LDS in tiles (a broadcast read)
__global__ __launch_bounds__(64) void match_ransac(const int* __restrict__ m_uv, const float* __restrict__ m_pn, const float* __restrict__ m_po,
                                                   const int* __restrict__ head, int n_hyp, unsigned int seed, Proj P, int* __restrict__ score)
{
    __shared__ float tx[KT_MATCH_RANSAC_TILE], ty[KT_MATCH_RANSAC_TILE], tz[KT_MATCH_RANSAC_TILE];
    __shared__ int tu[KT_MATCH_RANSAC_TILE], tv[KT_MATCH_RANSAC_TILE];
    const int lane = threadIdx.x, h = blockIdx.x * 64 + lane, m = min(head[2], KT_MATCH_MAX_KP);
    Rigid T;
    bool live = h < n_hyp && m >= 3;
    if (live) {
        unsigned int idx[3];
        match_draw(seed, (unsigned int)h, (unsigned int)m, idx);
        live = match_fit3(m_pn, m_po, idx, &T);
    }
    int count = 0;
    if (m >= 3)   // block-uniform
        for (int j0 = 0; j0 < m; j0 += KT_MATCH_RANSAC_TILE) {
            const int nt = min(KT_MATCH_RANSAC_TILE, m - j0);
            __syncthreads();
            for (int j = lane; j < nt; j += 64) {
                tx[j] = m_pn[3 * (size_t)(j0 + j)]; ty[j] = m_pn[3 * (size_t)(j0 + j) + 1]; tz[j] = m_pn[3 * (size_t)(j0 + j) + 2];
                tu[j] = m_uv[4 * (size_t)(j0 + j)]; tv[j] = m_uv[4 * (size_t)(j0 + j) + 1];
            }
            __syncthreads();
            if (live)
                for (int j = 0; j < nt; ++j) count += match_inlier(T, tx[j], ty[j], tz[j], tu[j], tv[j], P) ? 1 : 0;
        }
    if (h < n_hyp) score[h] = live ? count : 0;
}

// the highest score, ties to the lowest hypothesis: every lane over its hypotheses in ascending order, then a butterfly; best = {index, score}
__global__ __launch_bounds__(64) void match_best(const int* __restrict__ score, int n_hyp, int* __restrict__ best)
{
    int bs = -1, bi = 0x7fffffff;
    for (int h = threadIdx.x; h < n_hyp; h += 64) {
        const int s = score[h];
        if (s > bs) { bs = s; bi = h; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int os = __shfl_xor(bs, off, 64), oi = __shfl_xor(bi, off, 64);
        if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
    }
    if (threadIdx.x == 0) { best[0] = bi; best[1] = bs; }
}

}  // namespace

struct kt_match_ws {
    kt_mem mem;
    size_t pix_cap, row_cap, desc_cap;
    unsigned char* stage_host[2];       // pinned: depth (2 bytes per pixel) then rgb24, one frame each
    unsigned char* frame;               // device: the same layout (the frames pass through one after the other, in stream order)
    unsigned char* intensity;           // pix_cap
    unsigned short *score, *box, *kept; // pix_cap each
    unsigned int* hist;                 // KT_MATCH_BINS
    uint2* row;                         // row_cap
    unsigned long long* keys;           // KT_MATCH_MAX_KP
    // per frame (0: old, 1: new), KT_MATCH_MAX_KP keypoints each
    unsigned int* cut[2];               // {cut score, above, take, n}
    int *uv[2], *kp_score[2];
    unsigned int* desc[2];
    float* xyz[2];
    int *near_idx[2], *near_d1[2], *near_d2;   // 0: new -> old (with d2), 1: old -> new
    int *m_uv, *head, *hyp_score;       // matches: 4 ints each; head = {n_kp_old, n_kp_new, n_matches, best index, best score}
    float *m_pn, *m_po;
    int *head_host, *m_uv_host;         // pinned mirrors
    float *m_pn_host, *m_po_host;
    // kt_descriptor_match's own arrays, desc_cap descriptors
    unsigned int *dm_new, *dm_old;
    int *dm_idx, *dm_d1, *dm_d2;
};

int kt_match_ws_destroy(kt_match_ws* w)
{
    if (w) w->mem.release();
    delete w;
    return KT_OK;
}

static int match_ws_alloc(kt_match_ws* w)
{
    kt_mem& m = w->mem;
    const size_t K = KT_MATCH_MAX_KP;
    KT_TRY(m.pinned(&w->stage_host[0], w->pix_cap * 5)); KT_TRY(m.pinned(&w->stage_host[1], w->pix_cap * 5));
    KT_TRY(m.device(&w->frame, w->pix_cap * 5)); KT_TRY(m.device(&w->intensity, w->pix_cap));
    KT_TRY(m.device(&w->score, w->pix_cap)); KT_TRY(m.device(&w->box, w->pix_cap)); KT_TRY(m.device(&w->kept, w->pix_cap));
    KT_TRY(m.device(&w->hist, KT_MATCH_BINS)); KT_TRY(m.device(&w->row, w->row_cap)); KT_TRY(m.device(&w->keys, K));
    for (int f = 0; f < 2; ++f) {
        KT_TRY(m.device(&w->cut[f], 4)); KT_TRY(m.device(&w->uv[f], K * 2)); KT_TRY(m.device(&w->kp_score[f], K)); KT_TRY(m.device(&w->desc[f], K * 8));
        KT_TRY(m.device(&w->xyz[f], K * 3)); KT_TRY(m.device(&w->near_idx[f], K)); KT_TRY(m.device(&w->near_d1[f], K));
    }
    KT_TRY(m.device(&w->near_d2, K)); KT_TRY(m.device(&w->m_uv, K * 4)); KT_TRY(m.device(&w->head, 8)); KT_TRY(m.device(&w->hyp_score, KT_MATCH_MAX_HYP));
    KT_TRY(m.device(&w->m_pn, K * 3)); KT_TRY(m.device(&w->m_po, K * 3));
    KT_TRY(m.pinned(&w->head_host, 8)); KT_TRY(m.pinned(&w->m_uv_host, K * 4)); KT_TRY(m.pinned(&w->m_pn_host, K * 3)); KT_TRY(m.pinned(&w->m_po_host, K * 3));
    KT_TRY(m.device(&w->dm_new, w->desc_cap * 8)); KT_TRY(m.device(&w->dm_old, w->desc_cap * 8));
    KT_TRY(m.device(&w->dm_idx, w->desc_cap)); KT_TRY(m.device(&w->dm_d1, w->desc_cap));
    return m.device(&w->dm_d2, w->desc_cap);
}

// the context's workspace, for frames of `pixels` pixels / `rows` rows and kt_descriptor_match sets of `descs` descriptors; grown as
// kt_loop.hip's loop_ws_reserve grows its own
static int match_ws_reserve(kt_ctx* c, size_t pixels, size_t rows, size_t descs, kt_match_ws** out)
{
    kt_match_ws* w = c->match_ws;
    if (w && w->pix_cap >= pixels && w->row_cap >= rows && w->desc_cap >= descs) { *out = w; return KT_OK; }
    KT_HIP(hipStreamSynchronize(c->stream));
    if (!w) c->match_ws = w = new kt_match_ws();
    w->mem.release();
    w->pix_cap = std::max({w->pix_cap, pixels, (size_t)1}); w->row_cap = std::max({w->row_cap, rows, (size_t)1}); w->desc_cap = std::max({w->desc_cap, descs, (size_t)1});
    const int s = match_ws_alloc(w);
    if (s != KT_OK) { (void)kt_match_ws_destroy(w); c->match_ws = nullptr; return s; }
    *out = w;
    return KT_OK;
}

static bool match_params_ok(const kt_loop_match_params* p)
{
    return p && p->fast_threshold >= 0 && p->fast_threshold <= 255 && p->max_keypoints >= 1 && p->max_keypoints <= KT_MATCH_MAX_KP && p->max_hamming >= 0 &&
           p->max_hamming <= 256 && p->ratio_num > 0 && p->ratio_den > 0 && p->ratio_num <= 65536 && p->ratio_den <= 65536 && p->n_hypotheses >= 0 &&
           p->n_hypotheses <= KT_MATCH_MAX_HYP && p->reproj_px > 0.0f && p->max_dist > 0.0f;
}

static bool match_frame_args(const uint8_t* rgb, const uint16_t* depth, int cols, int rows)
{
    return rgb && depth && cols > 0 && rows > 0 && (long long)cols * rows < (1 << 28);
}

extern "C" int kt_loop_match_params_default(kt_loop_match_params* p)
{
    KT_ARG(p);
    p->fast_threshold = 20; p->max_keypoints = 2048; p->max_hamming = 64; p->ratio_num = 4; p->ratio_den = 5; p->n_hypotheses = 500;
    p->reproj_px = 2.0f; p->max_dist = 4.0f; p->seed = 1u;
    return KT_OK;
}

// steps a - d for one host frame, enqueued: the keypoints of slot f (cut[f][3] of them) on the device.  ONE upload.
static int match_frame(kt_ctx* c, kt_match_ws* w, const uint8_t* rgb, const uint16_t* depth, int cols, int rows, const kt_intr& intr, const kt_loop_match_params* p, int f)
{
    const size_t pixels = (size_t)cols * rows;
    hipStream_t st = c->stream;
    memcpy(w->stage_host[f], depth, pixels * 2);
    memcpy(w->stage_host[f] + pixels * 2, rgb, pixels * 3);
    KT_HIP(hipMemcpyAsync(w->frame, w->stage_host[f], pixels * 5, hipMemcpyHostToDevice, st));
    const unsigned short* depth_dev = (const unsigned short*)w->frame;
    KT_TRY(kt_bgr_to_intensity(c, w->frame + pixels * 2, w->intensity, cols, rows));
    KT_HIP(hipMemsetAsync(w->hist, 0, KT_MATCH_BINS * sizeof(unsigned int), st));
    const int nb = kt_div_up((int)pixels, 256);
    hipLaunchKernelGGL(match_score_box, dim3(nb), dim3(256), 0, st, w->intensity, cols, rows, p->fast_threshold, w->score, w->box);
    hipLaunchKernelGGL(match_nms_hist, dim3(nb), dim3(256), 0, st, w->score, depth_dev, cols, rows, p->max_dist * 1000.0f, w->kept, w->hist);
    hipLaunchKernelGGL(match_cut, dim3(1), dim3(256), 0, st, w->hist, (unsigned int)p->max_keypoints, w->cut[f]);
    hipLaunchKernelGGL(match_row_count, dim3(rows), dim3(64), 0, st, w->kept, cols, w->cut[f], w->row);
    hipLaunchKernelGGL(kt_scan_runs_kernel<2>, dim3(1), dim3(256), 0, st, (unsigned int*)w->row, rows, (unsigned int*)nullptr);
    hipLaunchKernelGGL(match_row_emit, dim3(rows), dim3(64), 0, st, w->kept, cols, w->cut[f], w->row, w->keys);
    int padded = 2;
    while (padded < p->max_keypoints) padded <<= 1;
    hipLaunchKernelGGL(match_sort, dim3(1), dim3(1024), 0, st, w->keys, w->cut[f], padded, cols, w->uv[f], w->kp_score[f]);
    hipLaunchKernelGGL(match_describe, dim3(kt_div_up(p->max_keypoints, 64)), dim3(64), 0, st, w->box, depth_dev, cols, w->cut[f], w->uv[f], intr, w->desc[f], w->xyz[f]);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

extern "C" int kt_frame_keypoints(kt_ctx* c, const uint8_t* rgb, const uint16_t* depth, int cols, int rows, const kt_loop_match_params* p, int32_t* out_uv,
                                  int32_t* out_score, uint32_t* out_desc, size_t capacity, size_t* n_out)
{
    KT_ARG(c && n_out && match_frame_args(rgb, depth, cols, rows) && match_params_ok(p) && ((out_uv && out_score && out_desc) || capacity == 0));
    *n_out = 0;
    kt_match_ws* w = nullptr;
    KT_TRY(match_ws_reserve(c, (size_t)cols * rows, (size_t)rows, 0, &w));
    const kt_intr unit = {1.0f, 1.0f, 0.0f, 0.0f};   // the 3D points are not part of this call's output
    KT_TRY(match_frame(c, w, rgb, depth, cols, rows, unit, p, 0));
    hipStream_t st = c->stream;
    KT_HIP(hipMemcpyAsync(w->head_host, w->cut[0], 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    const size_t n = (size_t)w->head_host[3];
    *n_out = n;
    if (n > capacity) { kt_set_error("kt_frame_keypoints: %zu keypoints, capacity %zu", n, capacity); return KT_ERR_CAPACITY; }
    if (n) {
        KT_HIP(hipMemcpyAsync(out_uv, w->uv[0], n * 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(out_score, w->kp_score[0], n * sizeof(int), hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(out_desc, w->desc[0], n * 8 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
    }
    return KT_OK;
}

bool kt_match_params_valid(const kt_loop_match_params* p) { return match_params_ok(p); }

// steps a - c for one host frame, enqueued on the context's stream and left on the device (kt_loopdb.hip): *desc_dev = max_keypoints x 8
// words of which the first *count_dev (a device word, <= max_keypoints) are written.  Both belong to the context's workspace: the next
// call of this file overwrites them.
int kt_match_frame_enqueue(kt_ctx* c, const uint8_t* rgb, const uint16_t* depth, int cols, int rows, const kt_loop_match_params* p, const unsigned int** desc_dev,
                           const unsigned int** count_dev)
{
    KT_ARG(c && desc_dev && count_dev && match_frame_args(rgb, depth, cols, rows) && match_params_ok(p));
    kt_match_ws* w = nullptr;
    KT_TRY(match_ws_reserve(c, (size_t)cols * rows, (size_t)rows, 0, &w));
    const kt_intr unit = {1.0f, 1.0f, 0.0f, 0.0f};   // the 3D points are not used
    KT_TRY(match_frame(c, w, rgb, depth, cols, rows, unit, p, 0));
    *desc_dev = w->desc[0]; *count_dev = w->cut[0] + 3;
    return KT_OK;
}

extern "C" int kt_descriptor_match(kt_ctx* c, const uint32_t* desc_new, size_t n_new, const uint32_t* desc_old, size_t n_old, const kt_loop_match_params* p,
                                   int32_t* out_old_index, int32_t* out_d1, int32_t* out_d2)
{
    KT_ARG(c && desc_new && desc_old && out_old_index && out_d1 && out_d2 && n_new > 0 && n_old > 0 && n_new < (1u << 24) && n_old < (1u << 24) && match_params_ok(p));
    kt_match_ws* w = nullptr;
    KT_TRY(match_ws_reserve(c, 0, 0, n_new > n_old ? n_new : n_old, &w));
    hipStream_t st = c->stream;
    KT_HIP(hipMemcpyAsync(w->dm_new, desc_new, n_new * 8 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    KT_HIP(hipMemcpyAsync(w->dm_old, desc_old, n_old * 8 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(match_nearest, dim3(kt_div_up((int)n_new, 64)), dim3(64), 0, st, w->dm_new, (const unsigned int*)nullptr, (int)n_new, w->dm_old,
                       (const unsigned int*)nullptr, (int)n_old, w->dm_idx, w->dm_d1, w->dm_d2);
    const AcceptRule rule = {p->max_hamming, p->ratio_num, p->ratio_den};
    hipLaunchKernelGGL(match_apply_rule, dim3(kt_div_up((int)n_new, 256)), dim3(256), 0, st, w->dm_idx, w->dm_d1, w->dm_d2, (int)n_new, rule);
    KT_LAUNCH_CHECK();
    KT_HIP(hipMemcpyAsync(out_old_index, w->dm_idx, n_new * sizeof(int), hipMemcpyDeviceToHost, st));
    KT_HIP(hipMemcpyAsync(out_d1, w->dm_d1, n_new * sizeof(int), hipMemcpyDeviceToHost, st));
    KT_HIP(hipMemcpyAsync(out_d2, w->dm_d2, n_new * sizeof(int), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    return KT_OK;
}

// the projection of step f: the kt_intr floats widened to double, the squared threshold in double
static Proj match_proj(const kt_intr& intr, float reproj_px)
{
    Proj P;
    P.fx = (double)intr.fx; P.fy = (double)intr.fy; P.cx = (double)intr.cx; P.cy = (double)intr.cy; P.thr2 = (double)reproj_px * (double)reproj_px;
    return P;
}

// step f, enqueued: the score of every hypothesis over the workspace's match list (head[2] matches) -> hyp_score, the winner -> head[3..4]
static void match_ransac_enqueue(kt_ctx* c, kt_match_ws* w, int nh, unsigned int seed, const Proj& P)
{
    hipLaunchKernelGGL(match_ransac, dim3(kt_div_up(nh, 64)), dim3(64), 0, c->stream, w->m_uv, w->m_pn, w->m_po, w->head, nh, seed, P, w->hyp_score);
    hipLaunchKernelGGL(match_best, dim3(1), dim3(64), 0, c->stream, w->hyp_score, nh, w->head + 3);
}

// test hook (kt_debug.h): step f on a caller's match list
extern "C" int kt_debug_match_ransac(kt_ctx* c, const int32_t* m_uv, const float* m_pn, const float* m_po, int m, int n_hyp, unsigned int seed, const kt_intr* intr,
                                     float reproj_px, int32_t* out_score, int32_t* out_best)
{
    KT_ARG(c && intr && intr->fx != 0.0f && intr->fy != 0.0f && reproj_px > 0.0f && out_score && out_best && m >= 0 && m <= KT_MATCH_MAX_KP && n_hyp >= 1 &&
           n_hyp <= KT_MATCH_MAX_HYP && ((m_uv && m_pn && m_po) || m == 0));
    kt_match_ws* w = nullptr;
    KT_TRY(match_ws_reserve(c, 0, 0, 0, &w));
    hipStream_t st = c->stream;
    KT_HIP(hipStreamSynchronize(st));   // the pinned mirrors are free
    w->head_host[0] = w->head_host[1] = w->head_host[2] = m;
    KT_HIP(hipMemcpyAsync(w->head, w->head_host, 3 * sizeof(int), hipMemcpyHostToDevice, st));
    if (m) {
        memcpy(w->m_uv_host, m_uv, (size_t)m * 4 * sizeof(int)); memcpy(w->m_pn_host, m_pn, (size_t)m * 3 * sizeof(float)); memcpy(w->m_po_host, m_po, (size_t)m * 3 * sizeof(float));
        KT_HIP(hipMemcpyAsync(w->m_uv, w->m_uv_host, (size_t)m * 4 * sizeof(int), hipMemcpyHostToDevice, st));
        KT_HIP(hipMemcpyAsync(w->m_pn, w->m_pn_host, (size_t)m * 3 * sizeof(float), hipMemcpyHostToDevice, st));
        KT_HIP(hipMemcpyAsync(w->m_po, w->m_po_host, (size_t)m * 3 * sizeof(float), hipMemcpyHostToDevice, st));
    }
    match_ransac_enqueue(c, w, n_hyp, seed, match_proj(*intr, reproj_px));
    KT_LAUNCH_CHECK();
    KT_HIP(hipMemcpyAsync(out_score, w->hyp_score, (size_t)n_hyp * sizeof(int), hipMemcpyDeviceToHost, st));
    KT_HIP(hipMemcpyAsync(w->head_host, w->head, 5 * sizeof(int), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    out_best[0] = w->head_host[3]; out_best[1] = w->head_host[4];
    return KT_OK;
}

extern "C" int kt_loop_match_frames(kt_ctx* c, const uint8_t* rgb_old, const uint16_t* depth_old, const uint8_t* rgb_new, const uint16_t* depth_new, int cols, int rows,
                                    const kt_intr* intr, const kt_loop_match_params* p, float out_pose[16], float out_bootstrap[16], int32_t* out_matches,
                                    uint8_t* out_inlier, size_t match_capacity, kt_loop_match_info* out_info)
{
    KT_ARG(c && match_frame_args(rgb_old, depth_old, cols, rows) && rgb_new && depth_new && intr && intr->fx != 0.0f && intr->fy != 0.0f && match_params_ok(p) &&
           out_pose && out_bootstrap && out_info && ((out_matches && out_inlier) || match_capacity == 0));
    kt_match_ws* w = nullptr;
    KT_TRY(match_ws_reserve(c, (size_t)cols * rows, (size_t)rows, 0, &w));
    hipStream_t st = c->stream;
    KT_TRY(match_frame(c, w, rgb_old, depth_old, cols, rows, *intr, p, 0));
    KT_TRY(match_frame(c, w, rgb_new, depth_new, cols, rows, *intr, p, 1));
    const int K = p->max_keypoints, kb = kt_div_up(K, 64), nh = p->n_hypotheses;
    // new -> old with the second distance, old -> new for the cross-check
    hipLaunchKernelGGL(match_nearest, dim3(kb), dim3(64), 0, st, w->desc[1], w->cut[1] + 3, 0, w->desc[0], w->cut[0] + 3, 0, w->near_idx[0], w->near_d1[0], w->near_d2);
    hipLaunchKernelGGL(match_nearest, dim3(kb), dim3(64), 0, st, w->desc[0], w->cut[0] + 3, 0, w->desc[1], w->cut[1] + 3, 0, w->near_idx[1], w->near_d1[1], (int*)nullptr);
    const AcceptRule rule = {p->max_hamming, p->ratio_num, p->ratio_den};
    hipLaunchKernelGGL(match_pairs, dim3(1), dim3(64), 0, st, w->near_idx[0], w->near_d1[0], w->near_d2, w->near_idx[1], w->cut[0], w->cut[1], rule, w->uv[0], w->uv[1],
                       w->xyz[0], w->xyz[1], w->m_uv, w->m_pn, w->m_po, w->head);
    const Proj P = match_proj(*intr, p->reproj_px);
    if (nh > 0) match_ransac_enqueue(c, w, nh, p->seed, P);
    KT_LAUNCH_CHECK();
    // one round trip: the counts, the winner and the match arrays (max_keypoints bounds the matches)
    KT_HIP(hipMemcpyAsync(w->head_host, w->head, 5 * sizeof(int), hipMemcpyDeviceToHost, st));
    KT_HIP(hipMemcpyAsync(w->m_uv_host, w->m_uv, (size_t)K * 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    KT_HIP(hipMemcpyAsync(w->m_pn_host, w->m_pn, (size_t)K * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    KT_HIP(hipMemcpyAsync(w->m_po_host, w->m_po, (size_t)K * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    const int m = w->head_host[2];
    out_info->n_kp_old = w->head_host[0]; out_info->n_kp_new = w->head_host[1]; out_info->n_matches = m; out_info->n_inliers = 0; out_info->best_hypothesis = -1;
    if ((size_t)m > match_capacity) { kt_set_error("kt_loop_match_frames: %d matches, capacity %zu", m, match_capacity); return KT_ERR_CAPACITY; }
    for (int k = 0; k < 16; ++k) out_pose[k] = out_bootstrap[k] = (k % 5 == 0) ? 1.0f : 0.0f;
    if (m) memcpy(out_matches, w->m_uv_host, (size_t)m * 4 * sizeof(int));
    if (m) memset(out_inlier, 0, (size_t)m);
    if (m < 3 || nh < 1 || w->head_host[4] < 3) return KT_OK;
    // the winner's fit and inliers again on the host (the same double arithmetic), the refit over them, one more scoring
    const int best = w->head_host[3];
    const float *pn = w->m_pn_host, *po = w->m_po_host;
    const int* uv = w->m_uv_host;
    unsigned int idx[3];
    Rigid T;
    match_draw(p->seed, (unsigned int)best, (unsigned int)m, idx);
    if (!match_fit3(pn, po, idx, &T)) { kt_set_error("kt_loop_match_frames: the winning hypothesis is degenerate on the host"); return KT_ERR_STATE; }
    double sums[15], n = 0.0;
    for (int k = 0; k < 15; ++k) sums[k] = 0.0;
    for (int j = 0; j < m; ++j) {
        if (!match_inlier(T, pn[3 * j], pn[3 * j + 1], pn[3 * j + 2], uv[4 * j], uv[4 * j + 1], P)) continue;
        const double s[3] = {pn[3 * j], pn[3 * j + 1], pn[3 * j + 2]}, t[3] = {po[3 * j], po[3 * j + 1], po[3 * j + 2]};
        double term[15];
        kt_rigid_terms(s, t, term);
        for (int k = 0; k < 15; ++k) sums[k] += term[k];
        n += 1.0;
    }
    double M[16];
    KT_TRY(kt_host_rigid_fit(sums, n, M));
    for (int a = 0; a < 3; ++a) { T.R[3 * a] = M[4 * a]; T.R[3 * a + 1] = M[4 * a + 1]; T.R[3 * a + 2] = M[4 * a + 2]; T.t[a] = M[4 * a + 3]; }
    int inliers = 0;
    for (int j = 0; j < m; ++j) {
        const bool in = match_inlier(T, pn[3 * j], pn[3 * j + 1], pn[3 * j + 2], uv[4 * j], uv[4 * j + 1], P);
        out_inlier[j] = in ? 1 : 0;
        inliers += in ? 1 : 0;
    }
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) { out_pose[4 * a + b] = (float)T.R[3 * a + b]; out_bootstrap[4 * a + b] = (float)T.R[3 * b + a]; }
        out_pose[4 * a + 3] = (float)T.t[a];
        out_bootstrap[4 * a + 3] = (float)(-((T.R[a] * T.t[0] + T.R[3 + a] * T.t[1]) + T.R[6 + a] * T.t[2]));
    }
    out_info->n_inliers = inliers; out_info->best_hypothesis = best;
    return KT_OK;
}
