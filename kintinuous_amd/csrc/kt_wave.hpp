// kt_wave.hpp -- wave and workgroup primitives of the side stages (kt_slice.hip, kt_mesh.hip, kt_mesh_weld.hip, kt_mesh_simplify.hip,
// kt_mesh_components.hip, kt_mesh_holes.hip, kt_mesh_smooth.hip, kt_mesh_render.hip, kt_loop.hip, kt_match.hip, kt_loopdb.hip, kt_posegraph.hip, kt_deform.hip).  A new side stage
// uses these instead of a copy; the mesh post-passes' shared host code is kt_mesh_pass.hpp, their union-find and its flatten kernel
// kt_unionfind.hpp.  The operation order of each is part of the stages' bit-exact contracts: do not reorder.
#pragma once

#include "kt_common.hpp"

// sum over the 64 lanes, in every lane: the xor butterfly 32, 16, ..., 1 (int, unsigned, double -- whose sums depend on this order)
template <class T>
__device__ __forceinline__ T kt_wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// inclusive prefix sum over the lanes of a wave
__device__ __forceinline__ int kt_wave_incl(int v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(v, off, 64);
        if (lane >= off) v += u;
    }
    return v;
}

// a lane's rank among the set bits of a ballot: how many lanes below it voted
__device__ __forceinline__ unsigned int kt_wave_rank(unsigned long long ballot, int lane)
{
    return (unsigned int)__popcll(ballot & ((1ull << lane) - 1ull));
}

// Exclusive scan, in place, of n items of W interleaved counters each (count[W * i + k]; a uint2 array is a W = 2 array) by ONE
// workgroup of 256 threads: every thread owns a run of ceil(n / 256) consecutive items.  The W totals go to total[0 .. W) when given.
template <int W>
__global__ __launch_bounds__(256) void kt_scan_runs_kernel(unsigned int* __restrict__ count, int n, unsigned int* __restrict__ total)
{
    __shared__ unsigned int sh[W][256];
    const int per = (n + 255) / 256, i0 = threadIdx.x * per, i1 = min(n, i0 + per);
    unsigned int s[W] = {}, base[W];
    for (int i = i0; i < i1; ++i)
        for (int k = 0; k < W; ++k) s[k] += count[W * i + k];
    for (int k = 0; k < W; ++k) sh[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        unsigned int add[W];
        for (int k = 0; k < W; ++k) add[k] = threadIdx.x >= off ? sh[k][threadIdx.x - off] : 0u;
        __syncthreads();
        for (int k = 0; k < W; ++k) sh[k][threadIdx.x] += add[k];
        __syncthreads();
    }
    for (int k = 0; k < W; ++k) base[k] = sh[k][threadIdx.x] - s[k];
    for (int i = i0; i < i1; ++i)
        for (int k = 0; k < W; ++k) { const unsigned int c = count[W * i + k]; count[W * i + k] = base[k]; base[k] += c; }
    if (total && threadIdx.x == 255)
        for (int k = 0; k < W; ++k) total[k] = sh[k][255];
}

// ---- runs of a sorted (key, index) list, back in input order: what the seam weld (kt_mesh_weld.hip) and the simplification
// (kt_mesh_simplify.hip) share.  si: the sorted indices; hps[j]: the sorted position of the head of entry j's run; rep[i]: the head
// (first vertex) of vertex i's run; a vertex is kept when rep[i] == i; newidx[i]: the kept vertices below i. ----
#define KT_RUNS_PER_WAVE 256          // vertices per wave of the count pass and of the passes that rank the kept vertices

// the span of vertex i: the last s in [0, S) with first[s] <= i (first[0] = 0; empty spans share their first entry with the next span)
__device__ __forceinline__ int kt_span_of(const unsigned int* first, int S, unsigned int i)
{
    int lo = 0, hi = S;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

template <int LANES>
__global__ __launch_bounds__(LANES) void kt_runs_reps_kernel(const unsigned int* __restrict__ si, const unsigned int* __restrict__ hps, unsigned int n,
                                                             unsigned int* __restrict__ rep)
{
    const size_t j = (size_t)blockIdx.x * LANES + threadIdx.x;
    if (j < n) rep[si[j]] = si[hps[j]];
}

template <int LANES>
__global__ __launch_bounds__(LANES) void kt_runs_count_kernel(const unsigned int* __restrict__ rep, unsigned int n, unsigned int* __restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * (LANES / 64) + (threadIdx.x >> 6);
    const size_t base = w * KT_RUNS_PER_WAVE;
    if (base >= n) return;   // wave-uniform
    unsigned int c = 0;
#pragma unroll
    for (int k = 0; k < KT_RUNS_PER_WAVE / 64; ++k) {
        const size_t i = base + 64 * k + lane;
        c += (unsigned int)__popcll(__ballot(i < n && rep[i] == (unsigned int)i));
    }
    if (lane == 0) cnt[w] = c;
}

// newidx[i] = the kept vertices below i, from the scanned counts of kt_runs_count_kernel (kt_mesh_components.hip, kt_mesh_holes.hip)
template <int LANES>
__global__ __launch_bounds__(LANES) void kt_runs_rank_kernel(const unsigned int* __restrict__ rep, unsigned int n, const unsigned int* __restrict__ cnt,
                                                             unsigned int* __restrict__ newidx)
{
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * (LANES / 64) + (threadIdx.x >> 6);
    const size_t base = w * KT_RUNS_PER_WAVE;
    if (base >= n) return;   // wave-uniform
    unsigned int o = cnt[w];
#pragma unroll
    for (int k = 0; k < KT_RUNS_PER_WAVE / 64; ++k) {
        const size_t i = base + 64 * k + lane;
        const unsigned long long b = __ballot(i < n && rep[i] == (unsigned int)i);
        if (i < n) newidx[i] = o + kt_wave_rank(b, lane);
        o += (unsigned int)__popcll(b);
    }
}

template <int LANES>
__global__ __launch_bounds__(LANES) void kt_runs_spans_kernel(const unsigned int* __restrict__ first, int S1, unsigned int n, const unsigned int* __restrict__ newidx,
                                                              const unsigned int* __restrict__ total, unsigned int* __restrict__ first_out)
{
    const int s = blockIdx.x * LANES + threadIdx.x;
    if (s < S1) first_out[s] = first[s] < n ? newidx[first[s]] : *total;
}

// rep[i] becomes the new index of i's representative, in place (lane i alone reads and writes rep[i]): a remap then costs one gather
// per index instead of two that depend on each other
template <int LANES>
__global__ __launch_bounds__(LANES) void kt_runs_map_kernel(unsigned int* __restrict__ rep, const unsigned int* __restrict__ newidx, unsigned int n)
{
    const size_t i = (size_t)blockIdx.x * LANES + threadIdx.x;
    if (i < n) rep[i] = newidx[rep[i]];
}

// ---- half-edges of a triangle list (kt_mesh_holes.hip, kt_mesh_smooth.hip): triangle t, corner k gives half-edge h = 3 t + k from
// a = tri[t][k] to b = tri[t][(k + 1) % 3].  Its key is min(a, b) << 32 | max(a, b), the same for both directions of an undirected edge;
// a triangle with two equal indices (degenerate) or with an index >= n (bad) has no half-edges: its three keys are KT_NO_HALF_EDGE, which
// sorts last.  h < 3 m; only the triangle's own three indices are read ----
#define KT_NO_HALF_EDGE (~0ull)
__device__ __forceinline__ unsigned long long kt_half_edge_key(const unsigned int* __restrict__ tri, unsigned int h, unsigned int n, bool* bad, bool* degenerate)
{
    const unsigned int t3 = h - h % 3u;
    const unsigned int i0 = tri[t3], i1 = tri[t3 + 1], i2 = tri[t3 + 2];
    *bad = i0 >= n || i1 >= n || i2 >= n;
    *degenerate = i0 == i1 || i1 == i2 || i0 == i2;
    const unsigned int a = h == t3 ? i0 : h == t3 + 1 ? i1 : i2, b = h == t3 ? i1 : h == t3 + 1 ? i2 : i0;
    return *bad || *degenerate ? KT_NO_HALF_EDGE : (unsigned long long)min(a, b) << 32 | (unsigned long long)max(a, b);
}

// DepthCamera.cpp:151-157 in float: the point of pixel (u, v) at d millimetres
__device__ __forceinline__ f3 kt_unproject_mm(int u, int v, unsigned short d, const kt_intr& k)
{
    const float z = (float)d * 0.001f;
    return {((float)u - k.cx) * z * (1.0f / k.fx), ((float)v - k.cy) * z * (1.0f / k.fy), z};
}

// descriptor matching (kt_match.hip's match_nearest, kt_loopdb.hip's loopdb_score): the limits of a descriptor list and the acceptance rule
#define KT_MATCH_MAX_KP 4096                      // max_keypoints' limit: the sort's LDS array
#define KT_MATCH_DESC_TILE 512                    // descriptors per LDS tile (16 KB)
#define KT_MATCH_NO_SECOND 257                    // d2 when there is one descriptor to match against
struct kt_accept_rule { int max_hamming, ratio_num, ratio_den; };
__device__ __forceinline__ bool kt_match_accept(int d1, int d2, kt_accept_rule r) { return d1 <= r.max_hamming && r.ratio_den * d1 < r.ratio_num * d2; }

// one pair's 15 terms of the rigid fit's sums (kt_host_rigid_fit): s, t, s t^T row-major
__host__ __device__ inline void kt_rigid_terms(const double s[3], const double t[3], double term[15])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        term[a] = s[a]; term[3 + a] = t[a];
#pragma unroll
        for (int b = 0; b < 3; ++b) term[6 + 3 * a + b] = s[a] * t[b];
    }
}
