// kt_wave.hpp -- wave and workgroup primitives of the side stages (kt_slice.hip, kt_mesh.hip, kt_mesh_weld.hip, kt_mesh_simplify.hip,
// kt_mesh_normals.hip, kt_mesh_components.hip, kt_mesh_holes.hip, kt_mesh_smooth.hip, kt_mesh_render.hip, kt_loop.hip, kt_match.hip, kt_loopdb.hip,
// kt_posegraph.hip, kt_deform.hip), and the device rules that the passes over the -m mesh share: the runs of a sorted key list and their heads
// kernel, the half-edge key and the class of a run of half-edges, the vertex validity rule and the 32.32 fixed point.  A new side stage
// uses these instead of a copy; the mesh post-passes' shared host code is kt_mesh_pass.hpp, their sorted key list kt_mesh_keys.hpp, their
// union-find and its flatten kernel kt_unionfind.hpp.  The operation order of each is part of the stages' bit-exact contracts: do not reorder.
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

// inclusive prefix sum over the lanes of a wave (int, unsigned)
template <class T>
__device__ __forceinline__ T kt_wave_incl(T v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T u = __shfl_up(v, off, 64);
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

// hp[j] = j where sorted entry j starts a run, else 0: the first of its key, or one that the rule splits from the entry before it.  GATED
// (the weld): their spans' times lie further apart than max_gap; max_gap == ~0 is no gate, and no table is read at all.  Not GATED (the
// simplification): their spans differ; one span needs no search.  A workgroup takes CHUNK entries and stages the table in LDS once for
// them, the times beside the firsts only where GATED (24 KB against 8 KB); a table of more than KT_RUNS_LDS_SPANS spans is searched in
// global memory.  time and max_gap are not read unless GATED
#define KT_RUNS_LDS_SPANS 2048
template <int LANES, int CHUNK, bool GATED>
__global__ __launch_bounds__(LANES) void kt_runs_heads_kernel(const unsigned long long* __restrict__ sk, const unsigned int* __restrict__ si, unsigned int n,
                                                              const unsigned int* __restrict__ first, const unsigned long long* __restrict__ time, int S,
                                                              unsigned long long max_gap, unsigned int* __restrict__ hp)
{
    __shared__ unsigned int lf[KT_RUNS_LDS_SPANS];
    __shared__ unsigned long long lt[GATED ? KT_RUNS_LDS_SPANS : 1];   // (never named unless GATED: no LDS is taken for it)
    const bool search = GATED ? max_gap != ~0ull : S > 1;
    const bool staged = search && S <= KT_RUNS_LDS_SPANS;
    if (staged) {
        for (int s = threadIdx.x; s < S; s += LANES) {
            lf[s] = first[s];
            if constexpr (GATED) lt[s] = time[s];
        }
        __syncthreads();
    }
    const unsigned int* f = staged ? lf : first;
    const unsigned long long* t = time;
    if constexpr (GATED) t = staged ? lt : time;
    const size_t base = (size_t)blockIdx.x * CHUNK + threadIdx.x;
    for (int k = 0; k < CHUNK / LANES; ++k) {
        const size_t j = base + (size_t)k * LANES;
        if (j >= n) break;
        bool head = j == 0 || sk[j] != sk[j - 1];
        if (!head && search) {
            if constexpr (GATED) {
                const unsigned long long ta = t[kt_span_of(f, S, si[j])], tb = t[kt_span_of(f, S, si[j - 1])];
                head = (ta > tb ? ta - tb : tb - ta) > max_gap;
            } else head = kt_span_of(f, S, si[j]) != kt_span_of(f, S, si[j - 1]);
        }
        hp[j] = head ? (unsigned int)j : 0u;
    }
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

// the other end of half-edge h
__device__ __forceinline__ unsigned int kt_half_edge_next(const unsigned int* __restrict__ tri, unsigned int h)
{
    const unsigned int t3 = h - h % 3u;
    return tri[h + 1u - t3 == 3u ? t3 : h + 1u];
}

// The class of entry j of the sorted list (sk, sh) of the m3 half-edge keys of tri (kt_mesh_keys.hpp): an undirected edge is the run of
// its key, and the head of the run answers for it.  The lane reads its predecessor and its two followers
#define KT_HE_NONE 0                  // no head, or no key
#define KT_HE_BOUNDARY 1              // a run of one
#define KT_HE_INTERIOR 2              // a run of exactly two, exactly one of which runs min -> max
#define KT_HE_NONMANIFOLD 3           // any other head
__device__ __forceinline__ int kt_half_edge_class(const unsigned long long* __restrict__ sk, const unsigned int* __restrict__ sh, const unsigned int* __restrict__ tri,
                                                  size_t j, unsigned int m3)
{
    const unsigned long long k = sk[j];
    if (k == KT_NO_HALF_EDGE || (j != 0 && sk[j - 1] == k)) return KT_HE_NONE;
    if (!(j + 1 < m3 && sk[j + 1] == k)) return KT_HE_BOUNDARY;
    const bool three = j + 2 < m3 && sk[j + 2] == k;
    const unsigned int lo = (unsigned int)(k >> 32);
    return !three && (tri[sh[j]] == lo) != (tri[sh[j + 1]] == lo) ? KT_HE_INTERIOR : KT_HE_NONMANIFOLD;
}

// ---- a vertex of the -m mesh (16 bytes: three floats and a colour word) is valid when every |coordinate| < 8192: false for a NaN and for
// an infinity.  The rule of every pass that computes with positions (simplify, normals, holes, smooth, render) ----
__device__ __forceinline__ bool kt_mesh_valid_coord(float x) { return fabsf(x) < 8192.0f; }
__device__ __forceinline__ bool kt_mesh_valid(const uint4 p)
{
    return kt_mesh_valid_coord(__uint_as_float(p.x)) && kt_mesh_valid_coord(__uint_as_float(p.y)) && kt_mesh_valid_coord(__uint_as_float(p.z));
}

// 32.32 fixed point of a coordinate, and back: q = rint((double)x * 2^32) as int64, x = (float)((double)q * 2^-32).  __double2ll_rn
// rounds to nearest even like rint, and the two agree wherever the result fits an int64: |q| < 2^45 for a valid coordinate
__device__ __forceinline__ long long kt_q32(float x) { return __double2ll_rn((double)x * 4294967296.0); }
__device__ __forceinline__ float kt_q32_float(long long q) { return (float)((double)q * (1.0 / 4294967296.0)); }

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
