// kt_mesh_smooth.hip -- Taubin's lambda|mu smoothing of the -m mesh (kt_mesh_smooth, kt_mesh_smooth_device).
//
// Not in the reference: its -m meshes a cloud that was voxel-filtered and given 20-NN normals (backend/MeshGenerator.cpp), so its surface
// is smooth before it is a mesh.  A vertex of kt_mesh.hip sits where a noisy, quantised TSDF crosses zero along one voxel edge, and no
// pass of the chain removes that noise.  This one low-pass filters the vertex positions over the mesh's own edges: a half-step with
// factor lambda shrinks, the one with the negative factor mu behind it grows again (G. Taubin, "A signal processing approach to fair
// surface design", SIGGRAPH 1995).  No vertex is added, dropped or renumbered: triangles and span tables stay as they are.
//
// Semantics (include/kt_abi.h; restated in numpy by kintinuous_amd/mesh_smooth_ref.py, which the device equals on every byte, on every
// call):
//   - half-edges and their keys are kt_wave.hpp's (the hole pass reads the same): a triangle with two equal indices has none, an index >= n
//     fails the call;
//   - an undirected edge with exactly one half-edge each way is interior, any other rim; a vertex is rim when it ends a rim edge; an edge
//     counts once however many triangles hold it (uniform umbrella weights);
//   - neighbours: an interior vertex has the other ends of all its edges; a rim vertex has none with mode 0 and the other ends of its rim
//     edges with mode 1; d = their number, d > 65535 fails the call, d = 0 leaves the vertex alone;
//   - a vertex that ends a half-edge must be valid (finite, |coordinate| < 8192), or the call fails;
//   - q = rint((double)x * 2^32) as int64; a half-step with factor f: S = the int64 sum of the neighbours' q before the half-step,
//     D = S - d q, q' = q + (int64)rint(f * ((double)D / (double)d)); |q'| >= 2^45 fails the call; a step is lambda, then mu;
//   - output: a vertex with d = 0 (and every vertex when steps = 0) keeps its 16 bytes, any other gets (float)((double)q * 2^-32).
//
// The passes, all on the object's stream:
//   memset    flag, degree, cursor and the four result words
//   keys      one lane per half-edge: key = min << 32 | max, all ones for a degenerate triangle or one with an index >= n (which ORs a
//             bit into the status word)
//   sort      the sorted key list (kt_mesh_keys.hpp) of (key, h)
//   classify  grid-stride, at most KT_SMO_COUNT_BLOCKS workgroups; a lane per sorted entry takes its class from kt_half_edge_class
//             (kt_wave.hpp): an interior edge stays one, a boundary or non-manifold edge is a rim edge; the class goes into a byte
//             per entry, REFERENCED (and RIM) into the flags of both ends; the heads are counted by ballot, one atomic per wave
//   degree    one lane per sorted entry: a head adds one to the degree of each end that takes the other as a neighbour
//   rows      off[v] = the sum of the degrees below v: a wave sums 256 degrees, kt_scan_runs_kernel<1> scans the waves' sums, a wave
//             scans its 256 degrees
//   fill      as degree: nbr[off[a] + cursor[a]++] = b.  The order inside a row depends on the order of arrival; only integer sums read
//             a row, so the result does not
//   init      grid-stride like classify, a lane per vertex: q into three planes of int64; an invalid referenced vertex and a degree
//             over the bound OR their bits into the status word and get d = 0; the rim vertices and the ones that can move are counted
//             by ballot
//   step      2 * steps launches, one lane per vertex: gathers the d neighbours' q from the planes before the half-step, writes its own
//             q' (or q when d = 0) to the other planes.  No atomics, no float additions; a lane waits for no other
//   finish    one lane per vertex: nothing when the status word is set; otherwise 16 bytes, converted or copied
// then the four result words go to pinned memory and the host waits once.
// Loops without a compile-time trip count: the step's gather runs d <= 65535 times, a bound smo_init enforces before the first step;
// the grid-stride loops of classify and init advance by the grid's stride > 0 per round.
// The workspace: 64 bytes per vertex (two states of 24 bytes, degree, offset, flags, cursor) and 4 per 256 vertices, 29 bytes per
// half-edge (two keys, the sorted half-edge, two neighbour entries, a class byte) and the sort's own.
#include "kt_mesh_keys.hpp"
#include "kt_wave.hpp"

#define KT_SMO_LANES 256
#define KT_SMO_PER_WAVE KT_RUNS_PER_WAVE   // vertices per wave of the rows passes
#define KT_SMO_MAX_VERTICES ((size_t)1 << 29)
#define KT_SMO_MAX_TRIANGLES ((size_t)1 << 29)
#define KT_SMO_MAX_STEPS 64
#define KT_SMO_MAX_VALENCE 65535u
#define KT_SMO_RANGE (1ll << 45)      // |q| stays below it: 8192 m in units of 2^-32 m
#define KT_SMO_INTERIOR 1             // the class of a sorted entry: 0 for one that is no head
#define KT_SMO_RIM_EDGE 2
#define KT_SMO_RIM 1u                 // flag[v]: v ends a rim edge
#define KT_SMO_REFERENCED 2u          // flag[v]: v ends a half-edge
#define KT_SMO_COUNT_BLOCKS 2048      // of the grid-stride passes that count (classify, init): a wave adds its counts once, at the end
#define KT_SMO_RES 4                  // the result words: status, rim vertices, moved vertices, unique edges
#define KT_SMO_BAD_INDEX 1u           // the bits of the status word
#define KT_SMO_BAD_VERTEX 2u
#define KT_SMO_BAD_VALENCE 4u
#define KT_SMO_LEFT_RANGE 8u

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;
typedef unsigned char u8;

__global__ __launch_bounds__(KT_SMO_LANES) void smo_keys(const u32* __restrict__ tri, u32 m3, u32 n, u64* __restrict__ keys, u32* __restrict__ res)
{
    const size_t h = (size_t)blockIdx.x * KT_SMO_LANES + threadIdx.x;
    if (h >= m3) return;
    bool bad, deg;
    keys[h] = kt_half_edge_key(tri, (u32)h, n, &bad, &deg);   // (kt_wave.hpp: the hole pass's keys)
    if (bad && (u32)h % 3u == 0u) atomicOr(res, KT_SMO_BAD_INDEX);
}

// res[3]: the unique edges
__global__ __launch_bounds__(KT_SMO_LANES) void smo_classify(const u64* __restrict__ sk, const u32* __restrict__ sh, u32 m3, const u32* __restrict__ tri,
                                                             u8* __restrict__ ec, u32* __restrict__ flag, u32* __restrict__ res)
{
    const int lane = threadIdx.x & 63;
    const size_t stride = (size_t)gridDim.x * KT_SMO_LANES;
    u32 edges = 0;   // of this wave, over its rounds
    for (size_t base = (size_t)blockIdx.x * KT_SMO_LANES + threadIdx.x - lane; base < m3; base += stride) {   // wave-uniform; ceil(3 m / stride) rounds
        const size_t j = base + lane;
        int c = 0;
        if (j < m3) {
            const int he = kt_half_edge_class(sk, sh, tri, j, m3);   // (kt_wave.hpp)
            if (he != KT_HE_NONE) {                                    // the head of a run
                const u64 k = sk[j];
                const u32 lo = (u32)(k >> 32), hi = (u32)k;             // (both below n: the key is one)
                c = he == KT_HE_INTERIOR ? KT_SMO_INTERIOR : KT_SMO_RIM_EDGE;
                const u32 f = c == KT_SMO_RIM_EDGE ? KT_SMO_REFERENCED | KT_SMO_RIM : KT_SMO_REFERENCED;
                atomicOr(flag + lo, f);
                atomicOr(flag + hi, f);
            }
            ec[j] = (u8)c;
        }
        edges += (u32)__popcll(__ballot(c != 0));
    }
    if (lane == 0 && edges) atomicAdd(res + 3, edges);   // (one word for every wave: a wave per 64 entries adding here took most of the pass)
}

// whether a vertex with these flags takes the other end of an edge of class c as a neighbour
__device__ __forceinline__ bool smo_takes(u32 f, int c, int mode) { return !(f & KT_SMO_RIM) || (c == KT_SMO_RIM_EDGE && mode == 1); }

__global__ __launch_bounds__(KT_SMO_LANES) void smo_degree(const u64* __restrict__ sk, const u8* __restrict__ ec, u32 m3, const u32* __restrict__ flag, int mode,
                                                           u32* __restrict__ deg)
{
    const size_t j = (size_t)blockIdx.x * KT_SMO_LANES + threadIdx.x;
    if (j >= m3) return;
    const int c = ec[j];
    if (!c) return;
    const u64 k = sk[j];
    const u32 lo = (u32)(k >> 32), hi = (u32)k;
    if (smo_takes(flag[lo], c, mode)) atomicAdd(deg + lo, 1u);
    if (smo_takes(flag[hi], c, mode)) atomicAdd(deg + hi, 1u);
}

// cnt[w] = the sum of wave w's KT_SMO_PER_WAVE degrees (below 2^32: at most two entries per half-edge, 3 m <= 3 * 2^29)
__global__ __launch_bounds__(KT_SMO_LANES) void smo_rows_count(const u32* __restrict__ deg, u32 n, u32* __restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * (KT_SMO_LANES / 64) + (threadIdx.x >> 6);
    const size_t base = w * KT_SMO_PER_WAVE;
    if (base >= n) return;   // wave-uniform
    u32 c = 0;
#pragma unroll
    for (int k = 0; k < KT_SMO_PER_WAVE / 64; ++k) {
        const size_t i = base + 64 * k + lane;
        c += i < n ? deg[i] : 0u;
    }
    c = kt_wave_sum(c);
    if (lane == 0) cnt[w] = c;
}

// off[i] = the degrees below i, from the scanned sums of smo_rows_count
__global__ __launch_bounds__(KT_SMO_LANES) void smo_rows_offsets(const u32* __restrict__ deg, u32 n, const u32* __restrict__ cnt, u32* __restrict__ off)
{
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * (KT_SMO_LANES / 64) + (threadIdx.x >> 6);
    const size_t base = w * KT_SMO_PER_WAVE;
    if (base >= n) return;   // wave-uniform
    u32 o = cnt[w];
#pragma unroll
    for (int k = 0; k < KT_SMO_PER_WAVE / 64; ++k) {
        const size_t i = base + 64 * k + lane;
        const u32 d = i < n ? deg[i] : 0u;
        const u32 s = kt_wave_incl(d, lane);
        if (i < n) off[i] = o + s - d;
        o += __shfl(s, 63, 64);
    }
}

// cur: zero on entry, the degree afterwards
__global__ __launch_bounds__(KT_SMO_LANES) void smo_fill(const u64* __restrict__ sk, const u8* __restrict__ ec, u32 m3, const u32* __restrict__ flag, int mode,
                                                         const u32* __restrict__ off, u32* __restrict__ cur, u32* __restrict__ nbr)
{
    const size_t j = (size_t)blockIdx.x * KT_SMO_LANES + threadIdx.x;
    if (j >= m3) return;
    const int c = ec[j];
    if (!c) return;
    const u64 k = sk[j];
    const u32 lo = (u32)(k >> 32), hi = (u32)k;
    // (smo_degree counted the same entries: a slot lies below off[v] + deg[v], and the rows' total below the 2 * 3 m entries of nbr)
    if (smo_takes(flag[lo], c, mode)) nbr[off[lo] + atomicAdd(cur + lo, 1u)] = hi;
    if (smo_takes(flag[hi], c, mode)) nbr[off[hi] + atomicAdd(cur + hi, 1u)] = lo;
}

// the word of vertex i's coordinate k: three planes of n words, so that a wave's own reads and writes are contiguous
__device__ __forceinline__ size_t smo_word(u32 i, int k, u32 n) { return (size_t)k * n + i; }

// deg becomes the degree the steps use: 0 for a vertex that failed a check.  res[1], res[2]: the rim vertices, the ones that move
__global__ __launch_bounds__(KT_SMO_LANES) void smo_init(const uint4* __restrict__ v, u32 n, const u32* __restrict__ flag, u32* __restrict__ deg, int steps,
                                                         long long* __restrict__ q, u32* __restrict__ res)
{
    const int lane = threadIdx.x & 63;
    const size_t stride = (size_t)gridDim.x * KT_SMO_LANES;
    u32 nr = 0, nm = 0;   // of this wave, over its rounds
    for (size_t base = (size_t)blockIdx.x * KT_SMO_LANES + threadIdx.x - lane; base < n; base += stride) {   // wave-uniform; ceil(n / stride) rounds
        const size_t i = base + lane;
        bool rim = false, moves = false;
        if (i < n) {
            const uint4 p = v[i];
            const u32 f = flag[i];
            u32 d = deg[i];
            const bool ok = kt_mesh_valid(p);
            if ((f & KT_SMO_REFERENCED) && !ok) { atomicOr(res, KT_SMO_BAD_VERTEX); d = 0u; }
            if (d > KT_SMO_MAX_VALENCE) { atomicOr(res, KT_SMO_BAD_VALENCE); d = 0u; }
            deg[i] = d;
            q[smo_word((u32)i, 0, n)] = ok ? kt_q32(__uint_as_float(p.x)) : 0ll;   // (valid: |q| < 2^45)
            q[smo_word((u32)i, 1, n)] = ok ? kt_q32(__uint_as_float(p.y)) : 0ll;
            q[smo_word((u32)i, 2, n)] = ok ? kt_q32(__uint_as_float(p.z)) : 0ll;
            rim = (f & KT_SMO_RIM) != 0u;
            moves = d > 0u && steps > 0;
        }
        nr += (u32)__popcll(__ballot(rim));
        nm += (u32)__popcll(__ballot(moves));
    }
    if (lane == 0) {
        if (nr) atomicAdd(res + 1, nr);
        if (nm) atomicAdd(res + 2, nm);
    }
}

// One half-step with factor f: qa before, qb after.  Every |q| of qa is below 2^45 and d <= 65535, so |S| < 2^61 and |D| < 2^62; a q' that
// leaves the range raises the status bit and is not kept, so the bound holds for the next half-step too.
__global__ __launch_bounds__(KT_SMO_LANES) void smo_step(const long long* __restrict__ qa, long long* __restrict__ qb, const u32* __restrict__ off,
                                                         const u32* __restrict__ deg, const u32* __restrict__ nbr, u32 n, double f, u32* __restrict__ res)
{
    const size_t i = (size_t)blockIdx.x * KT_SMO_LANES + threadIdx.x;
    if (i >= n) return;
    const u32 d = deg[i];
    long long q[3] = {qa[smo_word((u32)i, 0, n)], qa[smo_word((u32)i, 1, n)], qa[smo_word((u32)i, 2, n)]};
    if (d > 0u) {
        const u32* __restrict__ row = nbr + off[i];
        long long S[3] = {0, 0, 0};
        for (u32 k = 0; k < d; ++k) {   // d <= 65535 (smo_init)
            const u32 j = row[k];       // (below n: an end of a key)
#pragma unroll
            for (int c = 0; c < 3; ++c) S[c] += qa[smo_word(j, c, n)];
        }
        const double dd = (double)d;
        bool left = false;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long D = S[c] - (long long)d * q[c];
            const long long qn = q[c] + __double2ll_rn(f * ((double)D / dd));
            if (qn >= KT_SMO_RANGE || qn <= -KT_SMO_RANGE) left = true; else q[c] = qn;
        }
        if (left) atomicOr(res, KT_SMO_LEFT_RANGE);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) qb[smo_word((u32)i, c, n)] = q[c];
}

__global__ __launch_bounds__(KT_SMO_LANES) void smo_finish(const uint4* __restrict__ v, const long long* __restrict__ q, const u32* __restrict__ deg, u32 n, int steps,
                                                           const u32* __restrict__ res, uint4* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * KT_SMO_LANES + threadIdx.x;
    if (i >= n || res[0] != 0u) return;   // a check failed: nothing is written
    uint4 p = v[i];
    if (steps > 0 && deg[i] > 0u) {
        p.x = __float_as_uint(kt_q32_float(q[smo_word((u32)i, 0, n)]));
        p.y = __float_as_uint(kt_q32_float(q[smo_word((u32)i, 1, n)]));
        p.z = __float_as_uint(kt_q32_float(q[smo_word((u32)i, 2, n)]));
    }
    out[i] = p;
}

}  // namespace

struct smo_per_vertex {
    long long *qa, *qb;               // device, 3 per vertex: the two states, three planes each
    u32 *deg, *off, *flag, *cur, *cnt;   // device, a word per vertex (cnt: one per KT_SMO_PER_WAVE vertices)
};
struct smo_per_half_edge {
    u64* keys;                        // device, one per half-edge: the keys before the sort
    u32* nbr;                         // device, two per half-edge: the neighbour lists
    u8* ec;                           // device, one per half-edge: the class of the sorted entry
};
struct smo_staging { uint4 *v, *vo; u32* t; };

struct kt_mesh_smooth_pass : kt_pass_head {   // (kt_mesh_pass.hpp)
    u32* res;                         // device, KT_SMO_RES
    u32* res_host;                    // pinned, KT_SMO_RES
    kt_group<smo_per_vertex> ws;      // sized by vertices
    kt_sorted_keys<false> srt;        // (kt_mesh_keys.hpp) sized by half-edges: sk, and the sorted half-edges as si
    kt_group<smo_per_half_edge> he;   // sized by half-edges
    kt_group<smo_staging, 2> st;      // the host form's staging, sized by vertices and triangles
};

extern "C" int kt_mesh_smooth_destroy(kt_mesh_smooth_pass* w) { return kt_pass_destroy(w); }

extern "C" int kt_mesh_smooth_create(kt_ctx* c, void* hip_stream, kt_mesh_smooth_pass** out) { return kt_pass_create(c, hip_stream, out, KT_SMO_RES, KT_SMO_RES); }

namespace {

int smo_reserve(kt_mesh_smooth_pass* w, size_t n)
{
    return w->ws.grow(w->stream, {n}, [](kt_mem& mem, smo_per_vertex& g, const size_t* c) {
        u32** per_vertex[4] = {&g.deg, &g.off, &g.flag, &g.cur};
        int s = mem.device(&g.qa, 3 * c[0]);
        if (s == KT_OK) s = mem.device(&g.qb, 3 * c[0]);
        for (int k = 0; k < 4 && s == KT_OK; ++k) s = mem.device(per_vertex[k], c[0]);
        if (s == KT_OK) s = mem.device(&g.cnt, (c[0] + KT_SMO_PER_WAVE - 1) / KT_SMO_PER_WAVE);
        return s;
    });
}

int smo_reserve_half_edges(kt_mesh_smooth_pass* w, size_t m3)
{
    KT_TRY(w->srt.reserve(w->stream, m3));
    return w->he.grow(w->stream, {m3}, [](kt_mem& mem, smo_per_half_edge& g, const size_t* c) {
        int s = mem.device(&g.keys, c[0]);
        if (s == KT_OK) s = mem.device(&g.nbr, 2 * c[0]);
        if (s == KT_OK) s = mem.device(&g.ec, c[0]);
        return s;
    });
}

int smo_reserve_staging(kt_mesh_smooth_pass* w, size_t n, size_t m)
{
    return w->st.grow(w->stream, {n, m}, [](kt_mem& mem, smo_staging& g, const size_t* c) {
        int s = mem.device(&g.v, c[0]);
        if (s == KT_OK) s = mem.device(&g.vo, c[0]);
        if (s == KT_OK) s = mem.device(&g.t, 3 * c[1]);
        return s;
    });
}

// the checks both forms share: KT_ERR_ARG with nothing written, before any allocation or launch
int smo_check(const kt_mesh_smooth_pass* w, const void* vertices, size_t n, const void* triangles, size_t m, int steps, float lambda, float mu, int mode,
              const void* vertices_out, const kt_mesh_smooth_stats* stats)
{
    KT_ARG(w && stats && n <= KT_SMO_MAX_VERTICES && m <= KT_SMO_MAX_TRIANGLES);
    KT_ARG(steps >= 0 && steps <= KT_SMO_MAX_STEPS && (mode == 0 || mode == 1));
    KT_ARG(lambda > 0.0f && lambda <= 1.0f && mu >= -1.1f && mu <= 1.0f);   // (false for a NaN)
    KT_TRY(kt_mesh_check_inputs(vertices, n, triangles, m));
    KT_TRY(kt_mesh_check_outputs(vertices_out, n, nullptr, 0, n, m));
    if (n > 0) {
        const kt_byte_range ins[2] = {{vertices, n * sizeof(kt_mesh_vertex)}, {triangles, 3 * m * sizeof(uint32_t)}};
        const kt_byte_range outs[1] = {{vertices_out, n * sizeof(kt_mesh_vertex)}};
        KT_TRY(kt_mesh_check_disjoint(outs, 1, ins, 2));
    }
    return KT_OK;
}

}  // namespace

extern "C" int kt_mesh_smooth_device(kt_mesh_smooth_pass* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m, int steps,
                                     float lambda, float mu, int mode, kt_mesh_vertex* vertices_out_dev, kt_mesh_smooth_stats* stats)
{
    static_assert(sizeof(kt_mesh_vertex) == sizeof(uint4), "vertex layout");
    KT_TRY(smo_check(w, vertices_dev, n, triangles_dev, m, steps, lambda, mu, mode, vertices_out_dev, stats));
    if (n == 0) { stats->rim_vertices = stats->moved_vertices = stats->unique_edges = 0; return KT_OK; }
    KT_HIP(hipSetDevice(w->ctx->device));
    const size_t m3 = 3 * m;
    KT_TRY(smo_reserve(w, n));
    KT_TRY(smo_reserve_half_edges(w, m3));
    hipStream_t st = w->stream;
    const u32 n32 = (u32)n, m32 = (u32)m3;
    const uint4* v = reinterpret_cast<const uint4*>(vertices_dev);
    const unsigned vblocks = (unsigned)((n + KT_SMO_LANES - 1) / KT_SMO_LANES), hblocks = (unsigned)((m3 + KT_SMO_LANES - 1) / KT_SMO_LANES);
    KT_HIP(hipMemsetAsync(w->res, 0, KT_SMO_RES * sizeof(u32), st));
    KT_HIP(hipMemsetAsync(w->ws.flag, 0, n * sizeof(u32), st));
    KT_HIP(hipMemsetAsync(w->ws.deg, 0, n * sizeof(u32), st));
    if (m > 0) {
        KT_HIP(hipMemsetAsync(w->ws.cur, 0, n * sizeof(u32), st));
        hipLaunchKernelGGL(smo_keys, dim3(hblocks), dim3(KT_SMO_LANES), 0, st, triangles_dev, m32, n32, w->he.keys, w->res);
        KT_LAUNCH_CHECK();
        KT_TRY(w->srt.sort(st, w->he.keys, m3, "kt_mesh_smooth"));
        hipLaunchKernelGGL(smo_classify, dim3(std::min<unsigned>(hblocks, KT_SMO_COUNT_BLOCKS)), dim3(KT_SMO_LANES), 0, st, (const u64*)w->srt.sk, (const u32*)w->srt.si, m32, triangles_dev, w->he.ec, w->ws.flag, w->res);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(smo_degree, dim3(hblocks), dim3(KT_SMO_LANES), 0, st, (const u64*)w->srt.sk, (const u8*)w->he.ec, m32, (const u32*)w->ws.flag, mode, w->ws.deg);
        KT_LAUNCH_CHECK();
        const size_t waves = (n + KT_SMO_PER_WAVE - 1) / KT_SMO_PER_WAVE;
        const unsigned wblocks = (unsigned)((waves + KT_SMO_LANES / 64 - 1) / (KT_SMO_LANES / 64));
        hipLaunchKernelGGL(smo_rows_count, dim3(wblocks), dim3(KT_SMO_LANES), 0, st, (const u32*)w->ws.deg, n32, w->ws.cnt);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(kt_scan_runs_kernel<1>, dim3(1), dim3(256), 0, st, w->ws.cnt, (int)waves, (u32*)nullptr);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(smo_rows_offsets, dim3(wblocks), dim3(KT_SMO_LANES), 0, st, (const u32*)w->ws.deg, n32, (const u32*)w->ws.cnt, w->ws.off);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(smo_fill, dim3(hblocks), dim3(KT_SMO_LANES), 0, st, (const u64*)w->srt.sk, (const u8*)w->he.ec, m32, (const u32*)w->ws.flag, mode,
                           (const u32*)w->ws.off, w->ws.cur, w->he.nbr);
        KT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(smo_init, dim3(std::min<unsigned>(vblocks, KT_SMO_COUNT_BLOCKS)), dim3(KT_SMO_LANES), 0, st, v, n32, (const u32*)w->ws.flag, w->ws.deg, steps, w->ws.qa, w->res);
    KT_LAUNCH_CHECK();
    long long *qa = w->ws.qa, *qb = w->ws.qb;
    if (m > 0) {
        for (int h = 0; h < 2 * steps; ++h) {
            hipLaunchKernelGGL(smo_step, dim3(vblocks), dim3(KT_SMO_LANES), 0, st, (const long long*)qa, qb, (const u32*)w->ws.off, (const u32*)w->ws.deg,
                               (const u32*)w->he.nbr, n32, h & 1 ? (double)mu : (double)lambda, w->res);
            KT_LAUNCH_CHECK();
            std::swap(qa, qb);
        }
    }
    hipLaunchKernelGGL(smo_finish, dim3(vblocks), dim3(KT_SMO_LANES), 0, st, v, (const long long*)qa, (const u32*)w->ws.deg, n32, steps, (const u32*)w->res,
                       reinterpret_cast<uint4*>(vertices_out_dev));
    KT_LAUNCH_CHECK();
    for (int k = 0; k < KT_SMO_RES; ++k) w->res_host[k] = 0;
    KT_HIP(hipMemcpyAsync(w->res_host, w->res, KT_SMO_RES * sizeof(u32), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    const u32* r = w->res_host;
    if (r[0]) {
        kt_set_error("kt_mesh_smooth:%s%s%s%s; nothing was written", r[0] & KT_SMO_BAD_INDEX ? " a triangle index out of range" : "",
                     r[0] & KT_SMO_BAD_VERTEX ? " a triangle's vertex that is not finite or has a coordinate of 8192 m or more" : "",
                     r[0] & KT_SMO_BAD_VALENCE ? " a valence over the bound of 65535" : "",
                     r[0] & KT_SMO_LEFT_RANGE ? " a coordinate that left the range of 8192 m" : "");
        return KT_ERR_ARG;
    }
    stats->rim_vertices = r[1]; stats->moved_vertices = r[2]; stats->unique_edges = r[3];
    return KT_OK;
}

extern "C" int kt_mesh_smooth(kt_mesh_smooth_pass* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m, int steps, float lambda, float mu,
                              int mode, kt_mesh_vertex* vertices_out, kt_mesh_smooth_stats* stats)
{
    KT_TRY(smo_check(w, vertices, n, triangles, m, steps, lambda, mu, mode, vertices_out, stats));
    if (n == 0) { stats->rim_vertices = stats->moved_vertices = stats->unique_edges = 0; return KT_OK; }
    KT_HIP(hipSetDevice(w->ctx->device));
    KT_TRY(smo_reserve_staging(w, n, m));
    return kt_mesh_host_form(w->stream, {{w->st.v, vertices, n * sizeof(kt_mesh_vertex)}, {w->st.t, triangles, 3 * m * sizeof(uint32_t)}}, [&] {
        return kt_mesh_smooth_device(w, reinterpret_cast<const kt_mesh_vertex*>(w->st.v), n, w->st.t, m, steps, lambda, mu, mode,
                                     reinterpret_cast<kt_mesh_vertex*>(w->st.vo), stats);
    }, [&](kt_host_copy* down) { down[0] = {vertices_out, w->st.vo, n * sizeof(kt_mesh_vertex)}; });
}
