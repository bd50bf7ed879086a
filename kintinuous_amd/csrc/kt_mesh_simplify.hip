// kt_mesh_simplify.hip -- coarsens the -m mesh by vertex clustering (kt_mesh_simplify, kt_mesh_simplify_device).
//
// Not in the reference (its -m meshes a voxel-grid-filtered cloud, backend/MeshGenerator.cpp, and is coarse by construction).  The mesh
// of kt_mesh.hip has one vertex per crossed voxel edge; this pass merges the vertices of one span that fall into one cubic cell of a
// caller-chosen edge length and drops the triangles that collapse.  It is the weld (kt_mesh_weld.hip) with another key, plus a
// segmented sum (the merged vertex is the mean of its cluster) and a triangle compaction.
//
// Semantics (include/kt_abi.h; restated in numpy by kintinuous_amd/mesh_simplify_ref.py, which the device equals on every byte):
//   - key = (cz + 2^19) << 40 | (cy + 2^19) << 20 | (cx + 2^19), c = floor((double)x * inv), inv = 1 / (double)cell from the host; a
//     vertex that is not finite, has |coordinate| >= 8192 or a c outside [-2^19, 2^19) gets 1 << 63 and fails the call;
//   - the occurrences of a key in index order; an occurrence starts a new cluster when it is the first of its key or when its span
//     differs from the previous occurrence's; output vertices = one per cluster in the order of the clusters' first vertices (heads);
//   - per member and axis q = rint((double)x * 2^20) as int64, S = sum, k = count, mean = floor((2 S + k) / (2 k)), the coordinate
//     (float)((double)mean * 2^-20); each byte of the colour word alike; a cluster of one keeps its 16 bytes;
//   - every triangle index becomes its vertex's cluster; a triangle with two equal indices is dropped, the others keep their order.
//
// The passes, all on the object's stream, integers only:
//   keys     one key per vertex
//   sort     the sorted key list (kt_mesh_keys.hpp) of (key, index) -> sk, si; the last sorted key tells whether any vertex was invalid
//   heads    kt_runs_heads_kernel, not gated (kt_wave.hpp): hp[j] = j where sorted entry j starts a cluster, else 0; a workgroup takes
//            KT_SIMP_CHUNK entries
//   scan     the list's scan_max over hp: every entry learns the sorted position of its cluster's head
//   reps, count, kt_scan_runs_kernel<1>: the weld's (kt_wave.hpp); rank: newidx[i] = the heads below i, headof[c] = the head of cluster c
//   spans, map: the weld's; rep[i] is then the cluster of vertex i
//   zero     the sums of the clusters there are (the count is read on the device)
//   sums     a wave takes 64 sorted entries: every lane gathers its vertex and forms three int64 terms and the four byte terms packed
//            in 16-bit fields; a segmented scan over the head ballot; the last lane of a segment holds its sums.  A segment that begins
//            and ends inside the wave is complete and is STORED (one of a single member is not even stored: the finish pass copies the
//            head); one that crosses a wave boundary is added with 64-bit integer atomics, one set per wave it touches.  Integer
//            sums: the result does not depend on the order of arrival.
//   tcount   every triangle's three clusters, kept in the workspace (tm); a wave counts the survivors of its 256 (ballots);
//            kt_scan_runs_kernel<1> gives every wave its first output position
//   finish   divides and writes the output vertices; twrite streams tm and writes the surviving triangles
// finish and twrite write the caller's buffers only when both counts fit and no key had bit 63 set: they read these facts from device
// memory, so the whole call is enqueued at once and the host waits once.
#include "kt_mesh_keys.hpp"
#include "kt_wave.hpp"

#include <cmath>

#define KT_SIMP_LANES 256
#define KT_SIMP_CHUNK 2048            // sorted entries per workgroup of the head pass
#define KT_SIMP_PER_WAVE KT_RUNS_PER_WAVE   // vertices (triangles) per wave of the count and rank (tcount and twrite) passes
#define KT_SIMP_MAX_VERTICES ((size_t)1 << 29)
#define KT_SIMP_MAX_TRIANGLES ((size_t)1 << 31)
#define KT_SIMP_ACC 8                 // 64-bit words per cluster: three coordinate sums, four byte sums, the count
#define KT_SIMP_MAX_BLOCKS 65536      // of the grid-stride passes

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

__global__ __launch_bounds__(KT_SIMP_LANES) void simp_keys(const uint4* __restrict__ v, u32 n, double inv, u64* __restrict__ key)
{
    const size_t i = (size_t)blockIdx.x * KT_SIMP_LANES + threadIdx.x;
    if (i >= n) return;
    const uint4 p = v[i];
    const float x[3] = {__uint_as_float(p.x), __uint_as_float(p.y), __uint_as_float(p.z)};
    bool ok = true;
    u64 k = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double c = floor((double)x[a] * inv);
        const bool in = kt_mesh_valid_coord(x[a]) && c >= -524288.0 && c < 524288.0;   // (per coordinate: the cell index is bounded too)
        ok = ok && in;
        k |= (u64)((in ? (long long)c : 0ll) + 524288ll) << (20 * a);
    }
    key[i] = ok ? k : 1ull << 63;
}

// newidx[i] = the heads below vertex i; headof[that] = i for a head
__global__ __launch_bounds__(KT_SIMP_LANES) void simp_rank(const u32* __restrict__ rep, u32 n, const u32* __restrict__ cnt, u32* __restrict__ newidx,
                                                           u32* __restrict__ headof)
{
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * (KT_SIMP_LANES / 64) + (threadIdx.x >> 6);
    const size_t base = w * KT_SIMP_PER_WAVE;
    if (base >= n) return;   // wave-uniform
    u32 o = cnt[w];
#pragma unroll
    for (int k = 0; k < KT_SIMP_PER_WAVE / 64; ++k) {
        const size_t i = base + 64 * k + lane;
        const bool in = i < n, kept = in && rep[i] == (u32)i;
        const u64 b = __ballot(kept);
        const u32 r = o + kt_wave_rank(b, lane);
        if (in) newidx[i] = r;
        if (kept) headof[r] = (u32)i;
        o += (u32)__popcll(b);
    }
}

__global__ __launch_bounds__(KT_SIMP_LANES) void simp_zero(u64* __restrict__ acc, const u32* __restrict__ totals)
{
    const size_t words = (size_t)totals[0] * KT_SIMP_ACC, stride = (size_t)gridDim.x * KT_SIMP_LANES;
    for (size_t k = (size_t)blockIdx.x * KT_SIMP_LANES + threadIdx.x; k < words; k += stride) acc[k] = 0ull;
}

// cluster: rep after the map pass.  acc: KT_SIMP_ACC words per cluster, zero on entry
__global__ __launch_bounds__(KT_SIMP_LANES) void simp_sums(const uint4* __restrict__ v, const u32* __restrict__ si, const u32* __restrict__ hps,
                                                           const u32* __restrict__ cluster, u32 n, u64* __restrict__ acc)
{
    const int lane = threadIdx.x & 63;
    const size_t j = (size_t)blockIdx.x * KT_SIMP_LANES + threadIdx.x;
    if (j - lane >= n) return;   // wave-uniform
    const bool in = j < n;
    u32 i = 0;
    bool head = false;
    long long q0 = 0, q1 = 0, q2 = 0;
    u64 pb = 0;                // the four bytes in 16-bit fields: a wave's sum of a byte is at most 64 * 255
    if (in) {
        i = si[j];
        head = hps[j] == (u32)j;
        const uint4 p = v[i];
        q0 = (long long)rint((double)__uint_as_float(p.x) * 1048576.0);
        q1 = (long long)rint((double)__uint_as_float(p.y) * 1048576.0);
        q2 = (long long)rint((double)__uint_as_float(p.z) * 1048576.0);
        pb = (u64)(p.w & 255u) | (u64)((p.w >> 8) & 255u) << 16 | (u64)((p.w >> 16) & 255u) << 32 | (u64)(p.w >> 24) << 48;
    }
    const u64 hb = __ballot(head);
    // the lane my segment starts at: the highest head at or below me; lane 0 when the segment came in from the wave before
    const u64 below = hb & ((2ull << lane) - 1ull);
    const int start = below ? 63 - __clzll((long long)below) : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long a0 = __shfl_up(q0, off, 64), a1 = __shfl_up(q1, off, 64), a2 = __shfl_up(q2, off, 64);
        const u64 ab = __shfl_up(pb, off, 64);
        if (lane - off >= start) { q0 += a0; q1 += a1; q2 += a2; pb += ab; }
    }
    bool last = false;         // the segment's last entry in this wave
    if (in) {
        if (j + 1 == n) last = true;
        else if (lane < 63) last = (hb >> (lane + 1)) & 1ull;
        else last = hps[j + 1] == (u32)(j + 1);
    }
    // (at lane 63 `last` says the segment ends with the wave; otherwise it goes on and the sums so far are added)
    const bool ends = last, crosses = in && lane == 63 && !last;
    if (!ends && !crosses) return;
    const bool complete = ends && ((hb >> start) & 1ull);   // it began at a head of this wave and ends here
    const u64 k = (u64)(lane - start + 1);
    if (complete && k == 1) return;                          // the finish pass copies the head
    u64* a = acc + (size_t)cluster[i] * KT_SIMP_ACC;
    const u64 t[KT_SIMP_ACC] = {(u64)q0, (u64)q1, (u64)q2, pb & 0xffffull, (pb >> 16) & 0xffffull, (pb >> 32) & 0xffffull, pb >> 48, k};
    if (complete) {
#pragma unroll
        for (int e = 0; e < KT_SIMP_ACC; ++e) a[e] = t[e];
    } else {
#pragma unroll
        for (int e = 0; e < KT_SIMP_ACC; ++e) atomicAdd(a + e, t[e]);
    }
}

// a triangle's three clusters go to tm; the wave counts those that do not collapse (an index at or above n names no vertex: it stays
// as it is).  The write pass then streams tm instead of gathering a second time
__device__ __forceinline__ bool simp_alive(const u32 x[3]) { return x[0] != x[1] && x[1] != x[2] && x[0] != x[2]; }

__global__ __launch_bounds__(KT_SIMP_LANES) void simp_tcount(const u32* __restrict__ tri, size_t m, const u32* __restrict__ cluster, u32 n, u32* __restrict__ tm,
                                                             u32* __restrict__ tcnt)
{
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * (KT_SIMP_LANES / 64) + (threadIdx.x >> 6);
    const size_t base = w * KT_SIMP_PER_WAVE;
    if (base >= m) return;   // wave-uniform
    u32 c = 0;
#pragma unroll
    for (int k = 0; k < KT_SIMP_PER_WAVE / 64; ++k) {
        const size_t t = base + 64 * k + lane;
        u32 x[3] = {0u, 0u, 0u};
        if (t < m) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const u32 a = tri[3 * t + e];
                x[e] = a < n ? cluster[a] : a;
                tm[3 * t + e] = x[e];
            }
        }
        c += (u32)__popcll(__ballot(t < m && simp_alive(x)));
    }
    if (lane == 0) tcnt[w] = c;
}

// the facts that decide whether the caller's buffers are written: both counts fit, and no key has bit 63 set
__device__ __forceinline__ bool simp_writes(const u32* totals, const u64* sk, u32 n, u64 vcap, u64 tcap)
{
    return (u64)totals[0] <= vcap && (u64)totals[1] <= tcap && (sk[n - 1] >> 63) == 0;
}

// floor(a / b) for b > 0
__device__ __forceinline__ long long simp_floor_div(long long a, long long b)
{
    const long long q = a / b;
    return a % b < 0 ? q - 1 : q;
}

__global__ __launch_bounds__(KT_SIMP_LANES) void simp_finish(const uint4* __restrict__ v, const u32* __restrict__ headof, const u64* __restrict__ acc,
                                                             const u32* __restrict__ totals, const u64* __restrict__ sk, u32 n, u64 vcap, u64 tcap,
                                                             uint4* __restrict__ vout)
{
    if (!simp_writes(totals, sk, n, vcap, tcap)) return;
    const size_t total = totals[0], stride = (size_t)gridDim.x * KT_SIMP_LANES;
    for (size_t c = (size_t)blockIdx.x * KT_SIMP_LANES + threadIdx.x; c < total; c += stride) {
        uint4 p = v[headof[c]];
        const u64* a = acc + c * KT_SIMP_ACC;
        const long long k = (long long)a[7];
        if (k > 1) {         // (0: a cluster of one, which the sums pass never stored)
            u32 xyz[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const long long mean = simp_floor_div(2 * (long long)a[e] + k, 2 * k);
                xyz[e] = __float_as_uint((float)((double)mean * (1.0 / 1048576.0)));
            }
            u32 w = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) w |= (u32)((2 * a[3 + e] + (u64)k) / (2 * (u64)k)) << (8 * e);
            p = make_uint4(xyz[0], xyz[1], xyz[2], w);
        }
        vout[c] = p;
    }
}

__global__ __launch_bounds__(KT_SIMP_LANES) void simp_twrite(const u32* __restrict__ tm, size_t m, u32 n, const u32* __restrict__ tcnt, const u32* __restrict__ totals,
                                                             const u64* __restrict__ sk, u64 vcap, u64 tcap, u32* __restrict__ tout)
{
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * (KT_SIMP_LANES / 64) + (threadIdx.x >> 6);
    const size_t base = w * KT_SIMP_PER_WAVE;
    if (base >= m) return;   // wave-uniform
    if (!simp_writes(totals, sk, n, vcap, tcap)) return;
    size_t o = tcnt[w];
#pragma unroll
    for (int k = 0; k < KT_SIMP_PER_WAVE / 64; ++k) {
        const size_t t = base + 64 * k + lane;
        u32 x[3] = {0u, 0u, 0u};
        if (t < m) { x[0] = tm[3 * t]; x[1] = tm[3 * t + 1]; x[2] = tm[3 * t + 2]; }
        const bool alive = t < m && simp_alive(x);
        const u64 b = __ballot(alive);
        if (alive) {
            u32* d = tout + 3 * (o + kt_wave_rank(b, lane));
            d[0] = x[0]; d[1] = x[1]; d[2] = x[2];
        }
        o += (size_t)__popcll(b);
    }
}

}  // namespace

struct simp_per_vertex {
    u64 *key, *acc;                   // device: a key per vertex, KT_SIMP_ACC words of sums per vertex
    u32 *hp, *hps, *rep, *headof, *cnt;   // device, a word per vertex (cnt: one per KT_SIMP_PER_WAVE vertices): head positions before and after the
                                      // scan (hp is newidx once the scan has read it), heads and then clusters, the head of every cluster
};
struct simp_per_triangle { u32 *tcnt, *tm; };   // device: one count per wave, the three clusters of every triangle

struct kt_mesh_simplifier : kt_pass_head {   // (kt_mesh_pass.hpp)
    u32* res;                         // device, 2: the output vertices, the surviving triangles
    u64* res_host;                    // pinned, 3 words: the two counts, the last sorted key
    kt_sorted_keys<true> srt;         // (kt_mesh_keys.hpp) sized by vertices
    kt_group<simp_per_vertex> ws;     // sized by vertices
    kt_group<simp_per_triangle> tc;   // sized by waves of KT_SIMP_PER_WAVE triangles
    kt_span_table sp;
    kt_mesh_staging st;
};

extern "C" int kt_mesh_simplify_destroy(kt_mesh_simplifier* w) { return kt_pass_destroy(w); }

extern "C" int kt_mesh_simplify_create(kt_ctx* c, void* hip_stream, kt_mesh_simplifier** out) { return kt_pass_create(c, hip_stream, out, 2, 3); }

namespace {

int simp_reserve(kt_mesh_simplifier* w, size_t n)
{
    KT_TRY(w->srt.reserve(w->stream, n));
    return w->ws.grow(w->stream, {n}, [](kt_mem& mem, simp_per_vertex& g, const size_t* c) {
        int s = mem.device(&g.key, c[0]);
        if (s == KT_OK) s = mem.device(&g.acc, KT_SIMP_ACC * c[0]);
        if (s == KT_OK) s = mem.device(&g.hp, c[0]);
        if (s == KT_OK) s = mem.device(&g.hps, c[0]);
        if (s == KT_OK) s = mem.device(&g.rep, c[0]);
        if (s == KT_OK) s = mem.device(&g.headof, c[0]);
        if (s == KT_OK) s = mem.device(&g.cnt, (c[0] + KT_SIMP_PER_WAVE - 1) / KT_SIMP_PER_WAVE);
        return s;
    });
}

int simp_reserve_triangles(kt_mesh_simplifier* w, size_t waves)
{
    return w->tc.grow(w->stream, {waves}, [](kt_mem& mem, simp_per_triangle& g, const size_t* c) {
        int s = mem.device(&g.tcnt, c[0]);
        if (s == KT_OK) s = mem.device(&g.tm, 3 * KT_SIMP_PER_WAVE * c[0]);
        return s;
    });
}

// the checks both forms share: KT_ERR_ARG with nothing written
int simp_check(const kt_mesh_simplifier* w, const void* vertices, size_t n, const void* triangles, size_t m, const size_t* span_first, int n_spans, float cell,
               const void* vertices_out, size_t vertex_capacity, const void* triangles_out, size_t triangle_capacity, const size_t* span_first_out,
               const size_t* n_out, const size_t* m_out)
{
    KT_ARG(w && n_out && m_out && span_first_out && n <= KT_SIMP_MAX_VERTICES && m <= KT_SIMP_MAX_TRIANGLES);
    KT_ARG(std::isfinite(cell) && cell > 0.0f);
    KT_TRY(kt_mesh_check_inputs(vertices, n, triangles, m));
    KT_TRY(kt_mesh_check_outputs(vertices_out, vertex_capacity, triangles_out, triangle_capacity, n, m));
    KT_ARG(n == 0 || vertices_out != vertices);                                   // neither compaction is in place
    KT_ARG(n == 0 || m == 0 || !triangles_out || triangles_out != triangles);
    return kt_mesh_check_spans(span_first, n_spans, n);
}

}  // namespace

extern "C" int kt_mesh_simplify_device(kt_mesh_simplifier* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m,
                                       const size_t* span_first, int n_spans, float cell, kt_mesh_vertex* vertices_out_dev, size_t vertex_capacity,
                                       uint32_t* triangles_out_dev, size_t triangle_capacity, size_t* span_first_out, size_t* n_out, size_t* m_out)
{
    static_assert(sizeof(kt_mesh_vertex) == sizeof(uint4) && sizeof(u64) == sizeof(uint64_t), "vertex and key layout");
    KT_TRY(simp_check(w, vertices_dev, n, triangles_dev, m, span_first, n_spans, cell, vertices_out_dev, vertex_capacity, triangles_out_dev, triangle_capacity,
                      span_first_out, n_out, m_out));
    *n_out = 0; *m_out = 0;
    if (n == 0) { kt_mesh_empty_spans(span_first_out, n_spans); return KT_OK; }
    KT_HIP(hipSetDevice(w->ctx->device));
    const size_t twaves = (m + KT_SIMP_PER_WAVE - 1) / KT_SIMP_PER_WAVE;
    KT_TRY(simp_reserve(w, n));
    KT_TRY(simp_reserve_triangles(w, twaves));
    hipStream_t st = w->stream;
    const size_t S = (size_t)n_spans;
    const u32 n32 = (u32)n;
    const double inv = 1.0 / (double)cell;
    KT_TRY(w->sp.upload(st, span_first, n_spans));
    const u32* df = w->sp.first();
    u32* dfo = w->sp.first_out();
    KT_HIP(hipMemsetAsync(w->res, 0, 2 * sizeof(u32), st));
    const uint4* v = reinterpret_cast<const uint4*>(vertices_dev);
    const unsigned vblocks = (unsigned)((n + KT_SIMP_LANES - 1) / KT_SIMP_LANES);
    hipLaunchKernelGGL(simp_keys, dim3(vblocks), dim3(KT_SIMP_LANES), 0, st, v, n32, inv, w->ws.key);
    KT_LAUNCH_CHECK();
    KT_TRY(w->srt.sort(st, w->ws.key, n, "kt_mesh_simplify"));
    hipLaunchKernelGGL((kt_runs_heads_kernel<KT_SIMP_LANES, KT_SIMP_CHUNK, false>), dim3((unsigned)((n + KT_SIMP_CHUNK - 1) / KT_SIMP_CHUNK)), dim3(KT_SIMP_LANES), 0, st,
                       (const u64*)w->srt.sk, (const u32*)w->srt.si, n32, df, (const u64*)nullptr, n_spans, (u64)0, w->ws.hp);
    KT_LAUNCH_CHECK();
    KT_TRY(w->srt.scan_max(st, w->ws.hp, w->ws.hps, n, "kt_mesh_simplify"));
    hipLaunchKernelGGL(kt_runs_reps_kernel<KT_SIMP_LANES>, dim3(vblocks), dim3(KT_SIMP_LANES), 0, st, w->srt.si, w->ws.hps, n32, w->ws.rep);
    KT_LAUNCH_CHECK();
    const size_t waves = (n + KT_SIMP_PER_WAVE - 1) / KT_SIMP_PER_WAVE;
    const unsigned wblocks = (unsigned)((waves + KT_SIMP_LANES / 64 - 1) / (KT_SIMP_LANES / 64));
    hipLaunchKernelGGL(kt_runs_count_kernel<KT_SIMP_LANES>, dim3(wblocks), dim3(KT_SIMP_LANES), 0, st, w->ws.rep, n32, w->ws.cnt);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kt_scan_runs_kernel<1>, dim3(1), dim3(256), 0, st, w->ws.cnt, (int)waves, w->res);
    KT_LAUNCH_CHECK();
    u32* newidx = w->ws.hp;
    hipLaunchKernelGGL(simp_rank, dim3(wblocks), dim3(KT_SIMP_LANES), 0, st, w->ws.rep, n32, w->ws.cnt, newidx, w->ws.headof);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kt_runs_spans_kernel<KT_SIMP_LANES>, dim3((unsigned)((S + 1 + KT_SIMP_LANES - 1) / KT_SIMP_LANES)), dim3(KT_SIMP_LANES), 0, st, df, (int)(S + 1),
                       n32, newidx, w->res, dfo);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kt_runs_map_kernel<KT_SIMP_LANES>, dim3(vblocks), dim3(KT_SIMP_LANES), 0, st, w->ws.rep, newidx, n32);
    KT_LAUNCH_CHECK();
    const u32* cluster = w->ws.rep;
    const unsigned zblocks = (unsigned)std::min<size_t>((KT_SIMP_ACC * n + KT_SIMP_LANES - 1) / KT_SIMP_LANES, KT_SIMP_MAX_BLOCKS);
    hipLaunchKernelGGL(simp_zero, dim3(zblocks), dim3(KT_SIMP_LANES), 0, st, w->ws.acc, w->res);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(simp_sums, dim3(vblocks), dim3(KT_SIMP_LANES), 0, st, v, w->srt.si, w->ws.hps, cluster, n32, w->ws.acc);
    KT_LAUNCH_CHECK();
    const unsigned tblocks = (unsigned)((twaves + KT_SIMP_LANES / 64 - 1) / (KT_SIMP_LANES / 64));
    if (m > 0) {
        hipLaunchKernelGGL(simp_tcount, dim3(tblocks), dim3(KT_SIMP_LANES), 0, st, triangles_dev, m, cluster, n32, w->tc.tm, w->tc.tcnt);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(kt_scan_runs_kernel<1>, dim3(1), dim3(256), 0, st, w->tc.tcnt, (int)twaves, w->res + 1);
        KT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(simp_finish, dim3(std::min<unsigned>(vblocks, KT_SIMP_MAX_BLOCKS)), dim3(KT_SIMP_LANES), 0, st, v, w->ws.headof, w->ws.acc, w->res, w->srt.sk, n32,
                       (u64)vertex_capacity, (u64)triangle_capacity, reinterpret_cast<uint4*>(vertices_out_dev));
    KT_LAUNCH_CHECK();
    if (m > 0) {
        hipLaunchKernelGGL(simp_twrite, dim3(tblocks), dim3(KT_SIMP_LANES), 0, st, (const u32*)w->tc.tm, m, n32, w->tc.tcnt, w->res, w->srt.sk, (u64)vertex_capacity,
                           (u64)triangle_capacity, triangles_out_dev);
        KT_LAUNCH_CHECK();
    }
    w->res_host[0] = 0;
    KT_HIP(hipMemcpyAsync(&w->res_host[0], w->res, 2 * sizeof(u32), hipMemcpyDeviceToHost, st));
    KT_HIP(hipMemcpyAsync(&w->res_host[1], w->srt.sk + (n - 1), sizeof(u64), hipMemcpyDeviceToHost, st));
    KT_TRY(w->sp.download(st));
    KT_HIP(hipStreamSynchronize(st));
    if (w->res_host[1] >> 63) {
        kt_set_error("kt_mesh_simplify: a vertex that is not finite, has a coordinate of 8192 m or more, or a cell index outside [-2^19, 2^19); nothing was written");
        return KT_ERR_ARG;
    }
    const u32* counts = reinterpret_cast<const u32*>(&w->res_host[0]);
    *n_out = (size_t)counts[0];
    *m_out = (size_t)counts[1];
    if (*n_out > vertex_capacity || *m_out > triangle_capacity) {
        kt_set_error("kt_mesh_simplify: %zu vertices and %zu triangles do not fit (capacities %zu and %zu); nothing was written", *n_out, *m_out, vertex_capacity,
                     triangle_capacity);
        return KT_ERR_CAPACITY;
    }
    w->sp.get(span_first_out);
    return KT_OK;
}

extern "C" int kt_mesh_simplify(kt_mesh_simplifier* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m, const size_t* span_first,
                                int n_spans, float cell, kt_mesh_vertex* vertices_out, size_t vertex_capacity, uint32_t* triangles_out, size_t triangle_capacity,
                                size_t* span_first_out, size_t* n_out, size_t* m_out)
{
    KT_TRY(simp_check(w, vertices, n, triangles, m, span_first, n_spans, cell, vertices_out, vertex_capacity, triangles_out, triangle_capacity, span_first_out, n_out,
                      m_out));
    *n_out = 0; *m_out = 0;
    if (n == 0) { kt_mesh_empty_spans(span_first_out, n_spans); return KT_OK; }
    KT_HIP(hipSetDevice(w->ctx->device));
    const size_t vcap = std::min(vertex_capacity, n), tcap = std::min(triangle_capacity, m);   // (neither count exceeds its input's)
    KT_TRY(w->st.reserve(w->stream, n, m, vcap, tcap, false));
    return kt_mesh_host_form(w->stream, {{w->st.v, vertices, n * sizeof(kt_mesh_vertex)}, {w->st.t, triangles, 3 * m * sizeof(uint32_t)}}, [&] {
        return kt_mesh_simplify_device(w, reinterpret_cast<const kt_mesh_vertex*>(w->st.v), n, w->st.t, m, span_first, n_spans, cell,
                                       reinterpret_cast<kt_mesh_vertex*>(w->st.vo), vcap, w->st.to, tcap, span_first_out, n_out, m_out);
    }, [&](kt_host_copy* down) {
        down[0] = {vertices_out, w->st.vo, *n_out * sizeof(kt_mesh_vertex)};
        down[1] = {triangles_out, w->st.to, 3 * *m_out * sizeof(uint32_t)};
    });
}
