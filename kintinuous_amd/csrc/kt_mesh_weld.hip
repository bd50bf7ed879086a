// kt_mesh_weld.hip -- welds the slab seams of the -m mesh by voxel-edge key (kt_mesh_weld, kt_mesh_weld_device).
//
// Not in the reference (its -m is a greedy projection of the whole processed cloud, backend/MeshGenerator.cpp).  Two neighbouring slabs
// of the mesh stage both emit a vertex on the in-plane edges of the plane that stayed behind as the new logical 0 (kt_abi.h,
// kt_tracker_enable_mesh_stage); kt_mesh.hip names every vertex by its GLOBAL voxel edge, and this pass merges the vertices that share
// a name.
//
// Semantics (include/kt_abi.h; restated in numpy by kintinuous_amd/mesh_weld_ref.py, which the device equals on every byte):
//   - the occurrences of a key in index order; an occurrence starts a new group when it is the first of its key or when its span's
//     time and the previous occurrence's differ by more than max_gap; a vertex's representative is the first vertex of its group;
//   - kept vertices = the representatives in input order, 16 bytes and key untouched; every triangle index becomes the new index of
//     its vertex's representative; span_first_out[s] = the kept vertices below span_first[s].
//
// The passes, all on the object's stream, integers only, no atomics (the output does not depend on scheduling):
//   sort     the sorted key list (kt_mesh_keys.hpp) of (key, index) -> sk, si: the occurrences of a key lie together in index order,
//            and the last sorted key tells whether any key had a top bit set
//   heads    kt_runs_heads_kernel, gated (kt_wave.hpp): hp[j] = j where sorted entry j starts a group, else 0; a workgroup takes
//            KT_WELD_CHUNK entries
//   scan     the list's scan_max over hp: every entry learns the sorted position of its group's head
//   reps     rep[si[j]] = si[head position]: back in input order; a vertex is kept when rep[i] == i
//   count    a wave counts the kept vertices of its 256 (ballots); kt_scan_runs_kernel turns the counts into first output indices
//   compact  the ballot rank gives every vertex the number of kept vertices below it (newidx); a kept vertex moves its 16 bytes and
//            its key there
//   spans    span_first_out from newidx
//   map      rep[i] = newidx[rep[i]] in place: the new index of every vertex's representative
//   remap    every triangle index t becomes map[t]
// heads, reps, count, spans, map and the span search are kt_wave.hpp's (kt_runs_*_kernel, kt_span_of): kt_mesh_simplify.hip runs the same
// code.
// compact and remap write the caller's buffers only when the kept count fits vertex_capacity and no key had a top bit set: they read
// both facts from device memory, so the whole call is enqueued at once and the host waits once.
#include "kt_mesh_keys.hpp"
#include "kt_wave.hpp"

#define KT_WELD_LANES 256
#define KT_WELD_CHUNK 2048            // sorted entries per workgroup of the head pass
#define KT_WELD_PER_WAVE KT_RUNS_PER_WAVE   // vertices per wave of the count and compact passes
#define KT_WELD_KEY_BITS 62
#define KT_WELD_MAX_VERTICES ((size_t)1 << 29)

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

// the two facts that decide whether the caller's buffers are written: the kept count fits, and no key has a top bit set
__device__ __forceinline__ bool weld_writes(const u32* total, const u64* sk, u32 n, u64 cap)
{
    return (u64)*total <= cap && (sk[n - 1] >> KT_WELD_KEY_BITS) == 0;
}

__global__ __launch_bounds__(KT_WELD_LANES) void weld_compact(const uint4* __restrict__ v, const u64* __restrict__ keys, const u32* __restrict__ rep, u32 n,
                                                              const u32* __restrict__ cnt, const u32* __restrict__ total, const u64* __restrict__ sk, u64 cap,
                                                              uint4* __restrict__ vout, u64* __restrict__ kout, u32* __restrict__ newidx)
{
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * (KT_WELD_LANES / 64) + (threadIdx.x >> 6);
    const size_t base = w * KT_WELD_PER_WAVE;
    if (base >= n) return;   // wave-uniform
    const bool writes = weld_writes(total, sk, n, cap);
    u32 o = cnt[w];
#pragma unroll
    for (int k = 0; k < KT_WELD_PER_WAVE / 64; ++k) {
        const size_t i = base + 64 * k + lane;
        const bool in = i < n, kept = in && rep[i] == (u32)i;
        const u64 b = __ballot(kept);
        const u32 r = o + kt_wave_rank(b, lane);
        if (in) newidx[i] = r;
        if (kept && writes) { vout[r] = v[i]; kout[r] = keys[i]; }
        o += (u32)__popcll(b);
    }
}

// (an index at or above n names no vertex: it stays as it is)
__global__ __launch_bounds__(KT_WELD_LANES) void weld_remap(u32* __restrict__ tri, size_t m3, const u32* __restrict__ map, u32 n, const u32* __restrict__ total,
                                                            const u64* __restrict__ sk, u64 cap)
{
    if (!weld_writes(total, sk, n, cap)) return;
    const size_t stride = (size_t)gridDim.x * KT_WELD_LANES;
    for (size_t k = (size_t)blockIdx.x * KT_WELD_LANES + threadIdx.x; k < m3; k += stride) {
        const u32 t = tri[k];
        if (t < n) tri[k] = map[t];
    }
}

}  // namespace

struct weld_per_vertex {
    u32 *hp, *hps, *rep, *cnt;        // device, a word per vertex (cnt: one per KT_WELD_PER_WAVE vertices): head positions before and after
                                      // the scan (hp is newidx once the scan has read it), representatives, kept counts
};
struct weld_staging { uint4 *v, *vo; u64 *k, *ko; u32* t; };

struct kt_mesh_welder : kt_pass_head {   // (kt_mesh_pass.hpp)
    u32* res;                         // device: the kept count
    u64* res_host;                    // pinned, 2 words: the kept count, the last sorted key
    kt_sorted_keys<true> srt;         // (kt_mesh_keys.hpp) sized by vertices
    kt_group<weld_per_vertex> ws;     // sized by vertices
    kt_span_table sp;                 // (with the spans' times in front)
    kt_group<weld_staging, 3> st;     // the host form's staging, sized by vertices in, triangles, vertices out
};

extern "C" int kt_mesh_weld_destroy(kt_mesh_welder* w) { return kt_pass_destroy(w); }

extern "C" int kt_mesh_weld_create(kt_ctx* c, void* hip_stream, kt_mesh_welder** out) { return kt_pass_create(c, hip_stream, out, 1, 2); }

namespace {

int weld_reserve(kt_mesh_welder* w, size_t n)
{
    KT_TRY(w->srt.reserve(w->stream, n));
    return w->ws.grow(w->stream, {n}, [](kt_mem& mem, weld_per_vertex& g, const size_t* c) {
        int s = mem.device(&g.hp, c[0]);
        if (s == KT_OK) s = mem.device(&g.hps, c[0]);
        if (s == KT_OK) s = mem.device(&g.rep, c[0]);
        if (s == KT_OK) s = mem.device(&g.cnt, (c[0] + KT_WELD_PER_WAVE - 1) / KT_WELD_PER_WAVE);
        return s;
    });
}

int weld_reserve_staging(kt_mesh_welder* w, size_t n, size_t m, size_t o)
{
    return w->st.grow(w->stream, {n, m, o}, [](kt_mem& mem, weld_staging& g, const size_t* c) {
        int s = mem.device(&g.v, c[0]);
        if (s == KT_OK) s = mem.device(&g.k, c[0]);
        if (s == KT_OK) s = mem.device(&g.t, 3 * c[1]);
        if (s == KT_OK) s = mem.device(&g.vo, c[2]);
        if (s == KT_OK) s = mem.device(&g.ko, c[2]);
        return s;
    });
}

// the checks both forms share: KT_ERR_ARG with nothing written
int weld_check(const kt_mesh_welder* w, const void* vertices, const void* keys, size_t n, const void* triangles, size_t m, const size_t* span_first,
               const uint64_t* span_time, int n_spans, const void* vertices_out, const void* keys_out, size_t vertex_capacity, const size_t* span_first_out,
               const size_t* n_out)
{
    KT_ARG(w && n_out && span_first_out && n <= KT_WELD_MAX_VERTICES && m <= ((size_t)1 << 40));
    KT_TRY(kt_mesh_check_inputs(vertices, n, triangles, m));
    KT_ARG((keys && ((uintptr_t)keys & 7) == 0) || n == 0);
    KT_TRY(kt_mesh_check_outputs(vertices_out, vertex_capacity, nullptr, 0, n, m));   // (the triangles are remapped in place)
    KT_ARG((keys_out && ((uintptr_t)keys_out & 7) == 0) || vertex_capacity == 0 || n == 0);
    KT_ARG(n == 0 || (vertices_out != vertices && keys_out != keys));   // the compaction is not in place
    KT_ARG(span_time || n_spans == 0);
    return kt_mesh_check_spans(span_first, n_spans, n);
}

}  // namespace

extern "C" int kt_mesh_weld_device(kt_mesh_welder* w, const kt_mesh_vertex* vertices_dev, const uint64_t* keys_dev, size_t n, uint32_t* triangles_dev, size_t m,
                                   const size_t* span_first, const uint64_t* span_time, int n_spans, uint64_t max_gap, kt_mesh_vertex* vertices_out_dev,
                                   uint64_t* keys_out_dev, size_t vertex_capacity, size_t* span_first_out, size_t* n_out)
{
    static_assert(sizeof(kt_mesh_vertex) == sizeof(uint4) && sizeof(u64) == sizeof(uint64_t), "vertex and key layout");
    KT_TRY(weld_check(w, vertices_dev, keys_dev, n, triangles_dev, m, span_first, span_time, n_spans, vertices_out_dev, keys_out_dev, vertex_capacity,
                      span_first_out, n_out));
    *n_out = 0;
    if (n == 0) { kt_mesh_empty_spans(span_first_out, n_spans); return KT_OK; }
    KT_HIP(hipSetDevice(w->ctx->device));
    KT_TRY(weld_reserve(w, n));
    hipStream_t st = w->stream;
    const size_t S = (size_t)n_spans;
    const u32 n32 = (u32)n;
    KT_TRY(w->sp.upload(st, span_first, n_spans, span_time));
    const u64* dt = w->sp.time();
    const u32* df = w->sp.first();
    u32* dfo = w->sp.first_out();
    const u64* keys = reinterpret_cast<const u64*>(keys_dev);
    KT_TRY(w->srt.sort(st, keys, n, "kt_mesh_weld"));
    const unsigned vblocks = (unsigned)((n + KT_WELD_LANES - 1) / KT_WELD_LANES);
    hipLaunchKernelGGL((kt_runs_heads_kernel<KT_WELD_LANES, KT_WELD_CHUNK, true>), dim3((unsigned)((n + KT_WELD_CHUNK - 1) / KT_WELD_CHUNK)), dim3(KT_WELD_LANES), 0, st,
                       (const u64*)w->srt.sk, (const u32*)w->srt.si, n32, df, dt, n_spans, (u64)max_gap, w->ws.hp);
    KT_LAUNCH_CHECK();
    KT_TRY(w->srt.scan_max(st, w->ws.hp, w->ws.hps, n, "kt_mesh_weld"));
    hipLaunchKernelGGL(kt_runs_reps_kernel<KT_WELD_LANES>, dim3(vblocks), dim3(KT_WELD_LANES), 0, st, w->srt.si, w->ws.hps, n32, w->ws.rep);
    KT_LAUNCH_CHECK();
    const size_t waves = (n + KT_WELD_PER_WAVE - 1) / KT_WELD_PER_WAVE;
    const unsigned wblocks = (unsigned)((waves + KT_WELD_LANES / 64 - 1) / (KT_WELD_LANES / 64));
    hipLaunchKernelGGL(kt_runs_count_kernel<KT_WELD_LANES>, dim3(wblocks), dim3(KT_WELD_LANES), 0, st, w->ws.rep, n32, w->ws.cnt);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kt_scan_runs_kernel<1>, dim3(1), dim3(256), 0, st, w->ws.cnt, (int)waves, w->res);
    KT_LAUNCH_CHECK();
    u32* newidx = w->ws.hp;
    hipLaunchKernelGGL(weld_compact, dim3(wblocks), dim3(KT_WELD_LANES), 0, st, reinterpret_cast<const uint4*>(vertices_dev), keys, w->ws.rep, n32, w->ws.cnt, w->res,
                       w->srt.sk, (u64)vertex_capacity, reinterpret_cast<uint4*>(vertices_out_dev), reinterpret_cast<u64*>(keys_out_dev), newidx);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kt_runs_spans_kernel<KT_WELD_LANES>, dim3((unsigned)((S + 1 + KT_WELD_LANES - 1) / KT_WELD_LANES)), dim3(KT_WELD_LANES), 0, st, df, (int)(S + 1), n32, newidx, w->res, dfo);
    KT_LAUNCH_CHECK();
    if (m > 0) {
        const size_t m3 = 3 * m;
        const unsigned rblocks = (unsigned)std::min<size_t>((m3 + KT_WELD_LANES - 1) / KT_WELD_LANES, 65536);
        hipLaunchKernelGGL(kt_runs_map_kernel<KT_WELD_LANES>, dim3(vblocks), dim3(KT_WELD_LANES), 0, st, w->ws.rep, newidx, n32);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(weld_remap, dim3(rblocks), dim3(KT_WELD_LANES), 0, st, triangles_dev, m3, w->ws.rep, n32, w->res, w->srt.sk, (u64)vertex_capacity);
        KT_LAUNCH_CHECK();
    }
    w->res_host[0] = 0;
    KT_HIP(hipMemcpyAsync(&w->res_host[0], w->res, sizeof(u32), hipMemcpyDeviceToHost, st));
    KT_HIP(hipMemcpyAsync(&w->res_host[1], w->srt.sk + (n - 1), sizeof(u64), hipMemcpyDeviceToHost, st));
    KT_TRY(w->sp.download(st));
    KT_HIP(hipStreamSynchronize(st));
    if (w->res_host[1] >> KT_WELD_KEY_BITS) {
        kt_set_error("kt_mesh_weld: a key with a top bit set (the largest is %#llx); nothing was written", w->res_host[1]);
        return KT_ERR_ARG;
    }
    *n_out = (size_t)w->res_host[0];
    if (*n_out > vertex_capacity) {
        kt_set_error("kt_mesh_weld: %zu welded vertices do not fit (capacity %zu); nothing was written", *n_out, vertex_capacity);
        return KT_ERR_CAPACITY;
    }
    w->sp.get(span_first_out);
    return KT_OK;
}

extern "C" int kt_mesh_weld(kt_mesh_welder* w, const kt_mesh_vertex* vertices, const uint64_t* keys, size_t n, uint32_t* triangles, size_t m, const size_t* span_first,
                            const uint64_t* span_time, int n_spans, uint64_t max_gap, kt_mesh_vertex* vertices_out, uint64_t* keys_out, size_t vertex_capacity,
                            size_t* span_first_out, size_t* n_out)
{
    KT_TRY(weld_check(w, vertices, keys, n, triangles, m, span_first, span_time, n_spans, vertices_out, keys_out, vertex_capacity, span_first_out, n_out));
    *n_out = 0;
    if (n == 0) { kt_mesh_empty_spans(span_first_out, n_spans); return KT_OK; }
    KT_HIP(hipSetDevice(w->ctx->device));
    const size_t cap = std::min(vertex_capacity, n);   // (the kept count is at most n)
    KT_TRY(weld_reserve_staging(w, n, m, cap));
    const size_t tbytes = 3 * m * sizeof(uint32_t);
    return kt_mesh_host_form(w->stream, {{w->st.v, vertices, n * sizeof(kt_mesh_vertex)}, {w->st.k, keys, n * sizeof(uint64_t)}, {w->st.t, triangles, tbytes}}, [&] {
        return kt_mesh_weld_device(w, reinterpret_cast<const kt_mesh_vertex*>(w->st.v), reinterpret_cast<const uint64_t*>(w->st.k), n, w->st.t, m, span_first, span_time,
                                   n_spans, max_gap, reinterpret_cast<kt_mesh_vertex*>(w->st.vo), reinterpret_cast<uint64_t*>(w->st.ko), cap, span_first_out, n_out);
    }, [&](kt_host_copy* down) {
        down[0] = {vertices_out, w->st.vo, *n_out * sizeof(kt_mesh_vertex)};
        down[1] = {keys_out, w->st.ko, *n_out * sizeof(uint64_t)};
        down[2] = {triangles, w->st.t, tbytes};
    });
}
