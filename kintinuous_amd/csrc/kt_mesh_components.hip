// kt_mesh_components.hip -- drops the small disconnected pieces of the -m mesh (kt_mesh_components, kt_mesh_components_device).
//
// Not in the reference: its -m grows surfaces from seeds over the processed cloud (backend/MeshGenerator.cpp) and never shows an island.
// The mesh of kt_mesh.hip is cut straight from the volume and keeps every speckle of depth noise as a few triangles joined to nothing.
// This pass labels the connected components of the mesh and keeps those with at least min_triangles triangles.
//
// Semantics (include/kt_abi.h; restated in numpy by kintinuous_amd/mesh_components_ref.py, which the device equals on every byte, on
// every call):
//   - two vertices are joined when one triangle holds both (a triangle with repeated indices joins what it names); position plays no
//     part; an index >= n fails the call;
//   - label[v] = the smallest vertex index of v's component; size of a component = the triangles whose FIRST index carries its label
//     (duplicates count each time; an unreferenced vertex is a component of size 0);
//   - kept: size >= min_triangles.  Output vertices = those of kept components in input order, 16 bytes untouched; output triangles =
//     those of kept components in input order, orientation kept, indices renumbered; span_first_out[s] = the kept vertices below
//     span_first[s]; labels_out[v] = label[v] for every INPUT vertex; stats = {all components, the kept ones, the largest size}.
//
// The passes, all on the object's stream, integers only (the union-find and its termination arguments: kt_unionfind.hpp):
//   init     parent[v] = v, size[v] = 0
//   hook     one lane per triangle: unite(i0, i1), unite(i0, i2); an index >= n ORs a bit into the status word and the lane does nothing
//   flatten  one lane per vertex: parent[v] = find(v) (by atomic minimum, so that the walks of other lanes through v stay valid).  The
//            root of a component is its smallest index, so parent IS the label afterwards
//   sizes    one lane per triangle: size[label[i0]] += 1; the lanes of a wave that share the label of its lowest lane are added by that
//            lane at once (a real mesh is mostly one component: without this every triangle's atomic lands on one word)
//   mark     grid-stride, at most KT_CMP_MARK_BLOCKS workgroups: rep[v] = v when size[label[v]] >= min_triangles, else KT_CMP_DROPPED;
//            a wave counts the roots it meets (ballots) and keeps the largest size, and adds them once at its end: the stats
//   kt_runs_count_kernel, kt_scan_runs_kernel<1>, kt_runs_rank_kernel (newidx[v] = the kept vertices below v), kt_runs_spans_kernel (kt_wave.hpp)
//   tcount   a wave counts the kept of its 256 triangles (rep[i0] == i0: a triangle's three vertices share their component);
//            kt_scan_runs_kernel<1> gives every wave its first output position
//   vwrite   the kept vertices to newidx[v], the labels of all; twrite: the kept triangles, every index through newidx
// vwrite and twrite write the caller's buffers only when the status word is clear and both counts fit: they read these facts from device
// memory, so the whole call is enqueued at once and the host waits once, for six words and the span table.  Nothing here depends on the
// order of arrival: the union-find ends at the same forest roots under every interleaving, every sum is an integer sum.
// The workspace: 16 bytes per vertex (parent, size, rep, newidx) and one word per 256 vertices and per 256 triangles.
#include "kt_mesh_pass.hpp"
#include "kt_unionfind.hpp"
#include "kt_wave.hpp"

#define KT_CMP_LANES 256
#define KT_CMP_PER_WAVE KT_RUNS_PER_WAVE   // vertices (triangles) per wave of the count, rank, tcount and twrite passes
#define KT_CMP_MAX_VERTICES ((size_t)1 << 29)
#define KT_CMP_MAX_TRIANGLES ((size_t)1 << 29)
#define KT_CMP_DROPPED 0xffffffffu    // rep of a dropped vertex: no index (n <= 2^29)
#define KT_CMP_RES 6                  // the result words: status, n_out, m_out, components, kept components, largest
#define KT_CMP_BAD_INDEX 1u
#define KT_CMP_MARK_BLOCKS 512        // of the grid-stride mark pass: at most 2048 waves add to the three stats words (a second round from 131073 vertices on)

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

__global__ __launch_bounds__(KT_CMP_LANES) void cmp_init(u32* __restrict__ parent, u32* __restrict__ size, u32 n)
{
    const size_t v = (size_t)blockIdx.x * KT_CMP_LANES + threadIdx.x;
    if (v < n) { parent[v] = (u32)v; size[v] = 0u; }
}

__global__ __launch_bounds__(KT_CMP_LANES) void cmp_hook(const u32* __restrict__ tri, size_t m, u32 n, u32* parent, u32* __restrict__ res)
{
    const size_t t = (size_t)blockIdx.x * KT_CMP_LANES + threadIdx.x;
    if (t >= m) return;
    const u32 i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    if (i0 >= n || i1 >= n || i2 >= n) { atomicOr(res, KT_CMP_BAD_INDEX); return; }
    if (i1 != i0) kt_uf_unite(parent, i0, i1);
    if (i2 != i0 && i2 != i1) kt_uf_unite(parent, i0, i2);
}

__global__ __launch_bounds__(KT_CMP_LANES) void cmp_sizes(const u32* __restrict__ tri, size_t m, u32 n, const u32* __restrict__ label, u32* __restrict__ size)
{
    const int lane = threadIdx.x & 63;
    const size_t t = (size_t)blockIdx.x * KT_CMP_LANES + threadIdx.x;
    if (t - lane >= m) return;   // wave-uniform
    u32 l = 0;
    bool mine = false;
    if (t < m) {
        const u32 i0 = tri[3 * t];
        mine = i0 < n;           // (an index out of range has set the status word: nothing will be written)
        if (mine) l = label[i0];
    }
    // the lanes that share the label of the lowest lane are added by that lane at once; the others add their own one
    const u64 all = __ballot(mine);
    if (!all) return;
    const int lead = __ffsll((long long)all) - 1;
    const u32 ll = __shfl(l, lead, 64);
    const u64 same = __ballot(mine && l == ll);
    if (lane == lead) atomicAdd(size + ll, (u32)__popcll(same));
    else if (mine && l != ll) atomicAdd(size + l, 1u);
}

// res[3], res[4], res[5]: the components, the kept ones, the largest size
__global__ __launch_bounds__(KT_CMP_LANES) void cmp_mark(const u32* __restrict__ label, const u32* __restrict__ size, u32 n, u32 min_triangles, u32* __restrict__ rep,
                                                         u32* __restrict__ res)
{
    const int lane = threadIdx.x & 63;
    const size_t stride = (size_t)gridDim.x * KT_CMP_LANES;
    u32 roots = 0, kept_roots = 0, big = 0;   // of this wave, over its rounds
    for (size_t base = (size_t)blockIdx.x * KT_CMP_LANES + threadIdx.x - lane; base < n; base += stride) {   // wave-uniform; ceil(n / stride) rounds
        const size_t v = base + lane;
        bool root = false, kept = false;
        if (v < n) {
            const u32 l = label[v], s = size[l];
            root = l == (u32)v;
            kept = s >= min_triangles;
            rep[v] = kept ? (u32)v : KT_CMP_DROPPED;
            if (root) big = max(big, s);
        }
        roots += (u32)__popcll(__ballot(root));
        kept_roots += (u32)__popcll(__ballot(root && kept));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) big = max(big, (u32)__shfl_xor(big, off, 64));
    if (lane == 0 && roots) {
        atomicAdd(res + 3, roots);
        if (kept_roots) atomicAdd(res + 4, kept_roots);
        if (big) atomicMax(res + 5, big);
    }
}

// a triangle is kept with its first vertex (its three vertices share their component); one out of range is not
__device__ __forceinline__ bool cmp_tkept(const u32* __restrict__ tri, size_t t, size_t m, u32 n, const u32* __restrict__ rep)
{
    if (t >= m) return false;
    const u32 i0 = tri[3 * t];
    return i0 < n && rep[i0] == i0;
}

__global__ __launch_bounds__(KT_CMP_LANES) void cmp_tcount(const u32* __restrict__ tri, size_t m, u32 n, const u32* __restrict__ rep, u32* __restrict__ tcnt)
{
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * (KT_CMP_LANES / 64) + (threadIdx.x >> 6);
    const size_t base = w * KT_CMP_PER_WAVE;
    if (base >= m) return;   // wave-uniform
    u32 c = 0;
#pragma unroll
    for (int k = 0; k < KT_CMP_PER_WAVE / 64; ++k) c += (u32)__popcll(__ballot(cmp_tkept(tri, base + 64 * k + lane, m, n, rep)));
    if (lane == 0) tcnt[w] = c;
}

// the facts that decide whether the caller's buffers are written: every index in range, both counts fit
__device__ __forceinline__ bool cmp_writes(const u32* res, u64 vcap, u64 tcap) { return res[0] == 0 && (u64)res[1] <= vcap && (u64)res[2] <= tcap; }

__global__ __launch_bounds__(KT_CMP_LANES) void cmp_vwrite(const uint4* __restrict__ v, u32 n, const u32* __restrict__ label, const u32* __restrict__ rep,
                                                           const u32* __restrict__ newidx, const u32* __restrict__ res, u64 vcap, u64 tcap, uint4* __restrict__ vout,
                                                           u32* __restrict__ labels_out)
{
    const size_t i = (size_t)blockIdx.x * KT_CMP_LANES + threadIdx.x;
    if (i >= n || !cmp_writes(res, vcap, tcap)) return;
    if (rep[i] == (u32)i) vout[newidx[i]] = v[i];   // (newidx[i] < res[1] <= vcap)
    if (labels_out) labels_out[i] = label[i];
}

__global__ __launch_bounds__(KT_CMP_LANES) void cmp_twrite(const u32* __restrict__ tri, size_t m, u32 n, const u32* __restrict__ rep, const u32* __restrict__ newidx,
                                                           const u32* __restrict__ tcnt, const u32* __restrict__ res, u64 vcap, u64 tcap, u32* __restrict__ tout)
{
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * (KT_CMP_LANES / 64) + (threadIdx.x >> 6);
    const size_t base = w * KT_CMP_PER_WAVE;
    if (base >= m) return;   // wave-uniform
    if (!cmp_writes(res, vcap, tcap)) return;
    size_t o = tcnt[w];
#pragma unroll
    for (int k = 0; k < KT_CMP_PER_WAVE / 64; ++k) {
        const size_t t = base + 64 * k + lane;
        const bool kept = cmp_tkept(tri, t, m, n, rep);
        const u64 b = __ballot(kept);
        if (kept) {   // (the status word is clear: all three indices are below n, and kept like the first)
            u32* d = tout + 3 * (o + kt_wave_rank(b, lane));
            d[0] = newidx[tri[3 * t]]; d[1] = newidx[tri[3 * t + 1]]; d[2] = newidx[tri[3 * t + 2]];
        }
        o += (size_t)__popcll(b);
    }
}

}  // namespace

struct cmp_per_vertex { u32 *parent, *size, *rep, *newidx, *cnt; };   // device, a word per vertex (cnt: one per KT_CMP_PER_WAVE vertices); parent is the label once flattened
struct cmp_per_triangle { u32* tcnt; };                                // device: one count per wave

struct kt_mesh_component_pass : kt_pass_head {   // (kt_mesh_pass.hpp)
    u32* res;                         // device, KT_CMP_RES
    u32* res_host;                    // pinned, KT_CMP_RES
    kt_group<cmp_per_vertex> ws;      // sized by vertices
    kt_group<cmp_per_triangle> tc;    // sized by waves of KT_CMP_PER_WAVE triangles
    kt_span_table sp;
    kt_mesh_staging st;               // (l: the labels)
};

extern "C" int kt_mesh_components_destroy(kt_mesh_component_pass* w) { return kt_pass_destroy(w); }

extern "C" int kt_mesh_components_create(kt_ctx* c, void* hip_stream, kt_mesh_component_pass** out) { return kt_pass_create(c, hip_stream, out, KT_CMP_RES, KT_CMP_RES); }

namespace {

int cmp_reserve(kt_mesh_component_pass* w, size_t n)
{
    return w->ws.grow(w->stream, {n}, [](kt_mem& mem, cmp_per_vertex& g, const size_t* c) {
        int s = mem.device(&g.parent, c[0]);
        if (s == KT_OK) s = mem.device(&g.size, c[0]);
        if (s == KT_OK) s = mem.device(&g.rep, c[0]);
        if (s == KT_OK) s = mem.device(&g.newidx, c[0]);
        if (s == KT_OK) s = mem.device(&g.cnt, (c[0] + KT_CMP_PER_WAVE - 1) / KT_CMP_PER_WAVE);
        return s;
    });
}

int cmp_reserve_triangles(kt_mesh_component_pass* w, size_t waves)
{
    return w->tc.grow(w->stream, {waves}, [](kt_mem& mem, cmp_per_triangle& g, const size_t* c) { return mem.device(&g.tcnt, c[0]); });
}

// the checks both forms share: KT_ERR_ARG with nothing written, before any allocation or launch
int cmp_check(const kt_mesh_component_pass* w, const void* vertices, size_t n, const void* triangles, size_t m, const size_t* span_first, int n_spans,
              const void* vertices_out, size_t vertex_capacity, const void* triangles_out, size_t triangle_capacity, const void* labels_out,
              const size_t* span_first_out, const size_t* n_out, const size_t* m_out, const kt_mesh_component_stats* stats)
{
    KT_ARG(w && n_out && m_out && span_first_out && stats && n <= KT_CMP_MAX_VERTICES && m <= KT_CMP_MAX_TRIANGLES);
    KT_TRY(kt_mesh_check_inputs(vertices, n, triangles, m));
    KT_TRY(kt_mesh_check_outputs(vertices_out, vertex_capacity, triangles_out, triangle_capacity, n, m));
    if (n > 0) {
        const kt_byte_range ins[2] = {{vertices, n * sizeof(kt_mesh_vertex)}, {triangles, 3 * m * sizeof(uint32_t)}};
        const kt_byte_range outs[3] = {{vertices_out, std::min(vertex_capacity, n) * sizeof(kt_mesh_vertex)},
                                       {triangles_out, 3 * std::min(triangle_capacity, m) * sizeof(uint32_t)}, {labels_out, n * sizeof(uint32_t)}};
        KT_TRY(kt_mesh_check_disjoint(outs, 3, ins, 2));
    }
    return kt_mesh_check_spans(span_first, n_spans, n);
}

// the answers for an empty mesh
void cmp_empty(int n_spans, size_t* span_first_out, kt_mesh_component_stats* stats)
{
    kt_mesh_empty_spans(span_first_out, n_spans);
    stats->components = stats->kept_components = stats->largest = 0;
}

}  // namespace

extern "C" int kt_mesh_components_device(kt_mesh_component_pass* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m,
                                         const size_t* span_first, int n_spans, uint32_t min_triangles, kt_mesh_vertex* vertices_out_dev, size_t vertex_capacity,
                                         uint32_t* triangles_out_dev, size_t triangle_capacity, uint32_t* labels_out_dev, size_t* span_first_out, size_t* n_out,
                                         size_t* m_out, kt_mesh_component_stats* stats)
{
    static_assert(sizeof(kt_mesh_vertex) == sizeof(uint4), "vertex layout");
    KT_TRY(cmp_check(w, vertices_dev, n, triangles_dev, m, span_first, n_spans, vertices_out_dev, vertex_capacity, triangles_out_dev, triangle_capacity, labels_out_dev,
                     span_first_out, n_out, m_out, stats));
    *n_out = 0; *m_out = 0;
    if (n == 0) { cmp_empty(n_spans, span_first_out, stats); return KT_OK; }
    KT_HIP(hipSetDevice(w->ctx->device));
    const size_t twaves = (m + KT_CMP_PER_WAVE - 1) / KT_CMP_PER_WAVE;
    KT_TRY(cmp_reserve(w, n));
    KT_TRY(cmp_reserve_triangles(w, twaves));
    hipStream_t st = w->stream;
    const size_t S = (size_t)n_spans;
    const u32 n32 = (u32)n;
    KT_TRY(w->sp.upload(st, span_first, n_spans));
    const u32* df = w->sp.first();
    u32* dfo = w->sp.first_out();
    KT_HIP(hipMemsetAsync(w->res, 0, KT_CMP_RES * sizeof(u32), st));
    const uint4* v = reinterpret_cast<const uint4*>(vertices_dev);
    const unsigned vblocks = (unsigned)((n + KT_CMP_LANES - 1) / KT_CMP_LANES), mblocks = (unsigned)((m + KT_CMP_LANES - 1) / KT_CMP_LANES);
    hipLaunchKernelGGL(cmp_init, dim3(vblocks), dim3(KT_CMP_LANES), 0, st, w->ws.parent, w->ws.size, n32);
    KT_LAUNCH_CHECK();
    if (m > 0) {
        hipLaunchKernelGGL(cmp_hook, dim3(mblocks), dim3(KT_CMP_LANES), 0, st, triangles_dev, m, n32, w->ws.parent, w->res);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(kt_uf_flatten_kernel<KT_CMP_LANES>, dim3(vblocks), dim3(KT_CMP_LANES), 0, st, w->ws.parent, n32);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(cmp_sizes, dim3(mblocks), dim3(KT_CMP_LANES), 0, st, triangles_dev, m, n32, (const u32*)w->ws.parent, w->ws.size);
        KT_LAUNCH_CHECK();
    }
    const u32* label = w->ws.parent;
    hipLaunchKernelGGL(cmp_mark, dim3(std::min<unsigned>(vblocks, KT_CMP_MARK_BLOCKS)), dim3(KT_CMP_LANES), 0, st, label, (const u32*)w->ws.size, n32, (u32)min_triangles, w->ws.rep, w->res);
    KT_LAUNCH_CHECK();
    const size_t waves = (n + KT_CMP_PER_WAVE - 1) / KT_CMP_PER_WAVE;
    const unsigned wblocks = (unsigned)((waves + KT_CMP_LANES / 64 - 1) / (KT_CMP_LANES / 64));
    hipLaunchKernelGGL(kt_runs_count_kernel<KT_CMP_LANES>, dim3(wblocks), dim3(KT_CMP_LANES), 0, st, (const u32*)w->ws.rep, n32, w->ws.cnt);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kt_scan_runs_kernel<1>, dim3(1), dim3(256), 0, st, w->ws.cnt, (int)waves, w->res + 1);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kt_runs_rank_kernel<KT_CMP_LANES>, dim3(wblocks), dim3(KT_CMP_LANES), 0, st, (const u32*)w->ws.rep, n32, (const u32*)w->ws.cnt, w->ws.newidx);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kt_runs_spans_kernel<KT_CMP_LANES>, dim3((unsigned)((S + 1 + KT_CMP_LANES - 1) / KT_CMP_LANES)), dim3(KT_CMP_LANES), 0, st, df, (int)(S + 1), n32,
                       (const u32*)w->ws.newidx, (const u32*)(w->res + 1), dfo);
    KT_LAUNCH_CHECK();
    const unsigned tblocks = (unsigned)((twaves + KT_CMP_LANES / 64 - 1) / (KT_CMP_LANES / 64));
    if (m > 0) {
        hipLaunchKernelGGL(cmp_tcount, dim3(tblocks), dim3(KT_CMP_LANES), 0, st, triangles_dev, m, n32, (const u32*)w->ws.rep, w->tc.tcnt);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(kt_scan_runs_kernel<1>, dim3(1), dim3(256), 0, st, w->tc.tcnt, (int)twaves, w->res + 2);
        KT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(cmp_vwrite, dim3(vblocks), dim3(KT_CMP_LANES), 0, st, v, n32, label, (const u32*)w->ws.rep, (const u32*)w->ws.newidx, (const u32*)w->res,
                       (u64)vertex_capacity, (u64)triangle_capacity, reinterpret_cast<uint4*>(vertices_out_dev), labels_out_dev);
    KT_LAUNCH_CHECK();
    if (m > 0) {
        hipLaunchKernelGGL(cmp_twrite, dim3(tblocks), dim3(KT_CMP_LANES), 0, st, triangles_dev, m, n32, (const u32*)w->ws.rep, (const u32*)w->ws.newidx, (const u32*)w->tc.tcnt,
                           (const u32*)w->res, (u64)vertex_capacity, (u64)triangle_capacity, triangles_out_dev);
        KT_LAUNCH_CHECK();
    }
    for (int k = 0; k < KT_CMP_RES; ++k) w->res_host[k] = 0;
    KT_HIP(hipMemcpyAsync(w->res_host, w->res, KT_CMP_RES * sizeof(u32), hipMemcpyDeviceToHost, st));
    KT_TRY(w->sp.download(st));
    KT_HIP(hipStreamSynchronize(st));
    const u32* r = w->res_host;
    if (r[0]) {
        kt_set_error("kt_mesh_components: a triangle index out of range; nothing was written");
        return KT_ERR_ARG;
    }
    *n_out = (size_t)r[1];
    *m_out = (size_t)r[2];
    if (*n_out > vertex_capacity || *m_out > triangle_capacity) {
        kt_set_error("kt_mesh_components: %zu vertices and %zu triangles do not fit (capacities %zu and %zu); nothing was written", *n_out, *m_out, vertex_capacity,
                     triangle_capacity);
        return KT_ERR_CAPACITY;
    }
    w->sp.get(span_first_out);
    stats->components = r[3]; stats->kept_components = r[4]; stats->largest = r[5];
    return KT_OK;
}

extern "C" int kt_mesh_components(kt_mesh_component_pass* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m, const size_t* span_first,
                                  int n_spans, uint32_t min_triangles, kt_mesh_vertex* vertices_out, size_t vertex_capacity, uint32_t* triangles_out,
                                  size_t triangle_capacity, uint32_t* labels_out, size_t* span_first_out, size_t* n_out, size_t* m_out, kt_mesh_component_stats* stats)
{
    KT_TRY(cmp_check(w, vertices, n, triangles, m, span_first, n_spans, vertices_out, vertex_capacity, triangles_out, triangle_capacity, labels_out, span_first_out,
                     n_out, m_out, stats));
    *n_out = 0; *m_out = 0;
    if (n == 0) { cmp_empty(n_spans, span_first_out, stats); return KT_OK; }
    KT_HIP(hipSetDevice(w->ctx->device));
    const size_t vcap = std::min(vertex_capacity, n), tcap = std::min(triangle_capacity, m);   // (neither count exceeds its input's)
    KT_TRY(w->st.reserve(w->stream, n, m, vcap, tcap, true));
    return kt_mesh_host_form(w->stream, {{w->st.v, vertices, n * sizeof(kt_mesh_vertex)}, {w->st.t, triangles, 3 * m * sizeof(uint32_t)}}, [&] {
        return kt_mesh_components_device(w, reinterpret_cast<const kt_mesh_vertex*>(w->st.v), n, w->st.t, m, span_first, n_spans, min_triangles,
                                         reinterpret_cast<kt_mesh_vertex*>(w->st.vo), vcap, w->st.to, tcap, labels_out ? w->st.l : nullptr, span_first_out, n_out, m_out, stats);
    }, [&](kt_host_copy* down) {
        down[0] = {vertices_out, w->st.vo, *n_out * sizeof(kt_mesh_vertex)};
        down[1] = {triangles_out, w->st.to, 3 * *m_out * sizeof(uint32_t)};
        down[2] = {labels_out, w->st.l, labels_out ? n * sizeof(uint32_t) : 0};
    });
}
