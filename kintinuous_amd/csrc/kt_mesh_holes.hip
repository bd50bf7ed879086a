// kt_mesh_holes.hip -- reports the open boundaries of the -m mesh and fills its small holes (kt_mesh_holes, kt_mesh_holes_device).
//
// Not in the reference: its -m grows one surface over the processed cloud (backend/MeshGenerator.cpp) and never asks whether it is closed.
// The mesh of kt_mesh.hip, welded by kt_mesh_weld.hip, keeps a crack where the sign change of a seam edge sits on another edge at the two
// times, and a one-cell gap where the cleared plane was never fused again.  This pass finds every boundary of the surface, tells the simple
// loops from the rest, and closes the loops of at most max_edges edges with a fan around their centre.  It is the first pass of the chain
// that works on half-edges, not vertices.
//
// Semantics (include/kt_abi.h; restated in numpy by kintinuous_amd/mesh_holes_ref.py, which the device equals on every byte, on every
// call):
//   - triangle t, corner k gives half-edge h = 3 t + k from a = tri[t][k] to b = tri[t][(k + 1) % 3]; a triangle with two equal indices is
//     degenerate: no half-edges, counted, copied like any other; an index >= n fails the call;
//   - an undirected edge with f half-edges min -> max and r the other way: f == r == 1 interior, f + r == 1 boundary, anything else
//     non-manifold (counted once, both ends BLOCKED);
//   - out[v], in[v]: the boundary half-edges that leave and enter v; in + out > 0 and not in == out == 1: COMPLEX;
//   - the boundary half-edges join their ends into components, labelled by their smallest vertex; a component without a COMPLEX or BLOCKED
//     vertex is a simple loop of L = its vertex count edges, any other is open;
//   - a simple loop is filled when 3 <= L <= max_edges and every vertex is valid (finite, |coordinate| < 8192); its centre is the mean of
//     its vertices by int64 sums of rint(x * 2^32), its colour the rounded mean per byte; one triangle (b, a, centre) per half-edge a -> b;
//   - output: every span keeps its vertices and takes the centres of the loops whose label it holds, ascending by label; the m triangles
//     through the index map, then the fill triangles ascending by h; span_first_out, loop_out, nine stats.
//
// The passes, all on the object's stream (the union-find and its termination arguments: kt_unionfind.hpp):
//   init      parent[v] = v; out, in, flag and len zero
//   keys      one lane per half-edge: key = min << 32 | max, all ones for a degenerate triangle or one with an index >= n (which ORs a
//             bit into the status word); a wave counts its degenerate triangles by ballot
//   sort      the sorted key list (kt_mesh_keys.hpp) of (key, h)
//   classify  one lane per sorted entry takes its class from kt_half_edge_class (kt_wave.hpp): a boundary half-edge gives hrep[h] = h,
//             out[a] += 1, in[b] += 1, unite(a, b); a non-manifold edge flag |= BLOCKED on both ends; both kinds are counted by ballot
//   flatten   parent[v] = find(v): parent IS the label afterwards
//   lengths   one lane per boundary vertex: len[label] += 1 (the lanes of a wave that share the label of its lowest lane are added by
//             that lane at once: a long rim is one label), flag[label] |= OPEN if COMPLEX or BLOCKED, |= INVALID if not valid
//   mark      grid-stride, at most KT_HOL_MARK_BLOCKS workgroups: frep[v] = v for a filled root, else no index; the loops, the open
//             components, the longest loop: ballots and one set of atomics per wave
//   kt_runs_count_kernel, kt_scan_runs_kernel<1>, kt_runs_rank_kernel over frep: rank[v] = the filled labels below v
//   map       map[v] = v + rank[first[span(v)]]: where input vertex v goes; n_out = n + filled
//   kt_runs_spans_kernel: span_first_out from map
//   sums      one lane per vertex of a filled loop: three int64 and four uint32 atomic sums onto the loop's rank (at most 256 per word)
//   hmark     hrep[h] stays h only where the loop of h is filled; kt_runs_count_kernel, kt_scan_runs_kernel<1> over hrep: every wave's
//             first fill triangle
//   vwrite    the input vertices to map[v], loop_out, the centres to first[span(label) + 1] + rank[label]
//   twrite    a wave per 256 half-edges: every index through map, and the fill triangles behind the m copies
// vwrite and twrite write the caller's buffers only when the status word is clear and both counts fit: they read these facts from device
// memory, so the whole call is enqueued at once and the host waits once, for ten words and the span table.  Nothing depends on the order
// of arrival: the union-find ends at the same roots under every interleaving, every count and every sum is an integer sum.
// The workspace: 32 bytes per vertex, 40 bytes per three vertices for the sums, 24 bytes per half-edge and the sort's own.
#include "kt_mesh_keys.hpp"
#include "kt_unionfind.hpp"
#include "kt_wave.hpp"

#define KT_HOL_LANES 256
#define KT_HOL_PER_WAVE KT_RUNS_PER_WAVE   // vertices (half-edges) per wave of the count, rank and twrite passes
#define KT_HOL_MAX_VERTICES ((size_t)1 << 29)
#define KT_HOL_MAX_TRIANGLES ((size_t)1 << 29)
#define KT_HOL_MAX_EDGES 256u
#define KT_HOL_NONE 0xffffffffu       // no index (n <= 2^29, 3 m < 2^32 - 1); loop_out of a vertex on no boundary
#define KT_HOL_OPEN_LOOP 0xfffffffeu  // loop_out of a boundary vertex of an open component
#define KT_HOL_BLOCKED 1u             // flag[v]: v ends a non-manifold edge
#define KT_HOL_OPEN 2u                // flag[label]: the component holds a COMPLEX or BLOCKED vertex
#define KT_HOL_INVALID 4u             // flag[label]: the component holds an invalid vertex
#define KT_HOL_RES 10                 // the result words: status, filled, fill triangles, boundary, non-manifold, degenerate, loops, open, longest, n_out
#define KT_HOL_BAD_INDEX 1u
#define KT_HOL_MARK_BLOCKS 512        // of the grid-stride mark pass

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

__global__ __launch_bounds__(KT_HOL_LANES) void hol_init(u32* __restrict__ parent, u32* __restrict__ outc, u32* __restrict__ inc, u32* __restrict__ flag,
                                                         u32* __restrict__ len, u32 n)
{
    const size_t v = (size_t)blockIdx.x * KT_HOL_LANES + threadIdx.x;
    if (v < n) { parent[v] = (u32)v; outc[v] = 0u; inc[v] = 0u; flag[v] = 0u; len[v] = 0u; }
}

__global__ __launch_bounds__(KT_HOL_LANES) void hol_keys(const u32* __restrict__ tri, u32 m3, u32 n, u64* __restrict__ keys, u32* __restrict__ hrep, u32* __restrict__ res)
{
    const int lane = threadIdx.x & 63;
    const size_t h = (size_t)blockIdx.x * KT_HOL_LANES + threadIdx.x;
    if (h - lane >= m3) return;   // wave-uniform
    bool degenerate = false;
    if (h < m3) {
        bool bad, deg;
        keys[h] = kt_half_edge_key(tri, (u32)h, n, &bad, &deg);   // (kt_wave.hpp)
        const bool first = (u32)h % 3u == 0u;
        if (bad && first) atomicOr(res, KT_HOL_BAD_INDEX);
        degenerate = deg && !bad && first;   // counted at its first corner
        hrep[h] = KT_HOL_NONE;
    }
    const u32 c = (u32)__popcll(__ballot(degenerate));
    if (lane == 0 && c) atomicAdd(res + 5, c);
}

__global__ __launch_bounds__(KT_HOL_LANES) void hol_classify(const u64* __restrict__ sk, const u32* __restrict__ sh, u32 m3, const u32* __restrict__ tri, u32* parent,
                                                             u32* __restrict__ outc, u32* __restrict__ inc, u32* __restrict__ flag, u32* __restrict__ hrep,
                                                             u32* __restrict__ res)
{
    const int lane = threadIdx.x & 63;
    const size_t j = (size_t)blockIdx.x * KT_HOL_LANES + threadIdx.x;
    if (j - lane >= m3) return;   // wave-uniform
    bool boundary = false, odd = false;
    if (j < m3) {
        const int c = kt_half_edge_class(sk, sh, tri, j, m3);   // (kt_wave.hpp)
        boundary = c == KT_HE_BOUNDARY;
        odd = c == KT_HE_NONMANIFOLD;
        if (boundary) {
            const u32 h = sh[j], a = tri[h], b = kt_half_edge_next(tri, h);
            hrep[h] = h;
            atomicAdd(outc + a, 1u);
            atomicAdd(inc + b, 1u);
            kt_uf_unite(parent, a, b);
        } else if (odd) {
            const u64 k = sk[j];
            atomicOr(flag + (u32)(k >> 32), KT_HOL_BLOCKED);
            atomicOr(flag + (u32)k, KT_HOL_BLOCKED);
        }
    }
    const u32 nb = (u32)__popcll(__ballot(boundary)), no = (u32)__popcll(__ballot(odd));
    if (lane == 0) {
        if (nb) atomicAdd(res + 3, nb);
        if (no) atomicAdd(res + 4, no);
    }
}

__global__ __launch_bounds__(KT_HOL_LANES) void hol_lengths(const uint4* __restrict__ v, u32 n, const u32* __restrict__ label, const u32* __restrict__ outc,
                                                            const u32* __restrict__ inc, u32* flag, u32* __restrict__ len)
{
    const int lane = threadIdx.x & 63;
    const size_t i = (size_t)blockIdx.x * KT_HOL_LANES + threadIdx.x;
    if (i - lane >= n) return;   // wave-uniform
    u32 l = 0, f = 0;
    bool mine = false;
    if (i < n) {
        const u32 o = outc[i], e = inc[i];
        mine = o + e > 0;
        if (mine) {
            l = label[i];
            if (o != 1u || e != 1u || (__hip_atomic_load(flag + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & KT_HOL_BLOCKED)) f |= KT_HOL_OPEN;
            if (!kt_mesh_valid(v[i])) f |= KT_HOL_INVALID;
        }
    }
    // the lanes that share the label of the lowest lane are added by that lane at once; the others add their own one
    const u64 all = __ballot(mine);
    if (!all) return;
    const int lead = __ffsll((long long)all) - 1;
    const u32 ll = __shfl(l, lead, 64);
    const u64 same = __ballot(mine && l == ll);
    if (lane == lead) atomicAdd(len + ll, (u32)__popcll(same));
    else if (mine && l != ll) atomicAdd(len + l, 1u);
    if (mine && f) atomicOr(flag + l, f);
}

// res[6], res[7], res[8]: the simple loops, the open components, the edges of the longest simple loop
__global__ __launch_bounds__(KT_HOL_LANES) void hol_mark(const u32* __restrict__ label, const u32* __restrict__ len, const u32* __restrict__ flag, u32 n, u32 max_edges,
                                                         u32* __restrict__ frep, u32* __restrict__ res)
{
    const int lane = threadIdx.x & 63;
    const size_t stride = (size_t)gridDim.x * KT_HOL_LANES;
    u32 loops = 0, open = 0, big = 0;   // of this wave, over its rounds
    for (size_t base = (size_t)blockIdx.x * KT_HOL_LANES + threadIdx.x - lane; base < n; base += stride) {   // wave-uniform; ceil(n / stride) rounds
        const size_t v = base + lane;
        bool simple = false, other = false;
        if (v < n) {
            const u32 L = len[v], f = flag[v];
            const bool root = L > 0 && label[v] == (u32)v;   // (len is added at labels only)
            simple = root && !(f & KT_HOL_OPEN);
            other = root && (f & KT_HOL_OPEN);
            frep[v] = simple && !(f & KT_HOL_INVALID) && L >= 3u && L <= max_edges ? (u32)v : KT_HOL_NONE;
            if (simple) big = max(big, L);
        }
        loops += (u32)__popcll(__ballot(simple));
        open += (u32)__popcll(__ballot(other));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) big = max(big, (u32)__shfl_xor(big, off, 64));
    if (lane == 0) {
        if (loops) atomicAdd(res + 6, loops);
        if (open) atomicAdd(res + 7, open);
        if (big) atomicMax(res + 8, big);
    }
}

// map[v]: where input vertex v goes: the centres of the spans before its own lie in front of it.  res[9] = n_out
__global__ __launch_bounds__(KT_HOL_LANES) void hol_map(const u32* __restrict__ first, int S, u32 n, const u32* __restrict__ rank, u32* __restrict__ map, u32* res)
{
    const size_t v = (size_t)blockIdx.x * KT_HOL_LANES + threadIdx.x;
    if (v == 0) res[9] = n + res[1];   // (one lane, two words; read by kt_runs_spans_kernel in a later launch)
    if (v < n) map[v] = (u32)v + rank[first[kt_span_of(first, S, (u32)v)]];   // (first[span(v)] <= v < n)
}

__global__ __launch_bounds__(KT_HOL_LANES) void hol_sums(const uint4* __restrict__ v, u32 n, const u32* __restrict__ label, const u32* __restrict__ outc,
                                                         const u32* __restrict__ inc, const u32* __restrict__ frep, const u32* __restrict__ rank, u64* __restrict__ sums,
                                                         u32* __restrict__ col)
{
    const size_t i = (size_t)blockIdx.x * KT_HOL_LANES + threadIdx.x;
    if (i >= n || outc[i] + inc[i] == 0u) return;
    const u32 l = label[i];
    if (frep[l] != l) return;
    const u32 r = rank[l];   // (below n / 3: filled loops are disjoint and have three vertices or more)
    const uint4 p = v[i];    // (valid: |q| < 2^45)
    atomicAdd(sums + 3 * (size_t)r, (u64)kt_q32(__uint_as_float(p.x)));
    atomicAdd(sums + 3 * (size_t)r + 1, (u64)kt_q32(__uint_as_float(p.y)));
    atomicAdd(sums + 3 * (size_t)r + 2, (u64)kt_q32(__uint_as_float(p.z)));
#pragma unroll
    for (int k = 0; k < 4; ++k) atomicAdd(col + 4 * (size_t)r + k, (p.w >> (8 * k)) & 255u);
}

// hrep[h] stays h only where the loop of boundary half-edge h is filled
__global__ __launch_bounds__(KT_HOL_LANES) void hol_hmark(const u32* __restrict__ tri, u32 m3, const u32* __restrict__ label, const u32* __restrict__ frep, u32* __restrict__ hrep)
{
    const size_t h = (size_t)blockIdx.x * KT_HOL_LANES + threadIdx.x;
    if (h >= m3 || hrep[h] != (u32)h) return;
    const u32 l = label[tri[h]];   // (a boundary half-edge: its indices are below n)
    if (frep[l] != l) hrep[h] = KT_HOL_NONE;
}

// the facts that decide whether the caller's buffers are written: every index in range, both counts fit
__device__ __forceinline__ bool hol_writes(const u32* res, u32 n, u64 m, u64 vcap, u64 tcap) { return res[0] == 0 && (u64)n + res[1] <= vcap && m + res[2] <= tcap; }

__device__ __forceinline__ u32 hol_centre_index(const u32* __restrict__ first, int S, const u32* __restrict__ rank, u32 l) { return first[kt_span_of(first, S, l) + 1] + rank[l]; }

__global__ __launch_bounds__(KT_HOL_LANES) void hol_vwrite(const uint4* __restrict__ v, u32 n, u64 m, const u32* __restrict__ label, const u32* __restrict__ outc,
                                                           const u32* __restrict__ inc, const u32* __restrict__ flag, const u32* __restrict__ len,
                                                           const u32* __restrict__ frep, const u32* __restrict__ rank, const u32* __restrict__ map,
                                                           const u64* __restrict__ sums, const u32* __restrict__ col, const u32* __restrict__ first, int S,
                                                           const u32* __restrict__ res, u64 vcap, u64 tcap, uint4* __restrict__ vout, u32* __restrict__ loop_out)
{
    const size_t i = (size_t)blockIdx.x * KT_HOL_LANES + threadIdx.x;
    if (i >= n || !hol_writes(res, n, m, vcap, tcap)) return;
    vout[map[i]] = v[i];   // (map[i] < n + res[1] <= vcap)
    if (loop_out) {
        const u32 l = label[i];
        loop_out[i] = outc[i] + inc[i] == 0u ? KT_HOL_NONE : (flag[l] & KT_HOL_OPEN) ? KT_HOL_OPEN_LOOP : l;
    }
    if (frep[i] != (u32)i) return;
    const u32 r = rank[i], L = len[i];
    const double dl = (double)L;
    uint4 c;
    c.x = __float_as_uint((float)((double)(long long)sums[3 * (size_t)r] / dl * (1.0 / 4294967296.0)));
    c.y = __float_as_uint((float)((double)(long long)sums[3 * (size_t)r + 1] / dl * (1.0 / 4294967296.0)));
    c.z = __float_as_uint((float)((double)(long long)sums[3 * (size_t)r + 2] / dl * (1.0 / 4294967296.0)));
    c.w = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) c.w |= ((2u * col[4 * (size_t)r + k] + L) / (2u * L)) << (8 * k);
    vout[hol_centre_index(first, S, rank, (u32)i)] = c;   // (below the first vertex of the next span in the output)
}

__global__ __launch_bounds__(KT_HOL_LANES) void hol_twrite(const u32* __restrict__ tri, u32 m3, u32 n, const u32* __restrict__ label, const u32* __restrict__ hrep,
                                                           const u32* __restrict__ hcnt, const u32* __restrict__ rank, const u32* __restrict__ map,
                                                           const u32* __restrict__ first, int S, const u32* __restrict__ res, u64 vcap, u64 tcap, u32* __restrict__ tout)
{
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * (KT_HOL_LANES / 64) + (threadIdx.x >> 6);
    const size_t base = w * KT_HOL_PER_WAVE;
    if (base >= m3) return;   // wave-uniform
    if (!hol_writes(res, n, (u64)(m3 / 3u), vcap, tcap)) return;
    size_t o = (size_t)(m3 / 3u) + hcnt[w];
#pragma unroll
    for (int k = 0; k < KT_HOL_PER_WAVE / 64; ++k) {
        const size_t h = base + 64 * k + lane;
        const bool in = h < m3;
        u32 a = 0;
        if (in) { a = tri[h]; tout[h] = map[a]; }   // (the status word is clear: every index is below n)
        const bool fill = in && hrep[h] == (u32)h;
        const u64 b = __ballot(fill);
        if (fill) {
            u32* d = tout + 3 * (o + kt_wave_rank(b, lane));   // (below m + res[2] <= tcap)
            d[0] = map[kt_half_edge_next(tri, (u32)h)]; d[1] = map[a]; d[2] = hol_centre_index(first, S, rank, label[a]);
        }
        o += (size_t)__popcll(b);
    }
}

}  // namespace

struct hol_per_vertex {
    u32 *parent, *outc, *inc, *flag, *len, *frep, *rank, *map, *cnt;   // device, a word per vertex (cnt: one per KT_HOL_PER_WAVE vertices); parent is the label once flattened
    u64* sums; u32* col;              // device, 3 and 4 per filled loop, vertices / 3 + 1 loops
};
struct hol_per_half_edge {
    u64* keys;                        // device, one per half-edge: the keys before the sort
    u32 *hrep, *hcnt;                 // device, one per half-edge (hcnt: one per KT_HOL_PER_WAVE half-edges): the fill marks, their counts
};

struct kt_mesh_hole_pass : kt_pass_head {   // (kt_mesh_pass.hpp)
    u32* res;                         // device, KT_HOL_RES
    u32* res_host;                    // pinned, KT_HOL_RES
    kt_group<hol_per_vertex> ws;      // sized by vertices
    kt_sorted_keys<false> srt;        // (kt_mesh_keys.hpp) sized by half-edges: sk, and the sorted half-edges as si
    kt_group<hol_per_half_edge> he;   // sized by half-edges
    kt_span_table sp;
    kt_mesh_staging st;               // (l: the loop words)
};

extern "C" int kt_mesh_holes_destroy(kt_mesh_hole_pass* w) { return kt_pass_destroy(w); }

extern "C" int kt_mesh_holes_create(kt_ctx* c, void* hip_stream, kt_mesh_hole_pass** out) { return kt_pass_create(c, hip_stream, out, KT_HOL_RES, KT_HOL_RES); }

namespace {

int hol_reserve(kt_mesh_hole_pass* w, size_t n)
{
    return w->ws.grow(w->stream, {n}, [](kt_mem& mem, hol_per_vertex& g, const size_t* c) {
        u32** per_vertex[8] = {&g.parent, &g.outc, &g.inc, &g.flag, &g.len, &g.frep, &g.rank, &g.map};
        int s = KT_OK;
        for (int k = 0; k < 8 && s == KT_OK; ++k) s = mem.device(per_vertex[k], c[0]);
        if (s == KT_OK) s = mem.device(&g.cnt, (c[0] + KT_HOL_PER_WAVE - 1) / KT_HOL_PER_WAVE);
        if (s == KT_OK) s = mem.device(&g.sums, 3 * (c[0] / 3 + 1));
        if (s == KT_OK) s = mem.device(&g.col, 4 * (c[0] / 3 + 1));
        return s;
    });
}

int hol_reserve_half_edges(kt_mesh_hole_pass* w, size_t m3)
{
    KT_TRY(w->srt.reserve(w->stream, m3));
    return w->he.grow(w->stream, {m3}, [](kt_mem& mem, hol_per_half_edge& g, const size_t* c) {
        int s = mem.device(&g.keys, c[0]);
        if (s == KT_OK) s = mem.device(&g.hrep, c[0]);
        if (s == KT_OK) s = mem.device(&g.hcnt, (c[0] + KT_HOL_PER_WAVE - 1) / KT_HOL_PER_WAVE);
        return s;
    });
}

// the most a call can give: a filled loop has three vertices or more of its own, and one fill triangle per vertex
size_t hol_most_vertices(size_t n) { return n + n / 3; }
size_t hol_most_triangles(size_t n, size_t m) { return m + std::min(n, 3 * m); }

// the checks both forms share: KT_ERR_ARG with nothing written, before any allocation or launch
int hol_check(const kt_mesh_hole_pass* w, const void* vertices, size_t n, const void* triangles, size_t m, const size_t* span_first, int n_spans, uint32_t max_edges,
              const void* vertices_out, size_t vertex_capacity, const void* triangles_out, size_t triangle_capacity, const void* loop_out, const size_t* span_first_out,
              const size_t* n_out, const size_t* m_out, const kt_mesh_hole_stats* stats)
{
    KT_ARG(w && n_out && m_out && span_first_out && stats && n <= KT_HOL_MAX_VERTICES && m <= KT_HOL_MAX_TRIANGLES);
    KT_ARG(max_edges <= KT_HOL_MAX_EDGES);
    KT_TRY(kt_mesh_check_inputs(vertices, n, triangles, m));
    KT_TRY(kt_mesh_check_outputs(vertices_out, vertex_capacity, triangles_out, triangle_capacity, n, m));
    if (n > 0) {
        const kt_byte_range ins[2] = {{vertices, n * sizeof(kt_mesh_vertex)}, {triangles, 3 * m * sizeof(uint32_t)}};
        const kt_byte_range outs[3] = {{vertices_out, std::min(vertex_capacity, hol_most_vertices(n)) * sizeof(kt_mesh_vertex)},
                                       {triangles_out, 3 * std::min(triangle_capacity, hol_most_triangles(n, m)) * sizeof(uint32_t)},
                                       {loop_out, n * sizeof(uint32_t)}};
        KT_TRY(kt_mesh_check_disjoint(outs, 3, ins, 2));
    }
    return kt_mesh_check_spans(span_first, n_spans, n);
}

// the answers for an empty mesh
void hol_empty(int n_spans, size_t* span_first_out, kt_mesh_hole_stats* s)
{
    kt_mesh_empty_spans(span_first_out, n_spans);
    s->boundary_edges = s->nonmanifold_edges = s->degenerate_triangles = s->loops = s->open_components = s->filled = s->longest = s->new_vertices = s->new_triangles = 0;
}

}  // namespace

extern "C" int kt_mesh_holes_device(kt_mesh_hole_pass* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m, const size_t* span_first,
                                    int n_spans, uint32_t max_edges, kt_mesh_vertex* vertices_out_dev, size_t vertex_capacity, uint32_t* triangles_out_dev,
                                    size_t triangle_capacity, uint32_t* loop_out_dev, size_t* span_first_out, size_t* n_out, size_t* m_out, kt_mesh_hole_stats* stats)
{
    static_assert(sizeof(kt_mesh_vertex) == sizeof(uint4), "vertex layout");
    KT_TRY(hol_check(w, vertices_dev, n, triangles_dev, m, span_first, n_spans, max_edges, vertices_out_dev, vertex_capacity, triangles_out_dev, triangle_capacity,
                     loop_out_dev, span_first_out, n_out, m_out, stats));
    *n_out = 0; *m_out = 0;
    if (n == 0) { hol_empty(n_spans, span_first_out, stats); return KT_OK; }
    KT_HIP(hipSetDevice(w->ctx->device));
    const size_t m3 = 3 * m;
    KT_TRY(hol_reserve(w, n));
    KT_TRY(hol_reserve_half_edges(w, m3));
    hipStream_t st = w->stream;
    const size_t S = (size_t)n_spans;
    const u32 n32 = (u32)n, m32 = (u32)m3;
    KT_TRY(w->sp.upload(st, span_first, n_spans));
    const u32* df = w->sp.first();
    u32* dfo = w->sp.first_out();
    KT_HIP(hipMemsetAsync(w->res, 0, KT_HOL_RES * sizeof(u32), st));
    KT_HIP(hipMemsetAsync(w->ws.sums, 0, 3 * (n / 3 + 1) * sizeof(u64), st));
    KT_HIP(hipMemsetAsync(w->ws.col, 0, 4 * (n / 3 + 1) * sizeof(u32), st));
    const uint4* v = reinterpret_cast<const uint4*>(vertices_dev);
    const unsigned vblocks = (unsigned)((n + KT_HOL_LANES - 1) / KT_HOL_LANES), hblocks = (unsigned)((m3 + KT_HOL_LANES - 1) / KT_HOL_LANES);
    hipLaunchKernelGGL(hol_init, dim3(vblocks), dim3(KT_HOL_LANES), 0, st, w->ws.parent, w->ws.outc, w->ws.inc, w->ws.flag, w->ws.len, n32);
    KT_LAUNCH_CHECK();
    if (m > 0) {
        hipLaunchKernelGGL(hol_keys, dim3(hblocks), dim3(KT_HOL_LANES), 0, st, triangles_dev, m32, n32, w->he.keys, w->he.hrep, w->res);
        KT_LAUNCH_CHECK();
        KT_TRY(w->srt.sort(st, w->he.keys, m3, "kt_mesh_holes"));
        hipLaunchKernelGGL(hol_classify, dim3(hblocks), dim3(KT_HOL_LANES), 0, st, (const u64*)w->srt.sk, (const u32*)w->srt.si, m32, triangles_dev, w->ws.parent, w->ws.outc, w->ws.inc,
                           w->ws.flag, w->he.hrep, w->res);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(kt_uf_flatten_kernel<KT_HOL_LANES>, dim3(vblocks), dim3(KT_HOL_LANES), 0, st, w->ws.parent, n32);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(hol_lengths, dim3(vblocks), dim3(KT_HOL_LANES), 0, st, v, n32, (const u32*)w->ws.parent, (const u32*)w->ws.outc, (const u32*)w->ws.inc, w->ws.flag, w->ws.len);
        KT_LAUNCH_CHECK();
    }
    const u32* label = w->ws.parent;
    hipLaunchKernelGGL(hol_mark, dim3(std::min<unsigned>(vblocks, KT_HOL_MARK_BLOCKS)), dim3(KT_HOL_LANES), 0, st, label, (const u32*)w->ws.len, (const u32*)w->ws.flag, n32,
                       (u32)max_edges, w->ws.frep, w->res);
    KT_LAUNCH_CHECK();
    const size_t waves = (n + KT_HOL_PER_WAVE - 1) / KT_HOL_PER_WAVE;
    const unsigned wblocks = (unsigned)((waves + KT_HOL_LANES / 64 - 1) / (KT_HOL_LANES / 64));
    hipLaunchKernelGGL(kt_runs_count_kernel<KT_HOL_LANES>, dim3(wblocks), dim3(KT_HOL_LANES), 0, st, (const u32*)w->ws.frep, n32, w->ws.cnt);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kt_scan_runs_kernel<1>, dim3(1), dim3(256), 0, st, w->ws.cnt, (int)waves, w->res + 1);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kt_runs_rank_kernel<KT_HOL_LANES>, dim3(wblocks), dim3(KT_HOL_LANES), 0, st, (const u32*)w->ws.frep, n32, (const u32*)w->ws.cnt, w->ws.rank);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(hol_map, dim3(vblocks), dim3(KT_HOL_LANES), 0, st, df, n_spans, n32, (const u32*)w->ws.rank, w->ws.map, w->res);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kt_runs_spans_kernel<KT_HOL_LANES>, dim3((unsigned)((S + 1 + KT_HOL_LANES - 1) / KT_HOL_LANES)), dim3(KT_HOL_LANES), 0, st, df, (int)(S + 1), n32,
                       (const u32*)w->ws.map, (const u32*)(w->res + 9), dfo);
    KT_LAUNCH_CHECK();
    const size_t hwaves = (m3 + KT_HOL_PER_WAVE - 1) / KT_HOL_PER_WAVE;
    const unsigned hwblocks = (unsigned)((hwaves + KT_HOL_LANES / 64 - 1) / (KT_HOL_LANES / 64));
    if (m > 0) {
        hipLaunchKernelGGL(hol_sums, dim3(vblocks), dim3(KT_HOL_LANES), 0, st, v, n32, label, (const u32*)w->ws.outc, (const u32*)w->ws.inc, (const u32*)w->ws.frep,
                           (const u32*)w->ws.rank, w->ws.sums, w->ws.col);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(hol_hmark, dim3(hblocks), dim3(KT_HOL_LANES), 0, st, triangles_dev, m32, label, (const u32*)w->ws.frep, w->he.hrep);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(kt_runs_count_kernel<KT_HOL_LANES>, dim3(hwblocks), dim3(KT_HOL_LANES), 0, st, (const u32*)w->he.hrep, m32, w->he.hcnt);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(kt_scan_runs_kernel<1>, dim3(1), dim3(256), 0, st, w->he.hcnt, (int)hwaves, w->res + 2);
        KT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(hol_vwrite, dim3(vblocks), dim3(KT_HOL_LANES), 0, st, v, n32, (u64)m, label, (const u32*)w->ws.outc, (const u32*)w->ws.inc, (const u32*)w->ws.flag,
                       (const u32*)w->ws.len, (const u32*)w->ws.frep, (const u32*)w->ws.rank, (const u32*)w->ws.map, (const u64*)w->ws.sums, (const u32*)w->ws.col, df, n_spans,
                       (const u32*)w->res, (u64)vertex_capacity, (u64)triangle_capacity, reinterpret_cast<uint4*>(vertices_out_dev), loop_out_dev);
    KT_LAUNCH_CHECK();
    if (m > 0) {
        hipLaunchKernelGGL(hol_twrite, dim3(hwblocks), dim3(KT_HOL_LANES), 0, st, triangles_dev, m32, n32, label, (const u32*)w->he.hrep, (const u32*)w->he.hcnt,
                           (const u32*)w->ws.rank, (const u32*)w->ws.map, df, n_spans, (const u32*)w->res, (u64)vertex_capacity, (u64)triangle_capacity, triangles_out_dev);
        KT_LAUNCH_CHECK();
    }
    for (int k = 0; k < KT_HOL_RES; ++k) w->res_host[k] = 0;
    KT_HIP(hipMemcpyAsync(w->res_host, w->res, KT_HOL_RES * sizeof(u32), hipMemcpyDeviceToHost, st));
    KT_TRY(w->sp.download(st));
    KT_HIP(hipStreamSynchronize(st));
    const u32* r = w->res_host;
    if (r[0]) {
        kt_set_error("kt_mesh_holes: a triangle index out of range; nothing was written");
        return KT_ERR_ARG;
    }
    *n_out = n + (size_t)r[1];
    *m_out = m + (size_t)r[2];
    if (*n_out > vertex_capacity || *m_out > triangle_capacity) {
        kt_set_error("kt_mesh_holes: %zu vertices and %zu triangles do not fit (capacities %zu and %zu); nothing was written", *n_out, *m_out, vertex_capacity,
                     triangle_capacity);
        return KT_ERR_CAPACITY;
    }
    w->sp.get(span_first_out);
    stats->boundary_edges = r[3]; stats->nonmanifold_edges = r[4]; stats->degenerate_triangles = r[5]; stats->loops = r[6]; stats->open_components = r[7];
    stats->filled = r[1]; stats->longest = r[8]; stats->new_vertices = r[1]; stats->new_triangles = r[2];
    return KT_OK;
}

extern "C" int kt_mesh_holes(kt_mesh_hole_pass* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m, const size_t* span_first, int n_spans,
                             uint32_t max_edges, kt_mesh_vertex* vertices_out, size_t vertex_capacity, uint32_t* triangles_out, size_t triangle_capacity,
                             uint32_t* loop_out, size_t* span_first_out, size_t* n_out, size_t* m_out, kt_mesh_hole_stats* stats)
{
    KT_TRY(hol_check(w, vertices, n, triangles, m, span_first, n_spans, max_edges, vertices_out, vertex_capacity, triangles_out, triangle_capacity, loop_out,
                     span_first_out, n_out, m_out, stats));
    *n_out = 0; *m_out = 0;
    if (n == 0) { hol_empty(n_spans, span_first_out, stats); return KT_OK; }
    KT_HIP(hipSetDevice(w->ctx->device));
    const size_t vcap = std::min(vertex_capacity, hol_most_vertices(n)), tcap = std::min(triangle_capacity, hol_most_triangles(n, m));
    KT_TRY(w->st.reserve(w->stream, n, m, vcap, tcap, true));
    return kt_mesh_host_form(w->stream, {{w->st.v, vertices, n * sizeof(kt_mesh_vertex)}, {w->st.t, triangles, 3 * m * sizeof(uint32_t)}}, [&] {
        return kt_mesh_holes_device(w, reinterpret_cast<const kt_mesh_vertex*>(w->st.v), n, w->st.t, m, span_first, n_spans, max_edges,
                                    reinterpret_cast<kt_mesh_vertex*>(w->st.vo), vcap, w->st.to, tcap, loop_out ? w->st.l : nullptr, span_first_out, n_out, m_out, stats);
    }, [&](kt_host_copy* down) {
        down[0] = {vertices_out, w->st.vo, *n_out * sizeof(kt_mesh_vertex)};
        down[1] = {triangles_out, w->st.to, 3 * *m_out * sizeof(uint32_t)};
        down[2] = {loop_out, w->st.l, loop_out ? n * sizeof(uint32_t) : 0};
    });
}
