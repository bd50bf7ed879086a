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
//
// The quadric form (kt_mesh_simplify_quadric, kt_mesh_simplify_quadric_device; Lindstrom 2000) keeps every pass above but the finish and
// puts a cluster of more than one member at the minimiser of the summed plane quadrics of the triangles that touch it, regularised
// towards the mean (include/kt_abi.h has the definition, operation by operation).  Between tcount and the finish it runs
//   qzero    the nine sums of the clusters there are (nine planes of n int64, taken on the first quadric call)
//   qsums    one lane per triangle: its indices (one at or above n ORs a bit into the status word), the rotation that puts the smallest
//            first, three 16-byte vertex loads, the cross product and the unit normal in double; then per distinct cluster among tm's
//            three the nine terms, bounded (|term| < 1, else a status bit) and rounded to 32.32.  A workgroup first adds by cluster in an
//            LDS table (a slot per cluster by compare-and-swap, 64-bit LDS adds: the pattern of kt_mesh_normals.hip) and then every used
//            slot adds its sums with up to nine 64-bit global atomics without a return value: a workgroup's triangles name few clusters,
//            and all of them ONE cluster in the worst case, which then costs nine global atomics per workgroup instead of nine per lane
//   qfinish  simp_finish with the 3 x 3 solve by the adjugate behind the mean, at most KT_SIMPQ_FINISH_BLOCKS workgroups striding over the
//            clusters; counts the placed clusters with one atomic per workgroup
// and twrite also reads the status word.
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
#define KT_SIMPQ_LANES 128            // the quadric sums: triangles per workgroup
#define KT_SIMPQ_SLOT_BITS 9
#define KT_SIMPQ_SLOTS (1 << KT_SIMPQ_SLOT_BITS)   // of a workgroup's table: four per lane, more than the three clusters of a lane's triangle (38 KB of LDS)
#define KT_SIMPQ_TERMS 9              // xx, xy, xz, yy, yz, zz, bx, by, bz
#define KT_SIMPQ_FREE 0xffffffffu     // no cluster: n <= 2^29
#define KT_SIMPQ_MAX_TRIANGLES ((size_t)1 << 29)   // |term| < 1 in 32.32, so |S| <= 2^61
#define KT_SIMPQ_FINISH_BLOCKS 1024   // of the quadric finish: every workgroup ends with one atomic on the placed count
#define KT_SIMPQ_BAD_INDEX 1u         // the bits of the status word (res[2])
#define KT_SIMPQ_TOO_LARGE 2u

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

// the representative of a cluster of k > 1 members from its sums a: the integer means (kept in mean[]) as floats, the colour bytes alike
__device__ __forceinline__ uint4 simp_mean(const u64* __restrict__ a, long long k, long long mean[3])
{
    u32 xyz[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        mean[e] = simp_floor_div(2 * (long long)a[e] + k, 2 * k);
        xyz[e] = __float_as_uint((float)((double)mean[e] * (1.0 / 1048576.0)));
    }
    u32 w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) w |= (u32)((2 * a[3 + e] + (u64)k) / (2 * (u64)k)) << (8 * e);
    return make_uint4(xyz[0], xyz[1], xyz[2], w);
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
        long long mean[3];
        if (k > 1) p = simp_mean(a, k, mean);   // (0: a cluster of one, which the sums pass never stored)
        vout[c] = p;
    }
}

// ---- the quadric form ----
// the nine sums of the clusters there are: totals[0] words of each plane of n
__global__ __launch_bounds__(KT_SIMP_LANES) void simp_qzero(u64* __restrict__ qacc, const u32* __restrict__ totals, u32 n)
{
    const size_t total = totals[0], words = total * KT_SIMPQ_TERMS, stride = (size_t)gridDim.x * KT_SIMP_LANES;
    for (size_t k = (size_t)blockIdx.x * KT_SIMP_LANES + threadIdx.x; k < words; k += stride) qacc[(k / total) * n + k % total] = 0ull;
}

// the word of cluster c's sum k: nine planes of n words, so that neighbouring clusters' atomics and the finish pass's reads are contiguous
__device__ __forceinline__ size_t simpq_word(u32 c, int k, u32 n) { return (size_t)k * n + c; }

__device__ __forceinline__ double simpq_coord(const uint4 p, int a) { return (double)__uint_as_float(a == 0 ? p.x : a == 1 ? p.y : p.z); }

// qacc: nine planes of n words, zero for the clusters there are.  tm: the three clusters of every triangle (simp_tcount).  res[2]: the status word
__global__ __launch_bounds__(KT_SIMPQ_LANES) void simp_qsums(const uint4* __restrict__ v, u32 n, const u32* __restrict__ tri, const u32* __restrict__ tm, size_t m,
                                                             double inv, double cell, u64* __restrict__ qacc, u32* __restrict__ res)
{
    __shared__ u32 hkey[KT_SIMPQ_SLOTS];
    __shared__ u64 hsum[KT_SIMPQ_TERMS][KT_SIMPQ_SLOTS];
    for (int s = threadIdx.x; s < KT_SIMPQ_SLOTS; s += KT_SIMPQ_LANES) {
        hkey[s] = KT_SIMPQ_FREE;
#pragma unroll
        for (int k = 0; k < KT_SIMPQ_TERMS; ++k) hsum[k][s] = 0ull;
    }
    __syncthreads();
    const size_t t = (size_t)blockIdx.x * KT_SIMPQ_LANES + threadIdx.x;
    if (t < m) {
        const u32 a0 = tri[3 * t], a1 = tri[3 * t + 1], a2 = tri[3 * t + 2];
        if (a0 >= n || a1 >= n || a2 >= n) atomicOr(res + 2, KT_SIMPQ_BAD_INDEX);
        else if (a0 != a1 && a1 != a2 && a0 != a2) {
            const u32 g0 = tm[3 * t], g1 = tm[3 * t + 1], g2 = tm[3 * t + 2];
            // the smallest index first, orientation kept
            const int r = (a1 < a0 && a1 < a2) ? 1 : (a2 < a0 && a2 < a1) ? 2 : 0;
            const u32 i0 = r == 0 ? a0 : r == 1 ? a1 : a2, i1 = r == 0 ? a1 : r == 1 ? a2 : a0, i2 = r == 0 ? a2 : r == 1 ? a0 : a1;
            const u32 cl[3] = {r == 0 ? g0 : r == 1 ? g1 : g2, r == 0 ? g1 : r == 1 ? g2 : g0, r == 0 ? g2 : r == 1 ? g0 : g1};
            const uint4 p[3] = {v[i0], v[i1], v[i2]};
            const double o[3] = {simpq_coord(p[0], 0), simpq_coord(p[0], 1), simpq_coord(p[0], 2)};
            const double e1[3] = {simpq_coord(p[1], 0) - o[0], simpq_coord(p[1], 1) - o[1], simpq_coord(p[1], 2) - o[2]};
            const double e2[3] = {simpq_coord(p[2], 0) - o[0], simpq_coord(p[2], 1) - o[1], simpq_coord(p[2], 2) - o[2]};
            const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            if (c[0] != 0.0 || c[1] != 0.0 || c[2] != 0.0) {
                const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
                const double nh[3] = {c[0] / len, c[1] / len, c[2] / len};
                double term[KT_SIMPQ_TERMS] = {c[0] * nh[0], c[0] * nh[1], c[0] * nh[2], c[1] * nh[1], c[1] * nh[2], c[2] * nh[2], 0.0, 0.0, 0.0};
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    if ((e == 1 && cl[1] == cl[0]) || (e == 2 && (cl[2] == cl[0] || cl[2] == cl[1]))) continue;   // once per cluster
                    double d = 0.0;
                    {
                        double rr[3];
#pragma unroll
                        for (int a = 0; a < 3; ++a) rr[a] = o[a] - (floor(simpq_coord(p[e], a) * inv) + 0.5) * cell;
                        d = (nh[0] * rr[0] + nh[1] * rr[1]) + nh[2] * rr[2];
                    }
                    term[6] = c[0] * d; term[7] = c[1] * d; term[8] = c[2] * d;
                    bool fits = true;
#pragma unroll
                    for (int k = 0; k < KT_SIMPQ_TERMS; ++k) fits = fits && fabs(term[k]) < 1.0;   // (false for a NaN)
                    if (!fits) { atomicOr(res + 2, KT_SIMPQ_TOO_LARGE); continue; }
                    u32 h = (cl[e] ^ (cl[e] >> KT_SIMPQ_SLOT_BITS)) & (KT_SIMPQ_SLOTS - 1);
                    for (int probe = 0; probe < KT_SIMPQ_SLOTS; ++probe) {   // (ends at a free slot or the cluster's own: at most 384 references, 512 slots)
                        const u32 old = atomicCAS(&hkey[h], KT_SIMPQ_FREE, cl[e]);
                        if (old == KT_SIMPQ_FREE || old == cl[e]) break;
                        h = (h + 1) & (KT_SIMPQ_SLOTS - 1);
                    }
#pragma unroll
                    for (int k = 0; k < KT_SIMPQ_TERMS; ++k) {
                        const long long q = (long long)rint(term[k] * 4294967296.0);
                        if (q != 0) atomicAdd(&hsum[k][h], (u64)q);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < KT_SIMPQ_SLOTS; s += KT_SIMPQ_LANES) {
        const u32 key = hkey[s];
        if (key == KT_SIMPQ_FREE) continue;
#pragma unroll
        for (int k = 0; k < KT_SIMPQ_TERMS; ++k)
            if (hsum[k][s] != 0ull) atomicAdd(qacc + simpq_word(key, k, n), hsum[k][s]);
    }
}

// simp_finish, and behind the mean the regularised minimiser; res: {n_out, m_out, status, n_placed}
__global__ __launch_bounds__(KT_SIMP_LANES) void simp_qfinish(const uint4* __restrict__ v, const u32* __restrict__ headof, const u64* __restrict__ acc,
                                                              const u64* __restrict__ qacc, u32* __restrict__ res, const u64* __restrict__ sk, u32 n, u64 vcap, u64 tcap,
                                                              double inv, double cell, double bias, uint4* __restrict__ vout)
{
    if (!simp_writes(res, sk, n, vcap, tcap) || res[2] != 0) return;   // uniform
    const size_t total = res[0], stride = (size_t)gridDim.x * KT_SIMP_LANES;
    u32 placed = 0;
    for (size_t c = (size_t)blockIdx.x * KT_SIMP_LANES + threadIdx.x; c < total; c += stride) {
        const uint4 head = v[headof[c]];
        uint4 p = head;
        const u64* a = acc + c * KT_SIMP_ACC;
        const long long k = (long long)a[7];
        if (k > 1) {
            long long mean[3];
            p = simp_mean(a, k, mean);
            double S[KT_SIMPQ_TERMS], kc[3], o[3], mm[3];
#pragma unroll
            for (int e = 0; e < KT_SIMPQ_TERMS; ++e) S[e] = (double)(long long)qacc[simpq_word((u32)c, e, n)];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                kc[e] = floor(simpq_coord(head, e) * inv);
                o[e] = (kc[e] + 0.5) * cell;
                mm[e] = (double)mean[e] * (1.0 / 1048576.0) - o[e];
            }
            const double t = (S[0] + S[3]) + S[5], lam = bias * t;
            const double M00 = S[0] + lam, M11 = S[3] + lam, M22 = S[5] + lam, M01 = S[1], M02 = S[2], M12 = S[4];
            const double r0 = S[6] + lam * mm[0], r1 = S[7] + lam * mm[1], r2 = S[8] + lam * mm[2];
            const double c00 = M11 * M22 - M12 * M12, c01 = M02 * M12 - M01 * M22, c02 = M01 * M12 - M02 * M11;
            const double c11 = M00 * M22 - M02 * M02, c12 = M01 * M02 - M00 * M12, c22 = M00 * M11 - M01 * M01;
            const double det = (M00 * c00 + M01 * c01) + M02 * c02;
            const double x[3] = {((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det, ((c02 * r0 + c12 * r1) + c22 * r2) / det};
            const float out[3] = {(float)(o[0] + x[0]), (float)(o[1] + x[1]), (float)(o[2] + x[2])};
            bool ok = t > 0.0 && det > 0.0;
#pragma unroll
            for (int e = 0; e < 3; ++e) ok = ok && fabsf(out[e]) < INFINITY && floor((double)out[e] * inv) == kc[e];   // (finite: false for a NaN)
            if (ok) { p.x = __float_as_uint(out[0]); p.y = __float_as_uint(out[1]); p.z = __float_as_uint(out[2]); ++placed; }
        }
        vout[c] = p;
    }
    // one atomic per workgroup: every wave of a large grid adding to the one word was most of this kernel's time
    __shared__ u32 part[KT_SIMP_LANES / 64];
    placed = kt_wave_sum(placed);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = placed;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 sum = 0;
#pragma unroll
        for (int k = 0; k < KT_SIMP_LANES / 64; ++k) sum += part[k];
        if (sum) atomicAdd(res + 3, sum);
    }
}

// QUADRIC: totals[2] is the quadric form's status word, and a set bit writes nothing
template <bool QUADRIC>
__global__ __launch_bounds__(KT_SIMP_LANES) void simp_twrite(const u32* __restrict__ tm, size_t m, u32 n, const u32* __restrict__ tcnt, const u32* __restrict__ totals,
                                                             const u64* __restrict__ sk, u64 vcap, u64 tcap, u32* __restrict__ tout)
{
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)blockIdx.x * (KT_SIMP_LANES / 64) + (threadIdx.x >> 6);
    const size_t base = w * KT_SIMP_PER_WAVE;
    if (base >= m) return;   // wave-uniform
    if (!simp_writes(totals, sk, n, vcap, tcap)) return;
    if (QUADRIC && totals[2] != 0) return;
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
struct simp_quadrics { u64* qacc; };  // device: KT_SIMPQ_TERMS planes of a word per vertex

struct kt_mesh_simplifier : kt_pass_head {   // (kt_mesh_pass.hpp)
    u32* res;                         // device, 4: the output vertices, the surviving triangles; of the quadric form the status bits, the placed clusters
    u64* res_host;                    // pinned, 3 words: the two counts, the last sorted key, the quadric form's status bits and placed clusters
    kt_sorted_keys<true> srt;         // (kt_mesh_keys.hpp) sized by vertices
    kt_group<simp_per_vertex> ws;     // sized by vertices
    kt_group<simp_per_triangle> tc;   // sized by waves of KT_SIMP_PER_WAVE triangles
    kt_group<simp_quadrics> qd;       // sized by vertices; taken on the first quadric call
    kt_span_table sp;
    kt_mesh_staging st;
};

extern "C" int kt_mesh_simplify_destroy(kt_mesh_simplifier* w) { return kt_pass_destroy(w); }

extern "C" int kt_mesh_simplify_create(kt_ctx* c, void* hip_stream, kt_mesh_simplifier** out) { return kt_pass_create(c, hip_stream, out, 4, 3); }

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

int simp_reserve_quadrics(kt_mesh_simplifier* w, size_t n)
{
    return w->qd.grow(w->stream, {n}, [](kt_mem& mem, simp_quadrics& g, const size_t* c) { return mem.device(&g.qacc, KT_SIMPQ_TERMS * c[0]); });
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

// what the quadric form checks on top: the bias, the triangle bound of its sums
int simp_check_quadric(size_t m, float bias, const size_t* n_placed)
{
    KT_ARG(n_placed && m <= KT_SIMPQ_MAX_TRIANGLES);
    KT_ARG(std::isfinite(bias) && bias >= 0x1p-20f && bias <= 1.0f);
    return KT_OK;
}

// both forms on device arrays, after their checks; n_placed: null for the mean form
int simp_run(kt_mesh_simplifier* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m, const size_t* span_first, int n_spans,
             float cell, const float* bias, kt_mesh_vertex* vertices_out_dev, size_t vertex_capacity, uint32_t* triangles_out_dev, size_t triangle_capacity,
             size_t* span_first_out, size_t* n_out, size_t* m_out, size_t* n_placed)
{
    static_assert(sizeof(kt_mesh_vertex) == sizeof(uint4) && sizeof(u64) == sizeof(uint64_t), "vertex and key layout");
    const bool quadric = bias != nullptr;
    const char* who = quadric ? "kt_mesh_simplify_quadric" : "kt_mesh_simplify";
    *n_out = 0; *m_out = 0;
    if (quadric) *n_placed = 0;
    if (n == 0) { kt_mesh_empty_spans(span_first_out, n_spans); return KT_OK; }
    KT_HIP(hipSetDevice(w->ctx->device));
    const size_t twaves = (m + KT_SIMP_PER_WAVE - 1) / KT_SIMP_PER_WAVE;
    KT_TRY(simp_reserve(w, n));
    KT_TRY(simp_reserve_triangles(w, twaves));
    if (quadric) KT_TRY(simp_reserve_quadrics(w, n));
    hipStream_t st = w->stream;
    const size_t S = (size_t)n_spans;
    const u32 n32 = (u32)n;
    const double inv = 1.0 / (double)cell;
    KT_TRY(w->sp.upload(st, span_first, n_spans));
    const u32* df = w->sp.first();
    u32* dfo = w->sp.first_out();
    KT_HIP(hipMemsetAsync(w->res, 0, (quadric ? 4 : 2) * sizeof(u32), st));
    const uint4* v = reinterpret_cast<const uint4*>(vertices_dev);
    const unsigned vblocks = (unsigned)((n + KT_SIMP_LANES - 1) / KT_SIMP_LANES);
    hipLaunchKernelGGL(simp_keys, dim3(vblocks), dim3(KT_SIMP_LANES), 0, st, v, n32, inv, w->ws.key);
    KT_LAUNCH_CHECK();
    KT_TRY(w->srt.sort(st, w->ws.key, n, who));
    hipLaunchKernelGGL((kt_runs_heads_kernel<KT_SIMP_LANES, KT_SIMP_CHUNK, false>), dim3((unsigned)((n + KT_SIMP_CHUNK - 1) / KT_SIMP_CHUNK)), dim3(KT_SIMP_LANES), 0, st,
                       (const u64*)w->srt.sk, (const u32*)w->srt.si, n32, df, (const u64*)nullptr, n_spans, (u64)0, w->ws.hp);
    KT_LAUNCH_CHECK();
    KT_TRY(w->srt.scan_max(st, w->ws.hp, w->ws.hps, n, who));
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
    const unsigned fblocks = std::min<unsigned>(vblocks, KT_SIMP_MAX_BLOCKS);
    if (!quadric) {
        hipLaunchKernelGGL(simp_finish, dim3(fblocks), dim3(KT_SIMP_LANES), 0, st, v, w->ws.headof, w->ws.acc, w->res, w->srt.sk, n32, (u64)vertex_capacity,
                           (u64)triangle_capacity, reinterpret_cast<uint4*>(vertices_out_dev));
        KT_LAUNCH_CHECK();
    } else {
        const unsigned qzblocks = (unsigned)std::min<size_t>((KT_SIMPQ_TERMS * n + KT_SIMP_LANES - 1) / KT_SIMP_LANES, KT_SIMP_MAX_BLOCKS);
        hipLaunchKernelGGL(simp_qzero, dim3(qzblocks), dim3(KT_SIMP_LANES), 0, st, w->qd.qacc, w->res, n32);
        KT_LAUNCH_CHECK();
        if (m > 0) {
            hipLaunchKernelGGL(simp_qsums, dim3((unsigned)((m + KT_SIMPQ_LANES - 1) / KT_SIMPQ_LANES)), dim3(KT_SIMPQ_LANES), 0, st, v, n32, triangles_dev,
                               (const u32*)w->tc.tm, m, inv, (double)cell, w->qd.qacc, w->res);
            KT_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(simp_qfinish, dim3(std::min<unsigned>(vblocks, KT_SIMPQ_FINISH_BLOCKS)), dim3(KT_SIMP_LANES), 0, st, v, w->ws.headof, w->ws.acc, (const u64*)w->qd.qacc, w->res, w->srt.sk, n32,
                           (u64)vertex_capacity, (u64)triangle_capacity, inv, (double)cell, (double)*bias, reinterpret_cast<uint4*>(vertices_out_dev));
        KT_LAUNCH_CHECK();
    }
    if (m > 0) {
        if (quadric)
            hipLaunchKernelGGL(simp_twrite<true>, dim3(tblocks), dim3(KT_SIMP_LANES), 0, st, (const u32*)w->tc.tm, m, n32, w->tc.tcnt, w->res, w->srt.sk,
                               (u64)vertex_capacity, (u64)triangle_capacity, triangles_out_dev);
        else
            hipLaunchKernelGGL(simp_twrite<false>, dim3(tblocks), dim3(KT_SIMP_LANES), 0, st, (const u32*)w->tc.tm, m, n32, w->tc.tcnt, w->res, w->srt.sk,
                               (u64)vertex_capacity, (u64)triangle_capacity, triangles_out_dev);
        KT_LAUNCH_CHECK();
    }
    w->res_host[0] = 0; w->res_host[2] = 0;
    KT_HIP(hipMemcpyAsync(&w->res_host[0], w->res, 2 * sizeof(u32), hipMemcpyDeviceToHost, st));
    KT_HIP(hipMemcpyAsync(&w->res_host[1], w->srt.sk + (n - 1), sizeof(u64), hipMemcpyDeviceToHost, st));
    if (quadric) KT_HIP(hipMemcpyAsync(&w->res_host[2], w->res + 2, 2 * sizeof(u32), hipMemcpyDeviceToHost, st));
    KT_TRY(w->sp.download(st));
    KT_HIP(hipStreamSynchronize(st));
    if (w->res_host[1] >> 63) {
        kt_set_error("%s: a vertex that is not finite, has a coordinate of 8192 m or more, or a cell index outside [-2^19, 2^19); nothing was written", who);
        return KT_ERR_ARG;
    }
    const u32* counts = reinterpret_cast<const u32*>(&w->res_host[0]);
    const u32* qres = reinterpret_cast<const u32*>(&w->res_host[2]);   // {status, placed}
    if (qres[0]) {
        kt_set_error("%s:%s%s; nothing was written", who, qres[0] & KT_SIMPQ_BAD_INDEX ? " a triangle index out of range" : "",
                     qres[0] & KT_SIMPQ_TOO_LARGE ? " a triangle with a quadric term of 1 or more" : "");
        return KT_ERR_ARG;
    }
    *n_out = (size_t)counts[0];
    *m_out = (size_t)counts[1];
    if (*n_out > vertex_capacity || *m_out > triangle_capacity) {
        kt_set_error("%s: %zu vertices and %zu triangles do not fit (capacities %zu and %zu); nothing was written", who, *n_out, *m_out, vertex_capacity,
                     triangle_capacity);
        return KT_ERR_CAPACITY;
    }
    if (quadric) *n_placed = (size_t)qres[1];
    w->sp.get(span_first_out);
    return KT_OK;
}

// both forms on host arrays, after their checks
int simp_run_host(kt_mesh_simplifier* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m, const size_t* span_first, int n_spans, float cell,
                  const float* bias, kt_mesh_vertex* vertices_out, size_t vertex_capacity, uint32_t* triangles_out, size_t triangle_capacity, size_t* span_first_out,
                  size_t* n_out, size_t* m_out, size_t* n_placed)
{
    *n_out = 0; *m_out = 0;
    if (bias) *n_placed = 0;
    if (n == 0) { kt_mesh_empty_spans(span_first_out, n_spans); return KT_OK; }
    KT_HIP(hipSetDevice(w->ctx->device));
    const size_t vcap = std::min(vertex_capacity, n), tcap = std::min(triangle_capacity, m);   // (neither count exceeds its input's)
    KT_TRY(w->st.reserve(w->stream, n, m, vcap, tcap, false));
    return kt_mesh_host_form(w->stream, {{w->st.v, vertices, n * sizeof(kt_mesh_vertex)}, {w->st.t, triangles, 3 * m * sizeof(uint32_t)}}, [&] {
        return simp_run(w, reinterpret_cast<const kt_mesh_vertex*>(w->st.v), n, w->st.t, m, span_first, n_spans, cell, bias, reinterpret_cast<kt_mesh_vertex*>(w->st.vo),
                        vcap, w->st.to, tcap, span_first_out, n_out, m_out, n_placed);
    }, [&](kt_host_copy* down) {
        down[0] = {vertices_out, w->st.vo, *n_out * sizeof(kt_mesh_vertex)};
        down[1] = {triangles_out, w->st.to, 3 * *m_out * sizeof(uint32_t)};
    });
}

}  // namespace

extern "C" int kt_mesh_simplify_device(kt_mesh_simplifier* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m,
                                       const size_t* span_first, int n_spans, float cell, kt_mesh_vertex* vertices_out_dev, size_t vertex_capacity,
                                       uint32_t* triangles_out_dev, size_t triangle_capacity, size_t* span_first_out, size_t* n_out, size_t* m_out)
{
    KT_TRY(simp_check(w, vertices_dev, n, triangles_dev, m, span_first, n_spans, cell, vertices_out_dev, vertex_capacity, triangles_out_dev, triangle_capacity,
                      span_first_out, n_out, m_out));
    return simp_run(w, vertices_dev, n, triangles_dev, m, span_first, n_spans, cell, nullptr, vertices_out_dev, vertex_capacity, triangles_out_dev, triangle_capacity,
                    span_first_out, n_out, m_out, nullptr);
}

extern "C" int kt_mesh_simplify_quadric_device(kt_mesh_simplifier* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m,
                                               const size_t* span_first, int n_spans, float cell, float bias, kt_mesh_vertex* vertices_out_dev, size_t vertex_capacity,
                                               uint32_t* triangles_out_dev, size_t triangle_capacity, size_t* span_first_out, size_t* n_out, size_t* m_out,
                                               size_t* n_placed)
{
    KT_TRY(simp_check(w, vertices_dev, n, triangles_dev, m, span_first, n_spans, cell, vertices_out_dev, vertex_capacity, triangles_out_dev, triangle_capacity,
                      span_first_out, n_out, m_out));
    KT_TRY(simp_check_quadric(m, bias, n_placed));
    return simp_run(w, vertices_dev, n, triangles_dev, m, span_first, n_spans, cell, &bias, vertices_out_dev, vertex_capacity, triangles_out_dev, triangle_capacity,
                    span_first_out, n_out, m_out, n_placed);
}

extern "C" int kt_mesh_simplify(kt_mesh_simplifier* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m, const size_t* span_first,
                                int n_spans, float cell, kt_mesh_vertex* vertices_out, size_t vertex_capacity, uint32_t* triangles_out, size_t triangle_capacity,
                                size_t* span_first_out, size_t* n_out, size_t* m_out)
{
    KT_TRY(simp_check(w, vertices, n, triangles, m, span_first, n_spans, cell, vertices_out, vertex_capacity, triangles_out, triangle_capacity, span_first_out, n_out,
                      m_out));
    return simp_run_host(w, vertices, n, triangles, m, span_first, n_spans, cell, nullptr, vertices_out, vertex_capacity, triangles_out, triangle_capacity, span_first_out,
                         n_out, m_out, nullptr);
}

extern "C" int kt_mesh_simplify_quadric(kt_mesh_simplifier* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m, const size_t* span_first,
                                        int n_spans, float cell, float bias, kt_mesh_vertex* vertices_out, size_t vertex_capacity, uint32_t* triangles_out,
                                        size_t triangle_capacity, size_t* span_first_out, size_t* n_out, size_t* m_out, size_t* n_placed)
{
    KT_TRY(simp_check(w, vertices, n, triangles, m, span_first, n_spans, cell, vertices_out, vertex_capacity, triangles_out, triangle_capacity, span_first_out, n_out,
                      m_out));
    KT_TRY(simp_check_quadric(m, bias, n_placed));
    return simp_run_host(w, vertices, n, triangles, m, span_first, n_spans, cell, &bias, vertices_out, vertex_capacity, triangles_out, triangle_capacity, span_first_out,
                         n_out, m_out, n_placed);
}
