// kt_mesh.hip -- marching cubes over the TSDF volume (kt_extract_mesh; the tracker's mesh stage, kt_tracker_enable_mesh_stage).
//
// Not in the reference: its -m switch triangulates the processed cloud on the CPU with PCL's greedy projection
// (backend/MeshGenerator.cpp:37-188).  This is marching cubes of the two volumes the tracker owns, with a case table generated from
// a face rule (kintinuous_amd/mc_table.py -> kt_mc_table.hpp), so two cells sharing a face always join the same edges.
//
// Semantics (include/kt_abi.h; restated in numpy by kintinuous_amd/mesh_ref.py):
//   - a box of CELLS [lo, hi) per axis, 0 <= lo <= hi <= N - 1; its voxels are [lo, hi] (inclusive);
//   - valid voxel: weight != 0 && F != 1.f (kt_extract_kernel's rule); a cell is meshed when its 8 corners are valid; inside: F < 0;
//   - one vertex per crossed edge adjacent to a meshed cell of the box, owned by the edge's lower endpoint and its axis, placed and
//     coloured exactly as kt_extract_kernel places and colours the point of that (voxel, axis) pair;
//   - vertices in (owner z, y, x, axis) order, triangles by cell (z, y, x) and then table order: the output is deterministic.
//
// Three passes of one kernel over the box, one wave per RUN -- 62 voxels of an x-row, with a halo lane on either side -- and one
// scan between them:
//   COUNT  each lane loads the 3 x 3 (y, z) column around its voxel (tsdf word + colour word); the x neighbours come from the next
//          lanes through shuffles, so the 27 voxels around each voxel are in registers; from them the lane derives the case of its own
//          cell, the meshed flags of the 7 cells that share an edge with it, its vertex flags (<= 3) and its triangle count (<= 5).
//          The wave's sums go to cnt[run] as nv | nt << 32.
//   scan   rocprim::inclusive_scan over the runs (runs are in box order, so the scan gives every run its first vertex and triangle).
//   VERTS  the same flags; a wave prefix gives each voxel its first vertex, written with the flags into W (first | flags << 29, 4 B
//          per box voxel), and the vertices are written.
//   TRIS   the same case; a wave prefix gives each cell its first triangle; its vertex indices come from W of the cell's corners.
// With a key buffer (kt_extract_mesh_keyed, kt_tracker_enable_mesh_keys) VERTS also writes each vertex's edge key -- the owner's GLOBAL
// voxel (logical + real wrap) and the axis, z in the high bits -- beside the vertex: the name under which kt_mesh_weld.hip finds the
// vertex a neighbouring slab emitted on the same edge.  Keys of one call come out strictly increasing.
// No atomics: the output does not depend on scheduling.  When the totals exceed either capacity (or 2^29 vertices) VERTS and TRIS
// write nothing; the caller reads the totals.
#include "kt_internal.hpp"
#include "kt_wave.hpp"

#define KT_MC_STORAGE __constant__
#include "kt_mc_table.hpp"

#include <rocprim/device/device_scan.hpp>
#include <algorithm>

#define KT_MESH_RUN 62            // voxels per run; lanes 0 and 63 are halo
#define KT_MESH_FIRST_BITS 29
#define KT_MESH_FIRST_MASK ((1u << KT_MESH_FIRST_BITS) - 1u)
#define KT_MESH_KEY_BIAS (1 << 19)  // global voxel coordinates of a keyed mesh lie in [-2^19, 2^19)

struct kt_mesh_args {
    const int16_t* volume; const uint32_t* color;   // colour word = r | g << 8 | b << 16 | weight << 24
    int N, wx, wy, wz;                              // storage wrap (normalised)
    int rwx, rwy, rwz;                              // real voxel wrap (output offset)
    float cx, cy, cz;                               // cell size
    int lo0, lo1, lo2, hi0, hi1, hi2;               // cells [lo, hi); voxels [lo, hi]
    int nvx, nvy;                                   // voxel box extents in x and y
    int rx;                                         // runs per row
    long long runs;
    uint32_t* W;
    unsigned long long* cnt;
    const unsigned long long* scan;
    float4* v; unsigned long long v_cap;
    uint32_t* tri; unsigned long long t_cap;
    unsigned long long* keys;                       // null, or v_cap entries: the edge key of every vertex (kt_extract_mesh_keyed)
};

enum { KT_MESH_COUNT = 0, KT_MESH_VERTS = 1, KT_MESH_TRIS = 2 };

// bit of voxel (x + dx, y + dy, z + dz) in the 27-bit masks
#define KT_MB(dx, dy, dz) (9 * ((dx) + 1) + ((dy) + 1) + 3 * ((dz) + 1))

// the 8 corners of the cell with origin (x + ox, y + oy, z + oz)
__host__ __device__ constexpr uint32_t kt_mesh_cell_mask(int ox, int oy, int oz)
{
    uint32_t m = 0;
    for (int i = 0; i < 8; ++i) m |= 1u << KT_MB(ox + (i & 1), oy + ((i >> 1) & 1), oz + ((i >> 2) & 1));
    return m;
}

__device__ __forceinline__ size_t kt_mesh_sidx(const kt_mesh_args& a, int x, int y, int z)
{
    const int X = (x + a.wx) % a.N, Y = (y + a.wy) % a.N, Z = (z + a.wz) % a.N;
    return (size_t)X + (size_t)Y * a.N + (size_t)Z * a.N * a.N;
}

__device__ __forceinline__ size_t kt_mesh_widx(const kt_mesh_args& a, int x, int y, int z)
{
    return (size_t)(x - a.lo0) + (size_t)a.nvx * ((size_t)(y - a.lo1) + (size_t)a.nvy * (size_t)(z - a.lo2));
}

template <int MODE>
__global__ __launch_bounds__(256) void kt_mesh_kernel(const kt_mesh_args a)
{
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.runs) return;   // wave-uniform
    unsigned long long first_v = 0, first_t = 0;
    if (MODE != KT_MESH_COUNT) {
        const unsigned long long tot = a.scan[a.runs - 1];
        const unsigned long long tv = tot & 0xffffffffull, tt = tot >> 32;
        if (tv > a.v_cap || tt > a.t_cap || tv > (unsigned long long)KT_MESH_FIRST_MASK + 1ull) return;   // nothing is written
        const unsigned long long prev = r > 0 ? a.scan[r - 1] : 0ull;
        first_v = prev & 0xffffffffull;
        first_t = prev >> 32;
    }
    const int rxi = (int)(r % a.rx);
    const long long row = r / a.rx;
    const int y = a.lo1 + (int)(row % a.nvy);
    const int z = a.lo2 + (int)(row / a.nvy);
    const int x = a.lo0 + rxi * KT_MESH_RUN + lane - 1;
    const bool xin = x >= a.lo0 && x <= a.hi0;
    // this lane's 3 x 3 column: valid / inside bits at (dy + 1) + 3 * (dz + 1); raw words of the voxel and its +y / +z neighbours
    uint32_t Vc = 0, Ic = 0;
    int16_t t000 = 0, t010 = 0, t001 = 0;
    uint32_t c000 = 0, c010 = 0, c001 = 0;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = y + dy, zz = z + dz;
            if (xin && yy >= a.lo1 && yy <= a.hi1 && zz >= a.lo2 && zz <= a.hi2) {
                const size_t s = kt_mesh_sidx(a, x, yy, zz);
                const int16_t tv = a.volume[s];
                const uint32_t cv = a.color[s];
                const int b = (dy + 1) + 3 * (dz + 1);
                // F != 1.f <=> the word is not 32767; F < 0 <=> the word is negative (kt_unpack_tsdf is monotonic, exact at 1)
                Vc |= (uint32_t)((cv >> 24) != 0 && tv != 32767) << b;
                Ic |= (uint32_t)(tv < 0) << b;
                if (dy == 0 && dz == 0) { t000 = tv; c000 = cv; }
                if (dy == 1 && dz == 0) { t010 = tv; c010 = cv; }
                if (dy == 0 && dz == 1) { t001 = tv; c001 = cv; }
            }
        }
    }
    const uint32_t V27 = __shfl_up(Vc, 1, 64) | (Vc << 9) | (__shfl_down(Vc, 1, 64) << 18);
    const uint32_t I27 = __shfl_up(Ic, 1, 64) | (Ic << 9) | (__shfl_down(Ic, 1, 64) << 18);
    const int16_t t100 = (int16_t)__shfl_down((int)t000, 1, 64);
    const uint32_t c100 = (uint32_t)__shfl_down((int)c000, 1, 64);
    const bool core = xin && lane >= 1 && lane <= KT_MESH_RUN;
    // meshed flags of the cells with origin (x + ox, y + oy, z + oz), ox, oy, oz in {-1, 0}
    const bool cx0 = x >= a.lo0 && x < a.hi0, cx1 = x - 1 >= a.lo0 && x - 1 < a.hi0;
    const bool cy0 = y >= a.lo1 && y < a.hi1, cy1 = y - 1 >= a.lo1 && y - 1 < a.hi1;
    const bool cz0 = z >= a.lo2 && z < a.hi2, cz1 = z - 1 >= a.lo2 && z - 1 < a.hi2;
#define KT_MESHED(ox, oy, oz) (((ox) ? cx1 : cx0) && ((oy) ? cy1 : cy0) && ((oz) ? cz1 : cz0) && \
                               (V27 & kt_mesh_cell_mask(-(ox), -(oy), -(oz))) == kt_mesh_cell_mask(-(ox), -(oy), -(oz)))
    const bool m000 = KT_MESHED(0, 0, 0);
    uint32_t cube = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) cube |= ((I27 >> KT_MB(i & 1, (i >> 1) & 1, (i >> 2) & 1)) & 1u) << i;
    const int ntri = (core && m000) ? (int)kt_mc_ntri[cube] : 0;
    if (MODE == KT_MESH_TRIS) {
        const int incl = kt_wave_incl(ntri, lane);
        if (ntri == 0) return;
        unsigned long long o = first_t + (unsigned long long)(incl - ntri);
        for (int k = 0; k < ntri; ++k, ++o) {
            const uint32_t word = kt_mc_tri[cube][k];
            uint32_t idx[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int e = (int)((word >> (4 * j)) & 15u);
                const int axis = e >> 2, q = e & 3;
                const int b = axis == 0 ? 1 : 0, c = axis == 2 ? 1 : 2;   // the two other axes, b < c
                const int base = ((q & 1) << b) | ((q >> 1) << c);
                const uint32_t w = a.W[kt_mesh_widx(a, x + (base & 1), y + ((base >> 1) & 1), z + ((base >> 2) & 1))];
                idx[j] = (w & KT_MESH_FIRST_MASK) + (uint32_t)__popc((w >> KT_MESH_FIRST_BITS) & ((1u << axis) - 1u));
            }
            uint32_t* dst = a.tri + 3 * o;
            dst[0] = idx[0]; dst[1] = idx[1]; dst[2] = idx[2];
        }
        return;
    }
    uint32_t flags = 0;
    if (core) {
        const bool m010 = KT_MESHED(0, 1, 0), m001 = KT_MESHED(0, 0, 1), m011 = KT_MESHED(0, 1, 1);
        const bool m100 = KT_MESHED(1, 0, 0), m110 = KT_MESHED(1, 1, 0), m101 = KT_MESHED(1, 0, 1);
        const uint32_t i0 = (I27 >> KT_MB(0, 0, 0)) & 1u;
        if (i0 != ((I27 >> KT_MB(1, 0, 0)) & 1u) && (m000 || m010 || m001 || m011)) flags |= 1u;   // x edge: cells (x, y - j, z - k)
        if (i0 != ((I27 >> KT_MB(0, 1, 0)) & 1u) && (m000 || m100 || m001 || m101)) flags |= 2u;   // y edge: cells (x - i, y, z - k)
        if (i0 != ((I27 >> KT_MB(0, 0, 1)) & 1u) && (m000 || m100 || m010 || m110)) flags |= 4u;   // z edge: cells (x - i, y - j, z)
    }
#undef KT_MESHED
    const int nv = __popc(flags);
    if (MODE == KT_MESH_COUNT) {
        const int sv = kt_wave_sum(nv), st = kt_wave_sum(ntri);
        if (lane == 0) a.cnt[r] = (unsigned long long)(unsigned)sv | ((unsigned long long)(unsigned)st << 32);
        return;
    }
    // VERTS
    const int incl = kt_wave_incl(nv, lane);
    if (nv == 0) return;
    unsigned long long o = first_v + (unsigned long long)(incl - nv);
    a.W[kt_mesh_widx(a, x, y, z)] = (uint32_t)o | (flags << KT_MESH_FIRST_BITS);
    // kt_extract_kernel's point for (x, y, z, axis), bit for bit
    const float F = kt_unpack_tsdf(t000);
    const float V[3] = {((float)x + 0.5f) * a.cx, ((float)y + 0.5f) * a.cy, ((float)z + 0.5f) * a.cz};
    const float cell[3] = {a.cx, a.cy, a.cz};
    const float rw[3] = {(float)a.rwx * a.cx, (float)a.rwy * a.cy, (float)a.rwz * a.cz};
    const float half[3] = {(a.cx * a.N) / 2, (a.cy * a.N) / 2, (a.cz * a.N) / 2};
    // the key of the owner's global voxel (logical + real wrap), z in the high bits, then y, x and the axis (include/kt_abi.h)
    const unsigned long long key0 = ((unsigned long long)(unsigned)(z + a.rwz + KT_MESH_KEY_BIAS) << 42) | ((unsigned long long)(unsigned)(y + a.rwy + KT_MESH_KEY_BIAS) << 22) |
                                    ((unsigned long long)(unsigned)(x + a.rwx + KT_MESH_KEY_BIAS) << 2);
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
        if (!(flags & (1u << axis))) continue;
        const int16_t tn = axis == 0 ? t100 : (axis == 1 ? t010 : t001);
        const uint32_t cn = axis == 0 ? c100 : (axis == 1 ? c010 : c001);
        const float Fn = kt_unpack_tsdf(tn);
        float p[3] = {V[0], V[1], V[2]};
        const float Vn = V[axis] + cell[axis];
        const float d_inv = 1.f / (fabsf(F) + fabsf(Fn));
        p[axis] = (axis == 2 ? __builtin_fmaf(Vn, fabsf(F), V[axis] * fabsf(Fn)) : __builtin_fmaf(V[axis], fabsf(Fn), Vn * fabsf(F))) * d_inv;
        float4 out;
        out.x = (p[0] + rw[0]) - half[0];
        out.y = (p[1] + rw[1]) - half[1];
        out.z = (p[2] + rw[2]) - half[2];
        // the far voxel's r, g, b and the base voxel's weight (kt_point_xyzrgb's b, g, r, a bytes)
        out.w = __uint_as_float((cn & 0x00ffffffu) | (c000 & 0xff000000u));
        if (a.keys) a.keys[o] = key0 | (unsigned long long)axis;
        a.v[o++] = out;
    }
}

struct kt_mesh_ws {
    kt_mem mem;
    uint32_t* W; size_t w_cap;                        // per box voxel
    unsigned long long* cnt; unsigned long long* scan; size_t r_cap;
    unsigned char* tmp; size_t tmp_bytes;
    unsigned long long* total;                        // device: nv | nt << 32 of the last mesh
};

int kt_mesh_ws_destroy(kt_mesh_ws* w)
{
    if (w) w->mem.release();
    delete w;
    return KT_OK;
}

static size_t kt_mesh_runs(const int lo[3], const int hi[3], size_t* voxels)
{
    for (int k = 0; k < 3; ++k)
        if (hi[k] <= lo[k]) { *voxels = 0; return 0; }
    const size_t nx = (size_t)(hi[0] - lo[0] + 1), ny = (size_t)(hi[1] - lo[1] + 1), nz = (size_t)(hi[2] - lo[2] + 1);
    *voxels = nx * ny * nz;
    return ((nx + KT_MESH_RUN - 1) / KT_MESH_RUN) * ny * nz;
}

static int mesh_ws_alloc(kt_mesh_ws* w)
{
    kt_mem& m = w->mem;
    KT_TRY(m.device(&w->total, 1)); KT_TRY(m.device(&w->W, w->w_cap)); KT_TRY(m.device(&w->cnt, w->r_cap)); KT_TRY(m.device(&w->scan, w->r_cap));
    KT_HIP(rocprim::inclusive_scan(nullptr, w->tmp_bytes, w->cnt, w->scan, w->r_cap, rocprim::plus<unsigned long long>(), (hipStream_t)0));
    return m.device(&w->tmp, w->tmp_bytes);
}

// buffers for boxes of up to `voxels` box voxels and `runs` runs.  Grown as kt_loop.hip's loop_ws_reserve grows its own, except that
// the workspace knows no stream: the device is drained (every stream of the process waits).  Nothing survives a growth, the word
// behind kt_mesh_ws_total included.  *pw is a valid workspace or null on every path: a failure destroys it.
int kt_mesh_ws_reserve(kt_mesh_ws** pw, size_t voxels, size_t runs)
{
    kt_mesh_ws* w = *pw;
    if (w && w->w_cap >= voxels && w->r_cap >= runs) return KT_OK;
    if (w) KT_HIP(hipDeviceSynchronize());
    else *pw = w = new kt_mesh_ws();
    w->mem.release();
    w->w_cap = std::max({w->w_cap, voxels, (size_t)1}); w->r_cap = std::max({w->r_cap, runs, (size_t)1});
    const int s = mesh_ws_alloc(w);
    if (s != KT_OK) { (void)kt_mesh_ws_destroy(w); *pw = nullptr; return s; }
    return KT_OK;
}

int kt_mesh_check(const int lo[3], const int hi[3], int N, size_t* voxels, size_t* runs)
{
    KT_ARG(N >= 2);
    for (int k = 0; k < 3; ++k) KT_ARG(lo[k] >= 0 && lo[k] <= hi[k] && hi[k] <= N - 1);
    *runs = kt_mesh_runs(lo, hi, voxels);
    // totals travel packed as nv | nt << 32: at most 3 vertices per voxel and 5 triangles per cell
    KT_ARG(*voxels * 3 < 0xffffffffull && *voxels * 5 < 0xffffffffull);
    return KT_OK;
}

// the key's 20 bits per axis hold the global voxels (logical + real wrap) of the box's voxels [lo, hi]
static int mesh_key_range(const int lo[3], const int hi[3], const int real_voxel_wrap[3])
{
    for (int k = 0; k < 3; ++k)
        KT_ARG((long long)lo[k] + real_voxel_wrap[k] >= -(long long)KT_MESH_KEY_BIAS && (long long)hi[k] + real_voxel_wrap[k] < (long long)KT_MESH_KEY_BIAS);
    return KT_OK;
}

// enqueue the whole mesh of the box on `st`; w->total receives nv | nt << 32 (stream-ordered).  Vertices and triangles are written
// only when both fit (and nv <= 2^29); v / tri may be device or pinned host memory.  keys: null, or v_cap entries written beside the
// vertices (under the same rule); then every global voxel of the box must lie in [-2^19, 2^19) (KT_ERR_ARG before any work).
int kt_mesh_enqueue(kt_mesh_ws* w, hipStream_t st, const int16_t* volume, const uint8_t* color, const float volume_size[3],
                    const int voxel_wrap[3], const int lo[3], const int hi[3], const int real_voxel_wrap[3], int N,
                    kt_mesh_vertex* v, size_t v_cap, uint32_t* tri, size_t t_cap, unsigned long long* keys)
{
    size_t voxels = 0, runs = 0;
    KT_TRY(kt_mesh_check(lo, hi, N, &voxels, &runs));
    if (keys) KT_TRY(mesh_key_range(lo, hi, real_voxel_wrap));
    KT_ARG(w && voxels <= w->w_cap && runs <= w->r_cap);
    for (int k = 0; k < 3; ++k) KT_ARG(voxel_wrap[k] >= 0);
    if (runs == 0) {
        KT_HIP(hipMemsetAsync(w->total, 0, sizeof(unsigned long long), st));
        return KT_OK;
    }
    kt_mesh_args a;
    a.volume = volume; a.color = (const uint32_t*)color;
    a.N = N;
    a.wx = voxel_wrap[0] % N; a.wy = voxel_wrap[1] % N; a.wz = voxel_wrap[2] % N;
    a.rwx = real_voxel_wrap[0]; a.rwy = real_voxel_wrap[1]; a.rwz = real_voxel_wrap[2];
    a.cx = volume_size[0] / N; a.cy = volume_size[1] / N; a.cz = volume_size[2] / N;   // as kt_extract_cloud_slice_async
    a.lo0 = lo[0]; a.lo1 = lo[1]; a.lo2 = lo[2]; a.hi0 = hi[0]; a.hi1 = hi[1]; a.hi2 = hi[2];
    a.nvx = hi[0] - lo[0] + 1; a.nvy = hi[1] - lo[1] + 1;
    a.rx = (a.nvx + KT_MESH_RUN - 1) / KT_MESH_RUN;
    a.runs = (long long)runs;
    a.W = w->W; a.cnt = w->cnt; a.scan = w->scan;
    a.v = (float4*)v; a.v_cap = v ? (unsigned long long)v_cap : 0ull;
    a.tri = tri; a.t_cap = tri ? (unsigned long long)t_cap : 0ull;
    a.keys = v ? keys : nullptr;
    const long long blocks = ((long long)runs + 3) / 4;
    KT_ARG(blocks < 0x7fffffffll);
    hipLaunchKernelGGL(kt_mesh_kernel<KT_MESH_COUNT>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    KT_LAUNCH_CHECK();
    size_t tb = 0;
    KT_HIP(rocprim::inclusive_scan(nullptr, tb, w->cnt, w->scan, runs, rocprim::plus<unsigned long long>(), st));
    if (tb > w->tmp_bytes) { kt_set_error("kt_mesh: scan workspace too small (%zu > %zu)", tb, w->tmp_bytes); return KT_ERR_STATE; }
    KT_HIP(rocprim::inclusive_scan(w->tmp, tb, w->cnt, w->scan, runs, rocprim::plus<unsigned long long>(), st));
    KT_HIP(hipMemcpyAsync(w->total, w->scan + (runs - 1), sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
    if (v_cap == 0 && t_cap == 0) return KT_OK;   // (an empty mesh still fits: the kernels below would write nothing)
    hipLaunchKernelGGL(kt_mesh_kernel<KT_MESH_VERTS>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kt_mesh_kernel<KT_MESH_TRIS>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

const unsigned long long* kt_mesh_ws_total(kt_mesh_ws* w) { return w->total; }

static int mesh_extract(kt_ctx* c, const int16_t* volume, const float volume_size[3], const int voxel_wrap[3], const uint8_t* color_volume,
                        const int lo[3], const int hi[3], const int real_voxel_wrap[3], int N, kt_mesh_vertex* vertices, size_t vertex_capacity,
                        uint32_t* triangles, size_t triangle_capacity, bool keyed, uint64_t* keys, size_t* n_vertices, size_t* n_triangles, const char* who)
{
    KT_ARG(c && volume && volume_size && voxel_wrap && color_volume && lo && hi && real_voxel_wrap && n_vertices && n_triangles);
    KT_ARG((vertices || vertex_capacity == 0) && (triangles || triangle_capacity == 0) && (!keyed || keys || vertex_capacity == 0));
    *n_vertices = 0; *n_triangles = 0;
    size_t voxels = 0, runs = 0;
    KT_TRY(kt_mesh_check(lo, hi, N, &voxels, &runs));
    if (keyed) KT_TRY(mesh_key_range(lo, hi, real_voxel_wrap));
    KT_TRY(kt_mesh_ws_reserve(&c->mesh_ws, voxels, runs));
    kt_mesh_ws* w = c->mesh_ws;
    KT_TRY(kt_mesh_enqueue(w, c->stream, volume, color_volume, volume_size, voxel_wrap, lo, hi, real_voxel_wrap, N, vertices,
                           vertex_capacity, triangles, triangle_capacity, reinterpret_cast<unsigned long long*>(keys)));
    unsigned long long* host = (unsigned long long*)c->int_out_host;
    KT_HIP(hipMemcpyAsync(host, w->total, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    KT_HIP(hipStreamSynchronize(c->stream));
    const unsigned long long tot = *host;
    *n_vertices = (size_t)(tot & 0xffffffffull);
    *n_triangles = (size_t)(tot >> 32);
    if (*n_vertices > vertex_capacity || *n_triangles > triangle_capacity || *n_vertices > (size_t)KT_MESH_FIRST_MASK + 1) {
        kt_set_error("%s: %zu vertices / %zu triangles do not fit (capacities %zu / %zu, at most 2^29 vertices); nothing "
                     "was written", who, *n_vertices, *n_triangles, vertex_capacity, triangle_capacity);
        return KT_ERR_CAPACITY;
    }
    return KT_OK;
}

extern "C" int kt_extract_mesh(kt_ctx* c, const int16_t* volume, const float volume_size[3], const int voxel_wrap[3],
                               const uint8_t* color_volume, const int lo[3], const int hi[3], const int real_voxel_wrap[3], int N,
                               kt_mesh_vertex* vertices, size_t vertex_capacity, uint32_t* triangles, size_t triangle_capacity,
                               size_t* n_vertices, size_t* n_triangles)
{
    return mesh_extract(c, volume, volume_size, voxel_wrap, color_volume, lo, hi, real_voxel_wrap, N, vertices, vertex_capacity, triangles,
                        triangle_capacity, false, nullptr, n_vertices, n_triangles, "kt_extract_mesh");
}

extern "C" int kt_extract_mesh_keyed(kt_ctx* c, const int16_t* volume, const float volume_size[3], const int voxel_wrap[3],
                                     const uint8_t* color_volume, const int lo[3], const int hi[3], const int real_voxel_wrap[3], int N,
                                     kt_mesh_vertex* vertices, size_t vertex_capacity, uint32_t* triangles, size_t triangle_capacity,
                                     uint64_t* keys, size_t* n_vertices, size_t* n_triangles)
{
    return mesh_extract(c, volume, volume_size, voxel_wrap, color_volume, lo, hi, real_voxel_wrap, N, vertices, vertex_capacity, triangles,
                        triangle_capacity, true, keys, n_vertices, n_triangles, "kt_extract_mesh_keyed");
}
