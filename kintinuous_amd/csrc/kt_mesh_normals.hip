// kt_mesh_normals.hip -- vertex normals of the -m mesh from its own triangles (kt_mesh_normals, kt_mesh_normals_device).
//
// The reference's -m meshes a PointXYZRGBNormal cloud (backend/MeshGenerator.cpp:41-201), so its .ply carries a normal per vertex.  Here
// the TSDF is gone when a file is written (a slab's voxels are cleared once it is meshed) and the weld, the clustering and the deformation
// have moved or merged vertices since: the normals that hold for every file are those of the triangles as written.  That is a scatter
// from triangles onto vertices, made reproducible the way the simplification's means are: integer sums.
//
// Semantics (include/kt_abi.h; restated in numpy by kintinuous_amd/mesh_normals_ref.py, which the device equals on every byte):
//   - a triangle with an index >= n fails the call; one with two equal indices adds nothing; the three vertices of any other must be
//     valid (kt_wave.hpp: finite with |coordinate| < 8192);
//   - in double, no contraction: e1 = v1 - v0, e2 = v2 - v0, c = e1 x e2 (two products and one subtraction per component); any
//     |c component| >= 1 fails the call; q = (int64)rint(c * 2^32), added to the three sums of each of the triangle's vertices;
//   - a vertex whose sums are all zero gets (0, 0, 0) and is counted; any other (float)(d / sqrt((dx dx + dy dy) + dz dz)), d = (double)S.
//   |q| <= 2^32 and m <= 2^29, so |S| <= 2^61.
//
// The passes, all on the object's stream:
//   memset   the 3 n sums (three planes of n int64) and the two result words
//   faces    one lane per triangle: three indices, three 16-byte vertex loads, the checks (a failed one ORs its bit into the status
//            word and the lane adds nothing), then the lane's three references go into the workgroup's LDS table -- a slot per vertex
//            found by compare-and-swap, three 64-bit LDS adds, a q of 0 skipped -- and after a barrier every used slot adds its sums
//            to the vertex with up to three 64-bit global integer atomics without a return value.  Marching cubes emits triangles in
//            cell order, so a workgroup's 768 references name about a third as many vertices.  The measured A/B against one global
//            atomic per reference and word is in profiles/mesh_normals.md
//   finish   one lane per vertex: nothing when the status word is set; otherwise converts, normalises, stores 12 bytes, and counts the
//            zero normals with a ballot and one atomic per wave
// then {status, n_zero} go to pinned memory and the host waits once.
#include "kt_mesh_pass.hpp"
#include "kt_wave.hpp"

#define KT_NRM_LANES 256
#define KT_NRM_SLOT_BITS 10
#define KT_NRM_SLOTS (1 << KT_NRM_SLOT_BITS)   // of a workgroup's table: four per lane, more than the three references of a lane's triangle (28 KB of LDS)
#define KT_NRM_FREE 0xffffffffu       // no vertex: n <= 2^29
#define KT_NRM_MAX_VERTICES ((size_t)1 << 29)
#define KT_NRM_MAX_TRIANGLES ((size_t)1 << 29)
#define KT_NRM_BAD_INDEX 1u           // the bits of the status word
#define KT_NRM_BAD_VERTEX 2u
#define KT_NRM_TOO_LARGE 4u

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

// one triangle's indices and term; false when it adds nothing (a failed check ORs its bit into the status word)
__device__ __forceinline__ bool nrm_term(const uint4* __restrict__ v, u32 n, const u32* __restrict__ tri, size_t t, u32 i[3], long long q[3], u32* __restrict__ status)
{
    i[0] = tri[3 * t]; i[1] = tri[3 * t + 1]; i[2] = tri[3 * t + 2];
    if (i[0] >= n || i[1] >= n || i[2] >= n) { atomicOr(status, KT_NRM_BAD_INDEX); return false; }
    if (i[0] == i[1] || i[1] == i[2] || i[0] == i[2]) return false;
    const uint4 p0 = v[i[0]], p1 = v[i[1]], p2 = v[i[2]];
    if (!(kt_mesh_valid(p0) && kt_mesh_valid(p1) && kt_mesh_valid(p2))) { atomicOr(status, KT_NRM_BAD_VERTEX); return false; }
    const double o[3] = {(double)__uint_as_float(p0.x), (double)__uint_as_float(p0.y), (double)__uint_as_float(p0.z)};
    const double e1[3] = {(double)__uint_as_float(p1.x) - o[0], (double)__uint_as_float(p1.y) - o[1], (double)__uint_as_float(p1.z) - o[2]};
    const double e2[3] = {(double)__uint_as_float(p2.x) - o[0], (double)__uint_as_float(p2.y) - o[1], (double)__uint_as_float(p2.z) - o[2]};
    const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    if (!(fabs(c[0]) < 1.0 && fabs(c[1]) < 1.0 && fabs(c[2]) < 1.0)) { atomicOr(status, KT_NRM_TOO_LARGE); return false; }
    q[0] = (long long)rint(c[0] * 4294967296.0); q[1] = (long long)rint(c[1] * 4294967296.0); q[2] = (long long)rint(c[2] * 4294967296.0);
    return (q[0] | q[1] | q[2]) != 0;
}

// the word of vertex i's sum k: three planes of n words, so that neighbouring vertices' atomics and the finish pass's reads are contiguous
__device__ __forceinline__ size_t nrm_word(u32 i, int k, u32 n) { return (size_t)k * n + i; }

// acc: three planes of n words, zero on entry.  The terms of a workgroup's 256 triangles are first added by target in an LDS table (open
// addressing, linear probing; more slots than the workgroup has references, so a probe always ends), then every used slot adds its
// sums to the vertex: the triangles of neighbouring cells share their vertices, and the global atomics are what the pass waits for.
// The slot of a vertex is its index folded to ten bits, so neighbouring vertices sit in neighbouring slots and a wave's global
// atomics fall on runs of contiguous words
__global__ __launch_bounds__(KT_NRM_LANES) void nrm_faces(const uint4* __restrict__ v, u32 n, const u32* __restrict__ tri, size_t m, u64* __restrict__ acc,
                                                          u32* __restrict__ status)
{
    __shared__ u32 hkey[KT_NRM_SLOTS];
    __shared__ u64 hsum[3][KT_NRM_SLOTS];
    for (int s = threadIdx.x; s < KT_NRM_SLOTS; s += KT_NRM_LANES) { hkey[s] = KT_NRM_FREE; hsum[0][s] = hsum[1][s] = hsum[2][s] = 0ull; }
    __syncthreads();
    const size_t t = (size_t)blockIdx.x * KT_NRM_LANES + threadIdx.x;
    u32 i[3] = {0u, 0u, 0u};
    long long q[3] = {0, 0, 0};
    if (t < m && nrm_term(v, n, tri, t, i, q, status)) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            u32 h = (i[e] ^ (i[e] >> KT_NRM_SLOT_BITS)) & (KT_NRM_SLOTS - 1);
            for (int probe = 0; probe < KT_NRM_SLOTS; ++probe) {   // (ends at a free slot or the vertex's own: 768 references, 1024 slots)
                const u32 old = atomicCAS(&hkey[h], KT_NRM_FREE, i[e]);
                if (old == KT_NRM_FREE || old == i[e]) break;
                h = (h + 1) & (KT_NRM_SLOTS - 1);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (q[k] != 0) atomicAdd(&hsum[k][h], (u64)q[k]);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < KT_NRM_SLOTS; s += KT_NRM_LANES) {
        const u32 key = hkey[s];
        if (key == KT_NRM_FREE) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (hsum[k][s] != 0ull) atomicAdd(acc + nrm_word(key, k, n), hsum[k][s]);
    }
}

// res: {status, n_zero}
__global__ __launch_bounds__(KT_NRM_LANES) void nrm_finish(const u64* __restrict__ acc, u32 n, u32* __restrict__ res, float* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const size_t i = (size_t)blockIdx.x * KT_NRM_LANES + threadIdx.x;
    if (i - lane >= n) return;   // wave-uniform
    if (res[0] != 0) return;     // a triangle failed: nothing is written
    bool zero = false;
    if (i < n) {
        const long long S[3] = {(long long)acc[nrm_word((u32)i, 0, n)], (long long)acc[nrm_word((u32)i, 1, n)], (long long)acc[nrm_word((u32)i, 2, n)]};
        float r[3] = {0.0f, 0.0f, 0.0f};
        zero = S[0] == 0 && S[1] == 0 && S[2] == 0;
        if (!zero) {
            const double d[3] = {(double)S[0], (double)S[1], (double)S[2]};
            const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            r[0] = (float)(d[0] / len); r[1] = (float)(d[1] / len); r[2] = (float)(d[2] / len);
        }
        out[3 * i] = r[0]; out[3 * i + 1] = r[1]; out[3 * i + 2] = r[2];
    }
    const u64 b = __ballot(zero);
    if (lane == 0 && b) atomicAdd(res + 1, (u32)__popcll(b));
}

}  // namespace

struct nrm_sums { u64* acc; };        // device, 3 words per vertex
struct nrm_staging { uint4* v; u32* t; float* o; };

struct kt_mesh_normal_pass : kt_pass_head {   // (kt_mesh_pass.hpp)
    u32* res;                         // device, 2: the status bits, the zero normals
    u32* res_host;                    // pinned, 2
    kt_group<nrm_sums> ws;            // the sums, sized by vertices
    kt_group<nrm_staging, 2> st;      // the host form's staging, sized by vertices and triangles
};

extern "C" int kt_mesh_normals_destroy(kt_mesh_normal_pass* w) { return kt_pass_destroy(w); }

extern "C" int kt_mesh_normals_create(kt_ctx* c, void* hip_stream, kt_mesh_normal_pass** out) { return kt_pass_create(c, hip_stream, out, 2, 2); }

namespace {

int nrm_reserve(kt_mesh_normal_pass* w, size_t n)
{
    return w->ws.grow(w->stream, {n}, [](kt_mem& mem, nrm_sums& g, const size_t* c) { return mem.device(&g.acc, 3 * c[0]); });
}

int nrm_reserve_staging(kt_mesh_normal_pass* w, size_t n, size_t m)
{
    return w->st.grow(w->stream, {n, m}, [](kt_mem& mem, nrm_staging& g, const size_t* c) {
        int s = mem.device(&g.v, c[0]);
        if (s == KT_OK) s = mem.device(&g.t, 3 * c[1]);
        if (s == KT_OK) s = mem.device(&g.o, 3 * c[0]);
        return s;
    });
}

// the checks both forms share: KT_ERR_ARG with nothing written, before any allocation or launch
int nrm_check(const kt_mesh_normal_pass* w, const void* vertices, size_t n, const void* triangles, size_t m, const void* normals_out, const size_t* n_zero)
{
    KT_ARG(w && n_zero && n <= KT_NRM_MAX_VERTICES && m <= KT_NRM_MAX_TRIANGLES);
    KT_TRY(kt_mesh_check_inputs(vertices, n, triangles, m));
    KT_ARG(normals_out || n == 0);
    KT_ARG(!kt_overlap(normals_out, n * sizeof(kt_mesh_normal), vertices, n * sizeof(kt_mesh_vertex)));
    KT_ARG(!kt_overlap(normals_out, n * sizeof(kt_mesh_normal), triangles, 3 * m * sizeof(uint32_t)));   // (an overlap, not an equal pointer: m may be 0)
    return KT_OK;
}

}  // namespace

extern "C" int kt_mesh_normals_device(kt_mesh_normal_pass* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m,
                                      kt_mesh_normal* normals_out_dev, size_t* n_zero)
{
    static_assert(sizeof(kt_mesh_vertex) == sizeof(uint4) && sizeof(kt_mesh_normal) == 3 * sizeof(float), "vertex and normal layout");
    KT_TRY(nrm_check(w, vertices_dev, n, triangles_dev, m, normals_out_dev, n_zero));
    *n_zero = 0;
    if (n == 0) return KT_OK;
    KT_HIP(hipSetDevice(w->ctx->device));
    KT_TRY(nrm_reserve(w, n));
    hipStream_t st = w->stream;
    KT_HIP(hipMemsetAsync(w->ws.acc, 0, 3 * n * sizeof(u64), st));
    KT_HIP(hipMemsetAsync(w->res, 0, 2 * sizeof(u32), st));
    if (m > 0) {
        hipLaunchKernelGGL(nrm_faces, dim3((unsigned)((m + KT_NRM_LANES - 1) / KT_NRM_LANES)), dim3(KT_NRM_LANES), 0, st, reinterpret_cast<const uint4*>(vertices_dev),
                           (u32)n, triangles_dev, m, w->ws.acc, w->res);
        KT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(nrm_finish, dim3((unsigned)((n + KT_NRM_LANES - 1) / KT_NRM_LANES)), dim3(KT_NRM_LANES), 0, st, (const u64*)w->ws.acc, (u32)n, w->res,
                       reinterpret_cast<float*>(normals_out_dev));
    KT_LAUNCH_CHECK();
    w->res_host[0] = 0; w->res_host[1] = 0;
    KT_HIP(hipMemcpyAsync(w->res_host, w->res, 2 * sizeof(u32), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    const u32 bad = w->res_host[0];
    if (bad) {
        kt_set_error("kt_mesh_normals:%s%s%s; nothing was written", bad & KT_NRM_BAD_INDEX ? " a triangle index out of range" : "",
                     bad & KT_NRM_BAD_VERTEX ? " a triangle's vertex that is not finite or has a coordinate of 8192 m or more" : "",
                     bad & KT_NRM_TOO_LARGE ? " a triangle whose cross product has a component of 1 m^2 or more" : "");
        return KT_ERR_ARG;
    }
    *n_zero = (size_t)w->res_host[1];
    return KT_OK;
}

extern "C" int kt_mesh_normals(kt_mesh_normal_pass* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m, kt_mesh_normal* normals_out,
                               size_t* n_zero)
{
    KT_TRY(nrm_check(w, vertices, n, triangles, m, normals_out, n_zero));
    *n_zero = 0;
    if (n == 0) return KT_OK;
    KT_HIP(hipSetDevice(w->ctx->device));
    KT_TRY(nrm_reserve_staging(w, n, m));
    return kt_mesh_host_form(w->stream, {{w->st.v, vertices, n * sizeof(kt_mesh_vertex)}, {w->st.t, triangles, 3 * m * sizeof(uint32_t)}}, [&] {
        return kt_mesh_normals_device(w, reinterpret_cast<const kt_mesh_vertex*>(w->st.v), n, w->st.t, m, reinterpret_cast<kt_mesh_normal*>(w->st.o), n_zero);
    }, [&](kt_host_copy* down) { down[0] = {normals_out, w->st.o, n * sizeof(kt_mesh_normal)}; });
}
