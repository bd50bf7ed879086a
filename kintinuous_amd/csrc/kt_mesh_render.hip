// kt_mesh_render.hip -- a software rasteriser for the -m mesh (kt_mesh_render, kt_mesh_render_device): index, depth, colour and shaded
// images of a kt_mesh_vertex mesh from a camera pose.
//
// Not in the reference: it shows its mesh in PangoVis through OpenGL (out of scope).  The driver's only views (-ppm) come
// from the ray cast of the TSDF volume, before any post-pass and only of what the volume still holds.
//
// Semantics (include/kt_abi.h; restated in numpy by kintinuous_amd/mesh_render_ref.py, which the device equals on every byte, on every
// call): vertices go to camera space and to a 24.8 fixed-point image position in double, each operation rounded once; a triangle with a
// vertex in front of `near` or beyond the guard band is dropped whole; coverage is decided by int64 edge functions at the pixel centres
// with a top-left style tie rule, so a centre on a shared edge is covered once; the depth is interpolated perspective-correctly and
// quantised to 16.16; a pixel's word is the minimum of zq << 32 | triangle index over its covering triangles.  A minimum of integers
// depends on no order of arrival: no floating-point atomic appears anywhere.
//
// The passes, all on the object's stream:
//   memset    the result words, the pixel words to all ones
//   vertex    one lane per vertex: one 16-byte load, one 16-byte record {int32 X, int32 Y, double iz}; X = KT_REN_HIDDEN marks a vertex
//             that is not visible, Y then tells whether it is valid
//   triangle  grid-stride, at most KT_REN_COUNT_BLOCKS workgroups, a lane per triangle and round: gathers its three records, classifies
//             and orients the triangle, intersects its box with the image.  A box of at most KT_REN_SMALL pixels each way is rasterised
//             by the lane itself: a plain load of the pixel's word and a no-return 64-bit atomicMin only when the new word is smaller
//             (the word only ever falls, so a stale load can cost an extra atomic and can never skip a needed one).  A larger one goes
//             on a list: one atomicAdd per wave and round that has one, lanes ranked by ballot.  The three counts are ballots, added
//             up over a wave's rounds: one atomic per wave each, at the end (with a wave per 64 triangles adding to the same three
//             words the pass took 1.57 ms at 8e6 triangles, like this 0.27 ms: profiles/mesh_render.md).  A bad index and an invalid
//             referenced vertex OR their bits into the status word
//   large     a fixed grid of waves strides over the list, whose length stays on the device: one wave per listed triangle, its lanes
//             over the pixels of the 8 x 8 blocks of its box
//   resolve   one lane per pixel: nothing when the status word is set; otherwise it recomputes the winner's weights and writes the wanted
//             planes; the covered pixels are counted by ballot, one atomic per wave
// then the result words go to pinned memory and the host waits once.
// Loops without a compile-time trip count: the triangle pass advances by the grid's stride > 0 per round; the small path's two run at most
// KT_REN_SMALL times each; the large pass strides over a list of at most m entries by the grid's wave count > 0 and walks
// ceil(w / 8) * ceil(h / 8) <= 2^20 blocks of a box inside the image.
// The workspace: 16 bytes per vertex, 8 per pixel, 4 per triangle; the host form's staging holds the inputs and the four planes.
#include "kt_mesh_pass.hpp"
#include "kt_wave.hpp"

#include <cmath>

#define KT_REN_LANES 256
#define KT_REN_MAX_VERTICES ((size_t)1 << 29)
#define KT_REN_MAX_TRIANGLES ((size_t)1 << 29)
#define KT_REN_MAX_SIDE 8192
#define KT_REN_SMALL 4                // a box of at most this many pixels each way is drawn by the triangle's own lane
#define KT_REN_LARGE_BLOCKS 1024      // workgroups of the large pass: 4096 waves stride over the list
#define KT_REN_COUNT_BLOCKS 2048      // at most, of the grid-stride triangle pass: a wave adds its three counts once, at the end
#define KT_REN_HIDDEN ((int)0x80000000)   // X of a vertex that is not visible (a visible one has |X| <= 2^22)
#define KT_REN_GUARD 4194304.0        // 2^22: |sx 256| and |sy 256| stay below it
#define KT_REN_ZQ_MAX 0xFFFFFFFEull
#define KT_REN_EMPTY (~0ull)
#define KT_REN_RES 8                  // the result words: status, drawn, clipped, degenerate, covered, the list's length
#define KT_REN_DRAWN 1
#define KT_REN_CLIPPED 2
#define KT_REN_DEGENERATE 3
#define KT_REN_COVERED 4
#define KT_REN_LISTED 5
#define KT_REN_BAD_INDEX 1u           // the bits of the status word
#define KT_REN_BAD_VERTEX 2u

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;
typedef unsigned char u8;
typedef long long i64;

// the camera of a call, in double: R camera-to-world row-major, t the centre
struct ren_cam { double R[9], t[3], fx, fy, cx, cy, near; };

// c = R^T (p - t)
__device__ __forceinline__ void ren_to_camera(const uint4 p, const ren_cam& k, double c[3])
{
    const double dx = (double)__uint_as_float(p.x) - k.t[0], dy = (double)__uint_as_float(p.y) - k.t[1], dz = (double)__uint_as_float(p.z) - k.t[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = (k.R[a] * dx + k.R[3 + a] * dy) + k.R[6 + a] * dz;
}

__global__ __launch_bounds__(KT_REN_LANES) void ren_vertex(const uint4* __restrict__ v, u32 n, const ren_cam k, uint4* __restrict__ rec)
{
    const size_t i = (size_t)blockIdx.x * KT_REN_LANES + threadIdx.x;
    if (i >= n) return;
    const uint4 p = v[i];
    const bool valid = kt_mesh_valid(p);   // (kt_wave.hpp)
    uint4 r = {(u32)KT_REN_HIDDEN, valid ? 0u : 1u, 0u, 0u};
    if (valid) {
        double c[3];
        ren_to_camera(p, k, c);
        if (c[2] >= k.near) {
            const double ax = ((c[0] * k.fx) / c[2] + k.cx) * 256.0, ay = ((c[1] * k.fy) / c[2] + k.cy) * 256.0;
            if (fabs(ax) < KT_REN_GUARD && fabs(ay) < KT_REN_GUARD) {
                const u64 iz = (u64)__double_as_longlong(1.0 / c[2]);
                r = {(u32)(int)rint(ax), (u32)(int)rint(ay), (u32)iz, (u32)(iz >> 32)};
            }
        }
    }
    rec[i] = r;
}

// a drawn triangle after the swap: corners, 1 / c_z, twice its area, the box clamped to the image (empty when x1 < x0 or y1 < y0)
struct ren_tri {
    u32 i[3];
    int X[3], Y[3];
    double iz[3];
    i64 A;
    int x0, x1, y0, y1;
};

__device__ __forceinline__ double ren_iz(const uint4 r) { return __longlong_as_double((i64)((u64)r.z | (u64)r.w << 32)); }

// the class of triangle (i0, i1, i2), all below n: 0 with a status bit raised, else KT_REN_DRAWN (T filled), _CLIPPED or _DEGENERATE
__device__ __forceinline__ int ren_setup(u32 i0, u32 i1, u32 i2, const uint4* __restrict__ rec, int cols, int rows, ren_tri& T, u32* __restrict__ res)
{
    const uint4 r0 = rec[i0], r1 = rec[i1], r2 = rec[i2];
    const bool h0 = (int)r0.x == KT_REN_HIDDEN, h1 = (int)r1.x == KT_REN_HIDDEN, h2 = (int)r2.x == KT_REN_HIDDEN;
    if ((h0 && r0.y) || (h1 && r1.y) || (h2 && r2.y)) { atomicOr(res, KT_REN_BAD_VERTEX); return 0; }
    if (i0 == i1 || i1 == i2 || i0 == i2) return KT_REN_DEGENERATE;
    if (h0 || h1 || h2) return KT_REN_CLIPPED;
    const int X0 = (int)r0.x, Y0 = (int)r0.y, X1 = (int)r1.x, Y1 = (int)r1.y, X2 = (int)r2.x, Y2 = (int)r2.y;
    const i64 A = (i64)(X1 - X0) * (i64)(Y2 - Y0) - (i64)(Y1 - Y0) * (i64)(X2 - X0);   // (differences below 2^24: |A| < 2^47)
    if (A == 0) return KT_REN_DEGENERATE;
    const bool swap = A < 0;
    T.i[0] = i0; T.i[1] = swap ? i2 : i1; T.i[2] = swap ? i1 : i2;
    T.X[0] = X0; T.X[1] = swap ? X2 : X1; T.X[2] = swap ? X1 : X2;
    T.Y[0] = Y0; T.Y[1] = swap ? Y2 : Y1; T.Y[2] = swap ? Y1 : Y2;
    T.iz[0] = ren_iz(r0); T.iz[1] = ren_iz(swap ? r2 : r1); T.iz[2] = ren_iz(swap ? r1 : r2);
    T.A = swap ? -A : A;
    const int xl = min(X0, min(X1, X2)), xh = max(X0, max(X1, X2)), yl = min(Y0, min(Y1, Y2)), yh = max(Y0, max(Y1, Y2));
    T.x0 = max((xl + 255) >> 8, 0); T.x1 = min(xh >> 8, cols - 1);   // (arithmetic shifts: ceil and floor of a signed value)
    T.y0 = max((yl + 255) >> 8, 0); T.y1 = min(yh >> 8, rows - 1);
    return KT_REN_DRAWN;
}

// the weight of pixel centre (PX, PY) for the edge a -> b; both factors of each product fit 25 bits
__device__ __forceinline__ i64 ren_edge(int ax, int ay, int bx, int by, int PX, int PY)
{
    return (i64)(bx - ax) * (i64)(PY - ay) - (i64)(by - ay) * (i64)(PX - ax);
}

__device__ __forceinline__ bool ren_takes(i64 w, int ax, int ay, int bx, int by)
{
    return w > 0 || (w == 0 && (by - ay > 0 || (by - ay == 0 && bx - ax < 0)));
}

// whether pixel (px, py) is inside T, and its three weights
__device__ __forceinline__ bool ren_weights(const ren_tri& T, int px, int py, i64 w[3])
{
    const int PX = px << 8, PY = py << 8;
    w[0] = ren_edge(T.X[1], T.Y[1], T.X[2], T.Y[2], PX, PY);
    w[1] = ren_edge(T.X[2], T.Y[2], T.X[0], T.Y[0], PX, PY);
    w[2] = ren_edge(T.X[0], T.Y[0], T.X[1], T.Y[1], PX, PY);
    return ren_takes(w[0], T.X[1], T.Y[1], T.X[2], T.Y[2]) && ren_takes(w[1], T.X[2], T.Y[2], T.X[0], T.Y[0]) && ren_takes(w[2], T.X[0], T.Y[0], T.X[1], T.Y[1]);
}

__device__ __forceinline__ double ren_sum(const ren_tri& T, const i64 w[3]) { return ((double)w[0] * T.iz[0] + (double)w[1] * T.iz[1]) + (double)w[2] * T.iz[2]; }

// pixel (px, py), inside the image: the word of triangle t there, when T covers it
__device__ __forceinline__ void ren_pixel(const ren_tri& T, u32 t, int px, int py, int cols, u64* __restrict__ words)
{
    i64 w[3];
    if (!ren_weights(T, px, py, w)) return;
    const double z = (double)T.A / ren_sum(T, w);
    const u64 zq = min((u64)__double2ll_rn(z * 65536.0), KT_REN_ZQ_MAX);   // (z > 0: the weights are >= 0 and sum to A > 0, every iz > 0)
    const u64 word = zq << 32 | t;
    u64* __restrict__ at = words + ((size_t)py * cols + px);
    if (word < *at) (void)atomicMin(at, word);
}

__global__ __launch_bounds__(KT_REN_LANES) void ren_triangles(const u32* __restrict__ tri, u32 m, u32 n, const uint4* __restrict__ rec, int cols, int rows,
                                                              u64* __restrict__ words, u32* __restrict__ list, u32* __restrict__ res)
{
    const int lane = threadIdx.x & 63;
    const size_t stride = (size_t)gridDim.x * KT_REN_LANES;
    u32 drawn = 0, clipped = 0, degenerate = 0;   // of this wave, over its rounds
    for (size_t base = (size_t)blockIdx.x * KT_REN_LANES + threadIdx.x - lane; base < m; base += stride) {   // wave-uniform; ceil(m / stride) rounds
        const size_t t = base + lane;
        int cls = 0;
        bool large = false;
        if (t < m) {
            const u32 i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
            if (i0 >= n || i1 >= n || i2 >= n) atomicOr(res, KT_REN_BAD_INDEX);
            else {
                ren_tri T;
                cls = ren_setup(i0, i1, i2, rec, cols, rows, T, res);
                if (cls == KT_REN_DRAWN && T.x0 <= T.x1 && T.y0 <= T.y1) {
                    large = T.x1 - T.x0 >= KT_REN_SMALL || T.y1 - T.y0 >= KT_REN_SMALL;
                    if (!large)
                        for (int py = T.y0; py <= T.y1; ++py)          // at most KT_REN_SMALL rows of at most KT_REN_SMALL pixels
                            for (int px = T.x0; px <= T.x1; ++px) ren_pixel(T, (u32)t, px, py, cols, words);
                }
            }
        }
        drawn += (u32)__popcll(__ballot(cls == KT_REN_DRAWN));
        clipped += (u32)__popcll(__ballot(cls == KT_REN_CLIPPED));
        degenerate += (u32)__popcll(__ballot(cls == KT_REN_DEGENERATE));
        const u64 listed = __ballot(large);
        if (listed) {   // wave-uniform
            u32 at = 0;
            if (lane == 0) at = atomicAdd(res + KT_REN_LISTED, (u32)__popcll(listed));
            at = __shfl(at, 0, 64);
            if (large) list[at + kt_wave_rank(listed, lane)] = (u32)t;   // (below m: every listed triangle is one of the m, listed once)
        }
    }
    if (lane == 0) {   // (one add per wave and word, at the end)
        if (drawn) atomicAdd(res + KT_REN_DRAWN, drawn);
        if (clipped) atomicAdd(res + KT_REN_CLIPPED, clipped);
        if (degenerate) atomicAdd(res + KT_REN_DEGENERATE, degenerate);
    }
}

__global__ __launch_bounds__(KT_REN_LANES) void ren_large(const u32* __restrict__ tri, const uint4* __restrict__ rec, int cols, int rows, u64* __restrict__ words,
                                                          const u32* __restrict__ list, u32* __restrict__ res)
{
    const int lane = threadIdx.x & 63;
    const u32 waves = gridDim.x * (KT_REN_LANES / 64), first = blockIdx.x * (KT_REN_LANES / 64) + (threadIdx.x >> 6);
    const u32 count = res[KT_REN_LISTED];
    for (u32 e = first; e < count; e += waves) {   // wave-uniform
        const u32 t = list[e];
        ren_tri T;
        (void)ren_setup(tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2], rec, cols, rows, T, res);   // (drawn: it was listed)
        const int bw = (T.x1 - T.x0 + 8) >> 3, bh = (T.y1 - T.y0 + 8) >> 3;
        for (int by = 0; by < bh; ++by)
            for (int bx = 0; bx < bw; ++bx) {
                const int px = T.x0 + 8 * bx + (lane & 7), py = T.y0 + 8 * by + (lane >> 3);
                if (px <= T.x1 && py <= T.y1) ren_pixel(T, t, px, py, cols, words);
            }
    }
}

__device__ __forceinline__ double ren_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ u8 ren_byte(double x) { return (u8)(int)fmin(fmax(rint(x), 0.0), 255.0); }

__global__ __launch_bounds__(KT_REN_LANES) void ren_resolve(const uint4* __restrict__ v, const u32* __restrict__ tri, const uint4* __restrict__ rec, const ren_cam k,
                                                            int cols, int rows, const u64* __restrict__ words, u32* __restrict__ index, unsigned short* __restrict__ depth,
                                                            u8* __restrict__ color, u8* __restrict__ model, u32* __restrict__ res)
{
    if (res[0] != 0u) return;   // a check failed: nothing is written (the same word for every lane)
    const int lane = threadIdx.x & 63;
    const size_t p = (size_t)blockIdx.x * KT_REN_LANES + threadIdx.x;
    bool covered = false;
    if (p < (size_t)cols * rows) {
        const u64 word = words[p];
        covered = word != KT_REN_EMPTY;
        const u64 zq = word >> 32;
        if (index) index[p] = (u32)word;
        if (depth) depth[p] = covered ? (unsigned short)min((zq * 1000ull + 32768ull) >> 16, 65535ull) : (unsigned short)0;
        if (color || model) {
            u8 rgb[3] = {0, 0, 0}, g = 0;
            if (covered) {
                const u32 t = (u32)word;
                ren_tri T;
                (void)ren_setup(tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2], rec, cols, rows, T, res);   // (drawn: it won a pixel)
                const uint4 p0 = v[T.i[0]], p1 = v[T.i[1]], p2 = v[T.i[2]];
                if (color) {
                    i64 w[3];
                    (void)ren_weights(T, (int)(p % cols), (int)(p / cols), w);
                    const double b0 = (double)w[0] * T.iz[0], b1 = (double)w[1] * T.iz[1], b2 = (double)w[2] * T.iz[2], S = (b0 + b1) + b2;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const int sh = 16 - 8 * ch;
                        rgb[ch] = ren_byte(((b0 * (double)((p0.w >> sh) & 255u) + b1 * (double)((p1.w >> sh) & 255u)) + b2 * (double)((p2.w >> sh) & 255u)) / S);
                    }
                }
                if (model) {
                    double c0[3], c1[3], c2[3];
                    ren_to_camera(p0, k, c0); ren_to_camera(p1, k, c1); ren_to_camera(p2, k, c2);
                    const double a[3] = {c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]}, b[3] = {c2[0] - c0[0], c2[1] - c0[1], c2[2] - c0[2]};
                    const double nrm[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
                    const double nc = ren_dot(nrm, c0), den = ren_dot(nrm, nrm) * ren_dot(c0, c0);
                    const double q = den == 0.0 ? 0.0 : (nc * nc) / den;
                    g = ren_byte(255.0 * (0.2 + 0.8 * q));
                }
            }
            if (color) { color[3 * p] = rgb[0]; color[3 * p + 1] = rgb[1]; color[3 * p + 2] = rgb[2]; }
            if (model) { model[3 * p] = g; model[3 * p + 1] = g; model[3 * p + 2] = g; }
        }
    }
    const u32 c = (u32)__popcll(__ballot(covered));
    if (lane == 0 && c) atomicAdd(res + KT_REN_COVERED, c);
}

}  // namespace

struct ren_records { uint4* rec; };                       // device, one per vertex
struct ren_words { u64* words; };                         // device, one per pixel
struct ren_list { u32* list; };                           // device, one per triangle: the large ones
struct ren_staging { uint4* v; u32 *t, *index; unsigned short* depth; u8 *color, *model; };

struct kt_mesh_render_pass : kt_pass_head {   // (kt_mesh_pass.hpp)
    u32* res;                         // device, KT_REN_RES
    u32* res_host;                    // pinned, KT_REN_RES
    kt_group<ren_records> vs;         // sized by vertices
    kt_group<ren_words> px;           // sized by pixels
    kt_group<ren_list> ls;            // sized by triangles
    kt_group<ren_staging, 3> st;      // the host form's staging, sized by vertices, triangles and pixels
};

extern "C" int kt_mesh_render_destroy(kt_mesh_render_pass* w) { return kt_pass_destroy(w); }

extern "C" int kt_mesh_render_create(kt_ctx* c, void* hip_stream, kt_mesh_render_pass** out) { return kt_pass_create(c, hip_stream, out, KT_REN_RES, KT_REN_RES); }

namespace {

int ren_reserve(kt_mesh_render_pass* w, size_t n, size_t m, size_t pixels)
{
    KT_TRY(w->vs.grow(w->stream, {n}, [](kt_mem& mem, ren_records& g, const size_t* c) { return mem.device(&g.rec, c[0]); }));
    KT_TRY(w->px.grow(w->stream, {pixels}, [](kt_mem& mem, ren_words& g, const size_t* c) { return mem.device(&g.words, c[0]); }));
    return w->ls.grow(w->stream, {m}, [](kt_mem& mem, ren_list& g, const size_t* c) { return mem.device(&g.list, c[0]); });
}

int ren_reserve_staging(kt_mesh_render_pass* w, size_t n, size_t m, size_t pixels)
{
    return w->st.grow(w->stream, {std::max<size_t>(n, 1), std::max<size_t>(m, 1), pixels}, [](kt_mem& mem, ren_staging& g, const size_t* c) {
        int s = mem.device(&g.v, c[0]);
        if (s == KT_OK) s = mem.device(&g.t, 3 * c[1]);
        if (s == KT_OK) s = mem.device(&g.index, c[2]);
        if (s == KT_OK) s = mem.device(&g.depth, c[2]);
        if (s == KT_OK) s = mem.device(&g.color, 3 * c[2]);
        if (s == KT_OK) s = mem.device(&g.model, 3 * c[2]);
        return s;
    });
}

// the checks both forms share: KT_ERR_ARG with nothing written, before any allocation or launch
int ren_check(const kt_mesh_render_pass* w, const void* vertices, size_t n, const void* triangles, size_t m, const kt_intr* intr, int cols, int rows, const float* R,
              const float* t, float near, const void* index, const void* depth, const void* color, const void* model, const kt_mesh_render_stats* stats)
{
    KT_ARG(w && stats && intr && R && t && n <= KT_REN_MAX_VERTICES && m <= KT_REN_MAX_TRIANGLES);
    KT_ARG(cols >= 1 && cols <= KT_REN_MAX_SIDE && rows >= 1 && rows <= KT_REN_MAX_SIDE);
    KT_ARG(std::isfinite(intr->fx) && std::isfinite(intr->fy) && std::isfinite(intr->cx) && std::isfinite(intr->cy) && intr->fx > 0.0f && intr->fy > 0.0f);
    for (int a = 0; a < 9; ++a) KT_ARG(std::isfinite(R[a]));
    for (int a = 0; a < 3; ++a) KT_ARG(std::isfinite(t[a]) && std::fabs(t[a]) < 8192.0f);
    KT_ARG(near >= 0.001f && near < 8192.0f);   // (false for a NaN)
    KT_TRY(kt_mesh_check_inputs(vertices, n, triangles, m));
    const size_t pixels = (size_t)cols * rows;
    const kt_byte_range ins[2] = {{vertices, n * sizeof(kt_mesh_vertex)}, {triangles, 3 * m * sizeof(uint32_t)}};
    const kt_byte_range outs[4] = {{index, pixels * sizeof(uint32_t)}, {depth, pixels * sizeof(uint16_t)}, {color, 3 * pixels}, {model, 3 * pixels}};
    return kt_mesh_check_disjoint(outs, 4, ins, 2);
}

}  // namespace

extern "C" int kt_mesh_render_device(kt_mesh_render_pass* w, const kt_mesh_vertex* vertices_dev, size_t n, const uint32_t* triangles_dev, size_t m, const kt_intr* intr,
                                     int cols, int rows, const float R[9], const float t[3], float near, uint32_t* index_dev, uint16_t* depth_dev, uint8_t* color_dev,
                                     uint8_t* model_dev, kt_mesh_render_stats* stats)
{
    static_assert(sizeof(kt_mesh_vertex) == sizeof(uint4), "vertex layout");
    KT_TRY(ren_check(w, vertices_dev, n, triangles_dev, m, intr, cols, rows, R, t, near, index_dev, depth_dev, color_dev, model_dev, stats));
    KT_HIP(hipSetDevice(w->ctx->device));
    const bool empty = n == 0 || m == 0;
    const size_t pixels = (size_t)cols * rows;
    KT_TRY(ren_reserve(w, empty ? 0 : n, empty ? 0 : m, pixels));
    hipStream_t st = w->stream;
    ren_cam k;
    for (int a = 0; a < 9; ++a) k.R[a] = (double)R[a];
    for (int a = 0; a < 3; ++a) k.t[a] = (double)t[a];
    k.fx = (double)intr->fx; k.fy = (double)intr->fy; k.cx = (double)intr->cx; k.cy = (double)intr->cy; k.near = (double)near;
    const uint4* v = reinterpret_cast<const uint4*>(vertices_dev);
    const unsigned pblocks = (unsigned)((pixels + KT_REN_LANES - 1) / KT_REN_LANES);
    KT_HIP(hipMemsetAsync(w->res, 0, KT_REN_RES * sizeof(u32), st));
    KT_HIP(hipMemsetAsync(w->px.words, 0xFF, pixels * sizeof(u64), st));
    if (!empty) {
        const unsigned vblocks = (unsigned)((n + KT_REN_LANES - 1) / KT_REN_LANES), tblocks = (unsigned)((m + KT_REN_LANES - 1) / KT_REN_LANES);
        hipLaunchKernelGGL(ren_vertex, dim3(vblocks), dim3(KT_REN_LANES), 0, st, v, (u32)n, k, w->vs.rec);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(ren_triangles, dim3(std::min<unsigned>(tblocks, KT_REN_COUNT_BLOCKS)), dim3(KT_REN_LANES), 0, st, triangles_dev, (u32)m, (u32)n, (const uint4*)w->vs.rec, cols, rows, w->px.words, w->ls.list,
                           w->res);
        KT_LAUNCH_CHECK();
        hipLaunchKernelGGL(ren_large, dim3(std::min<unsigned>(tblocks, KT_REN_LARGE_BLOCKS)), dim3(KT_REN_LANES), 0, st, triangles_dev, (const uint4*)w->vs.rec, cols, rows,
                           w->px.words, (const u32*)w->ls.list, w->res);
        KT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ren_resolve, dim3(pblocks), dim3(KT_REN_LANES), 0, st, v, triangles_dev, (const uint4*)w->vs.rec, k, cols, rows, (const u64*)w->px.words, index_dev,
                       depth_dev, color_dev, model_dev, w->res);
    KT_LAUNCH_CHECK();
    for (int a = 0; a < KT_REN_RES; ++a) w->res_host[a] = 0;
    KT_HIP(hipMemcpyAsync(w->res_host, w->res, KT_REN_RES * sizeof(u32), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    const u32* r = w->res_host;
    if (r[0]) {
        kt_set_error("kt_mesh_render:%s%s; nothing was written", r[0] & KT_REN_BAD_INDEX ? " a triangle index out of range" : "",
                     r[0] & KT_REN_BAD_VERTEX ? " a triangle's vertex that is not finite or has a coordinate of 8192 m or more" : "");
        return KT_ERR_ARG;
    }
    stats->drawn_triangles = r[KT_REN_DRAWN]; stats->clipped_triangles = r[KT_REN_CLIPPED]; stats->degenerate_triangles = r[KT_REN_DEGENERATE];
    stats->covered_pixels = r[KT_REN_COVERED];
    return KT_OK;
}

extern "C" int kt_mesh_render(kt_mesh_render_pass* w, const kt_mesh_vertex* vertices, size_t n, const uint32_t* triangles, size_t m, const kt_intr* intr, int cols, int rows,
                              const float R[9], const float t[3], float near, uint32_t* index, uint16_t* depth, uint8_t* color, uint8_t* model, kt_mesh_render_stats* stats)
{
    KT_TRY(ren_check(w, vertices, n, triangles, m, intr, cols, rows, R, t, near, index, depth, color, model, stats));
    KT_HIP(hipSetDevice(w->ctx->device));
    const bool empty = n == 0 || m == 0;
    const size_t pixels = (size_t)cols * rows;
    KT_TRY(ren_reserve_staging(w, n, m, pixels));
    return kt_mesh_host_form(w->stream, {{w->st.v, vertices, empty ? 0 : n * sizeof(kt_mesh_vertex)}, {w->st.t, triangles, empty ? 0 : 3 * m * sizeof(uint32_t)}}, [&] {
        return kt_mesh_render_device(w, reinterpret_cast<const kt_mesh_vertex*>(w->st.v), empty ? 0 : n, w->st.t, empty ? 0 : m, intr, cols, rows, R, t, near,
                                     index ? w->st.index : nullptr, depth ? w->st.depth : nullptr, color ? w->st.color : nullptr, model ? w->st.model : nullptr, stats);
    }, [&](kt_host_copy* down) {
        down[0] = {index, w->st.index, index ? pixels * sizeof(uint32_t) : 0};
        down[1] = {depth, w->st.depth, depth ? pixels * sizeof(uint16_t) : 0};
        down[2] = {color, w->st.color, color ? 3 * pixels : 0};
        down[3] = {model, w->st.model, model ? 3 * pixels : 0};
    });
}
