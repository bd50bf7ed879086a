// kt_jpeg.hip -- the pixel half of a baseline JPEG decode on the device: dequantisation + 8x8 inverse DCT, chroma upsampling and
// YCbCr -> B G R, for the colour payload of compressed .klg logs.  The entropy half (markers, Huffman, run lengths) is
// serial within a scan and stays on the host: kt::jpeg::parseCoefficients (host/JpegDecoder.h), the only entropy decoder in the tree;
// kt::jpeg::reconstructBGR in the same header is the host statement of what the two kernels below compute, byte for byte.
//
// All arithmetic is 32-bit integer, operation for operation that of libjpeg's jidctint.c (jpeg_idct_islow), jdsample.c
// (h2v1_fancy_upsample, h2v2_fancy_upsample, the replicating upsamplers) and jdcolor.c (build_ycc_rgb_table / ycc_rgb_convert).  Sums
// and products are formed in unsigned arithmetic (two's complement wrap, no undefined overflow): for every stream whose dequantised
// sums fit INT32 -- libjpeg's own domain -- the bytes are those of the host decoder; beyond it every input still has a defined byte.
//
// Both kernels are small next to a launch: a VGA 4:2:0 frame is 7200 blocks and 307200 pixels.  No MFMA, wave64.
#include <string>

#include "kt_common.hpp"
#include "../host/JpegDecoder.h"

namespace {

// ---- kt_jpeg_idct_kernel -----------------------------------------------------------------------------------------------------------
// 8 lanes per 8x8 block, 32 blocks per 256-thread workgroup.  Pass 1: lane c transforms column c (dequantising on the way); the
// workspace goes through LDS; pass 2: lane r transforms row r and stores its 8 samples as two dwords.
// LDS layout: int32 ws[block][row][9] with 72 dwords per block.  ds_write_b32 / ds_read_b32 bank = dword index % 32, conflicts are
// counted within a 32-lane half = 4 blocks x 8 lanes.  Pass 1 writes (for a fixed row) dword 72 b + c: 72 b % 32 = 0, 8, 16, 24 plus
// c = 0..7 -- 32 different banks.  Pass 2 reads (for a fixed column) dword 72 b + 9 r: 9 r % 32 = {0, 9, 18, 27, 4, 13, 22, 31}, and
// that set shifted by 8, 16 and 24 never meets itself -- 32 different banks again.
#define KT_JPEG_IDCT_THREADS 256
#define KT_JPEG_WS_ROW 9
#define KT_JPEG_WS_BLOCK 72

struct IdctArgs {
    int ncomp;
    unsigned int first_block[4];   // global index of each component's first block; [ncomp] = total
    unsigned int plane_offset[3];  // byte offset of the component's sample plane in the workspace
    int blocks_w[3];
    int tq[3];
    unsigned short qt[4][64];
};

typedef unsigned int u32;

__device__ __forceinline__ int descale(u32 x, int n) { return (int)(x + (1u << (n - 1))) >> n; }

// the even / odd part of jpeg_idct_islow shared by both passes: in = 8 dequantised frequencies, out = 8 sums before DESCALE
__device__ __forceinline__ void islow_1d(const int* in, u32* out, int dc_shift)
{
    const u32 F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373,
              F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819,
              F_2_562915447 = 20995, F_3_072711026 = 25172;
    u32 z2 = (u32)in[2], z3 = (u32)in[6];
    u32 z1 = (z2 + z3) * F_0_541196100;
    u32 tmp2 = z1 + z3 * (0u - F_1_847759065);
    u32 tmp3 = z1 + z2 * F_0_765366865;
    u32 tmp0 = ((u32)in[0] + (u32)in[4]) << dc_shift;
    u32 tmp1 = ((u32)in[0] - (u32)in[4]) << dc_shift;
    const u32 tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (u32)in[7]; tmp1 = (u32)in[5]; tmp2 = (u32)in[3]; tmp3 = (u32)in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    u32 z4 = tmp1 + tmp3;
    const u32 z5 = (z3 + z4) * F_1_175875602;
    tmp0 *= F_0_298631336; tmp1 *= F_2_053119869; tmp2 *= F_3_072711026; tmp3 *= F_1_501321110;
    z1 *= 0u - F_0_899976223; z2 *= 0u - F_2_562915447; z3 *= 0u - F_1_961570560; z4 *= 0u - F_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = tmp10 + tmp3; out[7] = tmp10 - tmp3;
    out[1] = tmp11 + tmp2; out[6] = tmp11 - tmp2;
    out[2] = tmp12 + tmp1; out[5] = tmp12 - tmp1;
    out[3] = tmp13 + tmp0; out[4] = tmp13 - tmp0;
}

// sample_range_limit indexed through (x & 1023) (RangeLimit in the host decoder): x in [-512, 511] after the mask, + 128, clamped
__device__ __forceinline__ u32 range_limit(int x)
{
    int s = (((x & 1023) ^ 512) - 512) + 128;
    s = s < 0 ? 0 : (s > 255 ? 255 : s);
    return (u32)s;
}

__global__ __launch_bounds__(KT_JPEG_IDCT_THREADS) void kt_jpeg_idct_kernel(const IdctArgs a, const int16_t* __restrict__ coef, unsigned char* __restrict__ planes)
{
    const int CONST_BITS = 13, PASS1_BITS = 2;
    __shared__ int ws[(KT_JPEG_IDCT_THREADS / 8) * KT_JPEG_WS_BLOCK];
    const u32 lane = threadIdx.x & 7u, lb = threadIdx.x >> 3;
    const u32 total = a.first_block[a.ncomp];
    const u32 blk = blockIdx.x * (KT_JPEG_IDCT_THREADS / 8) + lb;
    const bool live = blk < total;
    int comp = 0;
    if (live) {
        if (a.ncomp > 1 && blk >= a.first_block[1]) comp = 1;
        if (a.ncomp > 2 && blk >= a.first_block[2]) comp = 2;
    }
    int* w = ws + lb * KT_JPEG_WS_BLOCK;
    if (live) {
        // pass 1: column `lane` (the components' coefficient planes follow each other in block order: block b starts at 64 b)
        const int16_t* in = coef + (size_t)blk * 64 + lane;
        const unsigned short* q = a.qt[a.tq[comp]] + lane;
        int c[8];
        bool ac = false;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int v = in[r * 8];
            ac = ac || (r > 0 && v != 0);
            c[r] = (int)((u32)v * (u32)q[r * 8]);
        }
        if (!ac) {
            const int dc = (int)((u32)c[0] << PASS1_BITS);
#pragma unroll
            for (int r = 0; r < 8; ++r) w[r * KT_JPEG_WS_ROW + lane] = dc;
        } else {
            u32 o[8];
            islow_1d(c, o, CONST_BITS);
#pragma unroll
            for (int r = 0; r < 8; ++r) w[r * KT_JPEG_WS_ROW + lane] = descale(o[r], CONST_BITS - PASS1_BITS);
        }
    }
    __syncthreads();
    if (!live) return;
    // pass 2: row `lane`
    int x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = w[lane * KT_JPEG_WS_ROW + k];
    u32 px[8];
    if ((x[1] | x[2] | x[3] | x[4] | x[5] | x[6] | x[7]) == 0) {
        const u32 dc = range_limit(descale((u32)x[0], PASS1_BITS + 3));
#pragma unroll
        for (int k = 0; k < 8; ++k) px[k] = dc;
    } else {
        u32 o[8];
        islow_1d(x, o, CONST_BITS);
#pragma unroll
        for (int k = 0; k < 8; ++k) px[k] = range_limit(descale(o[k], CONST_BITS + PASS1_BITS + 3));
    }
    const u32 local = blk - a.first_block[comp];
    const u32 bw = (u32)a.blocks_w[comp];
    const u32 by = local / bw, bx = local - by * bw;
    const size_t stride = (size_t)bw * 8;
    // the plane starts 16-byte aligned and its stride is a multiple of 8: the 8 samples are one aligned 8-byte store
    uint2 v;
    v.x = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    v.y = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
    *reinterpret_cast<uint2*>(planes + a.plane_offset[comp] + ((size_t)by * 8 + lane) * stride + (size_t)bx * 8) = v;
}

// ---- kt_jpeg_colour_kernel ---------------------------------------------------------------------------------------------------------
// One thread per output pixel, pixels taken in the flat order of the dense output (p = y * W + x), 256 per workgroup: the workgroup's
// 768 output bytes start at a multiple of 4, are staged in LDS and leave as 192 dword stores (the last workgroup of an image whose byte
// count is no multiple of 4 finishes with byte stores).
#define KT_JPEG_COLOUR_THREADS 256

struct ColourArgs {
    int width, height, ncomp, swap_rb;
    unsigned int plane_offset[3];
    int stride[3];            // blocks_w * 8
    int cw[3], ch[3];         // downsampled width / height
    int hr[3], vr[3];         // hmax / h, vmax / v: 1 or 2
};

// one sample of component c at full resolution: jdsample.c.  Every index is clamped into the allocated plane.
__device__ __forceinline__ int upsampled(const ColourArgs& a, const unsigned char* __restrict__ planes, int c, int x, int y)
{
    const unsigned char* p = planes + a.plane_offset[c];
    const int stride = a.stride[c], w = a.cw[c], h = a.ch[c], hr = a.hr[c], vr = a.vr[c];
    if (hr == 1 && vr == 1) return p[(size_t)y * stride + x];   // fullsize_upsample
    int sy = vr == 2 ? y >> 1 : y;
    if (sy > h - 1) sy = h - 1;
    const unsigned char* near = p + (size_t)sy * stride;
    const bool fancy = w > 2;   // jinit_upsampler: the fancy routines need downsampled_width > 2
    if (hr == 2 && fancy) {
        const int col = x >> 1;                          // x <= 2 w - 1
        const int other = (x & 1) ? col + 1 : col - 1;    // the further neighbour: right of an odd output column, left of an even one
        const bool edge = other < 0 || other > w - 1;
        const int oc = edge ? col : other;
        if (vr == 1) {   // h2v1_fancy_upsample: 3/4 nearer + 1/4 further, rounding alternately down / up; the edge columns are copies
            if (edge) return near[col];
            return (near[col] * 3 + near[oc] + ((x & 1) ? 2 : 1)) >> 2;
        }
        // h2v2_fancy_upsample: the upper output row of a pair leans on the input row above, the lower one on the row below; beyond the
        // image the nearest real row is repeated (jdmainct.c context rows)
        int fy = (y & 1) ? sy + 1 : sy - 1;
        if (fy < 0) fy = 0;
        if (fy > h - 1) fy = h - 1;
        const unsigned char* far = p + (size_t)fy * stride;
        const int thiscol = near[col] * 3 + far[col];
        if (edge) return (thiscol * 4 + ((x & 1) ? 7 : 8)) >> 4;
        const int othercol = near[oc] * 3 + far[oc];
        return (thiscol * 3 + othercol + ((x & 1) ? 7 : 8)) >> 4;
    }
    // h2v1_upsample / h2v2_upsample / h1v2: replication
    int sx = hr == 2 ? x >> 1 : x;
    if (sx > stride - 1) sx = stride - 1;
    return near[sx];
}

__device__ __forceinline__ unsigned char clamp255(int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ __launch_bounds__(KT_JPEG_COLOUR_THREADS) void kt_jpeg_colour_kernel(const ColourArgs a, const unsigned char* __restrict__ planes, unsigned char* __restrict__ out)
{
    __shared__ unsigned int stage[KT_JPEG_COLOUR_THREADS * 3 / 4];
    unsigned char* sb = reinterpret_cast<unsigned char*>(stage);
    const size_t npix = (size_t)a.width * a.height;
    const size_t p0 = (size_t)blockIdx.x * KT_JPEG_COLOUR_THREADS;
    const size_t p = p0 + threadIdx.x;
    if (p < npix) {
        const int y = (int)(p / (unsigned)a.width), x = (int)(p - (size_t)y * a.width);
        const int Y = upsampled(a, planes, 0, x, y);
        unsigned char b0, b1, b2;
        if (a.ncomp == 1) b0 = b1 = b2 = (unsigned char)Y;
        else {
            // build_ycc_rgb_table: Cr_r_tab, Cb_b_tab, Cr_g_tab, Cb_g_tab (SCALEBITS 16, ONE_HALF in the Cb_g entry), computed instead of looked up
            const int cb = upsampled(a, planes, 1, x, y) - 128, cr = upsampled(a, planes, 2, x, y) - 128;
            const int r = Y + ((91881 * cr + 32768) >> 16);
            const int g = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
            const int b = Y + ((116130 * cb + 32768) >> 16);
            b0 = clamp255(a.swap_rb ? r : b); b1 = clamp255(g); b2 = clamp255(a.swap_rb ? b : r);
        }
        sb[threadIdx.x * 3 + 0] = b0; sb[threadIdx.x * 3 + 1] = b1; sb[threadIdx.x * 3 + 2] = b2;
    }
    __syncthreads();
    const size_t left = npix - p0;   // > 0: the grid covers no empty workgroup
    const unsigned int bytes = left >= KT_JPEG_COLOUR_THREADS ? KT_JPEG_COLOUR_THREADS * 3u : (unsigned int)left * 3u;
    unsigned char* o = out + p0 * 3;   // p0 * 3 is a multiple of 4
    const unsigned int t = threadIdx.x;
    if (t * 4 + 4 <= bytes) reinterpret_cast<unsigned int*>(o)[t] = stage[t];
    else if (t * 4 < bytes)
        for (unsigned int k = t * 4; k < bytes; ++k) o[k] = sb[k];
}

int check_layout(const kt_jpeg_layout* l)
{
    if (!l || l->width < 1 || l->height < 1 || l->width > 16384 || l->height > 16384 || (l->ncomp != 1 && l->ncomp != 3) || l->hmax < 1 ||
        l->hmax > 2 || l->vmax < 1 || l->vmax > 2) { kt_set_error("kt_jpeg: bad layout (size, components or sampling)"); return KT_ERR_ARG; }
    const int mcux = (l->width + 8 * l->hmax - 1) / (8 * l->hmax), mcuy = (l->height + 8 * l->vmax - 1) / (8 * l->vmax);
    size_t total = 0;
    for (int c = 0; c < l->ncomp; ++c) {
        const bool ok = l->h[c] >= 1 && l->h[c] <= l->hmax && l->v[c] >= 1 && l->v[c] <= l->vmax && l->tq[c] >= 0 && l->tq[c] <= 3 &&
                        l->blocks_w[c] == mcux * l->h[c] && l->blocks_h[c] == mcuy * l->v[c] &&
                        l->comp_width[c] == (l->width * l->h[c] + l->hmax - 1) / l->hmax &&
                        l->comp_height[c] == (l->height * l->v[c] + l->vmax - 1) / l->vmax && l->coef_offset[c] == total;
        if (!ok) { kt_set_error("kt_jpeg: the layout of component %d is inconsistent", c); return KT_ERR_ARG; }
        total += (size_t)l->blocks_w[c] * l->blocks_h[c] * 64;
    }
    if (total != l->n_coef) { kt_set_error("kt_jpeg: the layout's coefficient count is inconsistent"); return KT_ERR_ARG; }
    return KT_OK;
}

}  // namespace

// ---- workspace + entry points ---------------------------------------------------------------------------------------------------
struct kt_jpeg_ws {
    kt_mem mem;
    kt_ctx* ctx;
    hipStream_t stream; bool own_stream;
    hipEvent_t done;            // recorded behind the last enqueued work by kt_jpeg_ws_order; lives as long as the workspace
    size_t cap_coef;            // coefficients (= samples) the planes and the coefficient copy hold
    int16_t* coef;              // device copy of the coefficients of the image in flight
    unsigned char* planes;      // the components' sample planes, one after the other
    kt::jpeg::Coefficients* host;   // kt_jpeg_decode's entropy-stage output (kept: no allocation per image)
};

// the largest coefficient count an image of at most max_width x max_height can have: three components at full resolution, whole 16x16 MCUs
static size_t jpeg_capacity(int max_width, int max_height)
{
    const size_t w = ((size_t)max_width + 15) / 16 * 16, h = ((size_t)max_height + 15) / 16 * 16;
    return 3 * w * h;
}

extern "C" int kt_jpeg_ws_destroy(kt_jpeg_ws* w)
{
    if (!w) return KT_OK;
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    w->mem.release();
    if (w->done) (void)hipEventDestroy(w->done);
    if (w->own_stream && w->stream) (void)hipStreamDestroy(w->stream);
    delete w->host;
    delete w;
    return KT_OK;
}

// stream = the stream the reconstruction runs on (null: one of its own, so that the next image's reconstruction never queues behind a frame)
extern "C" int kt_jpeg_ws_create(kt_ctx* c, int max_width, int max_height, void* hip_stream, kt_jpeg_ws** out)
{
    KT_ARG(c && out && max_width > 0 && max_height > 0 && max_width <= 16384 && max_height <= 16384);
    kt_jpeg_ws* w = new kt_jpeg_ws();   // value-initialised: every pointer starts null
    w->ctx = c; w->cap_coef = jpeg_capacity(max_width, max_height);
    w->host = new kt::jpeg::Coefficients();
    int s = KT_OK;
    if (hip_stream) w->stream = (hipStream_t)hip_stream;
    else { s = kt_check(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking), "hipStreamCreateWithFlags", __FILE__, __LINE__); w->own_stream = s == KT_OK; }
    if (s == KT_OK) s = kt_check(hipEventCreateWithFlags(&w->done, hipEventDisableTiming), "hipEventCreateWithFlags", __FILE__, __LINE__);
    if (s == KT_OK) s = w->mem.device(&w->coef, w->cap_coef);
    if (s == KT_OK) s = w->mem.device(&w->planes, w->cap_coef);
    if (s != KT_OK) { (void)kt_jpeg_ws_destroy(w); return s; }
    *out = w;
    return KT_OK;
}

extern "C" void* kt_jpeg_ws_stream(kt_jpeg_ws* w) { return w ? (void*)w->stream : nullptr; }

extern "C" int kt_jpeg_ws_order(kt_jpeg_ws* w, void* hip_stream)
{
    KT_ARG(w && hip_stream);
    if ((hipStream_t)hip_stream == w->stream) return KT_OK;
    KT_HIP(hipEventRecord(w->done, w->stream));
    KT_HIP(hipStreamWaitEvent((hipStream_t)hip_stream, w->done, 0));
    return KT_OK;
}

extern "C" int kt_host_jpeg_entropy_decode(const uint8_t* data_host, size_t size, int width, int height, kt_jpeg_layout* layout, int16_t* coef_host,
                                           size_t coef_capacity, size_t* n_coef)
{
    KT_ARG(data_host && layout && n_coef && (coef_host || coef_capacity == 0));
    kt::jpeg::Coefficients c;
    std::string err;
    if (!kt::jpeg::parseCoefficients(data_host, size, width, height, c, &err)) { kt_set_error("%s", err.c_str()); return KT_ERR_ARG; }
    *n_coef = c.coef.size();
    if (c.coef.size() > coef_capacity) {
        kt_set_error("kt_host_jpeg_entropy_decode: %zu coefficients, room for %zu", c.coef.size(), coef_capacity);
        return KT_ERR_CAPACITY;
    }
    kt::jpeg::fillLayout(c, layout);
    memcpy(coef_host, c.coef.data(), c.coef.size() * sizeof(int16_t));
    return KT_OK;
}

extern "C" int kt_jpeg_reconstruct(kt_jpeg_ws* w, const kt_jpeg_layout* l, const int16_t* coef, int swap_rb, uint8_t* bgr_dev)
{
    KT_ARG(w && l && coef && bgr_dev && ((uintptr_t)bgr_dev & 3u) == 0);
    KT_TRY(check_layout(l));
    if (l->n_coef > w->cap_coef) { kt_set_error("kt_jpeg_reconstruct: %u coefficients, the workspace holds %zu", l->n_coef, w->cap_coef); return KT_ERR_CAPACITY; }
    IdctArgs ia;
    ColourArgs ca;
    memset(&ia, 0, sizeof(ia));
    memset(&ca, 0, sizeof(ca));
    ia.ncomp = ca.ncomp = l->ncomp;
    ca.width = l->width; ca.height = l->height; ca.swap_rb = swap_rb ? 1 : 0;
    unsigned int blocks = 0;
    for (int c = 0; c < l->ncomp; ++c) {
        ia.first_block[c] = blocks;
        ia.plane_offset[c] = ca.plane_offset[c] = blocks * 64;   // a sample per coefficient, planes in component order (multiples of 64 bytes)
        ia.blocks_w[c] = l->blocks_w[c];
        ia.tq[c] = l->tq[c];
        ca.stride[c] = l->blocks_w[c] * 8;
        ca.cw[c] = l->comp_width[c]; ca.ch[c] = l->comp_height[c];
        ca.hr[c] = l->hmax / l->h[c]; ca.vr[c] = l->vmax / l->v[c];
        blocks += (unsigned int)(l->blocks_w[c] * l->blocks_h[c]);
    }
    ia.first_block[l->ncomp] = blocks;
    memcpy(ia.qt, l->qt, sizeof(ia.qt));
    KT_HIP(hipMemcpyAsync(w->coef, coef, (size_t)l->n_coef * sizeof(int16_t), hipMemcpyDefault, w->stream));
    const unsigned int per = KT_JPEG_IDCT_THREADS / 8;
    hipLaunchKernelGGL(kt_jpeg_idct_kernel, dim3((blocks + per - 1) / per), dim3(KT_JPEG_IDCT_THREADS), 0, w->stream, ia, w->coef, w->planes);
    KT_LAUNCH_CHECK();
    const size_t npix = (size_t)l->width * l->height;
    hipLaunchKernelGGL(kt_jpeg_colour_kernel, dim3((unsigned int)((npix + KT_JPEG_COLOUR_THREADS - 1) / KT_JPEG_COLOUR_THREADS)), dim3(KT_JPEG_COLOUR_THREADS), 0,
                       w->stream, ca, w->planes, bgr_dev);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

extern "C" int kt_jpeg_decode(kt_jpeg_ws* w, const uint8_t* data_host, size_t size, int width, int height, int swap_rb, uint8_t* bgr_dev)
{
    KT_ARG(w && data_host && bgr_dev);
    std::string err;
    if (!kt::jpeg::parseCoefficients(data_host, size, width, height, *w->host, &err)) { kt_set_error("%s", err.c_str()); return KT_ERR_ARG; }
    kt_jpeg_layout l;
    kt::jpeg::fillLayout(*w->host, &l);
    KT_TRY(kt_jpeg_reconstruct(w, &l, w->host->coef.data(), swap_rb, bgr_dev));
    KT_HIP(hipStreamSynchronize(w->stream));   // also: w->host may be overwritten by the next call
    return KT_OK;
}
