// kt_volume_shift.hip -- what a shift of the cyclical TSDF volume runs, for gfx950: volume init, the slab clears (a14,
// clearVolume{X,Y,Z}{,Back}{,c}) and the cloud-slice extraction (a15, extractKernelSlice).  Hand-written wave64 HIP.
// Reference: src/frontend/cuda/tsdf_volume.cu, extract.cu (file:line cited per kernel).  Results are bit-identical to the oracle's
// restatement of those files: same operation order, explicit fmaf sites, IEEE div/sqrt.
//
// Volume layout as in kt_volume.hip: tsdf = int16[N^3] (x fastest), colour+weight = uchar4[N^3], storage index = logical index
// rotated by voxel_wrap.
#include "kt_internal.hpp"

#include <stdlib.h>

// ================================================================================================
// init  (initVolume / initColorVolume, tsdf_volume.cu:56-87, 450-479): pack_tsdf(0) == 0, uchar4(0)
// ================================================================================================
extern "C" int kt_init_volume(kt_ctx* c, int16_t* volume, int N)
{
    KT_ARG(c && volume && N > 0);
    KT_HIP(hipMemsetAsync(volume, 0, (size_t)N * N * N * sizeof(int16_t), c->stream));
    return KT_OK;
}
extern "C" int kt_init_color_volume(kt_ctx* c, uint8_t* cv, int N)
{
    KT_ARG(c && cv && N > 0);
    KT_HIP(hipMemsetAsync(cv, 0, (size_t)N * N * N * 4, c->stream));
    return KT_OK;
}

// ================================================================================================
// a14  clearVolume{X,Y,Z}{,Back}{,c}                  tsdf_volume.cu:88-448
// The reference launches one thread per (x,y) [or (x,z)] walking the slab; here every wave clears
// 64 consecutive storage x of one line, 16 bytes per lane where the slab is contiguous in x.
// The set of cleared voxels reproduces the reference's launch geometry (incl. quirk A.15).
// ================================================================================================
struct kt_clear_args {
    void* vol; int elem_size; int N;
    int axis;     // 0 x, 1 y, 2 z
    int start;    // first storage index along the axis
    int count;    // number of planes (walk length), consecutive modulo N
    int xthreads; // X variants: number of x "threads" the reference launched (multiple of 16)
    int xw_log2;  // X variants: a wave covers 2^xw_log2 slab indices of 64 >> xw_log2 consecutive y rows
};

template <typename T>
__global__ __launch_bounds__(256) void kt_clear_kernel(const kt_clear_args a)
{
    const int N = a.N;
    T* vol = (T*)a.vol;
    if (a.axis == 0) {
        // grid: (ceil(count / xw), ceil(N / (4 * rows per wave)), N): x index inside the slab, y, z.  An X slab is a few voxels thin in the
        // fastest dimension: a wave takes xw = 2^xw_log2 >= slab width indices of 64 / xw rows, so that most of its lanes store.
        const int xw = 1 << a.xw_log2, lane = threadIdx.x & 63;
        const int i = blockIdx.x * xw + (lane & (xw - 1));
        const int y = (blockIdx.y * 4 + (threadIdx.x >> 6)) * (64 >> a.xw_log2) + (lane >> a.xw_log2);
        const int z = blockIdx.z;
        if (i >= a.count || i >= a.xthreads || y >= N) return;
        int x = a.start + i; if (x >= N) x -= N;
        vol[(size_t)x + (size_t)y * N + (size_t)z * N * N] = T(0);
    } else {
        // grid: (ceil(N/64), ceil(N/4), count): storage x, the free axis, plane inside the slab
        const int x = blockIdx.x * 64 + (threadIdx.x & 63);
        const int o = blockIdx.y * 4 + (threadIdx.x >> 6);
        const int p = blockIdx.z;
        if (x >= N || o >= N) return;
        int s = a.start + p; if (s >= N) s -= N;
        const size_t idx = a.axis == 1 ? (size_t)x + (size_t)s * N + (size_t)o * N * N
                                        : (size_t)x + (size_t)o * N + (size_t)s * N * N;
        vol[idx] = T(0);
    }
}

static int kt_wrap_base(int currentVoxelWrap, int N)
{
    return currentVoxelWrap > 0 ? currentVoxelWrap % N : N - ((-currentVoxelWrap) % N);
}

extern "C" int kt_clear_volume(kt_ctx* c, void* volume, int elem_size, int N, int axis, int back, int currentVoxelWrap,
                               int deltaVoxelWrap)
{
    KT_ARG(c && volume && (elem_size == 2 || elem_size == 4) && N > 0 && axis >= 0 && axis <= 2);
    kt_clear_args a;
    a.vol = volume; a.elem_size = elem_size; a.N = N; a.axis = axis; a.xthreads = N;
    const int base = kt_wrap_base(currentVoxelWrap, N);
    if (!back) {
        // clearVolumeIn{Y,Z}: walk bottom, bottom+1, ... for numUp+1 planes  (tsdf_volume.cu:240-262, 345-367)
        const int numUp = -(currentVoxelWrap - deltaVoxelWrap);
        a.start = base % N;
        a.count = numUp + 1;
    } else {
        // clearVolumeIn{Y,Z}Back: walk top, top-1, ... for numDown+1 planes   (tsdf_volume.cu:290-317, 395-422)
        const int top = (base + N) % N;
        const int numDown = currentVoxelWrap - deltaVoxelWrap;
        a.count = numDown + 1;
        int bottom = (top - numDown) % N;
        if (bottom < 0) bottom += N;
        a.start = bottom;
    }
    if (a.count <= 0) return KT_OK;
    if (a.count > N) a.count = N;
    if (axis == 0) {
        // clearVolumeX / XBack launch geometry (tsdf_volume.cu:117-237): only ceil(r/16)*16 x-threads exist
        int remainder = (deltaVoxelWrap - currentVoxelWrap) % 16;
        if (remainder != 0) remainder = (deltaVoxelWrap - currentVoxelWrap) + 16 - remainder;
        else remainder = abs(deltaVoxelWrap - currentVoxelWrap);
        int grid_x = (remainder + 15) / 16;
        if (grid_x <= 0) return KT_OK;
        a.xthreads = grid_x * 16;
    }
    dim3 b(256), g;
    a.xw_log2 = 6;
    if (axis == 0) {
        const int w = a.count < a.xthreads ? a.count : a.xthreads;   // indices that are actually written
        a.xw_log2 = 0;
        while ((1 << a.xw_log2) < w && a.xw_log2 < 6) ++a.xw_log2;
        g = dim3(kt_div_up(w, 1 << a.xw_log2), kt_div_up(N, 4 * (64 >> a.xw_log2)), N);
    }
    else g = dim3(kt_div_up(N, 64), kt_div_up(N, 4), a.count);
    if (elem_size == 2) hipLaunchKernelGGL(kt_clear_kernel<int16_t>, g, b, 0, c->stream, a);
    else hipLaunchKernelGGL(kt_clear_kernel<uint32_t>, g, b, 0, c->stream, a);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

// ================================================================================================
// a15  extractCloudSlice -> extractKernelSlice        extract.cu:79-419
// One thread per candidate voxel of the slab (x fastest); wave-level compaction with a 64-lane ballot
// prefix and ONE global atomic per wave (the reference: 32-lane shared-memory scan + atomic per warp
// per z-step).  Output order is unspecified in both.
// ================================================================================================
struct kt_extract_args {
    const int16_t* volume; const uchar4* color;
    kt_point_xyzrgb* out; unsigned int out_cap;
    unsigned int* count;      // device counter
    float cx, cy, cz;         // cell size
    int wx, wy, wz;           // storage wrap (normalised)
    int rwx, rwy, rwz;        // real voxel wrap (for the output offset)
    int minX, maxX, minY, maxY, minZ, maxZ, subsample;
    int nx, ny, nz;           // extents of the scanned box
    int N;
};

__device__ __forceinline__ size_t kt_ex_index(const kt_extract_args& a, int x, int y, int z)
{
    // (x + wrap) % N with z + 1 possibly == N (wraps through the modulo, quirk of extract.cu:190-196)
    int X = (x + a.wx) % a.N, Y = (y + a.wy) % a.N, Z = (z + a.wz) % a.N;
    return (size_t)X + (size_t)Y * a.N + (size_t)Z * a.N * a.N;
}

__global__ __launch_bounds__(256) void kt_extract_kernel(const kt_extract_args a)
{
    const long long total = (long long)a.nx * a.ny * a.nz;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    // (up to three points per thread, one per axis.  Indexed by the AXIS, a compile-time constant in the unrolled loops, never by a
    // running count: a dynamically indexed array lives in scratch memory, and the first launch of a scratch-using kernel on a queue makes
    // the runtime allocate it -- 1 ms in the middle of the first shift frame of a process.)
    float4 pts[3];
    uint32_t cols[3];
    bool found[3] = {false, false, false};
    if (tid < total) {
        const int ix = (int)(tid % a.nx);
        const int iy = (int)((tid / a.nx) % a.ny);
        const int iz = (int)(tid / ((long long)a.nx * a.ny));
        const int x = a.minX + ix, y = a.minY + iy, z = a.minZ + iz * a.subsample;
        const int N = a.N;
        if (x >= 0 && y >= 0 && x < N && y < N && x % a.subsample == 0 && y % a.subsample == 0) {
            const size_t i0 = kt_ex_index(a, x, y, z);
            const int W = a.color[i0].w;
            const float F = kt_unpack_tsdf(a.volume[i0]);
            if (W != 0 && F != 1.f) {
                const float V[3] = {((float)x + 0.5f) * a.cx, ((float)y + 0.5f) * a.cy, ((float)z + 0.5f) * a.cz};
                const float cell[3] = {a.cx, a.cy, a.cz};
#pragma unroll
                for (int axis = 0; axis < 3; ++axis) {
                    const int nx = x + (axis == 0), ny = y + (axis == 1), nz = z + (axis == 2);
                    if (axis == 0 && !(x + 1 < N)) continue;
                    if (axis == 1 && !(y + 1 < N)) continue;
                    const size_t in = kt_ex_index(a, nx, ny, nz);
                    const uchar4 cn = a.color[in];
                    const float Fn = kt_unpack_tsdf(a.volume[in]);
                    if (!(cn.w != 0 && Fn != 1.f)) continue;
                    if (!((F > 0 && Fn < 0) || (F < 0 && Fn > 0))) continue;
                    float p[3] = {V[0], V[1], V[2]};
                    const float Vn = V[axis] + cell[axis];
                    const float d_inv = 1.f / (fabsf(F) + fabsf(Fn));
                    // dz: the other product is the contracted one (LLVM operand order on extract.cu:224, pinned by oracle/_ref)
                    p[axis] = (axis == 2 ? __builtin_fmaf(Vn, fabsf(F), V[axis] * fabsf(Fn)) : __builtin_fmaf(V[axis], fabsf(Fn), Vn * fabsf(F))) * d_inv;
                    pts[axis] = make_float4(p[0], p[1], p[2], 0.f);
                    // colour of the NEIGHBOUR voxel, alpha = weight of the base voxel; the point's byte order is
                    // b,g,r,a with ptr->b = colour.x and ptr->r = colour.z (store_point_type, quirk A.14)
                    cols[axis] = (uint32_t)cn.x | ((uint32_t)cn.y << 8) | ((uint32_t)cn.z << 16) | ((uint32_t)W << 24);
                    found[axis] = true;
                }
            }
        }
    }
    // wave compaction: exclusive prefix of `local` over the 64 lanes
    const int lane = threadIdx.x & 63;
    const int local = (int)found[0] + (int)found[1] + (int)found[2];
    int incl = local;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    const int wave_total = __shfl(incl, 63, 64);
    if (wave_total == 0) return;
    unsigned int base = 0;
    if (lane == 0) base = atomicAdd(a.count, (unsigned int)wave_total);
    base = __shfl(base, 0, 64);
    unsigned int o = base + (unsigned int)(incl - local);   // the thread's points in axis order, as before
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        if (!found[l]) continue;
        if (o < a.out_cap) {
            // store_point_type  extract.cu:307-317
            float4 lo, hi;
            // store_point_type extract.cu:307-317: the product realVoxelWrap * cell_size is loop invariant in the reference and ends up in
            // front of its loops, out of reach of the addition: not contracted (oracle/_ref pins it)
            lo.x = (pts[l].x + (float)a.rwx * a.cx) - ((a.cx * a.N) / 2);
            lo.y = (pts[l].y + (float)a.rwy * a.cy) - ((a.cy * a.N) / 2);
            lo.z = (pts[l].z + (float)a.rwz * a.cz) - ((a.cz * a.N) / 2);
            lo.w = 0.f;
            hi.x = __uint_as_float(cols[l]); hi.y = 0.f; hi.z = 0.f; hi.w = 0.f;
            float4* dst = (float4*)&a.out[o];  // two 16-byte stores per 32-byte point
            dst[0] = lo;
            dst[1] = hi;
        }
        ++o;
    }
}

int kt_extract_cloud_slice_async(kt_ctx* c, const int16_t* volume, const float volume_size[3], kt_point_xyzrgb* output,
                                 size_t output_capacity, const int voxel_wrap[3], const uint8_t* color_volume, int minX, int maxX,
                                 int minY, int maxY, int minZ, int maxZ, int subsample, const int real_voxel_wrap[3], int N,
                                 unsigned int* count_dev)
{
    KT_ARG(c && volume && volume_size && output && voxel_wrap && color_volume && real_voxel_wrap && count_dev);
    KT_ARG(N > 0 && subsample > 0);
    for (int k = 0; k < 3; ++k) KT_ARG(voxel_wrap[k] >= 0);
    KT_HIP(hipMemsetAsync(count_dev, 0, sizeof(unsigned int), c->stream));
    kt_extract_args a;
    a.volume = volume; a.color = (const uchar4*)color_volume;
    a.out = output; a.out_cap = (unsigned int)(output_capacity > 0xffffffffull ? 0xffffffffull : output_capacity);
    a.count = count_dev;
    a.cx = volume_size[0] / N; a.cy = volume_size[1] / N; a.cz = volume_size[2] / N;
    a.wx = voxel_wrap[0] % N; a.wy = voxel_wrap[1] % N; a.wz = voxel_wrap[2] % N;
    a.rwx = real_voxel_wrap[0]; a.rwy = real_voxel_wrap[1]; a.rwz = real_voxel_wrap[2];
    a.minX = minX < 0 ? 0 : minX; a.maxX = maxX > N ? N : maxX;
    a.minY = minY < 0 ? 0 : minY; a.maxY = maxY > N ? N : maxY;
    a.minZ = minZ; a.maxZ = maxZ; a.subsample = subsample;
    a.nx = a.maxX - a.minX; a.ny = a.maxY - a.minY;
    a.nz = (maxZ - minZ + subsample - 1) / subsample;  // for (z = minZ; z < maxZ; z += subsample)
    a.N = N;
    if (a.nx <= 0 || a.ny <= 0 || a.nz <= 0) return KT_OK;
    const long long total = (long long)a.nx * a.ny * a.nz;
    const long long blocks = (total + 255) / 256;
    KT_ARG(blocks < 0x7fffffffll);
    hipLaunchKernelGGL(kt_extract_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, a);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

extern "C" int kt_extract_cloud_slice(kt_ctx* c, const int16_t* volume, const float volume_size[3], kt_point_xyzrgb* output,
                                      size_t output_capacity, const int voxel_wrap[3], const uint8_t* color_volume, int minX,
                                      int maxX, int minY, int maxY, int minZ, int maxZ, int subsample,
                                      const int real_voxel_wrap[3], int N, size_t* count_host)
{
    KT_ARG(count_host);
    int s = kt_extract_cloud_slice_async(c, volume, volume_size, output, output_capacity, voxel_wrap, color_volume, minX, maxX,
                                         minY, maxY, minZ, maxZ, subsample, real_voxel_wrap, N, &c->counters[1]);
    if (s != KT_OK) return s;
    KT_HIP(hipMemcpyAsync(c->int_out_host, &c->counters[1], sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    KT_HIP(hipStreamSynchronize(c->stream));
    size_t n = (size_t)(unsigned int)c->int_out_host[0];
    *count_host = n < output_capacity ? n : output_capacity;  // output_count = min(output.size, global_count)
    return KT_OK;
}
