// kt_debug.hip -- measurement hooks that are not part of the data path (scripts/pmc_calibrate.py, scripts/valu_rates.py).  Since round 6 this
// file is a library of its own, libkt_debug.so (kintinuous_amd/build.py; declarations: csrc/kt_measure.h), linked against libkt_hip.so for the
// context type and the error plumbing: the product library carries no measurement kernels.
//   kt_debug_stream        PMC calibration on contiguous streams at tsdf23's access widths;
//   kt_debug_stream_rows   PMC calibration on tsdf23's REAL access pattern: a wave owns a 32 x 2 wave-column and walks z, so every
//                          access is two 32-lane rows (64 B of tsdf / 128 B of colour each), N^2 elements apart between z-steps;
//   kt_debug_valu_rates    issue cost of the instruction kinds tsdf23 is made of, at 1..8 waves per SIMD (shader cycles per
//                          wave-instruction per SIMD), so that the kernel's instruction roof is a measured number.
// and the test hooks of the negative-brick flags (tests/test_gpu_bricks.py), which launch nothing of their own: they hand a flags buffer and a
// counter buffer to the product library's internal entry points, which the boundary's kt_integrate_tsdf / kt_raycast call without either
//   kt_debug_brick_count / kt_debug_integrate_bricks / kt_debug_raycast_bricks
#include "kt_internal.hpp"
#include "kt_rc_index.hpp"

// One launch reads every element of an N x N x Z array exactly once (halves = 2), or only the columns of the even wave-columns
// (halves = 1: for 2-byte elements that is the LEFT 64 bytes of every 128-byte line -- if the memory side fetched whole lines the
// counters would not halve).  The 4 waves of a workgroup take 4 x-neighbouring wave-columns, like tsdf23's task order.
template <typename T>
__global__ __launch_bounds__(256) void kt_stream_rows_kernel(T* __restrict__ p, int N, int Z, int halves, int rmw, unsigned int* __restrict__ sink)
{
    const int lane = threadIdx.x & 63;
    const int XG = N / 32, YG = N / 2;
    const unsigned int plane = (unsigned int)N * (unsigned int)N;
    unsigned int acc = 0;
    for (int w = blockIdx.x * 4 + (threadIdx.x >> 6); w < XG * YG; w += gridDim.x * 4) {
        const int xg = w % XG, yg = w / XG;
        if (halves == 1 && (xg & 1)) continue;
        const size_t col = (size_t)(yg * 2 + (lane >> 5)) * N + xg * 32 + (lane & 31);
        for (int z = 0; z < Z; z += 4) {
            T v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = p[col + (size_t)(z + u) * plane];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc += (unsigned int)v[u];
                if (rmw) p[col + (size_t)(z + u) * plane] = (T)(v[u] + 1);
            }
        }
    }
    if (acc == 0x12345678u) *sink = acc;  // keeps the loads alive
}

extern "C" int kt_debug_stream_rows(kt_ctx* c, void* buf, int N, int Z, int elem_size, int halves, int rmw)
{
    KT_ARG(c && buf && (elem_size == 2 || elem_size == 4) && N > 0 && N % 32 == 0 && Z > 0 && Z % 4 == 0 && (halves == 1 || halves == 2));
    if (elem_size == 2) hipLaunchKernelGGL(kt_stream_rows_kernel<unsigned short>, dim3(2048), dim3(256), 0, c->stream, (unsigned short*)buf, N, Z, halves, rmw, &c->counters[8]);
    else hipLaunchKernelGGL(kt_stream_rows_kernel<unsigned int>, dim3(2048), dim3(256), 0, c->stream, (unsigned int*)buf, N, Z, halves, rmw, &c->counters[8]);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

// ---- VALU / SALU issue rates ----------------------------------------------------------------------------------------------
// Every wave runs `iters` trips of a loop whose body is 32 instructions of one kind over 8 independent register chains (so the
// chain latency of ~4 cycles is covered from 2 waves per SIMD on) and reports s_memtime ticks (= shader cycles) for the loop.
// kinds: 0 v_fma_f32   1 v_pk_fma_f32   2 v_rcp_f32   3 v_rndne_f32 + v_cvt_i32_f32   4 v_fma_f32 with an s_add_u32 between any two
//        5 v_readlane_b32 (to SGPR) + v_fma_f32 using it   6 v_sqrt_f32   7 v_cndmask_b32 + v_cmp_gt_f32 pairs   8 v_pk_add_f32
//        9 v_mad_u32_u24   10 v_cvt_f32_ubyte0   11 s_add_u32 only (4 independent chains)   12 two v_fma_f32 per s_add_u32
//        13 one v_fma_f32 per two s_add_u32   14 v_cmp_gt_f32 to an SGPR pair + s_and_b64 on it (a predicate step)
//        15 s_and_saveexec_b64 / s_or_b64 exec around one v_fma_f32 (an exec region)
// Round 4: every wave also stamps s_memrealtime (the constant 100 MHz counter) at both ends, so that the shader clock UNDER THIS LOAD
// is a measured number (ticks / real time) instead of the 2.4 GHz of the data sheet.
#define KT_RATE_KINDS 50
template <int KIND>
__global__ __launch_bounds__(256) void kt_valu_rate_kernel(int iters, unsigned long long* __restrict__ ticks, float* __restrict__ sink)
{
    float a0 = threadIdx.x * 1e-3f + 1.0f, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
    float b0 = a0 + 8, b1 = a0 + 9, b2 = a0 + 10, b3 = a0 + 11, b4 = a0 + 12, b5 = a0 + 13, b6 = a0 + 14, b7 = a0 + 15;
    const float m = 0.999f, k = 1e-3f;
    unsigned int s = blockIdx.x;
    unsigned int s1 = s + 1, s2 = s + 2, s3 = s + 3;
    unsigned long long m0 = 0, m1 = 0;
    unsigned long long q0 = threadIdx.x, q1 = q0 + 1, q2 = q0 + 2, q3 = q0 + 3;   // 64-bit chains (v_mad_u64_u32)
    __syncthreads();
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if constexpr (KIND == 0)
                asm volatile("v_fma_f32 %0, %0, %8, %9\n v_fma_f32 %1, %1, %8, %9\n v_fma_f32 %2, %2, %8, %9\n v_fma_f32 %3, %3, %8, %9\n"
                             "v_fma_f32 %4, %4, %8, %9\n v_fma_f32 %5, %5, %8, %9\n v_fma_f32 %6, %6, %8, %9\n v_fma_f32 %7, %7, %8, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k));
            else if constexpr (KIND == 1) {
                typedef float f2 __attribute__((ext_vector_type(2)));
                f2 p0 = {a0, b0}, p1 = {a1, b1}, p2 = {a2, b2}, p3 = {a3, b3}, p4 = {a4, b4}, p5 = {a5, b5}, p6 = {a6, b6}, p7 = {a7, b7};
                const f2 mm = {m, m}, kk = {k, k};
                asm volatile("v_pk_fma_f32 %0, %0, %8, %9\n v_pk_fma_f32 %1, %1, %8, %9\n v_pk_fma_f32 %2, %2, %8, %9\n v_pk_fma_f32 %3, %3, %8, %9\n"
                             "v_pk_fma_f32 %4, %4, %8, %9\n v_pk_fma_f32 %5, %5, %8, %9\n v_pk_fma_f32 %6, %6, %8, %9\n v_pk_fma_f32 %7, %7, %8, %9\n"
                             : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7) : "v"(mm), "v"(kk));
                a0 = p0.x; b0 = p0.y; a1 = p1.x; b1 = p1.y; a2 = p2.x; b2 = p2.y; a3 = p3.x; b3 = p3.y;
                a4 = p4.x; b4 = p4.y; a5 = p5.x; b5 = p5.y; a6 = p6.x; b6 = p6.y; a7 = p7.x; b7 = p7.y;
            } else if constexpr (KIND == 2)
                asm volatile("v_rcp_f32 %0, %0\n v_rcp_f32 %1, %1\n v_rcp_f32 %2, %2\n v_rcp_f32 %3, %3\n"
                             "v_rcp_f32 %4, %4\n v_rcp_f32 %5, %5\n v_rcp_f32 %6, %6\n v_rcp_f32 %7, %7\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));
            else if constexpr (KIND == 3)
                asm volatile("v_rndne_f32 %0, %0\n v_cvt_i32_f32 %1, %1\n v_rndne_f32 %2, %2\n v_cvt_i32_f32 %3, %3\n"
                             "v_rndne_f32 %4, %4\n v_cvt_i32_f32 %5, %5\n v_rndne_f32 %6, %6\n v_cvt_i32_f32 %7, %7\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));
            else if constexpr (KIND == 4)
                asm volatile("v_fma_f32 %0, %0, %9, %10\n s_add_u32 %8, %8, 1\n v_fma_f32 %1, %1, %9, %10\n s_add_u32 %8, %8, 1\n"
                             "v_fma_f32 %2, %2, %9, %10\n s_add_u32 %8, %8, 1\n v_fma_f32 %3, %3, %9, %10\n s_add_u32 %8, %8, 1\n"
                             "v_fma_f32 %4, %4, %9, %10\n s_add_u32 %8, %8, 1\n v_fma_f32 %5, %5, %9, %10\n s_add_u32 %8, %8, 1\n"
                             "v_fma_f32 %6, %6, %9, %10\n s_add_u32 %8, %8, 1\n v_fma_f32 %7, %7, %9, %10\n s_add_u32 %8, %8, 1\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7), "+s"(s) : "v"(m), "v"(k) : "scc");
            else if constexpr (KIND == 5) {
                unsigned int s0, s1, s2, s3;
                asm volatile("v_readlane_b32 %8, %0, 3\n v_readlane_b32 %9, %1, 5\n v_readlane_b32 %10, %2, 7\n v_readlane_b32 %11, %3, 9\n"
                             "s_nop 0\n"
                             "v_fma_f32 %4, %8, %4, %12\n v_fma_f32 %5, %9, %5, %12\n v_fma_f32 %6, %10, %6, %12\n v_fma_f32 %7, %11, %7, %12\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7), "=&s"(s0), "=&s"(s1), "=&s"(s2), "=&s"(s3) : "v"(k));
            } else if constexpr (KIND == 6)
                asm volatile("v_sqrt_f32 %0, %0\n v_sqrt_f32 %1, %1\n v_sqrt_f32 %2, %2\n v_sqrt_f32 %3, %3\n"
                             "v_sqrt_f32 %4, %4\n v_sqrt_f32 %5, %5\n v_sqrt_f32 %6, %6\n v_sqrt_f32 %7, %7\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));
            else if constexpr (KIND == 7)
                asm volatile("v_cmp_gt_f32 vcc, %0, %1\n v_cndmask_b32 %2, %2, %3, vcc\n v_cmp_gt_f32 vcc, %4, %5\n v_cndmask_b32 %6, %6, %7, vcc\n"
                             "v_cmp_gt_f32 vcc, %1, %0\n v_cndmask_b32 %3, %3, %2, vcc\n v_cmp_gt_f32 vcc, %5, %4\n v_cndmask_b32 %7, %7, %6, vcc\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : : "vcc");
            else if constexpr (KIND == 8) {
                typedef float f2 __attribute__((ext_vector_type(2)));
                f2 p0 = {a0, b0}, p1 = {a1, b1}, p2 = {a2, b2}, p3 = {a3, b3}, p4 = {a4, b4}, p5 = {a5, b5}, p6 = {a6, b6}, p7 = {a7, b7};
                const f2 kk = {k, k};
                asm volatile("v_pk_add_f32 %0, %0, %8\n v_pk_add_f32 %1, %1, %8\n v_pk_add_f32 %2, %2, %8\n v_pk_add_f32 %3, %3, %8\n"
                             "v_pk_add_f32 %4, %4, %8\n v_pk_add_f32 %5, %5, %8\n v_pk_add_f32 %6, %6, %8\n v_pk_add_f32 %7, %7, %8\n"
                             : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7) : "v"(kk));
                a0 = p0.x; b0 = p0.y; a1 = p1.x; b1 = p1.y; a2 = p2.x; b2 = p2.y; a3 = p3.x; b3 = p3.y;
                a4 = p4.x; b4 = p4.y; a5 = p5.x; b5 = p5.y; a6 = p6.x; b6 = p6.y; a7 = p7.x; b7 = p7.y;
            } else if constexpr (KIND == 9)
                asm volatile("v_mad_u32_u24 %0, %0, %8, %1\n v_mad_u32_u24 %1, %1, %8, %2\n v_mad_u32_u24 %2, %2, %8, %3\n v_mad_u32_u24 %3, %3, %8, %4\n"
                             "v_mad_u32_u24 %4, %4, %8, %5\n v_mad_u32_u24 %5, %5, %8, %6\n v_mad_u32_u24 %6, %6, %8, %7\n v_mad_u32_u24 %7, %7, %8, %0\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m));
            else if constexpr (KIND == 10)
                asm volatile("v_cvt_f32_ubyte0 %0, %0\n v_cvt_f32_ubyte0 %1, %1\n v_cvt_f32_ubyte0 %2, %2\n v_cvt_f32_ubyte0 %3, %3\n"
                             "v_cvt_f32_ubyte0 %4, %4\n v_cvt_f32_ubyte0 %5, %5\n v_cvt_f32_ubyte0 %6, %6\n v_cvt_f32_ubyte0 %7, %7\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));
            else if constexpr (KIND == 11)
                asm volatile("s_add_u32 %0, %0, 1\n s_add_u32 %1, %1, 1\n s_add_u32 %2, %2, 1\n s_add_u32 %3, %3, 1\n"
                             "s_add_u32 %0, %0, 1\n s_add_u32 %1, %1, 1\n s_add_u32 %2, %2, 1\n s_add_u32 %3, %3, 1\n"
                             : "+s"(s), "+s"(s1), "+s"(s2), "+s"(s3) : : "scc");
            else if constexpr (KIND == 12)   // 8 VALU + 4 SALU
                asm volatile("v_fma_f32 %0, %0, %12, %13\n v_fma_f32 %1, %1, %12, %13\n s_add_u32 %8, %8, 1\n"
                             "v_fma_f32 %2, %2, %12, %13\n v_fma_f32 %3, %3, %12, %13\n s_add_u32 %9, %9, 1\n"
                             "v_fma_f32 %4, %4, %12, %13\n v_fma_f32 %5, %5, %12, %13\n s_add_u32 %10, %10, 1\n"
                             "v_fma_f32 %6, %6, %12, %13\n v_fma_f32 %7, %7, %12, %13\n s_add_u32 %11, %11, 1\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7), "+s"(s), "+s"(s1), "+s"(s2), "+s"(s3)
                             : "v"(m), "v"(k) : "scc");
            else if constexpr (KIND == 13)   // 4 VALU + 8 SALU
                asm volatile("v_fma_f32 %0, %0, %8, %9\n s_add_u32 %4, %4, 1\n s_add_u32 %5, %5, 1\n"
                             "v_fma_f32 %1, %1, %8, %9\n s_add_u32 %6, %6, 1\n s_add_u32 %7, %7, 1\n"
                             "v_fma_f32 %2, %2, %8, %9\n s_add_u32 %4, %4, 1\n s_add_u32 %5, %5, 1\n"
                             "v_fma_f32 %3, %3, %8, %9\n s_add_u32 %6, %6, 1\n s_add_u32 %7, %7, 1\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+s"(s), "+s"(s1), "+s"(s2), "+s"(s3) : "v"(m), "v"(k) : "scc");
            else if constexpr (KIND == 14)   // 4 VALU + 4 SALU: compare into an SGPR pair, fold it into a mask
                asm volatile("v_cmp_gt_f32 vcc, %0, %1\n s_and_b64 %4, %4, vcc\n v_cmp_gt_f32 vcc, %1, %2\n s_or_b64 %5, %5, vcc\n"
                             "v_cmp_gt_f32 vcc, %2, %3\n s_and_b64 %4, %4, vcc\n v_cmp_gt_f32 vcc, %3, %0\n s_or_b64 %5, %5, vcc\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+s"(m0), "+s"(m1) : : "vcc", "scc");
            else if constexpr (KIND == 16)   // v_add_f32
                asm volatile("v_add_f32 %0, %0, %9\n v_add_f32 %1, %1, %9\n v_add_f32 %2, %2, %9\n v_add_f32 %3, %3, %9\n"
                             "v_add_f32 %4, %4, %9\n v_add_f32 %5, %5, %9\n v_add_f32 %6, %6, %9\n v_add_f32 %7, %7, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 17)   // v_mul_f32
                asm volatile("v_mul_f32 %0, %0, %8\n v_mul_f32 %1, %1, %8\n v_mul_f32 %2, %2, %8\n v_mul_f32 %3, %3, %8\n"
                             "v_mul_f32 %4, %4, %8\n v_mul_f32 %5, %5, %8\n v_mul_f32 %6, %6, %8\n v_mul_f32 %7, %7, %8\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 18)   // v_max_f32
                asm volatile("v_max_f32 %0, %0, %9\n v_max_f32 %1, %1, %9\n v_max_f32 %2, %2, %9\n v_max_f32 %3, %3, %9\n"
                             "v_max_f32 %4, %4, %9\n v_max_f32 %5, %5, %9\n v_max_f32 %6, %6, %9\n v_max_f32 %7, %7, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 19)   // v_add_u32
                asm volatile("v_add_u32 %0, %0, %9\n v_add_u32 %1, %1, %9\n v_add_u32 %2, %2, %9\n v_add_u32 %3, %3, %9\n"
                             "v_add_u32 %4, %4, %9\n v_add_u32 %5, %5, %9\n v_add_u32 %6, %6, %9\n v_add_u32 %7, %7, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 20)   // v_and_b32
                asm volatile("v_and_b32 %0, %0, %8\n v_and_b32 %1, %1, %8\n v_and_b32 %2, %2, %8\n v_and_b32 %3, %3, %8\n"
                             "v_and_b32 %4, %4, %8\n v_and_b32 %5, %5, %8\n v_and_b32 %6, %6, %8\n v_and_b32 %7, %7, %8\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 21)   // v_lshlrev_b32
                asm volatile("v_lshlrev_b32 %0, 1, %0\n v_lshlrev_b32 %1, 1, %1\n v_lshlrev_b32 %2, 1, %2\n v_lshlrev_b32 %3, 1, %3\n"
                             "v_lshlrev_b32 %4, 1, %4\n v_lshlrev_b32 %5, 1, %5\n v_lshlrev_b32 %6, 1, %6\n v_lshlrev_b32 %7, 1, %7\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 22)   // v_mov_b32
                asm volatile("v_mov_b32 %0, %1\n v_mov_b32 %1, %2\n v_mov_b32 %2, %3\n v_mov_b32 %3, %4\n"
                             "v_mov_b32 %4, %5\n v_mov_b32 %5, %6\n v_mov_b32 %6, %7\n v_mov_b32 %7, %0\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 23)   // v_cndmask_b32 (vcc fixed)
                asm volatile("v_cndmask_b32 %0, %0, %9, vcc\n v_cndmask_b32 %1, %1, %9, vcc\n v_cndmask_b32 %2, %2, %9, vcc\n v_cndmask_b32 %3, %3, %9, vcc\n"
                             "v_cndmask_b32 %4, %4, %9, vcc\n v_cndmask_b32 %5, %5, %9, vcc\n v_cndmask_b32 %6, %6, %9, vcc\n v_cndmask_b32 %7, %7, %9, vcc\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 24)   // v_cmp_gt_f32 only
                asm volatile("v_cmp_gt_f32 vcc, %0, %1\n v_cmp_gt_f32 vcc, %1, %2\n v_cmp_gt_f32 vcc, %2, %3\n v_cmp_gt_f32 vcc, %3, %4\n"
                             "v_cmp_gt_f32 vcc, %4, %5\n v_cmp_gt_f32 vcc, %5, %6\n v_cmp_gt_f32 vcc, %6, %7\n v_cmp_gt_f32 vcc, %7, %0\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 25)   // v_cvt_f32_u32
                asm volatile("v_cvt_f32_u32 %0, %0\n v_cvt_f32_u32 %1, %1\n v_cvt_f32_u32 %2, %2\n v_cvt_f32_u32 %3, %3\n"
                             "v_cvt_f32_u32 %4, %4\n v_cvt_f32_u32 %5, %5\n v_cvt_f32_u32 %6, %6\n v_cvt_f32_u32 %7, %7\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 26)   // v_med3_i32
                asm volatile("v_med3_i32 %0, %0, %8, %9\n v_med3_i32 %1, %1, %8, %9\n v_med3_i32 %2, %2, %8, %9\n v_med3_i32 %3, %3, %8, %9\n"
                             "v_med3_i32 %4, %4, %8, %9\n v_med3_i32 %5, %5, %8, %9\n v_med3_i32 %6, %6, %8, %9\n v_med3_i32 %7, %7, %8, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 27)   // v_mul_u32_u24
                asm volatile("v_mul_u32_u24 %0, %0, %9\n v_mul_u32_u24 %1, %1, %9\n v_mul_u32_u24 %2, %2, %9\n v_mul_u32_u24 %3, %3, %9\n"
                             "v_mul_u32_u24 %4, %4, %9\n v_mul_u32_u24 %5, %5, %9\n v_mul_u32_u24 %6, %6, %9\n v_mul_u32_u24 %7, %7, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 28)   // v_lshl_add_u32
                asm volatile("v_lshl_add_u32 %0, %0, 1, %9\n v_lshl_add_u32 %1, %1, 1, %9\n v_lshl_add_u32 %2, %2, 1, %9\n v_lshl_add_u32 %3, %3, 1, %9\n"
                             "v_lshl_add_u32 %4, %4, 1, %9\n v_lshl_add_u32 %5, %5, 1, %9\n v_lshl_add_u32 %6, %6, 1, %9\n v_lshl_add_u32 %7, %7, 1, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 29)   // v_mad_u64_u32 (pair dst)
                asm volatile("v_mad_u64_u32 %0, vcc, %4, 12, %0\n v_mad_u64_u32 %1, vcc, %5, 12, %1\n v_mad_u64_u32 %2, vcc, %6, 12, %2\n v_mad_u64_u32 %3, vcc, %7, 12, %3\n"
                             "v_mad_u64_u32 %0, vcc, %5, 12, %0\n v_mad_u64_u32 %1, vcc, %6, 12, %1\n v_mad_u64_u32 %2, vcc, %7, 12, %2\n v_mad_u64_u32 %3, vcc, %4, 12, %3\n"
                             : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3) : "v"(a4), "v"(a5), "v"(a6), "v"(a7) : "vcc");
            else if constexpr (KIND == 30)   // v_bfe_u32
                asm volatile("v_bfe_u32 %0, %0, 8, 8\n v_bfe_u32 %1, %1, 8, 8\n v_bfe_u32 %2, %2, 8, 8\n v_bfe_u32 %3, %3, 8, 8\n"
                             "v_bfe_u32 %4, %4, 8, 8\n v_bfe_u32 %5, %5, 8, 8\n v_bfe_u32 %6, %6, 8, 8\n v_bfe_u32 %7, %7, 8, 8\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 31)   // v_min_u32
                asm volatile("v_min_u32 %0, %0, %9\n v_min_u32 %1, %1, %9\n v_min_u32 %2, %2, %9\n v_min_u32 %3, %3, %9\n"
                             "v_min_u32 %4, %4, %9\n v_min_u32 %5, %5, %9\n v_min_u32 %6, %6, %9\n v_min_u32 %7, %7, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 32)   // v_sub_f32 |abs| (VOP3)
                asm volatile("v_sub_f32 %0, |%0|, %9\n v_sub_f32 %1, |%1|, %9\n v_sub_f32 %2, |%2|, %9\n v_sub_f32 %3, |%3|, %9\n"
                             "v_sub_f32 %4, |%4|, %9\n v_sub_f32 %5, |%5|, %9\n v_sub_f32 %6, |%6|, %9\n v_sub_f32 %7, |%7|, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(m0) : "vcc");
            else if constexpr (KIND == 33)   // v_cmp_lt_u32 to SGPR pair (VOP3)
                asm volatile("v_cmp_lt_u32 %8, %0, %1\n v_cmp_lt_u32 %8, %1, %2\n v_cmp_lt_u32 %8, %2, %3\n v_cmp_lt_u32 %8, %3, %4\n"
                             "v_cmp_lt_u32 %8, %4, %5\n v_cmp_lt_u32 %8, %5, %6\n v_cmp_lt_u32 %8, %6, %7\n v_cmp_lt_u32 %8, %7, %0\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) , "+s"(m0) : "v"(m), "v"(k) : "vcc");
            else if constexpr (KIND == 34)   // v_sub_u32
                asm volatile("v_sub_u32 %0, %0, %9\n v_sub_u32 %1, %1, %9\n v_sub_u32 %2, %2, %9\n v_sub_u32 %3, %3, %9\n"
                             "v_sub_u32 %4, %4, %9\n v_sub_u32 %5, %5, %9\n v_sub_u32 %6, %6, %9\n v_sub_u32 %7, %7, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 35)   // v_or_b32
                asm volatile("v_or_b32 %0, %0, %8\n v_or_b32 %1, %1, %8\n v_or_b32 %2, %2, %8\n v_or_b32 %3, %3, %8\n"
                             "v_or_b32 %4, %4, %8\n v_or_b32 %5, %5, %8\n v_or_b32 %6, %6, %8\n v_or_b32 %7, %7, %8\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 36)   // v_xor_b32
                asm volatile("v_xor_b32 %0, %0, %8\n v_xor_b32 %1, %1, %8\n v_xor_b32 %2, %2, %8\n v_xor_b32 %3, %3, %8\n"
                             "v_xor_b32 %4, %4, %8\n v_xor_b32 %5, %5, %8\n v_xor_b32 %6, %6, %8\n v_xor_b32 %7, %7, %8\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 37)   // v_min_f32
                asm volatile("v_min_f32 %0, %0, %9\n v_min_f32 %1, %1, %9\n v_min_f32 %2, %2, %9\n v_min_f32 %3, %3, %9\n"
                             "v_min_f32 %4, %4, %9\n v_min_f32 %5, %5, %9\n v_min_f32 %6, %6, %9\n v_min_f32 %7, %7, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 38)   // v_cvt_i32_f32
                asm volatile("v_cvt_i32_f32 %0, %0\n v_cvt_i32_f32 %1, %1\n v_cvt_i32_f32 %2, %2\n v_cvt_i32_f32 %3, %3\n"
                             "v_cvt_i32_f32 %4, %4\n v_cvt_i32_f32 %5, %5\n v_cvt_i32_f32 %6, %6\n v_cvt_i32_f32 %7, %7\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 39)   // v_rndne_f32
                asm volatile("v_rndne_f32 %0, %0\n v_rndne_f32 %1, %1\n v_rndne_f32 %2, %2\n v_rndne_f32 %3, %3\n"
                             "v_rndne_f32 %4, %4\n v_rndne_f32 %5, %5\n v_rndne_f32 %6, %6\n v_rndne_f32 %7, %7\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 40)   // v_perm_b32
                asm volatile("v_perm_b32 %0, %0, %8, %9\n v_perm_b32 %1, %1, %8, %9\n v_perm_b32 %2, %2, %8, %9\n v_perm_b32 %3, %3, %8, %9\n"
                             "v_perm_b32 %4, %4, %8, %9\n v_perm_b32 %5, %5, %8, %9\n v_perm_b32 %6, %6, %8, %9\n v_perm_b32 %7, %7, %8, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 41)   // v_bfi_b32
                asm volatile("v_bfi_b32 %0, %8, %0, %9\n v_bfi_b32 %1, %8, %1, %9\n v_bfi_b32 %2, %8, %2, %9\n v_bfi_b32 %3, %8, %3, %9\n"
                             "v_bfi_b32 %4, %8, %4, %9\n v_bfi_b32 %5, %8, %5, %9\n v_bfi_b32 %6, %8, %6, %9\n v_bfi_b32 %7, %8, %7, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 42)   // v_and_or_b32
                asm volatile("v_and_or_b32 %0, %0, %8, %9\n v_and_or_b32 %1, %1, %8, %9\n v_and_or_b32 %2, %2, %8, %9\n v_and_or_b32 %3, %3, %8, %9\n"
                             "v_and_or_b32 %4, %4, %8, %9\n v_and_or_b32 %5, %5, %8, %9\n v_and_or_b32 %6, %6, %8, %9\n v_and_or_b32 %7, %7, %8, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 43)   // v_or3_b32
                asm volatile("v_or3_b32 %0, %0, %8, %9\n v_or3_b32 %1, %1, %8, %9\n v_or3_b32 %2, %2, %8, %9\n v_or3_b32 %3, %3, %8, %9\n"
                             "v_or3_b32 %4, %4, %8, %9\n v_or3_b32 %5, %5, %8, %9\n v_or3_b32 %6, %6, %8, %9\n v_or3_b32 %7, %7, %8, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 44)   // v_add3_u32
                asm volatile("v_add3_u32 %0, %0, %8, %9\n v_add3_u32 %1, %1, %8, %9\n v_add3_u32 %2, %2, %8, %9\n v_add3_u32 %3, %3, %8, %9\n"
                             "v_add3_u32 %4, %4, %8, %9\n v_add3_u32 %5, %5, %8, %9\n v_add3_u32 %6, %6, %8, %9\n v_add3_u32 %7, %7, %8, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 45)   // v_lshl_or_b32
                asm volatile("v_lshl_or_b32 %0, %0, 1, %9\n v_lshl_or_b32 %1, %1, 1, %9\n v_lshl_or_b32 %2, %2, 1, %9\n v_lshl_or_b32 %3, %3, 1, %9\n"
                             "v_lshl_or_b32 %4, %4, 1, %9\n v_lshl_or_b32 %5, %5, 1, %9\n v_lshl_or_b32 %6, %6, 1, %9\n v_lshl_or_b32 %7, %7, 1, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 46)   // v_floor_f32
                asm volatile("v_floor_f32 %0, %0\n v_floor_f32 %1, %1\n v_floor_f32 %2, %2\n v_floor_f32 %3, %3\n"
                             "v_floor_f32 %4, %4\n v_floor_f32 %5, %5\n v_floor_f32 %6, %6\n v_floor_f32 %7, %7\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 47)   // v_cvt_u32_f32
                asm volatile("v_cvt_u32_f32 %0, %0\n v_cvt_u32_f32 %1, %1\n v_cvt_u32_f32 %2, %2\n v_cvt_u32_f32 %3, %3\n"
                             "v_cvt_u32_f32 %4, %4\n v_cvt_u32_f32 %5, %5\n v_cvt_u32_f32 %6, %6\n v_cvt_u32_f32 %7, %7\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 48)   // v_subrev_f32
                asm volatile("v_subrev_f32 %0, %9, %0\n v_subrev_f32 %1, %9, %1\n v_subrev_f32 %2, %9, %2\n v_subrev_f32 %3, %9, %3\n"
                             "v_subrev_f32 %4, %9, %4\n v_subrev_f32 %5, %9, %5\n v_subrev_f32 %6, %9, %6\n v_subrev_f32 %7, %9, %7\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 49)   // v_fma_f32 with SGPR operand
                asm volatile("v_fma_f32 %0, %0, %10, %9\n v_fma_f32 %1, %1, %10, %9\n v_fma_f32 %2, %2, %10, %9\n v_fma_f32 %3, %3, %10, %9\n"
                             "v_fma_f32 %4, %4, %10, %9\n v_fma_f32 %5, %5, %10, %9\n v_fma_f32 %6, %6, %10, %9\n v_fma_f32 %7, %7, %10, %9\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k), "s"(s) : "vcc");
            else if constexpr (KIND == 15)   // 4 VALU + 8 SALU: an exec region around every VALU
                asm volatile("s_and_saveexec_b64 %4, %5\n v_fma_f32 %0, %0, %6, %7\n s_or_b64 exec, exec, %4\n"
                             "s_and_saveexec_b64 %4, %5\n v_fma_f32 %1, %1, %6, %7\n s_or_b64 exec, exec, %4\n"
                             "s_and_saveexec_b64 %4, %5\n v_fma_f32 %2, %2, %6, %7\n s_or_b64 exec, exec, %4\n"
                             "s_and_saveexec_b64 %4, %5\n v_fma_f32 %3, %3, %6, %7\n s_or_b64 exec, exec, %4\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "=&s"(m0) : "s"(~0ull), "v"(m), "v"(k) : "scc");
        }
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* o = ticks + 4 * (size_t)(blockIdx.x * 4 + (threadIdx.x >> 6));
        o[0] = t0; o[1] = t1; o[2] = r0; o[3] = r1;
    }
    const float r = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + b0 + b1 + b2 + b3 + b4 + b5 + b6 + b7 + (float)(s + s1 + s2 + s3) + (float)(m0 ^ m1) + (float)(q0 + q1 + q2 + q3);
    if (r == 1.2345678f) *sink = r;
}

// waves_per_simd blocks of 256 threads per CU (4 waves = one per SIMD each); out_host[0] = mean ticks per wave for the loop,
// [1] = max, [2] = wave-instructions per wave (the kind's body x 4 x iters), [3] = the launch's duration in ms (HIP events),
// [4] = shader clock in MHz while the loop ran (sum of s_memtime ticks / sum of s_memrealtime ticks x 100 MHz over the waves),
// [5] = first wave in .. last wave out in us of real time, [6] = VALU per wave, [7] = SALU per wave
extern "C" int kt_debug_valu_rates(kt_ctx* c, int kind, int iters, int waves_per_simd, double out_host[8])
{
    KT_ARG(c && out_host && kind >= 0 && kind < KT_RATE_KINDS && iters > 0 && waves_per_simd >= 1 && waves_per_simd <= 8);
    const int blocks = 256 * waves_per_simd;
    unsigned long long* ticks = nullptr;
    KT_HIP(hipMalloc((void**)&ticks, sizeof(unsigned long long) * blocks * 16));
    float* sink = (float*)&c->counters[8];
#define KT_RATE_CASE(K) case K: hipLaunchKernelGGL(kt_valu_rate_kernel<K>, dim3(blocks), dim3(256), 0, c->stream, iters, ticks, sink); break;
    hipEvent_t ev[2];
    KT_HIP(hipEventCreate(&ev[0])); KT_HIP(hipEventCreate(&ev[1]));
    for (int rep = 0; rep < 2; ++rep) {   // the second launch is the one read back (clocks ramped, code resident)
        if (rep == 1) KT_HIP(hipEventRecord(ev[0], c->stream));
        switch (kind) {
            KT_RATE_CASE(0) KT_RATE_CASE(1) KT_RATE_CASE(2) KT_RATE_CASE(3) KT_RATE_CASE(4) KT_RATE_CASE(5)
            KT_RATE_CASE(6) KT_RATE_CASE(7) KT_RATE_CASE(8) KT_RATE_CASE(9) KT_RATE_CASE(10)
            KT_RATE_CASE(11) KT_RATE_CASE(12) KT_RATE_CASE(13) KT_RATE_CASE(14) KT_RATE_CASE(15)
            KT_RATE_CASE(16) KT_RATE_CASE(17) KT_RATE_CASE(18) KT_RATE_CASE(19) KT_RATE_CASE(20) KT_RATE_CASE(21) KT_RATE_CASE(22) KT_RATE_CASE(23) KT_RATE_CASE(24) KT_RATE_CASE(25) KT_RATE_CASE(26) KT_RATE_CASE(27) KT_RATE_CASE(28) KT_RATE_CASE(29) KT_RATE_CASE(30) KT_RATE_CASE(31) KT_RATE_CASE(32) KT_RATE_CASE(33)
            KT_RATE_CASE(34) KT_RATE_CASE(35) KT_RATE_CASE(36) KT_RATE_CASE(37) KT_RATE_CASE(38) KT_RATE_CASE(39) KT_RATE_CASE(40) KT_RATE_CASE(41) KT_RATE_CASE(42) KT_RATE_CASE(43) KT_RATE_CASE(44) KT_RATE_CASE(45) KT_RATE_CASE(46) KT_RATE_CASE(47) KT_RATE_CASE(48) KT_RATE_CASE(49)
        }
    }
    KT_HIP(hipEventRecord(ev[1], c->stream));
#undef KT_RATE_CASE
    KT_LAUNCH_CHECK();
    unsigned long long* h = (unsigned long long*)malloc(sizeof(unsigned long long) * blocks * 16);
    KT_HIP(hipMemcpyAsync(h, ticks, sizeof(unsigned long long) * blocks * 16, hipMemcpyDeviceToHost, c->stream));
    KT_HIP(hipStreamSynchronize(c->stream));
    double sum = 0, mx = 0, rsum = 0;
    unsigned long long rmin = ~0ull, rmax = 0;
    for (int i = 0; i < blocks * 4; ++i) {
        const double d = (double)(h[4 * i + 1] - h[4 * i]);
        sum += d; if (d > mx) mx = d;
        rsum += (double)(h[4 * i + 3] - h[4 * i + 2]);
        if (h[4 * i + 2] < rmin) rmin = h[4 * i + 2];
        if (h[4 * i + 3] > rmax) rmax = h[4 * i + 3];
    }
    // instructions of the kind's asm body per trip of the inner r loop: {VALU, SALU}
    static const int body[KT_RATE_KINDS][2] = {{8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 8}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0},
                                               {0, 8}, {8, 4}, {4, 8}, {4, 4}, {4, 8}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}, {8, 0}};
    out_host[0] = sum / (blocks * 4); out_host[1] = mx; out_host[2] = (double)iters * 4 * (body[kind][0] + body[kind][1]);
    float ms = 0;
    KT_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    out_host[3] = ms;
    out_host[4] = rsum > 0 ? sum / rsum * 100.0 : 0.0;
    out_host[5] = (double)(rmax - rmin) / 100.0;
    out_host[6] = (double)iters * 4 * body[kind][0];
    out_host[7] = (double)iters * 4 * body[kind][1];
    (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]);
    free(h);
    KT_HIP(hipFree(ticks));
    return KT_OK;
}

// PMC calibration hooks (MI355X_MICROARCH.md "HBM": FETCH_SIZE / WRITE_SIZE are uncalibrated for narrow accesses): stream a buffer
// with exactly tsdf23's access widths -- 2 B per lane (tsdf) or 4 B per lane (colour), one contiguous segment per wave -- so the
// counters can be scaled against a known byte count.  mode 0 = read, 1 = read-modify-write.
template <typename T>
__global__ __launch_bounds__(256) void kt_stream_kernel(T* __restrict__ p, size_t n, int rmw, unsigned int* __restrict__ sink)
{
    unsigned int acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        T v = p[i];
        acc += (unsigned int)v;
        if (rmw) p[i] = (T)(v + 1);
    }
    if (acc == 0x12345678u) *sink = acc;  // keeps the loads alive
}
extern "C" int kt_debug_stream(kt_ctx* c, void* buf, size_t bytes, int elem_size, int rmw)
{
    KT_ARG(c && buf && (elem_size == 2 || elem_size == 4));
    if (elem_size == 2) hipLaunchKernelGGL(kt_stream_kernel<unsigned short>, dim3(8192), dim3(256), 0, c->stream, (unsigned short*)buf, bytes / 2, rmw, &c->counters[8]);
    else hipLaunchKernelGGL(kt_stream_kernel<unsigned int>, dim3(8192), dim3(256), 0, c->stream, (unsigned int*)buf, bytes / 4, rmw, &c->counters[8]);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

// ---- exhaustive check of the voxel kernel's division shortcut --------------------------------------------------------------
// kt_tsdf_consume forms (F W + tsdf) / (W + 1) as q = n y, q' = fma(fma(-d, q, n), y, q) with y = RN(1 / d):
// compared here with the IEEE division for EVERY finite float numerator n and every divisor d = 1 .. 256.
// out[0] = mismatches, out[1] = largest |n| (as float bits) among them, out[2] = mismatches with |n| >= 2^-100
__global__ __launch_bounds__(256) void kt_div_check_kernel(unsigned int* __restrict__ out)
{
    const float d = (float)(blockIdx.y + 1);
    float y = 1.0f / d;
    asm volatile("" : "+v"(y));
    unsigned int bad = 0, bad_big = 0, worst = 0;
    for (unsigned int hi = blockIdx.x; hi < (1u << 16); hi += gridDim.x) {
        const unsigned int base = (hi << 16) | (threadIdx.x << 8);
#pragma unroll 4
        for (unsigned int lo = 0; lo < 256u; ++lo) {
            const unsigned int bits = base | lo;
            if ((bits & 0x7f800000u) == 0x7f800000u) continue;   // inf / NaN
            const float n = __uint_as_float(bits);
            float q = n / d;
            asm volatile("" : "+v"(q));
            const float q0 = n * y;
            const float q1 = __builtin_fmaf(__builtin_fmaf(-d, q0, n), y, q0);
            if (__float_as_uint(q1) != __float_as_uint(q)) {
                ++bad;
                const unsigned int mag = bits & 0x7fffffffu;
                if (mag >= 0x0d800000u) ++bad_big;   // 2^-100
                worst = max(worst, mag);
            }
        }
    }
    if (bad) { atomicAdd(out, bad); atomicMax(out + 1, worst); }
    if (bad_big) atomicAdd(out + 2, bad_big);
}
extern "C" int kt_debug_div_check(kt_ctx* c, unsigned int out_host[3])
{
    KT_ARG(c && out_host);
    unsigned int* d = nullptr;
    KT_HIP(hipMalloc((void**)&d, 3 * sizeof(unsigned int)));
    KT_HIP(hipMemsetAsync(d, 0, 3 * sizeof(unsigned int), c->stream));
    hipLaunchKernelGGL(kt_div_check_kernel, dim3(1024, 256), dim3(256), 0, c->stream, d);
    KT_HIP(hipMemcpyAsync(out_host, d, 3 * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    KT_HIP(hipStreamSynchronize(c->stream));
    KT_HIP(hipFree(d));
    return KT_OK;
}

// ---- negative-brick flags (csrc/kt_volume.hip) and the ray cast's empty-space hops (csrc/kt_raycast.hip) ----------------------
// kt_integrate_tsdf and kt_raycast pass bricks = nullptr; the tracker is the only caller that hands the flags on.  These hooks are the
// same calls with the flags buffer (and, for the ray cast, the COUNT form's counters) passed through -- no device code of their own.
extern "C" int kt_debug_brick_count(int N) { return N > 0 ? (int)kt_brick_count(N) : 0; }

extern "C" int kt_debug_integrate_bricks(kt_ctx* c, const uint16_t* depth_raw, int cols, int rows, const kt_intr* intr, const float volume_size[3],
                                         const kt_mat33* Rcurr_inv, const float tcurr[3], float tranc_dist, int16_t* volume, float* depth_raw_scaled,
                                         const int voxel_wrap[3], uint8_t* color_volume, const uint8_t* colors, const float* nmap_curr, int angle_color,
                                         int N, unsigned char* bricks_dev)
{
    kt_integrate_job j;
    j.depth_raw = depth_raw; j.cols = cols; j.rows = rows; j.intr = intr; j.volume_size = volume_size; j.Rcurr_inv = Rcurr_inv; j.tcurr = tcurr;
    j.tranc_dist = tranc_dist; j.volume = volume; j.depth_raw_scaled = depth_raw_scaled; j.voxel_wrap = voxel_wrap; j.color_volume = color_volume;
    j.colors = colors; j.nmap_curr = nmap_curr; j.angle_color = angle_color; j.N = N; j.bricks = bricks_dev;
    return kt_integrate_tsdf_impl(c, j);
}

// The planned pre-pass (kt_volume.hip "planning ahead") as the tracker runs it one frame early: the pixel records of the frame, then the plan
// for a PREDICTED pose with margins (theta, tau), and the plan's wave-column ranges copied out (tests/test_gpu_headings.py holds every voxel
// that the frame's own pose updates against them).  No device code of its own.  *made_out = 1: wrange_host holds *count_out ranges
// (z0 | z1 << 16, [yg][xg]) made under wave-column shape *wcl_out; 0: kt_integrate_plan answered KT_NO_PLAN, nothing was written.
extern "C" int kt_debug_tsdf_plan_ranges(kt_ctx* c, const uint16_t* depth_raw, const uint8_t* colors, const float* nmap_curr, int cols, int rows,
                                         const kt_intr* intr, const float volume_size[3], const kt_mat33* Rinv_pred, const float t_pred[3], float tranc_dist,
                                         const int voxel_wrap[3], int N, float theta, float tau, unsigned int* wrange_host, size_t wrange_cap,
                                         int* count_out, int* wcl_out, int* made_out)
{
    KT_ARG(c && depth_raw && colors && nmap_curr && intr && volume_size && Rinv_pred && t_pred && voxel_wrap && wrange_host && count_out && wcl_out && made_out);
    KT_ARG(cols > 0 && rows > 0 && N > 0 && N <= 1536 && theta >= 0 && tau >= 0);
    for (int k = 0; k < 3; ++k) KT_ARG(voxel_wrap[k] >= 0);
    *count_out = 0; *wcl_out = 0; *made_out = 0;
    kt_mem mem;
    kt_tsdf_plan plan;
    float* scaled = nullptr; float* dpmax = nullptr; unsigned char* rec = nullptr;
    int s = mem.device(&scaled, (size_t)cols * rows);
    if (s == KT_OK) s = mem.device(&dpmax, kt_integrate_dpmax_bytes(cols, rows) / sizeof(float));
    if (s == KT_OK) s = mem.device(&rec, kt_integrate_rec_bytes(cols, rows));
    if (s == KT_OK) s = kt_tsdf_plan_alloc(&plan, N);
    if (s == KT_OK) s = kt_integrate_prepare(c, depth_raw, colors, nmap_curr, cols, rows, intr, 1, scaled, rec, dpmax);
    int made = KT_NO_PLAN;
    if (s == KT_OK) {
        made = kt_integrate_plan(c->stream, &plan, rec, dpmax, cols, rows, intr, volume_size, Rinv_pred, t_pred, tranc_dist, voxel_wrap, N, theta, tau);
        if (made != KT_NO_PLAN) s = made;
    }
    if (s == KT_OK && made != KT_NO_PLAN) {
        int wx, wy, xg, yg;
        kt_tsdf_plan_shape(&plan, cols, rows, N, &wx, &wy, &xg, &yg);
        if ((size_t)xg * yg > wrange_cap) { kt_set_error("kt_debug_tsdf_plan_ranges: wrange_host is too small"); s = KT_ERR_ARG; }
        else {
            s = kt_check(hipMemcpyAsync(wrange_host, plan.wrange, sizeof(unsigned int) * (size_t)xg * yg, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync", __FILE__, __LINE__);
            *count_out = xg * yg; *wcl_out = plan.wcl; *made_out = 1;
        }
    }
    const int s2 = kt_check(hipStreamSynchronize(c->stream), "hipStreamSynchronize", __FILE__, __LINE__);   // (before the buffers go)
    kt_tsdf_plan_free(&plan);
    mem.release();
    return s != KT_OK ? s : s2;
}

extern "C" int kt_debug_raycast_bricks(kt_ctx* c, const kt_intr* intr, const kt_mat33* Rcurr, const float tcurr[3], float tranc_dist,
                                       const float volume_size[3], const int16_t* volume, float* vmap, float* nmap, int cols, int rows,
                                       const int voxel_wrap[3], uint8_t* vmap_curr_color, const uint8_t* color_volume, int N,
                                       const unsigned char* bricks_dev, unsigned long long counts_host[4])
{
    KT_ARG(c && counts_host);
    unsigned long long* d = nullptr;
    KT_HIP(hipMalloc((void**)&d, 4 * sizeof(unsigned long long)));
    int s = kt_check(hipMemsetAsync(d, 0, 4 * sizeof(unsigned long long), c->stream), "hipMemsetAsync", __FILE__, __LINE__);
    if (s == KT_OK)
        s = kt_raycast_impl(c, intr, Rcurr, tcurr, tranc_dist, volume_size, volume, vmap, nmap, cols, rows, voxel_wrap, vmap_curr_color, color_volume, N,
                            d, nullptr, nullptr, nullptr, bricks_dev);
    if (s == KT_OK) s = kt_check(hipMemcpyAsync(counts_host, d, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync", __FILE__, __LINE__);
    const int s2 = kt_check(hipStreamSynchronize(c->stream), "hipStreamSynchronize", __FILE__, __LINE__);
    (void)hipFree(d);
    return s != KT_OK ? s : s2;
}

// ---- the ray cast's voxel indexing: the forms the kernel runs (csrc/kt_rc_index.hpp) next to the ones they replaced ------------------------
// One launch per (w, N) pair, one thread per float.  Thread i takes the coordinates (q[i], q[i + 1], q[i + 2]) (indices modulo n) and the
// storage wrap (w, N - 1 - w, (w + N / 2 + 1) mod N), and writes KT_RCI_WORDS words per form:
//   0 voxel of q[i]   1 axis guard of q[i]   2 the march's guard of the three   3 inside the volume   4 the march's element (0 outside)
//   5 the march's load is inside the volume's N^3 words   6, 7 kt_rc::axis's tap offsets of voxel g, g + 1 of q[i] along z and y (0 unless
//   0 <= g, g + 1 < N)   8 kt_rc::index of the three voxels clamped to [0, N - 1]   9 the hop's brick index of the three voxels clamped to
//   [0, N] and divided by 32 (0 unless N % 32 == 0)
#define KT_RCI_WORDS 10
template <bool POW2>
__global__ __launch_bounds__(256) void kt_rc_index_kernel(const float* __restrict__ q, int n, int w, int N, int log2N, unsigned int* __restrict__ out_old,
                                                          unsigned int* __restrict__ out_new)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float c[3] = {q[i], q[(i + 1) % n], q[(i + 2) % n]};
    const int wr[3] = {w, N - 1 - w, (w + N / 2 + 1) % N};
    const unsigned int uN = (unsigned int)N;
    const int nb = N / KT_BRICK;
    const bool bricks = (N % KT_BRICK) == 0;
    unsigned int* o = out_old + (size_t)i * KT_RCI_WORDS;
    unsigned int* e = out_new + (size_t)i * KT_RCI_WORDS;
    // ---- the former forms, as the ray cast had them (csrc/kt_raycast.hip, then still a part of kt_volume.hip) ----
    {
        int g[3]; float fr[3];
        for (int k = 0; k < 3; ++k) { const float fl = __builtin_floorf(c[k]); g[k] = kt_cvt_i32(fl); fr[k] = c[k] - fl; }
        o[0] = (unsigned int)g[0];
        o[1] = fr[0] > 2e-4f && fr[0] < 1.0f - 2e-4f && fabsf(c[0]) < 1024.f;
        const float off = __builtin_fmaxf(__builtin_fmaxf(fabsf(fr[0] - 0.5f), fabsf(fr[1] - 0.5f)), fabsf(fr[2] - 0.5f));
        const float big = __builtin_fmaxf(__builtin_fmaxf(fabsf(c[0]), fabsf(c[1])), fabsf(c[2]));
        o[2] = off < 0.5f - 2e-4f && big < 1024.f;
        const unsigned int ux = (unsigned int)g[0], uy = (unsigned int)g[1], uz = (unsigned int)g[2];
        const bool inb = ux < uN && uy < uN && uz < uN;
        unsigned int X = ux + (unsigned int)wr[0]; X -= (X >= uN) ? uN : 0u;
        unsigned int Y = uy + (unsigned int)wr[1]; Y -= (Y >= uN) ? uN : 0u;
        unsigned int Z = uz + (unsigned int)wr[2]; Z -= (Z >= uN) ? uN : 0u;
        const unsigned int gidx = kt_mad24u(kt_mad24u(Z, uN, Y), uN, X);
        o[3] = inb; o[4] = inb ? gidx : 0u; o[5] = 1u;
        const bool taps = g[0] >= 0 && g[0] < N - 1;
        for (int d = 0; d < 2; ++d) {
            int t = g[0] + d + wr[d == 0 ? 2 : 1]; if (t >= N) t -= N;
            const unsigned int v = d == 0 ? kt_mul24(kt_mul24((unsigned int)t, uN), uN) : kt_mul24((unsigned int)t, uN);
            o[6 + d] = taps ? v : 0u;
        }
        int cl[3], br[3];
        for (int k = 0; k < 3; ++k) {
            cl[k] = max(0, min(g[k], N - 1)) + wr[k]; if (cl[k] >= N) cl[k] -= N;
            br[k] = (max(0, min(g[k], N)) >> KT_BRICK_LOG2) + (wr[k] >> KT_BRICK_LOG2); br[k] -= (br[k] >= nb) ? nb : 0;
        }
        o[8] = kt_mad24(kt_mad24((unsigned int)cl[2], uN, (unsigned int)cl[1]), uN, (unsigned int)cl[0]);
        o[9] = bricks ? kt_mad24(kt_mad24((unsigned int)br[2], (unsigned int)nb, (unsigned int)br[1]), (unsigned int)nb, (unsigned int)br[0]) : 0u;
    }
    // ---- the forms the kernel runs ----
    {
        const kt_rc_ix<POW2> ix{uN, (unsigned int)log2N};
        const kt_rc_ix<POW2> bix{(unsigned int)nb, (unsigned int)(log2N - KT_BRICK_LOG2)};
        int g[3];
        for (int k = 0; k < 3; ++k) g[k] = kt_cvt_flr_i32(c[k]);
        e[0] = (unsigned int)g[0];
        e[1] = kt_rc_safe1(c[0]);
        e[2] = kt_rc_safe3(c[0], c[1], c[2]);
        const unsigned int ux = (unsigned int)g[0], uy = (unsigned int)g[1], uz = (unsigned int)g[2];
        const bool inb = ix.inside(ux, uy, uz);
        unsigned int vw[3] = {(unsigned int)wr[0], (unsigned int)wr[1], (unsigned int)wr[2]};
        const unsigned int off = ix.sample_offset(ux, uy, uz, vw[0], vw[1], vw[2], inb);
        const unsigned int el = POW2 ? off >> 1 : off;   // (POW2: the byte offset of a 16-bit word, always even)
        e[3] = inb; e[4] = inb ? el : 0u; e[5] = (POW2 ? (off & 1u) == 0u : true) && (unsigned long long)el < (unsigned long long)uN * uN * uN;
        const bool taps = g[0] >= 0 && g[0] < N - 1;
        const unsigned int t0 = ix.template stride<2>(ix.wrap((unsigned int)g[0], (unsigned int)wr[2]));
        const unsigned int t1 = ix.template stride<1>(ix.wrap((unsigned int)(g[0] + 1), (unsigned int)wr[1]));
        e[6] = taps ? t0 : 0u; e[7] = taps ? t1 : 0u;
        unsigned int cl[3], br[3];
        for (int k = 0; k < 3; ++k) {
            cl[k] = ix.wrap((unsigned int)max(0, min(g[k], N - 1)), (unsigned int)wr[k]);
            br[k] = bricks ? bix.wrap((unsigned int)(max(0, min(g[k], N)) >> KT_BRICK_LOG2), (unsigned int)(wr[k] >> KT_BRICK_LOG2)) : 0u;
        }
        e[8] = ix.linear(cl[0], cl[1], cl[2]);
        e[9] = bricks ? bix.linear(br[0], br[1], br[2]) : 0u;
    }
}

extern "C" int kt_debug_rc_index(kt_ctx* c, const float* q_host, int n, const int32_t* wN_host, int pairs, uint32_t* out_old_host, uint32_t* out_new_host)
{
    KT_ARG(c && q_host && wN_host && out_old_host && out_new_host && n > 0 && pairs > 0);
    for (int p = 0; p < pairs; ++p) KT_ARG(wN_host[2 * p + 1] > 0 && wN_host[2 * p + 1] <= 1536 && wN_host[2 * p] >= 0 && wN_host[2 * p] < wN_host[2 * p + 1]);
    kt_mem mem;
    float* q = nullptr; unsigned int* o = nullptr; unsigned int* e = nullptr;
    const size_t words = (size_t)n * KT_RCI_WORDS;
    int s = mem.device(&q, (size_t)n);
    if (s == KT_OK) s = mem.device(&o, words);
    if (s == KT_OK) s = mem.device(&e, words);
    if (s == KT_OK) s = kt_check(hipMemcpyAsync(q, q_host, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync", __FILE__, __LINE__);
    for (int p = 0; p < pairs && s == KT_OK; ++p) {
        const int w = wN_host[2 * p], N = wN_host[2 * p + 1];
        int log2N = -1;
        if ((N & (N - 1)) == 0) { log2N = 0; while ((1 << log2N) < N) ++log2N; }
        if (log2N >= 0) hipLaunchKernelGGL(kt_rc_index_kernel<true>, dim3(kt_div_up(n, 256)), dim3(256), 0, c->stream, q, n, w, N, log2N, o, e);
        else hipLaunchKernelGGL(kt_rc_index_kernel<false>, dim3(kt_div_up(n, 256)), dim3(256), 0, c->stream, q, n, w, N, log2N, o, e);
        s = kt_check(hipGetLastError(), "kt_rc_index_kernel", __FILE__, __LINE__);
        if (s == KT_OK) s = kt_check(hipMemcpyAsync(out_old_host + (size_t)p * words, o, sizeof(unsigned int) * words, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync", __FILE__, __LINE__);
        if (s == KT_OK) s = kt_check(hipMemcpyAsync(out_new_host + (size_t)p * words, e, sizeof(unsigned int) * words, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync", __FILE__, __LINE__);
        if (s == KT_OK) s = kt_check(hipStreamSynchronize(c->stream), "hipStreamSynchronize", __FILE__, __LINE__);
    }
    const int s2 = kt_check(hipStreamSynchronize(c->stream), "hipStreamSynchronize", __FILE__, __LINE__);   // (before the buffers go)
    mem.release();
    return s != KT_OK ? s : s2;
}
