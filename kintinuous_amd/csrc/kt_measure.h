/* kt_measure.h -- libkt_debug.so: measurement kernels that are NOT in the product library (round 6).  Loaded by
 * scripts/pmc_calibrate.py, scripts/valu_rates.py and tests/test_gpu_volume.py next to libkt_hip.so, whose context type and error reporting it uses. */
#ifndef KT_MEASURE_H
#define KT_MEASURE_H

#include "../../include/kt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* PMC calibration hook: stream `bytes` of a device buffer with 2- or 4-byte-per-lane coalesced accesses (the widths of the tsdf /
 * colour volume accesses); rmw = 0 reads, 1 reads and writes back.  Used by scripts/pmc_calibrate.py to scale FETCH_SIZE / WRITE_SIZE. */
int kt_debug_stream(kt_ctx* ctx, void* buf, size_t bytes, int elem_size, int rmw);
/* PMC calibration on the voxel kernel's own access pattern: a wave owns a 32 x 2 wave-column of an N x N x Z array and walks z, so an
 * access is two 32-lane rows (64 B at elem_size 2, 128 B at 4).  halves = 2 reads every element once; halves = 1 only the even
 * wave-columns (elem_size 2: the left 64 bytes of every 128-byte line).  N % 32 == 0, Z % 4 == 0. */
int kt_debug_stream_rows(kt_ctx* ctx, void* buf, int N, int Z, int elem_size, int halves, int rmw);
/* issue cost of one instruction kind (csrc/kt_debug.hip lists them) at waves_per_simd resident waves: out_host = {mean, max shader
 * ticks per wave for the loop, wave-instructions per wave, launch duration in ms, shader clock in MHz while the loop ran (s_memtime
 * against the 100 MHz s_memrealtime), first wave in .. last wave out in us, VALU per wave, SALU per wave} */
int kt_debug_valu_rates(kt_ctx* ctx, int kind, int iters, int waves_per_simd, double out_host[8]);
/* test hook: the voxel kernel's division shortcut (table reciprocal + one correction) against the IEEE division for every finite float
 * numerator and every divisor 1..256: out_host = {mismatches, float bits of the largest |numerator| among them, mismatches at |n| >= 2^-100} */
int kt_debug_div_check(kt_ctx* ctx, unsigned int out_host[3]);
/* Test hooks of the negative-brick flags and the ray cast's empty-space hops (tests/test_gpu_bricks.py).  They run no device code of
 * their own: each is the boundary call of the same name with the arguments the library's internal entry points already take
 * (csrc/kt_internal.hpp: kt_integrate_tsdf_impl, kt_raycast_impl) and the boundary leaves null.  The fourth hook, kt_tracker_debug_bricks,
 * reads a tracker's own flags and is declared in csrc/kt_debug.h.
 * kt_debug_brick_count: the number of flag bytes of an N^3 volume, ceil(N / 32)^3 ([bz][by][bx] over storage bricks). */
int kt_debug_brick_count(int N);
/* kt_integrate_tsdf with the flags buffer handed on: every voxel-kernel form (lean, round-3, pointer-addressed, both wave-column shapes, NT
 * stores) sets bricks_dev[brick] = 1 when it stores a negative tsdf word into that storage brick, and writes nothing else to the buffer.
 * N % 32 != 0: the buffer is ignored (the call is kt_integrate_tsdf). */
int kt_debug_integrate_bricks(kt_ctx* ctx, const uint16_t* depth_raw, int cols, int rows, const kt_intr* intr, const float volume_size[3],
                              const kt_mat33* Rcurr_inv, const float tcurr[3], float tranc_dist, int16_t* volume, float* depth_raw_scaled,
                              const int voxel_wrap[3], uint8_t* color_volume, const uint8_t* colors, const float* nmap_curr, int angle_color,
                              int N, unsigned char* bricks_dev);
/* Test hook of the voxel pass's PLANNED pre-pass (tests/test_gpu_headings.py), no device code of its own: the frame's pixel records
 * (kt_integrate_prepare, colour-angle test on), then kt_integrate_plan for the predicted pose (Rinv_pred, t_pred) with margins theta (rad)
 * and tau (m) under the wave-column shape a launch would pick now (kt_debug_tsdf_wcl), and the plan's wave-column ranges copied to the host:
 * wrange_host[yg * XG + xg] = z0 | z1 << 16 over LOGICAL z for the 2^wcl x (64 >> wcl) STORAGE columns of wave-column (xg, yg),
 * XG = ceil(N / 2^wcl); z0 >= z1: no task.  *count_out = their number (<= wrange_cap, else KT_ERR_ARG), *wcl_out = the shape.
 * *made_out = 0: the margins are too wide for a plan (KT_NO_PLAN, not an error) and nothing was written.  Synchronous. */
int kt_debug_tsdf_plan_ranges(kt_ctx* ctx, const uint16_t* depth_raw, const uint8_t* colors, const float* nmap_curr, int cols, int rows,
                              const kt_intr* intr, const float volume_size[3], const kt_mat33* Rinv_pred, const float t_pred[3], float tranc_dist,
                              const int voxel_wrap[3], int N, float theta, float tau, unsigned int* wrange_host, size_t wrange_cap,
                              int* count_out, int* wcl_out, int* made_out);
/* kt_raycast in its counting form, with the flags handed on: bricks_dev != null and N % 32 == 0 (and at most 32768 bricks) runs
 * kt_raycast_kernel<COUNT, no PYR, SKIP>, otherwise the no-SKIP kernel with counters.  counts_host = {march samples S (hopped ones
 * included: equal to the reference's S), samples replaced by hops, wave-level hop iterations, wave-level batch iterations}.  Synchronous.
 * The pyramid-fused form (PYR) takes arguments kt_raycast does not have: PYR + SKIP is reached through the tracker only. */
int kt_debug_raycast_bricks(kt_ctx* ctx, const kt_intr* intr, const kt_mat33* Rcurr, const float tcurr[3], float tranc_dist,
                            const float volume_size[3], const int16_t* volume, float* vmap, float* nmap, int cols, int rows,
                            const int voxel_wrap[3], uint8_t* vmap_curr_color, const uint8_t* color_volume, int N,
                            const unsigned char* bricks_dev, unsigned long long counts_host[4]);
/* Test hook of the ray cast's voxel indexing (tests/test_gpu_raycast_index.py): the functions of csrc/kt_rc_index.hpp that the kernel runs --
 * floor-and-convert in one instruction, the guard band by the fraction instruction, the in-volume test, the storage wrap and the linear index
 * in their power-of-two and general forms -- next to the forms they replaced, on n caller-supplied floats and `pairs` (w, N) pairs
 * (wN_host = {w, N} each, 0 <= w < N <= 1536).  For pair p and float i, out_*_host[(p * n + i) * 10 ..] = the ten words csrc/kt_debug.hip
 * lists (voxel, both guard decisions, in-volume flag, march element, load-in-bounds flag, two axis tap offsets, kt_rc::index, brick index) of
 * the coordinates (q[i], q[i + 1], q[i + 2]) under the wrap (w, N - 1 - w, (w + N / 2 + 1) mod N): out_old from the former forms, out_new from
 * the present ones.  Every word must be equal.  Synchronous. */
int kt_debug_rc_index(kt_ctx* ctx, const float* q_host, int n, const int32_t* wN_host, int pairs, uint32_t* out_old_host, uint32_t* out_new_host);

#ifdef __cplusplus
}
#endif
#endif
