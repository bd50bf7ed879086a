// kt_deform.hip -- the consumer of the optimised trajectory: the deformation graph that the reference builds over the camera poses and
// solves after every accepted loop (backend/DeformationGraph.cpp, driven by Deformation::addCameraLoop, backend/Deformation.cpp:258-334).
// NOT a port: no CHOLMOD, no PCL, no incremental bookkeeping -- a defined stage with the reference's energy, graph, weights and constants
// (include/kt_abi.h and DESIGN.md 4.11 state it; kintinuous_amd/deform_ref.py restates it in the same operation order).
//   graph      M nodes in time order, node i = (g_i, t_i, A_i, b_i); the state x is 12 doubles per node in the reference's column order:
//              A column-major (x[3 c + r] = A(r, c)), then b.  Neighbours: i -+ 1, i -+ 2, the first / last two nodes take the first / last five.
//   weights    df_weigh: the node nearest in time, a window of 20 nodes around it, the five nearest of the window in float, weights in double
//   apply      df_normal_mats + df_apply on 48-byte points with stored weights; df_apply_mesh on the -m mesh's 16-byte vertices in spans of one
//              time each: weights and position fused, the span's window of nodes in LDS, from the bodies of df_weigh and df_position
//   energy     6 E_rot rows per node, 3 E_reg rows per (node, neighbour), 3 E_con rows per constraint (wRot 1, wReg 10, wCon 100)
//   a step     df_assemble (J^T J in scalar band storage: 12 x 12 blocks, block half-bandwidth 19, so 240 doubles per column), df_gradient,
//              df_solve (banded L D L^T, forward and backward substitution in ONE workgroup), df_update, then the evaluation: df_nodes_eval,
//              df_cons_eval, df_tally.  All steps are enqueued at once; every kernel returns at once when the state's `done` word is set.
// Everything is double, uncontracted, in a fixed order, with + - * / and sqrt alone: no floating-point atomics, every entry of the normal
// matrix is summed by one lane (rotation rows, then the regularisation rows by (owner, neighbour slot), then the constraints in index order
// from the per-node constraint lists), so a call returns the same bytes every time.
#include "kt_internal.hpp"
#include "kt_wave.hpp"

#include <math.h>
#include <string.h>

#define KT_DF_LANES 256
#define KT_DF_SOLVE_LANES 1024
#define KT_DF_LOOKBACK 20                          // weightVerticesSeq's lookBack
#define KT_DF_BAND (12 * KT_DF_LOOKBACK)           // scalar band: the diagonal and 239 entries below it
#define KT_DF_MAX_NODES 4096
#define KT_DF_MAX_CONSTRAINTS (1 << 17)              // df_list_count / df_list_fill walk every constraint once per node lane: O(M n_con)
#define KT_DF_PIVOT_MIN 1e-12                      // a pivot below this share of its diagonal entry of J^T J: singular (see df_solve)
#define KT_DF_MAX_STEPS 64                         // the limit of kt_deform_params::max_steps: every step is enqueued ahead
#define KT_DF_SQ_REG 3.1622776601683795            // sqrt(wReg = 10), correctly rounded
#define KT_DF_SQ_CON 10.0                          // sqrt(wCon = 100)

struct kt_df_state {
    double error_start, error_end, constraint_error, last_error;
    int steps, status, done, singular;
};

namespace {

// ---- the window of a time (weightVerticesSeq's search): the node nearest in time, then one run of at most 20 consecutive nodes ----
__device__ __forceinline__ void df_window(unsigned long long t, const unsigned long long* __restrict__ gt, int M, int* first_out, int* last_out)
{
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (gt[mid] < t) lo = mid + 1; else hi = mid;
    }
    int found;
    if (lo == 0) found = 0;
    else if (lo == M) found = M - 1;
    else {
        const long long a = (long long)(gt[lo - 1] - t), b = (long long)(gt[lo] - t);
        found = (a < 0 ? -a : a) <= (b < 0 ? -b : b) ? lo - 1 : lo;   // a tie goes to the lower index
    }
    // found, found - 1, ... (at most 20), topped up with found + 1, ...: one run of consecutive nodes
    const int first = max(0, found - (KT_DF_LOOKBACK - 1));
    *first_out = first;
    *last_out = min(M - 1, first + (KT_DF_LOOKBACK - 1));
}

// ---- the weights of one vertex over the window first..last: idx[4] ascending, w[4].  Node i is read at gf[i - base] and gd + 4 (i - base):
// base = 0 for the arrays in global memory, base = first for a workgroup's copy of the window in LDS (df_apply_mesh) ----
__device__ __forceinline__ void df_weigh_window(float px, float py, float pz, int first, int last, const float4* gf, const double* gd, int base, int* idx, double* w)
{
    float bd[5];
    int bi[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) { bd[s] = __builtin_inff(); bi[s] = 0x7fffffff; }
    for (int i = first; i <= last; ++i) {
        const float4 g = gf[i - base];
        const float dx = g.x - px, dy = g.y - py, dz = g.z - pz;
        float cd = sqrtf((dx * dx + dy * dy) + dz * dz);
        if (!(cd == cd)) cd = __builtin_inff();   // a NaN orders like +inf: the five slots always hold nodes
        int ci = i;
#pragma unroll
        for (int s = 0; s < 5; ++s) {   // insertion by (distance, index)
            if (cd < bd[s] || (cd == bd[s] && ci < bi[s])) {
                const float td = bd[s]; bd[s] = cd; cd = td;
                const int ti = bi[s]; bi[s] = ci; ci = ti;
            }
        }
    }
    const double dmax = (double)bd[4];
    double ws[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const double* g = gd + 4 * (size_t)(bi[s] - base);
        const double ex = (double)px - g[0], ey = (double)py - g[1], ez = (double)pz - g[2];
        const double dd = sqrt((ex * ex + ey * ey) + ez * ez), u = 1.0 - dd / dmax;
        ws[s] = u * u;
    }
    const double sum = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    const bool flat = sum == 0.0 || !(fabs(sum) < __builtin_inf());
#pragma unroll
    for (int s = 0; s < 4; ++s) ws[s] = flat ? 0.25 : ws[s] / sum;
    int id[4] = {bi[0], bi[1], bi[2], bi[3]};
#define KT_DF_CSWAP(a, b) if (id[b] < id[a]) { const int ti = id[a]; id[a] = id[b]; id[b] = ti; const double tw = ws[a]; ws[a] = ws[b]; ws[b] = tw; }
    KT_DF_CSWAP(0, 1) KT_DF_CSWAP(2, 3) KT_DF_CSWAP(0, 2) KT_DF_CSWAP(1, 3) KT_DF_CSWAP(1, 2)
#undef KT_DF_CSWAP
#pragma unroll
    for (int s = 0; s < 4; ++s) { idx[s] = id[s]; w[s] = ws[s]; }
}

// ---- the weights of one vertex (weightVerticesSeq), the node arrays in global memory ----
__device__ __forceinline__ void df_weigh(float px, float py, float pz, unsigned long long t, const float4* __restrict__ gf, const double* __restrict__ gd,
                                         const unsigned long long* __restrict__ gt, int M, int* idx, double* w)
{
    int first, last;
    df_window(t, gt, M, &first, &last);
    df_weigh_window(px, py, pz, first, last, gf, gd, 0, idx, w);
}

// POINTS: 48-byte kt_point_xyzrgbnormal records (the first 16 bytes are read); else 3 floats per vertex.  One lane per vertex.
template <bool POINTS>
__global__ __launch_bounds__(KT_DF_LANES) void df_weights(const float* __restrict__ src, const unsigned long long* __restrict__ times, size_t n,
                                                          const float4* __restrict__ gf, const double* __restrict__ gd,
                                                          const unsigned long long* __restrict__ gt, int M, int* __restrict__ idx, double* __restrict__ w)
{
    const size_t i = (size_t)blockIdx.x * KT_DF_LANES + threadIdx.x;
    if (i >= n) return;
    float px, py, pz;
    if (POINTS) { const float4 p = reinterpret_cast<const float4*>(src)[3 * i]; px = p.x; py = p.y; pz = p.z; }
    else { px = src[3 * i]; py = src[3 * i + 1]; pz = src[3 * i + 2]; }
    int id[4];
    double ws[4];
    df_weigh(px, py, pz, times[i], gf, gd, gt, M, id, ws);
    reinterpret_cast<int4*>(idx)[i] = make_int4(id[0], id[1], id[2], id[3]);
    reinterpret_cast<double2*>(w)[2 * i] = make_double2(ws[0], ws[1]);
    reinterpret_cast<double2*>(w)[2 * i + 1] = make_double2(ws[2], ws[3]);
}

// ---- computeVertexPosition: sum_i w_i (A_i (p - g_i) + g_i + b_i), the nodes in ascending order; node i at x + 12 (i - base), gd + 4 (i - base) ----
__device__ __forceinline__ void df_position(const double* p, const int* id, const double* ws, const double* x, const double* gd, int base, double* o)
{
    o[0] = o[1] = o[2] = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const double *xs = x + 12 * (size_t)(id[s] - base), *g = gd + 4 * (size_t)(id[s] - base);
        const double d0 = p[0] - g[0], d1 = p[1] - g[1], d2 = p[2] - g[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            double t = (xs[r] * d0 + xs[3 + r] * d1) + xs[6 + r] * d2;
            t = t + g[r];
            t = t + xs[9 + r];
            o[r] = o[r] + ws[s] * t;
        }
    }
}

// the workgroup's sum of v to *out: kt_wave_sum inside every wave, then the four waves in order
__device__ __forceinline__ void df_block_fold(double v, double* wave_sh, double* out)
{
    const int t = threadIdx.x;
    const double s = kt_wave_sum(v);
    if ((t & 63) == 0) wave_sh[t >> 6] = s;
    __syncthreads();
    if (t == 0) {
        double c = wave_sh[0];
        for (int k = 1; k < KT_DF_LANES / 64; ++k) c = c + wave_sh[k];
        *out = c;
    }
}

// entry (row, col) of a node's six E_rot rows over its nine rotation unknowns (sparseJacobian)
__device__ __forceinline__ double df_jrot(const double* A, int row, int col)
{
    const int c = col / 3, r = col % 3;
    switch (row) {
    case 0: return c == 0 ? A[3 + r] : c == 1 ? A[r] : 0.0;
    case 1: return c == 0 ? A[6 + r] : c == 2 ? A[r] : 0.0;
    case 2: return c == 1 ? A[6 + r] : c == 2 ? A[3 + r] : 0.0;
    default: return c == row - 3 ? 2.0 * A[col] : 0.0;
    }
}

// ---- the residuals of the nodes: 6 E_rot and 4 x 3 E_reg each, and the workgroup's share of the error ----
__global__ __launch_bounds__(KT_DF_LANES) void df_nodes_eval(const kt_df_state* __restrict__ st, const double* __restrict__ x, const double* __restrict__ gd,
                                                             const int* __restrict__ nb, int M, double* __restrict__ rrot, double* __restrict__ rreg,
                                                             double* __restrict__ part)
{
    __shared__ double wave_sh[KT_DF_LANES / 64];
    if (st->done) return;
    const int j = blockIdx.x * KT_DF_LANES + threadIdx.x;
    double en = 0.0;
    if (j < M) {
        double A[12];
        for (int e = 0; e < 12; ++e) A[e] = x[12 * (size_t)j + e];
        double rr[6];
        rr[0] = (A[0] * A[3] + A[1] * A[4]) + A[2] * A[5];
        rr[1] = (A[0] * A[6] + A[1] * A[7]) + A[2] * A[8];
        rr[2] = (A[3] * A[6] + A[4] * A[7]) + A[5] * A[8];
        rr[3] = ((A[0] * A[0] + A[1] * A[1]) + A[2] * A[2]) - 1.0;
        rr[4] = ((A[3] * A[3] + A[4] * A[4]) + A[5] * A[5]) - 1.0;
        rr[5] = ((A[6] * A[6] + A[7] * A[7]) + A[8] * A[8]) - 1.0;
        for (int e = 0; e < 6; ++e) { rrot[6 * (size_t)j + e] = rr[e]; en = en + rr[e] * rr[e]; }
        const double* gj = gd + 4 * (size_t)j;
        for (int k = 0; k < 4; ++k) {
            const int n = nb[4 * j + k];
            const double *gn = gd + 4 * (size_t)n, *bn = x + 12 * (size_t)n + 9;
            const double e0 = gn[0] - gj[0], e1 = gn[1] - gj[1], e2 = gn[2] - gj[2];
            for (int r = 0; r < 3; ++r) {
                double t = (A[r] * e0 + A[3 + r] * e1) + A[6 + r] * e2;
                t = t + gj[r];
                t = t + A[9 + r];
                const double u = gn[r] + bn[r], res = (t - u) * KT_DF_SQ_REG;
                rreg[3 * (size_t)(4 * j + k) + r] = res;
                en = en + res * res;
            }
        }
    }
    df_block_fold(en, wave_sh, part + blockIdx.x);
}

// ---- the residuals of the constraints and the workgroup's share of the error ----
__global__ __launch_bounds__(KT_DF_LANES) void df_cons_eval(const kt_df_state* __restrict__ st, const double* __restrict__ x, const double* __restrict__ gd,
                                                            const float* __restrict__ csrc, const int* __restrict__ cidx, const double* __restrict__ cw,
                                                            const double* __restrict__ ctgt, int n_con, double* __restrict__ rcon, double* __restrict__ part)
{
    __shared__ double wave_sh[KT_DF_LANES / 64];
    if (st->done) return;
    const int l = blockIdx.x * KT_DF_LANES + threadIdx.x;
    double ec = 0.0;
    if (l < n_con) {
        const double p[3] = {(double)csrc[3 * (size_t)l], (double)csrc[3 * (size_t)l + 1], (double)csrc[3 * (size_t)l + 2]};
        int id[4];
        double ws[4], o[3];
        for (int s = 0; s < 4; ++s) { id[s] = cidx[4 * (size_t)l + s]; ws[s] = cw[4 * (size_t)l + s]; }
        df_position(p, id, ws, x, gd, 0, o);
        for (int r = 0; r < 3; ++r) {
            const double res = (o[r] - ctgt[3 * (size_t)l + r]) * KT_DF_SQ_CON;
            rcon[3 * (size_t)l + r] = res;
            ec = ec + res * res;
        }
    }
    df_block_fold(ec, wave_sh, part + blockIdx.x);
}

// ---- the error of the state just evaluated and the bookkeeping of the step that led to it (step = 0: the start and the 0.1 gate) ----
__global__ void df_tally(kt_df_state* __restrict__ st, kt_deform_params p, const double* __restrict__ nodepart, int nnp, const double* __restrict__ conpart, int ncp,
                         const double* __restrict__ deltapart, int ndp, int n_con, int step)
{
    if (threadIdx.x != 0 || st->done) return;
    double en = 0.0, ec = 0.0;
    for (int i = 0; i < nnp; ++i) en = en + nodepart[i];
    for (int i = 0; i < ncp; ++i) ec = ec + conpart[i];
    const double err = en + ec;
    st->error_end = err;
    if (step == 0) {
        const double ce = n_con > 0 ? sqrt(ec) / (double)n_con : 0.0;
        st->error_start = err;
        st->constraint_error = ce;
        if (n_con == 0 || ce < p.significant_error) { st->done = 1; st->status = KT_DEFORM_INSIGNIFICANT; }
        else if (p.max_steps == 0) { st->done = 1; st->status = KT_DEFORM_MAX_STEPS; }
    } else {
        double d2 = 0.0;
        for (int i = 0; i < ndp; ++i) d2 = d2 + deltapart[i];
        if (st->singular) { st->done = 1; st->status = KT_DEFORM_SINGULAR; st->last_error = err; return; }   // steps stays at the last one applied
        st->steps = step;
        if (sqrt(d2) < p.delta_tol || err < p.error_tol || fabs(err - st->last_error) < p.change_tol * err) { st->done = 1; st->status = KT_DEFORM_CONVERGED; }
        else if (step == p.max_steps) { st->done = 1; st->status = KT_DEFORM_MAX_STEPS; }
    }
    st->last_error = err;
}

// ---- per-node constraint lists in constraint order: entry = 4 l + slot.  One lane per node walks the constraints twice (count, fill) ----
__device__ __forceinline__ int df_slot_of(const int4 v, int j) { return v.x == j ? 0 : v.y == j ? 1 : v.z == j ? 2 : v.w == j ? 3 : -1; }

__global__ __launch_bounds__(KT_DF_LANES) void df_list_count(const int4* __restrict__ cidx, int n_con, int M, unsigned int* __restrict__ count)
{
    const int j = blockIdx.x * KT_DF_LANES + threadIdx.x;
    if (j > M) return;
    unsigned int c = 0;
    if (j < M) for (int l = 0; l < n_con; ++l) c += df_slot_of(cidx[l], j) >= 0 ? 1u : 0u;
    count[j] = c;   // count[M] = 0: the scan leaves the total there
}

__global__ __launch_bounds__(KT_DF_LANES) void df_list_fill(const int4* __restrict__ cidx, int n_con, int M, const unsigned int* __restrict__ off, unsigned int* __restrict__ list)
{
    const int j = blockIdx.x * KT_DF_LANES + threadIdx.x;
    if (j >= M) return;
    unsigned int pos = off[j];
    for (int l = 0; l < n_con; ++l) {
        const int s = df_slot_of(cidx[l], j);
        if (s >= 0) list[pos++] = 4u * (unsigned int)l + (unsigned int)s;
    }
}

// a node's columns of one E_reg row triple it owns: v = sqrt(wReg) [e; 1], e = g_n - g_j
__device__ __forceinline__ double df_vreg(const double* gj, const double* gn, int a) { return a < 3 ? (gn[a] - gj[a]) * KT_DF_SQ_REG : KT_DF_SQ_REG; }
// a node's columns of one E_con row triple: sqrt(wCon) [w (s - g); w]
__device__ __forceinline__ double df_vcon(const float* s, const double* g, double w, int a) { return a < 3 ? (((double)s[a] - g[a]) * w) * KT_DF_SQ_CON : w * KT_DF_SQ_CON; }

// ---- J^T J: workgroup (d, j) owns block (i = j + d, j), lane (p, q) one entry; unknown p of a node is (a, r) = column a of [A | b], row r,
// and a regularisation or constraint term couples only unknowns of equal r.  d = 20 holds the zeros the factor fills in ----
__global__ __launch_bounds__(144) void df_assemble(const kt_df_state* __restrict__ st, const double* __restrict__ x, const double* __restrict__ gd,
                                                   const int* __restrict__ nb, int M, const float* __restrict__ csrc, const int* __restrict__ cidx,
                                                   const double* __restrict__ cw, const unsigned int* __restrict__ off, const unsigned int* __restrict__ list,
                                                   double* __restrict__ Hb, double* __restrict__ diag0)
{
    if (st->done) return;
    const int d = blockIdx.x, j = blockIdx.y, i = j + d, p = threadIdx.x / 12, q = threadIdx.x % 12;
    const int band = 12 * d + p - q;
    if (i >= M || band < 0 || band >= KT_DF_BAND) return;
    const int ap = p < 9 ? p / 3 : 3, rp = p < 9 ? p % 3 : p - 9, aq = q < 9 ? q / 3 : 3, rq = q < 9 ? q % 3 : q - 9;
    double val = 0.0;
    if (d == 0 && p < 9 && q < 9) {
        const double* A = x + 12 * (size_t)j;
        for (int row = 0; row < 6; ++row) val = val + df_jrot(A, row, p) * df_jrot(A, row, q);
    }
    if (rp == rq && d < KT_DF_LOOKBACK) {
        const double *gi = gd + 4 * (size_t)i, *gj = gd + 4 * (size_t)j;
        if (d == 0) {
            for (int m = max(0, j - 4); m <= min(M - 1, j + 4); ++m)
                for (int k = 0; k < 4; ++k) {
                    const int n = nb[4 * m + k];
                    if (m == j) { const double* gn = gd + 4 * (size_t)n; val = val + df_vreg(gj, gn, ap) * df_vreg(gj, gn, aq); }
                    else if (n == j && ap == 3 && aq == 3) val = val + (-KT_DF_SQ_REG) * (-KT_DF_SQ_REG);
                }
        } else if (d <= 4) {
            for (int k = 0; k < 4; ++k)
                if (nb[4 * j + k] == i && ap == 3) val = val + (-KT_DF_SQ_REG) * df_vreg(gj, gi, aq);
            for (int k = 0; k < 4; ++k)
                if (nb[4 * i + k] == j && aq == 3) val = val + df_vreg(gi, gj, ap) * (-KT_DF_SQ_REG);
        }
        for (unsigned int e = off[j]; e < off[j + 1]; ++e) {
            const unsigned int l = list[e] >> 2, sj = list[e] & 3u;
            int si = (int)sj;
            if (d != 0) si = df_slot_of(reinterpret_cast<const int4*>(cidx)[l], i);
            if (si < 0) continue;
            const float* s = csrc + 3 * (size_t)l;
            val = val + df_vcon(s, gi, cw[4 * (size_t)l + si], ap) * df_vcon(s, gj, cw[4 * (size_t)l + sj], aq);
        }
    }
    Hb[(size_t)(12 * j + q) * KT_DF_BAND + band] = val;
    if (band == 0) diag0[12 * j + q] = val;
}

// ---- the right-hand side -J^T r: one lane per unknown ----
__global__ __launch_bounds__(KT_DF_LANES) void df_gradient(const kt_df_state* __restrict__ st, const double* __restrict__ x, const double* __restrict__ gd,
                                                           const int* __restrict__ nb, int M, const float* __restrict__ csrc, const double* __restrict__ cw,
                                                           const unsigned int* __restrict__ off, const unsigned int* __restrict__ list,
                                                           const double* __restrict__ rrot, const double* __restrict__ rreg, const double* __restrict__ rcon,
                                                           double* __restrict__ rhs)
{
    if (st->done) return;
    const int u = blockIdx.x * KT_DF_LANES + threadIdx.x;
    if (u >= 12 * M) return;
    const int j = u / 12, p = u % 12, ap = p < 9 ? p / 3 : 3, rp = p < 9 ? p % 3 : p - 9;
    const double* gj = gd + 4 * (size_t)j;
    double val = 0.0;
    if (p < 9) {
        const double* A = x + 12 * (size_t)j;
        for (int row = 0; row < 6; ++row) val = val + df_jrot(A, row, p) * rrot[6 * (size_t)j + row];
    }
    for (int m = max(0, j - 4); m <= min(M - 1, j + 4); ++m)
        for (int k = 0; k < 4; ++k) {
            const int n = nb[4 * m + k];
            const double res = rreg[3 * (size_t)(4 * m + k) + rp];
            if (m == j) val = val + df_vreg(gj, gd + 4 * (size_t)n, ap) * res;
            else if (n == j && ap == 3) val = val + (-KT_DF_SQ_REG) * res;
        }
    for (unsigned int e = off[j]; e < off[j + 1]; ++e) {
        const unsigned int l = list[e] >> 2, sj = list[e] & 3u;
        val = val + df_vcon(csrc + 3 * (size_t)l, gj, cw[4 * (size_t)l + sj], ap) * rcon[3 * (size_t)l + rp];
    }
    rhs[u] = -val;
}

// ---- H delta = rhs by a right-looking banded L D L^T in ONE workgroup, the forward substitution riding along; then the diagonal and
// the backward substitution.  Hb[col * 240 + r] = H(col + r, col); y = rhs on entry, delta on exit.  A pivot that is not finite or not
// above 1e-12 of the diagonal entry it started from marks the system singular (a straight line of nodes, fewer than three constraints out
// of line: in exact arithmetic the pivot is 0, computed it is rounding noise of either sign, 1e-16 of the entry); the factorisation still
// runs to its end, df_update then leaves the state alone and df_tally ends the call with KT_DEFORM_SINGULAR.  At 1e-12 twelve of a double's
// sixteen digits are gone: a delta from such a system says nothing at the 1e-9 the stage is held to ----
__global__ __launch_bounds__(KT_DF_SOLVE_LANES) void df_solve(kt_df_state* __restrict__ st, double* __restrict__ Hb, double* __restrict__ y, int n,
                                                              const double* __restrict__ diag0)
{
    __shared__ double sh_a[KT_DF_BAND], sh_l[KT_DF_BAND];
    if (st->done) return;
    const int t = threadIdx.x, ty = t >> 5, tx = t & 31;
    for (int j = 0; j < n; ++j) {
        const int w = min(KT_DF_BAND - 1, n - 1 - j);
        double* col = Hb + (size_t)j * KT_DF_BAND;
        if (t == 0) {
            const double dj = col[0];
            if (!(dj > KT_DF_PIVOT_MIN * diag0[j] && dj < __builtin_inf())) st->singular = 1;
        }
        if (t >= 1 && t <= w) {
            const double a = col[t], lc = a / col[0];
            sh_a[t] = a; sh_l[t] = lc;
            col[t] = lc;
            y[j + t] = y[j + t] - lc * y[j];
        }
        __syncthreads();
        for (int c = 1 + ty; c <= w; c += 32) {
            const double ac = sh_a[c];
            double* cc = Hb + (size_t)(j + c) * KT_DF_BAND - c;   // cc[r] = H(j + r, j + c), c <= r <= w: inside column j + c's 240 slots
            for (int r = c + tx; r <= w; r += 32) cc[r] = cc[r] - sh_l[r] * ac;
        }
        __syncthreads();
    }
    for (int i = t; i < n; i += KT_DF_SOLVE_LANES) y[i] = y[i] / Hb[(size_t)i * KT_DF_BAND];
    __syncthreads();
    for (int j = n - 1; j >= 1; --j) {
        const int i = max(0, j - (KT_DF_BAND - 1)) + t;
        if (i < j) y[i] = y[i] - Hb[(size_t)i * KT_DF_BAND + (j - i)] * y[j];
        __syncthreads();
    }
}

// ---- x <- x + delta and the workgroup's share of |delta|^2 ----
__global__ __launch_bounds__(KT_DF_LANES) void df_update(const kt_df_state* __restrict__ st, double* __restrict__ x, const double* __restrict__ delta, int n,
                                                         double* __restrict__ part)
{
    __shared__ double wave_sh[KT_DF_LANES / 64];
    if (st->done) return;
    const int u = blockIdx.x * KT_DF_LANES + threadIdx.x;
    double sq = 0.0;
    if (u < n && !st->singular) { const double dl = delta[u]; x[u] = x[u] + dl; sq = dl * dl; }
    df_block_fold(sq, wave_sh, part + blockIdx.x);
}

__global__ __launch_bounds__(KT_DF_LANES) void df_identity(double* __restrict__ x, int n)
{
    const int u = blockIdx.x * KT_DF_LANES + threadIdx.x;
    if (u < n) { const int p = u % 12; x[u] = (p == 0 || p == 4 || p == 8) ? 1.0 : 0.0; }
}

// ---- the download: the state, then {error_start, error_end, constraint_error, steps, status} ----
__global__ __launch_bounds__(KT_DF_LANES) void df_export(const kt_df_state* __restrict__ st, const double* __restrict__ x, int n, double* __restrict__ out)
{
    const int u = blockIdx.x * KT_DF_LANES + threadIdx.x;
    if (u < n) out[u] = x[u];
    if (u == 0) {
        double* r = out + n;
        r[0] = st->error_start; r[1] = st->error_end; r[2] = st->constraint_error; r[3] = (double)st->steps; r[4] = (double)st->status;
    }
}

// ---- A^-T of every node, row-major: the cofactors and one division ----
__global__ __launch_bounds__(KT_DF_LANES) void df_normal_mats(const double* __restrict__ x, int M, double* __restrict__ Nm)
{
    const int j = blockIdx.x * KT_DF_LANES + threadIdx.x;
    if (j >= M) return;
    const double* A = x + 12 * (size_t)j;   // A(r, c) = A[3 c + r]
    const double a00 = A[0], a10 = A[1], a20 = A[2], a01 = A[3], a11 = A[4], a21 = A[5], a02 = A[6], a12 = A[7], a22 = A[8];
    double c[9];
    c[0] = a11 * a22 - a12 * a21; c[1] = a12 * a20 - a10 * a22; c[2] = a10 * a21 - a11 * a20;
    c[3] = a02 * a21 - a01 * a22; c[4] = a00 * a22 - a02 * a20; c[5] = a01 * a20 - a00 * a21;
    c[6] = a01 * a12 - a02 * a11; c[7] = a02 * a10 - a00 * a12; c[8] = a00 * a11 - a01 * a10;
    const double det = (a00 * c[0] + a01 * c[1]) + a02 * c[2], inv = 1.0 / det;
    for (int e = 0; e < 9; ++e) Nm[9 * (size_t)j + e] = c[e] * inv;
}

// ---- applyGraphToVertices: one lane per 48-byte point, the position and the normal read and written as 16-byte words ----
__global__ __launch_bounds__(KT_DF_LANES) void df_apply(float4* __restrict__ pts, const int* __restrict__ idx, const double* __restrict__ w, size_t n,
                                                        const double* __restrict__ x, const double* __restrict__ gd, const double* __restrict__ Nm)
{
    const size_t i = (size_t)blockIdx.x * KT_DF_LANES + threadIdx.x;
    if (i >= n) return;
    float4 q0 = pts[3 * i], q1 = pts[3 * i + 1];
    const int4 iv = reinterpret_cast<const int4*>(idx)[i];
    const double2 w01 = reinterpret_cast<const double2*>(w)[2 * i], w23 = reinterpret_cast<const double2*>(w)[2 * i + 1];
    const int id[4] = {iv.x, iv.y, iv.z, iv.w};
    const double ws[4] = {w01.x, w01.y, w23.x, w23.y};
    const double p[3] = {(double)q0.x, (double)q0.y, (double)q0.z}, nn[3] = {(double)q1.x, (double)q1.y, (double)q1.z};
    double o[3], m[3] = {0.0, 0.0, 0.0};
    df_position(p, id, ws, x, gd, 0, o);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const double* N = Nm + 9 * (size_t)id[s];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double t = (N[3 * r] * nn[0] + N[3 * r + 1] * nn[1]) + N[3 * r + 2] * nn[2];
            m[r] = m[r] + ws[s] * t;
        }
    }
    const double len = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    q0.x = (float)o[0]; q0.y = (float)o[1]; q0.z = (float)o[2];
    pts[3 * i] = q0;
    if (len > 0.0 && len < __builtin_inf()) {   // zero or not finite: the old normal stays
        q1.x = (float)(m[0] / len); q1.y = (float)(m[1] / len); q1.z = (float)(m[2] / len);
        pts[3 * i + 1] = q1;
    }
}

// ---- the -m mesh: 16-byte kt_mesh_vertex records in spans of one time each (a slab's vertices carry its slice's time), weights and
// position in ONE launch.  A workgroup works on at most KT_DF_LANES consecutive vertices of ONE span: it finds the span from its index in
// the prefix of per-span workgroup counts (empty spans have none), runs the time search once, copies the window's nodes -- float and
// widened positions, 12 doubles of state: 2880 bytes -- to LDS, and after one barrier every lane runs df_weigh_window and df_position on
// that copy.  The vertex is read and written as one 16-byte word; the rgb word passes through as an integer ----
__global__ __launch_bounds__(KT_DF_LANES) void df_apply_mesh(uint4* __restrict__ v, const unsigned int* __restrict__ sfirst, const unsigned int* __restrict__ spref,
                                                             const unsigned long long* __restrict__ stime, int n_spans, const float4* __restrict__ gf,
                                                             const double* __restrict__ gd, const unsigned long long* __restrict__ gt, int M,
                                                             const double* __restrict__ x)
{
    __shared__ float4 sh_gf[KT_DF_LOOKBACK];
    __shared__ double sh_gd[4 * KT_DF_LOOKBACK], sh_x[12 * KT_DF_LOOKBACK];
    const unsigned int b = blockIdx.x;
    int lo = 0, hi = n_spans - 1;
    while (lo < hi) {   // the first span whose workgroups end after b
        const int mid = (lo + hi) >> 1;
        if (spref[mid + 1] > b) hi = mid; else lo = mid + 1;
    }
    int first, last;
    df_window(stime[lo], gt, M, &first, &last);
    const int t = threadIdx.x, W = last - first + 1;
    if (t < W) sh_gf[t] = gf[first + t];
    if (t < 4 * W) sh_gd[t] = gd[4 * (size_t)first + t];
    if (t < 12 * W) sh_x[t] = x[12 * (size_t)first + t];
    __syncthreads();
    const unsigned int i = sfirst[lo] + (b - spref[lo]) * KT_DF_LANES + t;   // below 2^29 + KT_DF_LANES
    if (i >= sfirst[lo + 1]) return;
    uint4 q = v[i];
    const float px = __uint_as_float(q.x), py = __uint_as_float(q.y), pz = __uint_as_float(q.z);
    int id[4];
    double ws[4], o[3];
    df_weigh_window(px, py, pz, first, last, sh_gf, sh_gd, first, id, ws);
    const double p[3] = {(double)px, (double)py, (double)pz};
    df_position(p, id, ws, sh_x, sh_gd, first, o);
    q.x = __float_as_uint((float)o[0]); q.y = __float_as_uint((float)o[1]); q.z = __float_as_uint((float)o[2]);
    v[i] = q;
}

}  // namespace

struct kt_deform {
    kt_mem mem, pts_mem;             // pts_mem: the staging of kt_deform_apply alone, the group that grows
    kt_ctx* ctx;
    hipStream_t stream;
    int max_nodes, max_constraints, M;
    kt_df_state* state;
    float4* gf;                      // device, max_nodes: the nodes' float positions
    double* gd;                      // device, max_nodes x 4: the same, widened
    unsigned long long* gt;          // device, max_nodes
    int* nb;                         // device, max_nodes x 4
    double *x, *rrot, *rreg, *rhs, *diag0, *Nm, *Hb;   // device, per node: 12, 6, 12, 12, 12, 9, 12 x 240
    double *nodepart, *deltapart, *conpart;    // device, per workgroup of 256 nodes / unknowns / constraints
    unsigned int *off, *list;        // device, max_nodes + 1 and 4 x max_constraints
    float* csrc;                     // device, per constraint: 3
    unsigned long long* ctime;
    int* cidx;                       // 4
    double *cw, *ctgt, *rcon;        // 4, 3, 3
    double* out;                     // device, max_nodes x 12 + 8
    float* gf_host;                  // pinned, max_nodes x 4
    double* gd_host;                 // pinned, max_nodes x 4
    int* nb_host;                    // pinned, max_nodes x 4
    double* out_host;                // pinned, max_nodes x 12 + 8
    size_t pts_cap;
    float4* pts; unsigned long long* ptimes; int* pidx; double* pw;   // device, pts_cap points
    kt_mem mesh_mem;                 // of kt_deform_apply_mesh[_device]: the span table and the host form's vertex staging, the second group that grows
    size_t mv_cap, sp_cap;           // vertices; spans
    uint4* mv;                       // device, mv_cap vertices
    unsigned int *sp_dev, *sp_host;  // device and pinned, 4 sp_cap + 2 words.  A table of S spans: S + 1 first vertices, S + 1 counts of the
                                     // workgroups before a span, then S times as 64-bit words -- packed, so that ONE copy carries it
    hipEvent_t sp_uploaded;          // behind the table's copy: the pinned table is rewritten after it
};

extern "C" int kt_deform_destroy(kt_deform* dg)
{
    if (!dg) return KT_OK;
    if (dg->stream) (void)hipStreamSynchronize(dg->stream);
    dg->pts_mem.release();
    dg->mesh_mem.release();
    dg->mem.release();
    delete dg;
    return KT_OK;
}

extern "C" int kt_deform_create(kt_ctx* c, int max_nodes, int max_constraints, void* hip_stream, kt_deform** out)
{
    KT_ARG(c && out && max_nodes >= 5 && max_nodes <= KT_DF_MAX_NODES && max_constraints >= 0 && max_constraints <= KT_DF_MAX_CONSTRAINTS);
    KT_HIP(hipSetDevice(c->device));
    kt_deform* dg = new kt_deform();   // value-initialised: every pointer starts null
    dg->ctx = c; dg->stream = hip_stream ? (hipStream_t)hip_stream : c->stream; dg->max_nodes = max_nodes; dg->max_constraints = max_constraints;
    const size_t N = (size_t)max_nodes, L = (size_t)max_constraints + 1;
    const size_t NB = (N + KT_DF_LANES - 1) / KT_DF_LANES, UB = (12 * N + KT_DF_LANES - 1) / KT_DF_LANES, LB = (L + KT_DF_LANES - 1) / KT_DF_LANES;
    int s = dg->mem.device(&dg->state, 1);
    if (s == KT_OK) s = dg->mem.device(&dg->gf, N);
    if (s == KT_OK) s = dg->mem.device(&dg->gd, N * 4);
    if (s == KT_OK) s = dg->mem.device(&dg->gt, N);
    if (s == KT_OK) s = dg->mem.device(&dg->nb, N * 4);
    if (s == KT_OK) s = dg->mem.device(&dg->x, N * 12);
    if (s == KT_OK) s = dg->mem.device(&dg->rrot, N * 6);
    if (s == KT_OK) s = dg->mem.device(&dg->rreg, N * 12);
    if (s == KT_OK) s = dg->mem.device(&dg->rhs, N * 12);
    if (s == KT_OK) s = dg->mem.device(&dg->diag0, N * 12);
    if (s == KT_OK) s = dg->mem.device(&dg->Nm, N * 9);
    if (s == KT_OK) s = dg->mem.device(&dg->Hb, N * 12 * KT_DF_BAND);
    if (s == KT_OK) s = dg->mem.device(&dg->nodepart, NB);
    if (s == KT_OK) s = dg->mem.device(&dg->deltapart, UB);
    if (s == KT_OK) s = dg->mem.device(&dg->conpart, LB);
    if (s == KT_OK) s = dg->mem.device(&dg->off, N + 1);
    if (s == KT_OK) s = dg->mem.device(&dg->list, L * 4);
    if (s == KT_OK) s = dg->mem.device(&dg->csrc, L * 3);
    if (s == KT_OK) s = dg->mem.device(&dg->ctime, L);
    if (s == KT_OK) s = dg->mem.device(&dg->cidx, L * 4);
    if (s == KT_OK) s = dg->mem.device(&dg->cw, L * 4);
    if (s == KT_OK) s = dg->mem.device(&dg->ctgt, L * 3);
    if (s == KT_OK) s = dg->mem.device(&dg->rcon, L * 3);
    if (s == KT_OK) s = dg->mem.device(&dg->out, N * 12 + 8);
    if (s == KT_OK) s = dg->mem.pinned(&dg->gf_host, N * 4);
    if (s == KT_OK) s = dg->mem.pinned(&dg->gd_host, N * 4);
    if (s == KT_OK) s = dg->mem.pinned(&dg->nb_host, N * 4);
    if (s == KT_OK) s = dg->mem.pinned(&dg->out_host, N * 12 + 8);
    if (s != KT_OK) { (void)kt_deform_destroy(dg); return s; }
    *out = dg;
    return KT_OK;
}

extern "C" int kt_deform_set_graph(kt_deform* dg, int n_nodes, const float* node_pos, const uint64_t* node_time)
{
    KT_ARG(dg && node_pos && node_time && n_nodes >= 5);
    if (n_nodes > dg->max_nodes) {
        kt_set_error("kt_deform_set_graph: %d nodes, capacity %d", n_nodes, dg->max_nodes);
        return KT_ERR_CAPACITY;
    }
    for (int i = 1; i < n_nodes; ++i) KT_ARG(node_time[i - 1] < node_time[i]);
    const int M = n_nodes;
    hipStream_t st = dg->stream;
    KT_HIP(hipSetDevice(dg->ctx->device));
    KT_HIP(hipStreamSynchronize(st));   // the staging arrays may still feed the copies of the call before
    for (int i = 0; i < M; ++i) {
        for (int a = 0; a < 3; ++a) { dg->gf_host[4 * i + a] = node_pos[3 * i + a]; dg->gd_host[4 * i + a] = (double)node_pos[3 * i + a]; }
        dg->gf_host[4 * i + 3] = 0.0f; dg->gd_host[4 * i + 3] = 0.0;
        // connectGraphSeq, k = 4: i - 1, i + 1, i - 2, i + 2; the first and the last two nodes take the first / last five but themselves
        int* nb = dg->nb_host + 4 * i;
        if (i < 2 || i >= M - 2) {
            const int base = i < 2 ? 0 : M - 5;
            for (int n = base, k = 0; n < base + 5; ++n) if (n != i) nb[k++] = n;
        } else { nb[0] = i - 1; nb[1] = i + 1; nb[2] = i - 2; nb[3] = i + 2; }
    }
    KT_HIP(hipMemcpyAsync(dg->gf, dg->gf_host, (size_t)M * 4 * sizeof(float), hipMemcpyHostToDevice, st));
    KT_HIP(hipMemcpyAsync(dg->gd, dg->gd_host, (size_t)M * 4 * sizeof(double), hipMemcpyHostToDevice, st));
    KT_HIP(hipMemcpyAsync(dg->nb, dg->nb_host, (size_t)M * 4 * sizeof(int), hipMemcpyHostToDevice, st));
    KT_HIP(hipMemcpyAsync(dg->gt, node_time, (size_t)M * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(df_identity, dim3(kt_div_up(12 * M, KT_DF_LANES)), dim3(KT_DF_LANES), 0, st, dg->x, 12 * M);
    KT_LAUNCH_CHECK();
    KT_HIP(hipStreamSynchronize(st));
    dg->M = M;
    return KT_OK;
}

extern "C" int kt_deform_set_state(kt_deform* dg, const double* state)
{
    KT_ARG(dg && state);
    if (dg->M < 5) { kt_set_error("kt_deform_set_state: no graph set"); return KT_ERR_STATE; }
    KT_HIP(hipSetDevice(dg->ctx->device));
    KT_HIP(hipMemcpyAsync(dg->x, state, (size_t)dg->M * 12 * sizeof(double), hipMemcpyHostToDevice, dg->stream));
    KT_HIP(hipStreamSynchronize(dg->stream));
    return KT_OK;
}

// the residuals and the error of the state, then the tally of `step`
static int df_evaluate_enqueue(kt_deform* dg, int n_con, const kt_deform_params& p, int step)
{
    const int M = dg->M, nnp = kt_div_up(M, KT_DF_LANES), ncp = kt_div_up(n_con, KT_DF_LANES), ndp = kt_div_up(12 * M, KT_DF_LANES);
    hipStream_t st = dg->stream;
    hipLaunchKernelGGL(df_nodes_eval, dim3(nnp), dim3(KT_DF_LANES), 0, st, dg->state, dg->x, dg->gd, dg->nb, M, dg->rrot, dg->rreg, dg->nodepart);
    KT_LAUNCH_CHECK();
    if (n_con > 0) {
        hipLaunchKernelGGL(df_cons_eval, dim3(ncp), dim3(KT_DF_LANES), 0, st, dg->state, dg->x, dg->gd, dg->csrc, dg->cidx, dg->cw, dg->ctgt, n_con, dg->rcon, dg->conpart);
        KT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(df_tally, dim3(1), dim3(64), 0, st, dg->state, p, dg->nodepart, nnp, dg->conpart, ncp, dg->deltapart, ndp, n_con, step);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

extern "C" int kt_deform_optimise(kt_deform* dg, int n_con, const float* src_pos, const uint64_t* src_time, const double* target, const kt_deform_params* params,
                                  double* state_out, kt_deform_result* result)
{
    KT_ARG(dg && state_out && result && n_con >= 0 && ((src_pos && src_time && target) || n_con == 0));
    kt_deform_params p = {0.1, 1e-2, 1e-3, 1e-5, 10, 0};   // optimiseGraphSparse's
    if (params) p = *params;
    KT_ARG(p.max_steps >= 0 && p.max_steps <= KT_DF_MAX_STEPS);
    if (dg->M < 5) { kt_set_error("kt_deform_optimise: no graph set"); return KT_ERR_STATE; }
    if (n_con > dg->max_constraints) {
        kt_set_error("kt_deform_optimise: %d constraints, capacity %d", n_con, dg->max_constraints);
        return KT_ERR_CAPACITY;
    }
    const int M = dg->M, n = 12 * M;
    hipStream_t st = dg->stream;
    KT_HIP(hipSetDevice(dg->ctx->device));
    KT_HIP(hipMemsetAsync(dg->state, 0, sizeof(kt_df_state), st));
    hipLaunchKernelGGL(df_identity, dim3(kt_div_up(n, KT_DF_LANES)), dim3(KT_DF_LANES), 0, st, dg->x, n);   // a call does not depend on the one before it
    KT_LAUNCH_CHECK();
    if (n_con > 0) {
        KT_HIP(hipMemcpyAsync(dg->csrc, src_pos, (size_t)n_con * 3 * sizeof(float), hipMemcpyHostToDevice, st));
        KT_HIP(hipMemcpyAsync(dg->ctime, src_time, (size_t)n_con * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        KT_HIP(hipMemcpyAsync(dg->ctgt, target, (size_t)n_con * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(df_weights<false>, dim3(kt_div_up(n_con, KT_DF_LANES)), dim3(KT_DF_LANES), 0, st, dg->csrc, dg->ctime, (size_t)n_con, dg->gf, dg->gd, dg->gt, M,
                           dg->cidx, dg->cw);
        KT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(df_list_count, dim3(kt_div_up(M + 1, KT_DF_LANES)), dim3(KT_DF_LANES), 0, st, reinterpret_cast<const int4*>(dg->cidx), n_con, M, dg->off);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(kt_scan_runs_kernel<1>, dim3(1), dim3(256), 0, st, dg->off, M + 1, (unsigned int*)nullptr);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_list_fill, dim3(kt_div_up(M, KT_DF_LANES)), dim3(KT_DF_LANES), 0, st, reinterpret_cast<const int4*>(dg->cidx), n_con, M, dg->off, dg->list);
    KT_LAUNCH_CHECK();
    KT_TRY(df_evaluate_enqueue(dg, n_con, p, 0));
    if (n_con > 0) {
        for (int step = 1; step <= p.max_steps; ++step) {
            hipLaunchKernelGGL(df_assemble, dim3(KT_DF_LOOKBACK + 1, M), dim3(144), 0, st, dg->state, dg->x, dg->gd, dg->nb, M, dg->csrc, dg->cidx, dg->cw, dg->off, dg->list,
                               dg->Hb, dg->diag0);
            KT_LAUNCH_CHECK();
            hipLaunchKernelGGL(df_gradient, dim3(kt_div_up(n, KT_DF_LANES)), dim3(KT_DF_LANES), 0, st, dg->state, dg->x, dg->gd, dg->nb, M, dg->csrc, dg->cw, dg->off,
                               dg->list, dg->rrot, dg->rreg, dg->rcon, dg->rhs);
            KT_LAUNCH_CHECK();
            hipLaunchKernelGGL(df_solve, dim3(1), dim3(KT_DF_SOLVE_LANES), 0, st, dg->state, dg->Hb, dg->rhs, n, dg->diag0);
            KT_LAUNCH_CHECK();
            hipLaunchKernelGGL(df_update, dim3(kt_div_up(n, KT_DF_LANES)), dim3(KT_DF_LANES), 0, st, dg->state, dg->x, dg->rhs, n, dg->deltapart);
            KT_LAUNCH_CHECK();
            KT_TRY(df_evaluate_enqueue(dg, n_con, p, step));
        }
    }
    hipLaunchKernelGGL(df_export, dim3(kt_div_up(n, KT_DF_LANES)), dim3(KT_DF_LANES), 0, st, dg->state, dg->x, n, dg->out);
    KT_LAUNCH_CHECK();
    KT_HIP(hipMemcpyAsync(dg->out_host, dg->out, ((size_t)n + 8) * sizeof(double), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    memcpy(state_out, dg->out_host, (size_t)n * sizeof(double));
    const double* r = dg->out_host + n;
    result->error_start = r[0]; result->error_end = r[1]; result->constraint_error = r[2]; result->steps = (int)r[3]; result->status = (int)r[4];
    return KT_OK;
}

extern "C" int kt_deform_weights_device(kt_deform* dg, const kt_point_xyzrgbnormal* points_dev, const uint64_t* times_dev, size_t n, int32_t* idx_dev, double* w_dev)
{
    KT_ARG(dg && n <= 0x7fffffffu && ((points_dev && times_dev && idx_dev && w_dev) || n == 0));
    KT_ARG(((uintptr_t)points_dev & 15) == 0 && ((uintptr_t)idx_dev & 15) == 0 && ((uintptr_t)w_dev & 15) == 0);
    if (dg->M < 5) { kt_set_error("kt_deform_weights_device: no graph set"); return KT_ERR_STATE; }
    if (n == 0) return KT_OK;
    KT_HIP(hipSetDevice(dg->ctx->device));
    hipLaunchKernelGGL(df_weights<true>, dim3((unsigned int)((n + KT_DF_LANES - 1) / KT_DF_LANES)), dim3(KT_DF_LANES), 0, dg->stream,
                       reinterpret_cast<const float*>(points_dev), reinterpret_cast<const unsigned long long*>(times_dev), n, dg->gf, dg->gd, dg->gt, dg->M, idx_dev, w_dev);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

extern "C" int kt_deform_apply_device(kt_deform* dg, kt_point_xyzrgbnormal* points_dev, const int32_t* idx_dev, const double* w_dev, size_t n)
{
    KT_ARG(dg && n <= 0x7fffffffu && ((points_dev && idx_dev && w_dev) || n == 0));
    KT_ARG(((uintptr_t)points_dev & 15) == 0 && ((uintptr_t)idx_dev & 15) == 0 && ((uintptr_t)w_dev & 15) == 0);
    if (dg->M < 5) { kt_set_error("kt_deform_apply_device: no graph set"); return KT_ERR_STATE; }
    if (n == 0) return KT_OK;
    KT_HIP(hipSetDevice(dg->ctx->device));
    hipLaunchKernelGGL(df_normal_mats, dim3(kt_div_up(dg->M, KT_DF_LANES)), dim3(KT_DF_LANES), 0, dg->stream, dg->x, dg->M, dg->Nm);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_apply, dim3((unsigned int)((n + KT_DF_LANES - 1) / KT_DF_LANES)), dim3(KT_DF_LANES), 0, dg->stream, reinterpret_cast<float4*>(points_dev), idx_dev,
                       w_dev, n, dg->x, dg->gd, dg->Nm);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

extern "C" int kt_deform_apply(kt_deform* dg, kt_point_xyzrgbnormal* points, const uint64_t* times, size_t n)
{
    KT_ARG(dg && n <= 0x7fffffffu && ((points && times) || n == 0));
    if (dg->M < 5) { kt_set_error("kt_deform_apply: no graph set"); return KT_ERR_STATE; }
    if (n == 0) return KT_OK;
    hipStream_t st = dg->stream;
    KT_HIP(hipSetDevice(dg->ctx->device));
    if (n > dg->pts_cap) {   // grow: drain, release, allocate at the larger capacity
        KT_HIP(hipStreamSynchronize(st));
        dg->pts_mem.release();
        dg->pts_cap = 0; dg->pts = nullptr; dg->ptimes = nullptr; dg->pidx = nullptr; dg->pw = nullptr;
        int s = dg->pts_mem.device(&dg->pts, n * 3);
        if (s == KT_OK) s = dg->pts_mem.device(&dg->ptimes, n);
        if (s == KT_OK) s = dg->pts_mem.device(&dg->pidx, n * 4);
        if (s == KT_OK) s = dg->pts_mem.device(&dg->pw, n * 4);
        if (s != KT_OK) { dg->pts_mem.release(); dg->pts = nullptr; dg->ptimes = nullptr; dg->pidx = nullptr; dg->pw = nullptr; return s; }
        dg->pts_cap = n;
    }
    KT_HIP(hipMemcpyAsync(dg->pts, points, n * sizeof(kt_point_xyzrgbnormal), hipMemcpyHostToDevice, st));
    KT_HIP(hipMemcpyAsync(dg->ptimes, times, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    KT_TRY(kt_deform_weights_device(dg, reinterpret_cast<const kt_point_xyzrgbnormal*>(dg->pts), reinterpret_cast<const uint64_t*>(dg->ptimes), n, dg->pidx, dg->pw));
    KT_TRY(kt_deform_apply_device(dg, reinterpret_cast<kt_point_xyzrgbnormal*>(dg->pts), dg->pidx, dg->pw, n));
    KT_HIP(hipMemcpyAsync(points, dg->pts, n * sizeof(kt_point_xyzrgbnormal), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    return KT_OK;
}

// the span table for n_spans spans and the staging for n_vertices vertices: grow by drain, release, allocate at the larger capacities
static int df_mesh_reserve(kt_deform* dg, size_t n_vertices, size_t n_spans)
{
    if (n_vertices <= dg->mv_cap && n_spans <= dg->sp_cap && dg->sp_host) return KT_OK;
    const size_t vc = n_vertices > dg->mv_cap ? n_vertices : dg->mv_cap, sc = n_spans > dg->sp_cap ? n_spans : dg->sp_cap;
    KT_HIP(hipStreamSynchronize(dg->stream));
    dg->mesh_mem.release();
    dg->mv_cap = dg->sp_cap = 0; dg->mv = nullptr; dg->sp_dev = dg->sp_host = nullptr; dg->sp_uploaded = nullptr;
    int s = vc ? dg->mesh_mem.device(&dg->mv, vc) : KT_OK;
    if (s == KT_OK) s = dg->mesh_mem.device(&dg->sp_dev, 4 * sc + 2);
    if (s == KT_OK) s = dg->mesh_mem.pinned(&dg->sp_host, 4 * sc + 2);
    if (s == KT_OK) s = dg->mesh_mem.event(&dg->sp_uploaded, hipEventDisableTiming);
    if (s == KT_OK) s = kt_check(hipEventRecord(dg->sp_uploaded, dg->stream), "hipEventRecord", __FILE__, __LINE__);
    if (s != KT_OK) {
        dg->mesh_mem.release();
        dg->mv = nullptr; dg->sp_dev = dg->sp_host = nullptr; dg->sp_uploaded = nullptr;
        return s;
    }
    dg->mv_cap = vc; dg->sp_cap = sc;
    return KT_OK;
}

// arguments first (KT_ERR_ARG, nothing written), then the graph (KT_ERR_STATE)
static int df_mesh_check(const kt_deform* dg, const void* vertices, size_t n, const size_t* span_first, const uint64_t* span_time, int n_spans, const char* who)
{
    KT_ARG(dg && n <= ((size_t)1 << 29) && n_spans >= 0 && (n == 0 || n_spans > 0));
    KT_ARG((vertices && ((uintptr_t)vertices & 15) == 0) || n == 0);
    KT_ARG((span_first && span_time) || n_spans == 0);
    if (n_spans > 0) {
        KT_ARG(span_first[0] == 0 && span_first[n_spans] == n);
        for (int s = 0; s < n_spans; ++s) KT_ARG(span_first[s] <= span_first[s + 1]);
    }
    if (dg->M < 5) { kt_set_error("%s: no graph set", who); return KT_ERR_STATE; }
    return KT_OK;
}

// the table to the device and the launch; vertices_dev holds n checked vertices, n > 0
static int df_mesh_enqueue(kt_deform* dg, uint4* vertices_dev, const size_t* span_first, const uint64_t* span_time, int n_spans)
{
    const size_t S = (size_t)n_spans;
    hipStream_t st = dg->stream;
    KT_HIP(hipEventSynchronize(dg->sp_uploaded));   // the pinned table may still feed the copy of the call before
    unsigned int *hf = dg->sp_host, *hp = hf + (S + 1);
    unsigned long long* ht = reinterpret_cast<unsigned long long*>(hp + (S + 1));   // 2 (S + 1) words in: 8-byte aligned
    unsigned int groups = 0;
    for (size_t s = 0; s < S; ++s) {
        hf[s] = (unsigned int)span_first[s]; hp[s] = groups; ht[s] = span_time[s];
        groups += (unsigned int)((span_first[s + 1] - span_first[s] + KT_DF_LANES - 1) / KT_DF_LANES);
    }
    hf[S] = (unsigned int)span_first[S]; hp[S] = groups;
    KT_HIP(hipMemcpyAsync(dg->sp_dev, hf, (4 * S + 2) * sizeof(unsigned int), hipMemcpyHostToDevice, st));
    KT_HIP(hipEventRecord(dg->sp_uploaded, st));
    const unsigned int* df = dg->sp_dev;
    hipLaunchKernelGGL(df_apply_mesh, dim3(groups), dim3(KT_DF_LANES), 0, st, vertices_dev, df, df + (S + 1), reinterpret_cast<const unsigned long long*>(df + 2 * (S + 1)), n_spans,
                       dg->gf, dg->gd, dg->gt, dg->M, dg->x);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

extern "C" int kt_deform_apply_mesh_device(kt_deform* dg, kt_mesh_vertex* vertices_dev, size_t n, const size_t* span_first, const uint64_t* span_time, int n_spans)
{
    static_assert(sizeof(kt_mesh_vertex) == sizeof(uint4), "vertex layout");
    KT_TRY(df_mesh_check(dg, vertices_dev, n, span_first, span_time, n_spans, "kt_deform_apply_mesh_device"));
    if (n == 0) return KT_OK;
    KT_HIP(hipSetDevice(dg->ctx->device));
    KT_TRY(df_mesh_reserve(dg, 0, (size_t)n_spans));
    return df_mesh_enqueue(dg, reinterpret_cast<uint4*>(vertices_dev), span_first, span_time, n_spans);
}

extern "C" int kt_deform_apply_mesh(kt_deform* dg, kt_mesh_vertex* vertices, size_t n, const size_t* span_first, const uint64_t* span_time, int n_spans)
{
    KT_TRY(df_mesh_check(dg, vertices, n, span_first, span_time, n_spans, "kt_deform_apply_mesh"));
    if (n == 0) return KT_OK;
    KT_HIP(hipSetDevice(dg->ctx->device));
    KT_TRY(df_mesh_reserve(dg, n, (size_t)n_spans));
    KT_HIP(hipMemcpyAsync(dg->mv, vertices, n * sizeof(kt_mesh_vertex), hipMemcpyHostToDevice, dg->stream));
    KT_TRY(df_mesh_enqueue(dg, dg->mv, span_first, span_time, n_spans));
    KT_HIP(hipMemcpyAsync(vertices, dg->mv, n * sizeof(kt_mesh_vertex), hipMemcpyDeviceToHost, dg->stream));
    KT_HIP(hipStreamSynchronize(dg->stream));
    return KT_OK;
}
