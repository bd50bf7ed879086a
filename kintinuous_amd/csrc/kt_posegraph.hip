// kt_posegraph.hip -- the consumer of the accepted loop constraints: the dense pose graph that the reference keeps in iSAM
// (backend/iSAMInterface.cpp, driven by Deformation::addCameraCamera / addCameraLoop, backend/Deformation.cpp:130-346) and re-solves with
// batch_optimization() after every accepted loop.  NOT a port of iSAM: a defined stage with its role, inputs, outputs and acceptance rule
// (include/kt_abi.h and DESIGN.md 4.10 state it; kintinuous_amd/pose_graph_ref.py restates it in the same operation order).  No Euler-angle
// Pose3d, no basis change, no QR: the graph is a chain plus at most 64 loop edges, and Gauss-Newton uses that shape.
//   unknowns   the increments D_k = T_{k-1}^-1 T_k, updated as D_k <- D_k Exp(delta_k), Exp([v; w]) = [Exp_SO3(w) | v].  The chain's part
//              of the normal matrix is then block diagonal (H_k = J_k^T J_k, 6x6), the loops add A^T A with A of 6L rows, and
//              delta = u - H^-1 A^T S^-1 A u with u = H^-1 b, S = I + A H^-1 A^T (6L x 6L).
//   A          A_lk = Jr(E_l) Ad(T_j^-1 T_k) for i < k <= j.  Ad is a homomorphism, so A_lk = B_l Ad(T_k) with B_l = Jr(E_l) Ad(T_j^-1): one 6x6
//              per loop and one adjoint per node rebuild every block, and A_lk H_k^-1 A_mk^T = B_l G_k B_m^T with G_k = Ad(T_k) H_k^-1 Ad(T_k)^T.
//   a step     compose (scan of SE(3) products: pg_scan_local, pg_scan_carry, pg_scan_apply), pg_loops, pg_nodes, pg_tally (the cost), then
//              pg_pairs (S and v: one workgroup per pair of loops sums G_k over the intersection of their spans), pg_solve (dense LDLT in one
//              workgroup), pg_update.  All 20 steps are enqueued at once; every kernel returns at once when the state's `done` word is set.
// Everything is double, uncontracted, in a fixed order: no floating-point atomics (max |delta| goes through an integer atomicMax on the bits
// of a non-negative double), so a call returns the same bytes every time.
#include "kt_internal.hpp"
#include "kt_wave.hpp"

#include <math.h>
#include <string.h>

#define KT_PG_LANES 256
#define KT_PG_MAX_LOOPS 64
#define KT_PG_MAX_NODES (1 << 22)
#define KT_PG_MAX_STEPS 20
#define KT_PG_DELTA_TOL 1e-9
#define KT_PG_CHI2_SCALE 1000.0   // every factor of the reference has covariance 1e-3 I

struct kt_pg_state {
    double chi2_start, chi2_end;
    unsigned long long maxdelta_bits;   // the bits of max |delta|_inf of the step in flight
    int steps, status, done, pad;
};

// ---- SE(3) as 12 doubles {R row-major, t}; sums over the inner index in ascending order ----
__host__ __device__ inline void pg_mul(const double* a, const double* b, double* o)
{
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
        o[9 + i] = ((a[3 * i] * b[9] + a[3 * i + 1] * b[10]) + a[3 * i + 2] * b[11]) + a[9 + i];
    }
}
__host__ __device__ inline void pg_inv(const double* a, double* o)
{
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * j + i];
        o[9 + i] = -((a[i] * a[9] + a[3 + i] * a[10]) + a[6 + i] * a[11]);
    }
}
__host__ __device__ inline void pg_identity(double* o)
{
    for (int i = 0; i < 12; ++i) o[i] = 0.0;
    o[0] = o[4] = o[8] = 1.0;
}
__host__ __device__ inline void pg_from16(const double* m, double* o)
{
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o[3 * i + j] = m[4 * i + j];
        o[9 + i] = m[4 * i + 3];
    }
}

namespace {

template <int N, int P, int M>
__device__ __forceinline__ void pg_mm(const double* A, const double* B, double* O)   // (N x P)(P x M)
{
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < M; ++j) {
            double acc = A[i * P] * B[j];
            for (int c = 1; c < P; ++c) acc = acc + A[i * P + c] * B[c * M + j];
            O[i * M + j] = acc;
        }
}
template <int N, int P>
__device__ __forceinline__ void pg_mv(const double* A, const double* x, double* o)
{
    for (int i = 0; i < N; ++i) {
        double acc = A[i * P] * x[0];
        for (int c = 1; c < P; ++c) acc = acc + A[i * P + c] * x[c];
        o[i] = acc;
    }
}
template <int N, int P>
__device__ __forceinline__ void pg_mtv(const double* A, const double* x, double* o)   // A^T x, A (N x P)
{
    for (int i = 0; i < P; ++i) {
        double acc = A[i] * x[0];
        for (int c = 1; c < N; ++c) acc = acc + A[c * P + i] * x[c];
        o[i] = acc;
    }
}
__device__ __forceinline__ void pg_hat(const double* w, double* K)
{
    K[0] = 0.0; K[1] = -w[2]; K[2] = w[1];
    K[3] = w[2]; K[4] = 0.0; K[5] = -w[0];
    K[6] = -w[1]; K[7] = w[0]; K[8] = 0.0;
}
// I + a K + b K^2
__device__ __forceinline__ void pg_poly(const double* K, double a, double b, double* R)
{
    double K2[9];
    pg_mm<3, 3, 3>(K, K, K2);
    for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + a * K[i]) + b * K2[i];
}
__device__ __forceinline__ void pg_so3_exp(const double* w, double* R)
{
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = sqrt(th2);
    double A, B;
    if (th < 1e-4) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; }
    else { A = sin(th) / th; B = (1.0 - cos(th)) / (th * th); }
    double K[9];
    pg_hat(w, K);
    pg_poly(K, A, B, R);
}
// the rotation vector for angles away from pi (the residuals of a graph worth optimising are small)
__device__ __forceinline__ void pg_so3_log(const double* R, double* phi)
{
    const double a[3] = {(R[7] - R[5]) * 0.5, (R[2] - R[6]) * 0.5, (R[3] - R[1]) * 0.5};
    const double s = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    const double c = (((R[0] + R[4]) + R[8]) - 1.0) * 0.5;
    const double f = s < 1e-5 ? 1.0 + s * s / 6.0 : atan2(s, c) / s;
    for (int i = 0; i < 3; ++i) phi[i] = a[i] * f;
}
__device__ __forceinline__ void pg_so3_jr_inv(const double* phi, double* J)
{
    const double th2 = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2], th = sqrt(th2);
    double c2;
    if (th < 1e-2) c2 = (1.0 / 12.0 + th2 / 720.0) + th2 * th2 / 30240.0;
    else c2 = 1.0 / (th * th) - (1.0 + cos(th)) / ((2.0 * th) * sin(th));
    double K[9];
    pg_hat(phi, K);
    pg_poly(K, 0.5, c2, J);
}
// r = [trans(E); Log_SO3(rot(E))] and Jr(E) = [[R_E, 0], [0, Jr_SO3^-1(phi)]]
__device__ __forceinline__ void pg_residual(const double* E, double* r, double* J)
{
    r[0] = E[9]; r[1] = E[10]; r[2] = E[11];
    pg_so3_log(E, r + 3);
    double Ji[9];
    pg_so3_jr_inv(r + 3, Ji);
    for (int i = 0; i < 36; ++i) J[i] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { J[6 * i + j] = E[3 * i + j]; J[6 * (i + 3) + j + 3] = Ji[3 * i + j]; }
}
// Ad(P) on [v; w]: [[R, [t]x R], [0, R]]
__device__ __forceinline__ void pg_adjoint(const double* P, double* A)
{
    double K[9], KR[9];
    pg_hat(P + 9, K);
    pg_mm<3, 3, 3>(K, P, KR);
    for (int i = 0; i < 36; ++i) A[i] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { A[6 * i + j] = P[3 * i + j]; A[6 * i + j + 3] = KR[3 * i + j]; A[6 * (i + 3) + j + 3] = P[3 * i + j]; }
}
// the inverse of a symmetric positive definite 6x6 through an unpivoted L D L^T, column by column, then six solves
__device__ __forceinline__ void pg_ldlt6_inverse(const double* H, double* inv)
{
    double L[36], d[6];
    for (int j = 0; j < 6; ++j) {
        double s = H[6 * j + j];
        for (int p = 0; p < j; ++p) s = s - (L[6 * j + p] * L[6 * j + p]) * d[p];
        d[j] = s;
        for (int i = j + 1; i < 6; ++i) {
            double s2 = H[6 * i + j];
            for (int p = 0; p < j; ++p) s2 = s2 - (L[6 * i + p] * L[6 * j + p]) * d[p];
            L[6 * i + j] = s2 / d[j];
        }
    }
    for (int c = 0; c < 6; ++c) {
        double y[6];
        for (int i = 0; i < 6; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int p = 0; p < i; ++p) s = s - L[6 * i + p] * y[p];
            y[i] = s;
        }
        for (int i = 0; i < 6; ++i) y[i] = y[i] / d[i];
        for (int i = 5; i >= 0; --i) {
            double s = y[i];
            for (int p = i + 1; p < 6; ++p) s = s - L[6 * p + i] * y[p];
            y[i] = s;
        }
        for (int i = 0; i < 6; ++i) inv[6 * i + c] = y[i];
    }
}

// ---- compose: T_k = D_1 ... D_k, the poses RELATIVE TO NODE 0 (element 0 is the identity).  The solver never sees T_0: the adjoints' entries grow
// with the distance from the frame's origin (B_l linearly, G_k quadratically) and the O(1) blocks of S come out of their products, so the frame is
// put where the trajectory starts; pg_export multiplies T_0 back in ----
// Hillis-Steele over one block of 256 elements held as 12 planes in LDS (the tail of the last block is identities, which multiply exactly)
__device__ __forceinline__ void pg_block_scan(double (*sh)[KT_PG_LANES], double* mine, int t)
{
    for (int e = 0; e < 12; ++e) sh[e][t] = mine[e];
    __syncthreads();
    for (int off = 1; off < KT_PG_LANES; off <<= 1) {
        double a[12], o[12];
        const bool has = t >= off;
        if (has) for (int e = 0; e < 12; ++e) a[e] = sh[e][t - off];
        __syncthreads();
        if (has) {
            pg_mul(a, mine, o);
            for (int e = 0; e < 12; ++e) { mine[e] = o[e]; sh[e][t] = o[e]; }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(KT_PG_LANES) void pg_scan_local(const kt_pg_state* __restrict__ st, const double* __restrict__ D, int n, double* __restrict__ P,
                                                             double* __restrict__ tot)
{
    __shared__ double sh[12][KT_PG_LANES];
    if (st->done) return;
    const int t = threadIdx.x, g = blockIdx.x * KT_PG_LANES + t;
    double mine[12];
    if (g > 0 && g < n) for (int e = 0; e < 12; ++e) mine[e] = D[12 * (size_t)g + e];
    else pg_identity(mine);   // node 0 sits at the identity while the solver works (T_0 comes in at the export), the tail is padding
    pg_block_scan(sh, mine, t);
    if (g < n) for (int e = 0; e < 12; ++e) P[12 * (size_t)g + e] = mine[e];
    if (t == KT_PG_LANES - 1) for (int e = 0; e < 12; ++e) tot[12 * (size_t)blockIdx.x + e] = mine[e];
}

// ONE workgroup over the nb block totals, kt_scan_runs_kernel's shape: a serial run per lane, a scan over the lanes, the exclusive bases
__global__ __launch_bounds__(KT_PG_LANES) void pg_scan_carry(const kt_pg_state* __restrict__ st, const double* __restrict__ tot, int nb, double* __restrict__ base)
{
    __shared__ double sh[12][KT_PG_LANES];
    if (st->done) return;
    const int t = threadIdx.x, per = (nb + KT_PG_LANES - 1) / KT_PG_LANES, i0 = t * per, i1 = min(nb, i0 + per);
    double s[12], o[12];
    pg_identity(s);
    for (int i = i0; i < i1; ++i) {
        pg_mul(s, tot + 12 * (size_t)i, o);
        for (int e = 0; e < 12; ++e) s[e] = o[e];
    }
    pg_block_scan(sh, s, t);
    double b[12];
    if (t == 0) pg_identity(b);
    else for (int e = 0; e < 12; ++e) b[e] = sh[e][t - 1];
    for (int i = i0; i < i1; ++i) {
        for (int e = 0; e < 12; ++e) base[12 * (size_t)i + e] = b[e];
        pg_mul(b, tot + 12 * (size_t)i, o);
        for (int e = 0; e < 12; ++e) b[e] = o[e];
    }
}

// T_g = base[block] x P_g (one block: T = P)
__global__ __launch_bounds__(KT_PG_LANES) void pg_scan_apply(const kt_pg_state* __restrict__ st, const double* __restrict__ P, const double* __restrict__ base, int n,
                                                             int nb, double* __restrict__ T)
{
    if (st->done) return;
    const int g = blockIdx.x * KT_PG_LANES + threadIdx.x;
    if (g >= n) return;
    double o[12];
    if (nb > 1) pg_mul(base + 12 * (size_t)blockIdx.x, P + 12 * (size_t)g, o);
    else for (int e = 0; e < 12; ++e) o[e] = P[12 * (size_t)g + e];
    for (int e = 0; e < 12; ++e) T[12 * (size_t)g + e] = o[e];
}

// ---- per loop: r_l, B_l = Jr(E_l) Ad(T_j^-1), q_l = B_l^T r_l, |r_l|^2 ----
__global__ __launch_bounds__(KT_PG_MAX_LOOPS) void pg_loops(const kt_pg_state* __restrict__ st, const double* __restrict__ T, const int* __restrict__ li,
                                                            const int* __restrict__ lj, const double* __restrict__ LZ, int L, double* __restrict__ B,
                                                            double* __restrict__ q, double* __restrict__ cl)
{
    if (st->done) return;
    const int l = threadIdx.x;
    if (l >= L) return;
    const double *Ti = T + 12 * (size_t)li[l], *Tj = T + 12 * (size_t)lj[l];
    double iT[12], rel[12], Zi[12], E[12], r[6], J[36], jT[12], Ad[36], Bl[36], ql[6];
    pg_inv(Ti, iT);
    pg_mul(iT, Tj, rel);
    pg_inv(LZ + 12 * (size_t)l, Zi);
    pg_mul(Zi, rel, E);
    pg_residual(E, r, J);
    pg_inv(Tj, jT);
    pg_adjoint(jT, Ad);
    pg_mm<6, 6, 6>(J, Ad, Bl);
    pg_mtv<6, 6>(Bl, r, ql);
    for (int e = 0; e < 36; ++e) B[36 * l + e] = Bl[e];
    double c = 0.0;
    for (int e = 0; e < 6; ++e) { q[6 * l + e] = ql[e]; c = c + r[e] * r[e]; }
    cl[l] = c;
}

// ---- per node k = 1 .. n - 1 (row k - 1 of the per-node arrays): H_k^-1, u_k, G_k, h_k = Ad(T_k) u_k, and the workgroup's share of the cost ----
__global__ __launch_bounds__(KT_PG_LANES) void pg_nodes(const kt_pg_state* __restrict__ st, const double* __restrict__ T, const double* __restrict__ D,
                                                        const double* __restrict__ Zc, int n, const int* __restrict__ li, const int* __restrict__ lj,
                                                        const double* __restrict__ q, int L, double* __restrict__ Hinv, double* __restrict__ u,
                                                        double* __restrict__ G, double* __restrict__ h, double* __restrict__ costpart)
{
    __shared__ double wave_cost[KT_PG_LANES / 64];
    if (st->done) return;
    const int t = threadIdx.x, row = blockIdx.x * KT_PG_LANES + t, k = row + 1;
    double ck = 0.0;
    if (k < n) {
        double Zi[12], E[12], r[6], J[36], H[36], Hi[36], g[6], sq[6] = {0, 0, 0, 0, 0, 0}, Ad[36], w[6], b[6], uk[6], X[36], Gk[36], hk[6];
        pg_inv(Zc + 12 * (size_t)k, Zi);
        pg_mul(Zi, D + 12 * (size_t)k, E);
        pg_residual(E, r, J);
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) {
                double acc = J[i] * J[j];
                for (int c = 1; c < 6; ++c) acc = acc + J[6 * c + i] * J[6 * c + j];
                H[6 * i + j] = acc;
            }
        pg_ldlt6_inverse(H, Hi);
        pg_mtv<6, 6>(J, r, g);
        for (int l = 0; l < L; ++l)
            if (li[l] < k && k <= lj[l])
                for (int e = 0; e < 6; ++e) sq[e] = sq[e] + q[6 * l + e];
        pg_adjoint(T + 12 * (size_t)k, Ad);
        pg_mtv<6, 6>(Ad, sq, w);
        for (int e = 0; e < 6; ++e) b[e] = -(g[e] + w[e]);
        pg_mv<6, 6>(Hi, b, uk);
        pg_mm<6, 6, 6>(Ad, Hi, X);
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) {
                double acc = X[6 * i] * Ad[6 * j];
                for (int c = 1; c < 6; ++c) acc = acc + X[6 * i + c] * Ad[6 * j + c];
                Gk[6 * i + j] = acc;
            }
        pg_mv<6, 6>(Ad, uk, hk);
        for (int e = 0; e < 36; ++e) { Hinv[36 * (size_t)row + e] = Hi[e]; G[36 * (size_t)row + e] = Gk[e]; }
        for (int e = 0; e < 6; ++e) { u[6 * (size_t)row + e] = uk[e]; h[6 * (size_t)row + e] = hk[e]; ck = ck + r[e] * r[e]; }
    }
    const double ws = kt_wave_sum(ck);
    if ((t & 63) == 0) wave_cost[t >> 6] = ws;
    __syncthreads();
    if (t == 0) {
        double c = wave_cost[0];
        for (int w = 1; w < KT_PG_LANES / 64; ++w) c = c + wave_cost[w];
        costpart[blockIdx.x] = c;
    }
}

// ---- the cost of the poses just evaluated and the bookkeeping of the step that led to them (step = 0: the start) ----
__global__ void pg_tally(kt_pg_state* __restrict__ st, const double* __restrict__ costpart, int nparts, const double* __restrict__ cl, int L, int step, int zero_step)
{
    if (threadIdx.x != 0 || st->done) return;
    double cost = 0.0;
    for (int i = 0; i < nparts; ++i) cost = cost + costpart[i];
    for (int l = 0; l < L; ++l) cost = cost + cl[l];
    const double chi2 = KT_PG_CHI2_SCALE * cost;
    if (step == 0) st->chi2_start = chi2;
    st->chi2_end = chi2;
    if (step > 0) {
        st->steps = step;
        const double md = __longlong_as_double((long long)st->maxdelta_bits);
        if (md < KT_PG_DELTA_TOL) { st->done = 1; st->status = KT_POSE_GRAPH_CONVERGED; }
        else if (step == KT_PG_MAX_STEPS) { st->done = 1; st->status = KT_POSE_GRAPH_MAX_STEPS; }
        st->maxdelta_bits = 0ull;
    } else if (zero_step) { st->done = 1; st->status = KT_POSE_GRAPH_CONVERGED; }
}

// ---- S and v: workgroup p owns the pair (l, m), l <= m, and sums G_k over the nodes both loops span ----
__global__ __launch_bounds__(KT_PG_LANES) void pg_pairs(const kt_pg_state* __restrict__ st, const int* __restrict__ li, const int* __restrict__ lj,
                                                        const double* __restrict__ B, const double* __restrict__ G, const double* __restrict__ h, int L,
                                                        double* __restrict__ S, double* __restrict__ v)
{
    __shared__ double wave_part[KT_PG_LANES / 64][42];
    __shared__ double M[42];
    if (st->done) return;
    int p = blockIdx.x, l = 0;
    while (p >= L - l) { p -= L - l; ++l; }
    const int m = l + p, t = threadIdx.x, n6 = 6 * L;
    const int lo = max(li[l], li[m]) + 1, hi = min(lj[l], lj[m]);
    double acc[36], hs[6] = {0, 0, 0, 0, 0, 0};
    for (int e = 0; e < 36; ++e) acc[e] = 0.0;
    for (int k = lo + t; k <= hi; k += KT_PG_LANES) {
        const double* Gk = G + 36 * (size_t)(k - 1);
        for (int e = 0; e < 36; ++e) acc[e] = acc[e] + Gk[e];
        if (l == m) for (int e = 0; e < 6; ++e) hs[e] = hs[e] + h[6 * (size_t)(k - 1) + e];
    }
    for (int e = 0; e < 36; ++e) {
        const double ws = kt_wave_sum(acc[e]);
        if ((t & 63) == 0) wave_part[t >> 6][e] = ws;
    }
    for (int e = 0; e < 6; ++e) {
        const double ws = kt_wave_sum(hs[e]);
        if ((t & 63) == 0) wave_part[t >> 6][36 + e] = ws;
    }
    __syncthreads();
    if (t < 42) {
        double s = wave_part[0][t];
        for (int w = 1; w < KT_PG_LANES / 64; ++w) s = s + wave_part[w][t];
        M[t] = s;
    }
    __syncthreads();
    const double *Bl = B + 36 * l, *Bm = B + 36 * m;
    if (t < 36) {
        const int a = t / 6, b = t % 6;
        double X[6];
        for (int d = 0; d < 6; ++d) {
            double s = Bl[6 * a] * M[d];
            for (int c = 1; c < 6; ++c) s = s + Bl[6 * a + c] * M[6 * c + d];
            X[d] = s;
        }
        double val = X[0] * Bm[6 * b];
        for (int d = 1; d < 6; ++d) val = val + X[d] * Bm[6 * b + d];
        if (l == m && a == b) val = val + 1.0;
        // pg_solve reads the lower triangle: an off-diagonal block goes there as the mirror, a diagonal block is written entry by entry (G_k is
        // symmetric only up to rounding, so a mirror store would race with the lane that owns the address)
        S[(size_t)(6 * l + a) * n6 + 6 * m + b] = val;
        if (l != m) S[(size_t)(6 * m + b) * n6 + 6 * l + a] = val;
    } else if (t < 42 && l == m) {
        const int a = t - 36;
        double s = Bl[6 * a] * M[36];
        for (int c = 1; c < 6; ++c) s = s + Bl[6 * a + c] * M[36 + c];
        v[6 * l + a] = s;
    }
}

// ---- S y = v by a right-looking L D L^T in ONE workgroup (S stays in global memory), then z_l = B_l^T y_l ----
__global__ __launch_bounds__(KT_PG_LANES) void pg_solve(const kt_pg_state* __restrict__ st, double* __restrict__ S, const double* __restrict__ v,
                                                        const double* __restrict__ B, int L, double* __restrict__ z)
{
    __shared__ double sh_a[6 * KT_PG_MAX_LOOPS], sh_l[6 * KT_PG_MAX_LOOPS], y[6 * KT_PG_MAX_LOOPS], d[6 * KT_PG_MAX_LOOPS];
    if (st->done) return;
    const int t = threadIdx.x, n = 6 * L, ty = t >> 4, tx = t & 15;
    for (int i = t; i < n; i += KT_PG_LANES) y[i] = v[i];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        const double dj = S[(size_t)j * n + j];
        if (t == 0) d[j] = dj;
        for (int i = j + 1 + t; i < n; i += KT_PG_LANES) {
            const double a = S[(size_t)i * n + j], lc = a / dj;
            sh_a[i] = a; sh_l[i] = lc;
            S[(size_t)i * n + j] = lc;
        }
        __syncthreads();
        for (int i = j + 1 + ty; i < n; i += 16)
            for (int c = j + 1 + tx; c <= i; c += 16) S[(size_t)i * n + c] = S[(size_t)i * n + c] - sh_l[i] * sh_a[c];
        __syncthreads();
    }
    for (int j = 0; j < n; ++j) {
        const double yj = y[j];
        for (int i = j + 1 + t; i < n; i += KT_PG_LANES) y[i] = y[i] - S[(size_t)i * n + j] * yj;
        __syncthreads();
    }
    for (int i = t; i < n; i += KT_PG_LANES) y[i] = y[i] / d[i];
    __syncthreads();
    for (int j = n - 1; j >= 0; --j) {
        const double yj = y[j];
        for (int i = t; i < j; i += KT_PG_LANES) y[i] = y[i] - S[(size_t)j * n + i] * yj;
        __syncthreads();
    }
    for (int i = t; i < n; i += KT_PG_LANES) {
        const int l = i / 6, c = i % 6;
        double s = B[36 * l + c] * y[6 * l];
        for (int a = 1; a < 6; ++a) s = s + B[36 * l + 6 * a + c] * y[6 * l + a];
        z[i] = s;
    }
}

// ---- per node: delta_k = u_k - H_k^-1 Ad(T_k)^T sum_l z_l, D_k <- D_k Exp(delta_k), max |delta|_inf ----
__global__ __launch_bounds__(KT_PG_LANES) void pg_update(kt_pg_state* __restrict__ st, const double* __restrict__ T, double* __restrict__ D, int n,
                                                         const int* __restrict__ li, const int* __restrict__ lj, const double* __restrict__ z, int L,
                                                         const double* __restrict__ Hinv, const double* __restrict__ u)
{
    if (st->done) return;
    const int row = blockIdx.x * KT_PG_LANES + threadIdx.x, k = row + 1;
    if (k >= n) return;
    double sz[6] = {0, 0, 0, 0, 0, 0}, Ad[36], w[6], Hw[6], delta[6], Rw[9], Dk[12], o[12];
    for (int l = 0; l < L; ++l)
        if (li[l] < k && k <= lj[l])
            for (int e = 0; e < 6; ++e) sz[e] = sz[e] + z[6 * l + e];
    pg_adjoint(T + 12 * (size_t)k, Ad);
    pg_mtv<6, 6>(Ad, sz, w);
    pg_mv<6, 6>(Hinv + 36 * (size_t)row, w, Hw);
    double md = 0.0;
    for (int e = 0; e < 6; ++e) { delta[e] = u[6 * (size_t)row + e] - Hw[e]; md = fmax(md, fabs(delta[e])); }
    for (int e = 0; e < 12; ++e) Dk[e] = D[12 * (size_t)k + e];
    pg_so3_exp(delta + 3, Rw);
    pg_mm<3, 3, 3>(Dk, Rw, o);
    pg_mv<3, 3>(Dk, delta, o + 9);
    for (int e = 0; e < 3; ++e) o[9 + e] = o[9 + e] + Dk[9 + e];
    for (int e = 0; e < 12; ++e) D[12 * (size_t)k + e] = o[e];
    atomicMax(&st->maxdelta_bits, (unsigned long long)__double_as_longlong(md));   // an integer maximum: order does not matter
}

// ---- the download: n row-major 4x4 poses, then {chi2_start, chi2_end, steps, status} ----
__global__ __launch_bounds__(KT_PG_LANES) void pg_export(const kt_pg_state* __restrict__ st, const double* __restrict__ T, const double* __restrict__ T0, int n,
                                                         double* __restrict__ out)
{
    const int g = blockIdx.x * KT_PG_LANES + threadIdx.x;
    if (g < n) {
        double P[12];
        if (g == 0) for (int e = 0; e < 12; ++e) P[e] = T0[e];   // fixed: the caller's bits
        else pg_mul(T0, T + 12 * (size_t)g, P);
        double* o = out + 16 * (size_t)g;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) o[4 * i + j] = P[3 * i + j];
            o[4 * i + 3] = P[9 + i];
        }
        o[12] = o[13] = o[14] = 0.0; o[15] = 1.0;
    }
    if (g == 0) {
        double* r = out + 16 * (size_t)n;
        r[0] = st->chi2_start; r[1] = st->chi2_end; r[2] = (double)st->steps; r[3] = (double)st->status;
    }
}

// the rotation of R's normalised quaternion (w, x, y, z), taken from the largest of {trace, R00, R11, R22} (Shepperd)
void quat_rotation(const double* R, double* o)
{
    const double t = (R[0] + R[4]) + R[8];
    double q[4];
    if (t >= R[0] && t >= R[4] && t >= R[8]) { q[0] = 1.0 + t; q[1] = R[7] - R[5]; q[2] = R[2] - R[6]; q[3] = R[3] - R[1]; }
    else if (R[0] >= R[4] && R[0] >= R[8]) { q[0] = R[7] - R[5]; q[1] = ((1.0 + R[0]) - R[4]) - R[8]; q[2] = R[1] + R[3]; q[3] = R[2] + R[6]; }
    else if (R[4] >= R[8]) { q[0] = R[2] - R[6]; q[1] = R[1] + R[3]; q[2] = ((1.0 - R[0]) + R[4]) - R[8]; q[3] = R[5] + R[7]; }
    else { q[0] = R[3] - R[1]; q[1] = R[2] + R[6]; q[2] = R[5] + R[7]; q[3] = ((1.0 - R[0]) - R[4]) + R[8]; }
    const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const double w = q[0] / nrm, x = q[1] / nrm, y = q[2] / nrm, z = q[3] / nrm;
    o[0] = 1.0 - 2.0 * (y * y + z * z); o[1] = 2.0 * (x * y - w * z); o[2] = 2.0 * (x * z + w * y);
    o[3] = 2.0 * (x * y + w * z); o[4] = 1.0 - 2.0 * (x * x + z * z); o[5] = 2.0 * (y * z - w * x);
    o[6] = 2.0 * (x * z - w * y); o[7] = 2.0 * (y * z + w * x); o[8] = 1.0 - 2.0 * (x * x + y * y);
}

void pose12_of_float16(const float* m, double* o)
{
    double R[9];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (double)m[4 * i + j];
        o[9 + i] = (double)m[4 * i + 3];
    }
    quat_rotation(R, o);
}

}  // namespace

extern "C" int kt_host_pose_graph_measurement(const float prev16[16], const float curr16[16], double Z16[16])
{
    KT_ARG(prev16 && curr16 && Z16);
    double P[12], Cm[12], Pi[12], Z[12];
    pose12_of_float16(prev16, P);
    pose12_of_float16(curr16, Cm);
    pg_inv(P, Pi);
    pg_mul(Pi, Cm, Z);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Z16[4 * i + j] = Z[3 * i + j];
        Z16[4 * i + 3] = Z[9 + i];
    }
    Z16[12] = Z16[13] = Z16[14] = 0.0; Z16[15] = 1.0;
    return KT_OK;
}

struct kt_pose_graph {
    kt_mem mem;
    kt_ctx* ctx;
    hipStream_t stream;
    int max_nodes, max_loops;
    kt_pg_state* state;
    double *Zc, *D, *P, *T;          // device, max_nodes x 12: the chain measurements (row 0 = T_0), the increments, the blocks' prefixes, the poses relative to node 0
    double *tot, *base, *costpart;   // device, per block of 256
    double *Hinv, *G, *u, *h;        // device, per node: 36, 36, 6, 6
    int *li, *lj;                    // device, max_loops (+ 1: an empty graph still has an address)
    double *LZ, *B, *q, *cl, *z, *v; // device, per loop: 12, 36, 6, 1, 6, 6
    double* S;                       // device, (6 max_loops)^2
    double* out;                     // device, max_nodes x 16 + 4
    double* in_host;                 // pinned, max_nodes x 12 + max_loops x 12
    int* loops_host;                 // pinned, 2 x max_loops
    double* out_host;                // pinned, max_nodes x 16 + 4
};

extern "C" int kt_pose_graph_destroy(kt_pose_graph* pg)
{
    if (!pg) return KT_OK;
    if (pg->stream) (void)hipStreamSynchronize(pg->stream);
    pg->mem.release();
    delete pg;
    return KT_OK;
}

extern "C" int kt_pose_graph_create(kt_ctx* c, int max_nodes, int max_loops, void* hip_stream, kt_pose_graph** out)
{
    KT_ARG(c && out && max_nodes >= 1 && max_nodes <= KT_PG_MAX_NODES && max_loops >= 0 && max_loops <= KT_PG_MAX_LOOPS);
    KT_HIP(hipSetDevice(c->device));
    kt_pose_graph* pg = new kt_pose_graph();   // value-initialised: every pointer starts null
    pg->ctx = c; pg->stream = hip_stream ? (hipStream_t)hip_stream : c->stream; pg->max_nodes = max_nodes; pg->max_loops = max_loops;
    const size_t N = (size_t)max_nodes, L = (size_t)max_loops + 1, NB = (N + KT_PG_LANES - 1) / KT_PG_LANES;
    int s = pg->mem.device(&pg->state, 1);
    if (s == KT_OK) s = pg->mem.device(&pg->Zc, N * 12);
    if (s == KT_OK) s = pg->mem.device(&pg->D, N * 12);
    if (s == KT_OK) s = pg->mem.device(&pg->P, N * 12);
    if (s == KT_OK) s = pg->mem.device(&pg->T, N * 12);
    if (s == KT_OK) s = pg->mem.device(&pg->tot, NB * 12);
    if (s == KT_OK) s = pg->mem.device(&pg->base, NB * 12);
    if (s == KT_OK) s = pg->mem.device(&pg->costpart, NB);
    if (s == KT_OK) s = pg->mem.device(&pg->Hinv, N * 36);
    if (s == KT_OK) s = pg->mem.device(&pg->G, N * 36);
    if (s == KT_OK) s = pg->mem.device(&pg->u, N * 6);
    if (s == KT_OK) s = pg->mem.device(&pg->h, N * 6);
    if (s == KT_OK) s = pg->mem.device(&pg->li, L);
    if (s == KT_OK) s = pg->mem.device(&pg->lj, L);
    if (s == KT_OK) s = pg->mem.device(&pg->LZ, L * 12);
    if (s == KT_OK) s = pg->mem.device(&pg->B, L * 36);
    if (s == KT_OK) s = pg->mem.device(&pg->q, L * 6);
    if (s == KT_OK) s = pg->mem.device(&pg->cl, L);
    if (s == KT_OK) s = pg->mem.device(&pg->z, L * 6);
    if (s == KT_OK) s = pg->mem.device(&pg->v, L * 6);
    if (s == KT_OK) s = pg->mem.device(&pg->S, L * 6 * L * 6);
    if (s == KT_OK) s = pg->mem.device(&pg->out, N * 16 + 4);
    if (s == KT_OK) s = pg->mem.pinned(&pg->in_host, N * 12 + L * 12);
    if (s == KT_OK) s = pg->mem.pinned(&pg->loops_host, 2 * L);
    if (s == KT_OK) s = pg->mem.pinned(&pg->out_host, N * 16 + 4);
    if (s != KT_OK) { (void)kt_pose_graph_destroy(pg); return s; }
    *out = pg;
    return KT_OK;
}

// launches 1 and 2 of a step and the tally: the poses of the increments, the residuals and blocks at them, their cost
static int pg_evaluate_enqueue(kt_pose_graph* pg, int n, int L, int step, int zero_step)
{
    const int nb = kt_div_up(n, KT_PG_LANES), nparts = n > 1 ? kt_div_up(n - 1, KT_PG_LANES) : 0;
    hipStream_t st = pg->stream;
    hipLaunchKernelGGL(pg_scan_local, dim3(nb), dim3(KT_PG_LANES), 0, st, pg->state, pg->D, n, pg->P, pg->tot);
    KT_LAUNCH_CHECK();
    if (nb > 1) {
        hipLaunchKernelGGL(pg_scan_carry, dim3(1), dim3(KT_PG_LANES), 0, st, pg->state, pg->tot, nb, pg->base);
        KT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pg_scan_apply, dim3(nb), dim3(KT_PG_LANES), 0, st, pg->state, pg->P, pg->base, n, nb, pg->T);
    KT_LAUNCH_CHECK();
    if (n < 2) return KT_OK;
    if (L > 0) {
        hipLaunchKernelGGL(pg_loops, dim3(1), dim3(KT_PG_MAX_LOOPS), 0, st, pg->state, pg->T, pg->li, pg->lj, pg->LZ, L, pg->B, pg->q, pg->cl);
        KT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pg_nodes, dim3(nparts), dim3(KT_PG_LANES), 0, st, pg->state, pg->T, pg->D, pg->Zc, n, pg->li, pg->lj, pg->q, L, pg->Hinv, pg->u, pg->G, pg->h,
                       pg->costpart);
    KT_LAUNCH_CHECK();
    hipLaunchKernelGGL(pg_tally, dim3(1), dim3(64), 0, st, pg->state, pg->costpart, nparts, pg->cl, L, step, zero_step);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

extern "C" int kt_pose_graph_optimise(kt_pose_graph* pg, int n_nodes, const double T0[16], const double* chain_Z, int n_loops, const int* loop_a,
                                      const int* loop_b, const double* loop_Z, double* poses_out, kt_pose_graph_result* result)
{
    KT_ARG(pg && T0 && poses_out && result && n_nodes >= 1 && n_loops >= 0 && (chain_Z || n_nodes == 1) && ((loop_a && loop_b && loop_Z) || n_loops == 0));
    if (n_nodes > pg->max_nodes || n_loops > pg->max_loops) {
        kt_set_error("kt_pose_graph_optimise: %d nodes and %d loops, capacity %d and %d", n_nodes, n_loops, pg->max_nodes, pg->max_loops);
        return KT_ERR_CAPACITY;
    }
    for (int l = 0; l < n_loops; ++l) KT_ARG(loop_a[l] >= 0 && loop_a[l] < n_nodes && loop_b[l] >= 0 && loop_b[l] < n_nodes && loop_a[l] != loop_b[l]);
    const int n = n_nodes, L = n_loops;
    hipStream_t st = pg->stream;
    KT_HIP(hipSetDevice(pg->ctx->device));
    // stage: row 0 = T_0, row k = Z_k; every loop as (i, j, Z) with i < j, a swapped pair with the rigid inverse of its measurement
    double* lz_host = pg->in_host + (size_t)pg->max_nodes * 12;
    pg_from16(T0, pg->in_host);
    for (int k = 1; k < n; ++k) pg_from16(chain_Z + 16 * (size_t)(k - 1), pg->in_host + 12 * (size_t)k);
    for (int l = 0; l < L; ++l) {
        double Z[12];
        pg_from16(loop_Z + 16 * (size_t)l, Z);
        if (loop_a[l] < loop_b[l]) { pg->loops_host[l] = loop_a[l]; pg->loops_host[pg->max_loops + 1 + l] = loop_b[l]; memcpy(lz_host + 12 * (size_t)l, Z, sizeof(Z)); }
        else { pg->loops_host[l] = loop_b[l]; pg->loops_host[pg->max_loops + 1 + l] = loop_a[l]; pg_inv(Z, lz_host + 12 * (size_t)l); }
    }
    KT_HIP(hipMemsetAsync(pg->state, 0, sizeof(kt_pg_state), st));
    KT_HIP(hipMemcpyAsync(pg->Zc, pg->in_host, (size_t)n * 12 * sizeof(double), hipMemcpyHostToDevice, st));
    KT_HIP(hipMemcpyAsync(pg->D, pg->Zc, (size_t)n * 12 * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (L > 0) {
        KT_HIP(hipMemcpyAsync(pg->li, pg->loops_host, (size_t)L * sizeof(int), hipMemcpyHostToDevice, st));
        KT_HIP(hipMemcpyAsync(pg->lj, pg->loops_host + pg->max_loops + 1, (size_t)L * sizeof(int), hipMemcpyHostToDevice, st));
        KT_HIP(hipMemcpyAsync(pg->LZ, lz_host, (size_t)L * 12 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    // the start; with no loop there is nothing to optimise: status converged after a zero step (an all-zero state says so for one node)
    KT_TRY(pg_evaluate_enqueue(pg, n, L, 0, L == 0));
    if (L > 0) {
        const int nparts = kt_div_up(n - 1, KT_PG_LANES);
        for (int step = 1; step <= KT_PG_MAX_STEPS; ++step) {
            hipLaunchKernelGGL(pg_pairs, dim3(L * (L + 1) / 2), dim3(KT_PG_LANES), 0, st, pg->state, pg->li, pg->lj, pg->B, pg->G, pg->h, L, pg->S, pg->v);
            KT_LAUNCH_CHECK();
            hipLaunchKernelGGL(pg_solve, dim3(1), dim3(KT_PG_LANES), 0, st, pg->state, pg->S, pg->v, pg->B, L, pg->z);
            KT_LAUNCH_CHECK();
            hipLaunchKernelGGL(pg_update, dim3(nparts), dim3(KT_PG_LANES), 0, st, pg->state, pg->T, pg->D, n, pg->li, pg->lj, pg->z, L, pg->Hinv, pg->u);
            KT_LAUNCH_CHECK();
            KT_TRY(pg_evaluate_enqueue(pg, n, L, step, 0));
        }
    }
    hipLaunchKernelGGL(pg_export, dim3(kt_div_up(n, KT_PG_LANES)), dim3(KT_PG_LANES), 0, st, pg->state, pg->T, pg->Zc, n, pg->out);
    KT_LAUNCH_CHECK();
    KT_HIP(hipMemcpyAsync(pg->out_host, pg->out, ((size_t)n * 16 + 4) * sizeof(double), hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
    memcpy(poses_out, pg->out_host, (size_t)n * 16 * sizeof(double));
    const double* r = pg->out_host + (size_t)n * 16;
    result->chi2_start = r[0]; result->chi2_end = r[1]; result->steps = (int)r[2]; result->status = (int)r[3];
    return KT_OK;
}
