// kt_raycast.hip -- the ray cast of the cyclical TSDF volume for gfx950 (a12, rayCastKernel): kt_raycast_args, the per-axis voxel
// stepping (kt_rc_axis_t, kt_rc<POW2>; its indexing is kt_rc_index.hpp), the fused vertex / normal map resize of the tracker path
// (kt_tile_resize), kt_raycast_kernel, and its launcher kt_raycast_impl behind the C-ABI's kt_raycast.  Hand-written wave64 HIP.
// Reference: src/frontend/cuda/ray_caster.cu, maps.cu (file:line cited per kernel).  Results are bit-identical to the oracle's
// restatement of those files: same operation order, explicit fmaf sites, IEEE div/sqrt.
//
// Volume layout as in kt_volume.hip: tsdf = int16[N^3] (x fastest), colour+weight = uchar4[N^3], storage index = logical index
// rotated by voxel_wrap.  The "holds a negative tsdf" brick flags that steer the empty-space hops are raised by the voxel pass
// (kt_volume.hip); KT_BRICK is in kt_internal.hpp.
#include "kt_internal.hpp"
#include "kt_rc_index.hpp"

// ================================================================================================
// a12  raycast -> rayCastKernel                       ray_caster.cu:56-471
// ================================================================================================
struct kt_raycast_args {
    kt_mat33 R;
    float tx, ty, tz;
    float time_step;
    float vsx, vsy, vsz;        // volume size
    float cx_, cy_, cz_;        // cell size
    int cols, rows, N;
    const int16_t* volume;
    const uchar4* color;
    kt_intr intr;
    float* vmap; float* nmap;
    int wx, wy, wz;
    uchar4* vmap_color;
    unsigned long long* steps;  // optional march-step counter (S of SURVEY 8d)
    // optional fused resizeVMap / resizeNMap outputs for levels 1..3 (maps.cu:225-308), tracker path only
    float* vpyr[3]; float* npyr[3];
    const kt_frame_params* fp;  // when set: R / t come from the device
    const unsigned char* bricks; int nb;   // optional negative-brick flags maintained by tsdf23 (N % 32 == 0, nb^3 <= KT_RC_MAX_BRICKS)
    int log2N;                  // N = 2^log2N: the POW2 kernels (then nb = 2^(log2N - KT_BRICK_LOG2) too); -1 otherwise
};

struct kt_rc_axis_t {
    int gpre;            // floor(p / cell): getVoxel's coordinate
    bool ok;             // 0 < gpre < N - 1 (ray_caster.cu:166-173)
    float f;             // (p - (g + 0.5) cell) / cell for the lower tap g
    unsigned int o[2];   // storage offset contributions of taps g and g + 1 along this axis (wrapped; x: 1, y: N, z: N^2)
};

// POW2: N is a power of two (a.log2N holds the exponent) and the storage wrap and the linear index are masks and shifts (kt_rc_index.hpp);
// otherwise conditional subtractions and 24-bit multiplies.  Both give the same integers; kt_raycast_impl picks per launch.
template <bool POW2>
struct kt_rc {
    const kt_raycast_args& a;
    float rcx, rcy, rcz;   // RN(1 / cell) per axis, for voxel_fast
    kt_rc_ix<POW2> ix;
    // storage element of logical voxel (x, y, z), each inside [0, N).  32-bit, and every product through the 24-bit multiplier (v_mad_u32_u24,
    // full rate; a 32 x 32 multiply is quarter rate on CDNA): kt_raycast_impl requires N <= 1536, so Z N + Y < N^2 < 2^24 and the result
    // < N^3 < 2^32.
    __device__ __forceinline__ unsigned int index(int x, int y, int z) const
    {
        return ix.linear(ix.wrap((unsigned int)x, (unsigned int)a.wx), ix.wrap((unsigned int)y, (unsigned int)a.wy), ix.wrap((unsigned int)z, (unsigned int)a.wz));
    }
    __device__ __forceinline__ void voxel(float px, float py, float pz, int& gx, int& gy, int& gz) const
    {
        gx = kt_f2i_rd(px / a.cx_);
        gy = kt_f2i_rd(py / a.cy_);
        gz = kt_f2i_rd(pz / a.cz_);
    }
    // getVoxel for the march loop.  floor(RN(p / cell)) is needed bit-exactly, but the quotient itself only matters next
    // to an integer: q' = p * RN(1 / cell) differs from RN(p / cell) by at most 3 * 2^-24 * |q| (< 1e-4 for |q| <= 512), so
    // whenever q' is farther than 2e-4 from an integer (and |q'| < 1024) floor(q') is the reference's voxel.  Lanes that are
    // not provably safe take the correctly rounded division; the branch is wave-uniform and rare (~7% of wave steps).
    __device__ __forceinline__ void voxel_fast(float px, float py, float pz, int& gx, int& gy, int& gz) const
    {
        const float qx = px * rcx, qy = py * rcy, qz = pz * rcz;
        gx = kt_cvt_flr_i32(qx); gy = kt_cvt_flr_i32(qy); gz = kt_cvt_flr_i32(qz);
        if (!(kt_rc_safe1(qx) && kt_rc_safe1(qy) && kt_rc_safe1(qz))) voxel(px, py, pz, gx, gy, gz);
    }
    // interpolateTrilineary / ...Color / ...Heat bodies, ray_caster.cu:160-296, ONE AXIS AT A TIME (round 5).  Everything such a call derives
    // from a coordinate -- its voxel floor(p / cell), the in-volume test, the lower tap after the half-cell comparison, the fraction and the two
    // wrapped storage offsets -- depends on that coordinate alone, and a hit evaluates 12 interpolations at points that share coordinates: the
    // four colour channels sit at ONE point, and each of the six normal taps (ray_caster.cu:389-409) moves ONE coordinate of that point by a
    // cell.  15 axis evaluations instead of 36, each with the reference's expressions (the voxel through kt_rc::voxel_fast's rule, applied
    // per axis: floor(p * RN(1 / cell)) where provably equal to floor(RN(p / cell)), the division otherwise).
    typedef kt_rc_axis_t axis_t;
    template <int AX>
    __device__ __forceinline__ axis_t axis(float p) const
    {
        const float cell = AX == 0 ? a.cx_ : AX == 1 ? a.cy_ : a.cz_, rcell = AX == 0 ? rcx : AX == 1 ? rcy : rcz;
        const int w = AX == 0 ? a.wx : AX == 1 ? a.wy : a.wz, N = a.N;
        const float q = p * rcell;
        // the guard band by v_fract_f32, floor and convert in one instruction; a quotient that is not provably safe keeps the division and
        // the floor / convert pair (kt_rc_index.hpp)
        int g = kt_cvt_flr_i32(q);
        if (!kt_rc_safe1(q)) g = kt_f2i_rd(p / cell);   // (wave-uniform skip when every lane is safe)
        axis_t r;
        r.gpre = g;
        r.ok = !(g <= 0 || g >= N - 1);
        const float v = ((float)g + 0.5f) * cell;
        g = (p < v) ? (g - 1) : g;
        // (a short form of this division by a launch constant -- reciprocal + two residual corrections, verified exhaustively per
        // divisor -- was measured in round 3: no difference in the kernel's time; profiles/r03_experiments.md)
        r.f = __builtin_fmaf(-((float)g + 0.5f), cell, p) / cell;
#pragma unroll
        for (int d = 0; d < 2; ++d) r.o[d] = ix.template stride<AX>(ix.wrap((unsigned int)(g + d), (unsigned int)w));   // (used where ok: 0 <= g, g + 1 < N)
        return r;
    }
    // the 8-tap blend of interpolateTrilineary (ray_caster.cu:185-194), taps r[k] with k = 4 dx + 2 dy + dz
    static __device__ __forceinline__ float blend(const float (&r)[8], float fa, float fb, float fc)
    {
        const float ia = 1 - fa, ib = 1 - fb, ic = 1 - fc;
        float res = __builtin_fmaf(r[0] * ia * ib, ic, r[1] * ia * ib * fc);
        res = __builtin_fmaf(r[2] * ia * fb, ic, res);
        res = __builtin_fmaf(r[3] * ia * fb, fc, res);
        res = __builtin_fmaf(r[4] * fa * ib, ic, res);
        res = __builtin_fmaf(r[5] * fa * ib, fc, res);
        res = __builtin_fmaf(r[6] * fa * fb, ic, res);
        res = __builtin_fmaf(r[7] * fa * fb, fc, res);
        return res;
    }
    // interpolateTrilineary at the point whose axes are (ax, ay, az); NaN where the reference returns "outside" (ray_caster.cu:166-173)
    __device__ __forceinline__ float tsdf_at(const axis_t& ax, const axis_t& ay, const axis_t& az) const
    {
        if (!(ax.ok && ay.ok && az.ok)) return kt_nan();
        float r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = kt_unpack_tsdf(a.volume[az.o[k & 1] + ay.o[(k >> 1) & 1] + ax.o[(k >> 2) & 1]]);
        return blend(r, ax.f, ay.f, az.f);
    }
    // interpolateTrilinearyColor for the four channels of one point (ray_caster.cu:372-378): each uchar4 tap is loaded once
    __device__ __forceinline__ uchar4 colour_at(const axis_t& ax, const axis_t& ay, const axis_t& az) const
    {
        if (!(ax.ok && ay.ok && az.ok)) return make_uchar4(0, 0, 0, 0);
        uchar4 c[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] = a.color[az.o[k & 1] + ay.o[(k >> 1) & 1] + ax.o[(k >> 2) & 1]];
        float r0[8], r1[8], r2[8], r3[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { r0[k] = (float)c[k].x; r1[k] = (float)c[k].y; r2[k] = (float)c[k].z; r3[k] = (float)c[k].w; }
        return make_uchar4(kt_f2u8_rz(blend(r0, ax.f, ay.f, az.f)), kt_f2u8_rz(blend(r1, ax.f, ay.f, az.f)), kt_f2u8_rz(blend(r2, ax.f, ay.f, az.f)),
                           kt_f2u8_rz(blend(r3, ax.f, ay.f, az.f)));
    }
};

// 2x2 box down-sampling of one map level held in LDS (resizeMapKernel<normalize>, maps.cu:225-277): x-plane NaN in any of
// the four inputs -> NaN in the output x plane only.  src: [3][S][S] tile in LDS, dst written to LDS tile and to global.
template <bool NORMALIZE, int S>
__device__ __forceinline__ void kt_tile_resize(const float* __restrict__ src, float* __restrict__ dst, int lx, int ly, int gx, int gy, int dcols,
                                               int drows, float* __restrict__ out)
{
    constexpr int D = S / 2;
    const float x00 = src[(2 * ly) * S + 2 * lx], x01 = src[(2 * ly) * S + 2 * lx + 1];
    const float x10 = src[(2 * ly + 1) * S + 2 * lx], x11 = src[(2 * ly + 1) * S + 2 * lx + 1];
    const bool inside = gx < dcols && gy < drows;
    if (kt_isnan(x00) || kt_isnan(x01) || kt_isnan(x10) || kt_isnan(x11)) {
        dst[ly * D + lx] = kt_nan();
        if (inside) out[gy * dcols + gx] = kt_nan();
        return;
    }
    f3 n;
    n.x = (x00 + x01 + x10 + x11) / 4;
    const float* sy = src + S * S;
    n.y = (sy[(2 * ly) * S + 2 * lx] + sy[(2 * ly) * S + 2 * lx + 1] + sy[(2 * ly + 1) * S + 2 * lx] + sy[(2 * ly + 1) * S + 2 * lx + 1]) / 4;
    const float* sz = src + 2 * S * S;
    n.z = (sz[(2 * ly) * S + 2 * lx] + sz[(2 * ly) * S + 2 * lx + 1] + sz[(2 * ly + 1) * S + 2 * lx] + sz[(2 * ly + 1) * S + 2 * lx + 1]) / 4;
    if (NORMALIZE) n = kt_normalized(n);
    dst[ly * D + lx] = n.x;
    dst[D * D + ly * D + lx] = n.y;
    dst[2 * D * D + ly * D + lx] = n.z;
    if (inside) {
        out[gy * dcols + gx] = n.x;
        out[(gy + drows) * dcols + gx] = n.y;
        out[(gy + 2 * drows) * dcols + gx] = n.z;
    }
}

#ifndef KT_RC_BATCH
#define KT_RC_BATCH 6   // samples issued together per march iteration (round 5 A/B: 2: 57.2 us, 4: 52.6, 6: 51.4, 8: 52.2 serial stage at VGA; 255 / 243 / 244 us at 1280x960 for 4 / 6 / 8)
#endif
#define KT_RC_MAX_BRICKS 32768   // brick flags staged in LDS (N <= 1024)

// Empty-space skipping (SKIP).  The march only ever reacts to a sign change between two consecutive samples (+ -> - is the hit,
// - -> + leaves).  tsdf23 keeps one flag per 32^3 storage brick, raised when a negative value is stored into it and never lowered
// (clears only zero voxels, so a stale flag is merely conservative).  A sample inside an unflagged brick is >= 0: together with a
// non-negative predecessor it can trigger neither exit, so the whole run of samples up to the brick's far face is replaced by
// the same number of `time_curr += time_step` float adds (the sample times are DEFINED by that recurrence) -- ~80 instructions
// per brick instead of ~100 per sample.  The hop is taken only when every live lane of the wave can take it; the brick test
// uses a 0.01-voxel margin so that position rounding cannot move a skipped sample across a face.  The value of the last
// skipped sample is fetched lazily when the next normal step needs it as `tsdf_prev`.
template <bool COUNT, bool PYR, bool SKIP, bool POW2>
__global__ __launch_bounds__(256) void kt_raycast_kernel(const kt_raycast_args a_in)
{
    kt_raycast_args a = a_in;
    if (a.fp) {
        if (a.fp->skip) return;  // parked for the host's shift path; the predicted maps are rebuilt there
#pragma unroll
        for (int k = 0; k < 9; ++k) a.R.m[k] = a.fp->R[k];
        a.tx = a.fp->t[0]; a.ty = a.fp->t[1]; a.tz = a.fp->t[2];
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char s_bricks[];
    if (SKIP) {
        // dwords, then a byte tail: nb^3 with N % 32 == 0 need not be a multiple of 4 (nb = 3: 27), and only the tracker's own
        // buffer is known to start on a dword
        const int nbytes = a.nb * a.nb * a.nb;
        const int nwords = (((size_t)a.bricks & 3) == 0) ? nbytes >> 2 : 0;
#pragma unroll 1
        for (int i0 = threadIdx.x; i0 < nwords; i0 += 1024) {   // four loads in flight per thread: all of 512^3's 4096 flags in one turn
            unsigned int w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = (i0 + 256 * j < nwords) ? ((const unsigned int*)a.bricks)[i0 + 256 * j] : 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (i0 + 256 * j < nwords) ((unsigned int*)s_bricks)[i0 + 256 * j] = w[j];
        }
#pragma unroll 1
        for (int i = 4 * nwords + threadIdx.x; i < nbytes; i += 256) s_bricks[i] = a.bricks[i];
        __syncthreads();
    }
    // a 256-thread block covers a 16x16 pixel tile; each wave an 8x8 sub-tile (coherent gathers)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tx = (wave & 1) * 8 + (lane & 7), ty = (wave >> 1) * 8 + (lane >> 3);
    const int x = blockIdx.x * 16 + tx;
    const int y = blockIdx.y * 16 + ty;
    const bool in_image = x < a.cols && y < a.rows;
    const kt_rc_ix<POW2> ix{(unsigned int)a.N, (unsigned int)a.log2N};
    const kt_rc<POW2> rc{a, 1.0f / a.cx_, 1.0f / a.cy_, 1.0f / a.cz_, ix};
    const int cols = a.cols, rows = a.rows, N = a.N;
    unsigned int steps = 0, hopped = 0, n_hop_iters = 0, n_batch_iters = 0;

    float out_vx = kt_nan(), out_nx = kt_nan();
    bool hit = false, has_normal = false;
    float vfx = 0, vfy = 0, vfz = 0, nx = 0, ny = 0, nz = 0;
    uchar4 colr = make_uchar4(0, 0, 0, 0);

    if (in_image) {
        const f3 rs = {a.tx, a.ty, a.tz};
        f3 rnl = {((float)x - a.intr.cx) / a.intr.fx, ((float)y - a.intr.cy) / a.intr.fy, 1.0f};
        f3 ray_next = kt_add(kt_mul(a.R, rnl), rs);
        f3 rd = kt_normalized(kt_sub(ray_next, rs));
        rd.x = (rd.x == 0.f) ? (float)1e-15 : rd.x;
        rd.y = (rd.y == 0.f) ? (float)1e-15 : rd.y;
        rd.z = (rd.z == 0.f) ? (float)1e-15 : rd.z;
        // getMinTime / getMaxTime  ray_caster.cu:56-74
        const float txmin = ((rd.x > 0 ? 0.f : a.vsx) - rs.x) / rd.x;
        const float tymin = ((rd.y > 0 ? 0.f : a.vsy) - rs.y) / rd.y;
        const float tzmin = ((rd.z > 0 ? 0.f : a.vsz) - rs.z) / rd.z;
        const float txmax = ((rd.x > 0 ? a.vsx : 0.f) - rs.x) / rd.x;
        const float tymax = ((rd.y > 0 ? a.vsy : 0.f) - rs.y) / rd.y;
        const float tzmax = ((rd.z > 0 ? a.vsz : 0.f) - rs.z) / rd.z;
        float time_start_volume = fmaxf(fmaxf(txmin, tymin), tzmin);
        const float time_exit_volume = fminf(fminf(txmax, tymax), tzmax);
        time_start_volume = fmaxf(time_start_volume, 0.f);
        if (time_start_volume < time_exit_volume) {
            float time_curr = time_start_volume;
            int gx, gy, gz;
            rc.voxel(__builtin_fmaf(rd.x, time_curr, rs.x), __builtin_fmaf(rd.y, time_curr, rs.y), __builtin_fmaf(rd.z, time_curr, rs.z), gx, gy, gz);
            gx = max(0, min(gx, N - 1)); gy = max(0, min(gy, N - 1)); gz = max(0, min(gz, N - 1));
            // only the SIGN of the nearest-voxel tsdf steers the march: compare the packed shorts directly
            int tsdf = a.volume[rc.index(gx, gy, gz)];
            const float max_time = 3 * (a.vsx + a.vsy + a.vsz);
            const float rcx = rc.rcx, rcy = rc.rcy, rcz = rc.rcz;
            // The march (ray_caster.cu:340-352) visits time_curr, time_curr + step, ... one dependent gather per step.
            // The addresses do not depend on the loaded values, so KT_RC_BATCH steps are issued together and the exit
            // tests are then replayed in order; loads past the exit point are speculative and always in bounds.
            // The loop below is branch-free per step (selects instead of breaks) with 32-bit voxel offsets; the only
            // branches are the wave-uniform slow path of the voxel index and the batch-level exit.
            bool crossing = false, done = false;
            float t_cross = 0.f;
            // SKIP state: tsdf_known == false means "the previous sample was skipped: its value is >= 0 but not loaded"
            bool tsdf_known = true;
            const float fN = (float)N, eps_v = 0.01f;
            const float rwx = (float)(a.wx & (KT_BRICK - 1)), rwy = (float)(a.wy & (KT_BRICK - 1)), rwz = (float)(a.wz & (KT_BRICK - 1));
            const int awx = a.wx >> KT_BRICK_LOG2, awy = a.wy >> KT_BRICK_LOG2, awz = a.wz >> KT_BRICK_LOG2;
            const float fB = (float)KT_BRICK, rB = 1.0f / (float)KT_BRICK;
            const kt_rc_ix<POW2> bix{(unsigned int)a.nb, (unsigned int)(a.log2N - KT_BRICK_LOG2)};   // the brick grid: nb = N / 32 is a power of two when N is
            // voxels per unit of ray time along each axis, and its inverse (geometry only: the margins absorb their rounding)
            const float vdx = rd.x * rcx, vdy = rd.y * rcy, vdz = rd.z * rcz;
            const float ivx = __builtin_amdgcn_rcpf(vdx), ivy = __builtin_amdgcn_rcpf(vdy), ivz = __builtin_amdgcn_rcpf(vdz);
            const float inv_step = __builtin_amdgcn_rcpf(a.time_step);
            // the storage wrap as the march's sample_offset takes it: POW2 in vector registers, and opaque so that they stay there
            unsigned int vwx = (unsigned int)a.wx, vwy = (unsigned int)a.wy, vwz = (unsigned int)a.wz;
            if (POW2) asm volatile("" : "+v"(vwx), "+v"(vwy), "+v"(vwz));
            while (true) {
                if (SKIP) {
                    const float tn = time_curr + a.time_step;
                    const float qx = __builtin_fmaf(rd.x, tn, rs.x) * rcx, qy = __builtin_fmaf(rd.y, tn, rs.y) * rcy,
                                qz = __builtin_fmaf(rd.z, tn, rs.z) * rcz;
                    // cell of the storage-brick grid seen from logical coordinates: faces at 32 c - (wrap & 31)
                    const float cx = __builtin_floorf((qx + rwx) * rB), cy = __builtin_floorf((qy + rwy) * rB),
                                cz = __builtin_floorf((qz + rwz) * rB);
                    const float lox = fmaxf(__builtin_fmaf(cx, fB, -rwx), 0.0f) + eps_v, hix = fminf(__builtin_fmaf(cx, fB, fB - rwx), fN) - eps_v;
                    const float loy = fmaxf(__builtin_fmaf(cy, fB, -rwy), 0.0f) + eps_v, hiy = fminf(__builtin_fmaf(cy, fB, fB - rwy), fN) - eps_v;
                    const float loz = fmaxf(__builtin_fmaf(cz, fB, -rwz), 0.0f) + eps_v, hiz = fminf(__builtin_fmaf(cz, fB, fB - rwz), fN) - eps_v;
                    const bool inside = qx > lox && qx < hix && qy > loy && qy < hiy && qz > loz && qz < hiz;
                    bool canhop = false;
                    float dt = 0.f;
                    if (!done && inside && (!tsdf_known || tsdf >= 0)) {
                        // (inside: 0 <= c <= nb.  The floats cx, cy, cz make the faces above, so the convert stays a plain one)
                        const unsigned int bx = bix.wrap((unsigned int)kt_cvt_i32(cx), (unsigned int)awx), by = bix.wrap((unsigned int)kt_cvt_i32(cy), (unsigned int)awy),
                                           bz = bix.wrap((unsigned int)kt_cvt_i32(cz), (unsigned int)awz);
                        if (s_bricks[bix.linear(bx, by, bz)] == 0) {
                            // ray time from this sample to the (margin-shrunk) far face of the cell
                            const float dx = ((vdx > 0 ? hix : lox) - qx) * ivx, dy = ((vdy > 0 ? hiy : loy) - qy) * ivy,
                                        dz = ((vdz > 0 ? hiz : loz) - qz) * ivz;
                            dt = fminf(fminf(dx, dy), dz);
                            canhop = dt >= 0.0f && tn + dt < max_time;
                        }
                    }
                    if (__builtin_amdgcn_ballot_w64(!done && !canhop) == 0) {
                        // samples tn + j * step, j = 0 .. K - 1, lie inside the cell
                        int K = canhop ? 1 + kt_cvt_i32(dt * inv_step) : 0;
                        K = min(K, 64);   // a 32^3 brick holds at most ~14 samples; the bound keeps the replayed adds' drift << the margin
                        const int kmax = kt_wave_max(K);
                        for (int i = 0; i < kmax; ++i) time_curr = (i < K) ? time_curr + a.time_step : time_curr;
                        if (COUNT) { steps += (unsigned int)K; hopped += (unsigned int)K; if (lane == 0) ++n_hop_iters; }
                        tsdf_known = tsdf_known && K == 0;
                        if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
                        continue;
                    }
                    if (!tsdf_known && !done) {  // the next normal step needs the skipped predecessor's value
                        int gx2, gy2, gz2;
                        rc.voxel(__builtin_fmaf(rd.x, time_curr, rs.x), __builtin_fmaf(rd.y, time_curr, rs.y), __builtin_fmaf(rd.z, time_curr, rs.z),
                                 gx2, gy2, gz2);
                        tsdf = a.volume[rc.index(gx2, gy2, gz2)];
                    }
                    tsdf_known = true;
                }
                if (COUNT && lane == 0) ++n_batch_iters;
                float tc[KT_RC_BATCH];
                unsigned int gi[KT_RC_BATCH];
                bool inb[KT_RC_BATCH];
                float t = time_curr;
#pragma unroll
                for (int k = 0; k < KT_RC_BATCH; ++k) {
                    tc[k] = t;
                    const float tn = t + a.time_step;   // (this sample's position and the next one's time: one add)
                    const float px = __builtin_fmaf(rd.x, tn, rs.x), py = __builtin_fmaf(rd.y, tn, rs.y), pz = __builtin_fmaf(rd.z, tn, rs.z);
                    // getVoxel: floor(RN(p / cell)), via p * RN(1 / cell) when provably identical (see kt_rc::voxel_fast): every fraction
                    // farther than 2e-4 from an integer, every |q| < 1024.  The fraction comes from v_fract_f32 and feeds only that test,
                    // floor and convert are one instruction (kt_rc_index.hpp); a NaN coordinate fails the test, and the pair below
                    // converts floor(NaN) to voxel 0 as before.
                    const float qx = px * rcx, qy = py * rcy, qz = pz * rcz;
                    int vx = kt_cvt_flr_i32(qx), vy = kt_cvt_flr_i32(qy), vz = kt_cvt_flr_i32(qz);
                    if (!kt_rc_safe3(qx, qy, qz)) {   // (the compiler skips the block when no lane of the wave needs it)
                        vx = kt_f2i_rd(px / a.cx_);
                        vy = kt_f2i_rd(py / a.cy_);
                        vz = kt_f2i_rd(pz / a.cz_);
                    }
                    const unsigned int ux = (unsigned int)vx, uy = (unsigned int)vy, uz = (unsigned int)vz;
                    inb[k] = ix.inside(ux, uy, uz);  // checkInds (negative indices wrap to huge unsigned values)
                    gi[k] = ix.sample_offset(ux, uy, uz, vwx, vwy, vwz, inb[k]);
                    t = tn;
                }
                short v[KT_RC_BATCH];
#pragma unroll
                for (int k = 0; k < KT_RC_BATCH; ++k) v[k] = ix.fetch16(a.volume, gi[k]);
#pragma unroll
                for (int k = 0; k < KT_RC_BATCH; ++k) {
                    // for (; time_curr < max_time; ...) { if (!checkInds) break; ... }  replayed with selects
                    const bool alive = !done && (tc[k] < max_time) && inb[k];
                    const int cur = v[k];
                    const bool mp = alive && tsdf < 0 && cur > 0;   // - -> + : leave without a hit
                    const bool pm = alive && tsdf > 0 && cur < 0;   // + -> - : zero crossing
                    if (COUNT) steps += alive ? 1u : 0u;
                    t_cross = pm ? tc[k] : t_cross;
                    crossing = crossing || pm;
                    tsdf = alive ? cur : tsdf;
                    done = done || !alive || mp || pm;
                }
                time_curr = t;
                if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
            }
            if (crossing) {  // zero crossing, ray_caster.cu:354-422
                time_curr = t_cross;
                const float tn = time_curr + a.time_step;
                const float px = __builtin_fmaf(rd.x, tn, rs.x), py = __builtin_fmaf(rd.y, tn, rs.y), pz = __builtin_fmaf(rd.z, tn, rs.z);
                const float Ftdt = rc.tsdf_at(rc.template axis<0>(px), rc.template axis<1>(py), rc.template axis<2>(pz));
                if (!kt_isnan(Ftdt)) {
                    const float qx = __builtin_fmaf(rd.x, time_curr, rs.x), qy = __builtin_fmaf(rd.y, time_curr, rs.y), qz = __builtin_fmaf(rd.z, time_curr, rs.z);
                    const kt_rc_axis_t qax = rc.template axis<0>(qx), qay = rc.template axis<1>(qy), qaz = rc.template axis<2>(qz);
                    const float Ft = rc.tsdf_at(qax, qay, qaz);
                    if (!kt_isnan(Ft)) {
                        const float Ts = time_curr - a.time_step * Ft / (Ftdt - Ft);
                        vfx = __builtin_fmaf(rd.x, Ts, rs.x); vfy = __builtin_fmaf(rd.y, Ts, rs.y); vfz = __builtin_fmaf(rd.z, Ts, rs.z);
                        hit = true;
                        out_vx = vfx;
                        const int hx = qax.gpre, hy = qay.gpre, hz = qaz.gpre;   // getVoxel(ray_start + ray_dir * time_curr), ray_caster.cu:380
                        const kt_rc_axis_t cax = rc.template axis<0>(vfx), cay = rc.template axis<1>(vfy), caz = rc.template axis<2>(vfz);
                        colr = rc.colour_at(cax, cay, caz);
                        if (hx > 1 && hy > 1 && hz > 1 && hx < N - 2 && hy < N - 2 && hz < N - 2) {
                            const float Fx1 = rc.tsdf_at(rc.template axis<0>(vfx + a.cx_), cay, caz), Fx2 = rc.tsdf_at(rc.template axis<0>(vfx - a.cx_), cay, caz);
                            const float Fy1 = rc.tsdf_at(cax, rc.template axis<1>(vfy + a.cy_), caz), Fy2 = rc.tsdf_at(cax, rc.template axis<1>(vfy - a.cy_), caz);
                            const float Fz1 = rc.tsdf_at(cax, cay, rc.template axis<2>(vfz + a.cz_)), Fz2 = rc.tsdf_at(cax, cay, rc.template axis<2>(vfz - a.cz_));
                            const f3 n = kt_normalized({Fx1 - Fx2, Fy1 - Fy2, Fz1 - Fz2});
                            nx = n.x; ny = n.y; nz = n.z;
                            has_normal = true;
                            out_nx = nx;
                        }
                    }
                }
            }
        }
        // unhit pixels: NaN in the x planes only, y/z planes and the colour map keep their previous content
        a.vmap[y * cols + x] = out_vx;
        a.nmap[y * cols + x] = out_nx;
        if (hit) {
            a.vmap[(y + rows) * cols + x] = vfy;
            a.vmap[(y + 2 * rows) * cols + x] = vfz;
            a.vmap_color[y * cols + x] = colr;
            if (has_normal) {
                a.nmap[(y + rows) * cols + x] = ny;
                a.nmap[(y + 2 * rows) * cols + x] = nz;
            }
        }
    }
    if (COUNT) {
        for (int off = 32; off > 0; off >>= 1) { steps += __shfl_down(steps, off, 64); hopped += __shfl_down(hopped, off, 64); }
        if (lane == 0 && steps) atomicAdd(a.steps, (unsigned long long)steps);
        if (lane == 0 && hopped) atomicAdd(a.steps + 1, (unsigned long long)hopped);  // diagnostics: samples replaced by brick hops
        if (lane == 0) { atomicAdd(a.steps + 2, (unsigned long long)n_hop_iters); atomicAdd(a.steps + 3, (unsigned long long)n_batch_iters); }
    }
    if (PYR) {
        // fused resizeVMap / resizeNMap for levels 1..3 of this 16x16 tile (KintinuousTracker.cpp:892-899): 8x8, 4x4, 2x2
        __shared__ float tv0[3 * 16 * 16], tn0[3 * 16 * 16];
        __shared__ float tv1[3 * 8 * 8], tn1[3 * 8 * 8], tv2[3 * 4 * 4], tn2[3 * 4 * 4], tv3[3 * 2 * 2], tn3[3 * 2 * 2];
        const int li = ty * 16 + tx;
        tv0[li] = out_vx; tv0[256 + li] = vfy; tv0[512 + li] = vfz;
        tn0[li] = out_nx; tn0[256 + li] = ny; tn0[512 + li] = nz;
        __syncthreads();
        const int t = threadIdx.x;
        if (t < 64) {
            const int lx = t & 7, ly = t >> 3;
            kt_tile_resize<false, 16>(tv0, tv1, lx, ly, blockIdx.x * 8 + lx, blockIdx.y * 8 + ly, cols / 2, rows / 2, a.vpyr[0]);
        } else if (t < 128) {
            const int lx = t & 7, ly = (t >> 3) & 7;
            kt_tile_resize<true, 16>(tn0, tn1, lx, ly, blockIdx.x * 8 + lx, blockIdx.y * 8 + ly, cols / 2, rows / 2, a.npyr[0]);
        }
        __syncthreads();
        if (t < 16) {
            const int lx = t & 3, ly = t >> 2;
            kt_tile_resize<false, 8>(tv1, tv2, lx, ly, blockIdx.x * 4 + lx, blockIdx.y * 4 + ly, cols / 4, rows / 4, a.vpyr[1]);
        } else if (t >= 64 && t < 80) {
            const int lx = t & 3, ly = (t >> 2) & 3;
            kt_tile_resize<true, 8>(tn1, tn2, lx, ly, blockIdx.x * 4 + lx, blockIdx.y * 4 + ly, cols / 4, rows / 4, a.npyr[1]);
        }
        __syncthreads();
        if (t < 4) {
            const int lx = t & 1, ly = t >> 1;
            kt_tile_resize<false, 4>(tv2, tv3, lx, ly, blockIdx.x * 2 + lx, blockIdx.y * 2 + ly, cols / 8, rows / 8, a.vpyr[2]);
        } else if (t >= 64 && t < 68) {
            const int lx = t & 1, ly = (t >> 1) & 1;
            kt_tile_resize<true, 4>(tn2, tn3, lx, ly, blockIdx.x * 2 + lx, blockIdx.y * 2 + ly, cols / 8, rows / 8, a.npyr[2]);
        }
    }
}

int kt_raycast_impl(kt_ctx* c, const kt_intr* intr, const kt_mat33* Rcurr, const float tcurr[3], float tranc_dist,
                    const float volume_size[3], const int16_t* volume, float* vmap, float* nmap, int cols, int rows,
                    const int voxel_wrap[3], uint8_t* vmap_curr_color, const uint8_t* color_volume, int N,
                    unsigned long long* steps_dev, float* const* vpyr, float* const* npyr, const kt_frame_params* fp,
                    const unsigned char* bricks)
{
    KT_ARG(c && intr && Rcurr && tcurr && volume_size && volume && vmap && nmap && voxel_wrap && vmap_curr_color && color_volume);
    KT_ARG(N > 0 && cols > 0 && rows > 0);
    KT_ARG(N <= 1536);  // 32-bit voxel offsets (N^3 < 2^32)
    kt_raycast_args a;
    a.R = *Rcurr;
    a.tx = tcurr[0]; a.ty = tcurr[1]; a.tz = tcurr[2];
    a.time_step = tranc_dist * 0.8f;  // ray_caster.cu:444
    a.vsx = volume_size[0]; a.vsy = volume_size[1]; a.vsz = volume_size[2];
    a.cx_ = volume_size[0] / N; a.cy_ = volume_size[1] / N; a.cz_ = volume_size[2] / N;
    a.cols = cols; a.rows = rows; a.N = N;
    a.volume = volume;
    a.color = (const uchar4*)color_volume;
    a.intr = *intr;
    a.vmap = vmap; a.nmap = nmap;
    for (int k = 0; k < 3; ++k) KT_ARG(voxel_wrap[k] >= 0);
    a.wx = voxel_wrap[0] % N; a.wy = voxel_wrap[1] % N; a.wz = voxel_wrap[2] % N;
    a.vmap_color = (uchar4*)vmap_curr_color;
    a.steps = steps_dev;
    a.fp = fp;
    const bool pyr = vpyr && npyr;
    for (int k = 0; k < 3; ++k) { a.vpyr[k] = pyr ? vpyr[k] : nullptr; a.npyr[k] = pyr ? npyr[k] : nullptr; }
    if (pyr) KT_ARG((cols % 8) == 0 && (rows % 8) == 0);
    dim3 b(256), g(kt_div_up(cols, 16), kt_div_up(rows, 16));
    a.nb = N / KT_BRICK;
    const bool skip = bricks && (N % KT_BRICK) == 0 && a.nb * a.nb * a.nb <= KT_RC_MAX_BRICKS;
    a.bricks = skip ? bricks : nullptr;
    const size_t lds = skip ? (size_t)((a.nb * a.nb * a.nb + 15) & ~15) : 0;
    a.log2N = -1;
    if ((N & (N - 1)) == 0) { a.log2N = 0; while ((1 << a.log2N) < N) ++a.log2N; }
#define KT_RC_LAUNCH(C, P, S) do { if (a.log2N >= 0) hipLaunchKernelGGL((kt_raycast_kernel<C, P, S, true>), g, b, lds, c->stream, a); \
                                   else hipLaunchKernelGGL((kt_raycast_kernel<C, P, S, false>), g, b, lds, c->stream, a); } while (0)
    if (skip) {
        if (pyr) { if (steps_dev) KT_RC_LAUNCH(true, true, true); else KT_RC_LAUNCH(false, true, true); }
        else { if (steps_dev) KT_RC_LAUNCH(true, false, true); else KT_RC_LAUNCH(false, false, true); }
    } else {
        if (pyr) { if (steps_dev) KT_RC_LAUNCH(true, true, false); else KT_RC_LAUNCH(false, true, false); }
        else { if (steps_dev) KT_RC_LAUNCH(true, false, false); else KT_RC_LAUNCH(false, false, false); }
    }
#undef KT_RC_LAUNCH
    KT_LAUNCH_CHECK();
    return KT_OK;
}

extern "C" int kt_raycast(kt_ctx* c, const kt_intr* intr, const kt_mat33* Rcurr, const float tcurr[3], float tranc_dist,
                          const float volume_size[3], const int16_t* volume, float* vmap, float* nmap, int cols, int rows,
                          const int voxel_wrap[3], uint8_t* vmap_curr_color, const uint8_t* color_volume, int N)
{
    return kt_raycast_impl(c, intr, Rcurr, tcurr, tranc_dist, volume_size, volume, vmap, nmap, cols, rows, voxel_wrap,
                           vmap_curr_color, color_volume, N, nullptr, nullptr, nullptr, nullptr, nullptr);
}
