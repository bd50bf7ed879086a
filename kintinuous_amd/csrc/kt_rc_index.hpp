// kt_rc_index.hpp -- the ray cast's voxel indexing (csrc/kt_raycast.hip: kt_raycast_kernel, kt_rc): float coordinate -> voxel -> wrapped
// storage element.  A header of its own so that the check hook (csrc/kt_debug.hip: kt_debug_rc_index) runs these very functions next to the
// forms they replaced.  Every function is an integer or rounding identity of its former form; DESIGN.md 4.2 has the arguments, and
// tests/test_gpu_raycast_index.py holds them over every class of input.
#ifndef KT_RC_INDEX_HPP
#define KT_RC_INDEX_HPP

#include "kt_common.hpp"

#ifdef __HIPCC__
// v_cvt_flr_i32_f32: floor and convert in one instruction.  Equal to kt_cvt_i32(floorf(x)) = kt_f2i_rd(x) for every float that is not a
// NaN -- -0.0, denormals (-denormal -> -1 on both), integers, |x| >= 2^31 and the infinities (both saturate) included; a NaN becomes
// +-(2^31 - 1) by its sign where the pair gives 0 (tests/test_gpu_raycast_index.py holds both statements on the device).  The ray cast
// applies it to quotients that passed its guard-band test, which no NaN passes (kt_rc_safe1, kt_rc_safe3); every other quotient keeps the
// division and the floor / convert pair behind the wave-uniform slow path, and so does the unguarded kt_rc::voxel.
__device__ __forceinline__ int kt_cvt_flr_i32(float x)
{
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// v_fract_f32 = min(x - floorf(x), 1 - 2^-24): differs from the subtraction only where that rounds up to 1.0 (a tiny negative x), and
// both values fail "fraction < 1 - 2e-4".  A NaN gives NaN, and an infinity fails |x| < 1024 whatever its fraction.
__device__ __forceinline__ float kt_fract(float x) { return __builtin_amdgcn_fractf(x); }

#define KT_RC_GUARD 2e-4f    // |q' - RN(p / cell)| < 1e-4 for |q'| < 1024 (kt_rc::voxel_fast)
#define KT_RC_QMAX 1024.f

// "floor(q) is provably the reference's voxel": one coordinate (kt_rc::axis) ...
__device__ __forceinline__ bool kt_rc_safe1(float q)
{
    const float fr = kt_fract(q);
    return fr > KT_RC_GUARD && fr < 1.0f - KT_RC_GUARD && fabsf(q) < KT_RC_QMAX;
}
// ... and the three of a march sample at once: two three-way maxima and two compares.  v_max3_f32 returns its other operands when one
// is a NaN, so a NaN fraction does not spoil `off`; `big` is taken with v_maximum3_f32 (gfx950), which hands a NaN on, so that a sample
// with a NaN coordinate fails `big < 1024` and keeps the pair, whose NaN -> voxel 0 the one-instruction convert does not share.
__device__ __forceinline__ bool kt_rc_safe3(float qx, float qy, float qz)
{
    const float fx = kt_fract(qx), fy = kt_fract(qy), fz = kt_fract(qz);
    const float off = __builtin_fmaxf(__builtin_fmaxf(fabsf(fx - 0.5f), fabsf(fy - 0.5f)), fabsf(fz - 0.5f));
    const float big = __builtin_elementwise_maximum(__builtin_elementwise_maximum(fabsf(qx), fabsf(qy)), fabsf(qz));
    return off < 0.5f - KT_RC_GUARD && big < KT_RC_QMAX;
}

// Integer side.  POW2: N = 2^k (512, 256, 64 ...), chosen per launch; otherwise (768, 96 ...) the 24-bit multiplies and conditional
// subtractions.  N <= 1536 (kt_raycast_impl), u = (unsigned) voxel coordinate (negative ones are huge), 0 <= w < N the storage wrap.
template <bool POW2>
struct kt_rc_ix {
    unsigned int N, k;   // k = log2 N (POW2 only)

    // checkInds: every coordinate inside [0, N).  (ux | uy | uz) < 2^k iff no coordinate has a bit at or above k; max3 for the rest
    __device__ __forceinline__ bool inside(unsigned int ux, unsigned int uy, unsigned int uz) const
    {
        return POW2 ? (ux | uy | uz) < N : max(max(ux, uy), uz) < N;
    }
    // storage coordinate of logical coordinate u: (u + w) mod N for u < N; u + w < 2 N, so one conditional subtraction, or the mask
    __device__ __forceinline__ unsigned int wrap(unsigned int u, unsigned int w) const
    {
        unsigned int X = u + w;
        if (POW2) return X & (N - 1u);
        X -= (X >= N) ? N : 0u;
        return X;
    }
    // storage element (X, Y, Z), each < N: (Z N + Y) N + X
    __device__ __forceinline__ unsigned int linear(unsigned int X, unsigned int Y, unsigned int Z) const
    {
        return POW2 ? (((Z << k) | Y) << k) | X : kt_mad24u(kt_mad24u(Z, N, Y), N, X);
    }
    // wrap + linear of a march sample, as the offset that fetch16() takes.  POW2: the BYTE offset of the 16-bit word -- every field is
    // added and shifted into place in one instruction (v_add_lshl_u32) and masked there (v_and_b32, v_and_or_b32 twice): six instructions
    // instead of three add / compare / conditional subtract triples, two multiplies and the address shift.  N <= 1024 here, so
    // 2 N^3 <= 2^31 fits, and the result is inside the volume for ANY u: a sample outside the volume needs no select to keep its
    // speculative load in bounds.  Otherwise the element index, 0 where the sample is outside (inside_ = inside(ux, uy, uz)).
    // wx, wy, wz come in vector registers (the three-operand forms take one scalar operand; the compiler keeps them across the march).
    __device__ __forceinline__ unsigned int sample_offset(unsigned int ux, unsigned int uy, unsigned int uz, unsigned int wx, unsigned int wy,
                                                          unsigned int wz, bool inside_) const
    {
        if (POW2) {
            const unsigned int m = (N - 1u) << 1;
            unsigned int x, y, z;
            asm("v_add_lshl_u32 %0, %1, %2, 1" : "=v"(x) : "v"(ux), "v"(wx));
            asm("v_add_lshl_u32 %0, %1, %2, %3" : "=v"(y) : "v"(uy), "v"(wy), "s"(k + 1u));
            asm("v_add_lshl_u32 %0, %1, %2, %3" : "=v"(z) : "v"(uz), "v"(wz), "s"(2u * k + 1u));
            z &= m << (2u * k);
            asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(y) : "v"(y), "s"(m << k), "v"(z));
            asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(x) : "v"(x), "s"(m), "v"(y));
            return x;
        }
        const unsigned int g = linear(wrap(ux, wx), wrap(uy, wy), wrap(uz, wz));   // (garbage outside the volume: masked)
        return inside_ ? g : 0u;
    }
    __device__ __forceinline__ short fetch16(const int16_t* __restrict__ vol, unsigned int off) const
    {
        return POW2 ? *(const int16_t*)((const char*)vol + off) : vol[off];
    }
    // offset contribution of storage coordinate t < N along axis AX: t, t N, t N^2
    template <int AX>
    __device__ __forceinline__ unsigned int stride(unsigned int t) const
    {
        if (POW2) return t << ((unsigned int)AX * k);
        return AX == 0 ? t : AX == 1 ? kt_mul24(t, N) : kt_mul24(kt_mul24(t, N), N);
    }
};
#endif

#endif
