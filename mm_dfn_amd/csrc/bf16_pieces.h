// The bf16-piece primitives of every kernel that carries an fp32 product on the bf16 matrix pipe -- the ONE place where the
// piece arithmetic is defined.
//
// The cut:  x = p1 + p2 + p3  exactly, by TRUNCATION: p1 = the leading 8 significant bits of x (its upper 16 bits as a bf16),
// p2 = those of x - p1, p3 = those of x - p1 - p2 (every difference is exact in fp32; the remainder is O(2^-24 x)).  A product
// is assembled from the six piece products of weight >= 2^-16,
//     a.b ~= a1b1 + a1b2 + a2b1 + a1b3 + a2b2 + a3b1          (dropped: a2b3 + a3b2 + a3b3 <= 2^-23 |a||b|)
// each exact in the fp32 accumulator: fp32-level error at the bf16 MFMA rate (measurements: propagate_split.hip).
//
// Pieces travel packed: a uint32 holds one piece of two consecutive values (the lower index in the lower half), a u32x4 the
// eight bf16 of an MFMA operand.  The mask of the upper 16 bits is an operand of every cut: kernels that keep it in an SGPR
// pass that register (a literal doubles the v_and encoding), the others pass BF16_HI.
//
// The ORDER OF STATEMENTS inside a helper is part of the including kernel's schedule: helpers that do the same arithmetic in
// a different order (cut4 / cut2) are kept apart on purpose, and none of them may be "tidied" without comparing the assembly
// of every kernel that uses it (tools/isa_diff.py).
#pragma once
#include "mmdfn_internal.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
#define LDS_AS(T, p) ((__attribute__((address_space(3))) T*)(p))

constexpr uint32_t BF16_HI = 0xffff0000u;

__device__ __forceinline__ float as_f(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ uint32_t as_u(float f) { return __builtin_bit_cast(uint32_t, f); }

// v_mfma_f32_32x32x16_bf16 / v_mfma_f32_16x16x32_bf16 on packed pieces
__device__ __forceinline__ f32x16 mfma_bf16(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_bf16_16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// four consecutive values -> their three pieces, the four values INTERLEAVED stage by stage (gemm_tn_split_body.h, gru_mfma.hip)
__device__ __forceinline__ void cut4(float x0, float x1, float x2, float x3, uint32_t himask, u32x2& p1, u32x2& p2, u32x2& p3) {
    p1 = u32x2{__builtin_amdgcn_perm(as_u(x1), as_u(x0), 0x07060302u), __builtin_amdgcn_perm(as_u(x3), as_u(x2), 0x07060302u)};
    x0 -= as_f(as_u(x0) & himask); x1 -= as_f(as_u(x1) & himask); x2 -= as_f(as_u(x2) & himask); x3 -= as_f(as_u(x3) & himask);
    p2 = u32x2{__builtin_amdgcn_perm(as_u(x1), as_u(x0), 0x07060302u), __builtin_amdgcn_perm(as_u(x3), as_u(x2), 0x07060302u)};
    x0 -= as_f(as_u(x0) & himask); x1 -= as_f(as_u(x1) & himask); x2 -= as_f(as_u(x2) & himask); x3 -= as_f(as_u(x3) & himask);
    p3 = u32x2{__builtin_amdgcn_perm(as_u(x1), as_u(x0), 0x07060302u), __builtin_amdgcn_perm(as_u(x3), as_u(x2), 0x07060302u)};
}
// eight consecutive values -> the three u32x4 of an MFMA operand, as two interleaved fours
__device__ __forceinline__ void cut8(const float (&v)[8], uint32_t himask, u32x4& p1, u32x4& p2, u32x4& p3) {
    u32x2 a1, a2, a3, b1, b2, b3;
    cut4(v[0], v[1], v[2], v[3], himask, a1, a2, a3);
    cut4(v[4], v[5], v[6], v[7], himask, b1, b2, b3);
    p1 = u32x4{a1.x, a1.y, b1.x, b1.y};
    p2 = u32x4{a2.x, a2.y, b2.x, b2.y};
    p3 = u32x4{a3.x, a3.y, b3.x, b3.y};
}

// two consecutive values -> one packed pair per piece: the same cut ONE PAIR AFTER THE OTHER (the plane kernels)
__device__ __forceinline__ void cut2(float a, float b, uint32_t himask, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
    p1 = __builtin_amdgcn_perm(as_u(b), as_u(a), 0x07060302u);
    a -= as_f(as_u(a) & himask);
    b -= as_f(as_u(b) & himask);
    p2 = __builtin_amdgcn_perm(as_u(b), as_u(a), 0x07060302u);
    a -= as_f(as_u(a) & himask);
    b -= as_f(as_u(b) & himask);
    p3 = __builtin_amdgcn_perm(as_u(b), as_u(a), 0x07060302u);
}
// eight consecutive values -> the three u32x4 of an MFMA operand, pair after pair
__device__ __forceinline__ void cut8_pairs(const float (&x)[8], uint32_t himask, u32x4& p1, u32x4& p2, u32x4& p3) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t q1, q2, q3;
        cut2(x[2 * j], x[2 * j + 1], himask, q1, q2, q3);
        p1[j] = q1;
        p2[j] = q2;
        p3[j] = q3;
    }
}

// the six piece products of one K = 32 step of the 16x16 form, smallest first
__device__ __forceinline__ f32x4 six(const u32x4 (&a)[3], const u32x4 (&b)[3], f32x4 c) {
    c = mfma_bf16_16(a[2], b[0], c);
    c = mfma_bf16_16(a[1], b[0], c);
    c = mfma_bf16_16(a[1], b[1], c);
    c = mfma_bf16_16(a[0], b[2], c);
    c = mfma_bf16_16(a[0], b[1], c);
    c = mfma_bf16_16(a[0], b[0], c);
    return c;
}
