// The float32-exact operand split of the bf16 matrix kernels (conv_igemm.hip explains the arithmetic and its bounds):
// a = a0 + a1 + a2 in three bfloat16 pieces by round-to-nearest remainders, and the six piece products of one k-step.
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split3(const float v, __bf16 &p0, __bf16 &p1, __bf16 &p2) {
    const __bf16 h0 = (__bf16)v;
    const float r1 = v - (float)h0;
    const __bf16 h1 = (__bf16)r1;
    const float r2 = r1 - (float)h1;
    p0 = h0; p1 = h1; p2 = (__bf16)r2;
}

__device__ __forceinline__ void split3(const f32x4 v, bf16x4 &p0, bf16x4 &p1, bf16x4 &p2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        __bf16 h0, h1, h2;
        split3(v[e], h0, h1, h2);
        p0[e] = h0; p1[e] = h1; p2[e] = h2;
    }
}

// Piece product t of a k-step is (piece SPLIT_PA[t] of one operand) x (piece SPLIT_PB[t] of the other): small products first (the
// running sum absorbs them at its own rounding either way)
constexpr int SPLIT_PA[6] = {2, 1, 0, 1, 0, 0}, SPLIT_PB[6] = {0, 1, 2, 0, 1, 0};

// The six piece products of one 16-wide k-step on a wave tile of TM x TN 32 x 32 blocks (af / bf: the three pieces of each block row's
// fragment).  A piece pair sweeps all blocks of the wave tile before the next pair, so MFMAs on one accumulator are TM * TN
// instructions apart.
template <int TM, int TN>
__device__ __forceinline__ void split_mfma6(const bf16x8 (&af)[TM][3], const bf16x8 (&bf)[TN][3], f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][SPLIT_PA[t]], bf[j][SPLIT_PB[t]], acc[i][j], 0, 0, 0);
}
