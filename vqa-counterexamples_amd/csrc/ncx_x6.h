// ncx_x6.h -- what the bf16 x 6 (NCX_F_X6) kernels share: the cut of an fp32 value into three bf16 planes, the fragment types, the
// transposing fragment read and the orders in which the plane products run.  (The LDS row tile of the recurrent kernels is rnn_x6_tile,
// ncx_rnn.h.)
//
// The contract of every X6 kernel.  An fp32 operand element x is cut by truncation into x1 = x & 0xFFFF0000, x2 = (x - x1) & 0xFFFF0000,
// x3 = x - x1 - x2: every residual is exact in fp32 and at most 8 significant bits are left for x3, so x = x1 + x2 + x3 EXACTLY and each
// plane is a bf16 value.  The cut is taken once per element, when its tile is stored to LDS (or, in the fold of k_main_fwd, in
// registers).  Products of bf16 values are exact in fp32; they run on v_mfma_f32_16x16x32_bf16 with fp32 accumulation, small terms first:
//   six products    a1 b3 + a2 b2 + a3 b1 + a1 b2 + a2 b1 + a1 b1 on one accumulator (X6_A / X6_B): a2 b3, a3 b2 and a3 b3 are dropped,
//                   2^-24 relative;
//   eight products  the seven small ones a2 b3 + a3 b2 + a1 b3 + a2 b2 + a3 b1 + a1 b2 + a2 b1 on a second accumulator (X6S_A / X6S_B),
//                   then a1 b1 on the first, the two added when the tile leaves: only a3 b3 is dropped, 2^-32 relative, and the running
//                   sum takes one rounding per k-step at its full magnitude instead of six.
// A non-finite operand value is outside the contract: the cut computes Inf - Inf.
// Which accumulators alternate between two products of one order is each kernel's own business.
#pragma once
#include "ncx_gemm.h"

namespace ncx {

typedef __bf16 x6_bf16x8 __attribute__((ext_vector_type(8)));            // one MFMA operand: 8 k-values of one plane
typedef short x6_s16x4 __attribute__((ext_vector_type(4)));              // what one transposing read returns
typedef unsigned int x6_u32x2 __attribute__((ext_vector_type(2)));       // four bf16 values of one plane: one 8-byte LDS store
typedef __attribute__((address_space(3))) x6_s16x4* x6_lds_s16x4;        // the transposing read's pointer

// (a plane, b plane) of the six products, and of the seven small ones that precede (0, 0) in the eight-product order
constexpr int X6_A[6] = {0, 1, 2, 0, 1, 0}, X6_B[6] = {2, 1, 0, 1, 0, 0};
constexpr int X6S_A[7] = {1, 2, 0, 1, 2, 0, 1}, X6S_B[7] = {2, 1, 2, 1, 0, 1, 0};

// The cut of one value.  x is a scalar: __builtin_bit_cast applied to an element of a vector reads element 0 (hipcc 7.2), so a caller
// that has a vector copies its elements out first.
__device__ __forceinline__ void x6_cut1(float x, unsigned& p1, unsigned& p2, unsigned& p3) {
    p1 = __builtin_bit_cast(unsigned, x) & 0xFFFF0000u;
    const float r1 = x - __builtin_bit_cast(float, p1);
    p2 = __builtin_bit_cast(unsigned, r1) & 0xFFFF0000u;
    const float r2 = r1 - __builtin_bit_cast(float, p2);
    p3 = __builtin_bit_cast(unsigned, r2);                   // (at most 8 significant bits are left: the high half holds them all)
}
// ... of four values into registers: w1, w2, w3 hold plane 1, 2, 3 as packed bf16 pairs (the even element in the low half)
__device__ __forceinline__ void x6_cut4(const float (&x)[4], unsigned (&w1)[2], unsigned (&w2)[2], unsigned (&w3)[2]) {
    unsigned p1[4], p2[4], p3[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) x6_cut1(x[j], p1[j], p2[j], p3[j]);
    // v_perm_b32: the high halves of two dwords -> one dword
    w1[0] = __builtin_amdgcn_perm(p1[1], p1[0], 0x07060302u); w1[1] = __builtin_amdgcn_perm(p1[3], p1[2], 0x07060302u);
    w2[0] = __builtin_amdgcn_perm(p2[1], p2[0], 0x07060302u); w2[1] = __builtin_amdgcn_perm(p2[3], p2[2], 0x07060302u);
    w3[0] = __builtin_amdgcn_perm(p3[1], p3[0], 0x07060302u); w3[1] = __builtin_amdgcn_perm(p3[3], p3[2], 0x07060302u);
}

// ... and to LDS: one 8-byte store per plane, the planes `plane` bytes apart
__device__ __forceinline__ void x6_split_store(f32x4 v, unsigned char* base, int plane) {
    const float x[4] = {v[0], v[1], v[2], v[3]};
    unsigned w1[2], w2[2], w3[2];
    x6_cut4(x, w1, w2, w3);
    *(x6_u32x2*)(base) = x6_u32x2{w1[0], w1[1]}; *(x6_u32x2*)(base + plane) = x6_u32x2{w2[0], w2[1]}; *(x6_u32x2*)(base + 2 * plane) = x6_u32x2{w3[0], w3[1]};
}

// A fragment of an operand that lies in LDS row-is-k (`pitch` bytes per k-row), through ds_read_b64_tr_b16: lane 4 q + r of a 16-lane
// group gives the address of k-row q, columns 4 r .. + 3 of a 4 x 16 block, and lane i receives column i of the four k-rows.  Two reads
// 16 k-rows apart make one 8-deep fragment: lane group lk, whose p points at k-row 4 lk + q, holds k = 4 lk .. + 3 and 16 + 4 lk .. + 3.
__device__ __forceinline__ x6_bf16x8 x6_frag_tr(const unsigned char* p, int pitch) {
    const x6_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((x6_lds_s16x4)(p));
    const x6_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((x6_lds_s16x4)(p + 16 * pitch));
    return __builtin_bit_cast(x6_bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

}  // namespace ncx
