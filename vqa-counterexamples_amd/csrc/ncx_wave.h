// ncx_wave.h -- wave-wide reductions shared by the bandwidth kernels of the forward, backward and loss units.
#pragma once
#include "ncx_internal.h"

namespace ncx {
// Wave-wide reductions on the DPP network (round 3).  __shfl_xor compiles to ds_bpermute_b32 + s_waitcnt: six dependent LDS round
// trips per reduction -- k_train_tail's 24 row dots were 187 of them, ~9 of the kernel's 16 us.  Here: four DPP steps inside each row
// of 16 lanes (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror: every lane then holds its row's result), then the four
// row results through v_readlane.  Fixed association ((quad pairs) half rows) rows: deterministic, the same in every kernel that
// calls it (the fused and unfused paths stay bit-identical to each other).
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float lane_bcast(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_mov<0xB1>(v); v += dpp_mov<0x4E>(v); v += dpp_mov<0x141>(v); v += dpp_mov<0x140>(v);
    return (lane_bcast(v, 0) + lane_bcast(v, 16)) + (lane_bcast(v, 32) + lane_bcast(v, 48));
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_mov<0xB1>(v)); v = fmaxf(v, dpp_mov<0x4E>(v)); v = fmaxf(v, dpp_mov<0x141>(v)); v = fmaxf(v, dpp_mov<0x140>(v));
    return fmaxf(fmaxf(lane_bcast(v, 0), lane_bcast(v, 16)), fmaxf(lane_bcast(v, 32), lane_bcast(v, 48)));
}
// (explicit fma order: k_scores and k_train_tail must round identically)
__device__ __forceinline__ float dot4(const f32x4& a, const f32x4& e) {
    return __builtin_fmaf(a[3], e[3], __builtin_fmaf(a[2], e[2], __builtin_fmaf(a[1], e[1], a[0] * e[0])));
}
}  // namespace ncx
