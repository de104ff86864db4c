// Device helpers of the wave kernels (cnf_wave.hip: k_solve_wave; cnf_tangent.hip: k_tangent_wave): the tile product on
// v_mfma_f32_16x16x4_f32 with register-resident A fragments, the lane sums, and Tsit5's rows as a kernel argument.
#pragma once
#include "cnf_mfma_dev.h"

namespace {

__device__ __forceinline__ f32x4 mm4(const float (&A)[4], const f32x4& b, f32x4 acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[j], b[j], acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ float wv_wave_sum(float v) {            // every lane ends with the same total (fixed tree)
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, true));
    const int i = __float_as_int(v);
    return (__int_as_float(__builtin_amdgcn_readlane(i, 0)) + __int_as_float(__builtin_amdgcn_readlane(i, 16))) +
           (__int_as_float(__builtin_amdgcn_readlane(i, 32)) + __int_as_float(__builtin_amdgcn_readlane(i, 48)));
}
__device__ __forceinline__ float uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// Tsit5 rows a_{s+1, 1..6} by value in the kernel arguments (scalar loads, indexed by the stage of a ROLLED stage loop)
struct WvTab { float a[7][8]; };
static const WvTab kWvTab = {{
    {0, 0, 0, 0, 0, 0, 0, 0},
    {TS_A21, 0, 0, 0, 0, 0, 0, 0},
    {TS_A31, TS_A32, 0, 0, 0, 0, 0, 0},
    {TS_A41, TS_A42, TS_A43, 0, 0, 0, 0, 0},
    {TS_A51, TS_A52, TS_A53, TS_A54, 0, 0, 0, 0},
    {TS_A61, TS_A62, TS_A63, TS_A64, TS_A65, 0, 0, 0},
    {TS_A71, TS_A72, TS_A73, TS_A74, TS_A75, TS_A76, 0, 0}}};

// Sum over the four lanes of a sample (c, c + 16, c + 32, c + 48) on the VALU: v_permlane16_swap / v_permlane32_swap exchange
// rows of 16 / halves of 32 lanes between two registers; with both operands the same value, the two results are the value
// of this lane's row (half) partner pair, so their sum is the pair sum in every lane.  (The ds_bpermute form of
// __shfl_xor is an LDS-crossbar round trip per exchange, six of them per evaluation.)
__device__ __forceinline__ float wv_quad_sum(float v) {
    typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
    u32x2_ r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r.x) + __uint_as_float(r.y);
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}

}  // namespace
