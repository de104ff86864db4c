// The exact three-piece bf16 split behind the six-term products (cnf_step3.hip, cnf_grad.hip).
#pragma once
#include <hip/hip_runtime.h>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// v = h + m + l exactly.  Round 2 took the pieces by TRUNCATION (one AND each: the upper 16 bits of an fp32 are a bf16;
// residuals by exact subtractions; the last residual has at most 8 significant bits, so its upper half is all of it):
// -DCNF_SPLIT_TRUNC builds still do.  The kernels split pairs by round-to-nearest now, which is as cheap and keeps the
// dropped terms below 2^-23 |a b| in the worst case instead of 2^-21.

// The split by ROUND-TO-NEAREST pieces, two values at a time (v_cvt_pk_bf16_f32 converts a pair and packs it):
// |m| <= 2^-8 ulp-units, |l| <= 2^-17, so the three products a six-term product leaves out (m l, l m, l l) stay below
// 2^-24 |a b| for EVERY input, where truncated pieces reach 2^-21 |a b| when every mantissa bit is set
// (tests/test_gpu_parity.py::test_split_product_error_bound).  Still exact: v - h has at most 16 significant bits,
// (v - h) - m at most 8.  Same instruction count as the truncating form (per pair: 3 converts, 4 widenings, 4 subtractions
// against 4 ANDs, 4 subtractions, 3 packs).  -DCNF_SPLIT_TRUNC selects the truncating form (A/B).
typedef float f32x2_ __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
// The split is three dependent steps, kept apart so that a caller can place each one by hand among other instructions
// (s3b_wide): the packed leading piece of a pair, the exact remainder of either value, and the packed last piece.
__device__ __forceinline__ unsigned s3b_split2_lead(float v0, float v1) {
#if defined(S3_ABL_NOEPI) || defined(CNF_SPLIT_TRUNC)
    return (__float_as_uint(v0) >> 16) | (__float_as_uint(v1) & 0xFFFF0000u);
#else
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2_{v0, v1}, bf16x2_));
#endif
}
template <int HI>     // what value HI (0 / 1) of the pair keeps once its packed leading piece `p` is taken off
__device__ __forceinline__ float s3b_split2_rest(float v, unsigned p) {
#ifdef S3_ABL_NOEPI
    return 0.f;
#endif
    return v - __uint_as_float(HI ? p & 0xFFFF0000u : p << 16);
}
__device__ __forceinline__ unsigned s3b_split2_last(float v0, float v1) {
#ifdef S3_ABL_NOEPI
    return 0u;
#endif
    return s3b_split2_lead(v0, v1);
}
__device__ __forceinline__ void s3b_split2(float v0, float v1, unsigned& h2, unsigned& m2, unsigned& l2) {
    h2 = s3b_split2_lead(v0, v1);
    const float r0 = s3b_split2_rest<0>(v0, h2), r1 = s3b_split2_rest<1>(v1, h2);
    m2 = s3b_split2_lead(r0, r1);
    const float q0 = s3b_split2_rest<0>(r0, m2), q1 = s3b_split2_rest<1>(r1, m2);
    l2 = s3b_split2_last(q0, q1);
}
