// Device helpers shared by the step / solve kernels of the headline shape (cnf_step3.hip): the Tsit5 table
// as a kernel argument, the LDS-only barrier, wave reductions, the global weight image of the split kernels and the
// three-piece bf16 operand algebra (split, images, six-term products).
#pragma once
#include "cnf_step3.h"
#include "cnf_split.h"

// Tsit5 rows a_{s+1, 1..6} (s = 1..6), passed BY VALUE as a kernel argument: the stage sums then take their coefficients
// by scalar loads from the argument segment, which every wave has just read (scalar-cache hits).  A __constant__ table
// costs a scalar-cache miss -- a memory round trip -- in front of the first stage of every launch, and select chains
// over immediates put the 21 literals into vector registers.
struct S3Tab { float a[7][8]; };
static const S3Tab kS3Tab = {{
    {0, 0, 0, 0, 0, 0, 0, 0},
    {TS_A21, 0, 0, 0, 0, 0, 0, 0},
    {TS_A31, TS_A32, 0, 0, 0, 0, 0, 0},
    {TS_A41, TS_A42, TS_A43, 0, 0, 0, 0, 0},
    {TS_A51, TS_A52, TS_A53, TS_A54, 0, 0, 0, 0},
    {TS_A61, TS_A62, TS_A63, TS_A64, TS_A65, 0, 0, 0},
    {TS_A71, TS_A72, TS_A73, TS_A74, TS_A75, TS_A76, 0, 0}}};

#define S3_SB() __builtin_amdgcn_sched_barrier(0)
// workgroup barrier for LDS traffic only: does not drain global loads / stores in flight
// (the scheduling fences keep register-only instructions -- MFMAs -- in the interval the source puts them in)
__device__ __forceinline__ void s3_bar() {
    __builtin_amdgcn_sched_barrier(0);
#ifdef S3_ABL_NOBAR
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
    __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ f32x4 s3_tanh4(const f32x4& a) {
#ifdef S3_ABL_NOEPI
    return a * 0.25f;
#endif
    return f32x4{tanh_fast(a.x), tanh_fast(a.y), tanh_fast(a.z), tanh_fast(a.w)};
}
__device__ __forceinline__ f32x4 s3_tanh4_grad(const f32x4& a) {     // the pullbacks: relative accuracy near 0 (tanh_grad)
    return f32x4{tanh_grad(a.x), tanh_grad(a.y), tanh_grad(a.z), tanh_grad(a.w)};
}
__device__ __forceinline__ f32x4 s3_dtanh4(const f32x4& h) {       // sigma' from h
    return f32x4{fmaf(-h.x, h.x, 1.f), fmaf(-h.y, h.y, 1.f), fmaf(-h.z, h.z, 1.f), fmaf(-h.w, h.w, 1.f)};
}
__device__ __forceinline__ float s3_dot4(const f32x4& a, const f32x4& b) {
    return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}
// Sum over the 64 lanes of the wave, fixed tree, on the VALU: four DPP butterflies inside each row of 16 lanes (quad
// swaps, half-row mirror, row mirror: every lane ends with its row's total), then the four row totals through
// v_readlane.  The __shfl_down ladder does the same through the LDS crossbar: six dependent round trips per value.
__device__ __forceinline__ float s3_wave_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, true));   // row_mirror
    const int i = __float_as_int(v);
    return (__int_as_float(__builtin_amdgcn_readlane(i, 0)) + __int_as_float(__builtin_amdgcn_readlane(i, 16))) +
           (__int_as_float(__builtin_amdgcn_readlane(i, 32)) + __int_as_float(__builtin_amdgcn_readlane(i, 48)));
}

// Global image of the two split kernels (bytes).  The register-resident fragments travel in fp32 and are split on arrival
// (2/3 of the bytes of three bf16 pieces; the split runs while the rest of the stream is in flight).  Fragment = the 8
// weights M[16 tile + x][32 k-block + 8q .. +7] of lane 16q + x, as two 16-byte halves: [half 2][lane 64] x 16 B.
namespace s3g {
constexpr int BIASB = 0;                                   // b1 (128), b2 (128), b3 (32) fp32
constexpr int F32 = (2 * 128 + 32) * 4;                    // [wave 8][W1 | W2 x4 | W3^T | W2^T x4], then W3: [tile 2][k-block 4]
constexpr int NFR = 8 * 10 + 2 * 4;
constexpr int W3I = F32 + NFR * 2048;                      // k_step3b's LDS images (three bf16 pieces, LDS layout): W3 rows, W1^T rows
constexpr int WI = 3 * 32 * 256;
constexpr int IMG_BYTES = W3I + 2 * WI;
static_assert(F32 % 16 == 0 && W3I % 16 == 0, "16-byte loads");
}  // namespace s3g

// 4 rows of one sample -> the three images (8 bytes each)
typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void s3b_store4(char* img, int piece_bytes, const f32x4& v) {
#ifdef S3_ABL_NOSTORE
    { asm volatile("" :: "v"(v), "v"((unsigned)(size_t)img)); return; }
#endif
    u32x2_ h, m, l;
    { unsigned h_, m_, l_; s3b_split2(v[0], v[1], h_, m_, l_); h.x = h_; m.x = m_; l.x = l_; }
    { unsigned h_, m_, l_; s3b_split2(v[2], v[3], h_, m_, l_); h.y = h_; m.y = m_; l.y = l_; }
    *(u32x2_*)img = h; *(u32x2_*)(img + piece_bytes) = m; *(u32x2_*)(img + 2 * piece_bytes) = l;
}
struct S3bOp { bf16x8 h, m, l; };
__device__ __forceinline__ S3bOp s3b_load(const char* img, int piece_bytes) {
    S3bOp o;
#ifdef S3_ABL_NOLOAD
    { typedef unsigned u4_ __attribute__((ext_vector_type(4))); u4_ z = {0x3c003c00u, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u}; asm volatile("" : "+v"(z) : "v"((unsigned)(size_t)img));
      o.h = o.m = o.l = __builtin_bit_cast(bf16x8, z); return o; }
#endif
    o.h = *(const bf16x8*)img; o.m = *(const bf16x8*)(img + piece_bytes); o.l = *(const bf16x8*)(img + 2 * piece_bytes);
    return o;
}
// 8 consecutive fp32 values -> a split operand
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ S3bOp s3b_split8(const f32x4& lo4, const f32x4& hi4) {
    u32x4 h, m, l;
    { unsigned h_, m_, l_; s3b_split2(lo4[0], lo4[1], h_, m_, l_); h.x = h_; m.x = m_; l.x = l_; }
    { unsigned h_, m_, l_; s3b_split2(lo4[2], lo4[3], h_, m_, l_); h.y = h_; m.y = m_; l.y = l_; }
    { unsigned h_, m_, l_; s3b_split2(hi4[0], hi4[1], h_, m_, l_); h.z = h_; m.z = m_; l.z = l_; }
    { unsigned h_, m_, l_; s3b_split2(hi4[2], hi4[3], h_, m_, l_); h.w = h_; m.w = m_; l.w = l_; }
    S3bOp o;
    o.h = __builtin_bit_cast(bf16x8, h); o.m = __builtin_bit_cast(bf16x8, m); o.l = __builtin_bit_cast(bf16x8, l);
    return o;
}
// an ordered no-op that consumes and redefines the operand: pins its computation in program order
__device__ __forceinline__ void s3b_pin(S3bOp& o) {
    u32x4 a = __builtin_bit_cast(u32x4, o.h), b = __builtin_bit_cast(u32x4, o.m), c = __builtin_bit_cast(u32x4, o.l);
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c));
    o.h = __builtin_bit_cast(bf16x8, a); o.m = __builtin_bit_cast(bf16x8, b); o.l = __builtin_bit_cast(bf16x8, c);
}
// term T (0..5, smallest first) of the product a x b into acc
template <int T>
__device__ __forceinline__ f32x4 s3b_term(const S3bOp& a, const S3bOp& b, const f32x4& acc) {
#ifdef S3_ABL_NOMFMA
    { u32x4 x = __builtin_bit_cast(u32x4, a.h), y = __builtin_bit_cast(u32x4, b.h); asm volatile("" :: "v"(x), "v"(y)); return acc; }
#endif
    if (T == 0) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.l, b.h, acc, 0, 0, 0);
    if (T == 1) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.l, acc, 0, 0, 0);
    if (T == 2) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.m, acc, 0, 0, 0);
    if (T == 3) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.h, acc, 0, 0, 0);
    if (T == 4) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.m, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.h, acc, 0, 0, 0);
}
// NC independent products that share the A operand: term-major order, so that the six terms of one accumulator are NC
// MFMAs apart
template <int NC>
__device__ __forceinline__ void s3b_mm(f32x4 (&acc)[NC], const S3bOp& a, const S3bOp (&b)[NC]) {
#pragma unroll
    for (int n = 0; n < NC; ++n) acc[n] = s3b_term<0>(a, b[n], acc[n]);
#pragma unroll
    for (int n = 0; n < NC; ++n) acc[n] = s3b_term<1>(a, b[n], acc[n]);
#pragma unroll
    for (int n = 0; n < NC; ++n) acc[n] = s3b_term<2>(a, b[n], acc[n]);
#pragma unroll
    for (int n = 0; n < NC; ++n) acc[n] = s3b_term<3>(a, b[n], acc[n]);
#pragma unroll
    for (int n = 0; n < NC; ++n) acc[n] = s3b_term<4>(a, b[n], acc[n]);
#pragma unroll
    for (int n = 0; n < NC; ++n) acc[n] = s3b_term<5>(a, b[n], acc[n]);
}

// A narrow product (K = 128, four k-blocks) of a wave that is ALONE on its SIMD: rows `A` x rows `B` of two split images
// (+ (rd ^ 64 kb): k-block kb), on two accumulation chains (terms 0-2 / 3-5), k-blocks ascending.  No other wave covers an
// LDS round trip there, so the wave covers its own: the operands of k-block kb + 1 are requested in front of the MFMAs of
// k-block kb (the compiler's counted lgkmcnt waits then leave them in flight), and `a0`, the A operand of k-block 0, comes
// from the caller, who requests it in FRONT of the barrier that publishes B -- the A images are constant for the solve.
// `tail()` is issued behind the last operand request, in front of the last k-block's MFMAs: reads the caller's epilogue
// needs that do not depend on the product.
template <class Tail>
__device__ __forceinline__ void s3b_narrow(f32x4& z0, f32x4& z1, const S3bOp& a0, const char* A, const char* B, int rd,
                                           int piece_bytes, Tail&& tail) {
    S3bOp av = a0, bv = s3b_load(B + rd, piece_bytes);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
        S3bOp an = av, bn = bv;
        if (kb < 3) {
            an = s3b_load(A + (rd ^ (64 * (kb + 1))), piece_bytes);
            bn = s3b_load(B + (rd ^ (64 * (kb + 1))), piece_bytes);
        } else {
            tail();
        }
        S3_SB();
        z0 = s3b_term<0>(av, bv, z0); z1 = s3b_term<3>(av, bv, z1);
        z0 = s3b_term<1>(av, bv, z0); z1 = s3b_term<4>(av, bv, z1);
        z0 = s3b_term<2>(av, bv, z0); z1 = s3b_term<5>(av, bv, z1);
        // Both chains are pinned to their k-block: an MFMA has no side effect, so instruction selection is free to emit it
        // anywhere behind its operands, whatever the scheduling fences say -- left alone, the second chain's twelve MFMAs
        // are emitted as one dependent run BEHIND the loop, with the operands of all four k-blocks (96 VGPRs) held for it.
        asm volatile("" : "+v"(z0), "+v"(z1));
        S3_SB();
        av = an; bv = bn;
    }
}

// A wide product (K = 128, four k-blocks) of a wave that owns one 16-row tile of BOTH sample halves: the resident A
// fragments `w` x the rows at `B0` (half a, into acc[0]) and at `B1` (half b, into acc[1]) of a split image.  The halves run
// one after the other -- a single accumulation chain of this MFMA issues at full rate -- so that half a's epilogue (bias,
// activation, the three-piece split, the stores) has half b's 24 MFMAs to hide under: an MFMA holds vector issue for half
// of its 16 cycles, and interleaved term-major both accumulators finish on the last two MFMAs of the interval, with the
// matrix pipe empty under the whole epilogue.  Each accumulator takes the same MFMAs on the same operands in the same
// order as in s3b_mm<2> per k-block: k-blocks ascending, terms 0 to 5.
// Operands are requested one k-block ahead across both halves, as in s3b_narrow, and nothing is drained inside.  The
// caller places its own instructions through `at`, called with S3C<i>:
//   i = -2            in front of the last k-block of half a, behind its operand requests (reads that half a's epilogue needs)
//   i = -1            half a's last MFMA is issued
//   i = 0 .. 23       behind MFMA i of half b: a group of half a's epilogue, at most about three instructions' worth of
//                     issue (a transcendental counts as two).  A group stays where it is put only if the caller pins what
//                     it computes (s3_hold): see the comment in s3b_narrow on what the scheduling fences do not hold.
//   i = 24            half b's last MFMA is issued
// Half b's epilogue is the caller's, behind the call.
template <int I> struct S3C { static constexpr int value = I; };
__device__ __forceinline__ void s3_hold(float& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void s3_hold(unsigned& x) { asm volatile("" : "+v"(x)); }
template <int KB, class At>
__device__ __forceinline__ void s3b_wide_b(f32x4& acc, const S3bOp& a, const S3bOp& b, At& at) {
    acc = s3b_term<0>(a, b, acc); asm volatile("" : "+v"(acc)); at(S3C<6 * KB + 0>{}); S3_SB();
    acc = s3b_term<1>(a, b, acc); asm volatile("" : "+v"(acc)); at(S3C<6 * KB + 1>{}); S3_SB();
    acc = s3b_term<2>(a, b, acc); asm volatile("" : "+v"(acc)); at(S3C<6 * KB + 2>{}); S3_SB();
    acc = s3b_term<3>(a, b, acc); asm volatile("" : "+v"(acc)); at(S3C<6 * KB + 3>{}); S3_SB();
    acc = s3b_term<4>(a, b, acc); asm volatile("" : "+v"(acc)); at(S3C<6 * KB + 4>{}); S3_SB();
    acc = s3b_term<5>(a, b, acc); asm volatile("" : "+v"(acc)); at(S3C<6 * KB + 5>{}); S3_SB();
}
template <class At>
__device__ __forceinline__ void s3b_wide(f32x4 (&acc)[2], const S3bOp (&w)[4], const char* B0, const char* B1, int rd,
                                         int piece_bytes, At&& at) {
    S3bOp bv = s3b_load(B0 + rd, piece_bytes), bn;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {                                   // half a
        bn = s3b_load((kb < 3 ? B0 : B1) + (rd ^ (64 * ((kb + 1) & 3))), piece_bytes);
        if (kb == 3) at(S3C<-2>{});
        S3_SB();
        acc[0] = s3b_term<0>(w[kb], bv, acc[0]); acc[0] = s3b_term<1>(w[kb], bv, acc[0]); acc[0] = s3b_term<2>(w[kb], bv, acc[0]);
        acc[0] = s3b_term<3>(w[kb], bv, acc[0]); acc[0] = s3b_term<4>(w[kb], bv, acc[0]); acc[0] = s3b_term<5>(w[kb], bv, acc[0]);
        asm volatile("" : "+v"(acc[0]));                               // pinned to its k-block (s3b_narrow)
        S3_SB();
        bv = bn;
    }
    at(S3C<-1>{});
    S3_SB();
    // half b: every MFMA is a group of its own, with the caller's instructions behind it
    bn = s3b_load(B1 + (rd ^ 64), piece_bytes); S3_SB(); s3b_wide_b<0>(acc[1], w[0], bv, at); bv = bn;
    bn = s3b_load(B1 + (rd ^ 128), piece_bytes); S3_SB(); s3b_wide_b<1>(acc[1], w[1], bv, at); bv = bn;
    bn = s3b_load(B1 + (rd ^ 192), piece_bytes); S3_SB(); s3b_wide_b<2>(acc[1], w[2], bv, at); bv = bn;
    s3b_wide_b<3>(acc[1], w[3], bv, at);
    at(S3C<24>{});
}
// tanh_fast's three dependent steps, for epilogues placed by hand (s3_tanh4 is their composition per value)
__device__ __forceinline__ float s3_tanh_exp(float a) {
#ifdef S3_ABL_NOEPI
    return a * 0.25f;
#endif
    return tanh_fast_exp(a);
}
__device__ __forceinline__ float s3_tanh_rcp(float t) {
#ifdef S3_ABL_NOEPI
    return t;
#endif
    return tanh_fast_rcp(t);
}
__device__ __forceinline__ float s3_tanh_out(float r) {
#ifdef S3_ABL_NOEPI
    return r;
#endif
    return tanh_fast_out(r);
}
// s3b_store4 in groups to place by hand: `v` holds the four values and ends as scratch; group G (0 .. 11) is
//   pair P = G / 6 (values 2P, 2P + 1), step G % 6:  0 leading piece | 1, 2 what each value keeps | 3 middle piece, what
//   value 2P keeps | 4 what value 2P + 1 keeps | 5 last piece
// (issue weights 1, 2, 2, 3, 2, 1: a remainder is a widening and a subtraction), then s3b_store4s_put<0 .. 2> stores piece h, m, l.
struct S3bStore4s { u32x2_ h, m, l; };
template <int G>
__device__ __forceinline__ void s3b_store4s_step(S3bStore4s& st, float (&v)[4]) {
    constexpr int P = G / 6, S = G % 6;
    unsigned h = st.h[P], m = st.m[P], l = st.l[P];
    float v0 = v[2 * P], v1 = v[2 * P + 1];
    if (S == 0) { h = s3b_split2_lead(v0, v1); s3_hold(h); }
    if (S == 1) { v0 = s3b_split2_rest<0>(v0, h); s3_hold(v0); }
    if (S == 2) { v1 = s3b_split2_rest<1>(v1, h); s3_hold(v1); }
    if (S == 3) { m = s3b_split2_lead(v0, v1); v0 = s3b_split2_rest<0>(v0, m); s3_hold(m); s3_hold(v0); }
    if (S == 4) { v1 = s3b_split2_rest<1>(v1, m); s3_hold(v1); }
    if (S == 5) { l = s3b_split2_last(v0, v1); s3_hold(l); }
    st.h[P] = h; st.m[P] = m; st.l[P] = l; v[2 * P] = v0; v[2 * P + 1] = v1;
}
// Groups 1, 2 (7, 8) where value J is a product a * b formed for this store: what it keeps of the UNROUNDED product.  That is
// what s3b_store4(a * b) computes -- under -ffp-contract=fast the compiler folds the product into the first subtraction of the
// split -- and the bits of every build so far; a group placed by hand has to say so.
template <int J>
__device__ __forceinline__ void s3b_store4s_rest_of_product(const S3bStore4s& st, float (&v)[4], float a, float b) {
#ifdef S3_ABL_NOEPI
    v[J] = 0.f; return;
#endif
    const unsigned p = st.h[J / 2];
    v[J] = fmaf(a, b, -__uint_as_float(J & 1 ? p & 0xFFFF0000u : p << 16));
    s3_hold(v[J]);
}
template <int PIECE>
__device__ __forceinline__ void s3b_store4s_put(const S3bStore4s& st, char* img, int piece_bytes) {
#ifdef S3_ABL_NOSTORE
    { asm volatile("" :: "v"(st.h), "v"((unsigned)(size_t)img)); return; }
#endif
    *(u32x2_*)(img + PIECE * piece_bytes) = PIECE == 0 ? st.h : (PIECE == 1 ? st.m : st.l);
}

// 4 rows of one sample back from the three images: the pieces sum to the fp32 value exactly
// (request, then per value the low sum and the value: three steps a caller can place by hand)
struct S3bPieces4 { bf16x4 h, m, l; };
__device__ __forceinline__ S3bPieces4 s3b_load4_request(const char* img, int piece_bytes) {
    return S3bPieces4{*(const bf16x4*)img, *(const bf16x4*)(img + piece_bytes), *(const bf16x4*)(img + 2 * piece_bytes)};
}
__device__ __forceinline__ float s3b_load4_low(const S3bPieces4& p, int j) { return (float)p.m[j] + (float)p.l[j]; }
__device__ __forceinline__ float s3b_load4_value(const S3bPieces4& p, int j, float low) { return (float)p.h[j] + low; }
__device__ __forceinline__ f32x4 s3b_load4_values(const S3bPieces4& p) {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = s3b_load4_value(p, j, s3b_load4_low(p, j));
    return v;
}
__device__ __forceinline__ f32x4 s3b_load4(const char* img, int piece_bytes) {
    return s3b_load4_values(s3b_load4_request(img, piece_bytes));
}

