// The library's own counter-based generator: Philox4x32-10 words and their Box-Muller normals,
// drawn straight into device memory -- the Hutchinson probes and base samples the reference draws with the device RNG on a
// GPU resource (rng_AT(::CUDALibs) = CURAND, ext/ContinuousNormalizingFlowsCUDAExt/ContinuousNormalizingFlowsCUDAExt.jl:5-7;
// draws at src/base_icnf.jl:277-278 and :367-370).
//
// Element e of stream (seed, sub) is word e & 3 of the block Philox4x32-10(ctr = (q_lo, q_hi, sub_lo, sub_hi),
// key = (seed_lo, seed_hi)), q = e >> 2; its normal pairs lanes (0, 1) and (2, 3) of that block by Box-Muller, computed in
// double and rounded once; its Rademacher value is +1.0f if bit 31 of its word is 0 and -1.0f if it is 1 (one word per element).
// Every element is a function of (seed, sub, e) alone, so a draw of [o, o + n) equals any split of it into consecutive pieces.
#include "../../include/cnfhip.h"
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;   // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;   // key schedule (Weyl) increments
constexpr int RAND_THREADS = 256;
constexpr int RAND_WG_PER_CU = 4;

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += PHILOX_W0; k1 += PHILOX_W1; }
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c.x, p1 = (uint64_t)PHILOX_M1 * c.z;
        c = make_uint4((uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0);
    }
    return c;
}

// (w_even, w_odd) -> two N(0, 1) floats.  u1 in (0, 1], u2 in [0, 1): in float u1 would round to 1 for w_even near 2^32 and the
// normal would come out as 0 where its true value is up to ~3.5e-4; in double each float is within 1 ulp of the exact function.
__device__ __forceinline__ void box_muller(uint32_t we, uint32_t wo, uint32_t& a, uint32_t& b) {
    const double u1 = ((double)we + 1.0) * 0x1p-32;
    const double u2 = (double)wo * 0x1p-32;
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(2.0 * u2, &s, &c);
    a = __float_as_uint((float)(r * c));
    b = __float_as_uint((float)(r * s));
}

// One counter block per thread and grid-stride step: elements 4q .. 4q+3 land at out[4q - offset ..] where they fall inside
// [offset, last].  Full blocks take one 16-byte store when `vec` says the output is aligned for it (the same for every block).
enum { DRAW_WORDS = 0, DRAW_NORMAL = 1, DRAW_RADEMACHER = 2 };
template <int FORM>
__global__ void __launch_bounds__(RAND_THREADS)
k_draw(uint32_t* __restrict__ out, uint64_t offset, uint64_t last, uint64_t nblk, uint32_t k0, uint32_t k1, uint32_t s0,
       uint32_t s1, int vec) {
    const uint64_t q0 = offset >> 2;
    const uint64_t stride = (uint64_t)gridDim.x * RAND_THREADS;
    for (uint64_t b = (uint64_t)blockIdx.x * RAND_THREADS + threadIdx.x; b < nblk; b += stride) {
        const uint64_t q = q0 + b;
        uint4 w = philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), s0, s1), k0, k1);
        if constexpr (FORM == DRAW_NORMAL) {
            box_muller(w.x, w.y, w.x, w.y);
            box_muller(w.z, w.w, w.z, w.w);
        }
        if constexpr (FORM == DRAW_RADEMACHER) {          // the sign bit of the word under the bits of 1.0f
            constexpr uint32_t one = 0x3F800000u, sign = 0x80000000u;
            w = make_uint4((w.x & sign) | one, (w.y & sign) | one, (w.z & sign) | one, (w.w & sign) | one);
        }
        const uint64_t e0 = q << 2;                       // (e0 + 3 <= 2^64 - 1: no wrap)
        if (e0 >= offset && e0 + 3 <= last) {
            uint32_t* p = out + (e0 - offset);
            if (vec) {
                *reinterpret_cast<uint4*>(p) = w;
            } else {
                p[0] = w.x; p[1] = w.y; p[2] = w.z; p[3] = w.w;
            }
        } else {                                          // the partial first or last block
            const uint32_t v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint64_t e = e0 + j;
                if (e >= offset && e <= last) out[e - offset] = v[j];
            }
        }
    }
}

cnf_status draw(int device, uint64_t seed, uint64_t sub, uint64_t offset, uint32_t* out, size_t n, void* stream, int form) {
    if (n == 0) return CNF_OK;
    if (!out || ((uintptr_t)out & 3u) || (uint64_t)n > UINT64_MAX - offset) return CNF_ERR_BAD_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return CNF_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) return CNF_ERR_BAD_ARG;
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cu <= 0) return CNF_ERR_HIP;
    // the caller's current device is put back: the call leaves no state behind
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) return CNF_ERR_HIP;
    if (prev != device && hipSetDevice(device) != hipSuccess) return CNF_ERR_HIP;

    const uint64_t last = offset + (uint64_t)n - 1;
    const uint64_t nblk = (last >> 2) - (offset >> 2) + 1;
    const uint64_t want = (nblk + RAND_THREADS - 1) / RAND_THREADS;
    const uint64_t cap = (uint64_t)n_cu * RAND_WG_PER_CU;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    // full blocks start at out + 4q - offset: 16-byte aligned for all of them iff out - 4 (offset mod 4) floats is
    const int vec = (((uintptr_t)out - 4u * (uintptr_t)(offset & 3u)) & 15u) == 0;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), s0 = (uint32_t)sub, s1 = (uint32_t)(sub >> 32);
    if (form == DRAW_NORMAL)
        hipLaunchKernelGGL(k_draw<DRAW_NORMAL>, dim3(grid), dim3(RAND_THREADS), 0, (hipStream_t)stream, out, offset, last, nblk, k0, k1,
                           s0, s1, vec);
    else if (form == DRAW_RADEMACHER)
        hipLaunchKernelGGL(k_draw<DRAW_RADEMACHER>, dim3(grid), dim3(RAND_THREADS), 0, (hipStream_t)stream, out, offset, last, nblk,
                           k0, k1, s0, s1, vec);
    else
        hipLaunchKernelGGL(k_draw<DRAW_WORDS>, dim3(grid), dim3(RAND_THREADS), 0, (hipStream_t)stream, out, offset, last, nblk, k0, k1,
                           s0, s1, vec);
    const hipError_t e = hipGetLastError();
    if (prev != device) (void)hipSetDevice(prev);
    return e == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

}  // namespace

extern "C" cnf_status cnf_draw_normal(int device, uint64_t seed, uint64_t subsequence, uint64_t offset, float* out, size_t n,
                                      void* stream) {
    return draw(device, seed, subsequence, offset, reinterpret_cast<uint32_t*>(out), n, stream, DRAW_NORMAL);
}

extern "C" cnf_status cnf_draw_uint32(int device, uint64_t seed, uint64_t subsequence, uint64_t offset, uint32_t* out, size_t n,
                                      void* stream) {
    return draw(device, seed, subsequence, offset, out, n, stream, DRAW_WORDS);
}

// rand!(rng, icnf.epsdist, eps) for Rademacher probes (epsdist, src/base_icnf.jl:22-25; draws at :233-397)
extern "C" cnf_status cnf_draw_rademacher(int device, uint64_t seed, uint64_t subsequence, uint64_t offset, float* out, size_t n,
                                          void* stream) {
    return draw(device, seed, subsequence, offset, reinterpret_cast<uint32_t*>(out), n, stream, DRAW_RADEMACHER);
}
