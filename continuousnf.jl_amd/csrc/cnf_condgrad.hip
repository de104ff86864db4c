// The gradient w.r.t. the conditioning inputs ys of a conditional model (nn(vcat(z, ys)), src/layers/cond_layer.jl:7-9,
// src/base_icnf.jl:288-309) on the recorded TrainMode routes.  In the reference ys is an array argument like any other and
// Enzyme / Zygote differentiate it; here the discrete adjoint already forms, per stage pullback and sample, the total cotangent
// abar_1 of the first layer's pre-activation a_1 = W_1 [z; ys] + b_1 -- the layer-1 segment of an AB row, whose batch sum
// k_wgrad_* files as bbar_1 -- so the stage's share of d / d ys_b is W_1[:, n_in:]' abar_1[:, b].  ys is constant over the solve:
//
//     gy[b] = W_1[:, n_in:]' S1[b],      S1[b] = sum over all stages of all steps of abar_1[:, b].
//
// k_cond_rowsum forms S1 beside every contraction of a run of steps (a pure stream over the layer-1 segment of the AB rows);
// k_cond_project applies W_1y' once per pullback.  One owner thread per output element, sums in a fixed order, the first run
// stores and later runs add: no atomics, bit-reproducible from run to run.
#include "cnf_condgrad.h"

namespace {

constexpr int CG_THREADS = 256;

// One thread per (sample b, V consecutive features j): the slots in increasing order in a register.  V = 4: 16-byte loads (the
// rows and the layer-1 segment are 16-byte aligned: AdjMfmaLayout::vec4o, and d1 is then a multiple of 4).  Rows are
// [slot B + b] with no padding between slots: nothing past sample B - 1 of a slot is read.
template <int V>
__global__ void __launch_bounds__(CG_THREADS)
k_cond_rowsum(const float* __restrict__ AB, float* __restrict__ S1, int B, int nslots, int sum_out, int off, int d1, int first) {
    const int ng = (d1 + V - 1) / V;
    const size_t t = (size_t)blockIdx.x * CG_THREADS + threadIdx.x;
    if (t >= (size_t)B * ng) return;
    const int b = (int)(t / ng), j = (int)(t % ng) * V;
    const float* p = AB + (size_t)b * sum_out + off + j;
    const size_t stride = (size_t)B * sum_out;
    float* out = S1 + (size_t)b * d1 + j;
    if constexpr (V == 4) {
        float4 acc = first ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(out);
#pragma unroll 6
        for (int s = 0; s < nslots; ++s) {
            const float4 v = *reinterpret_cast<const float4*>(p + (size_t)s * stride);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        *reinterpret_cast<float4*>(out) = acc;
    } else {
        float acc = first ? 0.f : *out;
#pragma unroll 6
        for (int s = 0; s < nslots; ++s) acc += p[(size_t)s * stride];
        *out = acc;
    }
}

// One thread per (b, c), c fastest.  The block W_1y = W_1[:, n_in:] (column n_in + c: d1 contiguous floats in the Lux layout)
// is staged in LDS when it fits, with an odd column stride (lanes of one b walk different columns: different banks).
__global__ void __launch_bounds__(CG_THREADS)
k_cond_project(const float* __restrict__ Wy, const float* __restrict__ S1, float* __restrict__ gy, int B, int n_cond, int d1,
               int in_lds) {
    extern __shared__ float sw[];
    const int ld = in_lds ? (d1 | 1) : d1;
    if (in_lds) {
        for (int e = threadIdx.x; e < n_cond * d1; e += CG_THREADS) sw[(e / d1) * ld + e % d1] = Wy[e];
        __syncthreads();
    }
    const size_t t = (size_t)blockIdx.x * CG_THREADS + threadIdx.x;
    if (t >= (size_t)B * n_cond) return;
    const int b = (int)(t / n_cond), c = (int)(t % n_cond);
    const float* w = (in_lds ? sw : Wy) + (size_t)c * ld;
    const float* s = S1 + (size_t)b * d1;
    float acc = 0.f;
    for (int j = 0; j < d1; ++j) acc = fmaf(w[j], s[j], acc);
    gy[t] = acc;
}

}  // namespace

hipError_t launch_cond_rowsum(const NetDesc& nd, const GradLayout& g, const AdjMfmaLayout& m, const float* AB, float* S1, int B,
                              int nslots, int first, hipStream_t s) {
    const int d1 = nd.dims[1];
    const bool v4 = m.vec4o && (d1 & 3) == 0 && (((uintptr_t)AB | (uintptr_t)S1) & 15) == 0;
    const size_t threads = (size_t)B * (v4 ? d1 / 4 : d1);
    const unsigned blocks = (unsigned)((threads + CG_THREADS - 1) / CG_THREADS);
    if (v4) hipLaunchKernelGGL(k_cond_rowsum<4>, dim3(blocks), dim3(CG_THREADS), 0, s, AB, S1, B, nslots, g.sum_out, g.out_off[0], d1, first);
    else hipLaunchKernelGGL(k_cond_rowsum<1>, dim3(blocks), dim3(CG_THREADS), 0, s, AB, S1, B, nslots, g.sum_out, g.out_off[0], d1, first);
    return hipGetLastError();
}

hipError_t launch_cond_project(const NetDesc& nd, const float* P, const float* S1, float* gy, int B, hipStream_t s) {
    const int d1 = nd.dims[1], n_cond = nd.n_cond;
    const size_t lds = (size_t)n_cond * (d1 | 1) * sizeof(float);
    const int in_lds = lds <= 48 * 1024;
    const size_t threads = (size_t)B * n_cond;
    hipLaunchKernelGGL(k_cond_project, dim3((unsigned)((threads + CG_THREADS - 1) / CG_THREADS)), dim3(CG_THREADS), in_lds ? lds : 0, s,
                       P + nd.w_off[0] + (size_t)nd.n_in * d1, S1, gy, B, n_cond, d1, in_lds);
    return hipGetLastError();
}
