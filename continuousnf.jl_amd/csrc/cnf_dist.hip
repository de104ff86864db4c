// A general Gaussian base distribution (cnf_set_basedist; icnf.basedist, src/base_icnf.jl:16-21): the three launches a handle
// with a non-default base adds to the default path, which itself stays as it is.
//   k_base_post       logpdf(icnf.basedist, z) - dlogp from the final state (src/base_icnf.jl:155, :177-178) and the loss sums
//   k_base_cotangent  d loss / d z(t1) of that log-density: the generalisation of k_final_cotangent (cnf_grad.hip)
//   k_base_sample     rand!(rng, icnf.basedist, new_xs) from standard normals already drawn (src/base_icnf.jl:320-393)
// Four lanes share a sample, as in k_post_state: one sample's row of the final state is contiguous, so the lanes' loads are
// neighbours.  Plain vector code; no LDS beyond the block reduction of the sums, no per-lane arrays.
#include "cnf_dist.h"

namespace {

__device__ __forceinline__ float dist_wave_sum(float v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// |W (z - mean)|^2 of sample row c, summed over the four lanes p = 0..3 of the sample (every lane gets the total)
__device__ __forceinline__ float whitened_sq(const BaseDist& bd, const float* __restrict__ c, int n_in, int p) {
    float ss = 0.f;
    if (bd.kind == 1) {
        for (int i = p; i < n_in; i += 4) {
            const float w = bd.whiten[i] * (c[i] - bd.mean[i]);
            ss = fmaf(w, w, ss);
        }
    } else {
        for (int i = p; i < n_in; i += 4) {          // row i of the lower-triangular W
            const float* wr = bd.whiten + (size_t)i * n_in;
            float w = 0.f;
            for (int j = 0; j <= i; ++j) w = fmaf(wr[j], c[j] - bd.mean[j], w);
            ss = fmaf(w, w, ss);
        }
    }
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    return ss;
}

// Sums: the reduction of k_post_state (cnf_generic.hip) -- fixed tree inside the block, one partial per block, the block that
// draws the last ticket adds the partials in block order -- so the result is the same from run to run.
__global__ void __launch_bounds__(256)
k_base_post(int n_in, int D, BaseDist bd, const StepState* st, const float* U0, const float* U1, float* __restrict__ logpx,
            const float* __restrict__ regs, int B, float* __restrict__ sums5, float* part, unsigned* ticket) {
    const float* fsol = (st && st->cur) ? U1 : U0;
    const int tid = threadIdx.x, p = tid & 3;
    const int b = blockIdx.x * 64 + (tid >> 2);
    const float* c = fsol + (size_t)min(b, B - 1) * D;
    const float ss = whitened_sq(bd, c, n_in, p);
    float v4[4] = {0.f, 0.f, 0.f, 0.f};
    if (b < B && p == 0) {
        v4[0] = fmaf(-0.5f, ss, bd.logconst) - c[n_in];
        v4[1] = regs[b];
        v4[2] = regs[(size_t)B + b];
        v4[3] = regs[2 * (size_t)B + b];
        logpx[b] = v4[0];
    }
    if (!sums5) return;
    __shared__ float sm[4][4];
    __shared__ int last;
    const int w = tid >> 6, l = tid & 63;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float r = dist_wave_sum(v4[j]);
        if (l == 0) sm[j][w] = r;
    }
    __syncthreads();
    if (tid < 4)
        __hip_atomic_store(part + 4 * blockIdx.x + tid, (sm[tid][0] + sm[tid][1]) + (sm[tid][2] + sm[tid][3]),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (tid == 0) {
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = t == gridDim.x - 1;
        if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last) return;
    float r = 0.f;
    for (unsigned i = l; i < gridDim.x; i += 64) r += __hip_atomic_load(part + 4 * i + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    r = dist_wave_sum(r);
    if (l == 0) sums5[w] = r;
    if (tid == 0) sums5[4] = (float)B;
}

// -d logpdf / d z = W' W (z - mean) = prec (z - mean); the lambda3 term as in k_final_cotangent
__global__ void __launch_bounds__(256)
k_base_cotangent(NetDesc nd, int D, BaseDist bd, float lambda3, const float* __restrict__ fsol, float* __restrict__ lam, int B) {
    const int tid = threadIdx.x, p = tid & 3;
    const int b = blockIdx.x * 64 + (tid >> 2);
    const int n_in = nd.n_in;
    const float* c = fsol + (size_t)min(b, B - 1) * D;
    const bool aug = nd.norm_z_aug && nd.naugs > 0;
    float sa = 0.f;
    if (aug) {
        for (int i = nd.nvars + p; i < n_in; i += 4) sa = fmaf(c[i], c[i], sa);
        sa += __shfl_xor(sa, 1, 64);
        sa += __shfl_xor(sa, 2, 64);
    }
    if (b >= B) return;
    const float nrm = sqrtf(sa), inv = 1.0f / (float)B;
    for (int i = p; i < n_in; i += 4) {
        float v;
        if (bd.kind == 1) {
            v = bd.prec[i] * (c[i] - bd.mean[i]);
        } else {
            const float* pr = bd.prec + (size_t)i * n_in;
            v = 0.f;
            for (int j = 0; j < n_in; ++j) v = fmaf(pr[j], c[j] - bd.mean[j], v);
        }
        if (aug && i >= nd.nvars && nrm > 0.f) v = fmaf(lambda3, c[i] / nrm, v);
        lam[(size_t)b * n_in + i] = v * inv;
    }
}

// The general terminal cotangent (cnf_dist.h): k_base_cotangent with the sample's own (cot_l, cot_A) in place of (-1/B, lambda3/B),
// kind 0 included (prec = I, mean = 0), and the [3][B] weights of the scalar rows written by the sample's first lane.
__global__ void __launch_bounds__(256)
k_vjp_cotangent(NetDesc nd, int D, BaseDist bd, int with_A, const float* __restrict__ fsol, const float* __restrict__ cot,
                float* __restrict__ lam, float* __restrict__ cw, int B) {
    const int tid = threadIdx.x, p = tid & 3;
    const int b = blockIdx.x * 64 + (tid >> 2);
    const int n_in = nd.n_in;
    const float* c = fsol + (size_t)min(b, B - 1) * D;
    const bool aug = with_A && nd.norm_z_aug && nd.naugs > 0;
    float sa = 0.f;
    if (aug) {
        for (int i = nd.nvars + p; i < n_in; i += 4) sa = fmaf(c[i], c[i], sa);
        sa += __shfl_xor(sa, 1, 64);
        sa += __shfl_xor(sa, 2, 64);
    }
    if (b >= B) return;
    const float gl = cot[b], gA = aug ? cot[3 * (size_t)B + b] : 0.f;
    const float nrm = sqrtf(sa);
    for (int i = p; i < n_in; i += 4) {
        float v;                                     // -d logpdf / d z_i
        if (bd.kind == 0) {
            v = c[i];
        } else if (bd.kind == 1) {
            v = bd.prec[i] * (c[i] - bd.mean[i]);
        } else {
            const float* pr = bd.prec + (size_t)i * n_in;
            v = 0.f;
            for (int j = 0; j < n_in; ++j) v = fmaf(pr[j], c[j] - bd.mean[j], v);
        }
        v = -gl * v;
        if (aug && i >= nd.nvars && nrm > 0.f) v = fmaf(gA, c[i] / nrm, v);
        lam[(size_t)b * n_in + i] = v;
    }
    if (p == 0) {
        cw[b] = -gl;
        cw[(size_t)B + b] = cot[(size_t)B + b];
        cw[2 * (size_t)B + b] = cot[2 * (size_t)B + b];
    }
}

// z0[b][i] = mean_i + sum_{j <= i} L_ij n[b][j], one lane per entry; the sum runs over j upwards and the mean is added last
__global__ void __launch_bounds__(256)
k_base_sample(int n_in, BaseDist bd, const float* __restrict__ nrm, float* __restrict__ z0, size_t n) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int i = (int)(e % (size_t)n_in);
    if (bd.kind == 1) {
        z0[e] = fmaf(bd.chol[i], nrm[e], bd.mean[i]);
        return;
    }
    const float* row = nrm + (e - (size_t)i);
    const float* lr = bd.chol + (size_t)i * n_in;
    float v = 0.f;
    for (int j = 0; j <= i; ++j) v = fmaf(lr[j], row[j], v);
    z0[e] = v + bd.mean[i];
}

// ---- differentiable sampling (cnf_generate_record / cnf_generate_pullback) ----
// The sample and its log-density from the final state of the reverse solve and the base draw it started from:
//   z_out[b] = rows 1..n_in of fsol[b],   logq[b] = logpdf(base, z0_b) + dlogp_b    (k_base_post's arithmetic at z0, sign +;
//   kind 0: k_post_state's N(0, I)).  Four lanes per sample.
__global__ void __launch_bounds__(256)
k_generate_post(int n_in, int D, BaseDist bd, const float* __restrict__ fsol, const float* __restrict__ z0,
                float* __restrict__ z_out, float* __restrict__ logq, int B) {
    const int tid = threadIdx.x, p = tid & 3;
    const int b = blockIdx.x * 64 + (tid >> 2);
    const size_t bb = (size_t)min(b, B - 1);
    const float* c = fsol + bb * D;
    const float* z = z0 + bb * n_in;
    float ss;
    if (bd.kind == 0) {
        ss = 0.f;
        for (int i = p; i < n_in; i += 4) ss = fmaf(z[i], z[i], ss);
        ss += __shfl_xor(ss, 1, 64);
        ss += __shfl_xor(ss, 2, 64);
    } else {
        ss = whitened_sq(bd, z, n_in, p);
    }
    if (b >= B) return;
    for (int i = p; i < n_in; i += 4) z_out[bb * n_in + i] = c[i];
    if (p == 0) {
        const float log2pi = 1.8378770664093453f;
        const float logpz = bd.kind == 0 ? -0.5f * fmaf((float)n_in, log2pi, ss) : fmaf(-0.5f, ss, bd.logconst);
        logq[b] = logpz + c[n_in];
    }
}

// cnf_generate_many: the same for the M B columns of an ensemble (the members' columns are contiguous: one batch), N(0, I) base;
// only the first n_out = nvars rows of the sample are written, logq (may be null) with k_generate_post's arithmetic.
__global__ void __launch_bounds__(256)
k_generate_post_rows(int n_in, int n_out, int D, const float* __restrict__ fsol, const float* __restrict__ z0,
                     float* __restrict__ x_out, float* __restrict__ logq, size_t B, const int* __restrict__ counts, int Bm) {
    const int tid = threadIdx.x, p = tid & 3;
    const size_t b = (size_t)blockIdx.x * 64 + (tid >> 2);
    size_t bb = b < B ? b : B - 1;
    // heterogeneous members (counts: [M], Bm columns per member): a column at or behind its member's count is neither read nor
    // written -- its lanes read the member's first column for the shuffles and leave
    bool pad = false;
    if (counts) {
        const size_t m = bb / (size_t)Bm;
        pad = bb - m * (size_t)Bm >= (size_t)counts[m];
        if (pad) bb = m * (size_t)Bm;
    }
    const float* c = fsol + bb * D;
    const float* z = z0 + bb * n_in;
    float ss = 0.f;
    for (int i = p; i < n_in; i += 4) ss = fmaf(z[i], z[i], ss);
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    if (b >= B || pad) return;
    for (int i = p; i < n_out; i += 4) x_out[bb * n_out + i] = c[i];
    if (p == 0 && logq) {
        const float log2pi = 1.8378770664093453f;
        logq[b] = -0.5f * fmaf((float)n_in, log2pi, ss) + c[n_in];
    }
}

// The terminal cotangent of sampling: lam = cot_z (null: zeros), and the [3][B] weights of the scalar rows -- +cot_logq (null:
// zeros) on the dlogp row, zero on the E and n rows, which are integrated but are not outputs of sampling.
__global__ void __launch_bounds__(256)
k_generate_cotangent(int n_in, const float* __restrict__ cot_z, const float* __restrict__ cot_logq, float* __restrict__ lam,
                     float* __restrict__ cw, int B) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < (size_t)n_in * B) lam[e] = cot_z ? cot_z[e] : 0.f;
    if (e < (size_t)B) {
        cw[e] = cot_logq ? cot_logq[e] : 0.f;
        cw[(size_t)B + e] = 0.f;
        cw[2 * (size_t)B + e] = 0.f;
    }
}

// grad_z0[b] = lam0[b] + cot_logq[b] d logpdf(base, z0_b) / d z0 = lam0[b] - cot_logq[b] prec (z0_b - mean)   (kind 0: z0_b;
// the expression of k_vjp_cotangent).  One lane per entry; must not alias lam0.  (B: a batch, or the M B columns of an ensemble --
// cnf_generate_vjp_many, N(0, I) base -- as one batch.)
__global__ void __launch_bounds__(256)
k_generate_z0_grad(int n_in, BaseDist bd, const float* __restrict__ lam0, const float* __restrict__ cot_logq,
                   const float* __restrict__ z0, float* __restrict__ gz0, size_t B, const int* __restrict__ counts, int Bm) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n_in * B) return;
    const size_t b = e / (size_t)n_in;
    if (counts) {                                    // heterogeneous members: nothing of a column at or behind its member's count
        const size_t m = b / (size_t)Bm;
        if (b - m * (size_t)Bm >= (size_t)counts[m]) return;
    }
    const int i = (int)(e - b * (size_t)n_in);
    float g = lam0[e];
    if (cot_logq) {
        const float* c = z0 + b * n_in;
        float v;                                     // -d logpdf / d z_i
        if (bd.kind == 0) {
            v = c[i];
        } else if (bd.kind == 1) {
            v = bd.prec[i] * (c[i] - bd.mean[i]);
        } else {
            const float* pr = bd.prec + (size_t)i * n_in;
            v = 0.f;
            for (int j = 0; j < n_in; ++j) v = fmaf(pr[j], c[j] - bd.mean[j], v);
        }
        g = fmaf(-cot_logq[b], v, g);
    }
    gz0[e] = g;
}

// cnf_generate_many / cnf_generate_vjp_many with heterogeneous members: u0 = [z0; 0] of the columns below their member's count
// (one lane per entry of u0; the homogeneous calls do this with a memset and a strided copy of all M B columns)
__global__ void __launch_bounds__(256)
k_ens_u0_counts(int n_in, int D, const float* __restrict__ z0, float* __restrict__ u0, size_t cols, const int* __restrict__ counts, int Bm) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cols * (size_t)D) return;
    const size_t b = e / (size_t)D, m = b / (size_t)Bm;
    const int i = (int)(e - b * (size_t)D);
    if (b - m * (size_t)Bm >= (size_t)counts[m]) return;
    u0[e] = i < n_in ? z0[b * n_in + i] : 0.f;
}

}  // namespace

void launch_ens_u0_counts(int n_in, int D, const float* z0, float* u0, size_t cols, const int* counts, int Bm, hipStream_t s) {
    const size_t n = cols * (size_t)D;
    hipLaunchKernelGGL(k_ens_u0_counts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n_in, D, z0, u0, cols, counts, Bm);
}

void launch_base_post(int n_in, int D, const BaseDist& bd, const StepState* st, const float* U0, const float* U1, float* logpx,
                      const float* regs, int B, float* sums5, float* part, unsigned* ticket, hipStream_t s) {
    hipLaunchKernelGGL(k_base_post, dim3((B + 63) / 64), dim3(256), 0, s, n_in, D, bd, st, U0, U1, logpx, regs, B, sums5, part,
                       ticket);
}

void launch_base_cotangent(const NetDesc& nd, int D, const BaseDist& bd, float lambda3, const float* fsol, float* lam, int B,
                           hipStream_t s) {
    hipLaunchKernelGGL(k_base_cotangent, dim3((B + 63) / 64), dim3(256), 0, s, nd, D, bd, lambda3, fsol, lam, B);
}

void launch_vjp_cotangent(const NetDesc& nd, int D, const BaseDist& bd, int with_A, const float* fsol, const float* cot, float* lam,
                          float* cw, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_vjp_cotangent, dim3((B + 63) / 64), dim3(256), 0, s, nd, D, bd, with_A, fsol, cot, lam, cw, B);
}

void launch_base_sample(int n_in, const BaseDist& bd, const float* normals, float* z0, int B, hipStream_t s) {
    const size_t n = (size_t)n_in * B;
    hipLaunchKernelGGL(k_base_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n_in, bd, normals, z0, n);
}

void launch_generate_post(int n_in, int D, const BaseDist& bd, const float* fsol, const float* z0, float* z_out, float* logq, int B,
                          hipStream_t s) {
    hipLaunchKernelGGL(k_generate_post, dim3((B + 63) / 64), dim3(256), 0, s, n_in, D, bd, fsol, z0, z_out, logq, B);
}

void launch_generate_post_rows(int n_in, int n_out, int D, const float* fsol, const float* z0, float* x_out, float* logq, size_t B,
                               hipStream_t s, const int* counts, int Bm) {
    hipLaunchKernelGGL(k_generate_post_rows, dim3((unsigned)((B + 63) / 64)), dim3(256), 0, s, n_in, n_out, D, fsol, z0, x_out, logq, B,
                       counts, Bm);
}

void launch_generate_cotangent(int n_in, const float* cot_z, const float* cot_logq, float* lam, float* cw, int B, hipStream_t s) {
    const size_t n = (size_t)n_in * B;
    hipLaunchKernelGGL(k_generate_cotangent, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n_in, cot_z, cot_logq, lam, cw, B);
}

void launch_generate_z0_grad(int n_in, const BaseDist& bd, const float* lam0, const float* cot_logq, const float* z0, float* gz0,
                             size_t B, hipStream_t s, const int* counts, int Bm) {
    const size_t n = (size_t)n_in * B;
    hipLaunchKernelGGL(k_generate_z0_grad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n_in, bd, lam0, cot_logq, z0, gz0, B,
                       counts, Bm);
}
