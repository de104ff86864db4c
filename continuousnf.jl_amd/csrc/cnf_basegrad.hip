// The gradient w.r.t. the base distribution's mean and Cholesky factor (cnf_basegrad.h).  N(mean, L L'), W = inv(L),
// n_b = W (z_b - mean):
//     logpdf(z_b)                    = -sum_i log L_ii - n_in / 2 log(2 pi) - 1/2 |n_b|^2
//     d/d mean sum_b w_b logpdf(z_b) =  W' sum_b w_b n_b
//     d/d L    sum_b w_b logpdf(z_b) =  tril(W' sum_b w_b n_b n_b') - (sum_b w_b) diag(1 / L_ii)
// and the pullback of the draw z0_b = mean + L n_b is  g_mean = sum_b g_b,  g_L = tril(sum_b g_b n_b').  Both are the batch
// contraction  m = sum_b w_b a_b,  M = sum_b w_b a_b n_b'  and a tail that needs the base only:
//   k_bg_whiten    n_b = W (s_b - mean) per sample, the arithmetic of k_base_post (log-density direction only)
//   k_bg_contract  one workgroup per (chunk of samples, 16 x 16 tile of M); dense kind at n_in >= 16 on v_mfma_f32_16x16x4_f32
//                  with K = samples, the diagonal kind and n_in < 16 on the vector unit.  The partial of every chunk goes to
//                  the handle's buffer, and the workgroup that draws a tile's last ticket adds the tile's partials in chunk
//                  order (k_post_state's pattern): no float atomics, the same bits from run to run.
//   k_bg_tail      (m, M, sum w) -> (g_mean, g_chol) in the layout cnf_set_basedist takes chol in
#include "cnf_basegrad.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
enum { BG_MFMA = 0, BG_VALU_DENSE = 1, BG_VALU_DIAG = 2 };

// rows[b][i] = sum_{j <= i} W_ij (src[b][j] - mean_j), one lane per entry, j upwards (whitened_sq of cnf_dist.hip)
__global__ void __launch_bounds__(256)
k_bg_whiten(int n_in, BaseDist bd, const float* __restrict__ src, int stride, float* __restrict__ rows, size_t n) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const size_t b = e / (size_t)n_in;
    const int i = (int)(e - b * (size_t)n_in);
    const float* c = src + b * (size_t)stride;
    if (bd.kind == 1) {
        rows[e] = bd.whiten[i] * (c[i] - bd.mean[i]);
        return;
    }
    const float* wr = bd.whiten + (size_t)i * n_in;
    float w = 0.f;
    for (int j = 0; j <= i; ++j) w = fmaf(wr[j], c[j] - bd.mean[j], w);
    rows[e] = w;
}

// tile index -> (ti, tj), ti >= tj, tile = ti (ti + 1) / 2 + tj
__device__ __forceinline__ void bg_tile(int tile, int& ti, int& tj) {
    ti = (int)((sqrtf(8.0f * (float)tile + 1.0f) - 1.0f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
    while (ti * (ti + 1) / 2 > tile) --ti;
    tj = tile - ti * (ti + 1) / 2;
}

// A: rows a_b (sa floats per sample), N: rows n_b (sn floats per sample), w: per-sample weights or null (ones).
// grid (nchunks, ntiles), 256 threads.  buf: BaseGradPlan.
template <int PATH>
__global__ void __launch_bounds__(256)
k_bg_contract(int n_in, const float* __restrict__ A, int sa, const float* __restrict__ N, int sn, const float* __restrict__ w,
              int B, int chunk, unsigned* tickets, float* result, float* part) {
    __shared__ float sm[4][BG_REC];
    __shared__ int last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.y, ntiles = gridDim.y;
    const int b0 = blockIdx.x * chunk, b1 = min(B, b0 + chunk);
    int ti, tj;
    if (PATH == BG_VALU_DIAG) ti = tj = tile;
    else bg_tile(tile, ti, tj);
    for (int e = tid; e < 4 * BG_REC; e += 256) (&sm[0][0])[e] = 0.f;
    __syncthreads();

    if (PATH == BG_MFMA) {
        // lane (x, q): A operand = w_b a_b[16 ti + x], B operand = n_b[16 tj + x] of sample b = k-block's first + q;
        // accumulator register j = M[16 ti + 4 q + j][16 tj + x].  A wave takes every fourth k-block of the chunk; two
        // accumulators so that consecutive products do not wait for each other.
        const int x = lane & 15, q = lane >> 4;
        const int ra = 16 * ti + x, rn = 16 * tj + x;
        const bool va = ra < n_in, vn = rn < n_in;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f}, am0 = {0.f, 0.f, 0.f, 0.f}, am1 = {0.f, 0.f, 0.f, 0.f};
        auto operands = [&](int b, float& a, float& n, float& one) {
            const bool vb = b < b1;
            one = vb ? 1.f : 0.f;
            a = (vb && va) ? (w ? w[b] : 1.f) * A[(size_t)b * sa + ra] : 0.f;
            n = (vb && vn) ? N[(size_t)b * sn + rn] : 0.f;
        };
        for (int k = b0 + 4 * wave; k < b1; k += 32) {
            float a0, n0, o0, a1, n1, o1;
            operands(k + q, a0, n0, o0);
            operands(k + 16 + q, a1, n1, o1);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, n0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, n1, acc1, 0, 0, 0);
            if (tj == 0) {                                   // m: the same product against a column of ones
                am0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, o0, am0, 0, 0, 0);
                am1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, o1, am1, 0, 0, 0);
            }
        }
        acc0 += acc1;
        am0 += am1;
#pragma unroll
        for (int j = 0; j < 4; ++j) sm[wave][16 * (4 * q + j) + x] = acc0[j];
        if (tj == 0 && x == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) sm[wave][BG_M + 4 * q + j] = am0[j];
        }
    } else if (PATH == BG_VALU_DENSE) {
        // n_in < 16: the one tile, thread (r, c) owns M[r][c] and walks the chunk in order
        const int r = tid >> 4, c = tid & 15;
        if (r < n_in && c <= r) {
            float acc = 0.f, am = 0.f;
            for (int b = b0; b < b1; ++b) {
                const float a = (w ? w[b] : 1.f) * A[(size_t)b * sa + r];
                acc = fmaf(a, N[(size_t)b * sn + c], acc);
                am += a;
            }
            sm[0][16 * r + c] = acc;
            if (c == 0) sm[0][BG_M + r] = am;
        }
    } else {
        // diagonal kind: thread (x, r) owns entry 16 tile + x for the samples b0 + r, b0 + r + 16, ...
        const int x = tid & 15, r = tid >> 4, i = 16 * tile + x;
        float acc = 0.f, am = 0.f;
        if (i < n_in)
            for (int b = b0 + r; b < b1; b += 16) {
                const float a = (w ? w[b] : 1.f) * A[(size_t)b * sa + i];
                acc = fmaf(a, N[(size_t)b * sn + i], acc);
                am += a;
            }
        __shared__ float sd[2][16][17];
        sd[0][r][x] = acc;
        sd[1][r][x] = am;
        __syncthreads();
        if (tid < 32) {
            const int which = tid >> 4, xx = tid & 15;
            float t = 0.f;
            for (int rr = 0; rr < 16; ++rr) t += sd[which][rr][xx];
            sm[0][(which ? BG_M : 0) + xx] = t;
        }
    }
    if (tile == 0 && wave == 0) {                            // sum_b w_b: one wave, a fixed tree
        float sw = 0.f;
        for (int b = b0 + lane; b < b1; b += 64) sw += w ? w[b] : 1.f;
        for (int off = 32; off > 0; off >>= 1) sw += __shfl_down(sw, off, 64);
        if (lane == 0) sm[0][BG_W] = sw;
    }
    __syncthreads();
    float* mine = part + ((size_t)blockIdx.x * ntiles + tile) * BG_REC;
    for (int e = tid; e < BG_REC; e += 256)
        __hip_atomic_store(mine + e, (sm[0][e] + sm[1][e]) + (sm[2][e] + sm[3][e]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (tid == 0) {
        const unsigned t = __hip_atomic_fetch_add(tickets + tile, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = t == gridDim.x - 1;
        if (last) __hip_atomic_store(tickets + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last) return;
    for (int e = tid; e < BG_REC; e += 256) {
        float r = 0.f;
        for (unsigned c = 0; c < gridDim.x; ++c)
            r += __hip_atomic_load(part + ((size_t)c * ntiles + tile) * BG_REC + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        result[(size_t)tile * BG_REC + e] = r;
    }
}

__device__ __forceinline__ float bg_M(const float* __restrict__ result, int k, int j) {      // M[k][j], k >= j
    const int ti = k >> 4, tj = j >> 4;
    return result[(size_t)(ti * (ti + 1) / 2 + tj) * BG_REC + 16 * (k & 15) + (j & 15)];
}
__device__ __forceinline__ float bg_m(const float* __restrict__ result, int k, int kind) {
    const int ti = k >> 4;
    return result[(size_t)(kind == 1 ? ti : ti * (ti + 1) / 2) * BG_REC + BG_M + (k & 15)];
}

// One thread per output entry: e < n_in -> g_mean[e], then g_chol.  logpdf != 0: the W' products and the log-determinant term;
// else the plain copy tril(M) of the sample pullback.  The sums run over k upwards.
__global__ void __launch_bounds__(256)
k_bg_tail(int n_in, int kind, int logpdf, BaseDist bd, const float* __restrict__ result, float* __restrict__ g_mean,
          float* __restrict__ g_chol) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)n_in + (kind == 1 ? (size_t)n_in : (size_t)n_in * n_in);
    if (e >= total) return;
    const float sw = result[BG_W];
    if (e < (size_t)n_in) {
        const int i = (int)e;
        float v;
        if (!logpdf) v = bg_m(result, i, kind);
        else if (kind == 1) v = bd.whiten[i] * bg_m(result, i, kind);
        else {
            v = 0.f;
            for (int k = i; k < n_in; ++k) v = fmaf(bd.whiten[(size_t)k * n_in + i], bg_m(result, k, kind), v);
        }
        g_mean[i] = v;
        return;
    }
    const size_t o = e - n_in;
    if (kind == 1) {
        const int i = (int)o;
        const float d = result[(size_t)(i >> 4) * BG_REC + (i & 15)];
        g_chol[i] = logpdf ? (d - sw) * bd.whiten[i] : d;
        return;
    }
    const int i = (int)(o / (size_t)n_in), j = (int)(o % (size_t)n_in);
    float v = 0.f;
    if (j <= i) {
        if (!logpdf) v = bg_M(result, i, j);
        else {
            for (int k = i; k < n_in; ++k) v = fmaf(bd.whiten[(size_t)k * n_in + i], bg_M(result, k, j), v);
            if (i == j) v -= sw / bd.chol[(size_t)i * n_in + i];
        }
    }
    g_chol[o] = v;
}

hipError_t contract_and_tail(int n_in, int kind, int logpdf, const BaseDist& bd, const float* A, int sa, const float* N, int sn,
                             const float* w, int B, float* buf, const BaseGradPlan& p, float* g_mean, float* g_chol, hipStream_t s) {
    unsigned* tickets = reinterpret_cast<unsigned*>(buf);
    float *result = buf + p.off_result, *part = buf + p.off_part;
    const dim3 grid(p.nchunks, p.ntiles);
    if (kind == 1)
        hipLaunchKernelGGL(k_bg_contract<BG_VALU_DIAG>, grid, dim3(256), 0, s, n_in, A, sa, N, sn, w, B, p.chunk, tickets, result, part);
    else if (n_in < 16)
        hipLaunchKernelGGL(k_bg_contract<BG_VALU_DENSE>, grid, dim3(256), 0, s, n_in, A, sa, N, sn, w, B, p.chunk, tickets, result, part);
    else
        hipLaunchKernelGGL(k_bg_contract<BG_MFMA>, grid, dim3(256), 0, s, n_in, A, sa, N, sn, w, B, p.chunk, tickets, result, part);
    const size_t total = (size_t)n_in + (kind == 1 ? (size_t)n_in : (size_t)n_in * n_in);
    hipLaunchKernelGGL(k_bg_tail, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, n_in, kind, logpdf, bd, result, g_mean, g_chol);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_base_logpdf_pullback(int n_in, const BaseDist& bd, const float* src, int stride, const float* w, int B,
                                       float* buf, const BaseGradPlan& plan, float* g_mean, float* g_chol, hipStream_t s) {
    float* rows = buf + plan.off_rows;
    const size_t n = (size_t)n_in * B;
    hipLaunchKernelGGL(k_bg_whiten, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n_in, bd, src, stride, rows, n);
    return contract_and_tail(n_in, bd.kind, 1, bd, rows, n_in, rows, n_in, w, B, buf, plan, g_mean, g_chol, s);
}

hipError_t launch_base_sample_pullback(int n_in, int kind, const float* normals, const float* gz0, int B, float* buf,
                                       const BaseGradPlan& plan, float* g_mean, float* g_chol, hipStream_t s) {
    return contract_and_tail(n_in, kind, 0, BaseDist{}, gz0, n_in, normals, n_in, nullptr, B, buf, plan, g_mean, g_chol, s);
}
