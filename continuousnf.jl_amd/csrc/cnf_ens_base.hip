// The members' own Gaussian bases of the ensemble calls (cnf_ens_base.h; include/cnfhip_ensemble_base.h).  The terminal cotangent
// P_m (z - mu_m) of the gradient launch is k_solve_wave's (cnf_wave.hip); everything else a base needs is here:
//   k_ens_base_prepare          (mean, sigma | L) -> mu, P = W' W, W = inv(L), L, c per member, in double, rounded once
//   k_ens_base_post             logpdf_m(z(t1)) - dlogp afresh from the final columns, and the member's five loss sums
//   k_ens_base_sample           z0 = mu_m + L_m n
//   k_ens_base_generate_post    x and logq = logpdf_m(z0) + dlogp of the sampling calls
//   k_ens_base_z0_grad          the + g_logq d logpdf_m(z0) / d z0 tail of grad_z0
//   k_ens_base_pullback         d / d (mean, chol) of sum_b w_b logpdf_m(s_b), and of the draw mu_m + L_m n_b
// The arithmetic per column is cnf_dist.hip's and cnf_basegrad.hip's (the same sums in the same order), with the member's base
// read from its prepared record.  Plain vector code: at n_in <= 16 and the ensemble's batch sizes a member's contraction is a
// few thousand fmas, below what filling an MFMA pipeline and transposing through LDS would cost.
//
// No kernel here waits on another workgroup, polls a word or takes a ticket; every loop bound is a kernel argument (n_in, B,
// M) or a constant, never a value read from memory -- a member's count only masks work inside loops bounded by B.
#include "cnf_ens_base.h"

namespace {

__device__ __forceinline__ float eb_wave_sum(float v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ int eb_flag(const float* __restrict__ bm) { return __float_as_int(bm[WV_ENS_BASE_FLAG]); }

// |W (z - mu)|^2 of column c, summed over the four lanes p = 0..3 of the sample (whitened_sq of cnf_dist.hip on a padded record)
__device__ __forceinline__ float eb_whitened_sq(const float* __restrict__ bm, const float* __restrict__ c, int n_in, int p) {
    float ss = 0.f;
    for (int i = p; i < n_in; i += 4) {
        const float* wr = bm + WV_ENS_BASE_W + 16 * i;
        float w = 0.f;
        for (int j = 0; j <= i; ++j) w = fmaf(wr[j], c[j] - bm[WV_ENS_BASE_MU + j], w);
        ss = fmaf(w, w, ss);
    }
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    return ss;
}

// One workgroup per member, thread (r, c) = entry (r, c) of the 16 x 16 matrices.
__global__ void __launch_bounds__(256)
k_ens_base_prepare(int n_in, int kind, const float* __restrict__ mean, const float* __restrict__ chol, float* __restrict__ bases) {
    __shared__ double sL[16][16], sW[16][16];
    __shared__ float sWf[16][16];
    __shared__ double sc;
    __shared__ int bad;
    const int tid = threadIdx.x, r = tid >> 4, c = tid & 15;
    const size_t m = blockIdx.x, n = (size_t)n_in;
    float* out = bases + m * WV_ENS_BASE_FLOATS;
    if (tid == 0) bad = 0;
    __syncthreads();
    const bool in = r < n_in && c < n_in;
    float l = 0.f, mu = 0.f;
    if (in) {
        if (kind == 1) l = r == c ? chol[m * n + r] : 0.f;
        else l = c <= r ? chol[(m * n + r) * n + c] : 0.f;
        if (!isfinite(l) || (r == c && !(l > 0.f))) bad = 1;
    }
    if (tid < n_in) {
        mu = mean[m * n + tid];
        if (!isfinite(mu)) bad = 1;
    }
    sL[r][c] = (double)l;
    sW[r][c] = 0.0;
    __syncthreads();
    const bool bad_in = bad != 0;                          // (uniform: read behind the barrier)
    // W = inv(L), column tid by forward substitution: W_jj = 1 / L_jj, W_ij = -(sum_{j <= k < i} L_ik W_kj) / L_ii
    if (!bad_in && tid < n_in) {
        const int j = tid;
        sW[j][j] = 1.0 / sL[j][j];
        for (int i = j + 1; i < n_in; ++i) {
            double acc = 0.0;
            for (int k = j; k < i; ++k) acc += sL[i][k] * sW[k][j];
            sW[i][j] = -acc / sL[i][i];
        }
    }
    __syncthreads();
    const float wf = (float)sW[r][c];
    sWf[r][c] = wf;
    if (!bad_in && tid == 0) {
        double acc = 0.0;
        for (int i = 0; i < n_in; ++i) acc += log(sW[i][i]);
        sc = acc - 0.5 * (double)n_in * 1.8378770664093454836;
    }
    __syncthreads();
    float pf = 0.f;
    if (!bad_in && in) {                                   // (W' W)_rc from the rounded W, k >= max(r, c) upwards (cnf_set_basedist)
        double acc = 0.0;
        for (int k = r > c ? r : c; k < n_in; ++k) acc += (double)sWf[k][r] * (double)sWf[k][c];
        pf = (float)acc;
        if (!isfinite(wf) || !isfinite(pf) || (r == c && !(wf > 0.f))) bad = 1;
    }
    if (!bad_in && tid == 0 && !isfinite((float)sc)) bad = 1;
    __syncthreads();
    const bool ok = bad == 0;
    const float eye = (in && r == c) ? 1.f : 0.f;          // a flagged member: N(0, I), so that a launch that reads it stays finite
    out[WV_ENS_BASE_P + tid] = ok ? pf : eye;
    out[WV_ENS_BASE_W + tid] = ok ? wf : eye;
    out[WV_ENS_BASE_L + tid] = ok ? l : eye;
    if (tid < 16) out[WV_ENS_BASE_MU + tid] = (ok && tid < n_in) ? mu : 0.f;
    if (tid >= 16 && tid < 32) {                           // c | flag | padding
        const int e = WV_ENS_BASE_C + tid - 16;
        float v = 0.f;
        if (e == WV_ENS_BASE_C) v = ok ? (float)sc : (float)(-0.5 * (double)n_in * 1.8378770664093454836);
        if (e == WV_ENS_BASE_FLAG) v = __int_as_float(ok ? 0 : 1);
        out[e] = v;
    }
}

__global__ void __launch_bounds__(256) k_ens_base_flags(const float* __restrict__ bases, int* __restrict__ flags, int M) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m < M) flags[m] = eb_flag(bases + (size_t)m * WV_ENS_BASE_FLOATS);
}

// One workgroup per member; four lanes share a sample, 64 samples per pass, the passes upwards.  A thread adds its passes'
// values in pass order, then the fixed tree of k_base_post: the sums of member m depend on its own columns below its count
// only -- the same bits as the M = 1 call at B = counts[m].
__global__ void __launch_bounds__(256)
k_ens_base_post(int n_in, int D, const float* __restrict__ bases, const StepState* __restrict__ fin, const float* __restrict__ cols,
                float* __restrict__ logpx, const float* __restrict__ regs, int B, const int* __restrict__ counts, float* __restrict__ sums5) {
    const size_t m = blockIdx.x, Bz = (size_t)B;
    const float* bm = bases + m * WV_ENS_BASE_FLOATS;
    const StepState* f = fin + m;
    if (eb_flag(bm) || !f->done || f->nonfinite || f->n_partials < 0) return;      // (workgroup-uniform)
    const int cnt = counts ? counts[m] : B;
    const int tid = threadIdx.x, p = tid & 3, s = tid >> 2;
    const bool with_regs = D - n_in == 3;
    const float lc = bm[WV_ENS_BASE_C];
    float v4[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + s;
        const bool live = b < cnt;
        const float* c = cols + (m * Bz + (size_t)(live ? b : 0)) * D;
        const float ss = eb_whitened_sq(bm, c, n_in, p);
        if (live && p == 0) {
            const float lp = fmaf(-0.5f, ss, lc) - c[n_in];
            logpx[m * Bz + b] = lp;
            v4[0] += lp;
            if (with_regs) {
                v4[1] += regs[(m * 3 + 0) * Bz + b];
                v4[2] += regs[(m * 3 + 1) * Bz + b];
                v4[3] += regs[(m * 3 + 2) * Bz + b];
            }
        }
    }
    __shared__ float sm[4][4];
    const int w = tid >> 6, l = tid & 63;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float r = eb_wave_sum(v4[j]);
        if (l == 0) sm[j][w] = r;
    }
    __syncthreads();
    if (tid < 4) sums5[5 * m + tid] = (sm[tid][0] + sm[tid][1]) + (sm[tid][2] + sm[tid][3]);
    if (tid == 4) sums5[5 * m + 4] = (float)cnt;
}

// one lane per entry of z0 [M][B][n_in]
__global__ void __launch_bounds__(256)
k_ens_base_sample(int n_in, int kind, const float* __restrict__ bases, const float* __restrict__ nrm, float* __restrict__ z0, size_t per,
                  size_t n) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float* bm = bases + (e / per) * WV_ENS_BASE_FLOATS;
    const int i = (int)(e % (size_t)n_in);
    const float* lr = bm + WV_ENS_BASE_L + 16 * i;
    if (kind == 1) {
        z0[e] = fmaf(lr[i], nrm[e], bm[WV_ENS_BASE_MU + i]);
        return;
    }
    const float* row = nrm + (e - (size_t)i);
    float v = 0.f;
    for (int j = 0; j <= i; ++j) v = fmaf(lr[j], row[j], v);
    z0[e] = v + bm[WV_ENS_BASE_MU + i];
}

// the M B columns as one batch, four lanes per sample (k_generate_post_rows with the member's base)
__global__ void __launch_bounds__(256)
k_ens_base_generate_post(int n_in, int n_out, int D, const float* __restrict__ bases, const float* __restrict__ fsol,
                         const float* __restrict__ z0, float* __restrict__ x_out, float* __restrict__ logq, size_t cols_n,
                         const int* __restrict__ counts, int Bm) {
    const int tid = threadIdx.x, p = tid & 3;
    const size_t b = (size_t)blockIdx.x * 64 + (tid >> 2);
    size_t bb = b < cols_n ? b : cols_n - 1;
    const size_t m = bb / (size_t)Bm;
    const bool pad = counts && bb - m * (size_t)Bm >= (size_t)counts[m];
    if (pad) bb = m * (size_t)Bm;                          // (its lanes read the member's first column for the shuffles and leave)
    const float* bm = bases + m * WV_ENS_BASE_FLOATS;
    const float* c = fsol + bb * D;
    const float ss = eb_whitened_sq(bm, z0 + bb * n_in, n_in, p);
    if (b >= cols_n || pad) return;
    for (int i = p; i < n_out; i += 4) x_out[bb * n_out + i] = c[i];
    if (p == 0 && logq) logq[b] = fmaf(-0.5f, ss, bm[WV_ENS_BASE_C]) + c[n_in];
}

// one lane per entry of gz0 [M][B][n_in]
__global__ void __launch_bounds__(256)
k_ens_base_z0_grad(int n_in, const float* __restrict__ bases, const float* __restrict__ lam0, const float* __restrict__ cot_logq,
                   const float* __restrict__ z0, float* __restrict__ gz0, size_t cols_n, const int* __restrict__ counts, int Bm) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n_in * cols_n) return;
    const size_t b = e / (size_t)n_in, m = b / (size_t)Bm;
    if (counts && b - m * (size_t)Bm >= (size_t)counts[m]) return;
    const int i = (int)(e - b * (size_t)n_in);
    float g = lam0[e];
    if (cot_logq) {
        const float* bm = bases + m * WV_ENS_BASE_FLOATS;
        const float* c = z0 + b * n_in;
        const float* pr = bm + WV_ENS_BASE_P + 16 * i;
        float v = 0.f;                                   // -d logpdf / d z_i
        for (int j = 0; j < n_in; ++j) v = fmaf(pr[j], c[j] - bm[WV_ENS_BASE_MU + j], v);
        g = fmaf(-cot_logq[b], v, g);
    }
    gz0[e] = g;
}

// The batch contraction  mv = sum_b w_b a_b,  Mm = sum_b w_b a_b n_b'  of one member and the tail that needs the base only, one
// workgroup per member.  16 samples per pass: thread (s, i) forms a_b[i] and n_b[i] of sample b = b0 + s in LDS, then thread
// (r, c), c <= r, adds the pass's 16 samples to Mm[r][c] in sample order (c == 0: and to mv[r]).
// LOGPDF: a_b = n_b = W (s_b - mu), w = the caller's weights; else a_b = gz0_b, n_b = normals_b, w = 1.
template <bool LOGPDF>
__global__ void __launch_bounds__(256)
k_ens_base_pullback(int n_in, int kind, const float* __restrict__ bases, const float* __restrict__ A, int stride,
                    const float* __restrict__ N, const float* __restrict__ w, int B, const int* __restrict__ counts,
                    float* __restrict__ g_mean, float* __restrict__ g_chol) {
    __shared__ float sa[16][17], sn[16][17], sw[16], sM[16][17], sv[16], ssw;
    const int tid = threadIdx.x, r = tid >> 4, c = tid & 15;
    const size_t m = blockIdx.x, Bz = (size_t)B, n = (size_t)n_in;
    const float* bm = bases ? bases + m * WV_ENS_BASE_FLOATS : nullptr;
    const int cnt = counts ? counts[m] : B;
    const bool own = r < n_in && c <= r;
    float acc = 0.f, am = 0.f, wsum = 0.f;
    for (int b0 = 0; b0 < B; b0 += 16) {
        const int b = b0 + r;                              // (load phase: r is the sample of the pass, c the row)
        float av = 0.f, nv = 0.f;
        if (b < cnt && c < n_in) {
            if (LOGPDF) {
                const float* col = A + (m * Bz + b) * (size_t)stride;
                const float* wr = bm + WV_ENS_BASE_W + 16 * c;
                float t = 0.f;
                for (int j = 0; j <= c; ++j) t = fmaf(wr[j], col[j] - bm[WV_ENS_BASE_MU + j], t);
                av = nv = t;
            } else {
                av = A[(m * Bz + b) * n + c];
                nv = N[(m * Bz + b) * n + c];
            }
        }
        sa[r][c] = av;
        sn[r][c] = nv;
        if (c == 0) sw[r] = b < cnt ? (LOGPDF ? w[m * Bz + b] : 1.f) : 0.f;
        __syncthreads();
        if (own) {
            for (int s = 0; s < 16; ++s)
                if (b0 + s < cnt) {
                    const float a = LOGPDF ? sw[s] * sa[s][r] : sa[s][r];
                    acc = fmaf(a, sn[s][c], acc);
                    if (c == 0) am += a;
                }
        }
        if (tid == 1) {
            for (int s = 0; s < 16; ++s)
                if (b0 + s < cnt) wsum += sw[s];
        }
        __syncthreads();
    }
    sM[r][c] = own ? acc : 0.f;
    if (c == 0) sv[r] = r < n_in ? am : 0.f;
    if (tid == 1) ssw = wsum;
    __syncthreads();
    if (tid < n_in) {                                      // g_mean; the sums run over k upwards (k_bg_tail)
        const int i = tid;
        float v;
        if (!LOGPDF) v = sv[i];
        else if (kind == 1) v = bm[WV_ENS_BASE_W + 17 * i] * sv[i];
        else {
            v = 0.f;
            for (int k = i; k < n_in; ++k) v = fmaf(bm[WV_ENS_BASE_W + 16 * k + i], sv[k], v);
        }
        g_mean[m * n + i] = v;
    }
    if (kind == 1) {
        if (tid < n_in) {
            const int i = tid;
            const float d = sM[i][i];
            g_chol[m * n + i] = LOGPDF ? (d - ssw) * bm[WV_ENS_BASE_W + 17 * i] : d;
        }
        return;
    }
    if (r < n_in && c < n_in) {
        const int i = r, j = c;
        float v = 0.f;
        if (j <= i) {
            if (!LOGPDF) v = sM[i][j];
            else {
                for (int k = i; k < n_in; ++k) v = fmaf(bm[WV_ENS_BASE_W + 16 * k + i], sM[k][j], v);
                if (i == j) v -= ssw / bm[WV_ENS_BASE_L + 17 * i];
            }
        }
        g_chol[(m * n + i) * n + j] = v;
    }
}

}  // namespace

void launch_ens_base_prepare(int n_in, int kind, const float* mean, const float* chol, float* bases, int M, hipStream_t s) {
    hipLaunchKernelGGL(k_ens_base_prepare, dim3(M), dim3(256), 0, s, n_in, kind, mean, chol, bases);
}

void launch_ens_base_flags(const float* bases, int* flags, int M, hipStream_t s) {
    hipLaunchKernelGGL(k_ens_base_flags, dim3((M + 255) / 256), dim3(256), 0, s, bases, flags, M);
}

void launch_ens_base_post(int n_in, int D, const float* bases, const StepState* fin, const float* cols, float* logpx, const float* regs,
                          int B, const int* counts, float* sums5, int M, hipStream_t s) {
    hipLaunchKernelGGL(k_ens_base_post, dim3(M), dim3(256), 0, s, n_in, D, bases, fin, cols, logpx, regs, B, counts, sums5);
}

void launch_ens_base_sample(int n_in, int kind, const float* bases, const float* normals, float* z0, int B, int M, hipStream_t s) {
    const size_t per = (size_t)n_in * B, n = per * M;
    hipLaunchKernelGGL(k_ens_base_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n_in, kind, bases, normals, z0, per, n);
}

void launch_ens_base_generate_post(int n_in, int n_out, int D, const float* bases, const float* fsol, const float* z0, float* x_out,
                                   float* logq, int B, const int* counts, int M, hipStream_t s) {
    const size_t cols_n = (size_t)M * B;
    hipLaunchKernelGGL(k_ens_base_generate_post, dim3((unsigned)((cols_n + 63) / 64)), dim3(256), 0, s, n_in, n_out, D, bases, fsol, z0,
                       x_out, logq, cols_n, counts, B);
}

void launch_ens_base_z0_grad(int n_in, const float* bases, const float* lam0, const float* cot_logq, const float* z0, float* gz0, int B,
                             const int* counts, int M, hipStream_t s) {
    const size_t cols_n = (size_t)M * B, n = cols_n * n_in;
    hipLaunchKernelGGL(k_ens_base_z0_grad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n_in, bases, lam0, cot_logq, z0, gz0, cols_n,
                       counts, B);
}

void launch_ens_base_logpdf_pullback(int n_in, int kind, const float* bases, const float* src, int stride, const float* w, int B,
                                     const int* counts, float* g_mean, float* g_chol, int M, hipStream_t s) {
    hipLaunchKernelGGL(k_ens_base_pullback<true>, dim3(M), dim3(256), 0, s, n_in, kind, bases, src, stride, (const float*)nullptr, w, B,
                       counts, g_mean, g_chol);
}

void launch_ens_base_sample_pullback(int n_in, int kind, const float* normals, const float* gz0, int B, const int* counts, float* g_mean,
                                     float* g_chol, int M, hipStream_t s) {
    hipLaunchKernelGGL(k_ens_base_pullback<false>, dim3(M), dim3(256), 0, s, n_in, kind, (const float*)nullptr, gz0, n_in, normals,
                       (const float*)nullptr, B, counts, g_mean, g_chol);
}
