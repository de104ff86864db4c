// The base distribution of a handle (cnf_set_basedist) and the launches that evaluate it (cnf_dist.hip): log-density
// post-pass, terminal cotangent of the gradient, base sample.  Reference: icnf.basedist, src/base_icnf.jl:16-21, consumed by
// logpdf(icnf.basedist, z) (:155, :177) and rand!(rng, icnf.basedist, new_xs) (:320-393).
#pragma once
#include "cnf_dev.h"

// N(mean, Sigma), Sigma = L L', W = inv(L).  All pointers DEVICE memory.
//   kind 1 (diagonal): whiten = 1 / sigma, chol = sigma, prec = 1 / sigma^2; n_in floats each
//   kind 2 (dense):    whiten = W, chol = L (lower triangular), prec = W' W; n_in x n_in, ROW-major (entry (i, j) at i n_in + j)
struct BaseDist {
    int kind;                // 0: the default N(0, I) -- nothing of cnf_dist.hip is launched
    const float* mean;
    const float* whiten;
    const float* chol;
    const float* prec;
    float logconst;          // c = sum_i log W_ii - n_in / 2 log(2 pi)
};

// logpx[b] = c - 1/2 |W (z_b - mean)|^2 - dlogp_b, afresh from the final state (st != null: U[st->cur], else U0); D floats per
// sample.  regs (3 x B, written before by the N(0, I) post-processing) are read only; sums5 != null: also the five loss sums
// (sum logpx, sum E, sum n, sum A, B), through `part` (4 floats per 64 samples) and `ticket` (zero between launches).
void launch_base_post(int n_in, int D, const BaseDist& bd, const StepState* st, const float* U0, const float* U1, float* logpx,
                      const float* regs, int B, float* sums5, float* part, unsigned* ticket, hipStream_t s);
// lam[b] = (W' W (z_b - mean) + lambda3 unit(z_aug) on the augmented rows) / B   ([B][n_in]; fsol: D floats per sample)
void launch_base_cotangent(const NetDesc& nd, int D, const BaseDist& bd, float lambda3, const float* fsol, float* lam, int B,
                           hipStream_t s);
// z0[b] = mean + L n_b   ([B][n_in] both; must not alias)
void launch_base_sample(int n_in, const BaseDist& bd, const float* normals, float* z0, int B, hipStream_t s);
// The terminal cotangent of cnf_inference_pullback for cot = [4][B] (rows logpx, E, n, A) and, in the same launch, the pack of
// the per-sample weights of the three scalar rows for the pullback kernels (logpx = logpz - dlogp: the dlogp row carries -cot_l):
//   lam[b] = cot_l[b] d logpdf(basedist, z_b) / d z + cot_A[b] unit(z_aug, b)     (N(0, I), kind 0: -cot_l[b] z_b)
//   cw = [3][B]: w_l = -cot_l, w_E = cot_E, w_n = cot_n
// with_A = 0 (TestMode, or a handle that does not integrate the A row): cot_A is not read.
void launch_vjp_cotangent(const NetDesc& nd, int D, const BaseDist& bd, int with_A, const float* fsol, const float* cot, float* lam,
                          float* cw, int B, hipStream_t s);

// ---- differentiable sampling (cnf_generate_record / cnf_generate_pullback); all arrays [B][rows], kind 0 included ----
// z_out[b] = rows 1..n_in of fsol[b] (D floats per sample), logq[b] = logpdf(base, z0_b) + dlogp_b
void launch_generate_post(int n_in, int D, const BaseDist& bd, const float* fsol, const float* z0, float* z_out, float* logq, int B,
                          hipStream_t s);
// cnf_generate_many: the M B columns of an ensemble as one batch, N(0, I) base: x_out[b] = the first n_out rows, logq may be null
// (counts, device [M] with Bm columns per member: heterogeneous members -- columns at or behind their member's count are skipped)
void launch_generate_post_rows(int n_in, int n_out, int D, const float* fsol, const float* z0, float* x_out, float* logq, size_t B,
                               hipStream_t s, const int* counts = nullptr, int Bm = 0);
// ... and u0 = [z0; 0] of those members' own columns ([cols][D] from [cols][n_in])
void launch_ens_u0_counts(int n_in, int D, const float* z0, float* u0, size_t cols, const int* counts, int Bm, hipStream_t s);
// The terminal cotangent: lam = cot_z, cw = [3][B]: w_l = +cot_logq, w_E = w_n = 0 (null cotangents: zeros).  n_in >= 1.
void launch_generate_cotangent(int n_in, const float* cot_z, const float* cot_logq, float* lam, float* cw, int B, hipStream_t s);
// gz0 = lam0 + cot_logq d logpdf(base, z0) / d z0   (cot_logq null: a copy; gz0 must not alias lam0).  B: the columns -- of an
// ensemble (cnf_generate_vjp_many) all M B of them as one batch
void launch_generate_z0_grad(int n_in, const BaseDist& bd, const float* lam0, const float* cot_logq, const float* z0, float* gz0,
                             size_t B, hipStream_t s, const int* counts = nullptr, int Bm = 0);
