// The members' own Gaussian bases of the ensemble calls (cnf_ensemble_set_bases, include/cnfhip_ensemble_base.h) and the launches
// that evaluate them (cnf_ens_base.hip).  Reference: icnf.basedist, src/base_icnf.jl:16-21, consumed by logpdf(icnf.basedist, z)
// (:155, :177) and rand!(rng, icnf.basedist, new_xs) (:320-393) -- here one base per member of an ensemble call.
//
// A member's prepared base is WV_ENS_BASE_FLOATS floats (cnf_wave.h): mu | P | W | L | c | flag, the matrices 16 x 16 row-major
// and zero beyond n_in, so that k_solve_wave reads mu and P as a padded tile.  `bases` below is [M] of them, DEVICE memory.
// `counts` (device, [M], or null) are the members' own batch sizes: a column at or behind its member's count is neither read
// nor written.  n_in <= 16 everywhere (the ensemble envelope).
#pragma once
#include "cnf_wave.h"

// kind 1: chol = sigma [M][n_in]; kind 2: chol = L [M][n_in][n_in], row-major, lower triangular.  In double, rounded once:
// W = inv(L) by forward substitution, P = W' W from the rounded W, c = sum log W_ii - n_in / 2 log(2 pi).  A member with a
// non-finite entry or a non-positive diagonal gets flag 1 and the base N(0, I), so that nothing of it poisons a launch.
void launch_ens_base_prepare(int n_in, int kind, const float* mean, const float* chol, float* bases, int M, hipStream_t s);
// the members' flags, [M] ints, gathered for the one copy to the host
void launch_ens_base_flags(const float* bases, int* flags, int M, hipStream_t s);
// logpx[m][b] = c_m - 1/2 |W_m (z_b - mu_m)|^2 - dlogp_b afresh from the final columns cols [M][B][D], and the member's five
// loss sums (sum logpx, sum E, sum n, sum A, count) re-formed in a fixed order from logpx and regs [M][3][B].  Members whose
// final state `fin` is not a finished, finite solve, and flagged members, are skipped.
void launch_ens_base_post(int n_in, int D, const float* bases, const StepState* fin, const float* cols, float* logpx, const float* regs,
                          int B, const int* counts, float* sums5, int M, hipStream_t s);
// z0[m][b] = mu_m + L_m n_b (k_base_sample's arithmetic: the sum over j upwards, mu added last; diagonal kind: one fma)
void launch_ens_base_sample(int n_in, int kind, const float* bases, const float* normals, float* z0, int B, int M, hipStream_t s);
// sampling: x_out[m][b] = the first n_out rows of the final column, logq[m][b] = logpdf_m(z0_b) + dlogp_b (logq may be null)
void launch_ens_base_generate_post(int n_in, int n_out, int D, const float* bases, const float* fsol, const float* z0, float* x_out,
                                   float* logq, int B, const int* counts, int M, hipStream_t s);
// gz0 = lam0 - cot_logq P_m (z0 - mu_m)   (cot_logq null: a copy; gz0 must not alias lam0)
void launch_ens_base_z0_grad(int n_in, const float* bases, const float* lam0, const float* cot_logq, const float* z0, float* gz0, int B,
                             const int* counts, int M, hipStream_t s);
// The two pullbacks, one workgroup per member, a fixed summation order (the samples upwards), no float atomics.
//   logpdf: src [M][B][stride] (the first n_in floats of a column are s_b), w [M][B]:
//     g_mean[m] = W' sum_b w_b n_b,  g_chol[m] = tril(W' sum_b w_b n_b n_b') - (sum_b w_b) diag(1 / L_ii),  n_b = W (s_b - mu)
//     (diagonal kind: (sum_b w_b n_b[i]^2 - sum_b w_b) / sigma_i)
//   sample: normals, gz0 [M][B][n_in]:  g_mean[m] = sum_b g_b,  g_chol[m] = tril(sum_b g_b n_b')  (diagonal kind: its diagonal)
// g_mean [M][n_in]; g_chol [M][n_in] (kind 1) or [M][n_in][n_in] (kind 2, zeros above the diagonal).
void launch_ens_base_logpdf_pullback(int n_in, int kind, const float* bases, const float* src, int stride, const float* w, int B,
                                     const int* counts, float* g_mean, float* g_chol, int M, hipStream_t s);
void launch_ens_base_sample_pullback(int n_in, int kind, const float* normals, const float* gz0, int B, const int* counts, float* g_mean,
                                     float* g_chol, int M, hipStream_t s);
