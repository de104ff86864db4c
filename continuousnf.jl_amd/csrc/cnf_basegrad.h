// The gradient w.r.t. the base distribution's own parameters (cnf_base_logpdf_pullback / cnf_base_sample_pullback,
// cnf_basegrad.hip): one batch contraction
//     m = sum_b w_b a_b,    M = sum_b w_b a_b n_b'     (dense kind: the lower triangle of M; diagonal kind: its diagonal)
// over rows a_b, n_b of n_in floats, and a tail that turns (m, M, sum_b w_b) into (g_mean, g_chol).
#pragma once
#include "cnf_dist.h"
#include "cnf_basegrad_plan.h"      // BaseGradPlan, base_grad_plan: the layout of the handle's buffer

// The log-density direction: n_b = W (s_b - mean) from rows s_b (src: `stride` floats per sample), a_b = n_b, weights w[B];
// then g_mean = W' m and g_chol = tril(W' M) - (sum w) diag(1 / L_ii)   (diagonal kind: (M_ii - sum w) / sigma_i).
// buf: plan.floats floats whose ticket words are zero (they are left zero).  g_chol as cnf_set_basedist takes chol.
hipError_t launch_base_logpdf_pullback(int n_in, const BaseDist& bd, const float* src, int stride, const float* w, int B,
                                       float* buf, const BaseGradPlan& plan, float* g_mean, float* g_chol, hipStream_t s);
// The pullback of z0 = mean + L n: a_b = gz0[b], n_b = normals[b] ([B][n_in] both), unit weights;
// g_mean = m, g_chol = tril(M) (diagonal kind: its diagonal).
hipError_t launch_base_sample_pullback(int n_in, int kind, const float* normals, const float* gz0, int B, float* buf,
                                       const BaseGradPlan& plan, float* g_mean, float* g_chol, hipStream_t s);
