/* Differentiable ensembles: the vector-Jacobian product of M members' inference for a per-sample cotangent of its four outputs,
 * in the launch that cnf_loss_grad_many makes for the built-in loss.  Part of cnfhip.h, which includes it where its types are
 * declared (inside its extern "C" block): include cnfhip.h, not this file.  Like cnfhip_ensemble.h it has a binding table of its
 * own (`_lib.ENSEMBLE_VJP_EXPORTS`); tests/test_ensemble_vjp_host.py holds this header to the same rule: every name declared here
 * is exported by the library and bound. */
#ifndef CNFHIP_ENSEMBLE_VJP_H
#define CNFHIP_ENSEMBLE_VJP_H

/* The largest M one cnf_inference_vjp_many launch takes for this handle, mode and batch: cnf_ensemble_capacity's rule applied to
 * the per-sample-cotangent form of the kernel (which has its own register budget); 0 for whatever cnf_ensemble_capacity
 * answers 0 for. */
int cnf_ensemble_vjp_capacity(cnf_handle h, int mode, int B);

/* cnf_inference_vjp_many: for every member m, with its own parameters, data, probes and end time as in cnf_loss_grad_many,
 *   logpx_dev[m], regs_dev[m]  = the four outputs of its inference (rows E, n, A of regs),
 *   grad_dev[m]                = sum_b sum_r cot[m][r][b] d out_r[b] / d params[m],
 *   grad_x_dev[m] (may be NULL) = the same w.r.t. z(t0), [B][n_in] (its first nvars entries per sample are d / d xs),
 * through the steps the member's own adaptive solve accepted: the exact discrete adjoint of that solve (cnf_ensemble_steps
 * returns them).  cot_dev is [M][4][B], rows (g_logpx, g_E, g_n, g_A) -- the convention of cnf_inference_pullback: the
 * cotangents themselves, not multiplied by the regularisers' weights; a row the handle does not integrate (lambda1, lambda2 or
 * lambda3 = 0; all three in TestMode) is ignored.  params_dev [M][n_params], xs [M][B][nvars], eps [M][B][n_in] (NULL in
 * TestMode) and every output are DEVICE memory; t1_host (NULL: opts->t1 for all), status_out and stats_out (may be NULL) are
 * HOST arrays of M.  Synchronous; two kernel launches whatever M.
 * Per member status_out[m] as cnf_loss_grad_many: CNF_OK; CNF_ERR_NONFINITE; CNF_ERR_MAXITERS; CNF_ERR_UNSUPPORTED = this
 * member's part of the launch gave up.  For a member that is not CNF_OK the gradient and grad_x are zeros, logpx and regs NaN.
 * Returns CNF_OK whenever the launch ran; CNF_ERR_UNSUPPORTED with nothing enqueued if M exceeds cnf_ensemble_vjp_capacity (or
 * that is 0, or opts->kernel is CNF_KERNEL_GENERIC); CNF_ERR_BAD_ARG / CNF_ERR_BAD_SHAPE (NULL pointers, M < 1, B < 1, bad
 * options) before anything touches the device.  The handle's own parameters and solver state are untouched; a recorded solve and
 * cnf_grad_x end, as with every gradient call. */
cnf_status cnf_inference_vjp_many(cnf_handle h, int mode, int M, const float* params_dev, const float* xs, const float* eps,
                                  int B, const cnf_solve_opts* opts, const float* t1_host,
                                  const float* cot_dev,      /* [M][4][B] */
                                  float* logpx_dev,          /* [M][B]    */
                                  float* regs_dev,           /* [M][3][B] */
                                  float* grad_dev,           /* [M][n_params] */
                                  float* grad_x_dev,         /* [M][B][n_in] or NULL: d/d z(t0) */
                                  int* status_out, cnf_solve_stats* stats_out, void* stream);

#endif /* CNFHIP_ENSEMBLE_VJP_H */
