/* Differentiable ensemble sampling: M members' samples, their log-densities and the vector-Jacobian product of both for a
 * per-sample cotangent, in the launch that cnf_loss_grad_many makes for the built-in loss -- what cnf_generate_record +
 * cnf_generate_pullback give for one model.  Part of cnfhip.h, which includes it where its types are declared (inside its
 * extern "C" block): include cnfhip.h, not this file.  Like cnfhip_ensemble_vjp.h it has a binding table of its own
 * (`_lib.ENSEMBLE_GENERATE_VJP_EXPORTS`); tests/test_ensemble_gen_vjp_host.py holds this header to the same rule: every name
 * declared here is exported by the library and bound. */
#ifndef CNFHIP_ENSEMBLE_GENERATE_VJP_H
#define CNFHIP_ENSEMBLE_GENERATE_VJP_H

/* The largest M one cnf_generate_vjp_many launch takes for this handle, mode and batch: cnf_ensemble_capacity's rule applied to
 * the sampling form of the gradient kernel (which has its own register budget); 0 for whatever cnf_ensemble_capacity answers 0
 * for. */
int cnf_ensemble_generate_vjp_capacity(cnf_handle h, int mode, int B);

/* cnf_generate_vjp_many: every member m, with its own parameters, base draw, probes and start time as in cnf_generate_many,
 * integrates u0 = [z0[m]; 0] over the reversed span -- from its start time (t0_host[m], or opts->t0) to opts->t1 -- as
 * `generate` does (src/base_icnf.jl:358-380) and keeps the first nvars rows of the final state (:202-211):
 *   x_out[m]     = those rows, [B][nvars],
 *   logq_out[m]  = logpdf(N(0, I), z0[m]) + dlogp_end, the log-density of the whole n_in-row final state (sign +: `inference`
 *                  has logpz - dlogp),
 *   grad_dev[m]  = sum_b (<cot_z[m][b], d z_b / d params[m]> + cot_logq[m][b] d logq_b / d params[m]),
 *   grad_z0_dev[m] (may be NULL) = the same w.r.t. the base draw z0[m], [B][n_in],
 * through the steps the member's own adaptive solve accepted: the exact discrete adjoint of that solve (cnf_ensemble_steps
 * returns them).  The terminal cotangent of the backward sweep is the one of cnf_generate_pullback:
 *   lam_z(t_end) = cot_z,   lam_dlogp = +cot_logq,   lam_E = lam_n = 0
 * (the E and n rows are integrated in TrainMode but are not outputs of sampling), and once the sweep has reached
 * u(t_start) = [z0; 0],
 *   grad_z0 = lam_z(t_start) - cot_logq z0        (= lam_z(t_start) + cot_logq d logpdf(N(0, I), z0) / d z0).
 * cot_z_dev is [M][B][n_in]: a cotangent of ALL n_in rows of the final state (zeros on the rows behind nvars for a cotangent of
 * x alone); cot_logq_dev is [M][B]; either may be NULL (zeros), not both.  params_dev [M][n_params], z0 [M][B][n_in], eps
 * [M][B][n_in] (NULL in TestMode) and every output are DEVICE memory; t0_host (NULL: opts->t0 for all), status_out and stats_out
 * (may be NULL) are HOST arrays of M.  Synchronous; two kernel launches -- the solve with its adjoint, the partial sums -- plus
 * the column kernels (x and logq; the z0 tail), whatever M.
 * Per member status_out[m] as cnf_loss_grad_many: CNF_OK; CNF_ERR_NONFINITE; CNF_ERR_MAXITERS; CNF_ERR_UNSUPPORTED = this
 * member's part of the launch gave up.  For a member that is not CNF_OK the gradient and grad_z0 are zeros, x and logq NaN.
 * Returns CNF_OK whenever the launch ran; CNF_ERR_UNSUPPORTED with nothing enqueued if M exceeds
 * cnf_ensemble_generate_vjp_capacity (or that is 0, or opts->kernel is CNF_KERNEL_GENERIC); CNF_ERR_BAD_ARG / CNF_ERR_BAD_SHAPE
 * (NULL pointers, M < 1, B < 1, bad options, a member's empty span) before anything touches the device.  The handle's own
 * parameters and solver state are untouched; a recorded solve and cnf_grad_x end, as with every gradient call. */
cnf_status cnf_generate_vjp_many(cnf_handle h, int mode, int M, const float* params_dev,
                                 const float* z0,            /* [M][B][n_in] */
                                 const float* eps,           /* [M][B][n_in], NULL in TestMode */
                                 int B, const cnf_solve_opts* opts,   /* reverse(tspan): t0 = start, t1 = end */
                                 const float* t0_host,       /* NULL or the members' own start times [M] */
                                 const float* cot_z_dev,     /* [M][B][n_in] or NULL */
                                 const float* cot_logq_dev,  /* [M][B] or NULL (not both) */
                                 float* x_out,               /* [M][B][nvars] */
                                 float* logq_out,            /* [M][B] */
                                 float* grad_dev,            /* [M][n_params] */
                                 float* grad_z0_dev,         /* [M][B][n_in] or NULL */
                                 int* status_out, cnf_solve_stats* stats_out, void* stream);

#endif /* CNFHIP_ENSEMBLE_GENERATE_VJP_H */
