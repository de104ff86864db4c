/* Differentiable flow paths: one model's inference (or sampling) with the state of the flow at caller-given times, and the
 * vector-Jacobian product of its outputs AND of those slices, in ONE launch -- the solve, the path stores and the discrete
 * adjoint of the accepted steps with the slices' cotangents injected at the save times.  Part of cnfhip.h, which includes it
 * where its types are declared (inside its extern "C" block): include cnfhip.h, not this file.  Like cnfhip_path.h it has a
 * binding table of its own (`_lib.PATH_VJP_EXPORTS`); tests/test_path_vjp_ref_host.py holds this header to the same rule: every
 * name declared here is exported by the library and bound.
 *
 * The launch is the one of cnf_inference_vjp_many / cnf_generate_vjp_many with one member (the PATH forms of that kernel), so the
 * envelope is theirs: two-layer networks, tanh then tanh (or identity, up to 16 hidden units), n_in <= 16, at most 64 hidden
 * units, no conditioning, the default base, no lock-step shards.  params_dev is the caller's [n_params] DEVICE vector (the
 * handle's own parameters and solver state are untouched); a recorded solve and cnf_grad_x end, as with every gradient call.
 *
 * The mathematics.  The step sequence (t_n, h_n) the solve accepted is frozen, hence theta_j = (tau_j - t_n) / h_n is a
 * constant.  A save time is served by step n exactly as cnfhip_path.h states; with pbar_j the cotangent of slice j (all D rows):
 *   tau_j == t_start (the slice is u0):            pbar_j joins d / d u(t_start) at the very end: it reaches grad_x / grad_z0 only;
 *   the end of its step (the slice is u_{n+1}):    lambda += pbar_j before step n is pulled back;
 *   interior (u_n + h_n sum_i b_i(theta_j) k_i):   with s_i = sum_j b_i(theta_j) pbar_j, the stage cotangents are
 *       kbar_i = h_n (b_i lambda + s_i + sum_{m > i} a_{m,i} w_m), i = 6..1, and lambda += sum_j pbar_j after the step;
 *       k_7 = f(u_{n+1}) is k_1 of step n + 1 (FSAL), so h_n s_7 joins that stage's kbar_1; only the last step's k_7 costs one
 *       more stage pullback, at the final state, and only if that step has interior save times.
 * Cotangents through the controller (of h_n, theta_j) are not taken. */
#ifndef CNFHIP_PATH_VJP_H
#define CNFHIP_PATH_VJP_H

/* The largest B one cnf_inference_path_vjp / cnf_generate_path_vjp launch takes for this handle and mode (all its 16-column tiles
 * must be on the device at once, and the PATH forms have their own register budget); 0: no such form for this handle or mode. */
int cnf_path_vjp_max_batch(cnf_handle h, int mode);

/* cnf_inference_path_vjp: cnf_inference_vjp_many for one member, plus the path.
 *   logpx_dev [B], regs_dev [3][B]   = the four outputs of the inference,
 *   path_out_dev [K][B][D] (or NULL) = the state at saveat_host[k], in the layout of cnf_solve_path,
 *   grad_dev [n_params]              = sum_b (sum_r cot[r][b] d out_r[b] + sum_k <path_cot[k][b], d path[k][b]>) / d params,
 *   grad_x_dev [B][n_in] (or NULL)   = the same w.r.t. z(t0).
 * cot_dev [4][B] as for cnf_inference_vjp_many, or NULL (zeros); path_cot_dev [K][B][D] in the layout of path_out_dev, or NULL
 * (zeros: the call is then cnf_inference_vjp_many's gradient plus the path).  saveat_host: HOST, as for cnf_solve_path, along
 * opts->t0 -> opts->t1.  Synchronous; two kernel launches.
 * Returns CNF_ERR_BAD_ARG for bad save times (cnf_solve_path's check, made before the handle is looked at) and NULL pointers;
 * CNF_ERR_UNSUPPORTED with nothing enqueued outside the envelope above, for B > cnf_path_vjp_max_batch and for
 * opts->kernel = CNF_KERNEL_GENERIC; CNF_ERR_MAXITERS / CNF_ERR_NONFINITE as the solve ends; CNF_ERR_UNSUPPORTED AFTER the launch
 * if the solve took more accepted steps than one launch can differentiate (1024, fewer for large batches) or a wait of the
 * launch ran out.  THERE IS NO STREAMED ROUTE BEHIND THIS CALL: such a solve has to be differentiated span by span with
 * cnf_inference_record / cnf_inference_pullback.  After every return other than CNF_OK that followed a launch the gradients are
 * zeros and the outputs NaN. */
cnf_status cnf_inference_path_vjp(cnf_handle h, int mode, const float* params_dev, const float* xs, const float* eps, int B,
                                  const cnf_solve_opts* opts, const float* saveat_host, int K,
                                  const float* cot_dev,        /* [4][B] or NULL */
                                  const float* path_cot_dev,   /* [K][B][D] or NULL */
                                  float* logpx_dev,            /* [B] */
                                  float* regs_dev,             /* [3][B] */
                                  float* path_out_dev,         /* [K][B][D] or NULL */
                                  float* grad_dev,             /* [n_params] */
                                  float* grad_x_dev,           /* [B][n_in] or NULL */
                                  cnf_solve_stats* stats, void* stream);

/* cnf_generate_path_vjp: cnf_generate_vjp_many for one member, plus the path.  The span is the reversed one (opts->t0 = start,
 * opts->t1 = end) and saveat_host runs along it.  x_out [B][nvars] and logq_out [B] as cnf_generate_vjp_many gives them (column
 * kernels behind the launch, as the z0 tail grad_z0 = lam_z(t_start) - cot_logq z0); cot_z_dev [B][n_in], cot_logq_dev [B] and
 * path_cot_dev [K][B][D] may each be NULL (zeros).  path_cot_dev is a cotangent of the STATE rows: its dlogp row is not logq's --
 * a caller whose loss is on logq(tau_k) = logpdf(z0) + dlogp(tau_k) adds -(sum_k g_k) z0 to grad_z0 itself.  Returns as above. */
cnf_status cnf_generate_path_vjp(cnf_handle h, int mode, const float* params_dev, const float* z0, const float* eps, int B,
                                 const cnf_solve_opts* opts, const float* saveat_host, int K,
                                 const float* cot_z_dev,       /* [B][n_in] or NULL */
                                 const float* cot_logq_dev,    /* [B] or NULL */
                                 const float* path_cot_dev,    /* [K][B][D] or NULL */
                                 float* x_out,                 /* [B][nvars] */
                                 float* logq_out,              /* [B] */
                                 float* path_out_dev,          /* [K][B][D] or NULL */
                                 float* grad_dev,              /* [n_params] */
                                 float* grad_z0_dev,           /* [B][n_in] or NULL */
                                 cnf_solve_stats* stats, void* stream);

/* The accepted steps of the last of the two calls above on this handle that returned CNF_OK: returns their number and copies
 * min(number, cap) pairs into t_host (t_n) and h_host (signed h_n) (HOST; may be NULL).  -1: there is none. */
int cnf_path_vjp_steps(cnf_handle h, float* t_host, float* h_host, int cap);

#endif /* CNFHIP_PATH_VJP_H */
