/* Ensemble flow paths: the C ABI of libcnfhip.so for the paths of M independent models of one architecture, and the
 * vector-Jacobian product of those paths, in ONE launch -- cnfhip_path.h / cnfhip_path_vjp.h for the members of
 * cnfhip_ensemble_eval.h / cnfhip_ensemble_vjp.h / cnfhip_ensemble_generate_vjp.h.  Part of cnfhip.h, which includes it where its
 * types are declared (inside its extern "C" block): include cnfhip.h, not this file.  The entry points have a header and a
 * binding table (`_lib.ENSEMBLE_PATH_EXPORTS`) of their own, because the tests pin the lists the other headers declare;
 * tests/test_ensemble_path_host.py holds this header to the same rule: every name declared here is exported by the library and
 * bound.
 *
 * A path loss over M members -- snapshot matching on M folds, annealed reverse-KL over logq(tau_k) on a temperature ladder,
 * kinetic penalties of M restarts -- is M times the same small launch.  Here the M members -- each with its own parameters,
 * data (or base draw), probes, adaptive step sequence and, if the caller wishes, its own save times -- are solved side by side by
 * one launch of M x ceil(B / 16) workgroups.  The envelope is the one of cnf_ensemble_eval_capacity (two layers, tanh then tanh
 * or identity, n_in <= 16, at most 64 hidden units, 16 with the identity; no conditioning, the default base, no lock-step
 * shards).  The handle gives the architecture, the regularisers and the wait bounds; its own parameters, conditioning and
 * solver state are not touched, and neither are the steps cnf_path_steps / cnf_path_vjp_steps keep.
 *
 * What the four calls share.
 *   Save times.  saveat_host is HOST memory: [K] when saveat_per_member is 0 -- one set of times for all members --, [M][K] when
 *   it is 1 -- member m reads saveat_host[m K .. m K + K).  Every set is checked as cnf_solve_path checks its own (finite,
 *   monotone along opts->t0 -> opts->t1, inside the closed span; for the sampling calls that span is the reversed one), for
 *   every member, before the handle is looked at: CNF_ERR_BAD_ARG, with a NULL handle too.
 *   The span.  Every member integrates opts->t0 -> opts->t1: there are no per-member start or end times and no steering, as the
 *   single-model path calls have none.  The t1_host / t0_host arguments of the argument lists these calls extend must be NULL
 *   (CNF_ERR_BAD_ARG otherwise).
 *   The slices.  path_out_dev is DEVICE memory, [M][K][B][D]: member m's slab is what cnf_solve_path files for it alone.
 *   Capacity.  M above the call's capacity is CNF_ERR_UNSUPPORTED with nothing enqueued; the caller splits the members.
 *   Heterogeneous members.  Arrays pending from cnf_ensemble_set_members are taken and dropped: these calls have no per-member
 *   batch sizes, lambdas or tolerances.
 *   Steps.  Every member files its accepted steps (t_n, signed h_n): at most 4096 per member for the two plain calls, at most
 *   1024 -- what one launch can differentiate -- for the two vjp calls (cnf_solve_path keeps 16384 for its one model).  A member
 *   of a plain call that accepts more still has its outputs and path; only cnf_ensemble_path_steps answers -1 for it.
 *   Failure of a member.  Per member status_out[m] is CNF_OK, CNF_ERR_NONFINITE, CNF_ERR_MAXITERS or CNF_ERR_UNSUPPORTED (its part
 *   of the launch gave up: a wait ran out, or -- vjp calls -- more accepted steps than one launch differentiates; the caller
 *   runs it again alone).  Whatever is not CNF_OK: that member's outputs and its slab of path_out_dev are NaN and its gradients
 *   zero; the other members are untouched.  The calls return CNF_OK whenever the launch ran. */
#ifndef CNFHIP_ENSEMBLE_PATH_H
#define CNFHIP_ENSEMBLE_PATH_H

/* Members per launch of cnf_inference_path_many / cnf_generate_path_many for this handle, mode and batch: the workgroups of one
 * wave of the plain ensemble form WITH the path that the device holds at once / ceil(B / 16).  0: no such form (everything
 * cnf_ensemble_eval_capacity refuses), or B > 8192. */
int cnf_ensemble_path_capacity(cnf_handle h, int mode, int B);

/* Members per launch of cnf_inference_path_vjp_many / cnf_generate_path_vjp_many: the smaller of the two directions' capacities
 * (each has its own kernels, hence its own register budget), so that one answer serves both calls.  0: no such form. */
int cnf_ensemble_path_vjp_capacity(cnf_handle h, int mode, int B);

/* cnf_inference_path_many: cnf_inference_many plus the members' paths.  One launch. */
cnf_status cnf_inference_path_many(cnf_handle h, int mode, int M, const float* params_dev, const float* xs, const float* eps, int B,
                                   const cnf_solve_opts* opts, const float* t1_host, float* logpx_dev, float* regs_dev,
                                   float* loss_out, int* status_out, cnf_solve_stats* stats_out, int trace_cap, void* stream,
                                   const float* saveat_host, int K, int saveat_per_member, float* path_out_dev);

/* cnf_generate_path_many: cnf_generate_many (logq_out may be NULL) plus the members' paths; opts is the REVERSED span and the
 * save times run along it.  The launch and the column kernel. */
cnf_status cnf_generate_path_many(cnf_handle h, int mode, int M, const float* params_dev, const float* z0, const float* eps, int B,
                                  const cnf_solve_opts* opts, const float* t0_host, float* xs_out, float* logq_out,
                                  int* status_out, cnf_solve_stats* stats_out, int trace_cap, void* stream,
                                  const float* saveat_host, int K, int saveat_per_member, float* path_out_dev);

/* cnf_inference_path_vjp_many: cnf_inference_path_vjp of M members.  params_dev [M][n_params], xs [M][B][nvars], eps
 * [M][B][n_in] (NULL in TestMode), cot_dev [M][4][B] or NULL, path_cot_dev [M][K][B][D] or NULL, logpx_dev [M][B], regs_dev
 * [M][3][B], path_out_dev [M][K][B][D] or NULL, grad_dev [M][n_params], grad_x_dev [M][B][n_in] or NULL: DEVICE memory;
 * status_out [M] and stats_out [M] (may be NULL): HOST.  With M = 1 it is cnf_inference_path_vjp, the same kernel on the same
 * arguments.  Two launches. */
cnf_status cnf_inference_path_vjp_many(cnf_handle h, int mode, int M, const float* params_dev, const float* xs, const float* eps,
                                       int B, const cnf_solve_opts* opts, const float* saveat_host, int K, int saveat_per_member,
                                       const float* cot_dev, const float* path_cot_dev, float* logpx_dev, float* regs_dev,
                                       float* path_out_dev, float* grad_dev, float* grad_x_dev, int* status_out,
                                       cnf_solve_stats* stats_out, void* stream);

/* cnf_generate_path_vjp_many: cnf_generate_path_vjp of M members.  z0 [M][B][n_in], cot_z_dev [M][B][n_in] or NULL, cot_logq_dev
 * [M][B] or NULL, path_cot_dev [M][K][B][D] or NULL (a cotangent of the STATE rows, as for cnf_generate_path_vjp: the caller adds
 * the -(sum_k g_k) z0 tail of a logq-path cotangent to grad_z0 itself; the Python call does, summing over k by a fixed tree of
 * additions so that a member's result does not depend on M -- cnf_generate_path_vjp's Python call leaves that sum to the tensor
 * library, hence the two agree to rounding there and bit for bit everywhere else), x_out [M][B][nvars], logq_out [M][B], path_out_dev or
 * NULL, grad_dev [M][n_params], grad_z0_dev [M][B][n_in] or NULL.  The launch, the partial sums and the column kernels. */
cnf_status cnf_generate_path_vjp_many(cnf_handle h, int mode, int M, const float* params_dev, const float* z0, const float* eps,
                                      int B, const cnf_solve_opts* opts, const float* saveat_host, int K, int saveat_per_member,
                                      const float* cot_z_dev, const float* cot_logq_dev, const float* path_cot_dev, float* x_out,
                                      float* logq_out, float* path_out_dev, float* grad_dev, float* grad_z0_dev, int* status_out,
                                      cnf_solve_stats* stats_out, void* stream);

/* The accepted steps of member `member` of the last of the four calls above on this handle: returns their number and copies
 * min(number, cap) pairs into t_host (t_n) and h_host (signed h_n) (HOST; may be NULL).  -1: there is no such call or member,
 * the member was not CNF_OK, or it accepted more steps than a member files. */
int cnf_ensemble_path_steps(cnf_handle h, int member, float* t_host, float* h_host, int cap);

#endif /* CNFHIP_ENSEMBLE_PATH_H */
