/* Ensemble forward-mode: the C ABI of libcnfhip.so for the TANGENTS (Jacobian-vector products) of M independent models of one
 * architecture in one launch -- cnfhip_jvp.h with a member axis, the last of the single-model capabilities to get one.  Part of
 * cnfhip.h, which includes it where its types are declared (inside its extern "C" block): include cnfhip.h, not this file.  The
 * entry points have a header and a binding table (`_lib.ENSEMBLE_JVP_EXPORTS`) of their own, because the tests pin the lists the
 * other headers declare; tests/test_ensemble_jvp_host.py holds this header to the same rule: every name declared here is
 * exported by the library and bound.
 *
 * A call is cnf_inference_many / cnf_generate_many with every member's step attempts kept on the device, plus ONE more launch:
 * the ensemble form of k_tangent_wave (csrc/cnf_tangent.hip), grid (ceil(B / 16), R, M), enqueued right behind the solve on the
 * same stream with no host wait in between.  It reads each member's final state and attempts where the solve left them and
 * replays the member's ACCEPTED steps for R directions, one wave per (16-column tile, direction, member).  It has no controller,
 * no meeting and no atomics, so it needs no residency: the capacity of a call is cnf_ensemble_eval_capacity, the solve's.  The
 * guard is per member: for a member whose part of the solve gave up, did not reach its end time, went non-finite or made more
 * attempts than trace_cap the launch writes nothing, and the member's rows of the tangent outputs stay NaN (the call fills
 * them beforehand).
 *
 * Envelope: what cnf_ensemble_eval_capacity takes (two layers, tanh then tanh or identity, n_in <= 16, at most 64 hidden units,
 * 16 with the identity; no conditioning; the default base; no lock-step shards) -- which is the tangent kernel's own envelope --;
 * TrainMode in both compute modes and TestMode.  cnf_ensemble_set_members (counts, lambdas, tolerances) applies and is
 * consumed, as by the other ensemble calls: a member with its own count computes its first counts[m] columns, and no tangent
 * column at or behind the count is read or written (NaN).  Bases pending from cnf_ensemble_set_bases are consumed and the call
 * is refused with CNF_ERR_UNSUPPORTED.
 *
 * d_ps: DEVICE, [M][R][n_params] in the layout of cnf_set_params, or NULL (zero).  At least one of the two directions is given;
 * 1 <= R <= 65535, the same for all members.  trace_cap: step attempts a member has room for; 0 = min(maxiters, 1024), at most
 * 65536.  Arguments are checked before any device is asked for, with a NULL handle too: CNF_ERR_BAD_ARG / CNF_ERR_BAD_SHAPE as
 * cnf_inference_many, and CNF_ERR_BAD_ARG for both directions NULL, R or trace_cap out of range, a NULL tangent output.  Per
 * member status_out[m], loss, statistics and return value as cnf_inference_many; a member with more attempts than trace_cap
 * reports CNF_ERR_UNSUPPORTED too (the caller runs it again alone with cnf_inference_jvp / cnf_generate_jvp), and whatever the
 * status is not CNF_OK the member's outputs are NaN.  stats' launches count the tangent launch.  Synchronous.  The handle's own
 * parameters, record and single-model tangent trace are not touched: a record made before these calls still pulls back, and
 * cnf_jvp_steps answers as before. */
#ifndef CNFHIP_ENSEMBLE_JVP_H
#define CNFHIP_ENSEMBLE_JVP_H

/* cnf_inference_many plus R tangents of every member's four outputs along (d_ps, d_xs).  params_dev [M][n_params], xs
 * [M][B][nvars], eps [M][B][n_in] (NULL in TestMode), d_xs [M][R][B][nvars] or NULL: DEVICE.  t1_host: HOST [M] or NULL.
 * logpx_dev [M][B], regs_dev [M][3][B]: cnf_inference_many's, bit for bit.  d_out_dev: DEVICE, [M][R][4][B], rows (d logpx, d E,
 * d n, d A) as cnf_inference_jvp defines them.  loss_out (may be NULL), status_out, stats_out (may be NULL): HOST arrays of M. */
cnf_status cnf_inference_jvp_many(cnf_handle h, int mode, int M, const float* params_dev, const float* xs, const float* eps, int B,
                                  const float* d_ps, const float* d_xs, int R, const cnf_solve_opts* opts, const float* t1_host,
                                  int trace_cap, float* logpx_dev, float* regs_dev, float* d_out_dev, float* loss_out, int* status_out,
                                  cnf_solve_stats* stats_out, void* stream);

/* The sampling counterpart: cnf_generate_many (the caller passes the REVERSED span; t0_host: the members' start times or NULL)
 * plus R tangents along (d_ps, d_z0).  z0 [M][B][n_in], d_z0 [M][R][B][n_in] or NULL.  z_out [M][B][n_in]: ALL rows of the final
 * state (cnf_generate_many's xs_out are its first nvars rows, bit for bit); logq_out [M][B]: cnf_generate_many's, bit for bit.
 * d_z: DEVICE, [M][R][B][n_in];  d_logq [M][R][B] = -z0 . dz0 + d dlogp. */
cnf_status cnf_generate_jvp_many(cnf_handle h, int mode, int M, const float* params_dev, const float* z0, const float* eps, int B,
                                 const float* d_ps, const float* d_z0, int R, const cnf_solve_opts* opts, const float* t0_host,
                                 int trace_cap, float* z_out, float* logq_out, float* d_z, float* d_logq, int* status_out,
                                 cnf_solve_stats* stats_out, void* stream);

/* The accepted steps of member `member` of the last of the two calls above on this handle, in the shape of cnf_jvp_steps:
 * returns their number and copies min(number, cap) pairs into t_host (t_n, the controller's own time of the attempt) and h_host
 * (signed h_n) (HOST; may be NULL).  -1: no such member, it was not CNF_OK, or another call has written the trace since. */
int cnf_ensemble_jvp_steps(cnf_handle h, int member, float* t_host, float* h_host, int cap);

#endif /* CNFHIP_ENSEMBLE_JVP_H */
