/* Ensembles with a base distribution per member, fixed or learnable: a Gaussian base of its own for every member of the ensemble
 * calls of cnfhip_ensemble.h, cnfhip_ensemble_eval.h, cnfhip_ensemble_vjp.h and cnfhip_ensemble_generate_vjp.h.  Part of
 * cnfhip.h, which includes it where its types are declared (inside its extern "C" block): include cnfhip.h, not this file.  The
 * entry points have a header and a binding table (`_lib.ENSEMBLE_BASE_EXPORTS`) of their own, because the tests pin the lists the
 * other headers declare and no signature of theirs changes; tests/test_ensemble_base_host.py holds this header to the same rule:
 * every name declared here is exported by the library and bound. */
#ifndef CNFHIP_ENSEMBLE_BASE_H
#define CNFHIP_ENSEMBLE_BASE_H

/* ---- a base per member: N(mean_m, L_m L_m'), still ONE launch of the solve, no host wait for the base ----
 * The reference constructs every model with a base distribution of its own (`basedist` of `construct`, src/base_icnf.jl:16-21),
 * evaluates logpdf(icnf.basedist, z) at the final state (:155, :177) and samples it with rand!(rng, icnf.basedist, new_xs)
 * (:320-393).  A handle made with a non-default base (cnf_set_basedist) is still refused by every ensemble call; the members'
 * bases are given here, for a handle with the default base.
 *
 * cnf_ensemble_set_bases: DEVICE arrays for the NEXT ensemble call on the handle -- cnf_loss_grad_many, cnf_inference_many,
 * cnf_generate_many, cnf_inference_vjp_many or cnf_generate_vjp_many:
 *   mean_dev [M][n_in]
 *   chol_dev        kind 1 (diagonal): sigma, [M][n_in];  kind 2 (dense): L, [M][n_in][n_in], ROW-major and lower triangular
 *                   (the entries above the diagonal are not read), the layout cnf_set_basedist takes chol in.
 * The call is stream-ordered: it enqueues one small kernel on `stream` that reduces each member's base on the device, in double,
 * rounded once to float32 -- W = inv(L) by forward substitution, P = W' W from the rounded W (as cnf_set_basedist forms it),
 * c = sum_i log W_ii - n_in / 2 log(2 pi) -- into buffers of the handle (mu and P padded to 16 rows, as the gradient launch reads
 * them), and returns.  There is no host wait (the first call for a larger M grows the buffers); the ensemble call the bases apply to
 * must be enqueued on the same stream.  A member with a non-finite entry or a non-positive diagonal does not poison the launch:
 * the kernel marks it, it is solved under N(0, I), and the call the bases apply to reports CNF_ERR_BAD_ARG in that member's
 * status_out (its outputs are then not valid).  Like cnf_ensemble_set_members the bases apply to the next ensemble call on the
 * handle and are CONSUMED by it whether it succeeds or not; that call returns CNF_ERR_BAD_ARG with nothing enqueued if its M
 * differs.  The path calls (cnf_inference_path_many, cnf_generate_path_many, cnf_inference_path_vjp(_many),
 * cnf_generate_path_vjp(_many)) consume pending bases and return CNF_ERR_UNSUPPORTED with nothing enqueued.
 * With bases the calls compute
 *   logpx[m][b] = c_m - 1/2 |W_m (z_b(t1) - mean_m)|^2 - dlogp_b   afresh from the final columns (a column pass behind the launch;
 *                 the regulariser rows, the statistics and the step sequences are those of the call without bases: the base does
 *                 not enter the solve), loss_out[m] under the member's base, count and lambdas;
 *   gradients     with the terminal cotangent P_m (z(t1) - mean_m) in place of z(t1), inside the one gradient launch;
 *   logq[m][b]    = logpdf_m(z0_b) + dlogp_b and grad_z0 with the + g_logq d logpdf_m(z0) / d z0 tail (sampling; z0 is the caller's:
 *                 cnf_ensemble_base_sample forms it).
 * mean = 0, L = I gives the gradients of the call without bases bit for bit.  Member m of a call equals the M = 1 call on its
 * slices, bases included, bit for bit.
 * Returns CNF_ERR_BAD_ARG for a NULL handle or pointer, M < 1 or a kind other than 1 and 2 (nothing is pending then). */
cnf_status cnf_ensemble_set_bases(cnf_handle h, int M, int kind, const float* mean_dev, const float* chol_dev, void* stream);

/* Drops what cnf_ensemble_set_bases left, if anything (the replacement of nothing in the reference: its models are constructed
 * anew with their `basedist`, src/base_icnf.jl:16-21). */
cnf_status cnf_ensemble_clear_bases(cnf_handle h);

/* The largest M of cnf_loss_grad_many (per_sample = 0) or cnf_inference_vjp_many (per_sample != 0) WITH bases (the members'
 * logpdf(icnf.basedist, z), src/base_icnf.jl:155, :177, enters their terminal cotangent): those calls run kernels of their own,
 * with their own register budget.  0: no ensemble form.  The other calls' capacities do not depend on bases. */
int cnf_ensemble_base_capacity(cnf_handle h, int mode, int B, int per_sample);

/* z0[m][b] = mean_m + L_m normals[m][b] ([M][B][n_in] both, DEVICE, distinct buffers; rand!(rng, icnf.basedist, new_xs),
 * src/base_icnf.jl:320-393, per member) with the prepared bases: the pending ones (they stay pending for the ensemble call), else
 * those of the last ensemble call that had some.  The arithmetic is cnf_base_sample's: the sum over j upwards, the mean added
 * last; diagonal kind: one fma.  Stream-ordered.  CNF_ERR_BAD_ARG when there are no such bases of M members. */
cnf_status cnf_ensemble_base_sample(cnf_handle h, int M, const float* normals_dev, float* z0_dev, int B, void* stream);

/* The M-member form of cnf_base_logpdf_pullback (the derivative of logpdf(icnf.basedist, z), src/base_icnf.jl:155, :177, w.r.t.
 * the base): g_mean [M][n_in], g_chol ([M][n_in], or [M][n_in][n_in] row-major with zeros above the diagonal) =
 * sum_b w[m][b] d logpdf_m(s_b) / d (mean_m, chol_m) with the formulas of cnfhip_basegrad.h per member, where s_b is what the LAST
 * ensemble call with bases left in the ensemble's column store: the final states z(t1) of cnf_inference_many, cnf_loss_grad_many
 * and cnf_inference_vjp_many (w = the cotangent of logpx; the loss has w = -1 / counts[m]), the z0 columns of the sampling calls
 * (w = the cotangent of logq: the partial derivative at FIXED z0).  It uses that call's prepared bases and its counts: a column at
 * or behind a member's count contributes nothing.  Any later ensemble call on the handle ends that state.  One workgroup per
 * member, the samples added upwards, no float atomics: the same bits from run to run.  Stream-ordered.  CNF_ERR_BAD_ARG: a NULL
 * pointer, no such call on record, or another M or B than it had. */
cnf_status cnf_ensemble_base_logpdf_pullback(cnf_handle h, int M, const float* w_dev, int B, float* g_mean_dev, float* g_chol_dev,
                                             void* stream);

/* The M-member form of cnf_base_sample_pullback, the vector-Jacobian product of cnf_ensemble_base_sample (the draw of
 * rand!(rng, icnf.basedist, new_xs), src/base_icnf.jl:320-393); stateless: g_mean[m] = sum_b g_z0[m][b], g_chol[m] =
 * tril(sum_b g_z0[m][b] normals[m][b]') (diagonal kind: its diagonal).  normals_dev and g_z0_dev are [M][B][n_in].  The members'
 * counts are an explicit argument: counts_dev, DEVICE, [M] batch sizes within [1, B], or NULL (every member has B columns); a
 * column at or behind a member's count contributes nothing.  The same fixed summation order; stream-ordered. */
cnf_status cnf_ensemble_base_sample_pullback(cnf_handle h, int M, int kind, const float* normals_dev, const float* g_z0_dev, int B,
                                             const int* counts_dev, float* g_mean_dev, float* g_chol_dev, void* stream);

#endif /* CNFHIP_ENSEMBLE_BASE_H */
