/* Heterogeneous ensembles: per-member batch size, regularisers and tolerances for the ensemble calls of cnfhip_ensemble.h,
 * cnfhip_ensemble_eval.h, cnfhip_ensemble_vjp.h and cnfhip_ensemble_generate_vjp.h.  Part of cnfhip.h, which includes it where
 * its types are declared (inside its extern "C" block): include cnfhip.h, not this file.  The entry points have a header and a
 * binding table (`_lib.ENSEMBLE_HETERO_EXPORTS`) of their own, because the tests pin the lists the other headers declare and no
 * signature of theirs changes; tests/test_ensemble_hetero_host.py holds this header to the same rule: every name declared here
 * is exported by the library and bound. */
#ifndef CNFHIP_ENSEMBLE_HETERO_H
#define CNFHIP_ENSEMBLE_HETERO_H

/* ---- folds of unequal size, a sweep over lambda_1..3, a sweep over the tolerances: still ONE launch ----
 * The reference constructs every model with its own regularisers and solver options (`construct`: lambda_1, lambda_2, lambda_3
 * and sol_kwargs, src/base_icnf.jl:26-38) and calls it on a batch of whatever size; the members of an ensemble call could so
 * far differ in parameters, data, probes and end (start) time only.
 *
 * cnf_ensemble_set_members: HOST arrays for the NEXT ensemble call on the handle -- cnf_loss_grad_many, cnf_inference_many,
 * cnf_generate_many, cnf_inference_vjp_many or cnf_generate_vjp_many -- each NULL (that call's own value for every member) or:
 *   counts [M]     the members' batch sizes, 1 <= counts[m] <= B.  Every array of the call keeps its rectangular shape,
 *                  [M][B].., with B >= the largest count; the device neither reads nor writes a column at or behind its member's
 *                  count, in any input or output.  Losses are means over the member's own count; the grid stays M x ceil(B / 16)
 *                  workgroups, those beyond a member's ceil(counts[m] / 16) leave at once, and the capacity calls are asked at B.
 *   lams [M][3]    the members' lambda_1, lambda_2, lambda_3 (the replacement of `construct`'s, src/base_icnf.jl:26-38): zero
 *                  exactly where the handle's is, because that decides the rows of the state.  They weigh the loss and the
 *                  built-in loss's cotangent; the per-sample-cotangent calls read no lambda.
 *   tols [M][2]    the members' (abstol, reltol), finite and positive, in place of the call's cnf_solve_opts' (the replacement
 *                  of sol_kwargs' abstol / reltol, src/base_icnf.jl:26-38).
 * The arrays are copied; they are checked by the call they apply to, before it asks for a device, and that call returns
 * CNF_ERR_BAD_ARG with nothing enqueued if its M differs, a count is outside [1, B], a tolerance is not finite and positive or
 * a lambda is not finite or is zero where the handle's is not (or the reverse).  They are CONSUMED by that call whether it
 * succeeds or not: no later call is steered by them.  Member m of such a call computes, bit for bit, what the call with M = 1
 * and B = counts[m] computes on a handle made with that member's lambdas and tolerances.  The statistics, the steps
 * (cnf_ensemble_steps, cnf_ensemble_eval_steps) and the status per member are as before.
 * cnf_inference_path_vjp and cnf_generate_path_vjp, which run one member, consume the arrays and ignore them.
 * Returns CNF_ERR_BAD_ARG for a NULL handle or M < 1 (nothing is pending then). */
cnf_status cnf_ensemble_set_members(cnf_handle h, int M, const int* counts, const float* lams, const float* tols);

/* Drops what cnf_ensemble_set_members left, if anything (the replacement of nothing in the reference: its models are
 * constructed anew, src/base_icnf.jl:26-38). */
cnf_status cnf_ensemble_clear_members(cnf_handle h);

#endif /* CNFHIP_ENSEMBLE_HETERO_H */
