/* Ensemble inference and sampling: the C ABI of libcnfhip.so for scoring and sampling M independent models of one architecture
 * in one launch -- the other half of cnfhip_ensemble.h, which trains them.  Part of cnfhip.h, which includes it where its types
 * are declared (inside its extern "C" block): include cnfhip.h, not this file.  The entry points have a header and a binding
 * table (`_lib.ENSEMBLE_EVAL_EXPORTS`) of their own, because the tests pin the lists that cnfhip.h and cnfhip_ensemble.h
 * declare; tests/test_ensemble_eval_host.py holds this header to the same rule: every name declared here is exported by the
 * library and bound. */
#ifndef CNFHIP_ENSEMBLE_EVAL_H
#define CNFHIP_ENSEMBLE_EVAL_H

/* ---- held-out log-likelihoods of folds and replicas, a bagged density and its samples: M models in ONE launch ----
 * One `inference` / `generate` of a README-sized model is a launch of two to five 64-thread workgroups.  Here M models of the
 * handle's architecture -- each with its own parameters, data (or base draw), probes, start / end time and adaptive step
 * sequence -- are solved side by side by one launch of M x ceil(B / 16) workgroups of one wave; the members never wait for
 * each other.  The handle gives the architecture, the regularisers and the wait bounds; its own parameters, conditioning,
 * solver state and recorded solve are not touched: a record made before these calls still pulls back.
 *
 * cnf_ensemble_eval_capacity: the largest M one launch takes for this handle, mode and batch: the workgroups of one wave the
 * device holds at once / ceil(B / 16).  0: no ensemble form -- everything cnf_ensemble_capacity refuses (a network outside
 * two layers, tanh first, tanh or identity second, n_in <= 16, at most 64 hidden units, 16 with the identity; a conditional
 * model; a non-default base distribution; cnf_set_grad_ys on; lock-step shards; CNF_WAVE=0 / CNF_PERSISTENT=0), or more than
 * 512 tiles per member (B > 8192). */
int cnf_ensemble_eval_capacity(cnf_handle h, int mode, int B);

/* cnf_inference_many: `cnf_inference` of M members.  params_dev [M][n_params], xs [M][B][nvars], eps [M][B][n_in] (NULL in
 * TestMode), logpx_dev [M][B] and regs_dev [M][3][B] are DEVICE memory; t1_host (NULL: opts->t1 for all), loss_out (may be
 * NULL), status_out and stats_out (may be NULL) are HOST arrays of M.  trace_cap > 0: every member keeps the first trace_cap
 * step attempts of its solve for cnf_ensemble_eval_steps.  Synchronous.  Per member status_out[m]: CNF_OK; CNF_ERR_NONFINITE;
 * CNF_ERR_MAXITERS; or CNF_ERR_UNSUPPORTED = this member's part of the launch gave up (a wait ran out): the caller runs it
 * again on its own with cnf_inference.  Whatever the status is not CNF_OK, the member's outputs and loss are NaN.
 * Returns CNF_OK whenever the launch ran; CNF_ERR_UNSUPPORTED with nothing enqueued if M exceeds cnf_ensemble_eval_capacity
 * (or that is 0, or opts->kernel is CNF_KERNEL_GENERIC); CNF_ERR_BAD_ARG / CNF_ERR_BAD_SHAPE (NULL pointers, M < 1, B < 1,
 * unknown mode, bad options) before anything touches the device -- with a NULL handle too. */
cnf_status cnf_inference_many(cnf_handle h, int mode, int M, const float* params_dev, const float* xs, const float* eps, int B,
                              const cnf_solve_opts* opts, const float* t1_host, float* logpx_dev, float* regs_dev, float* loss_out,
                              int* status_out, cnf_solve_stats* stats_out, int trace_cap, void* stream);

/* cnf_generate_many: sampling of M members.  z0 [M][B][n_in] (the base draws), eps [M][B][n_in] (NULL in TestMode), xs_out
 * [M][B][nvars] and logq_out [M][B] (may be NULL) are DEVICE memory.  Every member integrates u0 = [z0; 0] over `opts` -- the
 * caller passes the REVERSED span, as cnf_generate_record takes it -- from its own start time t0_host[m] (HOST, NULL:
 * opts->t0 for all; a steered member starts elsewhere, every member ends at opts->t1).  xs_out are the first nvars rows of the
 * final state and logq = logpdf(N(0, I), z0) + dlogp, the arithmetic of cnf_generate_record.  Status, statistics, trace and
 * return value as for cnf_inference_many. */
cnf_status cnf_generate_many(cnf_handle h, int mode, int M, const float* params_dev, const float* z0, const float* eps, int B,
                             const cnf_solve_opts* opts, const float* t0_host, float* xs_out, float* logq_out, int* status_out,
                             cnf_solve_stats* stats_out, int trace_cap, void* stream);

/* The step attempts of member `member` in the last of the two calls above that was made with trace_cap > 0: returns their
 * number (accepted and rejected) and copies min(number, cap, trace_cap) rows (t, signed h, EEst, accepted) into rows (HOST,
 * 4 floats each; may be NULL).  -1: no such member, it gave up, or no trace was kept. */
int cnf_ensemble_eval_steps(cnf_handle h, int member, float* rows, int cap);

#endif /* CNFHIP_ENSEMBLE_EVAL_H */
