/* Ensembles: the C ABI of libcnfhip.so for M independent models of one architecture.  Part of cnfhip.h, which includes it where
 * its types are declared (inside its extern "C" block): include cnfhip.h, not this file.  Like the sampling direction
 * (cnfhip_generate.h) the entry points have a header and a binding table (`_lib.ENSEMBLE_EXPORTS`) of their own, because the
 * tests pin the list that cnfhip.h itself declares (`_lib.EXPORTS`); tests/test_ensemble_host.py holds this header to the same
 * rule: every name declared here is exported by the library and bound. */
#ifndef CNFHIP_ENSEMBLE_H
#define CNFHIP_ENSEMBLE_H

/* ---- cross-validation folds, bootstrap replicas, seeds, sweeps: M models' loss and gradient in ONE launch ----
 * The reference trains its README / regression networks at batch_size = 32 (src/exts/mlj_ext/core_icnf.jl:59-73): a gradient
 * of ONE such model is two workgroups.  Here M models of the handle's architecture -- each with its own parameters, data batch,
 * probes, end time and adaptive step sequence -- are solved and differentiated side by side by one launch of M x ceil(B / 16)
 * workgroups; the members never wait for each other.  The handle gives the architecture, the regularisers and the wait
 * bounds; its own parameters, recorded solve and gradient state are not touched (cnf_grad_x and a record end, as with every
 * gradient call).
 *
 * cnf_ensemble_capacity: the largest M one launch takes for this handle, mode and batch (the workgroups the device holds at
 * once / ceil(B / 16), capped so that every member keeps at least 64 step slots within the trajectory budget of one model's
 * call).  0: no ensemble form -- a network outside the envelope of the in-launch gradient (two layers, tanh first, tanh or
 * identity second, n_in <= 16, at most 64 hidden units), a conditional model, a non-default base distribution,
 * cnf_set_grad_ys on, lock-step shards, or CNF_WAVE=0 / CNF_WAVE_GRAD=0 / CNF_PERSISTENT=0. */
int cnf_ensemble_capacity(cnf_handle h, int mode, int B);

/* cnf_loss_grad_many: params_dev [M][n_params], xs [M][B][nvars], eps [M][B][n_in] (NULL in TestMode) and grad_dev
 * [M][n_params] are DEVICE memory; t1_host (NULL: opts->t1 for all), loss_out, status_out and stats_out (may be NULL) are HOST
 * arrays of M.  Synchronous.  Per member status_out[m]: CNF_OK; CNF_ERR_NONFINITE; CNF_ERR_MAXITERS; or CNF_ERR_UNSUPPORTED =
 * this member's part of the launch gave up (a wait ran out, or it accepted more steps than its store holds): nothing of it is
 * valid, its loss is NaN and its gradient zeros -- the caller runs it again on its own with cnf_loss_grad.  Whatever the
 * status is not CNF_OK, the member's loss is NaN and its gradient zeros.
 * Returns CNF_OK whenever the launch ran; CNF_ERR_UNSUPPORTED with nothing enqueued if M exceeds cnf_ensemble_capacity (or
 * that is 0, or opts->kernel is CNF_KERNEL_GENERIC); CNF_ERR_BAD_ARG / CNF_ERR_BAD_SHAPE (NULL pointers, M < 1, B < 1, bad
 * options) before anything touches the device. */
cnf_status cnf_loss_grad_many(cnf_handle h, int mode, int M, const float* params_dev, const float* xs, const float* eps, int B,
                              const cnf_solve_opts* opts, const float* t1_host, float* loss_out, float* grad_dev,
                              int* status_out, cnf_solve_stats* stats_out, void* stream);

/* The signed sizes of the steps member `member` accepted in the last ensemble gradient call -- cnf_loss_grad_many or
 * cnf_inference_vjp_many (cnfhip_ensemble_vjp.h), whichever came last --, in the manner of cnf_grad_steps: returns their number
 * and copies min(number, cap) of them into hs (HOST; may be NULL).  -1: no such member, or it gave up. */
int cnf_ensemble_steps(cnf_handle h, int member, float* hs, int cap);

#endif /* CNFHIP_ENSEMBLE_H */
