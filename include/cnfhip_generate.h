/* The sampling direction of the C ABI of libcnfhip.so.  Part of cnfhip.h, which includes it where its types are declared
 * (inside its extern "C" block): include cnfhip.h, not this file.  The two entry points have a header and a binding table
 * (`_lib.SAMPLING_EXPORTS`) of their own because the tests of the density direction pin the list that cnfhip.h itself declares
 * (`_lib.EXPORTS`, 62 names); tests/test_gen_vjp_ref_host.py holds this header to the same rule: every name declared here is
 * exported by the library and bound. */
#ifndef CNFHIP_GENERATE_H
#define CNFHIP_GENERATE_H

/* ---- differentiable sampling: `generate` with the log-density of the sample, and its vector-Jacobian product ----
 * (generate integrates the same augmented state over reverse(tspan), src/base_icnf.jl:358-380, and keeps rows 1..nvars,
 * :202-211; the dlogp row it has integrated on the way is the density of the sample: what a reverse-KL / variational loss
 * E_z[log q(x(z)) - log p(x(z))] or any other loss on samples needs, with its gradient.)
 *
 * cnf_generate_record: the solve from u0 = [z0; 0] over (opts->t0, opts->t1) -- the caller passes the REVERSED span: t0 =
 * tspan[1], t1 = tspan[0] -- RECORDED on the handle.  z0 is n_in x B (ALL n_in rows, the augmented ones included), eps n_in x B
 * (NULL in TestMode), DEVICE memory.  z_out (n_in x B) = rows 1..n_in of the final state (the sample is its first nvars rows),
 * logq[B] = logpdf(basedist, z0) + dlogp: the log-density of the whole n_in-dimensional final state under the flow, the
 * counterpart of what cnf_inference scores (TestMode: exact; TrainMode: the Hutchinson estimate for this eps).  The record
 * follows the rules of cnf_inference_record (it ends with the next call that solves, uploads parameters or conditioning, or
 * changes the base distribution; eps must stay alive and unchanged while it is used); z0 is copied, the caller's array need
 * not stay alive.  CNF_ERR_UNSUPPORTED where the gradient kernels do not take the network.
 *
 * cnf_generate_pullback: grad[n_params] = sum_b ( <cot_z[., b], d z_b / d ps> + cot_logq[b] d logq_b / d ps ) through the
 * recorded steps, and, if grad_z0 is not NULL, the same w.r.t. z0 (n_in x B).  cot_z (n_in x B) or cot_logq (B) may be NULL
 * (= zeros); both NULL: CNF_ERR_BAD_ARG.  cnf_grad_steps and, with cnf_set_grad_ys on, cnf_grad_ys apply afterwards;
 * cnf_grad_x does not (CNF_ERR_BAD_ARG).  May be called several times on one record.  The two kinds of record do not mix:
 * cnf_inference_pullback on a sampling record and cnf_generate_pullback on an inference record return CNF_ERR_BAD_ARG. */
cnf_status cnf_generate_record(cnf_handle h, int mode, const float* z0, const float* eps, int B,
                               const cnf_solve_opts* opts, float* z_out, float* logq,
                               cnf_solve_stats* stats, void* stream);
cnf_status cnf_generate_pullback(cnf_handle h, const float* cot_z, const float* cot_logq, int B, float* grad,
                                 float* grad_z0, void* stream);

#endif /* CNFHIP_GENERATE_H */
