/* Forward-mode derivatives: the C ABI of libcnfhip.so for the TANGENT (Jacobian-vector product) of inference and of sampling --
 * what the reference's tests take with `DifferentiationInterface.gradient(diff_loss, AutoEnzyme(mode = Forward), ...)` w.r.t.
 * `ps` and w.r.t. the data in every block of test/call_tests.jl (:32-66, :239-252), one pushforward per input entry.  Part of
 * cnfhip.h, which includes it where its types are declared (inside its extern "C" block): include cnfhip.h, not this file.  The
 * entry points have a header and a binding table (`_lib.JVP_EXPORTS`) of their own, because the tests pin the list that
 * cnfhip.h itself declares; tests/test_jvp_ref_host.py holds this header to the same rule: every name declared here is exported
 * by the library and bound.
 *
 * A call is the solve of the call it extends plus ONE more launch.  For inference the primal half is cnf_inference's own one-launch
 * solve with its step attempts filed on the device; the tangent launch (k_tangent_wave, csrc/cnf_tangent.hip) is enqueued right
 * behind it on the same stream, with no host wait in between, reads the attempts and the solve's final state from device memory
 * and replays the ACCEPTED steps for R directions at once, one wave per (16-column tile, direction).  The step sizes are
 * constants of the derivative, as in every gradient of this library (the discrete map through the accepted steps), so the
 * tangent launch has no controller, no error norm and no wait of any kind.  It writes nothing when the solve it follows gave
 * up, did not reach t1 or went non-finite.  When the one-launch solve gives up (cnf_solve_fallbacks counts it), or with
 * opts->kernel = CNF_KERNEL_GENERIC, the solve runs one attempt at a time as cnf_solve_path's streamed route does, the host
 * files the accepted steps, and the tangent launch follows over those.  Sampling's primal half is cnf_generate_record's RECORDED
 * solve (that call is what `generate(with_logp)` runs, and its route differs from the plain one-launch solve in the last bits and
 * sometimes by a step): z and logq are that call's bit for bit, and the tangent launch follows over the record's accepted steps.
 *
 * Envelope: two layers, tanh then tanh or identity (a one-layer tanh network through its appended identity), n_in <= 16, at most
 * 64 hidden units (16 with the identity), no conditioning, the default base distribution, no lock-step shards, any B the plain
 * one-launch solve takes; TrainMode in both compute modes and TestMode.  CNF_ERR_UNSUPPORTED outside it, and for a solve of more
 * attempts (accepted + rejected) than trace_cap -- in both cases no output array is written.
 *
 * d_ps: DEVICE, [R][n_params] in the layout of cnf_set_params, or NULL (zero).  At least one of the two directions is given;
 * 1 <= R <= 65535.  trace_cap: step attempts the call has room for; 0 = 4096, at most 65536.  Arguments are checked before any
 * device is asked for: CNF_ERR_BAD_ARG for a NULL handle, NULL arrays, both directions NULL, R or trace_cap out of range,
 * CNF_ERR_BAD_SHAPE for B < 1.  Synchronous; inferences submitted on the handle are collected first.  The handle's parameters
 * stay; like every solve, the call ends a record of cnf_inference_record / cnf_generate_record; a buffer given to
 * cnf_set_step_trace is not written by these calls (their attempts go to the handle's own).  stats: those of the solve,
 * launches counting every kernel launch the call made: the tangent launch (also one that went out behind a solve which then gave
 * up and wrote nothing) and sampling's post-processing launch too. */
#ifndef CNFHIP_JVP_H
#define CNFHIP_JVP_H

/* cnf_inference (test/call_tests.jl:32-66 with mode = Forward: `inference` inside diff_loss) plus R tangents of its four outputs
 * along (d_ps, d_xs).  xs [B][nvars], eps [B][n_in] (TrainMode; NULL in TestMode), d_xs: DEVICE, [R][B][nvars] or NULL.
 * logpx [B], regs [3][B]: cnf_inference's, bit for bit.  d_out: DEVICE, [R][4][B], rows (d logpx, d E, d n, d A):
 *   d logpx = -z(t1) . dz(t1) - d dlogp,   d E = int zdot . dzdot / |zdot|,   d n = int (eps'J) . d(eps'J) / |eps'J|,
 *   d A = z_aug . dz_aug / |z_aug|;   a term whose norm is 0 is 0; rows the handle does not integrate (lambda = 0, TestMode) are 0. */
cnf_status cnf_inference_jvp(cnf_handle h, int mode, const float* xs, const float* eps, int B, const float* d_ps, const float* d_xs,
                             int R, const cnf_solve_opts* opts, int trace_cap, float* logpx, float* regs, float* d_out,
                             cnf_solve_stats* stats, void* stream);

/* The sampling counterpart (test/call_tests.jl:239-252 with mode = Forward; src/base_icnf.jl:358-380, :202-211): the solve of
 * u0 = [z0; 0] over opts->t0 -> opts->t1 (the caller passes reverse(tspan)) plus R tangents along (d_ps, d_z0).  z0 [B][n_in],
 * d_z0: DEVICE, [R][B][n_in] or NULL.  z_out [B][n_in] (the sample is its first nvars rows), logq [B] = logpdf(N(0, I), z0) +
 * dlogp: cnf_generate_record's, bit for bit; d_z: DEVICE, [R][B][n_in];  d_logq [R][B] = -z0 . dz0 + d dlogp. */
cnf_status cnf_generate_jvp(cnf_handle h, int mode, const float* z0, const float* eps, int B, const float* d_ps, const float* d_z0,
                            int R, const cnf_solve_opts* opts, int trace_cap, float* z_out, float* logq, float* d_z, float* d_logq,
                            cnf_solve_stats* stats, void* stream);

/* The accepted steps of the last cnf_inference_jvp / cnf_generate_jvp on this handle, as cnf_path_steps gives them: returns their
 * number and copies min(number, cap) pairs into t_host (t_n) and h_host (signed h_n) (HOST; may be NULL).  -1: there is none
 * (no such call yet, or it failed).  After cnf_inference_jvp t_n is the controller's own time of the attempt; after
 * cnf_generate_jvp, whose record keeps the step sizes alone, t_n = t0 + h_0 + .. + h_{n-1} summed in float (it may differ from the
 * controller's time in the last bit; nothing is computed from it). */
int cnf_jvp_steps(cnf_handle h, float* t_host, float* h_host, int cap);

#endif /* CNFHIP_JVP_H */
