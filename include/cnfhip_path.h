/* Flow paths: the C ABI of libcnfhip.so for the state of a solve at caller-given times -- what `solve(prob; saveat = ...)` gives
 * the reference's users (its `inference_prob` / `generate_prob` return SciMLBase ODEProblems, src/base_icnf.jl:266-380).  Part of
 * cnfhip.h, which includes it where its types are declared (inside its extern "C" block): include cnfhip.h, not this file.  The
 * entry points have a header and a binding table (`_lib.PATH_EXPORTS`) of their own, because the tests pin the list that
 * cnfhip.h itself declares; tests/test_path_host.py holds this header to the same rule: every name declared here is exported
 * by the library and bound. */
#ifndef CNFHIP_PATH_H
#define CNFHIP_PATH_H

/* ---- dense output: the columns of the flow between t0 and t1 ----
 * Tsit5 carries a free 4th-order interpolant over the k_1 .. k_7 of an accepted step (Tsitouras 2011, as OrdinaryDiffEq's Tsit5
 * uses it): u(t_n + theta h) = u_n + h sum_i b_i(theta) k_i.  cnf_solve_path is cnf_solve_tsit5 plus its evaluation at the
 * caller's times.  The step sequence is not touched -- no clamping to the save times, no extra evaluations --, so u_out and the
 * statistics are those of cnf_solve_tsit5 on the same route.
 *
 * saveat_host: K >= 1 finite times (HOST), monotone (not necessarily strictly) along the direction of opts->t0 -> opts->t1 and
 * inside the closed span.  path_out_dev: DEVICE, [K][B][D] floats, slice k in the layout of u_out (all D rows: z, dlogp, and
 * in TrainMode E and n).  A time tau is served by the accepted step with t_n < tau <= t_n + h along the direction; the last
 * step, whose end the controller snaps onto t1, takes everything left.  tau == t0 stores u0 itself; tau at the end of its step
 * (theta >= 1 in float, or tau equal to the step's end) stores the accepted state itself, not the polynomial: a save time at
 * t1 reproduces u_out bit for bit.  Rejected attempts store nothing.
 *
 * Two routes; stats->launches tells which.  IN THE LAUNCH of the one-launch solve of small two-layer tanh networks (n_in <= 16,
 * at most 64 hidden units -- 16 with an identity second layer --, conditional models included, B <= 8192): the kernel evaluates
 * the interpolant from its registers; one launch, as cnf_solve_tsit5 reports for the same call.  It always runs one 16-column
 * tile per workgroup, so below 65 columns -- where cnf_solve_tsit5 runs the tiles as the waves of one workgroup -- u_out agrees
 * with cnf_solve_tsit5 to rounding, not bit for bit.  STREAMED, for every other network, mode and batch, for
 * opts->kernel = CNF_KERNEL_GENERIC, and when a wait of the one-launch solve runs out (cnf_solve_fallbacks counts it): one
 * attempt at a time on the per-stage kernels, the host looks at the state after each and enqueues the interpolation kernel
 * before the next attempt overwrites the Runge-Kutta buffers.
 *
 * Synchronous.  Inferences submitted on the handle are collected first.  Returns CNF_ERR_UNSUPPORTED under lock-step shards
 * (cnf_set_shard_reduce / cnf_set_shard_comm); CNF_ERR_BAD_ARG for NULL saveat_host / path_out_dev / u_out, K < 1 or save times
 * that are not finite, not monotone along the span or outside it -- all checked before the handle is looked at, so with a NULL
 * handle too; otherwise the returns of cnf_solve_tsit5. */
cnf_status cnf_solve_path(cnf_handle h, int mode, const float* u0, const float* eps, float* u_out, int B,
                          const cnf_solve_opts* opts, const float* saveat_host, int K, float* path_out_dev,
                          cnf_solve_stats* stats, void* stream);

/* The accepted steps of the last cnf_solve_path on this handle, on either route: returns their number and copies
 * min(number, cap) pairs into t_host (t_n) and h_host (signed h_n) (HOST; may be NULL).  -1: there is none (no such call yet,
 * it failed, or -- in-launch route -- it took more than 16384 accepted steps, which is what the launch files). */
int cnf_path_steps(cnf_handle h, float* t_host, float* h_host, int cap);

#endif /* CNFHIP_PATH_H */
