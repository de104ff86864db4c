// Which way a call goes through solve_core (cnf_abi.hip), as a value: what the call asks (SolveAsk), what the kernels' *_supported
// predicates answered for its network and batch (SolveCaps), and the route that follows (SolveRoute).  Plain C++ (no HIP, no
// handle), so that tests/support/solve_plan_test.cpp can hold the route to its rules on the CPU.  This function is the one source
// of DESIGN section 4.7's kernel table.
//
// The drivers, in the order solve_core tries them:
//   one launch   the whole solve in one kernel -- k_solve_wave, k_solve_bcast, k_trace3s<SOLVE>, k_solve3b / k_solve3jb, tried in
//                that order (the launchers may still answer "not this batch") -- under the process-wide lock; a launch that gives
//                up (a wait ran out) hands the call to one of the two host-driven drivers below
//   stepwise     one attempt at a time, the host reads the state after each: lock-step shards, the recorded solves the fused step
//                kernel cannot file, paths, tangent calls
//   streamed     launches kept a few attempts ahead of the last state the host has seen
#pragma once

struct SolveAsk {
    bool k_mfma;          // the resolved kernel is CNF_KERNEL_MFMA (else GENERIC)
    bool asked_generic;   // opts->kernel == CNF_KERNEL_GENERIC
    bool train;
    bool adaptive;
    bool dt_zero;         // opts->dt == 0: with `adaptive`, the automatic initial dt
    bool shards;          // a shard_reduce callback or a shard communicator is set
    bool no_persist;      // the fallback of a collected launch: no one-launch solve
    bool rec;             // a Recorder (gradient path) ...
    bool rec_wg;          //   ... that wants the whole gradient in the launch of the solve
    bool post_xs;         // a PostHook with the caller's data columns
    bool path, jvp;       // a PathHook / a tangent call
    bool conditional;     // n_cond > 0
    bool id2;             // a one-layer tanh network with its appended identity layer (nd_wave.id2)
};
// (a predicate that no route can ask about for this call may be left false: solve_core does not evaluate the two trace
// predicates where the auxiliary kernels cannot run, nor wave_grad_ok without rec_wg)
struct SolveCaps {
    bool mfma_ok;               // mfma_supported
    bool wave_solve_ok;         // wave_solve_supported
    bool wave_grad_ok;          // wave_grad_supported
    bool bcast_solve_ok;        // bcast_solve_supported
    bool bcast_store_is_zero;   // bcast_store_floats == 0: one tile per workgroup holds the batch
    bool trace_fused_ok;        // trace_fused_supported, TestMode
    bool trace_solve_ok;        // trace_solve_supported
};
enum SolvePartials { PARTIALS_GENERIC, PARTIALS_MFMA_GRID, PARTIALS_TRACE_GRID };     // whose blocks write the error partials
struct SolveRoute {
    bool hairer, lockstep;
    bool use_mfma;        // the fused step kernels (k_mfma / k_step3b) evaluate
    bool trace_on;        // the generic driver with an auxiliary MFMA kernel per stage (cnf_trace.hip)
    bool trace_fused;     //   ... with norms, controller and whole attempts inside its launches (k_trace3s)
    bool wave_ok, bcast_ok, tsolve_ok;      // one-launch kernels that take the call (besides use_mfma's k_solve3b)
    bool bcast_prepare;   // k_solve_bcast's images and tile store are wanted
    bool wg_refused;      // rec_wg, and the wave launch cannot be tried: handed back before anything runs
    bool one_launch;      // the one-launch driver is tried first
    bool stepwise;        // the host-driven driver: one attempt at a time (else streamed)
    SolvePartials partials;
};

inline SolveRoute solve_route(const SolveAsk& a, const SolveCaps& c) {
    SolveRoute r{};
    // (a path needs k_2 .. k_6 of every accepted step in the handle's buffers: where the fused step kernel would run, its solve
    // takes the per-stage generic kernel instead)
    const bool mfma_ok = a.k_mfma && c.mfma_ok;
    r.use_mfma = mfma_ok && !a.path;
    // Not for the recorded TrainMode solve of the gradient path: k_jvp_mfma does not file the stage states the pullback starts
    // from (k_mfma and the generic stage kernel do), so that solve runs the generic stage kernel
    r.trace_on = a.k_mfma && !mfma_ok && !(a.rec && a.train);
    // lock-step over shards only matters when the controller decides something
    r.lockstep = a.shards && a.adaptive;
    r.hairer = a.adaptive && a.dt_zero;
    // TestMode on k_trace3s: the trace launches write the error partials themselves (one pair per workgroup)
    r.trace_fused = r.trace_on && !r.lockstep && !a.rec && !a.path && c.trace_fused_ok;
    r.partials = r.trace_fused ? PARTIALS_TRACE_GRID : r.use_mfma ? PARTIALS_MFMA_GRID : PARTIALS_GENERIC;
    // k_solve_wave (a one-layer tanh network has no other MFMA kernel: AUTO resolves to GENERIC for it, and the wave kernels take
    // it through its appended identity layer unless GENERIC was asked for)
    const bool wave_k = a.k_mfma || (a.id2 && !a.asked_generic);
    r.wave_ok = wave_k && (!a.rec || (a.rec_wg && a.post_xs && c.wave_grad_ok)) && c.wave_solve_ok;
    r.wg_refused = a.rec_wg && !(r.wave_ok && !r.lockstep && !a.no_persist);
    // k_solve_bcast (the gradient's recorded forward too, where one tile per workgroup holds the batch)
    const bool bcast_rec = a.rec && !a.rec_wg && a.train && c.bcast_store_is_zero;
    r.bcast_ok = a.k_mfma && (!a.rec || bcast_rec) && !r.wave_ok && !a.path && c.bcast_solve_ok;
    r.bcast_prepare = r.bcast_ok && !r.lockstep && !a.no_persist;
    // k_trace3s<SOLVE>: the 32-128-128-32 network in TestMode
    r.tsolve_ok = r.trace_fused && !r.wave_ok && !r.bcast_ok && !r.use_mfma && !a.conditional && c.trace_solve_ok;
    // (a tangent call's one-launch solve is the wave kernel's: cnf_tangent.hip reads what that kernel leaves)
    r.one_launch = (r.use_mfma || r.wave_ok || r.bcast_ok || r.tsolve_ok) && !r.lockstep && !a.no_persist && (!a.jvp || r.wave_ok);
    // Lock-step: every shard must see the same global error norm before the next attempt is sized.  Recording: the host files
    // the state after every accepted step.  A path: the host enqueues the interpolation of an accepted step before the next
    // attempt overwrites k_2 .. k_6.  A tangent call: the host files the accepted steps for its replay.
    r.stepwise = r.lockstep || (a.rec && !r.use_mfma) || a.path || a.jvp;
    return r;
}
