// The route of a solve (continuousnf.jl_amd/csrc/cnf_solve_plan.h) on the CPU: every combination of what a call can ask and of
// what the kernels' predicates can answer is held to the rules the drivers in cnf_abi.hip rely on, and the routes of DESIGN
// section 4.7's kernel table are asserted by name.
#include "cnf_solve_plan.h"
#include <cstdio>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails <= 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const int ASK_BITS = 14, CAP_BITS = 7;
static SolveAsk ask_of(unsigned m) {
    SolveAsk a{};
    a.k_mfma = m & 1; a.asked_generic = m & 2; a.train = m & 4; a.adaptive = m & 8; a.dt_zero = m & 16; a.shards = m & 32;
    a.no_persist = m & 64; a.rec = m & 128; a.rec_wg = m & 256; a.post_xs = m & 512; a.path = m & 1024; a.jvp = m & 2048;
    a.conditional = m & 4096; a.id2 = m & 8192;
    return a;
}
static SolveCaps caps_of(unsigned m) {
    SolveCaps c{};
    c.mfma_ok = m & 1; c.wave_solve_ok = m & 2; c.wave_grad_ok = m & 4; c.bcast_solve_ok = m & 8; c.bcast_store_is_zero = m & 16;
    c.trace_fused_ok = m & 32; c.trace_solve_ok = m & 64;
    return c;
}
// what a caller can ask at all: a kernel asked for as GENERIC resolves to GENERIC, the in-launch gradient is a Recorder's, and at
// most one of the three hooks rides on a call
static bool possible(const SolveAsk& a) {
    return !(a.asked_generic && a.k_mfma) && !(a.rec_wg && !a.rec) && (int)a.rec + (int)a.path + (int)a.jvp <= 1;
}

// the named rows: a plain inference (data columns at hand, adaptive, automatic initial dt) unless the row says otherwise
static SolveAsk inference(bool k_mfma, bool train) {
    SolveAsk a{};
    a.k_mfma = k_mfma; a.asked_generic = !k_mfma; a.train = train; a.adaptive = true; a.dt_zero = true; a.post_xs = true;
    return a;
}
static void named_rows() {
    SolveCaps headline{}; headline.mfma_ok = true;                                      // 32-128-128-32, TrainMode: k_solve3b
    SolveCaps small{}; small.mfma_ok = small.wave_solve_ok = small.wave_grad_ok = true;  // 2-6-2: the wave kernels
    SolveCaps cfg5{}; cfg5.mfma_ok = cfg5.bcast_solve_ok = cfg5.bcast_store_is_zero = true;   // 128-384-128 at one tile per CU
    SolveCaps test3{}; test3.trace_fused_ok = test3.trace_solve_ok = true;              // 32-128-128-32, TestMode: k_trace3s
    SolveCaps deep{};                                                                   // a deep network: the auxiliary kernels only
    SolveRoute r = solve_route(inference(true, true), headline);
    CHECK(r.one_launch && r.use_mfma && !r.wave_ok && !r.bcast_ok && !r.tsolve_ok && !r.stepwise && r.partials == PARTIALS_MFMA_GRID, "headline");
    r = solve_route(inference(true, true), small);
    CHECK(r.one_launch && r.wave_ok && !r.bcast_ok && !r.stepwise, "wave");
    r = solve_route(inference(true, true), cfg5);
    CHECK(r.one_launch && r.bcast_ok && r.bcast_prepare && !r.wave_ok, "bcast");
    r = solve_route(inference(true, false), test3);
    CHECK(r.one_launch && r.tsolve_ok && r.trace_on && r.trace_fused && !r.use_mfma && r.partials == PARTIALS_TRACE_GRID, "k_trace3s<SOLVE>");
    SolveCaps test3_streamed = test3; test3_streamed.trace_solve_ok = false;            // (CNF_PERSISTENT=0)
    r = solve_route(inference(true, false), test3_streamed);
    CHECK(!r.one_launch && !r.stepwise && r.trace_fused, "streamed fused trace");
    r = solve_route(inference(true, false), deep);
    CHECK(!r.one_launch && !r.stepwise && r.trace_on && !r.trace_fused && r.partials == PARTIALS_GENERIC, "streamed auxiliary trace kernel");
    r = solve_route(inference(false, true), small);
    CHECK(!r.one_launch && !r.stepwise && !r.use_mfma && !r.trace_on && !r.wave_ok, "streamed generic");
    SolveAsk a = inference(true, true); a.shards = true;
    r = solve_route(a, headline);
    CHECK(!r.one_launch && r.stepwise && r.lockstep && r.use_mfma, "lock-step");
    a.adaptive = false; a.dt_zero = false;
    r = solve_route(a, headline);
    CHECK(r.one_launch && !r.lockstep, "fixed dt never runs lock-step");
    a = inference(true, true); a.rec = true;
    r = solve_route(a, headline);
    CHECK(r.one_launch && r.use_mfma && !r.stepwise, "recorded headline solve");
    r = solve_route(a, cfg5);
    CHECK(r.one_launch && r.bcast_ok, "recorded bcast solve");
    a.no_persist = true;
    r = solve_route(a, headline);
    CHECK(!r.one_launch && !r.stepwise, "streamed recording on the fused step kernel");
    a = inference(false, false); a.rec = true; a.post_xs = false;
    r = solve_route(a, small);
    CHECK(!r.one_launch && r.stepwise && !r.wg_refused, "TestMode recorded solve");
    a = inference(true, true); a.rec = a.rec_wg = true;
    r = solve_route(a, small);
    CHECK(r.one_launch && r.wave_ok && !r.wg_refused, "in-launch gradient");
    r = solve_route(a, headline);
    CHECK(r.wg_refused, "no in-launch gradient on the headline network");
    a = inference(true, true); a.post_xs = false; a.path = true;
    r = solve_route(a, small);
    CHECK(r.one_launch && r.wave_ok && !r.use_mfma && r.stepwise, "path in the wave launch");
    r = solve_route(a, headline);
    CHECK(!r.one_launch && r.stepwise && !r.use_mfma, "path one attempt at a time");
    a = inference(true, true); a.jvp = true;
    r = solve_route(a, small);
    CHECK(r.one_launch && r.wave_ok && r.stepwise, "tangent call");
    a = inference(false, true); a.asked_generic = false; a.id2 = true;                  // a one-layer network under AUTO
    r = solve_route(a, small);
    CHECK(r.one_launch && r.wave_ok && !r.use_mfma, "one-layer network through its appended identity");
}

int main() {
    long seen = 0;
    for (unsigned am = 0; am < (1u << ASK_BITS); ++am) {
        const SolveAsk a = ask_of(am);
        if (!possible(a)) continue;
        for (unsigned cm = 0; cm < (1u << CAP_BITS); ++cm) {
            const SolveRoute r = solve_route(a, caps_of(cm));
            ++seen;
            // exactly one first driver: the one-launch attempt, else stepwise, else streamed -- and the host-driven driver behind
            // a one-launch attempt that gives up is the same one of the two
            const int first = r.one_launch ? 0 : r.stepwise ? 1 : 2;
            CHECK((first == 0) + (first == 1) + (first == 2) == 1, "ask %x caps %x", am, cm);
            CHECK(!(r.one_launch && (r.lockstep || a.no_persist)), "ask %x caps %x: one launch under lock-step / no_persist", am, cm);
            CHECK(!(r.one_launch && a.jvp) || r.wave_ok, "ask %x caps %x: a tangent call's launch is not the wave kernel's", am, cm);
            CHECK(!(a.path && r.use_mfma), "ask %x caps %x: a path on the fused step kernel", am, cm);
            CHECK(!a.rec_wg || r.wg_refused || (r.one_launch && r.wave_ok), "ask %x caps %x: rec_wg reaches a host-driven driver", am, cm);
            CHECK(!r.wg_refused || a.rec_wg, "ask %x caps %x", am, cm);
            CHECK(!r.trace_fused || (r.trace_on && !r.lockstep && !a.rec && !a.path), "ask %x caps %x: trace_fused", am, cm);
            CHECK(!r.tsolve_ok || (r.trace_fused && !r.wave_ok && !r.bcast_ok && !r.use_mfma && !a.conditional), "ask %x caps %x: tsolve_ok", am, cm);
            CHECK((int)r.wave_ok + (int)r.bcast_ok + (int)r.tsolve_ok <= 1, "ask %x caps %x: two one-launch kernels", am, cm);
            // and what the drivers read besides
            CHECK(!(r.trace_on && r.use_mfma), "ask %x caps %x: both evaluators", am, cm);
            CHECK(!r.bcast_prepare || r.bcast_ok, "ask %x caps %x", am, cm);
            CHECK((r.partials == PARTIALS_TRACE_GRID) == r.trace_fused && (r.partials == PARTIALS_MFMA_GRID) == (r.use_mfma && !r.trace_fused),
                  "ask %x caps %x: partials", am, cm);
            CHECK(r.hairer == (a.adaptive && a.dt_zero) && r.lockstep == (a.shards && a.adaptive), "ask %x caps %x", am, cm);
            CHECK(!(a.rec && !r.wg_refused && !r.one_launch && !r.stepwise) || r.use_mfma, "ask %x caps %x: a streamed recording off the fused step kernel", am, cm);
        }
    }
    named_rows();
    std::printf("%ld routes\n%s\n", seen, fails ? "failed" : "ok");
    return fails ? 1 : 0;
}
