// The process-wide environment switches of libcnfhip.so, as one table: the kernels are picked by shape, and these select THE OTHER
// kernel or route for A/B measurements and for the parity legs of test_ab_switches_take_the_other_kernels_and_stay_parity_green.
// Plain C++ (no HIP, no handle), so that tests/support/switch_test.cpp can hold the parse rules to their edges on the CPU;
// tests/test_switches.py holds DESIGN section 4.7's sentence and the table of tools/README.md to the names below.
//
// cnf_switch<SW_x>() reads its variable once per process: the first use parses it, every later use (from any translation unit of
// the library, from any thread) returns that value.  Nothing else in csrc/ may call getenv("CNF_...").  A condition over several
// switches (wave_off: CNF_PERSISTENT off or CNF_WAVE off) short-circuits, so a later operand may be read at a later call than
// the first: set the variables before the library's first call, as a value read once per process requires anyway.
#pragma once
#include <cstdlib>

// How a variable's text becomes the value cnf_switch returns.  Only the first character counts for the three flag kinds.
enum SwitchKind {
    SWK_OFF_AT_0,     // 1; 0 when the first character is '0'          (unset, "", "1", "x": 1; "0", "01": 0)
    SWK_ON_AT_1,      // 0; 1 when the first character is '1'          (unset, "", "0", "01", "x": 0; "1": 1)
    SWK_ON_IF_SET,    // 0; 1 when the variable exists, WHATEVER it says ("", "0", "1", "x": 1 -- so NAME=0 means on)
    SWK_POS_INT,      // atoi when that is positive, else the default
    SWK_INT_ABOVE_4,  // atoi when that is above 4, else the default
    SWK_ANY_INT,      // atoi as it stands (unset: the default); the range is checked where the value is used
    SWK_TRISTATE,     // unset: the default (-1); first character '0': 0; anything else, "" included: 1
};

// X(name, kind, default, meaning): the variable is CNF_<name>, the index SW_<name>
#define CNF_SWITCH_TABLE(X) \
    X(PERSISTENT,        SWK_OFF_AT_0,    1,          "0: no one-launch solve at all (k_solve3b / k_solve3jb, k_solve_wave, k_solve_bcast, k_trace3s<SOLVE>): step launches from the start") \
    X(WAVE,              SWK_OFF_AT_0,    1,          "0: small two-layer networks on k_mfma behind the streamed driver instead of k_solve_wave") \
    X(WAVE_GRAD,         SWK_OFF_AT_0,    1,          "0: gradients of those networks on the streamed path (recorded solve, pullback launches, contraction) instead of k_solve_wave<GRAD>") \
    X(WAVE_RICH,         SWK_OFF_AT_0,    1,          "0: k_solve_wave<GRAD> recomputes the forward half of every stage instead of reading the rich store the forward pass filed") \
    X(WAVE_WG,           SWK_OFF_AT_0,    1,          "0: at most four tiles as one workgroup PER wave (meeting through memory words) instead of the waves of one workgroup") \
    X(WAVE_XWG_MIN,      SWK_INT_ABOVE_4, 513,        "n: k_solve_wave takes its four-tile workgroups from n tiles on (values <= 4 mean the default, 513: what 512 meeting words force)") \
    X(BCAST,             SWK_OFF_AT_0,    1,          "0: config 5's network on k_mfma instead of k_solve_bcast") \
    X(BCAST_FORCE_MULTI, SWK_ON_AT_1,     0,          "1: k_solve_bcast's several-tiles-per-workgroup form even when every tile has a CU of its own") \
    X(TRACE_SOLVE,       SWK_OFF_AT_0,    1,          "0: TestMode of the headline network as step launches of k_trace3s<STEP> instead of k_trace3s<SOLVE>") \
    X(TRACE_FP32,        SWK_ON_AT_1,     0,          "1: k_trace3 (fp32 MFMA, one evaluation per launch) instead of k_trace3s") \
    X(TRACE_UNFUSED,     SWK_ON_AT_1,     0,          "1: k_trace3s one evaluation per launch instead of one step attempt per launch") \
    X(TRACE_GENERIC,     SWK_ON_AT_1,     0,          "1: k_trace_mfma instead of k_trace3s / k_trace3") \
    X(SOLVE_WAIT_US,     SWK_POS_INT,     2000,       "n: microseconds per tile a workgroup carries that a wait inside a one-launch solve lasts before the call falls back (per handle: cnf_set_solve_wait)") \
    X(SOLVE_POLL_LIMIT,  SWK_POS_INT,     0x7fffffff, "n: polls such a wait makes before it gives up (default: the time bound decides); 1 forces the fallback") \
    X(STEP_FP32,         SWK_ON_AT_1,     0,          "1: the fp32-MFMA kernels k_step3 / k_step3j (and no k_solve3b / k_solve3jb) instead of the split-bf16 ones k_step3b / k_step3jb") \
    X(STEP_V1,           SWK_ON_AT_1,     0,          "1: the headline shape on the first-generation step kernel k_mfma instead of the k_step3* kernels") \
    X(ADJ_GENERIC,       SWK_ON_AT_1,     0,          "1: k_adj_mfma instead of k_adj3") \
    X(ADJ3B,             SWK_OFF_AT_0,    1,          "0: k_adj3 instead of k_adj3b") \
    X(ADJ_SPLIT,         SWK_TRISTATE,    -1,         "0 | anything else: never | always the two-launch pullback of k_adj_mfma (unset: by shape); the initial value of cnf_set_grad_split") \
    X(GRAD_FSTEPS,       SWK_POS_INT,     0,          "n: contract the weight gradient after every n steps where that is fewer than the handle's own count (default 0: the handle's)") \
    X(WGRAD_VALU,        SWK_ON_IF_SET,   0,          "set (CNF_WGRAD_VALU=0 too): the VALU weight-gradient contraction k_wgrad instead of the split-bf16 MFMA one") \
    X(WGRAD_FP32,        SWK_ON_IF_SET,   0,          "set (CNF_WGRAD_FP32=0 too): the fp32-MFMA contraction k_wgrad_mfma instead of the split-bf16 MFMA one") \
    X(WGRAD_LDS,         SWK_ON_IF_SET,   0,          "set (CNF_WGRAD_LDS=0 too): k_wgrad_mfma_b (workgroups, LDS images) instead of k_wgrad_wave (one wave per tile and K-split)") \
    X(WGRAD_KS,          SWK_ANY_INT,     0,          "n: force the K-splits of the contraction; grad_ksplit ignores a value outside 1..GRAD_MAX_KSPLIT")

enum CnfSwitch {
#define X(name, kind, dflt, meaning) SW_##name,
    CNF_SWITCH_TABLE(X)
#undef X
    SW_COUNT
};

// (hidden: one copy of the table and of each value in the library, and none of it among its exported symbols)
#pragma GCC visibility push(hidden)
struct SwitchRow { const char* env; SwitchKind kind; int dflt; const char* meaning; };
inline constexpr SwitchRow CNF_SWITCHES[SW_COUNT] = {
#define X(name, kind, dflt, meaning) {"CNF_" #name, kind, dflt, meaning},
    CNF_SWITCH_TABLE(X)
#undef X
};

// the value of a switch whose variable reads `e` (nullptr: unset)
inline int cnf_switch_parse(const SwitchRow& r, const char* e) {
    switch (r.kind) {
        case SWK_OFF_AT_0: return !(e && e[0] == '0');
        case SWK_ON_AT_1: return e && e[0] == '1';
        case SWK_ON_IF_SET: return e != nullptr;
        case SWK_POS_INT: { const int v = e ? atoi(e) : 0; return v > 0 ? v : r.dflt; }
        case SWK_INT_ABOVE_4: { const int v = e ? atoi(e) : 0; return v > 4 ? v : r.dflt; }
        case SWK_ANY_INT: return e ? atoi(e) : r.dflt;
        case SWK_TRISTATE: return e ? (e[0] == '0' ? 0 : 1) : r.dflt;
    }
    return r.dflt;
}
template <CnfSwitch S> inline int cnf_switch() {
    static const int v = cnf_switch_parse(CNF_SWITCHES[S], getenv(CNF_SWITCHES[S].env));
    return v;
}
#pragma GCC visibility pop
