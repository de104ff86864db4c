// What a call on a handle leaves behind for the calls that may follow it (cnf_abi.hip), as one value with named transitions.
//
// Three pieces, each ended by its own events:
//   the record   the last solve's steps are in the trajectory store and last_hs, its final state in g_US[1] (a sampling
//                record also keeps its base draw in d_gz0).  INFERENCE (cnf_inference_record) and GENERATE
//                (cnf_generate_record) can be pulled back, each by its own pullback only; LOSS (cnf_loss_grad /
//                cnf_loss_grad_test on the recorded route) is the final state alone, for cnf_base_logpdf_pullback.  Any solve,
//                an upload of parameters or conditioning and a change of the base distribution end it; so does a pullback
//                that failed half way.
//   lam_B        g_lam holds d / d u(t0) of a gradient over a batch of that size (cnf_grad_x); 0: none.  Set by every
//                backward pass; a sampling record and a sampling pullback zero it (their g_lam is d / d u(t_start) of a
//                SAMPLING solve: cnf_grad_x is not defined for it).  The end of the record leaves it alone.
//   gy_B         d_gy holds d / d ys of a batch of that size (cnf_grad_ys); 0: none, or cnf_set_grad_ys was off during the
//                last backward pass.  Cleared when a backward pass starts, set when one that accumulated it finishes.
// All three go when the gradient arena is reallocated and when cnf_loss_grad_many runs.
//
// Plain C++ (no HIP), like cnf_buf.h: tests/support/record_test.cpp walks every state.
#pragma once

enum CnfRecKind { REC_NONE = 0, REC_LOSS, REC_INFERENCE, REC_GENERATE };

class CnfRecord {
    CnfRecKind kind_ = REC_NONE;
    int mode_ = 0, B_ = 0, kernel_ = 0;
    const float* eps_ = nullptr;  // TrainMode records: the caller's probes, read again by the pullback
    int lam_B_ = 0, gy_B_ = 0;

public:
    // ---- transitions ----
    void begin(CnfRecKind kind, int mode, int B, int kernel = 0, const float* eps = nullptr) {
        kind_ = kind; mode_ = mode; B_ = B; kernel_ = kernel; eps_ = eps;
        if (kind == REC_GENERATE) lam_B_ = gy_B_ = 0;
    }
    void end() { kind_ = REC_NONE; }
    void pullback_failed() { kind_ = REC_NONE; }           // (the stores may be half overwritten)
    void clear() { kind_ = REC_NONE; lam_B_ = gy_B_ = 0; }
    void backward_begins() { gy_B_ = 0; }
    void backward_done(int B, bool with_ys) { lam_B_ = B; if (with_ys) gy_B_ = B; }
    void sampling_pullback_done() { lam_B_ = 0; }

    // ---- queries ----
    bool pullable(CnfRecKind kind, int B) const { return kind_ == kind && kind != REC_NONE && kind != REC_LOSS && B == B_; }
    int mode() const { return mode_; }                     // of the record (meaningful while there is one)
    int kernel() const { return kernel_; }
    const float* eps() const { return eps_; }
    // where cnf_base_logpdf_pullback reads the base's argument of a batch of B: SRC_Z0 = d_gz0, rows of n_in; SRC_FINAL_STATE =
    // g_US[1], rows of rows_of(mode())
    enum Source { SRC_NONE = 0, SRC_FINAL_STATE, SRC_Z0 };
    Source base_source(int B) const {
        if (kind_ == REC_NONE || B < 1 || B != B_) return SRC_NONE;
        return kind_ == REC_GENERATE ? SRC_Z0 : SRC_FINAL_STATE;
    }
    bool grad_x_ok(int B) const { return B >= 1 && B == lam_B_; }
    bool grad_ys_ok(int B) const { return B >= 1 && B == gy_B_; }
};
