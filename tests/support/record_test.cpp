// csrc/cnf_record.h against the table it replaced, on the CPU: from every state the library's calls can reach, every call-level
// event at batch sizes 1, 5 and 7, and after each one every query.
//
// The table is `Fields`: the ten loose fields cnf_ctx had, with -- per event -- the assignments cnf_abi.hip made to them at the
// commit before the record type (rec_valid, rec_mode, rec_B, rec_kernel, rec_eps, rec_kind, fs_B, fs_mode, grad_last_B,
// gy_last_B), and the conditions its five readers tested.  `Events` applies one event to either representation; the two must
// answer every query alike in every reachable state.  Then the facts a reader relies on, spelled out one by one.
#include "../../continuousnf.jl_amd/csrc/cnf_record.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static const float EPS_A[1] = {0.f}, EPS_B[1] = {0.f};
enum { TEST = 0, TRAIN = 1 };

// ---- the table: the parent's fields, assignments and conditions ------------------------------------------------------------------
struct Fields {
    bool rec_valid = false;
    int rec_mode = 0, rec_B = 0, rec_kernel = 0;
    const float* rec_eps = nullptr;
    int rec_kind = 0;                // 1: REC_INFERENCE, 2: REC_GENERATE
    int fs_B = 0, fs_mode = 0, grad_last_B = 0, gy_last_B = 0;

    void end_record() { rec_valid = false; fs_B = 0; }
    // transitions, under the names of CnfRecord
    void end() { end_record(); }
    void clear() { grad_last_B = 0; gy_last_B = 0; end_record(); }
    void backward_begins() { gy_last_B = 0; }
    void backward_done(int B, bool with_ys) { grad_last_B = B; if (with_ys) gy_last_B = B; }
    void pullback_failed() { rec_valid = false; }
    void sampling_pullback_done() { grad_last_B = 0; }
    void begin(CnfRecKind kind, int mode, int B, int kernel = 0, const float* eps = nullptr) {
        if (kind == REC_LOSS) { fs_B = B; fs_mode = mode; return; }
        if (kind == REC_GENERATE) { grad_last_B = 0; gy_last_B = 0; }
        rec_valid = true; rec_mode = mode; rec_B = B; rec_kernel = kernel; rec_eps = eps;
        rec_kind = kind == REC_INFERENCE ? 1 : 2;
    }
    // queries, as cnf_inference_pullback, cnf_generate_pullback, cnf_base_logpdf_pullback, cnf_grad_x and cnf_grad_ys tested them
    bool pullable(CnfRecKind kind, int B) const { return rec_valid && rec_kind == (kind == REC_INFERENCE ? 1 : 2) && B == rec_B; }
    int mode() const { return rec_valid ? rec_mode : fs_mode; }
    int kernel() const { return rec_kernel; }
    const float* eps() const { return rec_eps; }
    CnfRecord::Source base_source(int B) const {
        if (rec_valid && B == rec_B && B >= 1) return rec_kind == 2 ? CnfRecord::SRC_Z0 : CnfRecord::SRC_FINAL_STATE;
        if (fs_B >= 1 && B == fs_B) return CnfRecord::SRC_FINAL_STATE;
        return CnfRecord::SRC_NONE;
    }
    bool grad_x_ok(int B) const { return !(B < 1 || B != grad_last_B); }
    bool grad_ys_ok(int B) const { return !(B < 1 || B != gy_last_B); }

    typedef std::tuple<bool, int, int, int, const float*, int, int, int, int> Key;
    // (what can still be observed: a dead record's fields and a dead fs_mode cannot)
    Key key() const {
        return rec_valid ? Key(true, rec_kind, rec_mode, rec_B, rec_eps, rec_kernel, 0, grad_last_B, gy_last_B)
                         : Key(false, 0, fs_B ? fs_mode : 0, fs_B, nullptr, 0, 0, grad_last_B, gy_last_B);
    }
};

// ---- the events: what one call on the handle does to the record, in the order the call does it ------------------------------------
struct Event { int what, B, mode; bool ys; };
enum { SOLVE_OR_UPLOAD, ARENA_GROWS_OR_MANY, WAVE_LOSS_GRAD, LOSS_GRAD, LOSS_GRAD_FAILS, INFERENCE_RECORD, GENERATE_RECORD,
       INFERENCE_PULLBACK, INFERENCE_PULLBACK_FAILS, GENERATE_PULLBACK, GENERATE_PULLBACK_FAILS, N_EVENTS };

template <class R>
static void apply(R& r, const Event& e) {
    const float* eps = e.mode == TRAIN ? (e.B == 5 ? EPS_A : EPS_B) : nullptr;
    const int kernel = e.B == 7 ? 2 : 0;
    switch (e.what) {
        case SOLVE_OR_UPLOAD: r.end(); break;                       // any solve; cnf_set_params*, cnf_set_cond, cnf_set_basedist
        case ARENA_GROWS_OR_MANY: r.clear(); break;                 // ensure_grad_capacity grew the arena; cnf_loss_grad_many
        case WAVE_LOSS_GRAD: r.backward_begins(); r.end(); r.backward_done(e.B, false); break;      // solve and gradient in one launch
        case LOSS_GRAD:                                              // cnf_loss_grad / cnf_loss_grad_test, the recorded route
            r.end(); r.backward_begins(); r.backward_done(e.B, false);
            if (e.ys) r.backward_done(e.B, true);
            r.begin(REC_LOSS, e.mode, e.B);
            break;
        case LOSS_GRAD_FAILS: r.end(); r.backward_begins(); break;  // ... whose backward pass returned an error
        case INFERENCE_RECORD: r.end(); r.begin(REC_INFERENCE, e.mode, e.B, kernel, eps); break;
        case GENERATE_RECORD: r.end(); r.begin(REC_GENERATE, e.mode, e.B, kernel, eps); break;
        case INFERENCE_PULLBACK: case INFERENCE_PULLBACK_FAILS: case GENERATE_PULLBACK: case GENERATE_PULLBACK_FAILS: {
            const bool gen = e.what >= GENERATE_PULLBACK;
            if (!r.pullable(gen ? REC_GENERATE : REC_INFERENCE, e.B)) break;       // refused: nothing changes
            r.backward_begins();
            if (e.what == INFERENCE_PULLBACK_FAILS || e.what == GENERATE_PULLBACK_FAILS) { r.pullback_failed(); break; }
            r.backward_done(e.B, e.ys);
            if (gen) r.sampling_pullback_done();
            break;
        }
    }
}

static const int BS[] = {-3, 0, 1, 5, 7};
static int n_checks = 0;
static void same_answers(const CnfRecord& r, const Fields& f) {
    for (int B : BS) {
        for (CnfRecKind k : {REC_INFERENCE, REC_GENERATE}) {
            CHECK(r.pullable(k, B) == f.pullable(k, B));
            if (r.pullable(k, B)) CHECK(r.mode() == f.mode() && r.kernel() == f.kernel() && r.eps() == f.eps());
        }
        CHECK(!r.pullable(REC_NONE, B) && !r.pullable(REC_LOSS, B));
        CHECK(r.base_source(B) == f.base_source(B));
        if (r.base_source(B) == CnfRecord::SRC_FINAL_STATE) CHECK(r.mode() == f.mode());
        CHECK(r.grad_x_ok(B) == f.grad_x_ok(B));
        CHECK(r.grad_ys_ok(B) == f.grad_ys_ok(B));
        n_checks += 8;
    }
}

int main() {
    std::vector<Event> events;
    for (int what = 0; what < N_EVENTS; ++what)
        for (int B : {1, 5, 7})
            for (int mode : {TEST, TRAIN})
                for (bool ys : {false, true}) events.push_back(Event{what, B, mode, ys});

    // ---- every event from every reachable state ----
    struct State { CnfRecord r; Fields f; };
    std::vector<State> todo(1);
    std::set<Fields::Key> seen{todo[0].f.key()};
    same_answers(todo[0].r, todo[0].f);
    size_t n_states = 0;
    while (!todo.empty()) {
        const State s = todo.back();
        todo.pop_back();
        ++n_states;
        for (const Event& e : events) {
            State t = s;
            apply(t.r, e);
            apply(t.f, e);
            same_answers(t.r, t.f);
            if (seen.insert(t.f.key()).second) todo.push_back(t);
        }
    }
    CHECK(n_states > 50);          // (19 records, none included, times what a backward pass can have left)

    // ---- the facts, one by one ----
    const Event loss5{LOSS_GRAD, 5, TRAIN, true}, inf5{INFERENCE_RECORD, 5, TRAIN, false}, gen5{GENERATE_RECORD, 5, TEST, false};
    const Event solve{SOLVE_OR_UPLOAD, 0, 0, false}, grows{ARENA_GROWS_OR_MANY, 0, 0, false};
    {   // a solve ends the record but not lam_B (nor gy_B)
        CnfRecord r;
        apply(r, loss5);
        CHECK(r.base_source(5) == CnfRecord::SRC_FINAL_STATE && r.grad_x_ok(5) && r.grad_ys_ok(5));
        apply(r, solve);
        CHECK(r.base_source(5) == CnfRecord::SRC_NONE && r.grad_x_ok(5) && r.grad_ys_ok(5));
    }
    {   // LOSS serves the base pullback and neither of the other two pullbacks
        CnfRecord r;
        apply(r, loss5);
        CHECK(r.base_source(5) == CnfRecord::SRC_FINAL_STATE && r.mode() == TRAIN && r.base_source(7) == CnfRecord::SRC_NONE);
        CHECK(!r.pullable(REC_INFERENCE, 5) && !r.pullable(REC_GENERATE, 5));
    }
    {   // a refused pullback (wrong B or wrong kind) changes nothing
        CnfRecord r;
        apply(r, loss5);
        apply(r, inf5);
        for (const Event& e : {Event{INFERENCE_PULLBACK, 7, 0, false}, Event{GENERATE_PULLBACK, 5, 0, false}, Event{GENERATE_PULLBACK_FAILS, 5, 0, false},
                               Event{INFERENCE_PULLBACK_FAILS, 1, 0, false}}) {
            apply(r, e);
            CHECK(r.pullable(REC_INFERENCE, 5) && r.eps() == EPS_A && r.mode() == TRAIN && r.grad_x_ok(5) && r.grad_ys_ok(5));
            CHECK(r.base_source(5) == CnfRecord::SRC_FINAL_STATE);
        }
    }
    {   // a failed pullback ends the record only (it had started: d / d ys of the earlier pass is gone, d / d u(t0) is not)
        CnfRecord r;
        apply(r, loss5);
        apply(r, inf5);
        apply(r, Event{INFERENCE_PULLBACK_FAILS, 5, 0, false});
        CHECK(!r.pullable(REC_INFERENCE, 5) && r.base_source(5) == CnfRecord::SRC_NONE && r.grad_x_ok(5) && !r.grad_ys_ok(5));
    }
    {   // arena growth clears everything
        CnfRecord r;
        apply(r, inf5);
        apply(r, Event{INFERENCE_PULLBACK, 5, 0, true});
        CHECK(r.pullable(REC_INFERENCE, 5) && r.grad_x_ok(5) && r.grad_ys_ok(5));
        apply(r, grows);
        CHECK(!r.pullable(REC_INFERENCE, 5) && r.base_source(5) == CnfRecord::SRC_NONE && !r.grad_x_ok(5) && !r.grad_ys_ok(5));
    }
    {   // a sampling record and a sampling pullback zero lam_B; the record also zeroes gy_B, the pullback leaves its own
        CnfRecord r;
        apply(r, loss5);
        apply(r, gen5);
        CHECK(r.pullable(REC_GENERATE, 5) && !r.pullable(REC_INFERENCE, 5) && r.base_source(5) == CnfRecord::SRC_Z0);
        CHECK(!r.grad_x_ok(5) && !r.grad_ys_ok(5));
        apply(r, Event{GENERATE_PULLBACK, 5, 0, true});
        CHECK(r.pullable(REC_GENERATE, 5) && !r.grad_x_ok(5) && r.grad_ys_ok(5));
    }
    std::printf("ok: %zu states, %zu events each, %d answers compared\n", n_states, events.size(), n_checks);
    return 0;
}
