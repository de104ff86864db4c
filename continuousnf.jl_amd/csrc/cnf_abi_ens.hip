// C ABI of libcnfhip.so, the ensemble family (include/cnfhip_ensemble*.h) and the single-model path-VJP calls that are its
// M = 1 case (include/cnfhip_path_vjp.h).
#include "cnf_abi_int.h"
using namespace cnfabi;

// ---------------------------------------------------------------------------------------
// Ensembles (include/cnfhip_ensemble.h): M independent models of the handle's architecture -- folds, replicas, seeds -- whose
// losses and gradients come out of ONE launch of k_solve_wave<.., ENS> (cnf_wave.hip) and one launch of the partial sums.
// Nothing of the handle's own model is touched: parameters, data and probes are the caller's arrays, every store is a buffer
// of the ensemble's own.
// ---------------------------------------------------------------------------------------
// the handles that take an ensemble call at all (both capacity calls answer 0 for the others)
static bool ens_handle_ok(cnf_handle h, int mode) {
    if (!h || (mode != CNF_MODE_TEST && mode != CNF_MODE_TRAIN)) return false;
    return !(h->nd.n_cond > 0 || h->bd.kind || h->grad_ys || h->shard_reduce || h->shard_comm || h->no_persist);
}
// cw: of that per-sample-cotangent form (cnf_inference_vjp_many, cnf_generate_vjp_many), whose kernels have their own register budget
static int ens_grad_capacity(cnf_handle h, int mode, int B, WaveCot cw) {
    if (B < 1 || !ens_handle_ok(h, mode)) return 0;
    if (hipSetDevice(h->device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int cap = wave_ens_capacity(h->nd_wave, mode == CNF_MODE_TRAIN, B, cw);
    // ... and no more members than keep 64 step slots each within the trajectory budget of one model's call
    size_t fit = 0;
    traj_step_slots(wave_grad_traj_floats(h->nd_wave, B), &fit);
    if ((size_t)cap > fit) cap = (int)fit;
    return cap;
}
extern "C" int cnf_ensemble_capacity(cnf_handle h, int mode, int B) { return ens_grad_capacity(h, mode, B, WC_LOSS); }
extern "C" int cnf_ensemble_vjp_capacity(cnf_handle h, int mode, int B) { return ens_grad_capacity(h, mode, B, WC_INFERENCE); }
extern "C" int cnf_ensemble_generate_vjp_capacity(cnf_handle h, int mode, int B) { return ens_grad_capacity(h, mode, B, WC_SAMPLING); }

// ---- What cnf_loss_grad_many and ens_eval (cnf_inference_many, cnf_generate_many: further down) share, each step once: the
// checks, the growth of the stores, the launch preamble and the read-back.  EnsCall is one call's arguments and, from ens_begin
// to ens_finish, its lock and the common part of its Solve3Args. ----
namespace {
struct EnsCall {
    bool grad, gen;                // an ensemble gradient call | sampling (times are the members' START times) or inference
    int mode, M, B, trace_cap;
    const cnf_solve_opts* opts;
    const float* times;            // the members' own end (gen: start) times on the host, or null: opts' for all
    hipStream_t st;
    std::unique_lock<std::mutex> lock;     // g_persist_mu
    bool hairer = false;
    Solve3Args sv{};
    WaveCot cot = WC_LOSS;         // grad: the built-in loss (cnf_loss_grad_many) or per-sample cotangents (the two vjp calls)
    // heterogeneous members: what cnf_ensemble_set_members left for this call (ens_take_members); M = 0: nothing
    int het_M = 0;
    std::vector<int> counts;
    std::vector<float> lams, tols;
    const int* d_counts = nullptr;         // ... on the device, from ens_begin on (null: not given)
    const float *d_lams = nullptr, *d_tols = nullptr;
    bool path_many = false;        // one of the four calls of include/cnfhip_ensemble_path.h: their own capacities
    // the members' own bases: what cnf_ensemble_set_bases prepared for this call (ens_take_members); M = 0: none
    int base_M = 0, base_kind = 0;
    const float* d_bases = nullptr;        // [M][WV_ENS_BASE_FLOATS], device
};
}  // namespace
// The one-shot state changes hands: whatever becomes of the call, no later call is steered by these arrays.
static void ens_take_members(cnf_handle h, EnsCall& c) {
    if (!h) return;
    c.het_M = h->het_M; h->het_M = 0;
    c.counts.swap(h->het_counts); c.lams.swap(h->het_lams); c.tols.swap(h->het_tols);
    h->het_counts.clear(); h->het_lams.clear(); h->het_tols.clear();
    // ... and the bases: the pending buffer becomes the last call's; whatever an earlier call left for the base pullback is gone
    c.base_M = h->base_M; c.base_kind = h->base_kind; h->base_M = 0; h->lbase_M = 0;
    if (c.base_M > 0) { h->ens_bases_pend.swap(h->ens_bases_last); c.d_bases = h->ens_bases_last; }
}
constexpr size_t ENS_ST_F = (sizeof(StepState) + 3) / 4;     // floats of one member's final state in ens_fin / ens_hfin ...
static size_t ens_fin_floats(int M) { return (size_t)M * (ENS_ST_F + 5); }      // ... and of all M, their five loss sums behind them

static cnf_status ens_check(cnf_handle h, const EnsCall& c, bool null_ptr, const char* b_msg, const char* capacity_fn) {
    // (the arguments first, the handle last: what is wrong with a call is said before anything asks for a device)
    if (c.mode != CNF_MODE_TEST && c.mode != CNF_MODE_TRAIN) return fail(h, CNF_ERR_BAD_ARG, "unknown mode");
    if (null_ptr) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (c.M < 1) return fail(h, CNF_ERR_BAD_SHAPE, "an ensemble has at least one member");
    if (c.B < 1) return fail(h, CNF_ERR_BAD_SHAPE, b_msg);
    if (c.trace_cap < 0) return fail(h, CNF_ERR_BAD_ARG, "trace_cap must be >= 0");
    if (!h) return CNF_ERR_BAD_ARG;
    cnf_status s = check_solve_opts(h, c.opts);
    if (s != CNF_OK) return s;
    if (c.het_M > 0) {                                     // (cnf_ensemble_set_members: host arrays, checked before any device is asked for)
        if (c.het_M != c.M) return fail(h, CNF_ERR_BAD_ARG, "cnf_ensemble_set_members was called for another number of members");
        for (int v : c.counts)
            if (v < 1 || v > c.B) return fail(h, CNF_ERR_BAD_ARG, "a member's count must be within [1, B]");
        for (float v : c.tols)
            if (!std::isfinite(v) || !(v > 0.f)) return fail(h, CNF_ERR_BAD_ARG, "a member's tolerances must be finite and positive");
        for (size_t i = 0; i < c.lams.size(); ++i)         // (which of the lambdas are zero decides the state rows: the handle's)
            if (!std::isfinite(c.lams[i]) || (c.lams[i] == 0.f) != (h->lam[i % 3] == 0.f))
                return fail(h, CNF_ERR_BAD_ARG, "a member's lambda must be finite, and zero exactly where the handle's is");
    }
    if (c.base_M > 0 && c.base_M != c.M) return fail(h, CNF_ERR_BAD_ARG, "cnf_ensemble_set_bases was called for another number of members");
    if (c.times)
        for (int m = 0; m < c.M; ++m)
            if (!std::isfinite(c.times[m]) || c.times[m] == (c.gen ? c.opts->t1 : c.opts->t0))
                return fail(h, CNF_ERR_BAD_ARG, "empty or NaN time span of a member");
    while (!h->collecting && !h->submitted.empty())       // (as any other call: the inferences submitted on the handle end first)
        if ((s = collect_one(h, nullptr)) != CNF_OK) return s;
    if (c.opts->kernel == CNF_KERNEL_GENERIC) return fail(h, CNF_ERR_UNSUPPORTED, "the ensemble form exists on the wave kernels only");
    const int capacity = c.path_many ? (c.grad ? cnf_ensemble_path_vjp_capacity(h, c.mode, c.B) : cnf_ensemble_path_capacity(h, c.mode, c.B))
                         : c.grad    ? ens_grad_capacity(h, c.mode, c.B, c.base_M > 0 ? wave_cot_based(c.cot) : c.cot)
                                     : cnf_ensemble_eval_capacity(h, c.mode, c.B);
    if (capacity < 1) return fail(h, CNF_ERR_UNSUPPORTED, "no ensemble form for this model, mode or batch");
    if (c.M > capacity)
        return fail(h, CNF_ERR_UNSUPPORTED, (std::string("more members than one launch takes (") + capacity_fn + ")").c_str());
    HIPCHK(h, hipSetDevice(h->device));
    return CNF_OK;
}

// The members' stores: grown behind a wait for the device, so that steady-state calls allocate nothing.  cols_f: the column
// store; traj_f, hs_f, gpart_f: the gradient's trajectories, step sizes and partials; trace_f: the eval calls' trace (floats)
static cnf_status ens_grow(cnf_handle h, const EnsCall& c, size_t cols_f, size_t traj_f, size_t hs_f, size_t gpart_f, size_t trace_f) {
    const size_t Mz = (size_t)c.M, fin_f = ens_fin_floats(c.M), part_f = Mz * WV_ENS_PART_FLOATS;
    if (traj_f <= h->ens_traj.capacity() && hs_f <= h->ens_hs.capacity() && gpart_f <= h->ens_gpart.capacity() &&
        trace_f <= h->ens_trace.capacity() && cols_f <= h->ens_cols.capacity() && part_f <= h->ens_part.capacity() &&
        2 * Mz <= h->ens_words.capacity() && fin_f <= h->ens_fin.capacity() && fin_f + Mz <= h->ens_hfin.capacity() &&
        Mz <= h->ens_t1.capacity() && (c.het_M == 0 || (6 * Mz <= h->ens_het.capacity() && 6 * Mz <= h->ens_hhet.capacity())))
        return CNF_OK;
    HIPCHK(h, hipDeviceSynchronize());
    if (c.grad) h->ens_M = 0;
    if (trace_f > h->ens_trace.capacity()) { h->ensv_M = 0; h->ejvp_M = 0; }
    RESERVE(h, h->ens_traj, traj_f);
    RESERVE(h, h->ens_hs, hs_f);
    RESERVE(h, h->ens_gpart, gpart_f);
    RESERVE(h, h->ens_cols, cols_f);
    RESERVE(h, h->ens_words, 2 * Mz);
    RESERVE(h, h->ens_fin, fin_f);
    RESERVE(h, h->ens_hfin, fin_f + Mz);
    RESERVE(h, h->ens_t1, Mz);
    RESERVE(h, h->ens_trace, trace_f);
    if (c.het_M > 0) {
        RESERVE(h, h->ens_het, 6 * Mz);
        RESERVE(h, h->ens_hhet, 6 * Mz);
    }
    if (part_f > h->ens_part.capacity()) {
        RESERVE(h, h->ens_part, part_f);
        HIPCHK(h, hipMemset(h->ens_part, 0, part_f * sizeof(float)));
        h->ens_base = 0;
    }
    return CNF_OK;
}

// The launch preamble: the lock, the meeting words, the members' times, the common part of c.sv.  (An early return of the
// caller lets go of the lock with c.)
static cnf_status ens_begin(cnf_handle h, EnsCall& c) {
    const size_t Mz = (size_t)c.M;
    const cnf_solve_opts* opts = c.opts;
    c.lock = std::unique_lock<std::mutex>(g_persist_mu);   // one one-launch solve at a time in this process
    if (g_submitted_inflight > 0 && g_submitted_stream != c.st) HIPCHK(h, hipStreamSynchronize(g_submitted_stream));
    // the meeting indices of this launch go on from where the earlier ones may have ended (a meeting per attempt, the two of the
    // initial dt, the loss sums; twice that: a workgroup placed late reads a base its member has already advanced), so that no
    // word an earlier call left can pass for news; when the 32 bits run out the words are cleared and the count starts again
    const unsigned long long span = 2ull * ((unsigned long long)opts->maxiters + 8ull);
    if ((unsigned long long)h->ens_base + span >= 0xffffffffull) {
        HIPCHK(h, hipMemsetAsync(h->ens_part, 0, h->ens_part.capacity() * sizeof(float), c.st));
        h->ens_base = 0;
    }
    HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)h->ens_words.data(), (int)h->ens_base, Mz, c.st));
    HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)(h->ens_words.data() + Mz), 0, Mz, c.st));
    h->ens_base += (unsigned)(span < 0xffffffffull ? span : 0xfffffffeull);
    if (c.times) {                                         // (through the pinned tail of ens_hfin)
        float* pin = h->ens_hfin + ens_fin_floats(c.M);
        memcpy(pin, c.times, Mz * sizeof(float));
        HIPCHK(h, hipMemcpyAsync(h->ens_t1, pin, Mz * sizeof(float), hipMemcpyHostToDevice, c.st));
    }
    if (c.het_M > 0) {                                     // the members' own counts | lambdas | tolerances: one copy through pinned memory
        float* pin = h->ens_hhet;
        if (!c.counts.empty()) { memcpy(pin, c.counts.data(), Mz * sizeof(int)); c.d_counts = reinterpret_cast<const int*>(h->ens_het.data()); }
        if (!c.lams.empty()) { memcpy(pin + Mz, c.lams.data(), 3 * Mz * sizeof(float)); c.d_lams = h->ens_het + Mz; }
        if (!c.tols.empty()) { memcpy(pin + 4 * Mz, c.tols.data(), 2 * Mz * sizeof(float)); c.d_tols = h->ens_het + 4 * Mz; }
        HIPCHK(h, hipMemcpyAsync(h->ens_het, pin, 6 * Mz * sizeof(float), hipMemcpyHostToDevice, c.st));
    }
    c.hairer = opts->adaptive && opts->dt == 0.f;
    Solve3Args& sv = c.sv;
    sv.part = h->ens_part; sv.base_dev = h->ens_words; sv.abort_flag = reinterpret_cast<int*>(h->ens_words.data() + Mz);
    sv.maxiters = (int)opts->maxiters; sv.hairer = c.hairer ? 1 : 0; sv.init = init_step_state(opts, (c.B + 15) / 16);
    set_wait_bounds(h, sv);
    return CNF_OK;
}

// The tail: the final states come back, the call waits for the stream (no mirror is polled) and lets go of the lock.  Then per
// member its stats, its status and -- sums: the call has loss sums -- its loss.  steps[m]: the accepted steps (attempts: all
// attempts) of a member that succeeded, -1 of the others.
static cnf_status ens_finish(cnf_handle h, EnsCall& c, int launches, bool sums, float* loss_out, int* status_out,
                             cnf_solve_stats* stats_out, std::vector<int>& steps, bool attempts, std::vector<int>* nacc = nullptr) {
    const size_t Mz = (size_t)c.M;
    HIPCHK(h, hipMemcpyAsync(h->ens_hfin, h->ens_fin, ens_fin_floats(c.M) * sizeof(float), hipMemcpyDeviceToHost, c.st));
    HIPCHK(h, hipStreamSynchronize(c.st));
    c.lock.unlock();
    steps.assign(Mz, -1);
    if (nacc) nacc->assign(Mz, -1);                        // (the accepted steps beside the attempts: the path calls file pairs of them)
    for (int m = 0; m < c.M; ++m) {
        StepState fin;
        memcpy(&fin, h->ens_hfin + (size_t)m * ENS_ST_F, sizeof fin);
        const int natt = fin.naccept + fin.nreject;
        fill_stats(stats_out ? stats_out + m : nullptr, fin, (c.hairer ? 2 : 1) + 6 * natt, CNF_KERNEL_MFMA, launches);
        float loss = NAN;
        if (fin.n_partials < 0) status_out[m] = CNF_ERR_UNSUPPORTED;             // a wait ran out, or more steps than its store holds
        else if (fin.nonfinite) status_out[m] = CNF_ERR_NONFINITE;
        else if (!fin.done) status_out[m] = CNF_ERR_MAXITERS;
        else {
            // (a failure here is that member's status: the launch ran, so the call goes on and returns CNF_OK)
            // (the fifth sum is the member's own count, as its part of the launch wrote it; the lambdas are its own too)
            const float* lam = c.lams.empty() ? h->lam : c.lams.data() + 3 * (size_t)m;
            status_out[m] = sums ? loss_from_sums_lam(h, c.mode, h->ens_hfin + Mz * ENS_ST_F + 5 * (size_t)m, lam, &loss) : CNF_OK;
            if (status_out[m] == CNF_OK) { steps[m] = attempts ? natt : fin.naccept; if (nacc) (*nacc)[(size_t)m] = fin.naccept; }
            else loss = NAN;
        }
        if (loss_out) loss_out[m] = loss;
    }
    return CNF_OK;
}

// The members' own bases (cnf_ensemble_set_bases), in front of ens_finish: the flags k_ens_base_prepare left -- a member whose mean
// or scale was no valid Gaussian -- on their way to the host behind everything the call enqueued ...
static cnf_status ens_base_flags_enqueue(cnf_handle h, const EnsCall& c) {
    if (!c.d_bases) return CNF_OK;
    launch_ens_base_flags(c.d_bases, h->ens_bcounts, c.M, c.st);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(h->ens_hbflags, h->ens_bcounts, (size_t)c.M * sizeof(int), hipMemcpyDeviceToHost, c.st));
    return CNF_OK;
}
// ... and behind it (the stream has been waited for): such a member is CNF_ERR_BAD_ARG, whatever its solve did; and what
// cnf_ensemble_base_logpdf_pullback needs of this call -- the columns it reads are at `off` of the column store, `stride` floats
// each (an inference: the final columns; sampling: u0 = [z0; 0])
static void ens_base_close(cnf_handle h, const EnsCall& c, float* loss_out, int* status_out, size_t off, int stride) {
    if (!c.d_bases) return;
    for (int m = 0; m < c.M; ++m)
        if (h->ens_hbflags[m]) {
            status_out[m] = CNF_ERR_BAD_ARG;
            if (loss_out) loss_out[m] = NAN;
        }
    h->lbase_M = c.M; h->lbase_kind = c.base_kind; h->lbase_B = c.B; h->lbase_stride = stride; h->lbase_off = off;
    h->lbase_counts = c.d_counts != nullptr;
}

// Nothing of a member that is not CNF_OK is valid: NaN in its own columns of the two outputs (out1 may be null) -- out0 [B][nv]
// and out1 [B] of sampling, out0 [B] and out1 [3][B] of an inference; a heterogeneous member's columns behind its count stay
// as the caller left them.
static size_t ens_member_count(const EnsCall& c, int m) { return (size_t)(c.counts.empty() ? c.B : c.counts[(size_t)m]); }
static cnf_status ens_fill_member(cnf_handle h, const EnsCall& c, int m, bool gen, size_t nv, float* out0, float* out1) {
    const size_t Bz = (size_t)c.B, cnt = ens_member_count(c, m);
    HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)out0, 0x7fc00000, gen ? cnt * nv : cnt, c.st));
    if (!out1) return CNF_OK;
    for (size_t r = 0; r < (gen ? 1u : 3u); ++r) {
        if (cnt == Bz && !gen) { HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)out1, 0x7fc00000, 3 * Bz, c.st)); break; }
        HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)(out1 + r * Bz), 0x7fc00000, cnt, c.st));
    }
    return CNF_OK;
}

// u0 = [z0; 0] of all `cols_n` = M B columns of a sampling call (the members' columns are contiguous), D floats per column
static cnf_status ens_sampling_u0(cnf_handle h, float* u0, const float* z0, size_t cols_n, size_t n_in, size_t D, hipStream_t st,
                                  const int* counts, int B) {
    if (counts) {                                          // (heterogeneous members: a column kernel that skips what lies behind a count)
        launch_ens_u0_counts((int)n_in, (int)D, z0, u0, cols_n, counts, B, st);
        HIPCHK(h, hipGetLastError());
        return CNF_OK;
    }
    HIPCHK(h, hipMemsetAsync(u0, 0, cols_n * D * sizeof(float), st));
    HIPCHK(h, hipMemcpy2DAsync(u0, D * sizeof(float), z0, n_in * sizeof(float), n_in * sizeof(float), cols_n, hipMemcpyDeviceToDevice, st));
    return CNF_OK;
}

// What the three ensemble gradient calls share.
//   cnf_loss_grad_many (WC_LOSS): src = xs; the built-in loss's cotangent, losses in loss_out; logpx, regs and d / d z(t0) stay in
//     the ensemble's own column store.
//   cnf_inference_vjp_many (WC_INFERENCE): src = xs, cot0 = [M][4][B]: the CW form of the kernel; out0 = logpx, out1 = regs and --
//     may be null -- grad_in = d / d z(t0) are the caller's.
//   cnf_generate_vjp_many (WC_SAMPLING): src = z0, times = the START times, cot0 = cot_z, cot1 = cot_logq (either may be null); the
//     sampling CW form integrates u0 = [z0; 0] (built in the column store, the final columns behind it); out0 = x, out1 = logq
//     and grad_in = d / d z0 (may be null) come from the column kernels of cnf_dist.hip over the M B columns as one batch.
//   cnf_inference_path_vjp / cnf_generate_path_vjp and their _many forms (WC_INFERENCE_PATH, WC_SAMPLING_PATH): the two above plus
//     `ep` -- the save times, the cotangent of the slices and where the slices go (either may be null, and so may cot0 / cot1
//     then).  The single-model calls are the M = 1 case; they keep their own step record (cnf_path_vjp_steps) and capacity.
namespace {
struct EnsPath {
    const float* saveat;           // host, [K] or (per_member) [M][K]: checked by the caller (saveat_error / saveat_error_many)
    int K;
    const float* cot;              // device, [M][K][B][D] or null
    float* out;                    // device, [M][K][B][D] or null
    bool per_member = false;       // every member has its own save times
    bool many = false;             // a call of include/cnfhip_ensemble_path.h (false: of cnfhip_path_vjp.h, M = 1)
};
}  // namespace
// the save times of M members, each set checked as cnf_solve_path checks its own; looks at no handle
static const char* saveat_error_many(const cnf_solve_opts* opts, const float* saveat_host, int K, int M, int per_member) {
    if (per_member != 0 && per_member != 1) return "saveat_per_member is 0 or 1";
    const int sets = per_member && M > 1 ? M : 1;
    for (int m = 0; m < sets; ++m)
        if (const char* bad = saveat_error(opts, saveat_host ? saveat_host + (size_t)m * (size_t)(K > 0 ? K : 0) : nullptr, K)) return bad;
    return nullptr;
}
// the save times to the device, the members' step pairs: the path arguments of a launch of M members
static cnf_status ens_path_args(cnf_handle h, const EnsPath& ep, int M, bool grad, hipStream_t st, WavePathArgs& wp) {
    // the kernel reads [M][K] save times: one set for all members is laid out M times here (the stride arithmetic is the host's)
    const size_t Kz = (size_t)ep.K, Mz = (size_t)M;
    RESERVE(h, h->d_saveat, Mz * Kz);
    const float* src = ep.saveat;
    if (!ep.per_member && M > 1) {
        h->saveat_rep.resize(Mz * Kz);
        for (size_t m = 0; m < Mz; ++m) memcpy(h->saveat_rep.data() + m * Kz, ep.saveat, Kz * sizeof(float));
        src = h->saveat_rep.data();
    }
    HIPCHK(h, hipMemcpyAsync(h->d_saveat, src, Mz * Kz * sizeof(float), hipMemcpyHostToDevice, st));
    wp.times = h->d_saveat; wp.K = ep.K; wp.out = ep.out; wp.cot = ep.cot;
    if (ep.many) {
        wp.steps_cap = grad ? ENS_PATH_VJP_STEPS_CAP : ENS_PATH_STEPS_CAP;
        RESERVE(h, h->ens_psteps, (size_t)M * 2 * (size_t)wp.steps_cap);
        wp.steps = h->ens_psteps;
    } else {
        RESERVE(h, h->d_path_steps, (size_t)2 * PATH_STEPS_CAP);
        wp.steps = h->d_path_steps; wp.steps_cap = PATH_STEPS_CAP;
    }
    return CNF_OK;
}
// a member that is not CNF_OK: NaN in its own slab of the slices
static cnf_status ens_path_fill(cnf_handle h, const EnsPath& ep, int m, size_t slab, hipStream_t st) {
    if (ep.out) HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)(ep.out + (size_t)m * slab), 0x7fc00000, slab, st));
    return CNF_OK;
}
static cnf_status ens_grad(cnf_handle h, WaveCot cot, int mode, int M, const float* params_dev, const float* src, const float* eps, int B,
                           const cnf_solve_opts* opts, const float* times_host, const float* cot0, const float* cot1, float* loss_out,
                           float* out0, float* out1, float* grad_dev, float* grad_in, int* status_out, cnf_solve_stats* stats_out,
                           void* stream, const EnsPath* ep = nullptr) {
    const bool train = mode == CNF_MODE_TRAIN, vjp = cot != WC_LOSS, gen = wave_cot_sampling(cot);
    if (h && ep) { if (ep->many) h->epath_M = 0; else h->pvjp_valid = false; }
    EnsCall c{true, gen, mode, M, B, 0, opts, times_host, (hipStream_t)stream};
    c.cot = cot; c.path_many = ep && ep->many;
    ens_take_members(h, c);
    if (ep) { c.het_M = 0; c.counts.clear(); c.lams.clear(); c.tols.clear(); }      // (the path calls take no such arrays: taken and dropped)
    if (ep && c.base_M > 0) return fail(h, CNF_ERR_UNSUPPORTED, "the path calls take no bases (cnf_ensemble_set_bases): they were dropped");
    cnf_status s = ens_check(h, c, !params_dev || !src || !opts || !grad_dev || !status_out || (train && !eps) ||
                                       (gen ? (!ep && !cot0 && !cot1) || !out0 || !out1 : vjp ? (!ep && !cot0) || !out0 || !out1 : !loss_out),
                             vjp ? "B must be >= 1" : "the loss is a mean over the batch: B must be >= 1",
                             ep ? (ep->many ? "cnf_ensemble_path_vjp_capacity" : "cnf_path_vjp_max_batch") : gen ? "cnf_ensemble_generate_vjp_capacity" : vjp ? "cnf_ensemble_vjp_capacity" : "cnf_ensemble_capacity");
    if (s != CNF_OK) return s;
    const NetDesc& nd = h->nd_wave;
    const size_t Mz = (size_t)M, Bz = (size_t)B, n_in = (size_t)nd.n_in, nv = (size_t)nd.nvars, D = n_in + (train ? 3 : 1), np = h->n_params;
    const size_t per_step = wave_grad_traj_floats(nd, B);
    // step slots per member: the single model's, for the M trajectory stores together
    const int tiles = wave_grad_waves(B), cap = traj_step_slots(per_step * Mz);
    // the column store: final columns | logpx | regs | d / d z(t0);  sampling: u0 | final columns | d / d u(t_start)
    if ((s = ens_grow(h, c, Mz * Bz * (gen ? 2 * D + n_in : D + 4 + n_in), per_step * cap * Mz, Mz * cap, Mz * tiles * np, 0)) != CNF_OK) return s;
    h->rec.clear();                                        // (as every gradient call; the handle's own model is not touched)
    h->ens_M = 0;
    if ((s = ens_begin(h, c)) != CNF_OK) return s;
    StepState* fin_dev = reinterpret_cast<StepState*>(h->ens_fin.data());
    float* cols = h->ens_cols;
    float* fsol = gen ? cols + Mz * Bz * D : cols;         // the final columns
    Solve3Args& sv = c.sv;
    WaveGradArgs wg;
    if (gen) {
        if ((s = ens_sampling_u0(h, cols, src, Mz * Bz, n_in, D, c.st, c.d_counts, B)) != CNF_OK) return s;
        sv.u0 = cols;
        wg.lam_out = cols + Mz * Bz * 2 * D;               // (k_generate_z0_grad must not write where it reads)
    } else {
        sv.xs = src; sv.logpx = vjp ? out0 : cols + Mz * Bz * D; sv.regs = vjp ? out1 : cols + Mz * Bz * (D + 1);
        sv.sums5 = h->ens_fin + Mz * ENS_ST_F;
        wg.lam_out = grad_in ? grad_in : cols + Mz * Bz * (D + 4);
    }
    wg.traj = h->ens_traj; wg.traj_cap = cap; wg.hs_out = h->ens_hs; wg.gpart = h->ens_gpart; wg.n_params = (int)np;
    wg.lam1 = h->lam[0]; wg.lam2 = h->lam[1]; wg.lam3 = h->lam[2];
    WaveEnsLaunch ens;
    ens.M = M;
    ens.counts = c.d_counts; ens.lams = c.d_lams; ens.tols = c.d_tols;
    (gen ? ens.t0 : ens.t1) = times_host ? h->ens_t1.data() : nullptr;
    if (gen) { ens.sampling = true; ens.cot_z = cot0; ens.cot_logq = cot1; }
    else { ens.cw = vjp ? cot0 : nullptr; ens.bases = c.d_bases; }      // (sampling: the cotangent of the final state is an input)
    ens.p_stride = np; ens.traj_stride = per_step * cap; ens.part_stride = WV_ENS_PART_FLOATS;
    WavePathArgs wp{};
    if (ep && (s = ens_path_args(h, *ep, M, true, c.st, wp)) != CNF_OK) return s;
    int launches = 0;                                      // kernel launches of this call, counted where they are made
    s = wave_solve_launch(nd, train, params_dev, nullptr, 0, fin_dev, fsol, eps, B, c.st, nullptr, 0, sv, &wg, &ens, ep ? &wp : nullptr);
    if (s != CNF_OK) return fail(h, s, "the ensemble launch failed to start");
    ++launches;
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, launch_grad_reduce_many(wg.gpart, grad_dev, (int)np, tiles, fin_dev, M, c.st, c.d_counts));
    ++launches;
    if (gen) {                                             // the column kernels: x and logq off the final state, then the z0 tail
        if (c.d_bases) launch_ens_base_generate_post((int)n_in, (int)nv, (int)D, c.d_bases, fsol, src, out0, out1, B, c.d_counts, M, c.st);
        else launch_generate_post_rows((int)n_in, (int)nv, (int)D, fsol, src, out0, out1, Mz * Bz, c.st, c.d_counts, B);
        HIPCHK(h, hipGetLastError());
        ++launches;
        if (grad_in) {
            if (c.d_bases) launch_ens_base_z0_grad((int)n_in, c.d_bases, wg.lam_out, cot1, src, grad_in, B, c.d_counts, M, c.st);
            else launch_generate_z0_grad((int)n_in, BaseDist{}, wg.lam_out, cot1, src, grad_in, Mz * Bz, c.st, c.d_counts, B);
            HIPCHK(h, hipGetLastError());
            ++launches;
        }
    } else if (c.d_bases) {                                // logpx under the members' bases, and their loss sums, afresh
        launch_ens_base_post((int)n_in, (int)D, c.d_bases, fin_dev, fsol, sv.logpx, sv.regs, B, c.d_counts, sv.sums5, M, c.st);
        HIPCHK(h, hipGetLastError());
        ++launches;
    }
    if ((s = ens_base_flags_enqueue(h, c)) != CNF_OK) return s;
    if ((s = ens_finish(h, c, launches, !gen, loss_out, status_out, stats_out, h->ens_nacc, false)) != CNF_OK) return s;
    ens_base_close(h, c, loss_out, status_out, gen ? 0 : (size_t)(fsol - cols), (int)D);
    h->ens_M = M; h->ens_cap = cap;
    if (vjp) {                                             // nothing of a member that is not CNF_OK is valid: NaN outputs, zero gradients
        bool any_bad = false;
        const size_t n0 = gen ? Bz * nv : Bz, n1 = gen ? Bz : 3 * Bz;
        for (int m = 0; m < M; ++m)
            if (status_out[m] != CNF_OK) {
                any_bad = true;
                const size_t mz = (size_t)m;
                if ((s = ens_fill_member(h, c, m, gen, nv, out0 + mz * n0, out1 + mz * n1)) != CNF_OK) return s;
                HIPCHK(h, hipMemsetAsync(grad_dev + mz * np, 0, np * sizeof(float), c.st));
                if (grad_in) HIPCHK(h, hipMemsetAsync(grad_in + mz * Bz * n_in, 0, ens_member_count(c, m) * n_in * sizeof(float), c.st));
                if (ep && (s = ens_path_fill(h, *ep, m, (size_t)ep->K * Bz * D, c.st)) != CNF_OK) return s;
            }
        if (any_bad) HIPCHK(h, hipStreamSynchronize(c.st));
    }
    if (ep && ep->many) {                                  // (the members' step pairs stay on the device: cnf_ensemble_path_steps)
        h->epath_nacc = h->ens_nacc; h->epath_M = M; h->epath_cap = wp.steps_cap; h->epath_rows = -1;
    } else if (ep && status_out[0] == CNF_OK) {            // the accepted steps back from the device (cnf_path_vjp_steps)
        const int n = h->ens_nacc[0];
        std::vector<float> pairs((size_t)2 * (n > 0 ? n : 0));
        if (n > 0) HIPCHK(h, hipMemcpy(pairs.data(), h->d_path_steps, pairs.size() * sizeof(float), hipMemcpyDeviceToHost));
        h->pvjp_t.resize((size_t)(n > 0 ? n : 0)); h->pvjp_h.resize(h->pvjp_t.size());
        for (size_t i = 0; i < h->pvjp_t.size(); ++i) { h->pvjp_t[i] = pairs[2 * i]; h->pvjp_h[i] = pairs[2 * i + 1]; }
        h->pvjp_valid = n >= 0;
    }
    return CNF_OK;
}

extern "C" cnf_status cnf_loss_grad_many(cnf_handle h, int mode, int M, const float* params_dev, const float* xs, const float* eps,
                                         int B, const cnf_solve_opts* opts, const float* t1_host, float* loss_out, float* grad_dev,
                                         int* status_out, cnf_solve_stats* stats_out, void* stream) {
    return ens_grad(h, WC_LOSS, mode, M, params_dev, xs, eps, B, opts, t1_host, nullptr, nullptr, loss_out, nullptr, nullptr, grad_dev, nullptr,
                    status_out, stats_out, stream);
}

// Differentiable ensembles (include/cnfhip_ensemble_vjp.h): the vector-Jacobian product of the M members' inference for a
// per-sample cotangent of its four outputs, by the CW form of the same launch.
extern "C" cnf_status cnf_inference_vjp_many(cnf_handle h, int mode, int M, const float* params_dev, const float* xs, const float* eps,
                                             int B, const cnf_solve_opts* opts, const float* t1_host, const float* cot_dev,
                                             float* logpx_dev, float* regs_dev, float* grad_dev, float* grad_x_dev, int* status_out,
                                             cnf_solve_stats* stats_out, void* stream) {
    return ens_grad(h, WC_INFERENCE, mode, M, params_dev, xs, eps, B, opts, t1_host, cot_dev, nullptr, nullptr, logpx_dev, regs_dev, grad_dev,
                    grad_x_dev, status_out, stats_out, stream);
}

// Differentiable ensemble sampling (include/cnfhip_ensemble_generate_vjp.h): the M members' samples with their log-densities and
// the vector-Jacobian product of (x, logq) for a per-sample cotangent, by the sampling CW form of the same launch -- what
// cnf_generate_record + cnf_generate_pullback give for one model.
extern "C" cnf_status cnf_generate_vjp_many(cnf_handle h, int mode, int M, const float* params_dev, const float* z0, const float* eps,
                                            int B, const cnf_solve_opts* opts, const float* t0_host, const float* cot_z_dev,
                                            const float* cot_logq_dev, float* x_out, float* logq_out, float* grad_dev,
                                            float* grad_z0_dev, int* status_out, cnf_solve_stats* stats_out, void* stream) {
    return ens_grad(h, WC_SAMPLING, mode, M, params_dev, z0, eps, B, opts, t0_host, cot_z_dev, cot_logq_dev, nullptr, x_out, logq_out,
                    grad_dev, grad_z0_dev, status_out, stats_out, stream);
}

// Differentiable flow paths (include/cnfhip_path_vjp.h): one model's inference (sampling) with the flow at the caller's save times,
// and the vector-Jacobian product of the outputs AND of those slices, by the PATH forms of the per-sample-cotangent launch (M = 1).
extern "C" int cnf_path_vjp_max_batch(cnf_handle h, int mode) {
    if (!ens_handle_ok(h, mode)) return 0;
    // both directions' kernels hold it; a batch is tiles of 16 columns, at most 512 of them
    for (int B = 16 * 512; B >= 16; B -= 16)
        if (ens_grad_capacity(h, mode, B, WC_INFERENCE_PATH) >= 1 && ens_grad_capacity(h, mode, B, WC_SAMPLING_PATH) >= 1) return B;
    return 0;
}
// the member's status is the call's: there is one member and no streamed route behind this call
static cnf_status path_vjp_status(cnf_handle h, cnf_status s, int status) {
    if (s != CNF_OK || status == CNF_OK) return s;
    return fail(h, (cnf_status)status, status == CNF_ERR_UNSUPPORTED
                ? "the launch gave up: more accepted steps than it can differentiate, or a wait ran out (there is no streamed route for this call)"
                : status == CNF_ERR_MAXITERS ? "maxiters reached" : "solver state became NaN/Inf");
}
extern "C" cnf_status cnf_inference_path_vjp(cnf_handle h, int mode, const float* params_dev, const float* xs, const float* eps, int B,
                                             const cnf_solve_opts* opts, const float* saveat_host, int K, const float* cot_dev,
                                             const float* path_cot_dev, float* logpx_dev, float* regs_dev, float* path_out_dev,
                                             float* grad_dev, float* grad_x_dev, cnf_solve_stats* stats, void* stream) {
    if (const char* bad = saveat_error(opts, saveat_host, K)) return h ? fail(h, CNF_ERR_BAD_ARG, bad) : CNF_ERR_BAD_ARG;
    const EnsPath ep{saveat_host, K, path_cot_dev, path_out_dev};
    int status = CNF_OK;
    const cnf_status s = ens_grad(h, WC_INFERENCE_PATH, mode, 1, params_dev, xs, eps, B, opts, nullptr, cot_dev, nullptr, nullptr, logpx_dev,
                                  regs_dev, grad_dev, grad_x_dev, &status, stats, stream, &ep);
    return path_vjp_status(h, s, status);
}
extern "C" cnf_status cnf_generate_path_vjp(cnf_handle h, int mode, const float* params_dev, const float* z0, const float* eps, int B,
                                            const cnf_solve_opts* opts, const float* saveat_host, int K, const float* cot_z_dev,
                                            const float* cot_logq_dev, const float* path_cot_dev, float* x_out, float* logq_out,
                                            float* path_out_dev, float* grad_dev, float* grad_z0_dev, cnf_solve_stats* stats, void* stream) {
    if (const char* bad = saveat_error(opts, saveat_host, K)) return h ? fail(h, CNF_ERR_BAD_ARG, bad) : CNF_ERR_BAD_ARG;
    const EnsPath ep{saveat_host, K, path_cot_dev, path_out_dev};
    int status = CNF_OK;
    const cnf_status s = ens_grad(h, WC_SAMPLING_PATH, mode, 1, params_dev, z0, eps, B, opts, nullptr, cot_z_dev, cot_logq_dev, nullptr, x_out,
                                  logq_out, grad_dev, grad_z0_dev, &status, stats, stream, &ep);
    return path_vjp_status(h, s, status);
}
extern "C" int cnf_path_vjp_steps(cnf_handle h, float* t_host, float* h_host, int cap) {
    return h ? copy_steps(h->pvjp_valid, h->pvjp_t, h->pvjp_h, t_host, h_host, cap) : -1;
}

// Heterogeneous ensembles (include/cnfhip_ensemble_hetero.h): the members' own batch sizes, regularisers and tolerances for the
// NEXT ensemble call on the handle.  Host state only: the arrays are checked by that call (it knows M, B and the handle's
// lambdas), copied to the device in front of its launch, and gone when it returns.
extern "C" cnf_status cnf_ensemble_set_members(cnf_handle h, int M, const int* counts, const float* lams, const float* tols) {
    if (!h) return CNF_ERR_BAD_ARG;
    h->het_M = 0; h->het_counts.clear(); h->het_lams.clear(); h->het_tols.clear();
    if (M < 1) return fail(h, CNF_ERR_BAD_ARG, "cnf_ensemble_set_members: an ensemble has at least one member");
    const size_t Mz = (size_t)M;
    if (counts) h->het_counts.assign(counts, counts + Mz);
    if (lams) h->het_lams.assign(lams, lams + 3 * Mz);
    if (tols) h->het_tols.assign(tols, tols + 2 * Mz);
    h->het_M = (counts || lams || tols) ? M : 0;
    return CNF_OK;
}
extern "C" cnf_status cnf_ensemble_clear_members(cnf_handle h) {
    if (!h) return CNF_ERR_BAD_ARG;
    h->het_M = 0; h->het_counts.clear(); h->het_lams.clear(); h->het_tols.clear();
    return CNF_OK;
}

// Ensembles with a base per member (include/cnfhip_ensemble_base.h): N(mean_m, L_m L_m') for the NEXT ensemble call on the
// handle.  Unlike the members' counts these are DEVICE arrays, reduced on the device (k_ens_base_prepare) in stream order: a
// learnable base costs no host wait per step.
extern "C" cnf_status cnf_ensemble_set_bases(cnf_handle h, int M, int kind, const float* mean_dev, const float* chol_dev, void* stream) {
    if (!h) return CNF_ERR_BAD_ARG;
    h->base_M = 0;
    if (M < 1) return fail(h, CNF_ERR_BAD_ARG, "cnf_ensemble_set_bases: an ensemble has at least one member");
    if (kind != 1 && kind != 2) return fail(h, CNF_ERR_BAD_ARG, "cnf_ensemble_set_bases: kind must be 1 (diagonal) or 2 (dense)");
    if (!mean_dev || !chol_dev) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (h->nd.n_in > 16) return fail(h, CNF_ERR_UNSUPPORTED, "no ensemble form for this model (n_in > 16)");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t Mz = (size_t)M;
    RESERVE(h, h->ens_bases_pend, Mz * WV_ENS_BASE_FLOATS);      // (grow-only: a steady-state call allocates nothing)
    RESERVE(h, h->ens_bcounts, Mz);
    RESERVE(h, h->ens_hbflags, Mz);
    launch_ens_base_prepare(h->nd.n_in, kind, mean_dev, chol_dev, h->ens_bases_pend, M, (hipStream_t)stream);
    HIPCHK(h, hipGetLastError());
    h->base_M = M; h->base_kind = kind;
    return CNF_OK;
}
extern "C" cnf_status cnf_ensemble_clear_bases(cnf_handle h) {
    if (!h) return CNF_ERR_BAD_ARG;
    h->base_M = 0;
    return CNF_OK;
}
// the largest M of cnf_loss_grad_many (per_sample = 0) / cnf_inference_vjp_many (1) with bases: the BASE kernels' own budget
extern "C" int cnf_ensemble_base_capacity(cnf_handle h, int mode, int B, int per_sample) {
    return ens_grad_capacity(h, mode, B, per_sample ? WC_INFERENCE_BASE : WC_LOSS_BASE);
}
// the bases a base call finds: the pending ones (they stay pending), else the last call's
static const float* ens_bases_for(cnf_handle h, int M, int* kind) {
    if (h->base_M > 0) { *kind = h->base_kind; return h->base_M == M ? h->ens_bases_pend.data() : nullptr; }
    if (h->lbase_M > 0) { *kind = h->lbase_kind; return h->lbase_M == M ? h->ens_bases_last.data() : nullptr; }
    return nullptr;
}
extern "C" cnf_status cnf_ensemble_base_sample(cnf_handle h, int M, const float* normals_dev, float* z0_dev, int B, void* stream) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (!normals_dev || !z0_dev || normals_dev == z0_dev) return fail(h, CNF_ERR_BAD_ARG, "normals and z0 must be distinct buffers");
    if (M < 1 || B < 1) return fail(h, CNF_ERR_BAD_SHAPE, "M and B must be >= 1");
    int kind = 0;
    const float* bases = ens_bases_for(h, M, &kind);
    if (!bases) return fail(h, CNF_ERR_BAD_ARG, "cnf_ensemble_base_sample: no bases of M members are pending or on record");
    HIPCHK(h, hipSetDevice(h->device));
    launch_ens_base_sample(h->nd.n_in, kind, bases, normals_dev, z0_dev, B, M, (hipStream_t)stream);
    HIPCHK(h, hipGetLastError());
    return CNF_OK;
}
extern "C" cnf_status cnf_ensemble_base_logpdf_pullback(cnf_handle h, int M, const float* w_dev, int B, float* g_mean_dev, float* g_chol_dev,
                                                        void* stream) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (!w_dev || !g_mean_dev || !g_chol_dev) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (h->lbase_M < 1 || h->lbase_M != M || h->lbase_B != B)
        return fail(h, CNF_ERR_BAD_ARG, "cnf_ensemble_base_logpdf_pullback: the last ensemble call had no bases, or another M or B");
    HIPCHK(h, hipSetDevice(h->device));
    launch_ens_base_logpdf_pullback(h->nd.n_in, h->lbase_kind, h->ens_bases_last, h->ens_cols + h->lbase_off, h->lbase_stride, w_dev, B,
                                    h->lbase_counts ? reinterpret_cast<const int*>(h->ens_het.data()) : nullptr, g_mean_dev, g_chol_dev, M,
                                    (hipStream_t)stream);
    HIPCHK(h, hipGetLastError());
    return CNF_OK;
}
extern "C" cnf_status cnf_ensemble_base_sample_pullback(cnf_handle h, int M, int kind, const float* normals_dev, const float* g_z0_dev, int B,
                                                        const int* counts_dev, float* g_mean_dev, float* g_chol_dev, void* stream) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (!normals_dev || !g_z0_dev || !g_mean_dev || !g_chol_dev) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (kind != 1 && kind != 2) return fail(h, CNF_ERR_BAD_ARG, "kind must be 1 (diagonal) or 2 (dense)");
    if (M < 1 || B < 1) return fail(h, CNF_ERR_BAD_SHAPE, "M and B must be >= 1");
    if (h->nd.n_in > 16) return fail(h, CNF_ERR_UNSUPPORTED, "no ensemble form for this model (n_in > 16)");
    HIPCHK(h, hipSetDevice(h->device));
    launch_ens_base_sample_pullback(h->nd.n_in, kind, normals_dev, g_z0_dev, B, counts_dev, g_mean_dev, g_chol_dev, M, (hipStream_t)stream);
    HIPCHK(h, hipGetLastError());
    return CNF_OK;
}

// the signed accepted step sizes of member `member` of the last ensemble gradient call -- cnf_loss_grad_many,
// cnf_inference_vjp_many or cnf_generate_vjp_many -- (read from the device when asked for)
extern "C" int cnf_ensemble_steps(cnf_handle h, int member, float* hs, int cap) {
    if (!h || member < 0 || member >= h->ens_M) return -1;
    const int n = h->ens_nacc[member];
    if (n < 0) return -1;
    const int take = n < cap ? n : cap;
    if (hs && take > 0) {
        if (hipSetDevice(h->device) != hipSuccess ||
            hipMemcpy(hs, h->ens_hs + (size_t)member * h->ens_cap, (size_t)take * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            return -1;
        }
    }
    return n;
}

// ---------------------------------------------------------------------------------------
// Ensemble inference and sampling (include/cnfhip_ensemble_eval.h): the M members scored (cnf_inference_many) or sampled
// (cnf_generate_many) by ONE launch of the plain ENS form of k_solve_wave.  The meeting words, bases, final states and column
// store are the ensemble's own buffers above; nothing of the handle's model, solver state or record is touched.
// ---------------------------------------------------------------------------------------
extern "C" int cnf_ensemble_eval_capacity(cnf_handle h, int mode, int B) {
    if (B < 1 || !ens_handle_ok(h, mode)) return 0;
    if (hipSetDevice(h->device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return wave_ens_eval_capacity(h->nd_wave, mode == CNF_MODE_TRAIN, B);
}

// What the two calls share.  gen = false: src = xs [M][B][nvars], out0 = logpx [M][B], out1 = regs [M][3][B], times = the end
// times; gen = true: src = z0 [M][B][n_in], out0 = xs_out [M][B][nvars], out1 = logq [M][B] or null, times = the start times.
// jv (cnf_inference_jvp_many / cnf_generate_jvp_many, include/cnfhip_ensemble_jvp.h): the same call with every member's attempts
// kept, and the ENS form of k_tangent_wave enqueued right behind the solve (sampling: behind its column kernel) on the same
// stream, no host wait in between -- it reads the members' final states and attempts where the solve left them.  Sampling's out0
// is then z_out [M][B][n_in], all rows of the final state.
namespace {
struct EnsJvp {
    const float *d_ps, *d_x;       // device, [M][R][n_params] | [M][R][B][rows]; either may be null
    int R;
    float *d_out, *d_logq;         // device, [M][R][4][B] | sampling: [M][R][B][n_in] and [M][R][B]
};
}  // namespace
static const int ENS_JVP_TRACE_DEFAULT = 1024, ENS_JVP_TRACE_MAX = 65536;
static cnf_status ens_eval(cnf_handle h, bool gen, int mode, int M, const float* params_dev, const float* src, const float* eps, int B,
                           const cnf_solve_opts* opts, const float* times_host, float* out0, float* out1, float* loss_out,
                           int* status_out, cnf_solve_stats* stats_out, int trace_cap, void* stream, const EnsPath* ep = nullptr,
                           const EnsJvp* jv = nullptr) {
    const bool train = mode == CNF_MODE_TRAIN;
    if (h && ep) h->epath_M = 0;
    if (h && jv) h->ejvp_M = 0;
    EnsCall c{false, gen, mode, M, B, trace_cap, opts, times_host, (hipStream_t)stream};
    c.path_many = ep != nullptr;
    ens_take_members(h, c);
    if (ep) { c.het_M = 0; c.counts.clear(); c.lams.clear(); c.tols.clear(); }      // (the path calls take no such arrays: taken and dropped)
    if (ep && c.base_M > 0) return fail(h, CNF_ERR_UNSUPPORTED, "the path calls take no bases (cnf_ensemble_set_bases): they were dropped");
    if (jv) {                                              // (arguments before anything asks for a device; the taken arrays are gone either way)
        if (!jv->d_ps && !jv->d_x) return fail(h, CNF_ERR_BAD_ARG, "both directions are null");
        if (jv->R < 1 || jv->R > TG_MAX_R) return fail(h, CNF_ERR_BAD_ARG, "R must be within [1, 65535]");
        if (trace_cap > ENS_JVP_TRACE_MAX) return fail(h, CNF_ERR_BAD_ARG, "trace_cap must be within [0, 65536]");
    }
    cnf_status s = ens_check(h, c, !params_dev || !src || !opts || !out0 || (!gen && !out1) || !status_out || (train && !eps) || (ep && !ep->out) ||
                                       (jv && (!jv->d_out || (gen && (!jv->d_logq || !out1)))),
                             "B must be >= 1", ep ? "cnf_ensemble_path_capacity" : "cnf_ensemble_eval_capacity");
    if (s != CNF_OK) return s;
    if (jv) {
        if (c.base_M > 0) return fail(h, CNF_ERR_UNSUPPORTED, "the tangent calls take no bases (cnf_ensemble_set_bases): they were dropped");
        if (!tangent_supported(h->nd_wave))
            return fail(h, CNF_ERR_UNSUPPORTED, "tangents: two layers, tanh then tanh or identity, n_in <= 16, at most 64 hidden units (16 with the identity), no conditioning");
        if (trace_cap == 0) trace_cap = opts->maxiters < ENS_JVP_TRACE_DEFAULT ? (int)opts->maxiters : ENS_JVP_TRACE_DEFAULT;
        if (trace_cap < 1) trace_cap = 1;
    }
    const NetDesc& nd = h->nd_wave;
    // (a tangent call's samples are all rows of the final state)
    const size_t Mz = (size_t)M, Bz = (size_t)B, n_in = (size_t)nd.n_in, nv = jv && gen ? n_in : (size_t)nd.nvars, D = n_in + (train ? 3 : 1);
    // the column store: final columns (an inference) | u0 and the final columns (sampling)
    if ((s = ens_grow(h, c, Mz * Bz * (gen ? 2 * D : D), 0, 0, 0, Mz * 4 * (size_t)trace_cap)) != CNF_OK) return s;
    if (trace_cap > 0) { h->ensv_M = 0; h->ejvp_M = 0; }   // (the trace on record is about to be overwritten)
    if ((s = ens_begin(h, c)) != CNF_OK) return s;
    hipStream_t st = c.st;
    if (jv) {                                              // NaN wherever the tangent launch writes nothing: a member its guard turns away, columns behind a count
        const size_t MR = Mz * (size_t)jv->R;
        HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)jv->d_out, 0x7fc00000, MR * (gen ? Bz * n_in : 4 * Bz), st));
        if (gen) HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)jv->d_logq, 0x7fc00000, MR * Bz, st));
    }
    Solve3Args& sv = c.sv;
    if (trace_cap > 0) { sv.trace = h->ens_trace; sv.trace_cap = trace_cap; }
    float* cols = h->ens_cols;
    float* fsol = cols + Mz * Bz * D;                      // sampling: the final columns behind u0
    if (gen) {
        if ((s = ens_sampling_u0(h, cols, src, Mz * Bz, n_in, D, st, c.d_counts, B)) != CNF_OK) return s;
        sv.u0 = cols; sv.u_out = fsol;
    } else {
        sv.xs = src; sv.logpx = out0; sv.regs = out1; sv.sums5 = h->ens_fin + Mz * ENS_ST_F;
    }
    WaveEnsLaunch ens;
    ens.M = M;
    (gen ? ens.t0 : ens.t1) = times_host ? h->ens_t1.data() : nullptr;
    ens.p_stride = h->n_params; ens.part_stride = WV_ENS_PART_FLOATS;
    ens.counts = c.d_counts; ens.tols = c.d_tols;          // (the plain forms read no lambda; the members' losses take theirs: ens_finish)
    WavePathArgs wp{};
    if (ep && (s = ens_path_args(h, *ep, M, false, st, wp)) != CNF_OK) return s;
    int launches = 0;
    s = wave_solve_launch(nd, train, params_dev, nullptr, 0, reinterpret_cast<StepState*>(h->ens_fin.data()), cols, eps, B, st, nullptr, 0,
                          sv, nullptr, &ens, ep ? &wp : nullptr);
    if (s != CNF_OK) return fail(h, s, "the ensemble launch failed to start");
    ++launches;
    HIPCHK(h, hipGetLastError());
    if (gen) {
        if (c.d_bases) launch_ens_base_generate_post((int)n_in, (int)nv, (int)D, c.d_bases, fsol, src, out0, out1, B, c.d_counts, M, st);
        else launch_generate_post_rows((int)n_in, (int)nv, (int)D, fsol, src, out0, out1, Mz * Bz, st, c.d_counts, B);
        HIPCHK(h, hipGetLastError());
        ++launches;
    } else if (c.d_bases) {                                // logpx under the members' bases, and their loss sums, afresh
        launch_ens_base_post((int)n_in, (int)D, c.d_bases, reinterpret_cast<StepState*>(h->ens_fin.data()), cols, out0, out1, B, c.d_counts,
                             sv.sums5, M, st);
        HIPCHK(h, hipGetLastError());
        ++launches;
    }
    if (jv) {
        TangentArgs ta;
        ta.nd = nd; ta.P = params_dev; ta.dP = jv->d_ps; ta.n_params = (int)h->n_params; ta.eps = train ? eps : nullptr;
        ta.B = B; ta.R = jv->R; ta.sampling = gen ? 1 : 0; ta.x = src; ta.dX = jv->d_x;
        ta.st = reinterpret_cast<const StepState*>(h->ens_fin.data()); ta.trace = h->ens_trace; ta.trace_cap = trace_cap; ta.n_rows = -1;
        ta.out = jv->d_out; ta.out_logq = jv->d_logq;
        TangentEns te;
        te.M = M; te.p_stride = h->n_params; te.x_stride = Bz * (gen ? n_in : (size_t)nd.nvars); te.counts = c.d_counts;
        if ((s = tangent_launch_many(ta, te, train, st)) != CNF_OK) return fail(h, s, "the tangent launch failed to start");
        ++launches;
    }
    std::vector<int> att, nacc;
    if ((s = ens_base_flags_enqueue(h, c)) != CNF_OK) return s;
    if ((s = ens_finish(h, c, launches, !gen, loss_out, status_out, stats_out, att, true, ep ? &nacc : nullptr)) != CNF_OK) return s;
    ens_base_close(h, c, loss_out, status_out, 0, (int)D);
    if (jv)                                                // more attempts than the member had rows for: its tangent launch wrote nothing
        for (int m = 0; m < M; ++m)
            if (status_out[m] == CNF_OK && att[(size_t)m] > trace_cap) {
                status_out[m] = CNF_ERR_UNSUPPORTED; att[(size_t)m] = -1;
                if (loss_out) loss_out[m] = NAN;
            }
    bool any_bad = false;
    for (int m = 0; m < M; ++m)
        if (status_out[m] != CNF_OK) {                     // nothing of such a member is valid: NaN, whatever the kernel left
            any_bad = true;
            const size_t n0 = gen ? Bz * nv : Bz, n1 = gen ? Bz : 3 * Bz;
            if ((s = ens_fill_member(h, c, m, gen, nv, out0 + (size_t)m * n0, out1 ? out1 + (size_t)m * n1 : nullptr)) != CNF_OK) return s;
            if (ep && (s = ens_path_fill(h, *ep, m, (size_t)ep->K * Bz * D, st)) != CNF_OK) return s;
        }
    if (any_bad) HIPCHK(h, hipStreamSynchronize(st));
    if (ep) {                                              // (the members' step pairs stay on the device: cnf_ensemble_path_steps)
        for (int& n : nacc) if (n > wp.steps_cap) n = -1;  // (more accepted steps than a member files)
        h->epath_nacc.swap(nacc); h->epath_M = M; h->epath_cap = wp.steps_cap; h->epath_rows = -1;
    }
    if (trace_cap > 0) { h->ensv_att.swap(att); h->ensv_M = M; h->ensv_tcap = trace_cap; }
    if (jv) { h->ejvp_M = M; h->ejvp_rows = -1; }
    return CNF_OK;
}

extern "C" cnf_status cnf_inference_many(cnf_handle h, int mode, int M, const float* params_dev, const float* xs, const float* eps, int B,
                                         const cnf_solve_opts* opts, const float* t1_host, float* logpx_dev, float* regs_dev,
                                         float* loss_out, int* status_out, cnf_solve_stats* stats_out, int trace_cap, void* stream) {
    return ens_eval(h, false, mode, M, params_dev, xs, eps, B, opts, t1_host, logpx_dev, regs_dev, loss_out, status_out, stats_out,
                    trace_cap, stream);
}

extern "C" cnf_status cnf_generate_many(cnf_handle h, int mode, int M, const float* params_dev, const float* z0, const float* eps, int B,
                                        const cnf_solve_opts* opts, const float* t0_host, float* xs_out, float* logq_out,
                                        int* status_out, cnf_solve_stats* stats_out, int trace_cap, void* stream) {
    return ens_eval(h, true, mode, M, params_dev, z0, eps, B, opts, t0_host, xs_out, logq_out, nullptr, status_out, stats_out,
                    trace_cap, stream);
}

extern "C" int cnf_ensemble_eval_steps(cnf_handle h, int member, float* rows, int cap) {
    if (!h || member < 0 || member >= h->ensv_M || h->ensv_tcap < 1) return -1;
    const int n = h->ensv_att[member];
    if (n < 0) return -1;
    int take = n < cap ? n : cap;
    if (take > h->ensv_tcap) take = h->ensv_tcap;
    if (rows && take > 0) {
        if (hipSetDevice(h->device) != hipSuccess ||
            hipMemcpy(rows, h->ens_trace + (size_t)member * 4 * h->ensv_tcap, (size_t)take * 4 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            return -1;
        }
    }
    return n;
}

// ---------------------------------------------------------------------------------------
// Ensemble flow paths (include/cnfhip_ensemble_path.h): the paths of M members by the plain ensemble form with the path
// (ens_eval), and their vector-Jacobian products by the PATH forms of the per-sample-cotangent launch (ens_grad), M members each.
// ---------------------------------------------------------------------------------------
extern "C" int cnf_ensemble_path_capacity(cnf_handle h, int mode, int B) {
    if (B < 1 || !ens_handle_ok(h, mode)) return 0;
    if (hipSetDevice(h->device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return wave_ens_eval_capacity(h->nd_wave, mode == CNF_MODE_TRAIN, B, true);
}
extern "C" int cnf_ensemble_path_vjp_capacity(cnf_handle h, int mode, int B) {
    const int a = ens_grad_capacity(h, mode, B, WC_INFERENCE_PATH), b = ens_grad_capacity(h, mode, B, WC_SAMPLING_PATH);
    return a < b ? a : b;
}
// the save times first (with a NULL handle too), then: these calls have no per-member span
static cnf_status ens_path_entry(cnf_handle h, const cnf_solve_opts* opts, const float* saveat_host, int K, int M, int per_member,
                                 const float* times_host) {
    if (const char* bad = saveat_error_many(opts, saveat_host, K, M, per_member)) return h ? fail(h, CNF_ERR_BAD_ARG, bad) : CNF_ERR_BAD_ARG;
    if (times_host) return fail(h, CNF_ERR_BAD_ARG, "the ensemble path calls take no per-member start or end times");
    return CNF_OK;
}
extern "C" cnf_status cnf_inference_path_many(cnf_handle h, int mode, int M, const float* params_dev, const float* xs, const float* eps,
                                              int B, const cnf_solve_opts* opts, const float* t1_host, float* logpx_dev, float* regs_dev,
                                              float* loss_out, int* status_out, cnf_solve_stats* stats_out, int trace_cap, void* stream,
                                              const float* saveat_host, int K, int saveat_per_member, float* path_out_dev) {
    const cnf_status s = ens_path_entry(h, opts, saveat_host, K, M, saveat_per_member, t1_host);
    if (s != CNF_OK) return s;
    const EnsPath ep{saveat_host, K, nullptr, path_out_dev, saveat_per_member != 0, true};
    return ens_eval(h, false, mode, M, params_dev, xs, eps, B, opts, nullptr, logpx_dev, regs_dev, loss_out, status_out, stats_out, trace_cap,
                    stream, &ep);
}
extern "C" cnf_status cnf_generate_path_many(cnf_handle h, int mode, int M, const float* params_dev, const float* z0, const float* eps,
                                             int B, const cnf_solve_opts* opts, const float* t0_host, float* xs_out, float* logq_out,
                                             int* status_out, cnf_solve_stats* stats_out, int trace_cap, void* stream,
                                             const float* saveat_host, int K, int saveat_per_member, float* path_out_dev) {
    const cnf_status s = ens_path_entry(h, opts, saveat_host, K, M, saveat_per_member, t0_host);
    if (s != CNF_OK) return s;
    const EnsPath ep{saveat_host, K, nullptr, path_out_dev, saveat_per_member != 0, true};
    return ens_eval(h, true, mode, M, params_dev, z0, eps, B, opts, nullptr, xs_out, logq_out, nullptr, status_out, stats_out, trace_cap,
                    stream, &ep);
}
extern "C" cnf_status cnf_inference_path_vjp_many(cnf_handle h, int mode, int M, const float* params_dev, const float* xs,
                                                  const float* eps, int B, const cnf_solve_opts* opts, const float* saveat_host, int K,
                                                  int saveat_per_member, const float* cot_dev, const float* path_cot_dev,
                                                  float* logpx_dev, float* regs_dev, float* path_out_dev, float* grad_dev,
                                                  float* grad_x_dev, int* status_out, cnf_solve_stats* stats_out, void* stream) {
    const cnf_status s = ens_path_entry(h, opts, saveat_host, K, M, saveat_per_member, nullptr);
    if (s != CNF_OK) return s;
    const EnsPath ep{saveat_host, K, path_cot_dev, path_out_dev, saveat_per_member != 0, true};
    return ens_grad(h, WC_INFERENCE_PATH, mode, M, params_dev, xs, eps, B, opts, nullptr, cot_dev, nullptr, nullptr, logpx_dev, regs_dev,
                    grad_dev, grad_x_dev, status_out, stats_out, stream, &ep);
}
extern "C" cnf_status cnf_generate_path_vjp_many(cnf_handle h, int mode, int M, const float* params_dev, const float* z0,
                                                 const float* eps, int B, const cnf_solve_opts* opts, const float* saveat_host, int K,
                                                 int saveat_per_member, const float* cot_z_dev, const float* cot_logq_dev,
                                                 const float* path_cot_dev, float* x_out, float* logq_out, float* path_out_dev,
                                                 float* grad_dev, float* grad_z0_dev, int* status_out, cnf_solve_stats* stats_out,
                                                 void* stream) {
    const cnf_status s = ens_path_entry(h, opts, saveat_host, K, M, saveat_per_member, nullptr);
    if (s != CNF_OK) return s;
    const EnsPath ep{saveat_host, K, path_cot_dev, path_out_dev, saveat_per_member != 0, true};
    return ens_grad(h, WC_SAMPLING_PATH, mode, M, params_dev, z0, eps, B, opts, nullptr, cot_z_dev, cot_logq_dev, nullptr, x_out, logq_out,
                    grad_dev, grad_z0_dev, status_out, stats_out, stream, &ep);
}
// (read from the device when first asked for, all members at once)
extern "C" int cnf_ensemble_path_steps(cnf_handle h, int member, float* t_host, float* h_host, int cap) {
    if (!h || member < 0 || member >= h->epath_M) return -1;
    const int n = h->epath_nacc[(size_t)member];
    if (n < 0 || n > h->epath_cap) return -1;
    const int take = n < cap ? n : cap;
    if (take > 0 && (t_host || h_host)) {
        if (h->epath_rows < 0) {                           // every member's pairs in one strided copy (a copy per member costs a
            int rows = 0;                                  // synchronisation each: 1.2 ms of a 1.5 ms call at 64 members)
            for (int v : h->epath_nacc) if (v > rows && v <= h->epath_cap) rows = v;
            h->epath_host.resize((size_t)h->epath_M * 2 * (size_t)rows);
            if (hipSetDevice(h->device) != hipSuccess ||
                hipMemcpy2D(h->epath_host.data(), (size_t)2 * rows * sizeof(float), h->ens_psteps.data(),
                            (size_t)2 * h->epath_cap * sizeof(float), (size_t)2 * rows * sizeof(float), (size_t)h->epath_M,
                            hipMemcpyDeviceToHost) != hipSuccess) {
                (void)hipGetLastError();
                return -1;
            }
            h->epath_rows = rows;
        }
        const float* pairs = h->epath_host.data() + (size_t)member * 2 * (size_t)h->epath_rows;
        for (int i = 0; i < take; ++i) {
            if (t_host) t_host[i] = pairs[2 * (size_t)i];
            if (h_host) h_host[i] = pairs[2 * (size_t)i + 1];
        }
    }
    return n;
}

// ---------------------------------------------------------------------------------------
// Ensemble forward-mode (include/cnfhip_ensemble_jvp.h): cnf_inference_many / cnf_generate_many with every member's attempts kept
// and the ENS form of k_tangent_wave behind the solve (ens_eval's `jv`).
// ---------------------------------------------------------------------------------------
extern "C" cnf_status cnf_inference_jvp_many(cnf_handle h, int mode, int M, const float* params_dev, const float* xs, const float* eps,
                                             int B, const float* d_ps, const float* d_xs, int R, const cnf_solve_opts* opts,
                                             const float* t1_host, int trace_cap, float* logpx_dev, float* regs_dev, float* d_out_dev,
                                             float* loss_out, int* status_out, cnf_solve_stats* stats_out, void* stream) {
    const EnsJvp jv{d_ps, d_xs, R, d_out_dev, nullptr};
    return ens_eval(h, false, mode, M, params_dev, xs, eps, B, opts, t1_host, logpx_dev, regs_dev, loss_out, status_out, stats_out,
                    trace_cap, stream, nullptr, &jv);
}
extern "C" cnf_status cnf_generate_jvp_many(cnf_handle h, int mode, int M, const float* params_dev, const float* z0, const float* eps,
                                            int B, const float* d_ps, const float* d_z0, int R, const cnf_solve_opts* opts,
                                            const float* t0_host, int trace_cap, float* z_out, float* logq_out, float* d_z, float* d_logq,
                                            int* status_out, cnf_solve_stats* stats_out, void* stream) {
    const EnsJvp jv{d_ps, d_z0, R, d_z, d_logq};
    return ens_eval(h, true, mode, M, params_dev, z0, eps, B, opts, t0_host, z_out, logq_out, nullptr, status_out, stats_out,
                    trace_cap, stream, nullptr, &jv);
}
// (read from the device when first asked for, all members at once, as cnf_ensemble_path_steps reads its pairs)
extern "C" int cnf_ensemble_jvp_steps(cnf_handle h, int member, float* t_host, float* h_host, int cap) {
    if (!h || member < 0 || member >= h->ejvp_M || member >= h->ensv_M) return -1;
    const int natt = h->ensv_att[(size_t)member];
    if (natt < 0 || natt > h->ensv_tcap) return -1;
    if (h->ejvp_rows < 0) {
        int rows = 0;
        for (int v : h->ensv_att) if (v > rows && v <= h->ensv_tcap) rows = v;
        h->ejvp_host.resize((size_t)h->ejvp_M * 4 * (size_t)rows);
        if (rows > 0 &&
            (hipSetDevice(h->device) != hipSuccess ||
             hipMemcpy2D(h->ejvp_host.data(), (size_t)4 * rows * sizeof(float), h->ens_trace.data(), (size_t)4 * h->ensv_tcap * sizeof(float),
                         (size_t)4 * rows * sizeof(float), (size_t)h->ejvp_M, hipMemcpyDeviceToHost) != hipSuccess)) {
            (void)hipGetLastError();
            return -1;
        }
        h->ejvp_rows = rows;
    }
    const float* rows = h->ejvp_host.data() + (size_t)member * 4 * (size_t)h->ejvp_rows;
    int n = 0;
    for (int i = 0; i < natt; ++i) {
        if (rows[4 * (size_t)i + 3] == 0.f) continue;
        if (n < cap) {
            if (t_host) t_host[n] = rows[4 * (size_t)i];
            if (h_host) h_host[n] = rows[4 * (size_t)i + 1];
        }
        ++n;
    }
    return n;
}
