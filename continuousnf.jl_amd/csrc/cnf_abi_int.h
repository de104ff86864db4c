// Private to the C ABI sources (cnf_abi.hip, cnf_abi_ens.hip, cnf_abi_jvp.hip): the handle,
// and what one of those files uses of another -- nothing else.  A helper only one file calls is a `static` of that file; a type
// only one file uses sits in that file's anonymous namespace.  Everything below the handle is namespace cnfabi with hidden
// visibility: none of it is exported from libcnfhip.so.  The helpers defined in this header are all `static inline`.
#pragma once
#include "../../include/cnfhip.h"
#include "cnf_dev.h"
#include "cnf_kernels.h"
#include "cnf_mfma.h"
#include "cnf_grad.h"
#include "cnf_trace.h"
#include "cnf_mirror.h"
#include "cnf_buf.h"
#include "cnf_record.h"
#include "cnf_solve_plan.h"
#include "cnf_wave.h"
#include "cnf_tangent.h"
#include "cnf_bcast.h"
#include "cnf_gradt.h"
#include "cnf_condgrad.h"
#include "cnf_adj3b.h"
#include "cnf_step3.h"
#include "cnf_dist.h"
#include "cnf_basegrad.h"
#include "cnf_ens_base.h"
#include <immintrin.h>
#include <algorithm>
#include <sched.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <new>
#include <mutex>
#include <deque>
#include <string>
#include <vector>

// what the handle owns on the device and in pinned host memory (cnf_buf.h)
struct DevAlloc {
    static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
};
template <unsigned Flags>
struct HostAlloc {
    static int alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, Flags); }
    static void free(void* p) { (void)hipHostFree(p); }
};
template <class T> using DevBuf = CnfBuf<T, DevAlloc>;
template <class T> using PinnedBuf = CnfBuf<T, HostAlloc<hipHostMallocDefault>>;

// the words of d_sums: 8 floats of sums, then the device tickets (zero between launches) and the kernel clock words
enum { SUMS_NORM_TICKET = 8, SUMS_POST_TICKET = 9, SUMS_MEET_BASE = 10, SUMS_ABORT = 11, SUMS_CLOCK = 12 /* 3 x 64 bit */, SUMS_WORDS = 24 };

struct cnf_ctx {
    NetDesc nd{};
    float lam[3]{};
    int device = 0;
    size_t n_params = 0;
    DevBuf<float> d_params;
    bool have_params = false;
    MfmaPlan mfma{};              // packed weights etc. for the MFMA path (cnf_mfma.hip)

    // scratch, sized for cap_B samples
    size_t cap_B = 0;
    DevBuf<float> arena;          // one allocation carved into the buffers below (set by ensure_capacity, cleared with it)
    float* ws = nullptr;
    float* U[2] = {nullptr, nullptr};
    float* K1[2] = {nullptr, nullptr};
    float* Ks[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    DevBuf<float> d_cond;         // conditional models: per-sample first-layer bias [cond_B][cbs]
    int cond_B = 0, cbs = 0;
    float* tmp_logpx = nullptr;
    float* tmp_regs = nullptr;
    float* post_part = nullptr;   // loss-sum partials of the post-processing kernel: 4 floats per 64 columns
    // inferences submitted and not yet collected (cnf_inference_submit / cnf_inference_collect): the one-launch solve is
    // enqueued and the call returns; the outcome is read later from the launch's own slot of the host mirror
    struct Submitted {
        bool launched = false;    // a one-launch solve is in flight (else: the call completed synchronously; status / stats say how)
        unsigned seq = 0;         // its launch index = the tag it publishes its final state with
        int slot = 0;             // ... into this slot of the host mirror
        bool hairer = false;
        bool grad = false;        // a submitted GRADIENT (cnf_loss_grad_submit): nothing is run again if it gave up
        int mode = 0, B = 0, k = 0;
        const float *xs = nullptr, *eps = nullptr;
        float *logpx = nullptr, *regs = nullptr, *sums5 = nullptr;
        cnf_solve_opts opts{};
        hipStream_t st = nullptr;
        cnf_solve_stats stats{};
        cnf_status status = CNF_OK;
    };
    std::deque<Submitted> submitted;
    unsigned one_launch_count = 0; // one-launch solves so far: they take the mirror slots 1, 2, 3 in turn (slot 0: the streamed solves)
    bool submitting = false;      // inside cnf_inference_submit: a one-launch solve is recorded in `submitted`, not waited for
    bool sub_taken = false;       //   ... and this call was
    bool collecting = false;      // inside submit / collect: check_call does not drain the queue
    bool no_persist = false;      // the fallback of a collected launch: straight to the streamed driver
    bool time_kernel = false;     // cnf_solve_kernel_time: the one-launch solve kernel adds up its own durations
    int fallbacks = 0;            // one-launch solves that ran out of a wait and were run again on the streamed driver
    int wait_us = 0, poll_limit = 0;   // cnf_set_solve_wait (0: the process defaults)
    float* step_trace = nullptr;  // cnf_set_step_trace: caller-owned device buffer, 4 floats per step attempt
    int step_trace_cap = 0;
    DevBuf<float> partials;       // 8 * MAX_PARTIALS floats
    StepState* last_state = nullptr; // device slot holding the state at the end of the last solve
    DevBuf<StepState> d_state;      // two slots: [0] canonical, [1] ping-pong partner of the fused MFMA path
    PinnedBuf<StepState> h_state; // pinned, two slots for pipelined polling + one init slot (init_state / loss_sums_host)
    // streamed solve: the step kernel mirrors the state into pinned, host-coherent memory after every
    // controller run as tagged granules (cnf_mirror.h); the host polls them
    typedef CnfMirrorT<StepState> HostMirror;
    CnfBuf<HostMirror, HostAlloc<hipHostMallocCoherent | hipHostMallocMapped>> h_mirror;   // host address
    HostMirror* d_mirror = nullptr;        // the same memory as the device sees it
    unsigned mirror_base = 1;              // launch indices are monotonic over the handle's life: late launches of
                                           // an earlier solve can never look like news of the current one
    // lock-step sharded solves: host callback summing 3 floats over the shards (null: off)
    cnf_shard_reduce_fn shard_reduce = nullptr;
    void* shard_user = nullptr;
    cnf_comm shard_comm = nullptr;         // ... or an RCCL communicator: reduced on the stream, no host round trip
    // gradient path (cnf_loss_grad): transposed weights, per-step trajectory, adjoint scratch
    DevBuf<float> d_PT;
    DevBuf<float> d_adj_img;      // padded forward/reverse weight images of the MFMA pullback kernel
    bool pt_valid = false;
    bool img_valid = false;       // d_adj_img holds the images of the current parameters
    DevBuf<float> d_bimg;         // k_solve_bcast's images (cnf_bcast.hip), packed on first use after a parameter change
    DevBuf<float> d_gt;           // k_adj_test: one partial of the flat gradient and a scratch per workgroup (cnf_gradt.hip)
    DevBuf<float> d_bstore;       // ... and the store of its tiles' Runge-Kutta rows when a workgroup carries several (bcast_store_floats)
    bool bimg_valid = false;
    DevBuf<float> traj;                // trajectory store: traj_cap slots of 6 (n_in + 3) grad_cap_B floats (u_n, U_2..U_6)
    DevBuf<float> traj_hs;             // device: signed size of accepted step n (written by the step kernel)
    int traj_cap = 0;
    size_t grad_cap_B = 0;
    int grad_fsteps = 1;          // steps whose factor arrays are kept before one batch contraction
    DevBuf<float> grad_arena;     // carved into the g_ pointers below (set by ensure_grad_capacity, cleared with it)
    float* g_US[5] = {};          // stage states 2..6
    float* g_W[6] = {};           // zbar per stage
    float* g_lam = nullptr;
    float *g_HS = nullptr, *g_TS = nullptr, *g_AB = nullptr, *g_PB = nullptr;
    DevBuf<float> d_park;         // parked state of the two-launch headline pullback (adj3b_park_floats)
    DevBuf<float> d_sc;           // scratch rows of the two-launch MFMA pullback (adj_mfma_scratch_floats)
    DevBuf<AdjStepArgs> d_steps;         // ... and the arguments of the steps of its runs: device array and pinned staging
    PinnedBuf<AdjStepArgs> h_steps;
    float* g_part = nullptr;      // GRAD_MAX_KSPLIT x n_params
    NetDesc nd_wave{};            // what the wave kernels see: nd, or a one-layer tanh network with an identity layer appended
    DevBuf<float> wg_traj;        // k_solve_wave<GRAD>: z rows of u_n per accepted step, as the lanes hold them; + WV_GCAP step sizes
    float* g_grad = nullptr;      // n_params (host-pointer variant)
    std::vector<float> last_hs;   // signed step sizes of the last cnf_loss_grad solve
    // What the last calls left in the trajectory store, g_US[1], last_hs, g_lam and d_gy for cnf_inference_pullback,
    // cnf_generate_pullback, cnf_base_logpdf_pullback, cnf_grad_x and cnf_grad_ys -- and which events end which piece of it:
    // cnf_record.h.  Every change of it below is one of that type's named transitions.
    CnfRecord rec;
    DevBuf<float> d_gz0;          // cnf_generate_record: the handle's copy of the base draw z0 [B][n_in] (read again by the pullback)
    DevBuf<float> d_cw;           // [3][B] per-sample cotangents of the scalar rows, packed by k_vjp_cotangent
    // cnf_set_grad_ys / cnf_grad_ys: the gradient w.r.t. the conditioning inputs (cnf_condgrad.hip; k_adj_test's own in TestMode)
    bool grad_ys = false;         // the switch: gradient calls also accumulate d / d ys
    DevBuf<float> d_gy;           // [B][dims[1]] row sums of abar_1, then [B][n_cond] the result
    DevBuf<float> d_ys;           // conditional models: copy of ys (n_cond x cond_B), kept for the weight gradient
    DevBuf<float> stage;          // device staging area of the *_host entry points, owned by the handle, grown on demand:
                                  //   no allocation per call, nothing to free on an error path
    DevBuf<float> d_sums;         // SUMS_WORDS floats
    BaseDist bd{};                // cnf_set_basedist: kind 0 = the default N(0, I), nothing of cnf_dist.hip is launched
    DevBuf<float> d_bd;           //   its arrays (mean | whiten | chol | prec), one allocation
    // cnf_base_logpdf_pullback / cnf_base_sample_pullback (cnf_basegrad.hip): tickets, result, partials and whitened rows; grown
    // on demand, so a handle that never asks for the base's gradient never allocates it
    DevBuf<float> d_bg;
    PinnedBuf<float> h_sums;      // pinned, 4 floats
    // cnf_loss_grad_many (k_solve_wave<.., ENS>): what one model's call has once, per member; sized for (M, B), grow-only
    DevBuf<float> ens_traj;       // [M][cap] trajectory rows
    DevBuf<float> ens_hs;         // [M][cap] signed step sizes (read back on demand: cnf_ensemble_steps)
    DevBuf<float> ens_gpart;      // [M][tiles][n_params] the waves' partials
    DevBuf<float> ens_cols;       // [M][B][D] final columns | [M][B] logpx | [M][3][B] regs | [M][B][n_in] d loss / d z(t0)
    DevBuf<float> ens_part;       // [M] meeting words (WV_ENS_PART_FLOATS each), zero when allocated
    DevBuf<unsigned> ens_words;   // [M] meeting bases | [M] abort words: set by every call in front of its launch
    DevBuf<float> ens_fin;        // [M] final StepStates | [5 M] loss sums: one copy to the host per call
    PinnedBuf<float> ens_hfin;    //   ... its landing place, and behind it [M] end times on their way to the device
    DevBuf<float> ens_t1;
    unsigned ens_base = 0;        // meeting indices the ensemble launches so far may have used (tags go on from there)
    int ens_M = 0, ens_cap = 0;   // the last call: members, step slots per member
    std::vector<int> ens_nacc;    //   accepted steps per member (-1: the member gave up)
    // cnf_inference_many / cnf_generate_many share the meeting words, bases, final states and columns above; their own:
    DevBuf<float> ens_trace;      // [M][trace_cap][4] the members' step attempts (cnf_ensemble_eval_steps)
    int ensv_M = 0, ensv_tcap = 0;   // the last call that kept a trace: members, rows per member
    std::vector<int> ensv_att;    //   attempts per member (-1: the member gave up)
    // heterogeneous members (include/cnfhip_ensemble_hetero.h): what cnf_ensemble_set_members left for the NEXT ensemble call, which
    // takes it away at its entry (EnsHet) whatever becomes of that call; and that call's device copy with its pinned staging
    int het_M = 0;                //   0: nothing pending
    std::vector<int> het_counts;  //   [M], or empty: every member at the call's B
    std::vector<float> het_lams;  //   [M][3], or empty: the handle's
    std::vector<float> het_tols;  //   [M][2] (abstol, reltol), or empty: the options'
    DevBuf<float> ens_het;        // [M] counts (ints) | [M][3] lambdas | [M][2] tolerances
    PinnedBuf<float> ens_hhet;
    // the members' own bases (include/cnfhip_ensemble_base.h): what cnf_ensemble_set_bases prepared for the NEXT ensemble call
    // (`pend`), which takes it away at its entry; and the bases of the last call that ran with some (`last`), with what
    // cnf_ensemble_base_logpdf_pullback needs of that call.  Two buffers that change places: preparing the next call's bases
    // does not touch the last call's.
    DevBuf<float> ens_bases_pend, ens_bases_last;   // [M][WV_ENS_BASE_FLOATS]
    int base_M = 0, base_kind = 0;                  //   pending: members (0: nothing) and kind
    int lbase_M = 0, lbase_kind = 0, lbase_B = 0, lbase_stride = 0;   // the last call: members, kind, B, floats per column of ...
    size_t lbase_off = 0;                           //   ... the columns the pullback reads, at this offset of ens_cols
    bool lbase_counts = false;                      //   it had counts of its own: still in ens_het, which only a later ensemble call
                                                    //   overwrites -- and that call ends this state (ens_take_members)
    DevBuf<int> ens_bcounts;                        // [M] the members' flags (k_ens_base_flags), gathered for ...
    PinnedBuf<int> ens_hbflags;                     // ... their [M] landing place on the host
    // cnf_solve_path (include/cnfhip_path.h): the save times on the device and the step pairs the in-launch route files (both
    // allocated on first use), and the accepted steps of the last call on either route (cnf_path_steps)
    DevBuf<float> d_saveat;
    DevBuf<float> d_path_steps;   // [PATH_STEPS_CAP][2]
    std::vector<float> path_t, path_h;
    bool path_valid = false;
    // cnf_inference_path_vjp / cnf_generate_path_vjp (include/cnfhip_path_vjp.h) share the two device buffers above; the accepted
    // steps of the last such call (cnf_path_vjp_steps)
    std::vector<float> pvjp_t, pvjp_h;
    bool pvjp_valid = false;
    // the four calls of include/cnfhip_ensemble_path.h: the members' step pairs, a buffer of their own (the single-model calls'
    // steps above are not theirs to overwrite), read back on demand (cnf_ensemble_path_steps)
    DevBuf<float> ens_psteps;     // [M][epath_cap][2]
    int epath_M = 0, epath_cap = 0;  // the last such call: members, step pairs a member files
    std::vector<int> epath_nacc;  //   accepted steps per member (-1: the member was not CNF_OK)
    std::vector<float> epath_host;   // [M][epath_rows][2]: the pairs on the host, fetched by ONE strided copy when first asked for
    int epath_rows = -1;          //   pairs per member in epath_host (-1: not fetched yet)
    // cnf_inference_jvp_many / cnf_generate_jvp_many (include/cnfhip_ensemble_jvp.h): the attempts are ens_trace's
    int ejvp_M = 0;               // members of the last such call (0: none, or the trace has been written over since)
    std::vector<float> ejvp_host; // [M][ejvp_rows][4]: the members' attempts on the host, fetched by ONE strided copy when first asked for
    int ejvp_rows = -1;           //   rows per member in ejvp_host (-1: not fetched yet)
    std::vector<float> saveat_rep;   // one set of save times laid out M times, on its way to the device
    // cnf_inference_jvp / cnf_generate_jvp (include/cnfhip_jvp.h): SolveCall's `jvp` hook says what the solve does for such a call
    DevBuf<float> jvp_trace;      // [trace_cap][4]: (t, signed h, EEst, accepted) per attempt
    DevBuf<float> jvp_buf;        // the primal outputs until the call is known to succeed
    std::vector<float> jvp_t, jvp_h;   // the accepted steps of the last such call (cnf_jvp_steps)
    bool jvp_valid = false;
    std::string err;
};

#pragma GCC visibility push(hidden)
namespace cnfabi {

static const int PATH_STEPS_CAP = 16384;
// ... and per member of the ensemble path calls: the plain ones | the vjp ones (WV_GCAP: what a launch differentiates)
static const int ENS_PATH_STEPS_CAP = 4096, ENS_PATH_VJP_STEPS_CAP = 1024;

static const int MAX_PARTIALS = 1024;
// One cnf_inference_jvp in flight, SolveCall's `jvp` hook beside `rec` and `path`: the solve then files its step attempts in
// the handle's jvp_trace (not in the caller's cnf_set_step_trace buffer), takes the wave kernel as its only one-launch route,
// enqueues the tangent launch right behind that launch, and on the one-attempt-at-a-time route files the accepted steps here
struct JvpCall {
    TangentArgs ta{};             // everything of the tangent launch but where the solve leaves its state and its attempts
    bool train = false;
    int trace_cap = 0;
    bool enqueued = false;        // the tangent launch went out behind a one-launch solve
    bool host_steps = false;      // the solve ran one attempt at a time: its accepted steps are in t, h
    std::vector<float> t, h;
};

#define HIPCHK(h, call)                                                                  \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            char buf_[512];                                                              \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call,                  \
                     hipGetErrorString(e_), __FILE__, __LINE__);                         \
            if (h) (h)->err = buf_;                                                      \
            return CNF_ERR_HIP;                                                          \
        }                                                                                \
    } while (0)

static inline cnf_status fail(cnf_handle h, cnf_status s, const char* msg) {
    if (h) h->err = msg;
    return s;
}

// grow-only reserve of one of the handle's buffers (n elements); an allocator's refusal is the call's HIP error
#define RESERVE(h, buf, n) HIPCHK(h, (hipError_t)(buf).reserve(n))

template <class T>
static inline T* sums_word(cnf_handle h, int word) { return reinterpret_cast<T*>(h->d_sums.data() + word); }
// h_state[2] serves twice: the initial state of a solve, and -- free again once the solve is enqueued -- the pinned landing
// place of the five loss sums
static inline StepState* init_state(cnf_handle h) { return &h->h_state[2]; }
static inline float* loss_sums_host(cnf_handle h) { return reinterpret_cast<float*>(&h->h_state[2]); }
// the integrator's buffers into the argument struct of a kernel that works on them (RhsArgs, NormArgs, TraceArgs)
template <class Args>
static inline void set_rk_buffers(cnf_handle h, Args& a) {
    for (int i = 0; i < 2; ++i) { a.U[i] = h->U[i]; a.K1[i] = h->K1[i]; }
    for (int i = 0; i < 5; ++i) a.Ks[i] = h->Ks[i];
}

static inline int rows_of(const cnf_ctx* h, int mode) {
    return h->nd.n_in + 1 + (mode == CNF_MODE_TRAIN ? 2 : 0);
}

// Trajectory store of the gradient path: state after every accepted step + the step sizes.
struct Recorder {
    std::vector<float> hs;        // signed step of accepted step n (u_n -> u_{n+1})
    int n = 0;                    // accepted steps recorded; slot n holds u_n and the stage states of step n
    bool overflow = false;        // the solve took more steps than the store holds: grow it and solve again
    // the whole gradient in the launch of the solve (k_solve_wave<GRAD>): where it keeps its trajectory and leaves its results;
    // wg_done: it ran (hs holds the step sizes); wg_failed: it could not (not this network, a wait ran out, too many steps)
    const WaveGradArgs* wg = nullptr;
    bool wg_done = false, wg_failed = false, wg_submitted = false;     // wg_submitted: launched and left in flight (cnf_loss_grad_submit)
};

// Post-processing (and loss sums) the caller wants behind the solve.  The streamed driver enqueues it itself, right behind
// the attempt its step estimate says is the last one -- the kernel checks `done` and does nothing if the estimate was
// short -- so that it does not wait for the host to notice the end of the solve; `launched` tells the caller it ran.
struct PostHook {
    float* logpx; float* regs; float* sums5;
    const float* xs = nullptr;     // also assemble u0 from these columns, in the launch that sets the initial state
    bool launched = false;
};

// ---- what cnf_abi_ens.hip and cnf_abi_jvp.hip use of cnf_abi.hip; all of it is defined there
// One-launch solves of this process: one at a time (two would each hold CUs the other is waiting for), except that
// submitted launches may queue up behind each other on ONE stream.  ONE definition for the whole library.
extern std::mutex g_persist_mu;
extern int g_submitted_inflight;                   // (both under g_persist_mu)
extern hipStream_t g_submitted_stream;
// the statistics of a solve that ended in the state `fin`
void fill_stats(cnf_solve_stats* stats, const StepState& fin, int nf, int kernel_used, int launches);
// the bounds of a wait inside a one-launch solve of this handle (cnf_set_solve_wait; CNF_SOLVE_WAIT_US, CNF_SOLVE_POLL_LIMIT)
void set_wait_bounds(cnf_handle h, Solve3Args& sv);
// what every solve asks of its options
cnf_status check_solve_opts(cnf_handle h, const cnf_solve_opts* opts);
// the state a solve starts from; n_partials: the error partials (blocks, tiles) that meet per attempt
StepState init_step_state(const cnf_solve_opts* opts, int n_partials);
// What is wrong with the save times of a path call, or null.  Looks at no handle.
const char* saveat_error(const cnf_solve_opts* opts, const float* saveat_host, int K);
// The host step readers: the accepted steps (t_n, h_n) a call left on the host; the number there is, or -1 when there is none
int copy_steps(bool valid, const std::vector<float>& t, const std::vector<float>& hh, float* t_host, float* h_host, int cap);
cnf_status inference_impl(cnf_handle h, int mode, const float* xs, const float* eps,
                          float* logpx, float* regs, float* u_final, float* sums5, int B,
                          const cnf_solve_opts* opts, cnf_solve_stats* stats, void* stream, JvpCall* jvp = nullptr);
// The oldest submitted inference, completed and taken off the queue.
cnf_status collect_one(cnf_handle h, cnf_solve_stats* stats);
// (lam: the handle's regularisers, or a heterogeneous ensemble member's own)
cnf_status loss_from_sums_lam(cnf_handle h, int mode, const float* sums5, const float* lam, float* loss);
// Step slots of an in-launch gradient's trajectory store of `per_step` floats per accepted step; *fit: how many such stores fit
int traj_step_slots(size_t per_step, size_t* fit = nullptr);
// What the gradient entry points begin with: the call's checks in their one order, then room for B samples
cnf_status grad_prologue(cnf_handle h, int mode, int B, bool ptrs_ok, const char* empty_batch, bool width, hipStream_t st,
                         bool cw = false, bool gz0 = false);
// The RECORDED solve of the gradient entry points, from u0: stage states in the trajectory store, the final state in g_US[1]
cnf_status record_solve(cnf_handle h, int mode, const float* u0, const float* eps, int B, const cnf_solve_opts* opts, Recorder& rec,
                        cnf_solve_stats& sst, void* stream, PostHook* ph = nullptr);

}  // namespace cnfabi
#pragma GCC visibility pop
