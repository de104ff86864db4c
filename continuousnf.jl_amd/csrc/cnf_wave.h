// k_solve_wave (cnf_wave.hip): the whole Tsit5 solve of a small two-layer network in one launch, one wave per 16-sample
// tile, registers only (BASELINE configs 1 and 2; the README / regression networks n_in -> 3 n_in -> n_in).
#pragma once
#include "cnf_mfma.h"

// The gradient path of small batches in the same launch (k_solve_wave<.., GRAD>): after the forward solve the waves run the
// discrete adjoint of the accepted steps and leave one partial of the flat gradient each (k_grad_reduce adds them).
#define WV_GCAP 1024                   // accepted steps a launch can differentiate (step sizes in LDS)
struct WaveGradArgs {
    float* traj = nullptr;             // [traj_cap][6 stages][waves][64 lanes][n_in tiles] x 4 floats: z rows of U_1 = u_n, U_2..U_6 as the lanes hold them
    int traj_cap = 0;
    float* hs_out = nullptr;           // [traj_cap] signed step sizes (the host's copy: cnf_grad_steps)
    float* gpart = nullptr;            // [waves][n_params]
    float* lam_out = nullptr;          // [B][n_in]  d loss / d z(t0)   (cnf_grad_x)
    float* rich = nullptr;             // TrainMode / VJP, small batches: [traj_cap][6][waves][64][3 (n_in + hidden tiles)] x 4 floats -- the
                                       // forward evaluations' intermediates, so that the backward pass does not form them again
    const float* ys = nullptr;         // conditional models: [B][n_cond] (the columns of W_1 behind z get their gradient from them)
    int n_params = 0;
    float lam1 = 0.f, lam2 = 0.f, lam3 = 0.f;
};
// floats of trajectory store per accepted step, waves of a launch
size_t wave_grad_traj_floats(const NetDesc& nd, int B);
int wave_grad_waves(int B);
size_t wave_grad_rich_floats(const NetDesc& nd, int B, bool train);   // per accepted step; 0: no such form
// two tanh layers (or one + the appended identity), n_in (+ n_cond of a conditional model) <= 16, at most 512 waves
// (B <= 8192); TrainMode:
// both compute modes; TestMode: the adjoint of the exact-trace solve (closed form of two-layer networks)
bool wave_grad_supported(const NetDesc& nd, int B, bool train = true);

// a two-layer network whose 16-row tile counts have an instantiation, B within the meeting buffer's reach
bool wave_solve_supported(const NetDesc& nd, bool train, int B);
// sv as for mfma_solve_persistent (Solve3Args: the initial state by value, the meeting buffer and its index base, the wait
// bounds; either sv.xs + the post-processing outputs, or sv.u0 / sv.u_out of a bare solve -- u_out null: the final columns
// go to U0).  CNF_ERR_UNSUPPORTED: not this network / batch.
// ens: M models in one launch (k_solve_wave<.., ENS>; cnf_loss_grad_many).  Every array of the other arguments is then the
// first member's, with the members' copies behind it: [M][n_params] parameters (p_stride), [M][B][..] data, probes, logpx,
// regs and final columns, [M] final states, 5 M sums, [M][traj_cap] step sizes, [M][tiles][n_params] partials, and
// sv.base_dev / sv.abort_flag one word per member; no mirror, no trace, no clock, no rich store.
// what the backward pass of an ensemble gradient pulls back: the built-in loss's cotangent, or a per-sample one (the CW forms of
// the kernel) of inference's four outputs, or of sampling's (z, logq)
// ... and the two PATH forms of those (cnf_inference_path_vjp, cnf_generate_path_vjp): the same launch also stores the flow at the
// caller's save times and injects a cotangent of those slices into the backward sweep (the adjoint of Tsit5's interpolant)
// ... and the BASE forms of the first two (cnf_ensemble_set_bases): the members have Gaussian bases of their own, so the terminal
// cotangent's z is P_m (z - mu_m).  They are kernels of their own, so that the forms without bases stay the code they were.
enum WaveCot { WC_LOSS = 0, WC_INFERENCE = 1, WC_SAMPLING = 2, WC_INFERENCE_PATH = 3, WC_SAMPLING_PATH = 4, WC_LOSS_BASE = 5,
               WC_INFERENCE_BASE = 6 };
inline WaveCot wave_cot_based(WaveCot c) { return c == WC_LOSS ? WC_LOSS_BASE : c == WC_INFERENCE ? WC_INFERENCE_BASE : c; }
inline bool wave_cot_sampling(WaveCot c) { return c == WC_SAMPLING || c == WC_SAMPLING_PATH; }
inline bool wave_cot_path(WaveCot c) { return c == WC_INFERENCE_PATH || c == WC_SAMPLING_PATH; }
struct WaveEnsLaunch {
    int M = 0;
    const float* t1 = nullptr;     // device, [M]: the members' own end times (null: sv.init.t1 for all)
    const float* t0 = nullptr;     // device, [M]: the members' own start times (plain forms and `sampling`; null: sv.init.t0 for all)
    size_t p_stride = 0;           // floats between two members' parameters
    size_t traj_stride = 0;        // ... trajectory stores (traj_cap x wave_grad_traj_floats)
    size_t part_stride = 0;        // ... meeting words, in floats (WV_ENS_PART_FLOATS)
    const float* cw = nullptr;     // device, [M][4][B]: per-sample cotangents of (logpx, E, n, A) -- with `grad`, the CW form
                                   // (cnf_inference_vjp_many) in place of the built-in loss's cotangent; null: the loss
    // with `grad`, the sampling CW form (cnf_generate_vjp_many): a bare solve sv.u0 -> U0 from t0 (no t1, no cw) whose backward
    // pass is seeded with cot_z [M][B][n_in] on the state rows and +cot_logq [M][B] on the dlogp row (either may be null, not both)
    bool sampling = false;
    const float* cot_z = nullptr;
    const float* cot_logq = nullptr;
    // heterogeneous members (cnf_ensemble_set_members), device, each null or: counts [M] batch sizes within [1, B] -- every array
    // stays [M][B]..; a member's columns behind its count are neither read nor written --, lams [M][3] (the loss form of the
    // gradient), tols [M][2] (abstol, reltol)
    const int* counts = nullptr;
    const float* lams = nullptr;
    const float* tols = nullptr;
    // the members' own bases (cnf_ensemble_set_bases), device, [M][WV_ENS_BASE_FLOATS] as k_ens_base_prepare leaves them; the
    // loss and inference-cotangent forms of the gradient only (their BASE kernels are launched: WC_LOSS_BASE, WC_INFERENCE_BASE):
    // the terminal cotangent becomes P_m (z - mu_m).  null: N(0, I), the kernels of before
    const float* bases = nullptr;
};
// A member's prepared base (cnf_ens_base.hip), floats: mu [16] | P = W' W [16][16] | W = inv(L) [16][16] | L [16][16], row-major,
// zero beyond n_in rows / columns | c = sum log W_ii - n_in / 2 log(2 pi) | the member's flag (an int: 0, or 1 = not a valid base)
#define WV_ENS_BASE_MU 0
#define WV_ENS_BASE_P 16
#define WV_ENS_BASE_W 272
#define WV_ENS_BASE_L 528
#define WV_ENS_BASE_C 784
#define WV_ENS_BASE_FLAG 785
#define WV_ENS_BASE_FLOATS 800
#define WV_ENS_PART_FLOATS 8192    // a member's meeting words: 2 x 1024 of the meetings + 2048 of the loss-sum partials, 8 bytes each
// the largest M a launch takes at batch B: workgroups the device holds at once / tiles (0: no ensemble form of this network
// or mode, or the one-launch solves are switched off)
// (cw: of that CW form -- each has its own kernels, hence its own register budget)
int wave_ens_capacity(const NetDesc& nd, bool train, int B, WaveCot cw = WC_LOSS);
// Without `grad`, `ens` launches the PLAIN ensemble form (cnf_inference_many / cnf_generate_many): either an inference (sv.xs,
// sv.logpx [M][B], sv.regs [M][3][B], sv.sums5 [5 M]) or a bare solve (sv.u0 -> sv.u_out, [M][B][D] each); sv.trace, when
// set, is [M][sv.trace_cap][4].  Its capacity: workgroups of one wave the device holds at once / tiles, at most 512 tiles.
// path: of the plain form that also stores the members' paths (cnf_inference_path_many, cnf_generate_path_many; its own kernels)
int wave_ens_eval_capacity(const NetDesc& nd, bool train, int B, bool path = false);
// The path of a plain solve in the same launch (k_solve_wave<.., PATH>; cnf_solve_path): every accepted step evaluates Tsit5's
// interpolant at the save times it serves, from the k_1 .. k_7 it holds in registers, and stores those columns.
struct WavePathArgs {
    const float* times = nullptr;      // device, [K]: the save times, monotone along the direction of integration, inside the span
    int K = 0;
    float* out = nullptr;              // [K][B][D]: slice k in the layout of u_out
    float* steps = nullptr;            // [steps_cap][2]: (t_n, signed h_n) of accepted step n (steps beyond the capacity are not filed)
    int steps_cap = 0;
    // the PATH forms of the ensemble gradient (WC_INFERENCE_PATH, WC_SAMPLING_PATH) only: the cotangent of the slices, in the
    // layout of `out` (null: nothing is injected); there `out` and `steps` may be null too (nothing is stored)
    const float* cot = nullptr;
    // ENS forms (M members): `times` is [M][K] (one set for all members: laid out M times by the caller), `out` / `cot` are
    // [M][K][B][D] and `steps` is [M][steps_cap][2]
};
// `path`: the PATH form -- a plain solve (no grad, no ens) of one tile per workgroup, whatever the batch (B <= 8192), on the
// tanh networks with one input tile; CNF_ERR_UNSUPPORTED for everything else (the caller takes the streamed path).
// `path` with `grad` and `ens`: the PATH form of the per-sample-cotangent gradient -- ens->cw / ens->cot_z / ens->cot_logq
// may then all be null (no terminal cotangent).  `path` with `ens` alone: the plain ensemble form with the members' paths.
// LAYOUT CONTRACT of `path` with `ens`: path->times holds ens->M x path->K floats, member m's set at [m K, m K + K) -- also when
// all members share one set (the caller lays it out M times: cnf_abi_ens.hip's ens_path_args is the one caller and does) --,
// path->out / path->cot hold M slabs [K][B][D] and path->steps M x steps_cap pairs.  The launch cannot see the sizes of these
// device arrays: a [K] array with M > 1 would be read past its end.
cnf_status wave_solve_launch(const NetDesc& nd, bool train, const float* d_params, const float* cond, int cbs, StepState* st_out,
                             float* U0, const float* eps, int B, hipStream_t s, void* mirror, unsigned seq, const Solve3Args& sv,
                             const WaveGradArgs* grad = nullptr, const WaveEnsLaunch* ens = nullptr, const WavePathArgs* path = nullptr);
