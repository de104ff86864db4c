// k_tangent_wave (cnf_tangent.hip): the forward-mode derivative (tangent, JVP) of a finished solve of a small two-layer
// network -- R directions of (parameters, initial columns) pushed through the accepted Tsit5 steps, one wave per (16-column
// tile, direction), registers only, no waits (cnf_inference_jvp / cnf_generate_jvp, include/cnfhip_jvp.h).
#pragma once
#include "cnf_mfma.h"

#define TG_MAX_R 65535                 // directions of one launch (the grid's second axis)
struct TangentArgs {
    NetDesc nd;                        // the wave kernels' view of the network (an appended identity layer included)
    const float* P;                    // flat parameters
    const float* dP = nullptr;         // null, or [R][n_params]: the directions' parameter parts (an appended identity layer has none)
    int n_params = 0;                  // floats of one of them
    const float* eps = nullptr;        // TrainMode: [B][n_in]
    int B = 0, R = 0;
    // inference: the data columns [B][nvars] and their directions [R][B][nvars];  sampling: z0 [B][n_in] and [R][B][n_in]
    int sampling = 0;
    const float* x = nullptr;
    const float* dX = nullptr;         // null: zero
    // where the solve launch left its outcome: its final state (the guard: an aborted, unfinished or non-finite solve makes
    // the launch write nothing) and the attempts it made, rows (t, signed h, EEst, accepted)
    const StepState* st = nullptr;
    const float* trace = nullptr;
    int trace_cap = 0;                 // more attempts than this: nothing is written either
    int n_rows = -1;                   // >= 0: the rows of `trace` are this many (a route that filed them from the host), not st's count
    // inference: [R][4][B], rows (d logpx, d E, d n, d A);  sampling: d z [R][B][n_in] and d logq [R][B]
    float* out = nullptr;
    float* out_logq = nullptr;
};
// The ensemble form (ENS; cnf_inference_jvp_many / cnf_generate_jvp_many): M members in one launch, the grid (tiles, R, M).  The
// arrays of TangentArgs are then the members' one behind the other: P at p_stride, dP [M][R][n_params], eps [M][B][n_in], x at
// x_stride ([M][B][rows]; 0: one data set read by all), dX [M][R][B][rows], st + m, trace + m 4 trace_cap, out [M][R][4][B]
// (sampling: [M][R][B][n_in] and out_logq [M][R][B]).  n_rows stays -1: every member replays its own StepState's attempts.
#define TG_MAX_M 65535                 // members of one launch (the grid's third axis)
struct TangentEns {
    int M = 0;
    size_t p_stride = 0, x_stride = 0; // floats, the caller's
    size_t dp_stride = 0, eps_stride = 0, dx_stride = 0, out_stride = 0, logq_stride = 0;     // the dense ones: tangent_launch_many fills them in
    const int* counts = nullptr;       // null, or [M] (device): a member's own batch size within [1, B]
};
// two layers, tanh then tanh or identity, n_in <= 16, at most 64 hidden units (16 with the identity), no conditioning
bool tangent_supported(const NetDesc& nd);
// CNF_ERR_UNSUPPORTED: not this network;  CNF_ERR_BAD_ARG: R outside [1, TG_MAX_R], B < 1, a null array
cnf_status tangent_launch(const TangentArgs& a, bool train, hipStream_t s);
// ... and M < 1 or M > TG_MAX_M, n_rows >= 0
cnf_status tangent_launch_many(const TangentArgs& a, const TangentEns& en, bool train, hipStream_t s);
