// The gradient w.r.t. the conditioning inputs ys of a conditional model on the recorded TrainMode routes (cnf_condgrad.hip),
// used by the C ABI beside the weight-gradient contraction.
#pragma once
#include "cnf_grad.h"

// S1[b][j] (+)= sum over slot < nslots of AB[(slot B + b) sum_out + out_off[0] + j],  j < dims[1]: the rows of abar_1 the
// pullback kernels filed for one run of steps, summed per sample.  first != 0: S1 is stored, else added to.
hipError_t launch_cond_rowsum(const NetDesc& nd, const GradLayout& g, const AdjMfmaLayout& m, const float* AB, float* S1, int B,
                              int nslots, int first, hipStream_t s);
// gy[b][c] = sum_j W_1[j][n_in + c] S1[b][j],  c < n_cond  (P: flat parameters, Lux layout)
hipError_t launch_cond_project(const NetDesc& nd, const float* P, const float* S1, float* gy, int B, hipStream_t s);
