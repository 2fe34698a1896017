// bn_coef.h -- BatchNorm1d's per-column finalisation, once for every kernel that does it: the
// one-block-per-channel kernels (fused_support.hip, fused_readout.hip), the width-N kernels of the layered path
// (elementwise.hip) and the last workgroup's tail of the tile kernels (bn_tail.h).  Each expression is
// written as the earlier copies had it, so contraction into FMAs -- and with it every bit of the
// coefficient blocks -- is what it was.
#pragma once
#include "common.h"

namespace {

// Forward, column c: mean and biased variance of the batch from S1 = sum y and S2 = sum y^2 over
// `count` rows, and the running statistics updated (training); or mean and variance read from the
// running statistics (eval).  Writes the block [a | b | mean | invstd] (column stride ld: 64 or N) of
// X = a*y + b.  mean_off: the constant the statistics were taken without (the centred layer 0, 0
// elsewhere): the block describes y - mean_off, the running mean is that of y itself.
__device__ __forceinline__ void bn_fwd_coef(bool training, double S1, double S2, double count,
                                            const float* gamma, const float* beta, float* rmean,
                                            float* rvar, float momentum, float eps, float mean_off,
                                            float* coef, int ld, int c) {
  float mean, var;
  if (training) {
    const double m = S1 / count;
    double v = S2 / count - m * m;
    if (v < 0.0) v = 0.0;
    mean = (float)m;
    var = (float)v;
    // (rounded to float in each arm -- the same value as rounding the selected double -- so that the
    // tile kernels' tails compile to the instructions they had with their own copy)
    const float unbiased = count > 1.0 ? (float)(v * count / (count - 1.0)) : var;
    const float mean_y = (float)(m + (double)mean_off);
    rmean[c] = (1.0f - momentum) * rmean[c] + momentum * (mean_off != 0.f ? mean_y : mean);
    rvar[c] = (1.0f - momentum) * rvar[c] + momentum * unbiased;
  } else {
    mean = (float)((double)rmean[c] - (double)mean_off);
    var = rvar[c];
  }
  const float invstd = 1.0f / sqrtf(var + eps);
  const float a = gamma[c] * invstd;
  coef[c] = a;
  coef[ld + c] = beta[c] - mean * a;
  coef[2 * ld + c] = mean;
  coef[3 * ld + c] = invstd;
}

// Backward, column c, from S1 = sum dz and S2 = sum dz * xhat over `count` rows: dbeta, dgamma and the
// coefficients [c1 | c2] (column stride ld) of dY = a * (dz - c1 - xhat * c2).  zero_coef: c1 = c2 = 0
// (eval-mode BatchNorm's backward is a fixed affine map).
__device__ __forceinline__ void bn_bwd_coef(double S1, double S2, double count, int zero_coef,
                                            float* dgamma, float* dbeta, float* bwc, int ld, int c) {
  dbeta[c] = (float)S1;
  dgamma[c] = (float)S2;
  bwc[c] = zero_coef ? 0.f : (float)(S1 / count);
  bwc[ld + c] = zero_coef ? 0.f : (float)(S2 / count);
}

}  // namespace
