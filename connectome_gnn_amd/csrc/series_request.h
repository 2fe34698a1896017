// series_request.h -- the host side that the time-series entry points share (filter.hip, timeseries.hip, shrinkage.hip,
// confounds.hip, interpolate.hip, butterworth.hip): the bound on the frames of a run, the units of a
// window request, the component list of a band, and the byte count of an array of floats.  Host code only; every check
// is CGNN_OK or CGNN_EINVAL and touches no device.
#pragma once
#include "common.h"

// The longest run: frame indices a step past T stay inside an int, and S * T * 256 * 4 below 2^63 for S < 2^31.
constexpr int32_t CGNN_MAX_FRAMES = 1 << 30;

// The units of a request: unit u = s * W + w is subject s, frames [w * st, w * st + L); W = 1 and L = st = T without
// a window (window == 0).  U = S * W.
struct cgnn_units {
  int32_t L, st;
  int64_t W, U;
};

// (CGNN_OK, the units) of a valid (T, window, stride) for a cohort that cgnn_check_cohort has passed: T >= 2, a window
// in [2, T] with a stride >= 1, and the row index U * n of the units inside an int32.
inline int cgnn_check_units(int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride, cgnn_units* u) {
  if (T < 2 || (window != 0 && (window < 2 || window > T || stride < 1))) return CGNN_EINVAL;
  u->L = window ? window : T;
  u->st = window ? stride : T;
  u->W = (T - u->L) / u->st + 1;
  u->U = S * u->W;
  return u->U * n >= ((int64_t)1 << 31) ? CGNN_EINVAL : CGNN_OK;
}

// The DCT-II components of a T-frame run that a kernel takes by value, padded with zeros.
struct cgnn_components {
  int32_t k[CGNN_FILTER_MAX_COMPONENTS];
};

// (CGNN_OK, the padded list) of K components (0 <= K <= CGNN_FILTER_MAX_COMPONENTS, the caller's check) that lie in
// 1 .. T - 1 and ascend strictly.
inline int cgnn_check_components(const int32_t* comps, int32_t K, int32_t T, cgnn_components* list) {
  if (K > 0 && !comps) return CGNN_EINVAL;
  for (int i = 0; i < K; ++i) {
    if (comps[i] < 1 || comps[i] > T - 1 || (i > 0 && comps[i] <= comps[i - 1])) return CGNN_EINVAL;
    list->k[i] = comps[i];
  }
  for (int i = K; i < CGNN_FILTER_MAX_COMPONENTS; ++i) list->k[i] = 0;
  return CGNN_OK;
}

// Whether `bytes` (>= 0) hold `rows` rows of `width` (> 0) floats.  rows * width * 4 could wrap 64 bits (an output
// [S T][n] has S * n < 2^31 rows of T < 2^31), so the byte count is compared by division.
inline bool cgnn_holds_floats(int64_t bytes, int64_t rows, int64_t width) {
  return bytes / (int64_t)sizeof(float) / width >= rows;
}
