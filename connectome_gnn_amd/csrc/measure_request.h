// measure_request.h -- the host side that the cohort entry points share (measures.hip, paths.hip, wpaths.hip,
// modules.hip, pagerank.hip, core.hip, knn.hip, mst.hip): the columns a kernel writes, the check of a
// request, of the cohort's size, of its buffers and of an output that may be the input, and the two rules of a
// one-workgroup-per-subject launch on dynamic LDS.  Host code only; every check is CGNN_OK or CGNN_EINVAL
// (cgnn_check_cohort_within: or CGNN_EUNSUPPORTED) and touches no device.
#pragma once
#include "common.h"

// Where a kernel writes: measure m of row r goes to x[r * ldx + col[m]]; col[m] = -1 when m is not asked for.
template <int N>
struct cgnn_columns {
  int32_t col[N];
  int32_t ldx;
};

// (CGNN_OK, the columns) of a valid request: min_num to N distinct ids below N and, with_cols, as many distinct
// columns below ldx.  Without columns (the byte count does not depend on them; the classic family has none) the
// request is packed: measures[i] in column i of num.  An empty request has ldx = 1 and nothing to write.
template <int N>
inline int cgnn_check_request(const int32_t* measures, int32_t num, int32_t min_num, const int32_t* cols, int32_t ldx,
                              bool with_cols, cgnn_columns<N>* out) {
  if (num < min_num || num > N || (num > 0 && !measures)) return CGNN_EINVAL;
  for (int m = 0; m < N; ++m) out->col[m] = -1;
  out->ldx = num > 0 ? num : 1;
  for (int i = 0; i < num; ++i) {
    if (measures[i] < 0 || measures[i] >= N || out->col[measures[i]] >= 0) return CGNN_EINVAL;
    out->col[measures[i]] = i;
  }
  if (!with_cols || num == 0) return CGNN_OK;
  if (!cols || ldx < 1) return CGNN_EINVAL;
  for (int i = 0; i < num; ++i) {
    if (cols[i] < 0 || cols[i] >= ldx) return CGNN_EINVAL;
    for (int j = 0; j < i; ++j)
      if (cols[j] == cols[i]) return CGNN_EINVAL;
    out->col[measures[i]] = cols[i];
  }
  out->ldx = ldx;
  return CGNN_OK;
}

// cgnn_check_cohort for a family that keeps a subject in LDS: n <= max_n is the stricter bound on n * n.
inline int cgnn_check_cohort_upto(int64_t S, int32_t n, int32_t max_n) {
  return n > max_n ? CGNN_EINVAL : cgnn_check_cohort(S, n);
}

// The sizes of an entry point that answers CGNN_EUNSUPPORTED beyond its node bound (knn.hip, mst.hip): bad values
// first, then the bound, then cgnn_check_cohort.  cgnn_check_cohort_upto's families answer CGNN_EINVAL for the bound.
inline int cgnn_check_cohort_within(int64_t S, int32_t n, int32_t max_n) {
  if (S < 0 || n < 1) return CGNN_EINVAL;
  if (n > max_n) return CGNN_EUNSUPPORTED;
  return cgnn_check_cohort(S, n);
}

// Whether [p, p + p_bytes) and [q, q + q_bytes) share a byte.
inline bool cgnn_overlap(const void* p, int64_t p_bytes, const void* q, int64_t q_bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)q_bytes && b < a + (uintptr_t)p_bytes;
}

// A cohort-shaped `out` that may be the input itself: it holds S n n floats, and is `matrices` or disjoint from them.
inline int cgnn_check_cohort_out(const void* matrices, const void* out, int64_t out_bytes, int64_t S, int32_t n) {
  const int64_t bytes = S * (int64_t)n * n * (int64_t)sizeof(float);
  if (out_bytes < bytes) return CGNN_EINVAL;
  return matrices != out && cgnn_overlap(matrices, bytes, out, bytes) ? CGNN_EINVAL : CGNN_OK;
}

// What a call refuses even when S == 0 keeps it from launching (modules.hip, pagerank.hip): a negative byte count, a
// workspace that is not 16-byte aligned.
inline int cgnn_check_byte_counts(const void* workspace, std::initializer_list<int64_t> byte_counts) {
  for (const int64_t b : byte_counts)
    if (b < 0) return CGNN_EINVAL;
  return cgnn_misaligned({workspace}, 15) ? CGNN_EINVAL : CGNN_OK;
}

// The buffers of a call that launches (S > 0): matrices and thr are there, they and x are 4-byte aligned, the
// workspace 16-byte; if want_x, x is there and holds rows * ldx floats.  rows = S * n < 2^31 and ldx < 2^31: the
// product times 4 could wrap 64 bits, so the byte count is compared by division.
inline int cgnn_check_cohort_buffers(const void* matrices, const void* thr, const void* workspace, const void* x,
                                     int64_t x_bytes, bool want_x, int64_t rows, int32_t ldx) {
  if (!matrices || !thr || cgnn_misaligned({matrices, thr, x}, 3) || cgnn_misaligned({workspace}, 15)) return CGNN_EINVAL;
  if (want_x && (!x || x_bytes < 0 || x_bytes / (int64_t)sizeof(float) / ldx < rows)) return CGNN_EINVAL;
  return CGNN_OK;
}

// Workgroups of 8 waves a CU holds when each takes lds_bytes of the budget: by LDS, and against 32 wave slots.
inline int cgnn_wg_per_cu_by_lds(size_t lds_bytes, size_t budget) {
  const size_t by_lds = budget / lds_bytes;
  return by_lds > 4 ? 4 : (int)by_lds;
}

// Raises kKernel's dynamic LDS limit to `bytes`, once per device and kernel.  false: the runtime refused.
template <auto kKernel>
inline bool cgnn_raise_lds_limit(int bytes) {
  static bool done[CGNN_MAX_DEVICES] = {};
  bool& d = done[cgnn_device_ordinal()];
  if (!d) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kKernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            bytes) != hipSuccess)
      return false;
    d = true;
  }
  return true;
}
