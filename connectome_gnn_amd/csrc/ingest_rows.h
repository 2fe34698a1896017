// ingest_rows.h -- THE edge predicate and THE row summation of a thresholded connectivity matrix, defined once for
// ingest.hip (edge counts, the default strength feature) and measures.hip (degree, strength, the weight maximum):
// both must give the same bits for a row's strength, so neither restates the order of the additions.
#pragma once
#include <math.h>

#include "common.h"

typedef float cgnn_f32x4_e __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes at element alignment

// the edge predicate (diagonal aside): both comparisons strict, a NaN fails both
__device__ __forceinline__ bool cgnn_kept(float v, float t) { return v > t && v > 0.0f; }

// 4 consecutive entries of a row from column j0 on; columns >= n read as -inf (never kept)
__device__ __forceinline__ cgnn_f32x4 cgnn_load_row4(const float* __restrict__ row, int j0, int n) {
  if (j0 + 4 <= n) return *reinterpret_cast<const cgnn_f32x4_e*>(row + j0);
  cgnn_f32x4 v = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  if (j0 < n) v[0] = row[j0];
  if (j0 + 1 < n) v[1] = row[j0 + 1];
  if (j0 + 2 < n) v[2] = row[j0 + 2];
  return v;
}

// One wave over row i of a subject: the number of kept entries and their sum, on every lane.  Lane l adds the
// entries of columns 4 l + 256 c + (0..3) in ascending order, then the lanes are folded by cgnn_wave_sum; with
// kMax also the largest kept entry (0 for a row without one).
template <bool kMax>
__device__ __forceinline__ void cgnn_row_kept(const float* __restrict__ row, int i, int n, float thr, int lane,
                                              int& cnt, float& sum, float& mx) {
  cnt = 0;
  sum = 0.0f;
  mx = 0.0f;
  for (int j0 = 4 * lane; j0 < n; j0 += 256) {
    const cgnn_f32x4 v = cgnn_load_row4(row, j0, n);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (j0 + q != i && cgnn_kept(v[q], thr)) {
        ++cnt;
        sum += v[q];
        if (kMax) mx = fmaxf(mx, v[q]);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  sum = cgnn_wave_sum(sum);
  if (kMax) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
}

// the default node feature from a row's strength and the subject's largest
__device__ __forceinline__ float cgnn_strength_feature(float strength, float largest) {
  return strength / (largest + 1e-8f);
}
