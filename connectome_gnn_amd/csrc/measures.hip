// measures.hip -- graph-theoretic node features of a device-resident cohort of dense connectivity matrices
// (float [S, n, n]) at the thresholds of cgnn_ingest_select / cgnn_ingest_count:
// cgnn_ingest_measures, cgnn_ingest_measures_workspace_bytes.
//
// Per subject with matrix A and threshold t: e_ij iff i != j, A_ij > t and A_ij > 0 (ingest_rows.h);
// a_ij = A_ij on edges, b_ij = 1 on edges, k_i = sum_j b_ij, s_i = sum_j a_ij, wmax = max a_ij,
// u_ij = cbrt(a_ij / wmax) on edges; all are 0 elsewhere.  T_i(v) = sum_{j,k} v_ki v_kj v_ij.
//   strength  s_i / (max_i s_i + 1e-8)        degree  k_i / (n - 1)        mean_weight  s_i / (k_i + 1e-8)
//   clustering  T_i(b) / (k_i (k_i - 1))      weighted_clustering  T_i(u) / (k_i (k_i - 1))     (0 for k_i < 2)
//
//   k_measure_rows        a workgroup of 8 waves owns a subject, grid stride: a wave per row counts and sums the kept
//                         entries with THE row summation of ingest.hip (ingest_rows.h: the same bits) and takes their
//                         maximum; the workgroup then folds the largest strength and the largest weight.
//   k_measure_tri<map>    T_i(v) for v = b or u.  G = V^T V on the tile walk of gram_tile.h: a row-major matrix is
//                         its own frame-major panel with the rows k as the frames.  Stage: the edge test and the
//                         value map, applied on the way into LDS; rows and columns past n and the diagonal are zeros.
//                         Epilogue: G_ij v_ij summed over j is the partial of T_i for i in bi; for a block off the
//                         diagonal G_ij v_ji summed over i is the partial of T_j for j in bj (G is symmetric, so this
//                         is the mirrored block's row sum).  Lanes fold by shuffles, waves through LDS in wave order,
//                         and the item writes part[s][bj][i in bi] and part[s][bi][j in bj] (one slot, both sums, when
//                         bi == bj): every slot [s][b][i] is written exactly once, by the item
//                         (min(blk(i), b), max(blk(i), b)).
//   k_measure_finish      a thread per (subject, node): the nt partials in ascending b, the measures, x[s, i, column].
//
// No atomics: the same bits on every run and for every grid.  Element offsets into `matrices` are 64-bit.
// The request (1 to 5 distinct ids, packed columns), the cohort's size and its buffers are checked by
// measure_request.h.
#include <math.h>

#include "gram_tile.h"
#include "ingest_rows.h"
#include "measure_request.h"

namespace {

using namespace gram;

constexpr int kRowThreads = 512;              // k_measure_rows: 8 waves
constexpr int kRowWaves = kRowThreads / 64;
constexpr int kFinishThreads = 256;
static_assert(2 * kTile <= kThreads, "a thread per reduced row and per reduced column");

enum {
  kStrength = CGNN_MEASURE_STRENGTH,
  kDegree = CGNN_MEASURE_DEGREE,
  kMeanWeight = CGNN_MEASURE_MEAN_WEIGHT,
  kClustering = CGNN_MEASURE_CLUSTERING,
  kWeighted = CGNN_MEASURE_WEIGHTED_CLUSTERING
};

// ---- workspace: [k_i int32 S n | s_i float S n | (max_i s_i, wmax) float 2 S | T(b) partials | T(u) partials] ----
struct Layout {
  int64_t k, s, sub, part_b, part_u, total;
};
Layout layout_of(int64_t S, int32_t n, bool need_b, bool need_u) {
  const int64_t nt = tiles_of(n);
  const int64_t part = cgnn_align_up(S * nt * nt * kTile * (int64_t)sizeof(float), 256);
  Layout l;
  l.k = 0;
  l.s = l.k + cgnn_align_up(S * n * (int64_t)sizeof(int32_t), 256);
  l.sub = l.s + cgnn_align_up(S * n * (int64_t)sizeof(float), 256);
  l.part_b = l.sub + cgnn_align_up(2 * S * (int64_t)sizeof(float), 256);
  l.part_u = l.part_b + (need_b ? part : 0);
  l.total = l.part_u + (need_u ? part : 0);
  return l;
}

__global__ __launch_bounds__(kRowThreads) void k_measure_rows(const float* __restrict__ matrices, int64_t S, int n,
                                                              const float* __restrict__ thr, int32_t* __restrict__ deg,
                                                              float* __restrict__ strength, float* __restrict__ sub) {
  __shared__ float wave_s[kRowWaves], wave_w[kRowWaves];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const float* __restrict__ A = matrices + s * (int64_t)n * n;
    const float thr_s = thr[s];
    float smax = 0.0f, wmax = 0.0f;
    for (int i = wave; i < n; i += kRowWaves) {
      int cnt;
      float sum, mx;
      cgnn_row_kept<true>(A + (int64_t)i * n, i, n, thr_s, lane, cnt, sum, mx);
      if (lane == 0) {
        deg[s * n + i] = cnt;
        strength[s * n + i] = sum;
      }
      smax = fmaxf(smax, sum);
      wmax = fmaxf(wmax, mx);
    }
    if (lane == 0) {
      wave_s[wave] = smax;
      wave_w[wave] = wmax;
    }
    __syncthreads();
    if (t == 0) {
      float a = wave_s[0], b = wave_w[0];
#pragma unroll
      for (int w = 1; w < kRowWaves; ++w) {
        a = fmaxf(a, wave_s[w]);
        b = fmaxf(b, wave_w[w]);
      }
      sub[2 * s] = a;
      sub[2 * s + 1] = b;
    }
    __syncthreads();
  }
}

// The value map of one entry: 0 off the kept set, else 1 (binary) or cbrt(a / wmax), formed as cbrt(a) * rcw with
// rcw = 1 / cbrt(wmax) once per item: a staged entry costs a cube root and a multiply, no division, and neither factor
// leaves the fp32 range for any positive wmax (a subnormal wmax included).  wmax = +inf: rcw = 0, finite weights map to
// 0 and the infinite ones to NaN, as the quotient does.
template <bool kWeights>
__device__ __forceinline__ float value_of(float a, bool off_diagonal, float thr, float rcw) {
  if (!(off_diagonal && cgnn_kept(a, thr))) return 0.0f;
  return kWeights ? cbrtf(a) * rcw : 1.0f;
}

struct alignas(16) TriShared {
  Panels panel;                               // the rows k are the matrix rows
  float red[2][4][kTile / 2];                 // [row sums | column sums][wave][entry of the wave's quadrant]
};

template <bool kWeights, bool kVec>
__global__ __launch_bounds__(kThreads, 2) void k_measure_tri(const float* __restrict__ matrices, int64_t S, int n,
                                                          const float* __restrict__ thr,
                                                          const float* __restrict__ sub, float* __restrict__ part) {
  __shared__ TriShared sh;
  const Thread th;
  const int nt = tiles_of(n);
  const int64_t items = S * pairs_of(nt);

  for (int64_t item = first_item(); item < items; item += gridDim.x) {
    const Item it(item, nt, th.wave);
    const int64_t s = it.unit;
    const float* __restrict__ A = matrices + s * (int64_t)n * n;
    const float thr_s = thr[s];
    const float rcw = kWeights ? 1.0f / cbrtf(sub[2 * s + 1]) : 1.0f;

    f32x4 pre[2][kSlots], acc[3][3];
    load_panels<kVec>(pre, A, n, n, 0, it, th);
    __syncthreads();                          // the previous item's epilogue still reads sh.red and a panel

    // through the value map; what load4 read as 0 is never kept
    run<kVec>(sh.panel, pre, acc, A, n, n, it, th, [&](int side, int k, int c, f32x4 v) {
      f32x4 z;
#pragma unroll
      for (int e = 0; e < 4; ++e) z[e] = value_of<kWeights>(v[e], k != it.col0(side) + c + e, thr_s, rcw);
      return z;
    });

    float rsum[3][4], csum[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      csum[a] = 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) rsum[a][r] = 0.0f;
    }
    for_each_block(it, th, [&](int a, int b, bool tri, int, int gi0, int gj) {
      f32x4 mir = {0.f, 0.f, 0.f, 0.f};                       // A[gj][gi0 .. gi0 + 3], zeros outside the matrix
      if (!tri) mir = load4<kVec>(A, gj, n, gi0, n);         // (a block on the diagonal holds its own mirror)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = gi0 + r;
        const float aij = gi < n && gj < n ? A[(int64_t)gi * n + gj] : 0.0f;
        rsum[a][r] += acc[a][b][r] * value_of<kWeights>(aij, gi != gj, thr_s, rcw);
        if (!tri) csum[b] += acc[a][b][r] * value_of<kWeights>(mir[r], gi != gj, thr_s, rcw);
      }
    });
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = rsum[a][r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
        if (th.fcol == 0) sh.red[0][th.wave][a * 16 + 4 * th.frow + r] = v;
      }
      float c = csum[a];
      c += __shfl_xor(c, 16, 64);
      c += __shfl_xor(c, 32, 64);
      if (th.frow == 0) sh.red[1][th.wave][a * 16 + th.fcol] = c;
    }
    __syncthreads();
    // the waves of a quadrant row (column), in wave order; a diagonal tile adds both into the one slot it owns
    if (th.tid < 2 * kTile) {
      const int kind = th.tid / kTile, c = th.tid - kind * kTile;
      const int quad = c / (kTile / 2), e = c - quad * (kTile / 2);
      if (!(it.diag && kind == 1)) {
        float v = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w)
          if ((kind == 0 ? quad_row(w, it.diag) : quad_col(w, it.diag)) == quad) v += sh.red[kind][w][e];
        if (it.diag) {
#pragma unroll
          for (int w = 0; w < 4; ++w)
            if (quad_col(w, true) == quad) v += sh.red[1][w][e];
        }
        // row sums: nodes of tile bi, summed over the columns of tile bj; column sums the other way round
        const int node_tile = kind == 0 ? it.bi : it.bj, over_tile = kind == 0 ? it.bj : it.bi;
        part[((s * nt + over_tile) * nt + node_tile) * (int64_t)kTile + c] = v;
      }
    }
  }
}

typedef cgnn_columns<CGNN_NUM_MEASURES> Columns;

__global__ __launch_bounds__(kFinishThreads) void k_measure_finish(int64_t S, int n, const int32_t* __restrict__ deg,
                                                                   const float* __restrict__ strength,
                                                                   const float* __restrict__ sub,
                                                                   const float* __restrict__ part_b,
                                                                   const float* __restrict__ part_u, Columns cols,
                                                                   float* __restrict__ x) {
  const int nt = tiles_of(n);
  const int64_t rows = S * n;
  for (int64_t r = (int64_t)blockIdx.x * kFinishThreads + threadIdx.x; r < rows;
       r += (int64_t)gridDim.x * kFinishThreads) {
    const int64_t s = r / n;
    const int i = (int)(r - s * n);
    const int k = deg[r];
    const float si = strength[r], kf = (float)k;
    const float pairs = kf * (kf - 1.0f);
    float* __restrict__ o = x + r * cols.ldx;
    if (cols.col[kStrength] >= 0) o[cols.col[kStrength]] = cgnn_strength_feature(si, sub[2 * s]);
    if (cols.col[kDegree] >= 0) o[cols.col[kDegree]] = n > 1 ? kf / (float)(n - 1) : 0.0f;
    if (cols.col[kMeanWeight] >= 0) o[cols.col[kMeanWeight]] = si / (kf + 1e-8f);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int c = cols.col[m == 0 ? kClustering : kWeighted];
      if (c < 0) continue;
      const float* __restrict__ p = (m == 0 ? part_b : part_u) + s * nt * nt * (int64_t)kTile + i;
      float t = 0.0f;
      for (int b = 0; b < nt; ++b) t += p[(int64_t)b * nt * kTile];
      o[c] = k >= 2 ? t / pairs : 0.0f;
    }
  }
}

// Persistent grid of the product kernel, in workgroups per CU: its 57 KB of LDS admit two (k_corr's figure).
#ifndef CGNN_MEASURE_WG_PER_CU
#define CGNN_MEASURE_WG_PER_CU 2
#endif
#ifndef CGNN_MEASURE_ROWS_PER_CU
#define CGNN_MEASURE_ROWS_PER_CU 4
#endif

// (CGNN_OK, the packed columns) of a valid call: the cohort's size, then 1 to 5 distinct ids
int check(int64_t S, int32_t n, const int32_t* measures, int32_t num, Columns* c) {
  if (cgnn_check_cohort(S, n) != CGNN_OK) return CGNN_EINVAL;
  return cgnn_check_request(measures, num, 1, nullptr, 0, false, c);
}

template <bool kWeights>
void launch_tri(const float* matrices, int64_t S, int32_t n, const float* thr, const float* sub, float* part,
                hipStream_t hs) {
  const int grid = cgnn_grid_for(S * pairs_of(tiles_of(n)), CGNN_MEASURE_WG_PER_CU);
  if (n % 4 == 0 && !(reinterpret_cast<uintptr_t>(matrices) & 15))
    k_measure_tri<kWeights, true><<<grid, kThreads, 0, hs>>>(matrices, S, n, thr, sub, part);
  else
    k_measure_tri<kWeights, false><<<grid, kThreads, 0, hs>>>(matrices, S, n, thr, sub, part);
}

}  // namespace

extern "C" int64_t cgnn_ingest_measures_workspace_bytes(int64_t S, int32_t n, const int32_t* measures,
                                                        int32_t num_measures) {
  Columns c;
  if (check(S, n, measures, num_measures, &c) != CGNN_OK) return CGNN_EINVAL;
  return layout_of(S, n, c.col[kClustering] >= 0, c.col[kWeighted] >= 0).total;
}

extern "C" int cgnn_ingest_measures(const float* matrices, int64_t S, int32_t n, const float* thr,
                                    const int32_t* measures, int32_t num_measures, void* workspace,
                                    int64_t workspace_bytes, float* x, int64_t x_bytes, void* stream) {
  Columns cols;
  if (check(S, n, measures, num_measures, &cols) != CGNN_OK) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (!workspace || cgnn_check_cohort_buffers(matrices, thr, workspace, x, x_bytes, true, S * n, cols.ldx) != CGNN_OK)
    return CGNN_EINVAL;
  const bool need_b = cols.col[kClustering] >= 0, need_u = cols.col[kWeighted] >= 0;
  const Layout l = layout_of(S, n, need_b, need_u);
  CGNN_NEED_BYTES(workspace, workspace_bytes, l.total);
  char* ws = static_cast<char*>(workspace);
  int32_t* deg = reinterpret_cast<int32_t*>(ws + l.k);
  float* strength = reinterpret_cast<float*>(ws + l.s);
  float* sub = reinterpret_cast<float*>(ws + l.sub);
  float* part_b = need_b ? reinterpret_cast<float*>(ws + l.part_b) : nullptr;
  float* part_u = need_u ? reinterpret_cast<float*>(ws + l.part_u) : nullptr;
  hipStream_t hs = cgnn_stream(stream);
  k_measure_rows<<<cgnn_grid_for(S, CGNN_MEASURE_ROWS_PER_CU), kRowThreads, 0, hs>>>(matrices, S, n, thr, deg, strength,
                                                                                     sub);
  CGNN_CHECK_LAUNCH();
  if (need_b) {
    launch_tri<false>(matrices, S, n, thr, sub, part_b, hs);
    CGNN_CHECK_LAUNCH();
  }
  if (need_u) {
    launch_tri<true>(matrices, S, n, thr, sub, part_u, hs);
    CGNN_CHECK_LAUNCH();
  }
  const int64_t blocks = (S * n + kFinishThreads - 1) / kFinishThreads;
  k_measure_finish<<<cgnn_grid_for(blocks, 8), kFinishThreads, 0, hs>>>(S, n, deg, strength, sub, part_b, part_u, cols,
                                                                        x);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
