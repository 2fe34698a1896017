// knn.hip -- k-nearest-neighbour sparsification of a device-resident cohort of connectivity matrices (float [S, n, n]):
// every row keeps its k strongest positive entries, the picks are symmetrised, the rest becomes +0.0 (DESIGN.md 4.3p,
// include/cgnn_knn.h): cgnn_ingest_knn.
//
//   k_knn<NC>   one workgroup of 8 waves OWNS a subject; 2 per CU walk the subjects with a grid stride.  NC is the number
//               of 256-column chunks of a row (1..4), so that a lane's 4 * NC entries of a row are registers.
//       phase 1  a wave per row.  The candidates are the positive off-diagonal entries; the bits of a positive float
//                order as the floats do, so the key of an entry is its bits and 0 for everything else.  The last pick's
//                key has descending rank kk - 1, kk = min(k, p_i): an exact radix select, four 8-bit digits from the
//                top on a histogram of the wave's own in LDS (integer ds_add: the order of the adds does not matter),
//                a lane owning 4 bins and a lane prefix sum running down them, in registers: the select is bound by the
//                LDS operations it issues.  What is left of the rank is the pick's place in the tie
//                class, in column order: ballots and lane prefixes.  (v_i, c_i) go to LDS.
//       barrier  every pick of the subject exists before anything is written: out == matrices is safe.
//       phase 2  d_ij iff A_ij > 0 and (A_ij > v_i or (A_ij == v_i and j <= c_i)), i != j.
//                DIRECTED: a wave per row, 16-byte accesses, every entry read and written by the same lane.
//                UNION / MUTUAL: a wave takes pairs of 32 x 32 tiles (bi, bj), (bj, bi) with bi <= bj: both are loaded
//                whole into registers (lane l: row 8 t + l / 8, columns 4 (l % 8) .. + 3, t = 0..3), written to the
//                wave's own LDS at a row stride of 33 floats, read back transposed (both directions free of bank
//                conflicts: banks r + 4 m + q and 4 m + q + 8 t + w over a half wave are 32 different ones), decided
//                and stored.  Every entry belongs to one pair, so nothing is read after another wave wrote it.
//
// No atomics on global memory and no work assignment that depends on the grid: the same bits every run.  Rows of an
// odd n are only 4-byte aligned: 16-byte accesses are declared at element alignment (ingest_rows.h); element offsets
// are 64-bit.
#include <math.h>

#include "common.h"
#include "ingest_rows.h"
#include "measure_request.h"
#include "wave_ops.h"

namespace {

constexpr int kThreads = 512;                 // 8 waves
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 32;                     // phase 2: a wave's tiles are kTile x kTile
constexpr int kLd = kTile + 1;                // their row stride in LDS: the transposed read is conflict-free
constexpr int kMaxNodes = CGNN_KNN_MAX_NODES;
static_assert(kMaxNodes == 4 * 256, "a row is at most 4 chunks of 256 columns");

typedef cgnn_f32x4 f32x4;
typedef cgnn_f32x4_e f32x4_e;

struct KnnShared {
  float v[kMaxNodes];                         // the value of a row's last pick; +inf: no pick
  int32_t c[kMaxNodes];                       // its column; -1: no pick
  // phase 2: a wave's two tiles; phase 1: the wave's histogram of one digit, 256 counts, in the same place (the
  // phases are a workgroup barrier apart in both directions), so that two workgroups fit the LDS of a CU
  alignas(16) float tile[kWaves][2][kTile * kLd];
};
static_assert(sizeof(float) * 2 * kTile * kLd % 16 == 0 && 2 * kTile * kLd >= 256, "a histogram fits, 16-byte aligned");
static_assert(2 * sizeof(KnnShared) <= 160 * 1024, "two workgroups per CU");

// whether row i picks its entry x in column `col`, from the row's last pick (v, c); the diagonal is the caller's
__device__ __forceinline__ bool picked(float x, float v, int c, int col) {
  return x > 0.0f && (x > v || (x == v && col <= c));
}

// 4 entries of row i of A from column j0 on; what lies outside the matrix reads as -inf (never positive)
__device__ __forceinline__ f32x4 load4(const float* A, int n, int i, int j0) {
  if (i >= n) return f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  return cgnn_load_row4(A + (int64_t)i * n, j0, n);
}

__device__ __forceinline__ void store4(float* B, int n, int i, int j0, f32x4 x) {
  if (i >= n) return;
  float* row = B + (int64_t)i * n;
  if (j0 + 4 <= n) {
    *reinterpret_cast<f32x4_e*>(row + j0) = x;
  } else {
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (j0 + q < n) row[j0 + q] = x[q];
  }
}

// Phase 1 for row i, by one wave: (v_i, c_i) into LDS.
template <int NC>
__device__ __forceinline__ void row_picks(const float* A, int n, int i, int64_t k, int lane, KnnShared& sh) {
  constexpr int R = 4 * NC;
  const float* row = A + (int64_t)i * n;
  uint32_t key[R];
  int p = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int j0 = 256 * c + 4 * lane;
    const f32x4 x = cgnn_load_row4(row, j0, n);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool cand = x[q] > 0.0f && j0 + q != i;                  // (a NaN and the -inf past the row's end fail)
      key[4 * c + q] = cand ? __float_as_uint(x[q]) : 0u;
      p += __popcll(__ballot(cand));
    }
  }
  const int kk = k < (int64_t)p ? (int)k : p;
  if (kk == 0) {                                                       // (wave-uniform)
    if (lane == 0) {
      sh.v[i] = INFINITY;
      sh.c[i] = -1;
    }
    return;
  }
  // The key of descending rank kk - 1 among the candidates: a radix select, four 8-bit digits from the top, on the
  // wave's own histogram.  Lane l owns the bins 255 - 4 l .. 252 - 4 l, so a prefix sum over the lanes runs down the bins.
  uint32_t* hist = reinterpret_cast<uint32_t*>(sh.tile[threadIdx.x >> 6][0]);
  uint32_t last = 0u, lmask = 0u, rank = (uint32_t)(kk - 1);
  for (int shift = 24; shift >= 0; shift -= 8) {
    *reinterpret_cast<cgnn_u32x4*>(hist + 4 * lane) = cgnn_u32x4{0u, 0u, 0u, 0u};
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (key[r] != 0u && (key[r] & lmask) == last) atomicAdd(&hist[(key[r] >> shift) & 255u], 1u);
    wave_lds_fence();
    const cgnn_u32x4 h = *reinterpret_cast<const cgnn_u32x4*>(hist + 252 - 4 * lane);
    const uint32_t cnt[4] = {h[3], h[2], h[1], h[0]};                  // bins 255 - 4 l - q, q = 0..3
    const uint32_t tsum = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    const uint32_t incl = (uint32_t)wave_scan((int)tsum);   // (in registers: the select is bound by its LDS traffic)
    uint32_t run = incl - tsum, digit = 0u, left = 0u;
    const bool mine = run <= rank && rank < incl;                      // exactly one lane: the rank lies in its bins
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (rank >= run && rank < run + cnt[q]) {
        digit = (uint32_t)(255 - 4 * lane - q);
        left = rank - run;
      }
      run += cnt[q];
    }
    const int owner = __ffsll((unsigned long long)__ballot(mine)) - 1;
    last |= (uint32_t)__builtin_amdgcn_readlane((int)digit, owner) << shift;
    lmask |= 255u << shift;
    rank = (uint32_t)__builtin_amdgcn_readlane((int)left, owner);
    wave_lds_fence();                          // the bins are read before the next digit clears them
  }
  const int want = (int)rank;                  // the last pick is member `want` (0-based) of the tie class, by column
  const uint64_t below = (1ull << lane) - 1ull;
  int running = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    bool tie[4];
    int before = running;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      tie[q] = key[4 * c + q] == last;
      const uint64_t m = __ballot(tie[q]);
      before += __popcll(m & below);
      running += __popcll(m);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (tie[q]) {
        if (before == want) {                  // exactly one entry of the row
          sh.v[i] = __uint_as_float(last);
          sh.c[i] = 256 * c + 4 * lane + q;
        }
        ++before;
      }
    }
  }
}

// Phase 2, CGNN_KNN_DIRECTED: row i by one wave.
__device__ __forceinline__ void row_directed(const float* A, float* B, int n, int i, int lane, const KnnShared& sh) {
  const float v = sh.v[i];
  const int c = sh.c[i];
  for (int j0 = 4 * lane; j0 < n; j0 += 256) {
    const f32x4 x = load4(A, n, i, j0);
    f32x4 y;
#pragma unroll
    for (int q = 0; q < 4; ++q) y[q] = (j0 + q != i && picked(x[q], v, c, j0 + q)) ? x[q] : 0.0f;
    store4(B, n, i, j0, y);
  }
}

// One tile of a pair: `x` are the lane's entries of rows r0 + 8 t + w, columns c0 + 4 m + (0..3); `tr` is the LDS image
// of the tile across the diagonal, so tr[(4 m + q) * kLd + 8 t + w] is the entry (column, row).
__device__ __forceinline__ void decide_tile(float* B, int n, int r0, int c0, const f32x4 (&x)[4], const float* tr,
                                            bool mutual, int w, int m, const KnnShared& sh) {
  float vj[4];
  int cj[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = c0 + 4 * m + q;
    vj[q] = j < n ? sh.v[j] : INFINITY;
    cj[q] = j < n ? sh.c[j] : -1;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = r0 + 8 * t + w;
    const float vi = i < n ? sh.v[i] : INFINITY;
    const int ci = i < n ? sh.c[i] : -1;
    f32x4 y;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = c0 + 4 * m + q;
      const float a = x[t][q], at = tr[(4 * m + q) * kLd + 8 * t + w];
      const bool dij = picked(a, vi, ci, j), dji = picked(at, vj[q], cj[q], i);
      const bool kept = i != j && (mutual ? (dij && dji) : (dij || (dji && a > 0.0f)));
      y[q] = kept ? a : 0.0f;
    }
    store4(B, n, i, c0 + 4 * m, y);
  }
}

template <int NC>
__global__ __launch_bounds__(kThreads) void k_knn(const float* matrices, int64_t S, int n, int64_t k, int mode,
                                                  float* out) {
  __shared__ KnnShared sh;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w = lane >> 3, m = lane & 7;       // phase 2: the lane's row within 8 and its group of 4 columns
  const int nb = (n + kTile - 1) / kTile;
  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const float* A = matrices + s * (int64_t)n * n;
    float* B = out + s * (int64_t)n * n;
    for (int i = wave; i < n; i += kWaves) row_picks<NC>(A, n, i, k, lane, sh);
    __syncthreads();                           // all picks of the subject exist; nothing of it has been written
    if (mode == CGNN_KNN_DIRECTED) {
      for (int i = wave; i < n; i += kWaves) row_directed(A, B, n, i, lane, sh);
    } else {
      float* t1 = sh.tile[wave][0];
      float* t2 = sh.tile[wave][1];
      int bi = 0, bj = 0;                      // pair number `wave` of (0,0) (0,1) .. (0,nb-1) (1,1) ..
      for (int step = 0; step < wave; ++step)
        if (++bj == nb) bj = ++bi;
      while (bi < nb) {
        const int r0 = kTile * bi, c0 = kTile * bj;
        f32x4 x1[4], x2[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          x1[t] = load4(A, n, r0 + 8 * t + w, c0 + 4 * m);
          x2[t] = bi != bj ? load4(A, n, c0 + 8 * t + w, r0 + 4 * m) : x1[t];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            t1[(8 * t + w) * kLd + 4 * m + q] = x1[t][q];
            t2[(8 * t + w) * kLd + 4 * m + q] = x2[t][q];
          }
        }
        wave_lds_fence();                      // the tiles are the wave's own
        decide_tile(B, n, r0, c0, x1, t2, mode == CGNN_KNN_MUTUAL, w, m, sh);
        if (bi != bj) decide_tile(B, n, c0, r0, x2, t1, mode == CGNN_KNN_MUTUAL, w, m, sh);
        wave_lds_fence();                      // ... before the next pair overwrites the tiles
        for (int step = 0; step < kWaves && bi < nb; ++step)
          if (++bj == nb) bj = ++bi;
      }
    }
    __syncthreads();                           // the picks are read until here; the next subject overwrites them
  }
}

#ifndef CGNN_KNN_WG_PER_CU
#define CGNN_KNN_WG_PER_CU 2                   // 74 KB of LDS a workgroup
#endif

}  // namespace

extern "C" int cgnn_ingest_knn(const float* matrices, int64_t S, int32_t n, int64_t k, int32_t mode, float* out,
                               int64_t out_bytes, void* stream) {
  if (k < 0 || (mode != CGNN_KNN_DIRECTED && mode != CGNN_KNN_UNION && mode != CGNN_KNN_MUTUAL)) return CGNN_EINVAL;
  if (const int rc = cgnn_check_cohort_within(S, n, CGNN_KNN_MAX_NODES)) return rc;
  if (S == 0) return CGNN_OK;
  if (!matrices || !out || cgnn_misaligned({matrices, out}, 3)) return CGNN_EINVAL;
  if (cgnn_check_cohort_out(matrices, out, out_bytes, S, n) != CGNN_OK) return CGNN_EINVAL;
  const int grid = cgnn_grid_for(S, CGNN_KNN_WG_PER_CU);
  hipStream_t st = cgnn_stream(stream);
  switch ((n + 255) / 256) {
    case 1: k_knn<1><<<grid, kThreads, 0, st>>>(matrices, S, n, k, mode, out); break;
    case 2: k_knn<2><<<grid, kThreads, 0, st>>>(matrices, S, n, k, mode, out); break;
    case 3: k_knn<3><<<grid, kThreads, 0, st>>>(matrices, S, n, k, mode, out); break;
    default: k_knn<4><<<grid, kThreads, 0, st>>>(matrices, S, n, k, mode, out); break;
  }
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
