// mst.hip -- the maximum-spanning-tree backbone of a device-resident cohort of connectivity matrices (float [S, n, n]):
// every subject keeps the maximum spanning forest of its positive weights, united with what lies above its threshold;
// the rest becomes +0.0 (include/cgnn_mst.h): cgnn_ingest_mst, cgnn_ingest_mst_workspace_bytes.
//
// The statement, per subject, for a matrix A [n, n] fp32 of any sign that need not be symmetric:
//   p(x) = x if x > 0 else 0.  A NaN is not positive.  +inf is positive.  A subnormal is positive.
//   The pair {i, j}, i < j, has weight w_ij = max(p(A_ij), p(A_ji)).  It is a candidate iff w_ij > 0.
//   Order: the pair (i, j) comes before (i', j') iff w > w', or w == w' and (i, j) is lexicographically lower.  This is
//     a strict total order.
//   F is the maximum spanning forest under that order.  Kruskal takes a pair iff its ends lie in different components.
//     F is unique.  It has n - c pairs, where c is the number of components of the candidate graph.
//     Any correct algorithm that compares edges by this strict order finds the same F.  That includes Prim with restarts
//     from the lowest unvisited node, Boruvka and Kruskal.  The all-0.5 matrix gives the star at node 0.
//   kept_ij iff i != j, A_ij > 0 and ({i, j} in F or A_ij > t_s).  t_s is the subject's threshold.  No thresholds means
//     t_s = +inf, the tree alone.
//     A tree pair whose reverse entry is not positive keeps only the positive direction.  knn's "union" mode does the
//     same.
//   out_ij is the bits of A_ij where kept and +0.0 elsewhere.  The diagonal and every NaN become +0.0 too.
//   out may be `matrices` itself and gives the same bits.  Any other overlap is refused.
//
//   k_mst   one workgroup of 4 waves OWNS a subject; 2 per CU walk the subjects with a grid stride.
//       phase 0  W = max(p(A), p(A)^T) into the workgroup's slab of the workspace, [n][ld], ld = n rounded up to 4 (rows
//                16-byte aligned): a wave takes pairs of 32 x 32 tiles (bi, bj), (bj, bi), bi <= bj, as k_knn does,
//                exchanges them transposed through padded LDS of its own and stores both tiles of W.  The maximum is
//                taken on the bits: those of non-negative floats order as the floats do, and no subnormal is flushed.
//       phase 1  Prim with restarts.  Thread t owns the nodes 4 t .. 4 t + 3 and keeps one 64-bit key per node in
//                registers: 0 for a node in the tree (or past n); for a node outside it the best pair into the tree,
//                (bits(w) << 32) | ~((i << 11) | (j << 1) | f) with i < j and f = 1 iff the outside node is j, so that the
//                integer maximum is the statement's order ((i << 11) | (j << 1) orders as i n + j does) and the winner
//                decodes to the new node and its parent with shifts; without a pair, ~node in the low word: the maximum
//                of those is the lowest unvisited node, the root of the next tree.  Each of the n steps: the maximum
//                over the lanes (DPP), over the waves (two LDS slots by the step's parity: one barrier a step), the
//                decode, parent[u] into LDS, then one coalesced 16-byte read of row u of the slab and the relaxation.
//       barrier  every decision exists before anything is written: out == matrices is safe.
//       phase 2  a wave per row, 16-byte accesses, every entry read and written by the same lane:
//                kept iff A_ij > 0 and (A_ij > t_s or parent[i] == j or parent[j] == i), i != j.
//
// No atomics and no work assignment that depends on the grid: the same bits every run.  Rows of an odd n are only
// 4-byte aligned: 16-byte accesses to A and out are declared at element alignment (ingest_rows.h); element offsets are
// 64-bit.
#include <math.h>

#include "common.h"
#include "ingest_rows.h"
#include "measure_request.h"
#include "wave_ops.h"

namespace {

constexpr int kThreads = 256;                 // 4 waves: a thread owns 4 nodes of the tree phase
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 32;                     // phase 0: a wave's tiles are kTile x kTile
constexpr int kLd = kTile + 1;                // their row stride in LDS: the transposed read is conflict-free
constexpr int kMaxNodes = CGNN_MST_MAX_NODES;
static_assert(kMaxNodes == 4 * kThreads, "a thread owns 4 nodes");
static_assert(kMaxNodes <= 1024, "a node takes 10 bits of a key");

typedef cgnn_f32x4 f32x4;
typedef cgnn_f32x4_e f32x4_e;

struct MstShared {
  int32_t parent[kMaxNodes];                  // the node's neighbour towards its tree's root; -1: a root
  uint64_t best[2][kWaves];                   // a step's maximum of every wave, by the step's parity
  alignas(16) float tile[kWaves][2][kTile * kLd];
};

// 4 entries of row i of A from column j0 on; what lies outside the matrix reads as -inf (never positive)
__device__ __forceinline__ f32x4 load4(const float* A, int n, int i, int j0) {
  if (i >= n) return f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  return cgnn_load_row4(A + (int64_t)i * n, j0, n);
}

__device__ __forceinline__ void store4(float* B, int n, int i, int j0, f32x4 x) {
  float* row = B + (int64_t)i * n;
  if (j0 + 4 <= n) {
    *reinterpret_cast<f32x4_e*>(row + j0) = x;
  } else {
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (j0 + q < n) row[j0 + q] = x[q];
  }
}

// the bits of p(x): those of x if x > 0, else 0
__device__ __forceinline__ uint32_t pbits(float x) { return x > 0.0f ? __float_as_uint(x) : 0u; }

// One tile of W: `x` are the lane's entries of rows r0 + 8 t + w, columns c0 + 4 m + (0..3) of A; `tr` is the LDS image
// of the tile across the diagonal, so tr[(4 m + q) * kLd + 8 t + w] is the entry (column, row).  The slab's rows are
// ld >= n floats, ld % 4 == 0: a group of 4 that begins inside a row lies inside it (columns >= n hold 0).
__device__ __forceinline__ void weigh_tile(float* W, int n, int ld, int r0, int c0, const f32x4 (&x)[4], const float* tr,
                                           int w, int m) {
  const int j0 = c0 + 4 * m;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = r0 + 8 * t + w;
    f32x4 y;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t a = pbits(x[t][q]), b = pbits(tr[(4 * m + q) * kLd + 8 * t + w]);
      y[q] = __uint_as_float(a > b ? a : b);
    }
    if (i < n && j0 < ld) *reinterpret_cast<f32x4*>(W + (int64_t)i * ld + j0) = y;
  }
}

// max(x, what the lane that the DPP control names holds); a lane without a source, or in a row outside kRowMask, sees 0
template <int kCtrl, int kRowMask>
__device__ __forceinline__ uint64_t dpp_max(uint64_t x) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, kCtrl, kRowMask, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), kCtrl, kRowMask, 0xf, false);
  const uint64_t o = ((uint64_t)hi << 32) | lo;
  return o > x ? o : x;
}

// The maximum of x over the 64 lanes, on every lane: a running maximum within rows of 16 lanes by row_shr 1, 2, 4, 8,
// then lane 15 of a row into the next row (row_bcast:15 on rows 1 and 3) and lane 31 into the upper half (row_bcast:31
// on rows 2 and 3): lane 63 holds the whole wave's.
__device__ __forceinline__ uint64_t wave_max(uint64_t x) {
  x = dpp_max<0x111, 0xf>(x);
  x = dpp_max<0x112, 0xf>(x);
  x = dpp_max<0x114, 0xf>(x);
  x = dpp_max<0x118, 0xf>(x);
  x = dpp_max<0x142, 0xa>(x);
  x = dpp_max<0x143, 0xc>(x);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, 63);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), 63);
  return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kThreads) void k_mst(const float* matrices, int64_t S, int n, const float* thresholds,
                                                  float* slabs, int64_t slab_floats, float* out) {
  __shared__ MstShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int w = lane >> 3, m = lane & 7;       // phase 0: the lane's row within 8 and its group of 4 columns
  const int nb = (n + kTile - 1) / kTile;
  const int ld = (n + 3) & ~3;
  float* W = slabs + (int64_t)blockIdx.x * slab_floats;
  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const float* A = matrices + s * (int64_t)n * n;
    float* B = out + s * (int64_t)n * n;
    const float thr = thresholds ? thresholds[s] : INFINITY;
    // ---- phase 0: the symmetrised positive weights, into the slab
    {
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
        weigh_tile(W, n, ld, r0, c0, x1, t2, w, m);
        if (bi != bj) weigh_tile(W, n, ld, c0, r0, x2, t1, w, m);
        wave_lds_fence();                      // ... before the next pair overwrites the tiles
        for (int step = 0; step < kWaves && bi < nb; ++step)
          if (++bj == nb) bj = ++bi;
      }
    }
    __syncthreads();                           // the slab is whole (the workgroup's own stores, through its CU's cache)
    // ---- phase 1: Prim with restarts from the lowest unvisited node
    uint64_t key[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) key[q] = 4 * tid + q < n ? (uint64_t)~(uint32_t)(4 * tid + q) : 0ull;
    for (int step = 0; step < n; ++step) {
      uint64_t best = key[0] > key[1] ? key[0] : key[1];
      const uint64_t b23 = key[2] > key[3] ? key[2] : key[3];
      best = wave_max(best > b23 ? best : b23);
      if (lane == 0) sh.best[step & 1][wave] = best;
      __syncthreads();                         // (the other parity's slots are free: their readers passed the last barrier)
#pragma unroll
      for (int v = 0; v < kWaves; ++v) {
        const uint64_t o = sh.best[step & 1][v];
        best = o > best ? o : best;
      }
      if (best == 0ull) break;                 // (never: a node is outside the trees in each of the n steps; uniform)
      const uint32_t code = ~(uint32_t)best;
      int u, par;
      if ((uint32_t)(best >> 32) == 0u) {      // no pair reaches out of the trees so far: a new root
        u = (int)code;
        par = -1;
      } else {
        const int i = (int)(code >> 11), j = (int)((code >> 1) & 1023u);
        u = (code & 1u) ? j : i;
        par = (code & 1u) ? i : j;
      }
      if (tid == 0) sh.parent[u] = par;
      const f32x4 row = 4 * tid < ld ? *reinterpret_cast<const f32x4*>(W + (int64_t)u * ld + 4 * tid) : f32x4{0, 0, 0, 0};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 4 * tid + q;
        if (j == u) key[q] = 0ull;
        const uint32_t wb = __float_as_uint(row[q]);                   // (W holds +0.0 or a positive float)
        if (key[q] != 0ull && wb != 0u) {                              // j is outside the tree and {u, j} a candidate
          const uint32_t lo = u < j ? (uint32_t)u : (uint32_t)j, hi = u < j ? (uint32_t)j : (uint32_t)u;
          const uint64_t cand = ((uint64_t)wb << 32) | (uint64_t)~((lo << 11) | (hi << 1) | (u < j ? 1u : 0u));
          key[q] = cand > key[q] ? cand : key[q];
        }
      }
    }
    __syncthreads();                           // the forest is whole; nothing of the subject has been written
    // ---- phase 2: the forest united with what lies above the threshold
    for (int i = wave; i < n; i += kWaves) {
      const int pi = sh.parent[i];
      for (int j0 = 4 * lane; j0 < n; j0 += 256) {
        const f32x4 x = load4(A, n, i, j0);
        f32x4 y;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = j0 + q;
          const bool tree = j < n && (pi == j || sh.parent[j] == i);
          y[q] = (j != i && x[q] > 0.0f && (x[q] > thr || tree)) ? x[q] : 0.0f;
        }
        store4(B, n, i, j0, y);
      }
    }
    __syncthreads();                           // parent[] is read until here; the next subject overwrites it and the slab
  }
}

#ifndef CGNN_MST_WG_PER_CU
#define CGNN_MST_WG_PER_CU 2
#endif

int64_t slab_floats_of(int n) { return (int64_t)n * ((n + 3) & ~3); }      // rows of ld floats: a multiple of 16 bytes

}  // namespace

extern "C" int64_t cgnn_ingest_mst_workspace_bytes(int64_t S, int32_t n) {
  if (S < 0 || n < 1 || n > CGNN_MST_MAX_NODES || cgnn_check_cohort(S, n) != CGNN_OK) return CGNN_EINVAL;
  return cgnn_grid_for(S, CGNN_MST_WG_PER_CU) * slab_floats_of(n) * (int64_t)sizeof(float);
}

extern "C" int cgnn_ingest_mst(const float* matrices, int64_t S, int32_t n, const float* thresholds, void* workspace,
                               int64_t workspace_bytes, float* out, int64_t out_bytes, void* stream) {
  if (const int rc = cgnn_check_cohort_within(S, n, CGNN_MST_MAX_NODES)) return rc;
  if (S == 0) return CGNN_OK;
  if (!matrices || !out || !workspace || cgnn_misaligned({matrices, out, thresholds}, 3) ||
      cgnn_misaligned({workspace}, 15))
    return CGNN_EINVAL;
  if (cgnn_check_cohort_out(matrices, out, out_bytes, S, n) != CGNN_OK) return CGNN_EINVAL;
  const int64_t bytes = S * (int64_t)n * n * (int64_t)sizeof(float);
  const int grid = cgnn_grid_for(S, CGNN_MST_WG_PER_CU);
  const int64_t slab = slab_floats_of(n), need = grid * slab * (int64_t)sizeof(float);
  if (workspace_bytes < need) return CGNN_EINVAL;
  if (cgnn_overlap(workspace, need, matrices, bytes) || cgnn_overlap(workspace, need, out, bytes)) return CGNN_EINVAL;
  if (thresholds && cgnn_overlap(thresholds, S * (int64_t)sizeof(float), out, bytes)) return CGNN_EINVAL;
  k_mst<<<grid, kThreads, 0, cgnn_stream(stream)>>>(matrices, S, n, thresholds, static_cast<float*>(workspace), slab,
                                                    out);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
