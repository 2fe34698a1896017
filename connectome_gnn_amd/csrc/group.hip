// group.hip -- the group-level matrix of a device-resident cohort of connectivity matrices (float [S, n, n]) and the mask
// that gives every subject the group's edge set (include/cgnn_group.h): cgnn_ingest_group,
// cgnn_ingest_group_mask.  Both are bound by HBM traffic: the cohort is read once (and, by the mask, written once),
// 16 bytes a lane, several units in flight per lane.
//
//   k_group_partial<STAT>  the work items are (slice c of kSlice consecutive units, block b of 1024 consecutive entries of
//               the n * n), item = c * blocks + b, walked with a grid stride.  A lane owns the 4 consecutive entries
//               4 (256 b + thread) .. + 3 and their fp64 accumulators, which start at 0.0 and take the slice's included
//               units in ascending order: the partial of (slice, entry) does not depend on who computes it.  Units are
//               loaded kUnroll at a time so that their loads are in flight together; `among` (wave-uniform) and the edge
//               predicate are tests.  The partials go to the workspace [slices][n * n] as fp64, the number of included
//               units of a slice (written by the item of block 0) behind them, [slices].
//   k_group_fold<STAT>     a thread per entry: the partials and the counts in ascending slice order from 0.0, one fp64
//               division, the statistic's map, one rounding to fp32.
//   k_group_mask<NB>       the cohort is walked as a copy walks it: the work items are (unit s, span of NB blocks of 1024
//               consecutive entries), item = s * spans + span, with a grid stride.  A lane moves 4 entries in each of the
//               span's blocks, all loads in flight together, and decides each under the diagonal test and the edge
//               predicate of the group matrix at thr[0]; the group matrix (n * n floats against S n * n) is read along and
//               stays in cache.  NB = 4, but a unit of at most 8 blocks (n <= 90) is one item of exactly its blocks, so
//               that only the unit's last block has idle lanes.  (Items that keep a lane on its entries over many units,
//               as the reduce must, decide the group's entries once but write 4 KB pieces half a megabyte apart; with an
//               integer division per 16 bytes that form measured 1.27 x the copy at 360 ROIs, this one 1.07 x, DESIGN.md
//               4.3v.)  Every entry is read and written by the same lane, and a lane's loads stand before its stores:
//               out == matrices is safe.
//
// No atomics and no work assignment that decides a bit: the same bits every run and for every grid.  A unit's base is
// only 4-byte aligned when n * n is odd: 16-byte accesses are declared at element alignment (ingest_rows.h).  Element
// offsets are 64-bit.
#include <math.h>

#include "common.h"
#include "ingest_rows.h"
#include "measure_request.h"

namespace {

constexpr int kThreads = 256;                 // 4 waves
constexpr int kSlice = CGNN_GROUP_SLICE;
constexpr int kBlock = 4 * kThreads;          // entries of an item
constexpr int kUnroll = 8;                    // units in flight per lane: 8 KB a wave
constexpr int kWgPerCu = 8;                   // 32 waves a CU
constexpr int kMaskBlocks = 4;                // the mask: blocks of one unit a workgroup moves at a time, in flight together
constexpr int kMaskMaxBlocks = 8;             // ... a unit of no more blocks than this is one item, so that few lanes idle
static_assert(kSlice == CGNN_WAVE && kSlice % kUnroll == 0, "a wave's ballot holds a slice; a slice is whole batches");

typedef cgnn_f32x4 f32x4;
typedef cgnn_f32x4_e f32x4_e;

__host__ __device__ inline int64_t slices_of(int64_t S) { return (S + kSlice - 1) / kSlice; }
inline int64_t blocks_of(int64_t nn) { return (nn + kBlock - 1) / kBlock; }

// 4 consecutive entries of a unit from entry e0 on, streamed; what lies past the unit's end reads as -inf and is never stored
__device__ __forceinline__ f32x4 load4(const float* A, int64_t e0, int64_t nn) {
  if (e0 + 4 <= nn) return __builtin_nontemporal_load(reinterpret_cast<const f32x4_e*>(A + e0));
  f32x4 v = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (e0 + q < nn) v[q] = __builtin_nontemporal_load(A + e0 + q);
  return v;
}

// e mod m for 0 <= e < 2^31 and 1 < m < 2^17 without an integer division (which costs as much as streaming 16 bytes
// does): the fp64 quotient is off by one at most, which the two corrections take back.  inv_m = 1.0 / m.
__device__ __forceinline__ int remainder_of(int e, int m, double inv_m) {
  int r = e - (int)((double)e * inv_m) * m;
  if (r < 0) r += m;
  if (r >= m) r -= m;
  return r;
}

// whether entries e0 .. e0 + 3 of an n x n matrix lie off the diagonal, from r = e0 mod m, m = n + 1
__device__ __forceinline__ void off_diagonal4(int r, int m, bool (&off)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int d = r + q;                             // (d <= n + 3: at most two periods past, for n == 1)
    if (d >= m) d -= m;
    if (d >= m) d -= m;
    off[q] = d != 0;
  }
}

template <int STAT>
__global__ __launch_bounds__(kThreads) void k_group_partial(const float* __restrict__ matrices, int64_t S, int n,
                                                            const float* __restrict__ thr,
                                                            const uint8_t* __restrict__ among,
                                                            double* __restrict__ partial, double* __restrict__ counts) {
  const int64_t nn = (int64_t)n * n;
  const int64_t blocks = (nn + kBlock - 1) / kBlock, items = slices_of(S) * blocks;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t c = item / blocks, b = item - c * blocks;
    const int64_t s0 = c * kSlice, s1 = s0 + kSlice < S ? s0 + kSlice : S;
    // the slice's included units as a bit mask, one load per item: lane l of every wave answers for unit s0 + l
    const int64_t sl = s0 + (threadIdx.x & 63);
    const uint64_t inc = __ballot(sl < s1 && (!among || among[sl]));
    if (b == 0 && threadIdx.x == 0) counts[c] = (double)__popcll(inc);
    const int64_t e0 = b * kBlock + 4 * (int64_t)threadIdx.x;
    if (e0 >= nn) continue;                    // (no barrier in this kernel)
    bool off[4];                               // CONSISTENCY: the entry is not on the diagonal
    off_diagonal4((int)e0 % (n + 1), n + 1, off);                        // (once per kSlice units)
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t sb = s0; sb < s1; sb += kUnroll) {
      f32x4 x[kUnroll];
      bool in[kUnroll];
      float t[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t s = sb + u;
        in[u] = (inc >> (s - s0)) & 1;                                   // (uniform over the workgroup)
        x[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        t[u] = 0.0f;
        if (in[u]) {
          x[u] = load4(matrices + s * nn, e0, nn);
          if (STAT == CGNN_GROUP_CONSISTENCY) t[u] = thr[s];
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (!in[u]) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (STAT == CGNN_GROUP_MEAN) acc[q] += (double)x[u][q];
          if (STAT == CGNN_GROUP_FISHER_MEAN) acc[q] += atanh((double)x[u][q]);
          if (STAT == CGNN_GROUP_CONSISTENCY) acc[q] += (off[q] && cgnn_kept(x[u][q], t[u])) ? 1.0 : 0.0;
        }
      }
    }
    double* p = partial + c * nn + e0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (e0 + q < nn) p[q] = acc[q];
  }
}

template <int STAT>
__global__ __launch_bounds__(kThreads) void k_group_fold(const double* __restrict__ partial,
                                                         const double* __restrict__ counts, int64_t slices, int64_t nn,
                                                         float* __restrict__ out) {
  for (int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x; e < nn; e += (int64_t)gridDim.x * kThreads) {
    double sum = 0.0, N = 0.0;
#pragma unroll 8
    for (int64_t c = 0; c < slices; ++c) {
      sum += partial[c * nn + e];
      N += counts[c];
    }
    const double v = sum / N;
    out[e] = (float)(STAT == CGNN_GROUP_FISHER_MEAN ? tanh(v) : v);
  }
}

template <int NB>
__global__ __launch_bounds__(kThreads) void k_group_mask(const float* matrices, int64_t S, int n,
                                                         const float* __restrict__ group,
                                                         const float* __restrict__ thr, float* out) {
  const int64_t nn = (int64_t)n * n;
  constexpr int kSpan = NB * kBlock;
  const int64_t spans = (nn + kSpan - 1) / kSpan, items = S * spans;
  const float t = thr[0];
  const int m = n + 1, step = kBlock % m;      // the diagonal is every m-th entry; a block further, e mod m moves by step
  const double inv_m = 1.0 / m;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t s = item / spans, base = (item - s * spans) * kSpan + 4 * (int64_t)threadIdx.x;
    int r = base < nn ? remainder_of((int)base, m, inv_m) : 0;
    const float* A = matrices + s * nn;
    float* B = out + s * nn;
    f32x4 x[NB], g[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {    // every load of the lane stands before its first store
      const int64_t e0 = base + u * kBlock;
      if (e0 < nn) {
        x[u] = load4(A, e0, nn);
        g[u] = cgnn_load_row4(group, (int)e0, (int)nn);                // (from cache; past the end: -inf, never an edge)
      }
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int64_t e0 = base + u * kBlock;
      if (e0 >= nn) continue;
      bool off[4];
      off_diagonal4(r, m, off);
      r += step;
      if (r >= m) r -= m;
      f32x4 y;
#pragma unroll
      for (int q = 0; q < 4; ++q) y[q] = (off[q] && cgnn_kept(g[u][q], t) && x[u][q] > 0.0f) ? x[u][q] : 0.0f;
      if (e0 + 4 <= nn) {
        __builtin_nontemporal_store(y, reinterpret_cast<f32x4_e*>(B + e0));
      } else {
#pragma unroll
        for (int q = 0; q < 3; ++q)
          if (e0 + q < nn) B[e0 + q] = y[q];
      }
    }
  }
}

bool known(int32_t statistic) {
  return statistic == CGNN_GROUP_MEAN || statistic == CGNN_GROUP_FISHER_MEAN || statistic == CGNN_GROUP_CONSISTENCY;
}

int64_t workspace_bytes(int64_t S, int32_t n) {
  const int64_t slices = slices_of(S);
  return cgnn_align_up((slices * n * n + slices) * (int64_t)sizeof(double), 16);
}

}  // namespace

extern "C" int64_t cgnn_ingest_group_workspace_bytes(int64_t S, int32_t n) {
  if (cgnn_check_cohort(S, n) != CGNN_OK) return CGNN_EINVAL;
  return workspace_bytes(S, n);
}

extern "C" int cgnn_ingest_group(const float* matrices, int64_t S, int32_t n, int32_t statistic, const float* thr,
                                 const uint8_t* among, void* workspace, int64_t workspace_bytes_, float* out,
                                 int64_t out_bytes, void* stream) {
  if (!known(statistic) || cgnn_check_cohort(S, n) != CGNN_OK) return CGNN_EINVAL;
  if ((statistic == CGNN_GROUP_CONSISTENCY) != (thr != nullptr)) return CGNN_EINVAL;
  const int64_t nn = (int64_t)n * n, need = workspace_bytes(S, n);
  const int64_t cohort_bytes = S * nn * (int64_t)sizeof(float), group_bytes = nn * (int64_t)sizeof(float);
  if (!out || out_bytes < group_bytes || workspace_bytes_ < need) return CGNN_EINVAL;
  if (S > 0 && (!matrices || !workspace)) return CGNN_EINVAL;
  if (cgnn_misaligned({matrices, thr, out}, 3) || cgnn_misaligned({workspace}, 15)) return CGNN_EINVAL;
  if (S > 0) {
    if (matrices != out && cgnn_overlap(matrices, cohort_bytes, out, group_bytes)) return CGNN_EINVAL;
    if (cgnn_overlap(workspace, need, out, group_bytes) || cgnn_overlap(workspace, need, matrices, cohort_bytes))
      return CGNN_EINVAL;
    if (thr && cgnn_overlap(thr, S * (int64_t)sizeof(float), out, group_bytes)) return CGNN_EINVAL;
    if (among && cgnn_overlap(among, S, out, group_bytes)) return CGNN_EINVAL;
  }
  hipStream_t st = cgnn_stream(stream);
  const int64_t slices = slices_of(S);
  double* partial = static_cast<double*>(workspace);
  double* counts = partial + slices * nn;
  if (S > 0) {
    const int grid = cgnn_grid_for(slices * blocks_of(nn), kWgPerCu);
    switch (statistic) {
      case CGNN_GROUP_MEAN:
        k_group_partial<CGNN_GROUP_MEAN><<<grid, kThreads, 0, st>>>(matrices, S, n, thr, among, partial, counts);
        break;
      case CGNN_GROUP_FISHER_MEAN:
        k_group_partial<CGNN_GROUP_FISHER_MEAN><<<grid, kThreads, 0, st>>>(matrices, S, n, thr, among, partial, counts);
        break;
      default:
        k_group_partial<CGNN_GROUP_CONSISTENCY><<<grid, kThreads, 0, st>>>(matrices, S, n, thr, among, partial, counts);
        break;
    }
    CGNN_CHECK_LAUNCH();
  }
  const int grid = cgnn_grid_for((nn + kThreads - 1) / kThreads, kWgPerCu);
  if (statistic == CGNN_GROUP_FISHER_MEAN)
    k_group_fold<CGNN_GROUP_FISHER_MEAN><<<grid, kThreads, 0, st>>>(partial, counts, slices, nn, out);
  else
    k_group_fold<CGNN_GROUP_MEAN><<<grid, kThreads, 0, st>>>(partial, counts, slices, nn, out);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

extern "C" int cgnn_ingest_group_mask(const float* matrices, int64_t S, int32_t n, const float* group, const float* thr,
                                      float* out, int64_t out_bytes, void* stream) {
  if (const int rc = cgnn_check_cohort(S, n)) return rc;
  if (S == 0) return CGNN_OK;
  if (!matrices || !group || !thr || !out || cgnn_misaligned({matrices, group, thr, out}, 3)) return CGNN_EINVAL;
  if (cgnn_check_cohort_out(matrices, out, out_bytes, S, n) != CGNN_OK) return CGNN_EINVAL;
  const int64_t nn = (int64_t)n * n, cohort_bytes = S * nn * (int64_t)sizeof(float);
  if (cgnn_overlap(group, nn * (int64_t)sizeof(float), out, cohort_bytes) ||
      cgnn_overlap(thr, sizeof(float), out, cohort_bytes))
    return CGNN_EINVAL;
  const int64_t blocks = blocks_of(nn);
  const int nb = blocks <= kMaskMaxBlocks ? (int)blocks : kMaskBlocks;
  const int grid = cgnn_grid_for(S * ((blocks + nb - 1) / nb), kWgPerCu);
  hipStream_t st = cgnn_stream(stream);
  switch (nb) {
#define CGNN_GROUP_MASK_CASE(NB) \
  case NB: k_group_mask<NB><<<grid, kThreads, 0, st>>>(matrices, S, n, group, thr, out); break;
    CGNN_GROUP_MASK_CASE(1) CGNN_GROUP_MASK_CASE(2) CGNN_GROUP_MASK_CASE(3) CGNN_GROUP_MASK_CASE(4)
    CGNN_GROUP_MASK_CASE(5) CGNN_GROUP_MASK_CASE(6) CGNN_GROUP_MASK_CASE(7) CGNN_GROUP_MASK_CASE(8)
#undef CGNN_GROUP_MASK_CASE
  }
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
