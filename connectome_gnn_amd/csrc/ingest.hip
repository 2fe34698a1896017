// ingest.hip -- a device-resident cohort of dense connectivity matrices (float [S, n, n]) thresholded to its
// strongest connections and turned into the flat edge arrays of a RaggedPackedDataset:
// cgnn_ingest_select / cgnn_ingest_count / cgnn_ingest_fill.
//
// Semantics per subject: candidates are the n(n-1) off-diagonal entries, a NaN ranks as -inf; the threshold t
// is the candidate of descending rank k (0-based; -inf for k >= n(n-1)) or is given; i -> j is an edge iff
// i != j, A[i,j] > t and A[i,j] > 0 (float comparisons, both strict); edges leave in row-major order.
//
//   k_ingest<select, count>   one workgroup of 8 waves OWNS a subject; 3 per CU walk the subjects with a grid stride.
//       select: exact k-th largest by a radix select on an order-preserving uint32 image of the floats
//               (NaN -> key 0), three passes of 11 / 11 / 10 bits over the subject's flat n*n floats, the
//               histogram in LDS (ds_add; four copies by lane to thin same-address adds out, and a wave whose
//               lanes all hit one bin adds once).  No sort, no workspace: the only output is thr[s].
//       count:  right behind it, while the subject is still in cache: a wave per row counts the kept entries
//               (row_count[s*n + i]) and sums them (the row's strength); the workgroup then takes the
//               maximum strength and writes x[s, i] = strength_i / (max + 1e-8).
//   k_ingest_fill             a wave per (subject, row), grid stride over all S*n rows: the row's kept
//               entries are placed from row_off[row] on in column order by ballot + lane prefix.
//
// Placement is a function of the data alone (no atomics on global memory, no scratch): same bits every run.
// A thread reads 4 consecutive floats with one 16-byte access declared at element alignment (rows and
// subjects start at multiples of 4 bytes only when n is odd); element offsets into `matrices` are 64-bit.
#include <math.h>

#include "common.h"
#include "ingest_rows.h"

namespace {

constexpr int kThreads = 512;                 // k_ingest: 8 waves
constexpr int kWaves = kThreads / 64;
constexpr int kBins = 2048;                   // 11-bit digits
constexpr int kCopies = 4;                    // histogram copies, chosen by lane & 3
constexpr int kPerThread = kBins / kThreads;  // bins a thread scans
constexpr int kFillThreads = 256;             // k_ingest_fill: 4 waves, a row each
static_assert(kPerThread * kThreads == kBins, "every bin has one owner");

typedef cgnn_f32x4 f32x4;
typedef cgnn_f32x4_e f32x4_e;                           // 16 bytes at element alignment

// floats -> uint32 keys of the same order; every NaN is the smallest key
__device__ __forceinline__ uint32_t key_of(float v) {
  const uint32_t u = __float_as_uint(v);
  if (v != v) return 0u;
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t key) {
  if (key == 0u) return -INFINITY;            // the rank fell on a NaN
  return __uint_as_float((key >> 31) ? (key ^ 0x80000000u) : ~key);
}
// THE edge predicate (diagonal aside) and the row reads, the same expressions in count, fill and measures.hip
// (ingest_rows.h)
__device__ __forceinline__ bool kept(float v, float t) { return cgnn_kept(v, t); }
__device__ __forceinline__ f32x4 load_row4(const float* __restrict__ row, int j0, int n) {
  return cgnn_load_row4(row, j0, n);
}

struct SelectShared {
  uint32_t hist[kCopies * kBins];
  uint32_t wave_tot[kWaves];
  uint32_t sel[2];
  float wave_max[kWaves];
};

// one digit of one candidate into the histogram
__device__ __forceinline__ void hist_add(uint32_t* hist, bool act, uint32_t d, int lane) {
  const uint64_t am = __ballot(act);
  if (am == 0) return;
  const int leader = __ffsll((unsigned long long)am) - 1;
  const uint32_t d0 = (uint32_t)__shfl((int)d, leader, 64);
  const uint64_t same = __ballot(act && d == d0);
  if (same == am) {                            // the whole wave in one bin: one add
    if (lane == leader) atomicAdd(&hist[(lane & (kCopies - 1)) * kBins + d0], (uint32_t)__popcll(am));
  } else if (act) {
    atomicAdd(&hist[(lane & (kCopies - 1)) * kBins + d], 1u);
  }
}

// The key of descending rank `rank` (< the number of candidates) among the off-diagonal entries of A [n, n].
__device__ uint32_t select_key(const float* __restrict__ A, int n, uint32_t rank, SelectShared& sh) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t nn = (uint32_t)n * (uint32_t)n, np1 = (uint32_t)n + 1u;
  const uint32_t step = (4u * kThreads) % np1;
  uint32_t prefix = 0u, pmask = 0u;
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
    const uint32_t dmask = pass == 2 ? 0x3FFu : 0x7FFu;
    for (int i = t; i < kCopies * kBins; i += kThreads) sh.hist[i] = 0u;
    __syncthreads();
    uint32_t rd = (4u * (uint32_t)t) % np1;    // flat index mod (n+1): 0 on the diagonal
    for (uint32_t e0 = 4u * (uint32_t)t; e0 < nn; e0 += 4u * kThreads) {
      f32x4 v;
      if (e0 + 4u <= nn) {
        v = *reinterpret_cast<const f32x4_e*>(A + e0);
      } else {
        v = f32x4{0.f, 0.f, 0.f, 0.f};
        for (uint32_t q = 0; q < 4u; ++q) if (e0 + q < nn) v[q] = A[e0 + q];
      }
#pragma unroll
      for (uint32_t q = 0; q < 4u; ++q) {
        uint32_t m = rd + q;
        if (m >= np1) m -= np1;
        if (m >= np1) m -= np1;
        const uint32_t key = key_of(v[q]);
        const bool act = e0 + q < nn && m != 0u && (key & pmask) == prefix;
        hist_add(sh.hist, act, (key >> shift) & dmask, lane);
      }
      rd += step;
      if (rd >= np1) rd -= np1;
    }
    __syncthreads();
    // bins from the top: thread t owns the reversed bins [kPerThread * t, kPerThread * (t + 1))
    uint32_t c[kPerThread], tsum = 0u;
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
      const int bin = kBins - 1 - (kPerThread * t + q);
      uint32_t s = 0u;
#pragma unroll
      for (int k = 0; k < kCopies; ++k) s += sh.hist[k * kBins + bin];
      c[q] = s;
      tsum += s;
    }
    uint32_t incl = tsum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (lane == 63) sh.wave_tot[wave] = incl;
    __syncthreads();
    uint32_t excl = incl - tsum;
    for (int w = 0; w < wave; ++w) excl += sh.wave_tot[w];
    if (excl <= rank && rank < excl + tsum) {  // exactly one thread: the rank lies in its bins
      uint32_t run = excl;
#pragma unroll
      for (int q = 0; q < kPerThread; ++q) {
        if (rank >= run && rank < run + c[q]) {
          sh.sel[0] = (uint32_t)(kBins - 1 - (kPerThread * t + q));
          sh.sel[1] = rank - run;
        }
        run += c[q];
      }
    }
    __syncthreads();
    prefix |= sh.sel[0] << shift;
    pmask |= dmask << shift;
    rank = sh.sel[1];
  }
  return prefix;
}

template <bool kSelect, bool kCount>
__global__ __launch_bounds__(kThreads) void k_ingest(const float* __restrict__ matrices, int64_t S, int n, int64_t k,
                                                     float* __restrict__ thr, int32_t* __restrict__ row_count,
                                                     float* __restrict__ x) {
  __shared__ SelectShared sh;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t m = (int64_t)n * (n - 1);
  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const float* __restrict__ A = matrices + s * (int64_t)n * n;
    float thr_s;
    if (kSelect) {
      thr_s = k >= m ? -INFINITY : value_of(select_key(A, n, (uint32_t)k, sh));
      if (t == 0) thr[s] = thr_s;
    } else {
      thr_s = thr[s];
    }
    if (!kCount) continue;
    float wmax = 0.0f;
    for (int i = wave; i < n; i += kWaves) {
      const float* __restrict__ row = A + (int64_t)i * n;
      int cnt;
      float sum, unused;
      cgnn_row_kept<false>(row, i, n, thr_s, lane, cnt, sum, unused);
      if (lane == 0) {
        row_count[s * n + i] = cnt;
        if (x) x[s * n + i] = sum;
      }
      wmax = fmaxf(wmax, sum);
    }
    if (x) {                                   // (wave-uniform) normalise by the subject's largest strength
      if (lane == 0) sh.wave_max[wave] = wmax;
      __threadfence_block();
      __syncthreads();                         // ... which also orders the strengths written above
      float mx = sh.wave_max[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) mx = fmaxf(mx, sh.wave_max[w]);
      for (int i = t; i < n; i += kThreads) x[s * n + i] = cgnn_strength_feature(x[s * n + i], mx);
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kFillThreads) void k_ingest_fill(const float* __restrict__ matrices, int64_t rows, int n,
                                                              const float* __restrict__ thr,
                                                              const int64_t* __restrict__ row_off, int64_t E,
                                                              int64_t* __restrict__ out0, int64_t* __restrict__ out1,
                                                              float* __restrict__ outw) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * (kFillThreads / 64) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (kFillThreads / 64);
  const uint64_t below = (1ull << lane) - 1ull;
  for (int64_t r = wave0; r < rows; r += nwaves) {
    const int64_t s = r / n;
    const int i = (int)(r - s * n);
    const float thr_s = thr[s];
    const float* __restrict__ row = matrices + r * (int64_t)n;
    int64_t base = row_off[r];
    for (int j0 = 4 * lane; j0 - 4 * lane < n; j0 += 256) {     // every lane runs every chunk (ballots)
      const f32x4 v = load_row4(row, j0, n);
      bool kq[4];
      uint64_t mq[4];
      int before = 0, total = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        kq[q] = j0 + q != i && kept(v[q], thr_s);
        mq[q] = __ballot(kq[q]);
        before += __popcll(mq[q] & below);
        total += __popcll(mq[q]);
      }
      int64_t pos = base + before;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (kq[q]) {
          if (pos >= 0 && pos < E) {             // offsets are the caller's: never write outside the arrays
            out0[pos] = i;
            out1[pos] = j0 + q;
            outw[pos] = v[q];
          }
          ++pos;
        }
      }
      base += total;
    }
  }
}

// the checks every entry point shares; CGNN_OK when there is something to launch
int check_cohort(const float* matrices, int64_t S, int32_t n) {
  if (cgnn_check_cohort(S, n) != CGNN_OK) return CGNN_EINVAL;
  if (S > 0 && (!matrices || (reinterpret_cast<uintptr_t>(matrices) & 3))) return CGNN_EINVAL;
  return CGNN_OK;
}

// Persistent grids, in workgroups per CU (overridable for A/B builds: make variant DEFS=-D...).  Both kernels are
// bound by latency, not bandwidth, so they want every wave the CU can hold: 3 x 8 waves is what k_ingest's
// registers admit (measured 4096 x 360, keep 0.1: 3.53 ms at 2, 3.19 at 3, 3.60 at 4 -- the fourth is not
// resident), 8 x 4 waves fills the CU for the fill.
#ifndef CGNN_INGEST_WG_PER_CU
#define CGNN_INGEST_WG_PER_CU 3
#endif
#ifndef CGNN_INGEST_FILL_PER_CU
#define CGNN_INGEST_FILL_PER_CU 8
#endif
int subject_grid(int64_t S) { return cgnn_grid_for(S, CGNN_INGEST_WG_PER_CU); }

}  // namespace

extern "C" int cgnn_ingest_select(const float* matrices, int64_t S, int32_t n, int64_t k, float* thr,
                                  int64_t thr_bytes, void* stream) {
  if (check_cohort(matrices, S, n) != CGNN_OK || k < 0) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (!thr) return CGNN_EINVAL;
  CGNN_NEED_BYTES(thr, thr_bytes, S * (int64_t)sizeof(float));
  k_ingest<true, false><<<subject_grid(S), kThreads, 0, cgnn_stream(stream)>>>(matrices, S, n, k, thr, nullptr, nullptr);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

extern "C" int cgnn_ingest_count(const float* matrices, int64_t S, int32_t n, int32_t select, int64_t k, float* thr,
                                 int64_t thr_bytes, int32_t* row_count, int64_t row_count_bytes, float* strength,
                                 int64_t strength_bytes, void* stream) {
  if (check_cohort(matrices, S, n) != CGNN_OK || k < 0) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (!thr || !row_count) return CGNN_EINVAL;
  CGNN_NEED_BYTES(thr, thr_bytes, S * (int64_t)sizeof(float));
  CGNN_NEED_BYTES(row_count, row_count_bytes, S * n * (int64_t)sizeof(int32_t));
  CGNN_NEED_BYTES(strength, strength_bytes, S * n * (int64_t)sizeof(float));
  hipStream_t st = cgnn_stream(stream);
  if (select)
    k_ingest<true, true><<<subject_grid(S), kThreads, 0, st>>>(matrices, S, n, k, thr, row_count, strength);
  else
    k_ingest<false, true><<<subject_grid(S), kThreads, 0, st>>>(matrices, S, n, k, thr, row_count, strength);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

extern "C" int cgnn_ingest_fill(const float* matrices, int64_t S, int32_t n, const float* thr, const int64_t* row_off,
                                int64_t num_edges, int64_t* edge_local, int64_t edge_local_bytes, float* edge_weight,
                                int64_t edge_weight_bytes, void* stream) {
  if (check_cohort(matrices, S, n) != CGNN_OK || num_edges < 0) return CGNN_EINVAL;
  if (S == 0 || num_edges == 0) return CGNN_OK;
  if (num_edges > S * (int64_t)n * (n - 1)) return CGNN_EINVAL;
  if (!thr || !row_off || !edge_local || !edge_weight) return CGNN_EINVAL;
  CGNN_NEED_BYTES(edge_local, edge_local_bytes, 2 * num_edges * (int64_t)sizeof(int64_t));
  CGNN_NEED_BYTES(edge_weight, edge_weight_bytes, num_edges * (int64_t)sizeof(float));
  const int64_t rows = S * (int64_t)n;
  const int64_t blocks = (rows + kFillThreads / 64 - 1) / (kFillThreads / 64);
  k_ingest_fill<<<cgnn_grid_for(blocks, CGNN_INGEST_FILL_PER_CU), kFillThreads, 0, cgnn_stream(stream)>>>(
      matrices, rows, n, thr, row_off, num_edges, edge_local, edge_local + num_edges, edge_weight);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
