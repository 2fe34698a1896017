// timeseries.hip -- a device-resident cohort of ROI time series (float [S, T, n], one row per frame) turned into
// Pearson correlation matrices (float [U, n, n]), whole runs or sliding windows: cgnn_ingest_corr.
//
// A unit u = s * W + w is subject s, frames [w * stride, w * stride + L); W = 1 and L = T without a window.
// Per unit: m_i = the mean of column i, q_i = sum_t (x[t,i] - m_i)^2, both in fp64 as centred sums (blocked Welford);
// r[i,j] = sum_t z[t,i] z[t,j] with z[t,i] = (x[t,i] - m_i) / sqrt(q_i), centred and scaled in fp32 as the
// operands are staged; 1/sqrt(0) is taken as 0, so a constant column gives a zero row and column.
//
//   k_corr_stats   the stream of frame_mask.h: a workgroup of 4 waves per (unit, 64 columns), lane = column, wave =
//                  frame phase.  A thread centres 8 frames at a time in registers (their mean, then their centred
//                  squares, fp64) and merges the block into its running (count, mean, centred sum) by the pairwise
//                  update of Chan et al.; the four waves' moments merge the same way through LDS, in wave order.  One
//                  read of every frame, no E[x^2] - E[x]^2 anywhere; a constant column gives q = 0 exactly.  Writes
//                  stats[u, i] = (m_i, 1/sqrt(q_i)) as floats.
//   k_corr<vec>    r = Z^T Z on the tile walk of gram_tile.h (96 x 96 outputs per item, the frames 32 at a time on
//                  v_mfma_f32_16x16x4_f32; the design is told there).  Stage: the column statistics of the
//                  item's two tiles wait in LDS, an entry is centred and scaled in fp32 on its way into the
//                  panel, frames past L become zeros.
//                  Epilogue: clamp to [-1, 1], |.| if asked, store r[i,j] and its mirror r[j,i] from the same
//                  register; in a diagonal tile only i <= j is stored (and mirrored), and r[i,i] is written as
//                  1 (0 for a constant column) -- so the matrix is bit-symmetric by construction.
//
// cgnn_ingest_corr_masked is the same with a frame mask keep [S, T]: a unit's frames are its window's
// kept ones.  The mask is a template argument of both kernels and the predicate of frame_mask.h: in k_corr_stats a
// block's count is its kept frames and the waves' counts go through LDS; in k_corr a censored frame is staged as a zero
// row (the 32 flags of a step are one ballot, fetched a step ahead).  The unmasked instantiations keep their code.
//
// Accumulation is fp32 over the frames in ascending order, no atomics: the same bits on every run and for every
// grid.  Frames past L and columns past n are zeros in LDS and are never read from memory.  Element offsets
// into `ts` and `out` are 64-bit.
#include <math.h>

#include "frame_mask.h"
#include "gram_tile.h"
#include "series_request.h"

namespace {

using namespace gram;
static_assert(kKS == 32, "k_corr<., true> keeps the flags of a step in one 32-bit ballot");

// (count, mean, centred sum of squares) of two disjoint sets of samples -> of their union (Chan et al.)
__device__ __forceinline__ void merge_moments(int& cnt, double& mean, double& m2, int cb, double mb, double m2b) {
  if (cb == 0) return;
  const int tot = cnt + cb;
  const double d = mb - mean, f = (double)cb / (double)tot;
  mean += d * f;
  m2 += m2b + d * d * ((double)cnt * f);
  cnt = tot;
}

// The column statistics, on the stream of frame_mask.h: a block of frames is centred in registers and merged into the
// thread's running moments, then the four waves' moments in wave order.  kMask: `keep` [S, T] selects
// the frames.  A unit's frames are its window's kept ones: a censored frame is in no count, and the waves' counts go
// through LDS instead of being derived from L.
struct Moments {
  int cnt = 0;
  double mean = 0.0, m2 = 0.0;
};

template <bool kMask>
__global__ __launch_bounds__(kStreamThreads) void k_corr_stats(const float* __restrict__ ts, int64_t U, int T, int n,
                                                             int W, int L, int stride, float* __restrict__ stats,
                                                             const uint8_t* __restrict__ keep) {
  __shared__ double part[2][kStreamWaves][kStreamCols];
  cgnn_stream_columns<kMask, Moments>(
      ts, keep, U, T, n, W, L, stride,
      [](Moments& a, const float (&v)[kStreamBlock], unsigned bits, int frames) {
        const int cb = kMask ? __builtin_popcount(bits) : frames;
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < kStreamBlock; ++i)          // (the padding adds zeros; a censored frame is left out)
          sum += !kMask || ((bits >> i) & 1) ? (double)v[i] : 0.0;
        const double mb = sum / (double)cb;     // (cb == 0: nothing of this block is merged)
        double m2b = 0.0;
#pragma unroll
        for (int i = 0; i < kStreamBlock; ++i) {
          const double d = (double)v[i] - mb;
          if (kMask ? (bits >> i) & 1 : i < cb) m2b += d * d;
        }
        merge_moments(a.cnt, a.mean, a.m2, cb, mb, m2b);
      },
      [&](Moments a, int64_t u, int col, bool act, int lane, int wave) {
        part[0][wave][lane] = a.mean;
        part[1][wave][lane] = a.m2;
        if constexpr (kMask) {
          __shared__ int counts[kStreamWaves][kStreamCols];
          counts[wave][lane] = a.cnt;
          __syncthreads();
          if (wave == 0 && act)
            for (int k = 1; k < kStreamWaves; ++k)
              merge_moments(a.cnt, a.mean, a.m2, counts[k][lane], part[0][k][lane], part[1][k][lane]);
        } else {
          __syncthreads();
          if (wave == 0 && act)                    // the four waves' moments, in wave order
            for (int k = 1; k < kStreamWaves; ++k) {
              const int ck = k < L ? (L - k + 3) / 4 : 0;
              merge_moments(a.cnt, a.mean, a.m2, ck, part[0][k][lane], part[1][k][lane]);
            }
        }
        if (wave == 0 && act) {
          float* __restrict__ o = stats + (u * n + col) * 2;
          o[0] = (float)a.mean;
          o[1] = a.m2 == 0.0 ? 0.0f : (float)(1.0 / sqrt(a.m2));   // (a NaN stays a NaN)
        }
        __syncthreads();
      });
}

struct alignas(16) CorrShared {
  Panels panel;                               // the rows k are the frames of the window
  float mean[2][kTile];
  float rstd[2][kTile];
};

// kMask: a censored frame of the window is staged as a zero row, whatever it holds
template <bool kVec, bool kMask>
__global__ __launch_bounds__(kThreads) void k_corr(const float* __restrict__ ts, int64_t U, int T, int n, int W, int L,
                                                   int stride, int absolute, const float* __restrict__ stats,
                                                   float* __restrict__ out, const uint8_t* __restrict__ keep) {
  __shared__ CorrShared sh;
  const Thread th;
  const int nt = tiles_of(n);
  const int64_t items = U * pairs_of(nt);

  for (int64_t item = first_item(); item < items; item += gridDim.x) {
    const Item it(item, nt, th.wave);
    const int64_t u = it.unit, first = cgnn_first_frame(u, W, T, stride);
    const float* __restrict__ x = ts + first * n;
    const cgnn_frame_mask<kMask> mask(keep, first, L);

    __syncthreads();                          // the previous item's epilogue still reads sh.rstd
    if (th.tid < 2 * kTile) {
      const int side = th.tid / kTile, c = th.tid - side * kTile;
      const int col = it.col0(side) + c;
      float m = 0.f, r = 0.f;
      if (col < n) {
        const float* __restrict__ st = stats + (u * n + col) * 2;
        m = st[0];
        r = st[1];
      }
      sh.mean[side][c] = m;
      sh.rstd[side][c] = r;
    }
    f32x4 pre[2][kSlots], acc[3][3];
    load_panels<kVec>(pre, x, L, n, 0, it, th);
    // kMask: the 32 flags of a step are one ballot.  Lane l fetches the flag of frame k0 + (l & 31) a step ahead -- when
    // the step before it is staged, so the load flies under that step's MFMAs -- and the first slot staged of a step
    // turns the fetched flags into the step's bits.
    bool flag = false;
    uint64_t bits = 0;
    int bits_k0 = -1;
    auto fetch = [&](int k0) { flag = mask.kept(k0 + (th.tid & 31)); };
    if constexpr (kMask) fetch(0);
    __syncthreads();

    // centred and scaled; frames past L become zeros
    run<kVec>(sh.panel, pre, acc, x, L, n, it, th, [&](int side, int t, int c, f32x4 v) {
      const f32x4 m = *reinterpret_cast<const f32x4*>(&sh.mean[side][c]);
      const f32x4 r = *reinterpret_cast<const f32x4*>(&sh.rstd[side][c]);
      f32x4 z = {0.f, 0.f, 0.f, 0.f};
      bool in = t < L;
      if constexpr (kMask) {
        if ((t & ~31) != bits_k0) {           // (uniform: every thread stages the same step)
          bits_k0 = t & ~31;
          bits = __ballot(flag);
          fetch(bits_k0 + kKS);
        }
        in = (bits >> (t & 31)) & 1;          // (a frame past L has no flag set)
      }
      if (in) z = (v - m) * r;
      return z;
    });

    float* __restrict__ o = out + u * (int64_t)n * n;
    for_each_block(it, th, [&](int a, int b, bool tri, int li0, int gi0, int gj) {
      f32x4 v = acc[a][b];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float c = v[r];
        c = c > 1.0f ? 1.0f : (c < -1.0f ? -1.0f : c);       // (a NaN stays a NaN)
        if (absolute) c = fabsf(c);
        if (tri && gi0 + r == gj) {
          const float rs = sh.rstd[0][li0 + r];
          c = rs == 0.0f ? 0.0f : (rs != rs ? rs : 1.0f);
        }
        v[r] = c;
      }
      if (gj >= n) return;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (gi0 + r < n && (!tri || gi0 + r <= gj)) o[(int64_t)(gi0 + r) * n + gj] = v[r];
      if (kVec && !tri) {
        if (gi0 < n) *reinterpret_cast<f32x4*>(&o[(int64_t)gj * n + gi0]) = v;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (gi0 + r < n && (!tri || gi0 + r < gj)) o[(int64_t)gj * n + gi0 + r] = v[r];
      }
    });
  }
}

// Persistent grids, in workgroups per CU: the product kernel's 57 KB of LDS admit two workgroups (a wave of each
// per SIMD); the statistics pass is a stream and wants every wave the CU holds (4 per SIMD at its 110 VGPRs).
#ifndef CGNN_CORR_WG_PER_CU
#define CGNN_CORR_WG_PER_CU 2
#endif
#ifndef CGNN_CORR_STATS_PER_CU
#define CGNN_CORR_STATS_PER_CU 4
#endif

template <bool kMask>
int launch(const float* ts, const cgnn_units& un, int32_t T, int32_t n, int32_t absolute, const uint8_t* keep, float* stats,
           float* out, hipStream_t hs) {
  const int64_t chunks = (n + kStreamCols - 1) / kStreamCols;
  k_corr_stats<kMask><<<cgnn_grid_for(un.U * chunks, CGNN_CORR_STATS_PER_CU), kStreamThreads, 0, hs>>>(
      ts, un.U, T, n, (int)un.W, un.L, un.st, stats, keep);
  CGNN_CHECK_LAUNCH();
  const int grid = cgnn_grid_for(un.U * pairs_of(tiles_of(n)), CGNN_CORR_WG_PER_CU);
  if (n % 4 == 0 && !cgnn_misaligned({ts, out}, 15))
    k_corr<true, kMask><<<grid, kThreads, 0, hs>>>(ts, un.U, T, n, (int)un.W, un.L, un.st, absolute, stats, out, keep);
  else
    k_corr<false, kMask><<<grid, kThreads, 0, hs>>>(ts, un.U, T, n, (int)un.W, un.L, un.st, absolute, stats, out, keep);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

// what both entry points check and do; masked: keep [S, T] selects the frames
int corr_call(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride, int32_t absolute,
              const uint8_t* keep, int64_t keep_bytes, bool masked, float* stats, int64_t stats_bytes, float* out,
              int64_t out_bytes, void* stream) {
  cgnn_units un;
  if (cgnn_check_cohort(S, n) != CGNN_OK || cgnn_check_units(S, T, n, window, stride, &un) != CGNN_OK) return CGNN_EINVAL;
  if (keep_bytes < 0) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (!ts || !stats || !out || cgnn_misaligned({ts, stats, out}, 3) || (masked && !keep)) return CGNN_EINVAL;
  CGNN_NEED_BYTES(keep, keep_bytes, S * (int64_t)T);
  CGNN_NEED_BYTES(stats, stats_bytes, un.U * n * 2 * (int64_t)sizeof(float));
  CGNN_NEED_BYTES(out, out_bytes, un.U * n * (int64_t)n * (int64_t)sizeof(float));
  return masked ? launch<true>(ts, un, T, n, absolute, keep, stats, out, cgnn_stream(stream))
                : launch<false>(ts, un, T, n, absolute, nullptr, stats, out, cgnn_stream(stream));
}

}  // namespace

extern "C" int cgnn_ingest_corr(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride,
                                int32_t absolute, float* stats, int64_t stats_bytes, float* out, int64_t out_bytes,
                                void* stream) {
  return corr_call(ts, S, T, n, window, stride, absolute, nullptr, 0, false, stats, stats_bytes, out, out_bytes, stream);
}

// frame censoring: the same two launches over the frames keep [S, T] selects
extern "C" int cgnn_ingest_corr_masked(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride,
                                       int32_t absolute, const uint8_t* keep, int64_t keep_bytes, float* stats,
                                       int64_t stats_bytes, float* out, int64_t out_bytes, void* stream) {
  return corr_call(ts, S, T, n, window, stride, absolute, keep, keep_bytes, true, stats, stats_bytes, out, out_bytes,
                   stream);
}
