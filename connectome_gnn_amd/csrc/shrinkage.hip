// shrinkage.hip -- the Ledoit-Wolf shrinkage of every unit of a device-resident cohort of ROI time series, for the
// correlation matrices cgnn_ingest_corr built from them: cgnn_ingest_shrinkage.
//
// The project correlates standardised series: z[t,i] = (x[t,i] - m_i) rs_i, rs_i = 1 / sqrt(q_i) (0 for a constant
// column), R = Z^T Z, diag R = 1.  For those Ledoit-Wolf's target mu I is the identity cgnn_ingest_partial shrinks
// towards, and the estimator is two scalars per unit of L frames:
//   p   = the number of columns with rs_i != 0
//   s_t = sum_i z[t,i]^2                                   B = L sum_t s_t^2
//   O   = 2 sum_{i<j} R_ij^2                                F = p + O
//   a   = 0 if O == 0, else (B - F) / (L O) clipped to [0, 1]; a NaN stays a NaN
// L == 2 makes every z[t,i] = +-1/sqrt(2) and every R_ij = +-1: B - F is zero identically, and what rounding leaves of
// it is no estimate, so a = 0 there (or NaN, if the quotient is).
//
//   k_lw   one launch.  A workgroup of 4 waves owns a unit, grid stride (units are defined as in timeseries.hip).
//     stage    the unit's statistics (m_i, rs_i) -> LDS (n <= 1024: the bound of the kernel the estimate feeds); p.
//     frames   wave = frame phase, as in k_corr_stats: wave w takes frames w, w + 4, ..., 8 of them at a time; lane =
//              column, lane + 64, ... (a wave reads 256 consecutive bytes of a frame).  z is formed in fp32 as k_corr
//              stages it, its square and everything after it in fp64.  The 8 s_t of a block are summed over the wave
//              together (wave_sum8: 10 exchanges, not 48) and land one per group of 8 lanes, which adds its s_t^2 to
//              the running sum of its slot.
//     triangle row i of R from column i + 1 on, 4 rows of a wave in flight; wave = row phase, lane = column phase; a
//              thread's sum of squares in fp64 in the order it reads, then the butterfly.  O is summed from the
//              off-diagonal entries themselves, never as F - p.
//     merge    the 4 x 8 slot sums and the four waves' triangle sums through LDS, in wave and slot order; thread 0
//              forms the quotient in fp64.
// cgnn_ingest_shrinkage_masked: with a frame mask keep [S, T] a unit's frames are its window's kept
// ones; the kernel counts them (L_u) and L_u stands wherever L does: B = L_u sum_{t kept} s_t^2, a = (B - F) / (L_u O),
// and L_u <= 2 gives 0.  The mask is a template argument and the predicate of frame_mask.h.
// No atomics, and no work assignment depends on the grid: the same bits on every run and for every grid.  Overlapping
// windows read their frames again (each window has statistics of its own).  Element offsets into `ts` and `matrices`
// are 64-bit.
#include <math.h>

#include "frame_mask.h"
#include "measure_request.h"
#include "series_request.h"

namespace {

constexpr int kLwThreads = 256;
constexpr int kLwWaves = kLwThreads / 64;
constexpr int kLwFrames = 8;                  // frames a wave has in flight
constexpr int kLwRows = 4;                    // rows of the triangle a wave has in flight

// The sums over the wave of v[0 .. 7], one per lane: lane l returns that of v[(l >> 3) & 7].  Three exchanges halve what
// a lane holds (it keeps the half its lane bit selects and adds the partner's), three more sum the one value left over
// the lanes that share it; the order is fixed, and the 8 lanes of a group return the same bits.
__device__ __forceinline__ double wave_sum8(const double (&v)[kLwFrames], int lane) {
  static_assert(kLwFrames == 8, "three halvings");
  double a[4], b[2];
  const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = (h5 ? v[i + 4] : v[i]) + __shfl_xor(h5 ? v[i] : v[i + 4], 32, 64);
#pragma unroll
  for (int i = 0; i < 2; ++i) b[i] = (h4 ? a[i + 2] : a[i]) + __shfl_xor(h4 ? a[i] : a[i + 2], 16, 64);
  double c = (h3 ? b[1] : b[0]) + __shfl_xor(h3 ? b[0] : b[1], 8, 64);
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}

// kMask: `keep` [S, T] selects the frames; a unit's frames are its window's kept ones, L_u of them,
// counted here, and L_u stands wherever L does in the estimate.  A censored frame's values are loaded beside its flag and
// left out by selection.
template <bool kMask>
__global__ __launch_bounds__(kLwThreads) void k_lw(const float* __restrict__ ts, int64_t U, int T, int n, int W, int L,
                                                   int stride, const float* __restrict__ stats,
                                                   const float* __restrict__ matrices, double* __restrict__ alpha,
                                                   const uint8_t* __restrict__ keep) {
  __shared__ float mean[CGNN_PARTIAL_MAX_NODES], rstd[CGNN_PARTIAL_MAX_NODES];
  __shared__ double part_b[kLwWaves][kLwFrames], part_o[kLwWaves];
  __shared__ int kept[kLwWaves], frames[kLwWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = (lane >> 3) & 7;           // the frame of a block whose sum wave_sum8 hands this lane

  for (int64_t u = blockIdx.x; u < U; u += gridDim.x) {
    const int64_t first = cgnn_first_frame(u, W, T, stride);
    const float* __restrict__ x = ts + first * n;
    const float* __restrict__ R = matrices + u * (int64_t)n * n;
    const cgnn_frame_mask<kMask> mask(keep, first, L);
    int lu = 0;                               // kMask: this wave's share of L_u
    if constexpr (kMask) {
      for (int t = threadIdx.x; t < L; t += kLwThreads) lu += mask.kept(t);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) lu += __shfl_xor(lu, o, 64);
    }

    // ---- stage ----
    int p = 0;
    for (int c = threadIdx.x; c < n; c += kLwThreads) {
      const float* __restrict__ st = stats + (u * n + c) * 2;
      const float r = st[1];
      mean[c] = st[0];
      rstd[c] = r;
      p += r != 0.0f;                         // (a NaN counts: its unit is a NaN anyway)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
    __syncthreads();

    // ---- frames ----
    double b = 0.0;                           // sum of s_t^2 over the frames of this wave that fall in this slot
    for (int t0 = wave; t0 < L; t0 += kLwWaves * kLwFrames) {
      double sq[kLwFrames];
#pragma unroll
      for (int i = 0; i < kLwFrames; ++i) sq[i] = 0.0;
      const unsigned kf = mask.block(t0, kLwWaves, kLwFrames, lane);       // kMask: bit i says that frame t0 + 4 i counts
      for (int c = lane; c < n; c += 64) {
        const float m = mean[c], r = rstd[c];
        float v[kLwFrames];
#pragma unroll
        for (int i = 0; i < kLwFrames; ++i) {
          const int t = t0 + kLwWaves * i;
          v[i] = t < L ? x[(int64_t)t * n + c] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < kLwFrames; ++i) {
          const float z = (v[i] - m) * r;
          sq[i] += !kMask || ((kf >> i) & 1) ? (double)z * (double)z : 0.0;
        }
      }
      const double st = wave_sum8(sq, lane);
      if (kMask ? (kf >> slot) & 1 : mask.kept(t0 + kLwWaves * slot)) b += st * st;        // (a frame past L, or censored,
                                                                                         // holds nothing that counts)
    }

    // ---- triangle ----
    double o = 0.0;
    for (int i0 = wave; i0 < n - 1; i0 += kLwWaves * kLwRows) {
      const int len = n - 1 - i0;             // of the longest of the four rows
      for (int jj = lane; jj < len; jj += 64) {
        float v[kLwRows];
#pragma unroll
        for (int r = 0; r < kLwRows; ++r) {
          const int i = i0 + kLwWaves * r, j = i + 1 + jj;
          v[r] = j < n ? R[(int64_t)i * n + j] : 0.0f;      // (i < j < n)
        }
#pragma unroll
        for (int r = 0; r < kLwRows; ++r) o += (double)v[r] * (double)v[r];
      }
    }
    o = cgnn_wave_sum(o);

    // ---- merge ----
    if ((lane & 7) == 0) part_b[wave][slot] = b;
    if (lane == 0) {
      part_o[wave] = o;
      kept[wave] = p;
      frames[wave] = lu;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double bs = 0.0, os = 0.0;
      int ps = 0;
      for (int k = 0; k < kLwWaves; ++k) {
        for (int i = 0; i < kLwFrames; ++i) bs += part_b[k][i];
        os += part_o[k];
        ps += kept[k];
      }
      int lc = L;                             // the unit's frame count: L, or L_u under a mask
      if constexpr (kMask) lc = frames[0] + frames[1] + frames[2] + frames[3];
      const double B = (double)lc * bs, O = 2.0 * os, F = (double)ps + O;
      double a = 0.0;
      if (O != 0.0) {                         // (a NaN is not 0)
        const double q = (B - F) / ((double)lc * O);
        a = q != q ? q : ((kMask ? lc <= 2 : lc == 2) || q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q));
      }
      alpha[u] = a;
    }
    __syncthreads();                          // the next unit's stage overwrites the statistics and the parts
  }
}

// a stream, as the statistics pass is: every wave the CU holds
#ifndef CGNN_LW_PER_CU
#define CGNN_LW_PER_CU 4
#endif

// what both entry points check and do; masked: keep [S, T] selects the frames, and stats and matrices come with their
// byte counts
int lw_call(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride, const uint8_t* keep,
            int64_t keep_bytes, bool masked, const float* stats, int64_t stats_bytes, const float* matrices,
            int64_t matrices_bytes, double* alpha, int64_t alpha_bytes, void* stream) {
  cgnn_units un;
  if (cgnn_check_cohort_upto(S, n, CGNN_PARTIAL_MAX_NODES) != CGNN_OK) return CGNN_EINVAL;
  if (cgnn_check_units(S, T, n, window, stride, &un) != CGNN_OK) return CGNN_EINVAL;
  if (keep_bytes < 0 || stats_bytes < 0 || matrices_bytes < 0 || alpha_bytes < 0) return CGNN_EINVAL;
  const int64_t U = un.U;
  if (S == 0) return CGNN_OK;
  if (!ts || !stats || !matrices || !alpha || (masked && !keep)) return CGNN_EINVAL;
  if (cgnn_misaligned({ts, stats, matrices}, 3) || cgnn_misaligned({alpha}, 7)) return CGNN_EINVAL;
  CGNN_NEED_BYTES(alpha, alpha_bytes, U * (int64_t)sizeof(double));
  const int grid = cgnn_grid_for(U, CGNN_LW_PER_CU);
  hipStream_t hs = cgnn_stream(stream);
  if (masked) {
    CGNN_NEED_BYTES(keep, keep_bytes, S * (int64_t)T);
    CGNN_NEED_BYTES(stats, stats_bytes, U * n * 2 * (int64_t)sizeof(float));
    CGNN_NEED_BYTES(matrices, matrices_bytes, U * n * (int64_t)n * (int64_t)sizeof(float));
    k_lw<true><<<grid, kLwThreads, 0, hs>>>(ts, U, T, n, (int)un.W, un.L, un.st, stats, matrices, alpha, keep);
  } else {
    k_lw<false><<<grid, kLwThreads, 0, hs>>>(ts, U, T, n, (int)un.W, un.L, un.st, stats, matrices, alpha, nullptr);
  }
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

}  // namespace

extern "C" int cgnn_ingest_shrinkage(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride,
                                     const float* stats, const float* matrices, double* alpha, int64_t alpha_bytes,
                                     void* stream) {
  return lw_call(ts, S, T, n, window, stride, nullptr, 0, false, stats, 0, matrices, 0, alpha, alpha_bytes, stream);
}

// frame censoring: the same launch over the frames keep [S, T] selects; stats and matrices are what
// cgnn_ingest_corr_masked left for the same mask
extern "C" int cgnn_ingest_shrinkage_masked(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window,
                                            int32_t stride, const uint8_t* keep, int64_t keep_bytes, const float* stats,
                                            int64_t stats_bytes, const float* matrices, int64_t matrices_bytes,
                                            double* alpha, int64_t alpha_bytes, void* stream) {
  return lw_call(ts, S, T, n, window, stride, keep, keep_bytes, true, stats, stats_bytes, matrices, matrices_bytes, alpha,
                 alpha_bytes, stream);
}
