// activity.hip -- regional activity node features of a device-resident cohort of ROI time series (float [S, T, n], one row
// per frame): cgnn_ingest_activity.  Features of the series itself, not of the connectivity matrix: the
// temporal std, the lag-1 autocorrelation, ALFF and fALFF (Zang 2007, Zou 2008) and their C-PAC forms.
//
// Per subject and column i, stated in fp64: m = the mean, xc[t] = x[t, i] - m, q = sum xc^2, K = T / 2,
// X_k = sum_t xc[t] e^(-2 pi i k t / T) for k = 1 .. K, w_k = 2 but w_K = 1 when T is even, the band = bins k_lo .. k_hi:
//   std = sqrt(q / (T - 1))        autocorr1 = sum_{t < T-1} xc[t] xc[t+1] / q        alff = mean_band 2 |X_k| / T
//   falff = sum_band |X_k| / sum_{1..K} |X_k|        band_std = sqrt(sum_band w_k |X_k|^2 / T / (T - 1))
//   band_fraction = band_std / std                   a zero denominator gives +0.0
//
//   k_activity_table     float [T, ld]: cos and sin of bin kt + j in columns 2 j and 2 j + 1, an fp64 cospi / sinpi of the
//                        exactly reduced argument ((2 k t) mod 2 T) / T, rounded to fp32 once; columns past the bins zero.
//                        The bins are 1 .. K when falff is asked, else k_first .. k_hi with k_first = k_lo, less one if k_lo
//                        is even: the band's first column is then 16-byte aligned in either table.
//   k_activity_moments   a workgroup per item (subject, 64 columns), grid stride, a lane per column.  Wave w owns the
//                        contiguous frames [w seg, (w + 1) seg), seg = ceil(T / 4): their sum in fp64 in ascending order,
//                        the four sums in wave order, one division (the sum of T copies of an fp32 value is exact in fp64:
//                        a constant column's mean is the value itself and its xc exactly 0).  Then, with the UNROUNDED
//                        xc = double(x) - m, q and the lag-1 sum over the same segment, which reads one frame past its
//                        end for the last product; merged in wave order.  A lane has the next block of 8 frames in
//                        flight while it reduces this one.  Writes m, q and the lag-1 sum as doubles, and the features
//                        themselves when no spectral one is asked.
//   k_activity_spectrum<kPad, vec>   a persistent grid over the items, 4 waves, built as k_filter's phase 1 is
//                        (filter.hip): C = B^T xc on v_mfma_f32_16x16x4_f32, the frames 32 at a time, x centred as
//                        fl32(double(x) - m) on its way into LDS, the table's rows beside it, both panels frame-major with
//                        strides = 16 (mod 32), two LDS buffers, the next step's loads issued before this step's MFMAs,
//                        the 2 x 2 waves own half of the chunk's kPad table columns x 32 series columns each.  The bins
//                        k_first .. go in chunks of kPad / 2 <= 128; every chunk is a pass over the item's frames.
//       epilogue         D of the instruction: lane l, register r holds row 4 (l >> 4) + r, column l & 15.  Rows are
//                        table columns, so registers (0, 1) and (2, 3) are (re, im) of two bins of one series column.
//                        |X_k|^2 = re^2 + im^2 and its root in fp64; a lane adds the bins inside [k_a, k_b] in ascending
//                        order into its amplitude and power sums (power with w_k).  No coefficient is stored.
//       reduction        through LDS (over the panels): per series column the four lane groups in order, then the two
//                        waves that share the column, then the chunks ascending, all in one thread.
//                        One launch sums the band.  falff needs a second launch over 1 .. K (its kPad fits K, the band's
//                        fits the band); the band's sums wait in the workspace.  The last launch takes the ratios and
//                        roots in fp64 with the moments, rounds once and stores the F columns of its 64 nodes.
//
// A bin's place in the sums depends on (k_first, kPad) of its launch, which depend on the band (and on T) alone: a
// subset or another order of the names gives the same bits.  No atomics, and no work assignment depends on the grid: the
// same bits on every run and for every grid.  Columns never mix: column j of xc meets column j of C only, so a NaN stays
// in its column.  Frames past T and columns past n are zeros in LDS, never read from memory and never stored.  Element
// offsets are 64-bit.
#include <math.h>

#include "gram_tile.h"
#include "measure_request.h"
#include "series_request.h"

namespace {

using gram::f32x4;
using gram::load4;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCols = 64;                     // columns of an item
constexpr int kFS = 32;                       // frames per step
constexpr int kLdX = kCols + 16;              // LDS row stride of xc: = 16 (mod 32)
constexpr int kXSlots = kFS * (kCols / 4) / kThreads;       // float4 slots of a [32, 64] panel per thread
constexpr int kMaxPad = 256;                  // table columns of the widest chunk: 128 bins, 64 accumulator registers
constexpr int kLdsBytes = 160 * 1024;
constexpr int kBlock = 8;                     // frames a lane of k_activity_moments has in flight
static_assert(kXSlots * kThreads == kFS * (kCols / 4), "a panel is a whole number of slots per thread");

using Cols = cgnn_columns<CGNN_ACTIVITY_FEATURES>;

constexpr int ld_b(int kPad) { return kPad + 16; }          // = 16 (mod 32): row reads
constexpr int step_floats(int kPad) { return kFS * ld_b(kPad) + kFS * kLdX; }
constexpr int kRedDoubles = 2 * 2 * 4 * kCols;              // [sum][wave half][lane group][column]
constexpr size_t lds_of(int kPad) {
  const size_t panels = 2 * step_floats(kPad) * sizeof(float), red = kRedDoubles * sizeof(double);
  return kCols * sizeof(double) + (panels > red ? panels : red);
}
static_assert(lds_of(kMaxPad) <= (size_t)kLdsBytes, "the widest chunk fits the LDS of a CU");

// table columns of `bins` bins: one chunk of a multiple of 64 columns, or chunks of kMaxPad
constexpr int table_ld(int bins) {
  return 2 * bins <= kMaxPad ? (2 * bins + 63) / 64 * 64 : (2 * bins + kMaxPad - 1) / kMaxPad * kMaxPad;
}
constexpr int pad_of(int bins) { return 2 * bins <= kMaxPad ? table_ld(bins) : kMaxPad; }
static_assert((int64_t)CGNN_ACTIVITY_MAX_FRAMES * table_ld(CGNN_ACTIVITY_MAX_FRAMES / 2) * 4 <= (int64_t)64 << 20,
              "the whole-spectrum table stays at or below 64 MB");

__global__ __launch_bounds__(kThreads) void k_activity_table(int T, int ld, int kt, int bins, float* __restrict__ table) {
  const int64_t total = (int64_t)T * ld;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t t = e / ld;
    const int c = (int)(e - t * ld), j = c >> 1;
    float v = 0.0f;
    if (j < bins) {
      const int64_t arg = (2 * t * (int64_t)(kt + j)) % (2 * (int64_t)T);       // both have period 2 T in it
      const double a = (double)arg / (double)T;
      v = (float)(c & 1 ? sinpi(a) : cospi(a));
    }
    table[e] = v;
  }
}

// what a launch that finishes knows of a column
struct Sums {
  double q, lag, band_amp, band_pow, all_amp;
};

// the ratios and roots in fp64, one rounding each.  A comparison with a NaN is false: it takes the division
__device__ __forceinline__ void finish(const Cols& cols, const Sums& s, int T, int band_bins, float* __restrict__ o) {
  const double sd = sqrt(s.q / (double)(T - 1));
  const double bsd = sqrt(s.band_pow / (double)T / (double)(T - 1));
  const double v[CGNN_ACTIVITY_FEATURES] = {
      sd,
      s.q == 0.0 ? 0.0 : s.lag / s.q,
      2.0 * s.band_amp / (double)T / (double)band_bins,
      s.all_amp == 0.0 ? 0.0 : s.band_amp / s.all_amp,
      bsd,
      sd == 0.0 ? 0.0 : bsd / sd,
  };
#pragma unroll
  for (int f = 0; f < CGNN_ACTIVITY_FEATURES; ++f)
    if (cols.col[f] >= 0) o[cols.col[f]] = (float)v[f];
}

// mom: double [3][S n] = mean | q | lag-1 sum.  last: no spectral feature follows, the features are written here
__global__ __launch_bounds__(kThreads) void k_activity_moments(const float* __restrict__ ts, int64_t S, int T, int n,
                                                               double* __restrict__ mom, int last, Cols cols,
                                                               float* __restrict__ out) {
  __shared__ double part[3][kWaves][kCols];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = (n + kCols - 1) / kCols;
  const int64_t items = S * chunks, rows = S * n;
  const int seg = (T + kWaves - 1) / kWaves;
  const int t0 = wave * seg, t1 = t0 + seg < T ? t0 + seg : T;          // (t1 <= t0: a wave without frames)
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t s = item / chunks;
    const int col = (int)(item - s * chunks) * kCols + lane;
    const bool act = col < n;
    const float* __restrict__ x = ts + s * T * n + (act ? col : 0);
    double sum = 0.0;
    float v[kBlock], nx[kBlock];              // the next block's loads fly while this one is reduced
    if (act) {
      // the frames t .. t + 7 of the segment; past its end zeros, which are never read from memory
      auto load = [&](int t) {
#pragma unroll
        for (int i = 0; i < kBlock; ++i) nx[i] = t + i < t1 ? x[(int64_t)(t + i) * n] : 0.0f;
      };
      load(t0);
      for (int t = t0; t < t1; t += kBlock) {
#pragma unroll
        for (int i = 0; i < kBlock; ++i) v[i] = nx[i];
        load(t + kBlock);
#pragma unroll
        for (int i = 0; i < kBlock; ++i) sum += (double)v[i];           // (the padding adds zeros)
      }
    }
    part[0][wave][lane] = sum;
    __syncthreads();
    const double m = (((part[0][0][lane] + part[0][1][lane]) + part[0][2][lane]) + part[0][3][lane]) / (double)T;
    double q = 0.0, lag = 0.0;
    if (act && t0 < t1) {
      // the frames t + 1 .. t + 8: one past the segment for its last product, none past the run
      auto load = [&](int t) {
#pragma unroll
        for (int i = 0; i < kBlock; ++i) nx[i] = t + i < t1 && t + i + 1 < T ? x[(int64_t)(t + i + 1) * n] : 0.0f;
      };
      load(t0);
      double prev = (double)x[(int64_t)t0 * n] - m;
      for (int t = t0; t < t1; t += kBlock) {
#pragma unroll
        for (int i = 0; i < kBlock; ++i) v[i] = nx[i];
        load(t + kBlock);
#pragma unroll
        for (int i = 0; i < kBlock; ++i) {
          if (t + i < t1) {
            q += prev * prev;
            if (t + i + 1 < T) {
              const double next = (double)v[i] - m;
              lag += prev * next;
              prev = next;
            }
          }
        }
      }
    }
    part[1][wave][lane] = q;
    part[2][wave][lane] = lag;
    __syncthreads();                          // (every wave is past its reads of part[0] too)
    if (wave == 0 && act) {
      Sums r{};
      r.q = ((part[1][0][lane] + part[1][1][lane]) + part[1][2][lane]) + part[1][3][lane];
      r.lag = ((part[2][0][lane] + part[2][1][lane]) + part[2][2][lane]) + part[2][3][lane];
      const int64_t row = s * n + col;
      mom[row] = m;
      mom[rows + row] = r.q;
      mom[2 * rows + row] = r.lag;
      if (last) finish(cols, r, T, 1, out + row * cols.ldx);
    }
  }
}

// 4 loaded entries of frame t, columns c .. c + 3 of the item -> xc; frames past T and columns past n give zeros
__device__ __forceinline__ f32x4 centre(f32x4 v, int t, int T, int c, int col0, int n, const double* mu) {
  f32x4 z = {0.f, 0.f, 0.f, 0.f};
  if (t < T) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (col0 + c + e < n) z[e] = (float)((double)v[e] - mu[c + e]);
  }
  return z;
}

// One launch sums the bins [k_a, k_b] of the table columns from `off` on: column off + 2 j is the cosine of bin
// k_first + j.  sums: double [2][S n][2] = (amplitude sum, power sum) of the band launch | of the launch over 1 .. K.
// slot: which of the two this launch is.  last: it finishes the features.
template <int kPad, bool kVec>
__global__ __launch_bounds__(kThreads) void k_activity_spectrum(const float* __restrict__ ts, int64_t S, int T, int n,
                                                                const float* __restrict__ table, int ld, int off,
                                                                int nchunks, int k_first, int k_a, int k_b,
                                                                const double* __restrict__ mom, double* sums, int slot,
                                                                int last, int band_bins, Cols cols,
                                                                float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  double* mu = reinterpret_cast<double*>(lds);                // [64] the item's means, 0 past n
  float* area = reinterpret_cast<float*>(mu + kCols);
  double* red = reinterpret_cast<double*>(area);              // over the panels, once nobody reads them
  constexpr int kRB = kPad / 32;              // blocks of 16 table columns a wave owns, by 2 blocks of 16 series columns
  constexpr int kBSlots = kPad / 32;          // float4 slots of a [32, kPad] step of the table per thread
  constexpr int kLd1 = ld_b(kPad);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frow = lane >> 4, fcol = lane & 15;
  int xrow[kXSlots], xcol[kXSlots];
#pragma unroll
  for (int q = 0; q < kXSlots; ++q) {
    const int e = tid + kThreads * q;
    xrow[q] = e / (kCols / 4);
    xcol[q] = 4 * (e % (kCols / 4));
  }
  const int chunks = (n + kCols - 1) / kCols;
  const int64_t items = S * chunks, rows = S * n;
  const int nks = (T + kFS - 1) / kFS;
  const int nyquist = T % 2 == 0 ? T / 2 : 0;                 // the bin whose weight is 1

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t s = item / chunks;
    const int col0 = (int)(item - s * chunks) * kCols;
    const float* __restrict__ x = ts + s * T * n;

    __syncthreads();                          // the previous item's last reads of mu and red
    if (tid < kCols) mu[tid] = col0 + tid < n ? mom[s * n + col0 + tid] : 0.0;

    f32x4 px[kXSlots], pb[kBSlots];
    double tot_amp = 0.0, tot_pow = 0.0;      // tid < 64: this column's sums over the chunks so far

    for (int ch = 0; ch < nchunks; ++ch) {
      const int c0 = off + ch * kPad;         // the chunk's first table column
      auto load_x = [&](int t0) {
#pragma unroll
        for (int q = 0; q < kXSlots; ++q) px[q] = load4<kVec>(x, t0 + xrow[q], T, col0 + xcol[q], n);
      };
      // rows t0 .. t0 + 31, columns c0 .. c0 + kPad - 1 of the table; rows past T and columns past ld read as zeros
      auto load_b = [&](int t0) {
#pragma unroll
        for (int q = 0; q < kBSlots; ++q) {
          const int e = 4 * (tid + kThreads * q);
          const int r = t0 + e / kPad, c = c0 + e % kPad;
          pb[q] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (r < T && c < ld) pb[q] = *reinterpret_cast<const f32x4*>(table + (int64_t)r * ld + c);
        }
      };
      auto store_step = [&](int buf, int t0) {
        float* bb = area + buf * step_floats(kPad);
        float* bx = bb + kFS * kLd1;
#pragma unroll
        for (int q = 0; q < kBSlots; ++q) {
          const int e = 4 * (tid + kThreads * q);
          *reinterpret_cast<f32x4*>(&bb[(e / kPad) * kLd1 + e % kPad]) = pb[q];
        }
#pragma unroll
        for (int q = 0; q < kXSlots; ++q)
          *reinterpret_cast<f32x4*>(&bx[xrow[q] * kLdX + xcol[q]]) =
              centre(px[q], t0 + xrow[q], T, xcol[q], col0, n, mu);
      };
      load_x(0);
      load_b(0);
      __syncthreads();                        // mu; and the previous chunk's reads of red
      store_step(0, 0);
      __syncthreads();

      f32x4 acc[kRB][2];
#pragma unroll
      for (int a = 0; a < kRB; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

      int cur = 0;
      for (int ks = 0; ks < nks; ++ks) {
        const bool more = ks + 1 < nks;
        if (more) {
          load_x((ks + 1) * kFS);
          load_b((ks + 1) * kFS);
        }
        const float* __restrict__ pa = area + cur * step_floats(kPad) + frow * kLd1 + (wave >> 1) * (kPad / 2) + fcol;
        const float* __restrict__ pc =
            area + cur * step_floats(kPad) + kFS * kLd1 + frow * kLdX + (wave & 1) * 32 + fcol;
#pragma unroll
        for (int kk = 0; kk < kFS / 4; ++kk) {
          float fa[kRB], fb[2];
#pragma unroll
          for (int a = 0; a < kRB; ++a) fa[a] = pa[kk * 4 * kLd1 + a * 16];
#pragma unroll
          for (int b = 0; b < 2; ++b) fb[b] = pc[kk * 4 * kLdX + b * 16];
#pragma unroll
          for (int a = 0; a < kRB; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
              acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a], fb[b], acc[a][b], 0, 0, 0);
        }
        if (more) store_step(cur ^ 1, (ks + 1) * kFS);
        __syncthreads();
        cur ^= 1;
      }

      // ---- epilogue: registers (0, 1) and (2, 3) of a block are (re, im) of the bins kb + 8 a and kb + 8 a + 1 ----
      const int kb = k_first + ch * (kPad / 2) + (wave >> 1) * (kPad / 4) + 2 * frow;
      double amp[2] = {0.0, 0.0}, pw[2] = {0.0, 0.0};
#pragma unroll
      for (int a = 0; a < kRB; ++a)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const int k = kb + 8 * a + p;
          const bool in = k >= k_a && k <= k_b;
          const double w = k == nyquist ? 1.0 : 2.0;
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const double re = (double)acc[a][b][2 * p], im = (double)acc[a][b][2 * p + 1];
            const double p2 = re * re + im * im;
            amp[b] += in ? sqrt(p2) : 0.0;
            if (slot == 0) pw[b] += in ? w * p2 : 0.0;        // (only the band's power is ever read)
          }
        }
      // (every wave is past its last read of the panels: the loop ended on a barrier)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int c = (wave & 1) * 32 + b * 16 + fcol;
        red[((0 * 2 + (wave >> 1)) * 4 + frow) * kCols + c] = amp[b];
        red[((1 * 2 + (wave >> 1)) * 4 + frow) * kCols + c] = pw[b];
      }
      __syncthreads();
      if (tid < kCols) {
        double h[2][2];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const double* r = red + ((q * 2 + half) * 4) * kCols + tid;
            h[q][half] = ((r[0] + r[kCols]) + r[2 * kCols]) + r[3 * kCols];
          }
        tot_amp += h[0][0] + h[0][1];
        tot_pow += h[1][0] + h[1][1];
      }
      // (the next chunk's barrier in front of store_step separates these reads from its writes)
    }

    if (tid < kCols && col0 + tid < n) {
      const int64_t row = s * n + col0 + tid;
      double* mine = sums + ((int64_t)slot * rows + row) * 2;
      mine[0] = tot_amp;
      mine[1] = tot_pow;
      if (last) {
        Sums r{};
        r.q = mom[rows + row];
        r.lag = mom[2 * rows + row];
        if (slot == 0) {
          r.band_amp = tot_amp, r.band_pow = tot_pow;
        } else {                              // the band's sums were written by the launch before this one
          r.band_amp = sums[row * 2], r.band_pow = sums[row * 2 + 1];
          r.all_amp = tot_amp;
        }
        finish(cols, r, T, band_bins, out + row * cols.ldx);
      }
    }
  }
}

struct Launch {
  const float* table;
  int ld, off, bins, k_first, k_a, k_b, slot, last, band_bins;
};

template <int kPad, bool kVec>
int launch_as(const float* ts, int64_t S, int32_t T, int32_t n, const Launch& l, const double* mom, double* sums,
              const Cols& cols, float* out, hipStream_t hs) {
  constexpr size_t lds = lds_of(kPad);
  if (!cgnn_raise_lds_limit<k_activity_spectrum<kPad, kVec>>(kLdsBytes)) return CGNN_ELAUNCH;
  const int64_t items = S * ((n + kCols - 1) / kCols);
  const int grid = cgnn_grid_for(items, cgnn_wg_per_cu_by_lds(lds, kLdsBytes));
  const int nchunks = (2 * l.bins + kPad - 1) / kPad;
  k_activity_spectrum<kPad, kVec><<<grid, kThreads, lds, hs>>>(ts, S, T, n, l.table, l.ld, l.off, nchunks, l.k_first,
                                                               l.k_a, l.k_b, mom, sums, l.slot, l.last, l.band_bins,
                                                               cols, out);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

template <bool kVec>
int launch(const float* ts, int64_t S, int32_t T, int32_t n, const Launch& l, const double* mom, double* sums,
           const Cols& cols, float* out, hipStream_t hs) {
  switch (pad_of(l.bins)) {
    case 64: return launch_as<64, kVec>(ts, S, T, n, l, mom, sums, cols, out, hs);
    case 128: return launch_as<128, kVec>(ts, S, T, n, l, mom, sums, cols, out, hs);
    case 192: return launch_as<192, kVec>(ts, S, T, n, l, mom, sums, cols, out, hs);
    default: return launch_as<256, kVec>(ts, S, T, n, l, mom, sums, cols, out, hs);
  }
}

// the moments are a stream and want every wave the CU holds
#ifndef CGNN_ACTIVITY_MOMENTS_PER_CU
#define CGNN_ACTIVITY_MOMENTS_PER_CU 4
#endif

int check(int64_t S, int32_t T, int32_t n) {
  return cgnn_check_cohort(S, n) != CGNN_OK || T < 2 || T > CGNN_MAX_FRAMES ? CGNN_EINVAL : CGNN_OK;
}

int64_t table_bytes(int32_t T, int32_t bins) {
  return cgnn_align_up((int64_t)T * table_ld(bins) * (int64_t)sizeof(float), 16);
}

// the table | mean, q, lag-1 sum [3][S n] | the two launches' sums [2][S n][2], all doubles
int64_t need_bytes(int64_t S, int32_t T, int32_t n, int32_t bins) {
  return table_bytes(T, bins) + 7 * S * n * (int64_t)sizeof(double);
}

}  // namespace

extern "C" int64_t cgnn_ingest_activity_workspace_bytes(int64_t S, int32_t T, int32_t n, int32_t bins) {
  if (check(S, T, n) != CGNN_OK || bins < 0 || bins > T / 2) return CGNN_EINVAL;
  if (bins > 0 && T > CGNN_ACTIVITY_MAX_FRAMES) return CGNN_EINVAL;
  return need_bytes(S, T, n, bins);
}

extern "C" int cgnn_ingest_activity(const float* ts, int64_t S, int32_t T, int32_t n, const int32_t* feature_ids,
                                    int32_t F, int32_t k_lo, int32_t k_hi, void* workspace, int64_t workspace_bytes,
                                    float* out, int64_t out_bytes, void* stream) {
  Cols cols;
  if (check(S, T, n) != CGNN_OK) return CGNN_EINVAL;
  if (cgnn_check_request<CGNN_ACTIVITY_FEATURES>(feature_ids, F, 1, nullptr, 0, false, &cols) != CGNN_OK) return CGNN_EINVAL;
  bool spectral = false;
  for (int f = CGNN_ACTIVITY_ALFF; f < CGNN_ACTIVITY_FEATURES; ++f) spectral |= cols.col[f] >= 0;
  const bool whole = cols.col[CGNN_ACTIVITY_FALFF] >= 0;
  if (k_lo > k_hi) return CGNN_EINVAL;
  if (spectral && (k_lo < 1 || k_hi > T / 2 || T > CGNN_ACTIVITY_MAX_FRAMES)) return CGNN_EINVAL;
  if (workspace_bytes < 0 || out_bytes < 0) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (!ts || !out || !workspace || cgnn_misaligned({ts, out}, 3) || cgnn_misaligned({workspace}, 15)) return CGNN_EINVAL;
  const int k_first = spectral ? ((k_lo - 1) | 1) : 0;        // k_lo, less one if it is even
  const int band_table = spectral ? k_hi - k_first + 1 : 0;   // bins of the band's launch
  const int bins = whole ? T / 2 : band_table;                // bins of the table
  CGNN_NEED_BYTES(workspace, workspace_bytes, need_bytes(S, T, n, bins));
  if (!cgnn_holds_floats(out_bytes, S * n, F)) return CGNN_EINVAL;      // out [S n][F]

  hipStream_t hs = cgnn_stream(stream);
  float* table = static_cast<float*>(workspace);
  double* mom = reinterpret_cast<double*>(static_cast<unsigned char*>(workspace) + table_bytes(T, bins));
  double* sums = mom + 3 * S * n;
  const int64_t items = S * ((n + kCols - 1) / kCols);
  const int kt = whole ? 1 : k_first;                         // the bin of the table's first column
  if (spectral) {
    const int64_t blocks = ((int64_t)T * table_ld(bins) + kThreads - 1) / kThreads;
    k_activity_table<<<cgnn_grid_for(blocks, 8), kThreads, 0, hs>>>(T, table_ld(bins), kt, bins, table);
    CGNN_CHECK_LAUNCH();
  }
  k_activity_moments<<<cgnn_grid_for(items, CGNN_ACTIVITY_MOMENTS_PER_CU), kThreads, 0, hs>>>(ts, S, T, n, mom, !spectral,
                                                                                             cols, out);
  CGNN_CHECK_LAUNCH();
  if (!spectral) return CGNN_OK;
  const bool vec = n % 4 == 0 && !cgnn_misaligned({ts}, 15);
  const Launch band{table, table_ld(bins), 2 * (k_first - kt), band_table, k_first, k_lo, k_hi, 0, !whole, k_hi - k_lo + 1};
  int rc = vec ? launch<true>(ts, S, T, n, band, mom, sums, cols, out, hs)
               : launch<false>(ts, S, T, n, band, mom, sums, cols, out, hs);
  if (rc != CGNN_OK || !whole) return rc;
  const Launch all{table, table_ld(bins), 0, T / 2, 1, 1, T / 2, 1, 1, k_hi - k_lo + 1};
  return vec ? launch<true>(ts, S, T, n, all, mom, sums, cols, out, hs)
             : launch<false>(ts, S, T, n, all, mom, sums, cols, out, hs);
}
