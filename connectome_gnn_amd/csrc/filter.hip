// filter.hip -- a device-resident cohort of ROI time series (float [S, T, n], one row per frame) band-passed and
// detrended by projection on the orthonormal DCT-II basis: cgnn_ingest_filter, the step in front of
// cgnn_ingest_corr (timeseries.hip).  cgnn_ingest_regress is the same kernel in complement form against
// a table per subject, the orthonormal basis of its confounds (confounds.hip), in place of the one table of the cohort.
//
// Per subject and column i, over the T frames of the run: b_k[t] = sqrt(2 / T) cos(pi (2 t + 1) k / (2 T)), m_i = the
// column mean (fp64), xc[t,i] = fl32(double(x[t,i]) - m_i), and with the K components the caller names
//   keep        y = sum_k b_k (b_k . xc)            complement   y = xc - sum_k b_k (b_k . xc)
// (K == 0: y = xc, no product at all).  With B = [b_k] as float [T, Kpad], Kpad = K rounded up to 32, columns past K
// zero, that is C = B^T xc, [Kpad, 64] per 64 columns, and y = B C or xc - B C.
//
//   k_filter_basis  the table B [T, Kpad]: an fp64 cospi of the exactly reduced argument ((2 t + 1) k mod 4 T) / (2 T),
//                   scaled in fp64, rounded to fp32 once.
//   k_filter_mean   the stream of frame_mask.h, as k_corr_stats is: a thread's frames summed in fp64 in ascending order,
//                   the four waves' sums in wave order, one division.  (The sum of T copies of an fp32 value is exact
//                   in fp64, so a constant column's mean is the value itself and its xc is exactly 0.)
//   k_filter<Kpad, vec>  a persistent grid over the items (subject, 64 columns), grid stride; a workgroup of 4 waves owns
//                   all T frames of its item, which is what makes out == ts correct: phase 1 has read every frame
//                   before phase 2 writes the first, and phase 2 reads a chunk again (complement) in the thread that
//                   then writes it.
//     phase 1       C = B^T xc on v_mfma_f32_16x16x4_f32, the frames 32 at a time: the step's rows of B and of x are
//                   loaded into registers (the NEXT step's loads are issued before this step's MFMAs), x is centred in
//                   fp64 on its way into LDS, both panels are frame-major there -- lane l reads A[i][k] = B[t0 + (l >> 4)]
//                   [i0 + (l & 15)] and B[k][j] = xc[t0 + (l >> 4)][j0 + (l & 15)], rows of 16 whose strides = 16 (mod 32)
//                   keep the two rows of a 32-lane half on disjoint banks.  The 2 x 2 waves own half of the
//                   components x 32 columns each: Kpad / 4 accumulator registers, 64 at Kpad = 256.  Two LDS buffers,
//                   one barrier per step.  Then C goes to LDS (over the panels, which nobody reads any more).
//     phase 2       per chunk of 32 frames Y = B_chunk C: wave w owns columns [16 w, 16 w + 16) and both blocks of 16
//                   frames; A[i][k] = B[t0 + (l & 15)][k0 + (l >> 4)] is a column read of the chunk, so its LDS rows
//                   have a stride = 2 (mod 32) (conflict-free for that read) and are stored 8 bytes at a time.  Y goes
//                   through LDS so that a thread stores 4 consecutive columns of a frame (16-byte stores if n % 4 == 0
//                   and the pointers are aligned, scalar stores otherwise); the complement form loads x for the same 4
//                   columns, centres it as phase 1 did and subtracts.
//     LDS           Kpad = 64 / 128 / 192 / 256 take 41 / 65 / 77 / 154 KB: 3 / 2 / 2 / 1 workgroups a CU.  At 192 the
//                   chunk is 16 frames (one block a wave), which is what fits the second workgroup in; at 256 one
//                   workgroup has the CU to itself and the chunk of B is double-buffered instead.
//
// Frame censoring: cgnn_ingest_regress_masked is cgnn_ingest_regress with a frame mask keep [S, T], one
// host body for both (regress_call).  The mask is one more template argument of k_filter_mean and k_filter and the
// predicate of frame_mask.h: the mean is the kept frames' sum over their count, centre() gives a censored frame a zero
// row (phase 1, phase 2 and the kPad == 0 stream), and phase 2 selects an exact zero for it.  The unmasked instantiations
// keep their code.  k_design writes the design of a band that is removed by regression, [table values | confounds] per
// subject, with k_filter_basis's values.  What the entry points check alike is in series_request.h.
//
// Accumulation is fp32 in ascending order of the frame (phase 1) and of the component (phase 2), no atomics, and no work
// assignment depends on the grid: the same bits on every run and for every grid.  Columns never mix: column j of xc
// meets column j of C and of Y only.  Frames past T and columns past n are zeros in LDS, never read from memory and
// never stored.  Element offsets into `ts` and `out` are 64-bit.
#include <math.h>

#include "frame_mask.h"
#include "gram_tile.h"
#include "measure_request.h"
#include "series_request.h"

namespace {

using gram::f32x4;
using gram::load4;

constexpr int kThreads = 256;
constexpr int kCols = kStreamCols;            // columns of an item
constexpr int kFS = 32;                       // frames per step (phase 1) and per chunk (phase 2)
constexpr int kLdX = kCols + 16;              // LDS row stride of xc and of C: = 16 (mod 32)
constexpr int kLdY = kCols + 4;               // of Y: rows of float4
constexpr int kXSlots = kFS * (kCols / 4) / kThreads;      // float4 slots of a [32, 64] panel per thread
constexpr int kLdsBytes = 160 * 1024;
static_assert(kXSlots * kThreads == kFS * (kCols / 4), "a panel is a whole number of slots per thread");
static_assert(kThreads == kStreamThreads, "k_filter_mean runs on the stream of frame_mask.h");

constexpr int pad_of(int K) { return (K + 31) / 32 * 32; }

// LDS of k_filter<kPad>, in floats past the means: phase 1's two buffers (rows of B | rows of xc) and phase 2's
// C | chunk(s) of B | Y share the space
constexpr int ld_b1(int kPad) { return kPad + 16; }        // = 16 (mod 32): row reads
constexpr int ld_b2(int kPad) { return kPad + 2; }         // = 2 (mod 32): column reads
constexpr int step_floats(int kPad) { return kFS * ld_b1(kPad) + kFS * kLdX; }
constexpr size_t lds_with(int kPad, int frames, int buffers) {
  const int a = 2 * step_floats(kPad), b = kPad * kLdX + buffers * frames * ld_b2(kPad) + frames * kLdY;
  return kCols * sizeof(double) + (kPad ? sizeof(float) * (a > b ? a : b) : 0);
}
// Phase 2's chunk: 32 frames; 16 where that is what lets two workgroups share a CU (Kpad = 192: the second workgroup's
// MFMAs fill the barriers and the epilogue of the first, which a lone wave per SIMD leaves empty).  Two buffers for the
// chunk of B where one workgroup has the CU to itself anyway (Kpad = 256).
constexpr int chunk_frames(int kPad) {
  return kPad % 64 == 0 && lds_with(kPad, kFS, 1) > (size_t)kLdsBytes / 2 && lds_with(kPad, 16, 1) <= (size_t)kLdsBytes / 2
             ? 16
             : kFS;
}
constexpr bool double_chunk(int kPad) { return lds_with(kPad, chunk_frames(kPad), 1) > (size_t)kLdsBytes / 2; }
constexpr int chunk_floats(int kPad) { return chunk_frames(kPad) * ld_b2(kPad); }
constexpr size_t lds_of(int kPad) { return lds_with(kPad, chunk_frames(kPad), double_chunk(kPad) ? 2 : 1); }
static_assert(chunk_frames(160) == 32 && !double_chunk(160) && chunk_frames(192) == 16 && !double_chunk(192) &&
                  chunk_frames(224) == 32 && double_chunk(224) && chunk_frames(256) == 32 && double_chunk(256),
              "as the comment says");
static_assert(lds_of(CGNN_FILTER_MAX_COMPONENTS) <= (size_t)kLdsBytes, "the largest Kpad fits the LDS of a CU");

using Comps = cgnn_components;

// b_k[t] of a T-frame run, scale = sqrt(2 / T): the one value function of k_filter_basis and k_design
__device__ __forceinline__ float basis_value(int64_t t, int k, int T, double scale) {
  const int64_t arg = ((2 * t + 1) * (int64_t)k) % (4 * (int64_t)T);                // cos has period 4 T in it
  return (float)(scale * cospi((double)arg / (double)(2 * (int64_t)T)));
}

__global__ __launch_bounds__(kThreads) void k_filter_basis(Comps comps, int K, int kpad, int T,
                                                           float* __restrict__ table) {
  const int64_t total = (int64_t)T * kpad;
  const double scale = sqrt(2.0 / (double)T);
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t t = e / kpad;
    const int c = (int)(e - t * kpad);
    table[e] = c < K ? basis_value(t, comps.k[c], T, scale) : 0.0f;
  }
}

// The design of a regression under censoring: float [S, T, K + q] = [table values | confounds], the
// cosines at the frame's own t on the grid of the whole run.  A thread per entry, grid stride.
__global__ __launch_bounds__(kThreads) void k_design(Comps comps, int K, const float* __restrict__ conf, int64_t S,
                                                     int T, int q, float* __restrict__ design) {
  const int w = K + q;
  const int64_t total = S * T * w;
  const double scale = sqrt(2.0 / (double)T);
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t row = e / w;                // s * T + t
    const int c = (int)(e - row * w);
    design[e] = c < K ? basis_value(row % T, comps.k[c], T, scale) : conf[row * q + (c - K)];
  }
}

// The column means, on the stream of frame_mask.h: a thread's frames summed in fp64 in ascending order, the four waves'
// sums in wave order, one division.  kMask: `keep` [S, T] selects the frames: the sum and the count run
// over the kept ones, and a subject without a kept frame has mean 0
struct MeanAcc {
  double sum = 0.0;                           // of frames wave, wave + 4, ..., in that order
  int cnt = 0;                                // kMask: this wave's kept frames
};

template <bool kMask>
__global__ __launch_bounds__(kThreads) void k_filter_mean(const float* __restrict__ ts, int64_t S, int T, int n,
                                                          double* __restrict__ mean, const uint8_t* __restrict__ keep) {
  __shared__ double part[kStreamWaves][kCols];
  cgnn_stream_columns<kMask, MeanAcc>(
      ts, keep, S, T, n, 1, T, 0,
      [](MeanAcc& a, const float (&v)[kStreamBlock], unsigned bits, int) {
        if constexpr (kMask) a.cnt += __builtin_popcount(bits);
#pragma unroll
        for (int i = 0; i < kStreamBlock; ++i)          // (the padding adds zeros; a censored frame is left out)
          a.sum += !kMask || ((bits >> i) & 1) ? (double)v[i] : 0.0;
      },
      [&](const MeanAcc& a, int64_t s, int col, bool act, int lane, int wave) {
        part[wave][lane] = a.sum;
        if constexpr (kMask) {
          __shared__ int kept[kStreamWaves][kCols];
          kept[wave][lane] = a.cnt;
          __syncthreads();
          if (wave == 0 && act) {
            const int tk = kept[0][lane] + kept[1][lane] + kept[2][lane] + kept[3][lane];
            const double total = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
            mean[s * n + col] = tk ? total / (double)tk : 0.0;
          }
        } else {
          __syncthreads();
          if (wave == 0 && act)
            mean[s * n + col] = (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]) / (double)T;
        }
        __syncthreads();
      });
}

// 4 loaded entries of frame t, columns c .. c + 3 of the item -> xc; frames past T and columns past n give zeros
// (and so does a censored frame: kept == false)
__device__ __forceinline__ f32x4 centre(f32x4 v, int t, int T, int c, int col0, int n, const double* mu,
                                        bool kept = true) {
  f32x4 z = {0.f, 0.f, 0.f, 0.f};
  if (t < T && kept) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (col0 + c + e < n) z[e] = (float)((double)v[e] - mu[c + e]);
  }
  return z;
}

template <bool kVec>
__device__ __forceinline__ void store4(float* o, int t, int T, int col, int n, f32x4 v) {
  if (t >= T) return;
  float* p = o + (int64_t)t * n + col;
  if (kVec) {
    if (col < n) *reinterpret_cast<f32x4*>(p) = v;        // (n % 4 == 0: the four columns are there together)
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (col + e < n) p[e] = v[e];
  }
}

// `ts` and `out` may be the same array: neither is __restrict__.  table_stride: floats between the tables of two
// subjects (cgnn_ingest_regress: a basis per subject), 0 for the one table of the cohort.  kMask:
// `keep` [S, T] selects the frames; a censored frame is a zero row of xc in phase 1 and an exact zero row of the output
// (the table's rows there are zeros too: cgnn_ingest_confound_basis_masked writes them so)
template <int kPad, bool kVec, bool kMask = false>
__global__ __launch_bounds__(kThreads) void k_filter(const float* ts, int64_t S, int T, int n, int complement,
                                                     const float* __restrict__ tables, int64_t table_stride,
                                                     const double* __restrict__ mean, float* out,
                                                     const uint8_t* __restrict__ keep) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  double* mu = reinterpret_cast<double*>(lds);                // [64] the item's means, 0 past n
  float* area = reinterpret_cast<float*>(mu + kCols);
  constexpr int kRB = kPad / 32;              // blocks of 16 components a wave owns in phase 1, by 2 blocks of 16 columns
  constexpr int kBSlots = kPad / 32;          // float4 slots of a [32, kPad] chunk of B per thread
  constexpr int kLd1 = ld_b1(kPad), kLd2 = ld_b2(kPad);
  constexpr bool kDouble = double_chunk(kPad);

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
  const int64_t items = S * chunks;
  const int nks = (T + kFS - 1) / kFS;

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t s = item / chunks;
    const int col0 = (int)(item - s * chunks) * kCols;
    const float* x = ts + s * T * n;
    float* o = out + s * T * n;
    const float* __restrict__ table = tables + s * table_stride;
    const cgnn_frame_mask<kMask> mask(keep, s * T, T);

    __syncthreads();                          // the previous item's last chunk still reads mu and Y
    if (tid < kCols) mu[tid] = col0 + tid < n ? mean[s * n + col0 + tid] : 0.0;

    f32x4 px[kXSlots];
    bool fl = true;                           // kMask: frame t0 + (tid & 31) of px's step is kept: one load for the step,
    auto load_x = [&](int t0) {               // which a ballot turns into the step's 32 flags where they are used
#pragma unroll
      for (int q = 0; q < kXSlots; ++q) px[q] = load4<kVec>(x, t0 + xrow[q], T, col0 + xcol[q], n);
      if constexpr (kMask) fl = mask.kept(t0 + (tid & 31));
    };
    auto kept_rows = [&](bool f) {            // (every thread of the workgroup is here)
      if constexpr (kMask) return (uint32_t)__ballot(f);
      else return ~0u;
    };

    if constexpr (kPad == 0) {                // pure centring: a stream
      __syncthreads();
      for (int ks = 0; ks < nks; ++ks) {
        load_x(ks * kFS);
        const uint32_t rows = kept_rows(fl);
#pragma unroll
        for (int q = 0; q < kXSlots; ++q)
          store4<kVec>(o, ks * kFS + xrow[q], T, col0 + xcol[q], n,
                       centre(px[q], ks * kFS + xrow[q], T, xcol[q], col0, n, mu, (rows >> xrow[q]) & 1));
      }
    } else {
      f32x4 pb[kBSlots];
      // the rows t0 .. t0 + 31 of the table are 32 * kPad consecutive floats; rows past T read as zeros
      auto load_b = [&](int t0) {
        const float* __restrict__ src = table + (int64_t)t0 * kPad;
#pragma unroll
        for (int q = 0; q < kBSlots; ++q) {
          const int e = 4 * (tid + kThreads * q);
          pb[q] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (t0 + e / kPad < T) pb[q] = *reinterpret_cast<const f32x4*>(src + e);
        }
      };

      // ---- phase 1: C = B^T xc ----
      auto store_step = [&](int buf, int t0) {
        float* bb = area + buf * step_floats(kPad);
        float* bx = bb + kFS * kLd1;
#pragma unroll
        for (int q = 0; q < kBSlots; ++q) {
          const int e = 4 * (tid + kThreads * q);
          *reinterpret_cast<f32x4*>(&bb[(e / kPad) * kLd1 + e % kPad]) = pb[q];
        }
        const uint32_t rows = kept_rows(fl);
#pragma unroll
        for (int q = 0; q < kXSlots; ++q)
          *reinterpret_cast<f32x4*>(&bx[xrow[q] * kLdX + xcol[q]]) =
              centre(px[q], t0 + xrow[q], T, xcol[q], col0, n, mu, (rows >> xrow[q]) & 1);
      };
      load_x(0);
      load_b(0);
      __syncthreads();                        // mu
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

      // ---- C -> LDS (every wave is past its last read of the panels); the first chunk of B ----
      float* cl = area;                       // [kPad][kLdX]
      float* bc = cl + kPad * kLdX;           // [1 or 2][kF2][kLd2]
      float* yl = bc + (kDouble ? 2 : 1) * chunk_floats(kPad);          // [kF2][kLdY]
#pragma unroll
      for (int a = 0; a < kRB; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            cl[((wave >> 1) * (kPad / 2) + a * 16 + 4 * frow + r) * kLdX + (wave & 1) * 32 + b * 16 + fcol] = acc[a][b][r];
      // a chunk is kF2 frames: kF2 * kPad consecutive floats of the table, kF2 / 16 blocks of 16 frames a wave
      constexpr int kF2 = chunk_frames(kPad), kFB = kF2 / 16;
      constexpr int kB2Slots = kF2 * kPad / 4 / kThreads, kX2Slots = kF2 * (kCols / 4) / kThreads;
      static_assert(kB2Slots * kThreads * 4 == kF2 * kPad && kX2Slots * kThreads == kF2 * (kCols / 4), "whole slots");
      f32x4 pc2[kB2Slots], px2[kX2Slots];
      static_assert(!kMask || kF2 <= 32, "a masked chunk's flags are one 32-bit ballot");
      auto load_chunk = [&](int t0) {
        const float* __restrict__ src = table + (int64_t)t0 * kPad;
#pragma unroll
        for (int q = 0; q < kB2Slots; ++q) {
          const int e = 4 * (tid + kThreads * q);
          pc2[q] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (t0 + e / kPad < T) pc2[q] = *reinterpret_cast<const f32x4*>(src + e);
        }
      };
      auto store_chunk = [&](int buf) {
        float* bb = bc + buf * chunk_floats(kPad);
#pragma unroll
        for (int q = 0; q < kB2Slots; ++q) {
          const int e = 4 * (tid + kThreads * q);
          float* p = &bb[(e / kPad) * kLd2 + e % kPad];                 // (an even offset: 8-byte stores)
          *reinterpret_cast<float2*>(p) = make_float2(pc2[q][0], pc2[q][1]);
          *reinterpret_cast<float2*>(p + 2) = make_float2(pc2[q][2], pc2[q][3]);
        }
      };
      load_chunk(0);
      store_chunk(0);
      __syncthreads();

      // ---- phase 2: Y = B_chunk C, chunk by chunk ----
      cur = 0;
      for (int t0 = 0; t0 < T; t0 += kF2) {
        const bool more = t0 + kF2 < T;
        if (more) load_chunk(t0 + kF2);
        if (complement) {
#pragma unroll
          for (int q = 0; q < kX2Slots; ++q) px2[q] = load4<kVec>(x, t0 + xrow[q], T, col0 + xcol[q], n);
        }
        const bool fl2 = mask.kept(t0 + (tid & 31));
        const float* __restrict__ pa = bc + (kDouble ? cur : 0) * chunk_floats(kPad) + fcol * kLd2 + frow;
        const float* __restrict__ pc = cl + frow * kLdX + wave * 16 + fcol;
        f32x4 y[kFB];
#pragma unroll
        for (int f = 0; f < kFB; ++f) y[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int kk = 0; kk < kPad / 4; ++kk) {
          const float fc = pc[kk * 4 * kLdX];
          float fa[kFB];
#pragma unroll
          for (int f = 0; f < kFB; ++f) fa[f] = pa[f * 16 * kLd2 + kk * 4];
#pragma unroll
          for (int f = 0; f < kFB; ++f) y[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[f], fc, y[f], 0, 0, 0);
        }
#pragma unroll
        for (int f = 0; f < kFB; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) yl[(f * 16 + 4 * frow + r) * kLdY + wave * 16 + fcol] = y[f][r];
        if (kDouble && more) store_chunk(cur ^ 1);
        __syncthreads();                      // Y is whole; every wave is past its reads of this chunk of B
        if (!kDouble && more) store_chunk(0);
        const uint32_t rows2 = kept_rows(fl2);
#pragma unroll
        for (int q = 0; q < kX2Slots; ++q) {
          f32x4 v = *reinterpret_cast<const f32x4*>(&yl[xrow[q] * kLdY + xcol[q]]);
          if (complement) v = centre(px2[q], t0 + xrow[q], T, xcol[q], col0, n, mu) - v;
          if (kMask && !((rows2 >> xrow[q]) & 1)) v = f32x4{0.f, 0.f, 0.f, 0.f};      // selected, never multiplied
          store4<kVec>(o, t0 + xrow[q], T, col0 + xcol[q], n, v);
        }
        __syncthreads();                      // the next chunk overwrites Y
        cur ^= 1;
      }
    }
  }
}

// the means are a stream and want every wave the CU holds
#ifndef CGNN_FILTER_MEAN_PER_CU
#define CGNN_FILTER_MEAN_PER_CU 4
#endif

int check(int64_t S, int32_t T, int32_t n, int32_t K) {
  if (cgnn_check_cohort(S, n) != CGNN_OK || T < 2 || T > CGNN_MAX_FRAMES) return CGNN_EINVAL;
  return K < 0 || K > CGNN_FILTER_MAX_COMPONENTS ? CGNN_EINVAL : CGNN_OK;
}

int64_t table_bytes(int32_t T, int32_t K) { return cgnn_align_up((int64_t)T * pad_of(K) * (int64_t)sizeof(float), 16); }

template <int kPad, bool kVec, bool kMask = false>
int launch_as(const float* ts, int64_t S, int32_t T, int32_t n, int32_t complement, const float* table,
              int64_t table_stride, const double* mean, float* out, hipStream_t hs, const uint8_t* keep = nullptr) {
  constexpr size_t lds = lds_of(kPad);
  if (!cgnn_raise_lds_limit<k_filter<kPad, kVec, kMask>>(kLdsBytes)) return CGNN_ELAUNCH;
  const int64_t items = S * ((n + kCols - 1) / kCols);
  const int grid = cgnn_grid_for(items, cgnn_wg_per_cu_by_lds(lds, kLdsBytes));
  k_filter<kPad, kVec, kMask><<<grid, kThreads, lds, hs>>>(ts, S, T, n, complement, table, table_stride, mean, out,
                                                           keep);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

template <bool kVec>
int launch(int kpad, const float* ts, int64_t S, int32_t T, int32_t n, int32_t complement, const float* table,
           int64_t table_stride, const double* mean, float* out, hipStream_t hs) {
  switch (kpad) {
    case 0: return launch_as<0, kVec>(ts, S, T, n, complement, table, table_stride, mean, out, hs);
    case 32: return launch_as<32, kVec>(ts, S, T, n, complement, table, table_stride, mean, out, hs);
    case 64: return launch_as<64, kVec>(ts, S, T, n, complement, table, table_stride, mean, out, hs);
    case 96: return launch_as<96, kVec>(ts, S, T, n, complement, table, table_stride, mean, out, hs);
    case 128: return launch_as<128, kVec>(ts, S, T, n, complement, table, table_stride, mean, out, hs);
    case 160: return launch_as<160, kVec>(ts, S, T, n, complement, table, table_stride, mean, out, hs);
    case 192: return launch_as<192, kVec>(ts, S, T, n, complement, table, table_stride, mean, out, hs);
    case 224: return launch_as<224, kVec>(ts, S, T, n, complement, table, table_stride, mean, out, hs);
    default: return launch_as<256, kVec>(ts, S, T, n, complement, table, table_stride, mean, out, hs);
  }
}

// the masked complement form: pure centring (no table), or a basis of 32 or 64 columns per subject
template <bool kVec>
int launch_masked(int qpad, const float* ts, int64_t S, int32_t T, int32_t n, const float* basis, const double* mean,
                  float* out, hipStream_t hs, const uint8_t* keep) {
  const int64_t stride = (int64_t)T * qpad;
  switch (qpad) {
    case 0: return launch_as<0, kVec, true>(ts, S, T, n, 1, basis, stride, mean, out, hs, keep);
    case 32: return launch_as<32, kVec, true>(ts, S, T, n, 1, basis, stride, mean, out, hs, keep);
    default: return launch_as<64, kVec, true>(ts, S, T, n, 1, basis, stride, mean, out, hs, keep);
  }
}

}  // namespace

extern "C" int64_t cgnn_ingest_filter_workspace_bytes(int64_t S, int32_t T, int32_t n, int32_t K) {
  if (check(S, T, n, K) != CGNN_OK) return CGNN_EINVAL;
  return table_bytes(T, K) + S * n * (int64_t)sizeof(double);
}

extern "C" int cgnn_ingest_filter(const float* ts, int64_t S, int32_t T, int32_t n, const int32_t* comps, int32_t K,
                                  int32_t complement, void* workspace, int64_t workspace_bytes, float* out,
                                  int64_t out_bytes, void* stream) {
  Comps list;
  if (check(S, T, n, K) != CGNN_OK || cgnn_check_components(comps, K, T, &list) != CGNN_OK) return CGNN_EINVAL;
  if (K == 0 && !complement) return CGNN_EINVAL;              // (nothing kept: the band is empty)
  if (workspace_bytes < 0 || out_bytes < 0) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (!ts || !out || !workspace || cgnn_misaligned({ts, out}, 3) || cgnn_misaligned({workspace}, 15)) return CGNN_EINVAL;
  CGNN_NEED_BYTES(workspace, workspace_bytes, table_bytes(T, K) + S * n * (int64_t)sizeof(double));
  if (!cgnn_holds_floats(out_bytes, S * n, T)) return CGNN_EINVAL;      // out [S T][n]

  hipStream_t hs = cgnn_stream(stream);
  const int kpad = pad_of(K);
  float* table = static_cast<float*>(workspace);
  double* mean = reinterpret_cast<double*>(static_cast<unsigned char*>(workspace) + table_bytes(T, K));
  if (K > 0) {
    const int64_t blocks = ((int64_t)T * kpad + kThreads - 1) / kThreads;
    k_filter_basis<<<cgnn_grid_for(blocks, 8), kThreads, 0, hs>>>(list, K, kpad, T, table);
    CGNN_CHECK_LAUNCH();
  }
  const int64_t items = S * ((n + kCols - 1) / kCols);
  k_filter_mean<false><<<cgnn_grid_for(items, CGNN_FILTER_MEAN_PER_CU), kThreads, 0, hs>>>(ts, S, T, n, mean, nullptr);
  CGNN_CHECK_LAUNCH();
  const bool vec = n % 4 == 0 && !cgnn_misaligned({ts, out}, 15);
  return vec ? launch<true>(kpad, ts, S, T, n, complement, table, 0, mean, out, hs)
             : launch<false>(kpad, ts, S, T, n, complement, table, 0, mean, out, hs);
}

// ---- confound regression: the complement form against a basis per subject ----

extern "C" int64_t cgnn_ingest_regress_workspace_bytes(int64_t S, int32_t T, int32_t n) {
  if (check(S, T, n, 0) != CGNN_OK) return CGNN_EINVAL;
  return S * n * (int64_t)sizeof(double);
}

namespace {

// what both entry points check and do; masked (frame censoring): keep [S, T] selects the frames of the
// same two launches, and qpad == 0 with a null basis is masked centring alone
int regress_call(const float* ts, int64_t S, int32_t T, int32_t n, const uint8_t* keep, int64_t keep_bytes, bool masked,
                 const float* basis, int64_t basis_bytes, int32_t qpad, void* workspace, int64_t workspace_bytes,
                 float* out, int64_t out_bytes, void* stream) {
  if (check(S, T, n, 0) != CGNN_OK || (qpad != 32 && qpad != 64 && !(masked && qpad == 0))) return CGNN_EINVAL;
  if (keep_bytes < 0 || basis_bytes < 0 || workspace_bytes < 0 || out_bytes < 0) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (!ts || !out || !workspace || (masked && !keep) || (qpad == 0) != (basis == nullptr)) return CGNN_EINVAL;
  if (cgnn_misaligned({ts, out}, 3) || cgnn_misaligned({basis, workspace}, 15)) return CGNN_EINVAL;
  CGNN_NEED_BYTES(keep, keep_bytes, S * T);
  CGNN_NEED_BYTES(workspace, workspace_bytes, S * n * (int64_t)sizeof(double));
  // basis [S T][qpad] and out [S T][n]
  if (qpad && !cgnn_holds_floats(basis_bytes, S * T, qpad)) return CGNN_EINVAL;
  if (!cgnn_holds_floats(out_bytes, S * n, T)) return CGNN_EINVAL;

  hipStream_t hs = cgnn_stream(stream);
  double* mean = static_cast<double*>(workspace);
  const int grid = cgnn_grid_for(S * ((n + kCols - 1) / kCols), CGNN_FILTER_MEAN_PER_CU);
  if (masked)
    k_filter_mean<true><<<grid, kThreads, 0, hs>>>(ts, S, T, n, mean, keep);
  else
    k_filter_mean<false><<<grid, kThreads, 0, hs>>>(ts, S, T, n, mean, nullptr);
  CGNN_CHECK_LAUNCH();
  const bool vec = n % 4 == 0 && !cgnn_misaligned({ts, out}, 15);
  if (masked)
    return vec ? launch_masked<true>(qpad, ts, S, T, n, basis, mean, out, hs, keep)
               : launch_masked<false>(qpad, ts, S, T, n, basis, mean, out, hs, keep);
  const int64_t stride = (int64_t)T * qpad;
  return vec ? launch<true>(qpad, ts, S, T, n, 1, basis, stride, mean, out, hs)
             : launch<false>(qpad, ts, S, T, n, 1, basis, stride, mean, out, hs);
}

int check_design(int64_t S, int32_t T, int32_t K, int32_t q) {
  if (S < 0 || S >= ((int64_t)1 << 31) || T < 2 || T > CGNN_MAX_FRAMES) return CGNN_EINVAL;
  return K < 0 || q < 0 || K + q < 1 || K + q > CGNN_CONFOUND_MAX ? CGNN_EINVAL : CGNN_OK;
}

}  // namespace

extern "C" int cgnn_ingest_regress(const float* ts, int64_t S, int32_t T, int32_t n, const float* basis,
                                   int64_t basis_bytes, int32_t qpad, void* workspace, int64_t workspace_bytes,
                                   float* out, int64_t out_bytes, void* stream) {
  return regress_call(ts, S, T, n, nullptr, 0, false, basis, basis_bytes, qpad, workspace, workspace_bytes, out,
                      out_bytes, stream);
}

extern "C" int cgnn_ingest_regress_masked(const float* ts, int64_t S, int32_t T, int32_t n, const uint8_t* keep,
                                          int64_t keep_bytes, const float* basis, int64_t basis_bytes, int32_t qpad,
                                          void* workspace, int64_t workspace_bytes, float* out, int64_t out_bytes,
                                          void* stream) {
  return regress_call(ts, S, T, n, keep, keep_bytes, true, basis, basis_bytes, qpad, workspace, workspace_bytes, out,
                      out_bytes, stream);
}

// ---- the design of a regression under censoring: [table values | confounds] per subject ----

extern "C" int64_t cgnn_ingest_design_bytes(int64_t S, int32_t T, int32_t K, int32_t q) {
  if (check_design(S, T, K, q) != CGNN_OK) return CGNN_EINVAL;
  return S * T * (K + q) * (int64_t)sizeof(float);            // (S < 2^31, T <= 2^30, 256: below 2^63)
}

extern "C" int cgnn_ingest_design(const float* confounds, int64_t S, int32_t T, int32_t q, const int32_t* comps,
                                  int32_t K, float* design, int64_t design_bytes, void* stream) {
  Comps list;
  if (check_design(S, T, K, q) != CGNN_OK || design_bytes < 0) return CGNN_EINVAL;
  if (cgnn_check_components(comps, K, T, &list) != CGNN_OK || (q == 0) != (confounds == nullptr)) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (!design || cgnn_misaligned({confounds, design}, 3)) return CGNN_EINVAL;
  CGNN_NEED_BYTES(design, design_bytes, cgnn_ingest_design_bytes(S, T, K, q));
  const int64_t blocks = (S * T * (K + q) + kThreads - 1) / kThreads;
  k_design<<<cgnn_grid_for(blocks, 8), kThreads, 0, cgnn_stream(stream)>>>(list, K, confounds, S, T, q, design);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
