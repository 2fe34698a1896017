// butterworth.hip -- a zero-phase IIR filter in second-order sections over a device-resident cohort of ROI time series
// (float [S, T, n], one row per frame): cgnn_ingest_butterworth, scipy.signal.sosfiltfilt with its default
// padding (padtype="odd", padlen=None), which is nilearn's signal.clean(filter="butterworth").  The same call serves
// confounds [S, T, q].
//
// Per subject and column i, everything in fp64, with L sections (b0 b1 b2 1 a1 a2), edge = 3 (2 L + 1 - min(#b2 == 0,
// #a2 == 0)) and T > edge:
//     level      d[t] = double(x[t, i]) - double(x[0, i])                       (so d[0] == 0)
//     extension  frame e of T + 2 edge:  -d[edge - e] on the left (2 d[0] - d[edge - e]),  d[e - edge] inside,
//                2 d[T-1] - d[2 (T-1) - (e - edge)] on the right; formed on load, never stored
//     a section  transposed direct form II:   y = fma(b0, x, z0);   z0 = fma(-a1, y, fma(b1, x, z1));
//                z1 = fma(-a2, y, b2 * x);   the sections in the given order, y of one the x of the next
//     forward    over the T + 2 edge frames from z = zi * ext[0], with zi = scale (g - b0, b2 - a2 g),
//                g = (b0 + b1 + b2) / (1 + a1 + a2) and scale the product of g over the earlier sections (sosfilt_zi):
//                the states a constant input holds
//     backward   over the forward outputs last to first from z = zi * (the last forward output); the value between the
//                two passes is never rounded to fp32
//     out[t, i]  = fl32(w[edge + t] + lvl):  lvl = double(x[0, i]) if add_level, else 0.0;   one rounding
// The extension commutes with the level shift and zi makes a constant input give a constant output, so in exact
// arithmetic sosfiltfilt(x) = sosfiltfilt(d) + H(1)^2 x[0]: H(1)^2 is 0 for a high- or band-pass and 1 for a low-pass,
// which is what add_level says.  A constant column has d == 0 and every state exactly 0: it comes out as exactly 0.0, or
// as exactly its value under a low-pass, and an offset of 10^4 costs no accuracy.
//
//   k_butter<L>   an item is (subject, 64 consecutive columns), a lane per column, ONE WAVE per item; a persistent grid of
//                 workgroups of 4 independent waves strides over the items.  L is a template parameter (1 .. 8): the
//                 section loop is unrolled and the 2 L states live in registers; the coefficients are kernel arguments,
//                 the same for every lane.  The wave walks the frames in segments of a fixed length, so that no code
//                 depends on a count: chunks of kC = 48 real frames, and segments of 8 and of 1 for the pads and the
//                 last real frames.  A segment's rows of x (256 bytes a row) are loaded together and the recurrence runs
//                 unrolled in registers.
//       left pad      frames 0 .. edge - 1 from the sources x[edge] down to x[1]; the state it leaves is boundary 0.
//       forward       the frames edge .. T + 2 edge - 1 in segments that START AT e = edge, the first real frame: T / 48
//                     chunks, then the tail (T % 48 real frames and the right pad).  Only the 2 L states at each
//                     segment's start are kept: fp64 [segments][2 L][64] in a slab of the wave's own in the workspace
//                     (per wave of the launch, not per subject).
//       backward      the segments last to first: a segment's forward outputs are formed again from the boundary before
//                     it (the same code on the same operands, a second read of x), then the reversed recurrence runs
//                     over them and the real frames are stored as fp32.  It stops at e = edge: the left pad is only ever
//                     needed to reach the forward state there.
//                     The forward outputs of 64 columns are (T + 2 edge) * 512 bytes and fit nowhere on chip; writing
//                     them all to a slab would move 8 bytes per value out and in again, where the second read of x costs 4.
//
// out == ts is correct because a wave owns all frames of its columns and
//   * reads x[0] and x[T-1] once at the start and keeps them;
//   * forms the right pad, whose sources are x[T-1-edge .. T-2], in the segments that are walked first in the backward
//     pass, and every segment loads all its rows, sources of the pad included, before it stores anything: when the first
//     store happens no pad frame is left to form;
//   * thereafter loads a segment's real frames before it stores those same frames, and never looks at a later frame
//     again;
//   * never revisits the left pad's sources x[1 .. edge] in the backward pass.
// No atomics, no work assignment depends on the grid, and which buffer `out` is changes no arithmetic: the same bits on
// every run, for every grid, in place and out of place.  Columns never mix (a lane is a column): a NaN anywhere in a column
// reaches every frame of that column (the recurrence runs both ways) and no other column.  Element offsets into `ts` and
// `out` are 64-bit.
#include <cmath>

#include "series_request.h"

#pragma clang fp contract(off)                // every fused multiply-add below is written as one

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;                 // 4 waves, each with items of its own
constexpr int kWaves = kThreads / kWave;
constexpr int kCols = 64;                     // columns of an item
constexpr int kMaxL = CGNN_BUTTER_MAX_SECTIONS;
// frames of a chunk, and workgroups per cgnn_fused_grid() unit: what the chunk's registers admit, chosen by measurement
// (at five sections 32 frames: 164 VGPRs, 48: 174, 64: 207 -- DESIGN.md 4.3o)
#ifndef CGNN_BUTTER_CHUNK
#define CGNN_BUTTER_CHUNK 48
#endif
#ifndef CGNN_BUTTER_PER_CU
#define CGNN_BUTTER_PER_CU 2
#endif
constexpr int kC = CGNN_BUTTER_CHUNK;
constexpr int kS = 8;                         // frames of a short segment: the pads and the last real frames
constexpr int kPerCu = CGNN_BUTTER_PER_CU;
static_assert(kC % kS == 0, "a chunk is a whole number of short segments");

// the sections and the initial-state coefficients, by value: the same for every lane
struct Sections {
  double b0[kMaxL], b1[kMaxL], b2[kMaxL], a1[kMaxL], a2[kMaxL], zi0[kMaxL], zi1[kMaxL];
};

int64_t items_of(int64_t S, int32_t n) { return S * ((n + kCols - 1) / kCols); }

int grid_of(int64_t S, int32_t n) { return cgnn_grid_for((items_of(S, n) + kWaves - 1) / kWaves, kPerCu); }

// the slab of a wave: fp64 [segments][2 L][64].  The frames from e = edge on are T / kC chunks and a tail of fewer than
// kC + edge frames in segments of kS and of one; the largest edge a filter of L sections has is 3 (2 L + 1).
int64_t slab_stride(int32_t T, int32_t L) {
  const int64_t segments = T / kC + (kC - 1 + 3 * (2 * L + 1)) / kS + kS - 1;
  return segments * 2 * L * kCols;
}

template <int L>
struct State {
  double z0[L], z1[L];
};

// one frame through the L sections
template <int L>
__device__ __forceinline__ double step(const Sections& c, State<L>& z, double v) {
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const double y = fma(c.b0[l], v, z.z0[l]);
    z.z0[l] = fma(-c.a1[l], y, fma(c.b1[l], v, z.z1[l]));
    z.z1[l] = fma(-c.a2[l], y, c.b2[l] * v);
    v = y;
  }
  return v;
}

template <int L>
__device__ __forceinline__ void start(const Sections& c, State<L>& z, double v) {
#pragma unroll
  for (int l = 0; l < L; ++l) z.z0[l] = c.zi0[l] * v, z.z1[l] = c.zi1[l] * v;
}

// N frames from f0 on of one column as the recurrence takes them (N is kC, kS or 1: nothing in a segment's code depends
// on a count).  kLeft: f counts the left pad, frame e = f, source x[edge - f], and 2 d[0] - d = 0 - d.  kReal: f = e - edge
// and every frame is a real one, x[f].  kTail: f = e - edge, a real frame for f < T and beyond it the right pad, source
// x[2 (T-1) - f], 2 dl - d with dl = d[T-1].  x may be `out`: not __restrict__.
enum Kind { kLeft, kReal, kTail };

template <int N, Kind kKind>
__device__ __forceinline__ void load_frames(double (&d)[N], const float* x, int n, int cc, int T, int edge, int f0,
                                            double x0, double dl) {
  float raw[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int f = f0 + i;
    const int src = kKind == kReal ? f : kKind == kLeft ? edge - f : f < T ? f : 2 * (T - 1) - f;
    raw[i] = (x + (int64_t)src * n)[cc];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double v = (double)raw[i] - x0;
    if constexpr (kKind == kReal) d[i] = v;
    else if constexpr (kKind == kLeft) d[i] = 0.0 - v;
    else d[i] = f0 + i < T ? v : fma(2.0, dl, -v);
  }
}

// the forward recurrence over N loaded frames, its outputs left in d
template <int L, int N>
__device__ __forceinline__ void run_frames(const Sections& c, State<L>& z, double (&d)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) d[i] = step<L>(c, z, d[i]);
}

// the reversed recurrence over N forward outputs, the real frames stored as soon as they are known
template <int L, int N, Kind kKind>
__device__ __forceinline__ void back_frames(const Sections& c, State<L>& z, const double (&d)[N], int f0, int T, int n,
                                            int cc, double lvl, float* o) {
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    const double w = step<L>(c, z, d[i]);
    if (kKind == kReal || f0 + i < T) (o + (int64_t)(f0 + i) * n)[cc] = (float)(w + lvl);
  }
}

template <int L>
__device__ __forceinline__ void put_state(double* b, const State<L>& z) {
#pragma unroll
  for (int l = 0; l < L; ++l) b[(2 * l) * kCols] = z.z0[l], b[(2 * l + 1) * kCols] = z.z1[l];
}

template <int L>
__device__ __forceinline__ void get_state(const double* b, State<L>& z) {
#pragma unroll
  for (int l = 0; l < L; ++l) z.z0[l] = b[(2 * l) * kCols], z.z1[l] = b[(2 * l + 1) * kCols];
}

// a segment of N frames in the forward pass: the states at its start to the slab (the left pad's are never needed), then
// the recurrence; returns its last output
template <int L, int N, Kind kKind>
__device__ __forceinline__ double fwd_segment(const Sections& c, State<L>& zf, double* b, const float* x, int n, int cc,
                                              int T, int edge, int f0, double x0, double dl) {
  double d[N];
  if constexpr (kKind != kLeft) put_state<L>(b, zf);
  load_frames<N, kKind>(d, x, n, cc, T, edge, f0, x0, dl);
  run_frames<L, N>(c, zf, d);
  return d[N - 1];
}

// the same segment in the backward pass: its forward outputs again from the states at its start, then the reversed
// recurrence over them
template <int L, int N, Kind kKind>
__device__ __forceinline__ void bwd_segment(const Sections& c, State<L>& zb, const double* b, const float* x, int n, int cc,
                                            int T, int edge, int f0, double x0, double dl, double lvl, float* o) {
  double d[N];
  State<L> zf;
  get_state<L>(b, zf);
  load_frames<N, kKind>(d, x, n, cc, T, edge, f0, x0, dl);
  run_frames<L, N>(c, zf, d);
  back_frames<L, N, kKind>(c, zb, d, f0, T, n, cc, lvl, o);
}

// `ts` and `out` may be the same array: neither is __restrict__
template <int L>
__global__ __launch_bounds__(kThreads) void k_butter(const float* ts, int64_t S, int T, int n, int edge, int add_level,
                                                     Sections c, double* slab, int64_t stride, float* out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wid = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * kWaves;
  double* sl = slab + wid * stride + lane;                      // [segment][2 L][64]: the states at the segment's start
  constexpr int kB = 2 * L * kCols;                             // doubles of a boundary
  const int panels = (n + kCols - 1) / kCols;
  const int64_t items = S * panels;
  // the frames from e = edge on, f = e - edge in [0, T + edge): nfull chunks of kC real frames, then the tail -- the last
  // real frames and the right pad -- in n8 segments of kS frames and n1 of one
  const int nfull = T / kC, tail0 = nfull * kC;
  const int n8 = (T + edge - tail0) / kS, n1 = (T + edge - tail0) % kS, one0 = tail0 + n8 * kS;
  for (int64_t item = wid; item < items; item += waves) {
    const int64_t s = item / panels;
    // a lane past n walks column n - 1 along: it loads and stores what that column's own lane does, the same values at
    // the same addresses in the same instructions, so that no store sits under a lane mask
    const int col = (int)(item - s * panels) * kCols + lane;
    const int cc = col < n ? col : n - 1;
    const float* x = ts + s * T * n;
    float* o = out + s * T * n;
    const double x0 = (double)x[cc];
    const double dl = (double)(x + (int64_t)(T - 1) * n)[cc] - x0;
    const double lvl = add_level ? x0 : 0.0;
    State<L> zf;
    // the left pad, whose first frame starts the states
    start<L>(c, zf, 0.0 - ((double)(x + (int64_t)edge * n)[cc] - x0));
    int f = 0;
    for (; f + kC <= edge; f += kC) fwd_segment<L, kC, kLeft>(c, zf, sl, x, n, cc, T, edge, f, x0, dl);
    for (; f + kS <= edge; f += kS) fwd_segment<L, kS, kLeft>(c, zf, sl, x, n, cc, T, edge, f, x0, dl);
    for (; f < edge; ++f) fwd_segment<L, 1, kLeft>(c, zf, sl, x, n, cc, T, edge, f, x0, dl);
    // forward: the states at every segment's start, and the last output of all
    double last = 0.0;
    for (int k = 0; k < nfull; ++k)
      fwd_segment<L, kC, kReal>(c, zf, sl + (int64_t)k * kB, x, n, cc, T, edge, k * kC, x0, dl);
    for (int j = 0; j < n8; ++j)
      last = fwd_segment<L, kS, kTail>(c, zf, sl + (int64_t)(nfull + j) * kB, x, n, cc, T, edge, tail0 + j * kS, x0, dl);
    for (int j = 0; j < n1; ++j)
      last = fwd_segment<L, 1, kTail>(c, zf, sl + (int64_t)(nfull + n8 + j) * kB, x, n, cc, T, edge, one0 + j, x0, dl);
    // backward from the last forward output: the segments last to first
    State<L> zb;
    start<L>(c, zb, last);
    for (int j = n1 - 1; j >= 0; --j)
      bwd_segment<L, 1, kTail>(c, zb, sl + (int64_t)(nfull + n8 + j) * kB, x, n, cc, T, edge, one0 + j, x0, dl, lvl, o);
    for (int j = n8 - 1; j >= 0; --j)
      bwd_segment<L, kS, kTail>(c, zb, sl + (int64_t)(nfull + j) * kB, x, n, cc, T, edge, tail0 + j * kS, x0, dl, lvl, o);
    for (int k = nfull - 1; k >= 0; --k)
      bwd_segment<L, kC, kReal>(c, zb, sl + (int64_t)k * kB, x, n, cc, T, edge, k * kC, x0, dl, lvl, o);
  }
}

int check(int64_t S, int32_t T, int32_t n, int32_t L) {
  if (cgnn_check_cohort(S, n) != CGNN_OK || T < 2 || T > CGNN_MAX_FRAMES) return CGNN_EINVAL;
  return L < 1 || L > kMaxL ? CGNN_EINVAL : CGNN_OK;
}

int64_t slab_bytes(int64_t S, int32_t T, int32_t n, int32_t L) {
  return (int64_t)grid_of(S, n) * kWaves * slab_stride(T, L) * (int64_t)sizeof(double);
}

// (CGNN_OK, the sections as the kernel takes them, edge) of valid host sections [L][6]
int prepare(const double* sos, int32_t L, Sections* c, int32_t* edge) {
  int nb = 0, na = 0;
  double scale = 1.0;
  *c = Sections{};
  for (int l = 0; l < L; ++l) {
    const double* r = sos + 6 * l;
    for (int j = 0; j < 6; ++j)
      if (!std::isfinite(r[j])) return CGNN_EINVAL;
    const double den = 1.0 + r[4] + r[5];
    if (r[3] != 1.0 || den == 0.0) return CGNN_EINVAL;
    const double g = (r[0] + r[1] + r[2]) / den;
    c->b0[l] = r[0], c->b1[l] = r[1], c->b2[l] = r[2], c->a1[l] = r[4], c->a2[l] = r[5];
    c->zi0[l] = scale * (g - r[0]);
    c->zi1[l] = scale * (r[2] - r[5] * g);
    scale *= g;
    nb += r[2] == 0.0;
    na += r[5] == 0.0;
  }
  *edge = 3 * (2 * L + 1 - (nb < na ? nb : na));
  return CGNN_OK;
}

template <int L>
void launch(int grid, hipStream_t hs, const float* ts, int64_t S, int T, int n, int edge, int add_level,
            const Sections& c, double* slab, int64_t stride, float* out) {
  k_butter<L><<<grid, kThreads, 0, hs>>>(ts, S, T, n, edge, add_level, c, slab, stride, out);
}

}  // namespace

extern "C" int64_t cgnn_ingest_butterworth_workspace_bytes(int64_t S, int32_t T, int32_t n, int32_t L) {
  if (check(S, T, n, L) != CGNN_OK) return CGNN_EINVAL;
  return slab_bytes(S, T, n, L);
}

extern "C" int cgnn_ingest_butterworth(const float* ts, int64_t S, int32_t T, int32_t n, const double* sos, int32_t L,
                                       int32_t add_level, void* workspace, int64_t workspace_bytes, float* out,
                                       int64_t out_bytes, void* stream) {
  if (check(S, T, n, L) != CGNN_OK || !sos || (add_level != 0 && add_level != 1)) return CGNN_EINVAL;
  Sections c;
  int32_t edge = 0;
  if (prepare(sos, L, &c, &edge) != CGNN_OK || T <= edge) return CGNN_EINVAL;
  if (workspace_bytes < 0 || out_bytes < 0) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (!ts || !out || !workspace || cgnn_misaligned({ts, out}, 3) || cgnn_misaligned({workspace}, 15)) return CGNN_EINVAL;
  CGNN_NEED_BYTES(workspace, workspace_bytes, slab_bytes(S, T, n, L));
  if (!cgnn_holds_floats(out_bytes, S * n, T)) return CGNN_EINVAL;      // out [S T][n]

  hipStream_t hs = cgnn_stream(stream);
  const int grid = grid_of(S, n);
  double* slab = static_cast<double*>(workspace);
  const int64_t stride = slab_stride(T, L);
  switch (L) {
    case 1: launch<1>(grid, hs, ts, S, T, n, edge, add_level, c, slab, stride, out); break;
    case 2: launch<2>(grid, hs, ts, S, T, n, edge, add_level, c, slab, stride, out); break;
    case 3: launch<3>(grid, hs, ts, S, T, n, edge, add_level, c, slab, stride, out); break;
    case 4: launch<4>(grid, hs, ts, S, T, n, edge, add_level, c, slab, stride, out); break;
    case 5: launch<5>(grid, hs, ts, S, T, n, edge, add_level, c, slab, stride, out); break;
    case 6: launch<6>(grid, hs, ts, S, T, n, edge, add_level, c, slab, stride, out); break;
    case 7: launch<7>(grid, hs, ts, S, T, n, edge, add_level, c, slab, stride, out); break;
    default: launch<8>(grid, hs, ts, S, T, n, edge, add_level, c, slab, stride, out); break;
  }
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
