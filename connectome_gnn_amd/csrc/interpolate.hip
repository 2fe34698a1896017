// interpolate.hip -- the censored frames of a device-resident cohort of ROI time series (float [S, T, n], one row per
// frame) replaced by a cubic spline through the kept ones: cgnn_ingest_interpolate, the step that lets
// the orthogonal DCT band-pass of filter.hip run under a frame mask.  The same call serves confounds [S, T, q].
//
// Per subject, with keep [S, T] and t_0 < .. < t_{m-1} its kept frames, and per column i, in fp64: y_k = x[t_k, i],
// h_k = t_{k+1} - t_k, D_k = y_{k+1} - y_k.  Kept frames are bit copies; m == 0 gives zeros, m == 1 the one value; a
// censored frame before t_0 / after t_{m-1} takes the bits of x[t_0] / x[t_{m-1}]; inside (t_k, t_{k+1}) the C2 cubic
// spline with not-a-knot ends (the line at m == 2, the parabola at m == 3) in Hermite form on the knot derivatives s_k,
// with u = (t - t_k) / h_k:
//     v = y_k + u^2 (3 - 2u) D_k + h_k u (1-u)^2 s_k - h_k u^2 (1-u) s_{k+1},          rounded to fp32 once.
// s solves the tridiagonal system of cgnn.h (scipy's rows) by the Thomas recurrence
//     d'_k = (r_k - a_k d'_{k-1}) / p_k,   p_k = b_k - a_k c'_{k-1},   c'_k = c_k / p_k,   s_k = d'_k - c'_k s_{k+1}.
// The matrix depends on the mask alone, and every right-hand side is linear in two differences: r_k = pA_k P + pB_k Q
// with (P, Q) = (D_{k-1}, D_k), except (D_0, D_1) in row 0 and (D_{m-3}, D_{m-2}) in row m-1 (a difference that does
// not exist is 0 and its coefficient too).  So per subject and knot five numbers are formed once,
//     A_k = pA_k / p_k,  B_k = pB_k / p_k,  L_k = a_k / p_k,  c'_k,  1 / h_k,
// and a column's recurrence is   d'_k = A_k P + B_k Q - L_k d'_{k-1}:   no division in the sweep.
//
//   k_interp_knots    a wave per subject, grid stride: the kept frames compacted in order (ballot + prefix count of 64
//                     flags at a time) into kn [S, T], and their number m.
//   k_interp_factors  a wave per subject: the rows above and the Thomas factors, a sequential fp64 recurrence that every
//                     lane runs alike on knots fetched 64 at a time; lane j keeps row k0 + j and the 64 rows are stored
//                     together.  Two divisions a row (1 / p_k and 1 / h_k).
//   k_interp          an item is (subject, 64 consecutive columns), a lane per column, ONE WAVE per item; a persistent
//                     grid of workgroups of 4 independent waves strides over the items (12 waves a CU).  The wave walks
//                     the knots in chunks of 12: the chunk's knot indices and factors are one load each (lane l holds
//                     knot k0 + l; a readlane with a constant lane makes them scalars), its 15 rows of x (256 bytes a
//                     row) are loaded together, and the recurrence runs unrolled in registers.
//       forward       chunk after chunk, keeping only d' at each chunk's last knot: fp64 [chunks][64] in a slab of the
//                     wave's own in the workspace (per wave of the launch, not per subject; 51 KB at T = 1200).
//       backward      the chunks last to first: a chunk's d' are formed again from the boundary before it (the same
//                     code on the same operands, a second read of the kept frames), then s_k = d'_k - c'_k s_{k+1}
//                     downwards, and each gap (t_k, t_{k+1}) is evaluated and stored as soon as s_k is known; the kept
//                     frames go to `out` in passing when out != ts.
//                     d' of every knot of 64 columns is 614 KB at T = 1200 and fits nowhere on chip; writing it all to
//                     a slab instead would move 8 bytes per kept value out and in again, twice the series, where the
//                     second read costs once the series.
//
// out == ts is correct because a wave owns all frames of its columns, reads kept frames only and writes censored frames
// only.  No atomics, no work assignment depends on the grid, and which buffer `out` is changes no arithmetic: the same
// bits on every run, for every grid, in place and out of place.  Columns never mix (a lane is a column); a censored
// frame's stored value is never loaded.  Element offsets into `ts` and `out` are 64-bit.
#include "series_request.h"

#pragma clang fp contract(off)                // every fused multiply-add below is written as one

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;                 // k_interp: 4 waves, each with items of its own
constexpr int kWaves = kThreads / kWave;
constexpr int kCols = 64;                     // columns of an item
// knots of a chunk, and workgroups of k_interp per cgnn_fused_grid() unit: what the chunk's registers admit (16 knots:
// 189 VGPRs and 2; 12: 159 and 3; 8: 123 and 4 -- measured in DESIGN.md 4.3m)
#ifndef CGNN_INTERP_CHUNK
#define CGNN_INTERP_CHUNK 12
#endif
#ifndef CGNN_INTERP_PER_CU
#define CGNN_INTERP_PER_CU 3
#endif
constexpr int kC = CGNN_INTERP_CHUNK;
constexpr int kY = kC + 3;                    // rows of x a chunk needs: knots k0 - 2 .. k0 + kC
constexpr int kPerCu = CGNN_INTERP_PER_CU;
constexpr int kPrepPerCu = 16;                // single-wave workgroups of the two per-subject kernels
constexpr int64_t kMaxKnots = (int64_t)1 << 50;               // S T: the byte counts below stay inside an int64
static_assert(kY <= kWave && kC >= 2, "a chunk's knots are one load of a wave; row 0 looks two knots ahead");

// the workspace: five fp64 and one int32 per (subject, frame) -- used up to the subject's m --, m per subject, and the
// boundary slabs [waves of the largest launch][chunks of T][64] fp64
struct Layout {
  int64_t a, b, l, c, ih, kn, cnt, slab, slab_stride, total;
};

int64_t chunks_of(int32_t T) { return ((int64_t)T + kC - 1) / kC; }

Layout layout(int64_t S, int32_t T) {
  const int64_t st = S * T;
  Layout w;
  w.a = 0;
  w.b = 8 * st;
  w.l = 16 * st;
  w.c = 24 * st;
  w.ih = 32 * st;
  w.kn = 40 * st;
  w.cnt = 44 * st;
  w.slab = cgnn_align_up(w.cnt + 4 * S, 16);
  w.slab_stride = chunks_of(T) * kCols;
  w.total = w.slab + (int64_t)kPerCu * cgnn_fused_grid() * kWaves * w.slab_stride * (int64_t)sizeof(double);
  return w;
}

__global__ __launch_bounds__(kWave) void k_interp_knots(const uint8_t* __restrict__ keep, int64_t S, int T,
                                                        int32_t* __restrict__ kn, int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x;
  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const uint8_t* __restrict__ kp = keep + s * T;
    int32_t* __restrict__ k = kn + s * T;
    int m = 0;
    for (int t0 = 0; t0 < T; t0 += kWave) {
      const int t = t0 + lane;
      const bool f = t < T && kp[t] != 0;
      const uint64_t flags = __ballot(f);
      if (f) k[m + __popcll(flags & (((uint64_t)1 << lane) - 1))] = t;
      m += __popcll(flags);
    }
    if (lane == 0) cnt[s] = m;
  }
}

__global__ __launch_bounds__(kWave) void k_interp_factors(const int32_t* __restrict__ kn,
                                                          const int32_t* __restrict__ cnt, int64_t S, int T,
                                                          double* __restrict__ fa, double* __restrict__ fb,
                                                          double* __restrict__ fl, double* __restrict__ fc,
                                                          double* __restrict__ fih) {
  const int lane = threadIdx.x;
  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const int m = cnt[s];
    if (m < 2) continue;                      // nothing to solve: k_interp reads no factor of this subject
    const int64_t base = s * T;
    const int32_t* __restrict__ k = kn + base;
    const double h0 = (double)(k[1] - k[0]);
    const double h1 = m >= 3 ? (double)(k[2] - k[1]) : 0.0;
    const double hl = m >= 3 ? (double)(k[m - 2] - k[m - 3]) : 0.0;     // h_{m-3}
    double cprev = 0.0, ihprev = 0.0;
    int tprev = 0;
    for (int k0 = 0; k0 < m; k0 += kWave) {
      const int tk = k0 + lane < m ? k[k0 + lane] : 0;
      const int tn = k0 + kWave < m ? k[k0 + kWave] : 0;
      const int rows = m - k0 < kWave ? m - k0 : kWave;
      double ra = 0.0, rb = 0.0, rl = 0.0, rc = 0.0, rih = 0.0;
      for (int j = 0; j < rows; ++j) {
        const int r = k0 + j;
        const int tc = __builtin_amdgcn_readlane(tk, j);
        const int tx = j + 1 < kWave ? __builtin_amdgcn_readlane(tk, (j + 1) & (kWave - 1)) : tn;
        const double hp = (double)(tc - tprev);                         // h_{r-1} (r >= 1)
        const double hn = (double)(tx - tc);                            // h_r (r <= m - 2)
        const double ih = r < m - 1 ? 1.0 / hn : 0.0;
        double a, b, c, pa, pb;
        if (m == 2) {                         // the line: s_0 = s_1 = D_0 / h_0
          a = 0.0, b = 1.0, c = 0.0;
          pa = r == 0 ? ih : 0.0;
          pb = r == 0 ? 0.0 : ihprev;
        } else if (r == 0) {
          a = 0.0;
          if (m == 3) {                       // s_0 + s_1 = 2 D_0 / h_0
            b = 1.0, c = 1.0, pa = 2.0 * ih, pb = 0.0;
          } else {                            // not-a-knot: (P, Q) = (D_0, D_1)
            const double d = h0 + h1;
            b = h1, c = d;
            pa = (h0 + 2.0 * d) * h1 / (d * h0);
            pb = h0 * h0 / (d * h1);
          }
        } else if (r == m - 1) {              // (P, Q) = (D_{m-3}, D_{m-2}); hp = h_{m-2}
          c = 0.0;
          if (m == 3) {                       // s_1 + s_2 = 2 D_1 / h_1
            a = 1.0, b = 1.0, pa = 0.0, pb = 2.0 * ihprev;
          } else {
            const double d = hl + hp;
            a = d, b = hl;
            pa = hp * hp / (d * hl);
            pb = (2.0 * d + hp) * hl / (d * hp);
          }
        } else {                              // 3 (h_r D_{r-1} / h_{r-1} + h_{r-1} D_r / h_r)
          a = hn, b = 2.0 * (hp + hn), c = hp;
          pa = 3.0 * hn * ihprev;
          pb = 3.0 * hp * ih;
        }
        const double ip = 1.0 / (b - a * cprev);
        cprev = c * ip;
        if (lane == j) ra = pa * ip, rb = pb * ip, rl = a * ip, rc = cprev, rih = ih;
        ihprev = ih;
        tprev = tc;
      }
      if (k0 + lane < m) {
        const int64_t e = base + k0 + lane;
        fa[e] = ra, fb[e] = rb, fl[e] = rl, fc[e] = rc, fih[e] = rih;
      }
    }
  }
}

// lane l's value of a register, l a constant: a scalar for every lane
__device__ __forceinline__ double lane_value(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}

// a chunk of kC knots k0 .. k0 + kC - 1 of one item, as its wave holds it.  kEdge == false, a chunk strictly inside the
// knot list (k0 > 0 and k0 + kC < m): every knot k0 - 2 .. k0 + kC exists and every row is an interior row, so nothing
// in its code is conditional.  The first chunk, the last one and a chunk that is not full take kEdge == true.  Which of
// the two a chunk takes depends on k0 and m alone.
struct Chunk {
  int tl;                                     // lane l < kY: t_{k0 - 2 + l}, -1 where there is no such knot
  double fa, fb, fl, fc, fih;                 // lane l < kC: the factors of knot k0 + l
  float y[kY];                                // y[i] = x[t_{k0 - 2 + i}], 0 where there is no such knot
  double d[kC];                               // d'_{k0 + i}
};

struct Factors {
  const int32_t* __restrict__ kn;
  const double* __restrict__ a;
  const double* __restrict__ b;
  const double* __restrict__ l;
  const double* __restrict__ c;
  const double* __restrict__ ih;
};

// x: the subject's frames (a pointer that may be `out`: not __restrict__), the same in every lane, so that a row's
// address is a scalar and the lane adds its column cc; base: s * T
template <bool kEdge>
__device__ __forceinline__ void load_chunk(Chunk& ch, const Factors& f, int64_t base, int k0, int m, const float* x, int n,
                                           int cc, int lane) {
  const int j = k0 - 2 + lane;
  if constexpr (kEdge) ch.tl = lane < kY && j >= 0 && j < m ? f.kn[base + j] : -1;
  else ch.tl = f.kn[base + (lane < kY ? j : k0)];
  const bool has = lane < kC && (!kEdge || k0 + lane < m);
  const int64_t e = base + k0 + (has ? lane : 0);
  ch.fa = has ? f.a[e] : 0.0;
  ch.fb = has ? f.b[e] : 0.0;
  ch.fl = has ? f.l[e] : 0.0;
  ch.fc = has ? f.c[e] : 0.0;
  ch.fih = has ? f.ih[e] : 0.0;
#pragma unroll
  for (int i = 0; i < kY; ++i) {
    const int t = __builtin_amdgcn_readlane(ch.tl, i);
    ch.y[i] = !kEdge || t >= 0 ? (x + (int64_t)t * n)[cc] : 0.0f;
  }
}

// d'_k of the chunk's knots from d' of the knot before it; returns d' of the chunk's last knot
template <bool kEdge>
__device__ __forceinline__ double solve_chunk(Chunk& ch, int k0, int m, double dprev) {
  // D_{k0 - 2 + li}, 0 where y_j or y_{j+1} does not exist
  const auto diff = [&](int li) {
    const int j = k0 - 2 + li;
    return !kEdge || (j >= 0 && j <= m - 2) ? (double)ch.y[li + 1] - (double)ch.y[li] : 0.0;
  };
#pragma unroll
  for (int i = 0; i < kC; ++i) {
    const int k = k0 + i;
    if (!kEdge || k < m) {                    // (the same for every lane)
      double p, q;
      if (kEdge && i == 0 && k == 0) p = diff(2), q = diff(3);          // (D_0, D_1)
      else if (kEdge && k == m - 1) p = diff(i), q = diff(i + 1);       // (D_{m-3}, D_{m-2})
      else p = diff(i + 1), q = diff(i + 2);                            // (D_{k-1}, D_k)
      const double rhs = fma(lane_value(ch.fa, i), p, lane_value(ch.fb, i) * q);
      dprev = fma(-lane_value(ch.fl, i), dprev, rhs);
      ch.d[i] = dprev;
    }
  }
  return dprev;
}

// s_k of the chunk's knots downwards from s of the knot after it (snext), every gap (t_k, t_{k+1}) evaluated and stored
// as soon as s_k is known; o: the subject's frames of `out`; returns s of the chunk's first knot
template <bool kEdge>
__device__ __forceinline__ double back_chunk(const Chunk& ch, int k0, int m, int T, int n, int cc, bool act, bool copy,
                                             float* o, double snext) {
#pragma unroll
  for (int i = kC - 1; i >= 0; --i) {
    const int k = k0 + i;
    if (!kEdge || k < m) {                    // (the same for every lane)
      const float yk = ch.y[i + 2];
      const int tk = __builtin_amdgcn_readlane(ch.tl, i + 2);
      double sk;
      if (kEdge && k == m - 1) {
        sk = ch.d[i];
        if (act)
          for (int t = tk + 1; t < T; ++t) (o + (int64_t)t * n)[cc] = yk;
      } else {
        sk = fma(-lane_value(ch.fc, i), snext, ch.d[i]);
        const int tn = __builtin_amdgcn_readlane(ch.tl, i + 3);
        if (tn - tk > 1) {
          const double h = (double)(tn - tk), ih = lane_value(ch.fih, i);
          const double dy = (double)ch.y[i + 3] - (double)yk;
          for (int t = tk + 1; t < tn; ++t) {
            const double u = (double)(t - tk) * ih, w = 1.0 - u;
            const double w1 = u * u * (3.0 - 2.0 * u), g0 = h * u * (w * w), g1 = h * (u * u) * w;
            const double v = fma(g0, sk, fma(-g1, snext, fma(w1, dy, (double)yk)));
            if (act) (o + (int64_t)t * n)[cc] = (float)v;
          }
        }
      }
      if (act && copy) (o + (int64_t)tk * n)[cc] = yk;
      if (kEdge && k == 0 && act)
        for (int t = 0; t < tk; ++t) (o + (int64_t)t * n)[cc] = yk;
      snext = sk;
    }
  }
  return snext;
}

// `ts` and `out` may be the same array: neither is __restrict__
__global__ __launch_bounds__(kThreads) void k_interp(const float* ts, int64_t S, int T, int n, Factors f,
                                                     const int32_t* __restrict__ cnt, double* slab, int64_t slab_stride,
                                                     float* out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wid = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * kWaves;
  double* sl = slab + wid * slab_stride + lane;                 // [chunk][64]: d' of the chunk's last knot
  const bool copy = out != ts;
  const int panels = (n + kCols - 1) / kCols;
  const int64_t items = S * panels;
  for (int64_t item = wid; item < items; item += waves) {
    const int64_t s = item / panels;
    const int col = (int)(item - s * panels) * kCols + lane;
    const bool act = col < n;                 // a lane past n walks column n - 1 along and stores nothing
    const int64_t base = s * T;
    const int cc = act ? col : n - 1;
    const float* x = ts + base * n;
    float* o = out + base * n;
    const int m = __builtin_amdgcn_readfirstlane(cnt[s]);
    if (m < 2) {                              // no kept frame: zeros; one: its value (bits) in every frame
      const float v = m == 1 ? (x + (int64_t)f.kn[base] * n)[cc] : 0.0f;
      if (act)
        for (int t = 0; t < T; ++t) (o + (int64_t)t * n)[cc] = v;
      continue;
    }
    const int chunks = (m + kC - 1) / kC;
    Chunk ch;
    double dprev = 0.0;
    for (int c = 0; c + 1 < chunks; ++c) {    // (the last chunk's d' is formed in the backward walk alone)
      const int k0 = c * kC;
      if (k0 > 0 && k0 + kC < m) {
        load_chunk<false>(ch, f, base, k0, m, x, n, cc, lane);
        dprev = solve_chunk<false>(ch, k0, m, dprev);
      } else {
        load_chunk<true>(ch, f, base, k0, m, x, n, cc, lane);
        dprev = solve_chunk<true>(ch, k0, m, dprev);
      }
      sl[(int64_t)c * kCols] = dprev;
    }
    double snext = 0.0;
    for (int c = chunks - 1; c >= 0; --c) {
      const int k0 = c * kC;
      const double din = c ? sl[(int64_t)(c - 1) * kCols] : 0.0;
      if (k0 > 0 && k0 + kC < m) {
        load_chunk<false>(ch, f, base, k0, m, x, n, cc, lane);
        solve_chunk<false>(ch, k0, m, din);
        snext = back_chunk<false>(ch, k0, m, T, n, cc, act, copy, o, snext);
      } else {
        load_chunk<true>(ch, f, base, k0, m, x, n, cc, lane);
        solve_chunk<true>(ch, k0, m, din);
        snext = back_chunk<true>(ch, k0, m, T, n, cc, act, copy, o, snext);
      }
    }
  }
}

int check(int64_t S, int32_t T, int32_t n) {
  if (cgnn_check_cohort(S, n) != CGNN_OK || T < 2 || T > CGNN_MAX_FRAMES) return CGNN_EINVAL;
  return S * (int64_t)T > kMaxKnots ? CGNN_EINVAL : CGNN_OK;
}

}  // namespace

extern "C" int64_t cgnn_ingest_interpolate_workspace_bytes(int64_t S, int32_t T, int32_t n) {
  if (check(S, T, n) != CGNN_OK) return CGNN_EINVAL;
  return layout(S, T).total;
}

extern "C" int cgnn_ingest_interpolate(const float* ts, int64_t S, int32_t T, int32_t n, const uint8_t* keep,
                                       int64_t keep_bytes, void* workspace, int64_t workspace_bytes, float* out,
                                       int64_t out_bytes, void* stream) {
  if (check(S, T, n) != CGNN_OK) return CGNN_EINVAL;
  if (keep_bytes < 0 || workspace_bytes < 0 || out_bytes < 0) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (!ts || !keep || !out || !workspace || cgnn_misaligned({ts, out}, 3) || cgnn_misaligned({workspace}, 15))
    return CGNN_EINVAL;
  const Layout w = layout(S, T);
  CGNN_NEED_BYTES(keep, keep_bytes, S * T);
  CGNN_NEED_BYTES(workspace, workspace_bytes, w.total);
  if (!cgnn_holds_floats(out_bytes, S * n, T)) return CGNN_EINVAL;      // out [S T][n]

  hipStream_t hs = cgnn_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const auto f64 = [&](int64_t off) { return reinterpret_cast<double*>(ws + off); };
  int32_t* kn = reinterpret_cast<int32_t*>(ws + w.kn);
  int32_t* cnt = reinterpret_cast<int32_t*>(ws + w.cnt);
  const int prep = cgnn_grid_for(S, kPrepPerCu);
  k_interp_knots<<<prep, kWave, 0, hs>>>(keep, S, T, kn, cnt);
  CGNN_CHECK_LAUNCH();
  k_interp_factors<<<prep, kWave, 0, hs>>>(kn, cnt, S, T, f64(w.a), f64(w.b), f64(w.l), f64(w.c), f64(w.ih));
  CGNN_CHECK_LAUNCH();
  const int64_t items = S * ((n + kCols - 1) / kCols);
  const int grid = cgnn_grid_for((items + kWaves - 1) / kWaves, kPerCu);
  const Factors f{kn, f64(w.a), f64(w.b), f64(w.l), f64(w.c), f64(w.ih)};
  k_interp<<<grid, kThreads, 0, hs>>>(ts, S, T, n, f, cnt, f64(w.slab), w.slab_stride, out);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
