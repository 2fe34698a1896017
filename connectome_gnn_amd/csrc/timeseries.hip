// timeseries.hip -- a device-resident cohort of ROI time series (float [S, T, n], one row per frame) turned into
// Pearson correlation matrices (float [U, n, n]), whole runs or sliding windows: cgnn_ingest_corr.
//
// A unit u = s * W + w is subject s, frames [w * stride, w * stride + L); W = 1 and L = T without a window.
// Per unit: m_i = the mean of column i, q_i = sum_t (x[t,i] - m_i)^2, both in fp64 as centred sums (blocked Welford);
// r[i,j] = sum_t z[t,i] z[t,j] with z[t,i] = (x[t,i] - m_i) / sqrt(q_i), centred and scaled in fp32 as the
// operands are staged; 1/sqrt(0) is taken as 0, so a constant column gives a zero row and column.
//
//   k_corr_stats   a workgroup of 4 waves per (unit, 64 columns), grid stride: lane = column (a wave reads 256
//                  consecutive bytes of a frame), wave = frame phase.  A thread centres 8 frames at a time in
//                  registers (their mean, then their centred squares, fp64) and merges the block into its
//                  running (count, mean, centred sum) by the pairwise update of Chan et al.; the four waves'
//                  moments merge the same way through LDS, in wave order.  One read of every frame, no
//                  E[x^2] - E[x]^2 anywhere; a constant column gives q = 0 exactly.  Writes stats[u, i] =
//                  (m_i, 1/sqrt(q_i)) as floats.
//   k_corr<vec>    a persistent grid walks the items (unit, tile pair bi <= bj) of 96 x 96 outputs.  Per item
//                  it steps through the frames 32 at a time: the two [32, 96] column panels are loaded into
//                  registers (the NEXT step's loads are issued before this step's MFMAs), centred, scaled and
//                  stored to LDS as they are -- frame-major, rows of 112 floats.  With v_mfma_f32_16x16x4_f32
//                  lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], and here A[i][k] =
//                  z[k][i]: BOTH fragments are "row k, 16 consecutive columns" of a frame-major panel, so the
//                  transposition costs nothing, and 112 = 48 (mod 64) puts the four rows of a fragment read on
//                  disjoint banks.  Each of the 4 waves owns 3 x 3 blocks of 16 x 16 (36 accumulators; in a
//                  diagonal tile the 21 blocks on or above the diagonal are spread 6 / 5 / 4 / 6); two LDS
//                  buffers, one barrier per step.  Native f32 MFMA: every product is an fp32 multiply-add.
//                  Epilogue: clamp to [-1, 1], |.| if asked, store r[i,j] and its mirror r[j,i] from the same
//                  register; in a diagonal tile only i <= j is stored (and mirrored), and r[i,i] is written as
//                  1 (0 for a constant column) -- so the matrix is bit-symmetric by construction.
//
// Accumulation is fp32 over the frames in ascending order, no atomics: the same bits on every run and for every
// grid.  Frames past L and columns past n are zeros in LDS and are never read from memory.  Element offsets
// into `ts` and `out` are 64-bit.
#include <math.h>

#include "common.h"

extern "C" int cgnn_fused_grid(void);

namespace {

constexpr int kTile = 96;                     // output tile: 96 x 96 (360 -> 4 tiles = 384, 84 -> 1 tile)
constexpr int kKS = 32;                       // frames per K-step
constexpr int kLd = 112;                      // LDS row stride in floats: 112 % 64 == 48
constexpr int kThreads = 256;                 // 4 waves, 2 x 2 over the tile, 48 x 48 outputs each
constexpr int kSlots = kKS * (kTile / 4) / kThreads;   // float4 slots of a panel per thread
constexpr int kStatCols = 64;                 // k_corr_stats: columns per workgroup
constexpr int kStatThreads = 256;
constexpr int kStatBlock = 8;                 // frames a thread centres in registers before it merges them
static_assert(kSlots * kThreads == kKS * (kTile / 4), "a panel is a whole number of slots per thread");
static_assert(kTile % 16 == 0 && (kTile / 16) % 2 == 0, "2 x 2 waves of whole 16 x 16 blocks");

typedef float f32x4 __attribute__((ext_vector_type(4)));

// (count, mean, centred sum of squares) of two disjoint sets of samples -> of their union (Chan et al.)
__device__ __forceinline__ void merge_moments(int& cnt, double& mean, double& m2, int cb, double mb, double m2b) {
  if (cb == 0) return;
  const int tot = cnt + cb;
  const double d = mb - mean, f = (double)cb / (double)tot;
  mean += d * f;
  m2 += m2b + d * d * ((double)cnt * f);
  cnt = tot;
}

__global__ __launch_bounds__(kStatThreads) void k_corr_stats(const float* __restrict__ ts, int64_t U, int T, int n,
                                                             int W, int L, int stride, float* __restrict__ stats) {
  __shared__ double part[2][kStatThreads / 64][kStatCols];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = (n + kStatCols - 1) / kStatCols;
  const int64_t items = U * chunks;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t u = item / chunks;
    const int col = (int)(item - u * chunks) * kStatCols + lane;
    const int64_t s = u / W;
    const int w = (int)(u - s * W);
    const bool act = col < n;
    const float* __restrict__ x = ts + (s * T + (int64_t)w * stride) * n + (act ? col : 0);
    // this wave's frames are wave, wave + 4, ...: blocks of kStatBlock of them are centred in registers
    // and merged into the running moments, so every frame is read once
    int cnt = 0;
    double mean = 0.0, m2 = 0.0;
    if (act) {
      float v[kStatBlock], nx[kStatBlock];
#pragma unroll
      for (int i = 0; i < kStatBlock; ++i) nx[i] = wave + 4 * i < L ? x[(int64_t)(wave + 4 * i) * n] : 0.0f;
      for (int t0 = wave; t0 < L; t0 += 4 * kStatBlock) {
#pragma unroll
        for (int i = 0; i < kStatBlock; ++i) {          // the next block's loads fly while this one is reduced
          const int t = t0 + 4 * (kStatBlock + i);
          v[i] = nx[i];
          nx[i] = t < L ? x[(int64_t)t * n] : 0.0f;
        }
        const int left = (L - t0 + 3) / 4;
        const int cb = left < kStatBlock ? left : kStatBlock;
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < kStatBlock; ++i) sum += (double)v[i];      // (the padding adds zeros)
        const double mb = sum / (double)cb;
        double m2b = 0.0;
#pragma unroll
        for (int i = 0; i < kStatBlock; ++i) {
          const double d = (double)v[i] - mb;
          if (i < cb) m2b += d * d;
        }
        merge_moments(cnt, mean, m2, cb, mb, m2b);
      }
    }
    part[0][wave][lane] = mean;
    part[1][wave][lane] = m2;
    __syncthreads();
    if (wave == 0 && act) {                    // the four waves' moments, in wave order
      for (int k = 1; k < kStatThreads / 64; ++k) {
        const int ck = k < L ? (L - k + 3) / 4 : 0;
        merge_moments(cnt, mean, m2, ck, part[0][k][lane], part[1][k][lane]);
      }
      float* __restrict__ o = stats + (u * n + col) * 2;
      o[0] = (float)mean;
      o[1] = m2 == 0.0 ? 0.0f : (float)(1.0 / sqrt(m2));   // (a NaN stays a NaN)
    }
    __syncthreads();
  }
}

struct alignas(16) CorrShared {
  float panel[2][2][kKS * kLd];               // [buffer][side: bi | bj][frame][column]
  float mean[2][kTile];
  float rstd[2][kTile];
};

// 4 consecutive columns of frame t from column `col` on; frames >= L and columns >= n read as 0
template <bool kVec>
__device__ __forceinline__ f32x4 load4(const float* __restrict__ x, int t, int L, int col, int n) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (t < L) {
    const float* __restrict__ p = x + (int64_t)t * n + col;
    if (kVec) {
      if (col < n) v = *reinterpret_cast<const f32x4*>(p);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col + e < n) v[e] = p[e];
    }
  }
  return v;
}

// Which of its 3 x 3 blocks a wave computes (bit 3 a + b).  Off the diagonal the 2 x 2 waves own 48 x 48 outputs
// each.  A diagonal tile needs only the 21 of its 36 blocks on or above the diagonal (the mirror store writes the
// rest): waves 0 and 3 take the upper blocks of the two diagonal quadrants (6 each), waves 1 and 2 share the
// upper-right quadrant 5 + 4 -- 6 blocks on the busiest SIMD instead of 9.
constexpr int kAll = 0x1FF, kUpper = 0x137, kFirst5 = 0x01F, kLast4 = 0x1E0;

// one K-step of a wave: kKS / 4 MFMA steps over the blocks of kMask (fragments nobody uses are not read)
template <int kMask>
__device__ __forceinline__ void mma_step(const float* __restrict__ pa, const float* __restrict__ pb,
                                         f32x4 (&acc)[3][3]) {
#pragma unroll
  for (int kk = 0; kk < kKS / 4; ++kk) {
    float fa[3], fb[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      fa[a] = (kMask >> (3 * a)) & 7 ? pa[kk * 4 * kLd + a * 16] : 0.0f;
      fb[a] = (kMask >> a) & 0x49 ? pb[kk * 4 * kLd + a * 16] : 0.0f;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        if ((kMask >> (3 * a + b)) & 1)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a], fb[b], acc[a][b], 0, 0, 0);
  }
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void k_corr(const float* __restrict__ ts, int64_t U, int T, int n, int W, int L,
                                                   int stride, int absolute, const float* __restrict__ stats,
                                                   float* __restrict__ out) {
  __shared__ CorrShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = (n + kTile - 1) / kTile;
  const int pairs = nt * (nt + 1) / 2;
  const int64_t items = U * pairs;
  const int nks = (L + kKS - 1) / kKS;
  // the pairs of one unit on workgroups that share an L2 (blockIdx % 8), where the grid allows it
  int64_t first = blockIdx.x;
  if (gridDim.x % 8 == 0) first = (int64_t)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  int srow[kSlots], scol[kSlots];
#pragma unroll
  for (int q = 0; q < kSlots; ++q) {
    const int e = tid + kThreads * q;
    srow[q] = e / (kTile / 4);
    scol[q] = 4 * (e % (kTile / 4));
  }
  const int frow = lane >> 4, fcol = lane & 15;

  for (int64_t item = first; item < items; item += gridDim.x) {
    const int64_t u = item / pairs;
    int rem = (int)(item - u * pairs), bi = 0;
    while (rem >= nt - bi) {
      rem -= nt - bi;
      ++bi;
    }
    const int bj = bi + rem;
    const bool diag = bi == bj;
    const int64_t s = u / W;
    const int w = (int)(u - s * W);
    const float* __restrict__ x = ts + (s * T + (int64_t)w * stride) * n;
    const int col0[2] = {bi * kTile, bj * kTile};
    // this wave's quadrant (wr, wc) of the tile and its blocks there (wave-uniform)
    const int wr = diag ? wave == 3 : wave >> 1, wc = diag ? wave != 0 : wave & 1;
    const int mask = !diag ? kAll : (wave == 0 || wave == 3) ? kUpper : wave == 1 ? kFirst5 : kLast4;

    __syncthreads();                          // the previous item's epilogue still reads sh.rstd
    if (tid < 2 * kTile) {
      const int side = tid / kTile, c = tid - side * kTile;
      const int col = col0[side] + c;
      float m = 0.f, r = 0.f;
      if (col < n) {
        const float* __restrict__ st = stats + (u * n + col) * 2;
        m = st[0];
        r = st[1];
      }
      sh.mean[side][c] = m;
      sh.rstd[side][c] = r;
    }
    f32x4 pre[2][kSlots];
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
      pre[0][q] = load4<kVec>(x, srow[q], L, col0[0] + scol[q], n);
      if (!diag) pre[1][q] = load4<kVec>(x, srow[q], L, col0[1] + scol[q], n);
    }
    __syncthreads();

    // registers -> LDS buffer `buf`, centred and scaled; frames of step `ks` past L become zeros
    auto stage = [&](int buf, int ks) {
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        if (side == 1 && diag) break;
#pragma unroll
        for (int q = 0; q < kSlots; ++q) {
          const f32x4 m = *reinterpret_cast<const f32x4*>(&sh.mean[side][scol[q]]);
          const f32x4 r = *reinterpret_cast<const f32x4*>(&sh.rstd[side][scol[q]]);
          f32x4 z = {0.f, 0.f, 0.f, 0.f};
          if (ks * kKS + srow[q] < L) z = (pre[side][q] - m) * r;
          *reinterpret_cast<f32x4*>(&sh.panel[buf][side][srow[q] * kLd + scol[q]]) = z;
        }
      }
    };
    stage(0, 0);
    __syncthreads();

    f32x4 acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    int cur = 0;
    for (int ks = 0; ks < nks; ++ks) {
      const bool more = ks + 1 < nks;
      if (more) {
#pragma unroll
        for (int q = 0; q < kSlots; ++q) {
          const int t = (ks + 1) * kKS + srow[q];
          pre[0][q] = load4<kVec>(x, t, L, col0[0] + scol[q], n);
          if (!diag) pre[1][q] = load4<kVec>(x, t, L, col0[1] + scol[q], n);
        }
      }
      const float* __restrict__ pa = &sh.panel[cur][0][frow * kLd + wr * 48 + fcol];
      const float* __restrict__ pb = &sh.panel[cur][diag ? 0 : 1][frow * kLd + wc * 48 + fcol];
      if (mask == kAll) mma_step<kAll>(pa, pb, acc);
      else if (mask == kUpper) mma_step<kUpper>(pa, pb, acc);
      else if (mask == kFirst5) mma_step<kFirst5>(pa, pb, acc);
      else mma_step<kLast4>(pa, pb, acc);
      if (more) stage(cur ^ 1, ks + 1);
      __syncthreads();
      cur ^= 1;
    }

    // D[i][j] of a 16 x 16 block: lane l, register r holds i = 4 (l >> 4) + r, j = l & 15
    float* __restrict__ o = out + u * (int64_t)n * n;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const int rb = wr * 3 + a, cb = wc * 3 + b;           // block row / column inside the tile
        if (!((mask >> (3 * a + b)) & 1)) continue;           // another wave's, or below the diagonal
        const bool tri = diag && rb == cb;
        const int li0 = rb * 16 + 4 * frow;
        const int gi0 = col0[0] + li0, gj = col0[1] + cb * 16 + fcol;
        f32x4 v = acc[a][b];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float c = v[r];
          c = c > 1.0f ? 1.0f : (c < -1.0f ? -1.0f : c);     // (a NaN stays a NaN)
          if (absolute) c = fabsf(c);
          if (tri && gi0 + r == gj) {
            const float rs = sh.rstd[0][li0 + r];
            c = rs == 0.0f ? 0.0f : (rs != rs ? rs : 1.0f);
          }
          v[r] = c;
        }
        if (gj >= n) continue;
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
      }
    }
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

int grid_for(int64_t items, int per_cu) {
  const int64_t cap = per_cu * (int64_t)cgnn_fused_grid();
  return (int)(items < cap ? items : cap);
}

}  // namespace

extern "C" int cgnn_ingest_corr(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride,
                                int32_t absolute, float* stats, int64_t stats_bytes, float* out, int64_t out_bytes,
                                void* stream) {
  constexpr int64_t kLimit = (int64_t)1 << 31;
  if (S < 0 || S >= kLimit || n <= 0 || T < 2) return CGNN_EINVAL;
  if (window != 0 && (window < 2 || window > T || stride < 1)) return CGNN_EINVAL;
  const int L = window ? window : T;
  const int st = window ? stride : T;
  const int64_t W = (T - L) / st + 1;
  const int64_t U = S * W;
  if ((int64_t)n * n >= kLimit || U * n >= kLimit) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (!ts || !stats || !out || (reinterpret_cast<uintptr_t>(ts) & 3)) return CGNN_EINVAL;
  if ((reinterpret_cast<uintptr_t>(stats) & 3) || (reinterpret_cast<uintptr_t>(out) & 3)) return CGNN_EINVAL;
  CGNN_NEED_BYTES(stats, stats_bytes, U * n * 2 * (int64_t)sizeof(float));
  CGNN_NEED_BYTES(out, out_bytes, U * n * (int64_t)n * (int64_t)sizeof(float));
  hipStream_t hs = cgnn_stream(stream);
  const int64_t chunks = (n + kStatCols - 1) / kStatCols;
  const int stat_grid = grid_for(U * chunks, CGNN_CORR_STATS_PER_CU);
  k_corr_stats<<<stat_grid, kStatThreads, 0, hs>>>(ts, U, T, n, (int)W, L, st, stats);
  CGNN_CHECK_LAUNCH();
  const int64_t nt = (n + kTile - 1) / kTile;
  const int grid = grid_for(U * (nt * (nt + 1) / 2), CGNN_CORR_WG_PER_CU);
  const bool vec = n % 4 == 0 && !(reinterpret_cast<uintptr_t>(ts) & 15) && !(reinterpret_cast<uintptr_t>(out) & 15);
  if (vec)
    k_corr<true><<<grid, kThreads, 0, hs>>>(ts, U, T, n, (int)W, L, st, absolute, stats, out);
  else
    k_corr<false><<<grid, kThreads, 0, hs>>>(ts, U, T, n, (int)W, L, st, absolute, stats, out);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
