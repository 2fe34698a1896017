// gram_tile.h -- THE tile walk of a symmetric product G = Z^T Z on the matrix pipe, defined once for k_corr
// (timeseries.hip: Z = the centred, scaled frames of a window), k_measure_tri (measures.hip: Z = the value map of
// a thresholded connectivity matrix) and k_partial (partial.hip: Z = the scaled inverse of a triangular factor, walked
// from the first row that is not known to be zero).  DESIGN.md 4.3c, 4.3d, 4.3h.
//
// Z is never materialised.  A caller names a row-major source (float rows of n columns, `rows` of them) and a stage
// functor that turns 4 loaded entries of row k into 4 entries of Z; it gets the 96 x 96 tile of G in registers.
//
//   items      A persistent grid walks the items (unit, tile pair bi <= bj), the pairs of a unit in row-major order
//              of the upper triangle; a workgroup starts at first_item() and strides by the grid.
//   panels     Per item the rows k go by 32 at a time.  The two [32, 96] column panels (tile bi | tile bj; one when
//              bi == bj) are loaded into registers (the NEXT step's loads are issued before this step's MFMAs),
//              staged through the functor and stored to LDS as they are: row-major in k ("frame-major"), rows of
//              112 floats.  Rows >= `rows` and columns >= n are never read from memory: the functor sees zeros.
//   fragments  With v_mfma_f32_16x16x4_f32 lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], and
//              here A[i][k] = Z[k][i]: BOTH fragments are "row k, 16 consecutive columns" of a frame-major panel, so
//              the transposition costs nothing, and 112 = 48 (mod 64) puts the four rows of a fragment read on
//              disjoint banks.  Native f32 MFMA: every product is an fp32 multiply-add, k ascending.
//   waves      Each of the 4 waves owns 3 x 3 blocks of 16 x 16 (36 accumulators): off the diagonal the 2 x 2 waves
//              own 48 x 48 outputs each.  A diagonal tile needs only the 21 of its 36 blocks on or above the
//              diagonal (its callers mirror): waves 0 and 3 take the upper blocks of the two diagonal quadrants (6
//              each), waves 1 and 2 share the upper-right quadrant 5 + 4 -- 6 blocks on the busiest SIMD, not 9.
//   buffers    Two LDS buffers, one barrier per K-step.  The caller owns the barrier(s) between load_panels() and
//              run(): what else it keeps in LDS decides where they go.
#pragma once
#include "common.h"

namespace gram {

constexpr int kTile = 96;                     // output tile: 96 x 96 (360 -> 4 tiles = 384, 84 -> 1 tile)
constexpr int kKS = 32;                       // rows k per K-step
constexpr int kLd = 112;                      // LDS row stride in floats: 112 % 64 == 48
constexpr int kThreads = 256;                 // 4 waves, 2 x 2 over the tile, 48 x 48 outputs each
constexpr int kSlots = kKS * (kTile / 4) / kThreads;   // float4 slots of a panel per thread
static_assert(kSlots * kThreads == kKS * (kTile / 4), "a panel is a whole number of slots per thread");
static_assert(kTile % 16 == 0 && (kTile / 16) % 2 == 0, "2 x 2 waves of whole 16 x 16 blocks");

typedef cgnn_f32x4 f32x4;
typedef float Panels[2][2][kKS * kLd];        // [buffer][side: bi | bj][row k][column]

// 4 consecutive columns of row `row` from column `col` on; rows >= `rows` and columns >= n read as 0
template <bool kVec>
__device__ __forceinline__ f32x4 load4(const float* __restrict__ base, int row, int rows, int col, int n) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (row < rows) {
    const float* __restrict__ p = base + (int64_t)row * n + col;
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

// Which of its 3 x 3 blocks a wave computes (bit 3 a + b): all of them off the diagonal, 6 / 5 / 4 / 6 in a
// diagonal tile (`waves` above).
constexpr int kAll = 0x1FF, kUpper = 0x137, kFirst5 = 0x01F, kLast4 = 0x1E0;

// quadrant row / column of wave w in a tile
__device__ __forceinline__ int quad_row(int w, bool diag) { return diag ? w == 3 : w >> 1; }
__device__ __forceinline__ int quad_col(int w, bool diag) { return diag ? w != 0 : w & 1; }

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

// What a thread keeps for the whole walk: its place in the workgroup, its fragment row / column (lane l reads row
// l >> 4, column l & 15 of a fragment) and the (row, column) of its float4 slots in a [kKS, kTile] panel.
struct Thread {
  int tid, wave, frow, fcol;
  int srow[kSlots], scol[kSlots];
  __device__ __forceinline__ Thread() {
    tid = threadIdx.x;
    wave = tid >> 6;
    frow = (tid & 63) >> 4;
    fcol = tid & 15;
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
      const int e = tid + kThreads * q;
      srow[q] = e / (kTile / 4);
      scol[q] = 4 * (e % (kTile / 4));
    }
  }
};

__host__ __device__ __forceinline__ int tiles_of(int n) { return (n + kTile - 1) / kTile; }
__host__ __device__ __forceinline__ int pairs_of(int nt) { return nt * (nt + 1) / 2; }

// the first item of this workgroup: the pairs of one unit on workgroups that share an L2 (blockIdx % 8), where the
// grid allows it
__device__ __forceinline__ int64_t first_item() {
  int64_t first = blockIdx.x;
  if (gridDim.x % 8 == 0) first = (int64_t)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  return first;
}

// One item: its unit and tile pair, and this wave's quadrant (wr, wc) of the tile with its blocks there
// (wave-uniform).  No arrays: a thread-dependent `side` must not turn the item into an indexed stack object.
struct Item {
  int64_t unit;
  int bi, bj, wr, wc, mask;
  bool diag;
  __device__ __forceinline__ Item(int64_t item, int nt, int wave) {
    const int pairs = pairs_of(nt);
    unit = item / pairs;
    int rem = (int)(item - unit * pairs);
    bi = 0;
    while (rem >= nt - bi) {
      rem -= nt - bi;
      ++bi;
    }
    bj = bi + rem;
    diag = bi == bj;
    wr = quad_row(wave, diag);
    wc = quad_col(wave, diag);
    mask = !diag ? kAll : (wave == 0 || wave == 3) ? kUpper : wave == 1 ? kFirst5 : kLast4;
  }
  // the first column of tile side `side` (0: bi, 1: bj)
  __device__ __forceinline__ int col0(int side) const { return (side ? bj : bi) * kTile; }
};

// issue the loads of the K-step that starts at row k0 into `pre`
template <bool kVec>
__device__ __forceinline__ void load_panels(f32x4 (&pre)[2][kSlots], const float* __restrict__ base, int rows, int n,
                                            int k0, const Item& it, const Thread& th) {
#pragma unroll
  for (int q = 0; q < kSlots; ++q) {
    pre[0][q] = load4<kVec>(base, k0 + th.srow[q], rows, it.col0(0) + th.scol[q], n);
    if (!it.diag) pre[1][q] = load4<kVec>(base, k0 + th.srow[q], rows, it.col0(1) + th.scol[q], n);
  }
}

// The K loop of one item over the rows k_begin .. rows - 1 (k_begin a multiple of kKS: a caller whose operand is
// known to be zero above it, such as the inverse of a triangular factor, skips those rows; 0 walks them all).
// `pre` holds the loads of the first step (load_panels at k0 = k_begin), and a barrier separates the
// previous item's last LDS reads from this call.  stage(side, k, c, v) maps the 4 loaded entries v of row k, columns
// c .. c + 3 of tile side `side` (c counted inside the tile), to what LDS holds for them.  On return acc is this
// wave's 3 x 3 blocks and every wave is past its last read of the panels.
template <bool kVec, class Stage>
__device__ __forceinline__ void run(Panels& panel, f32x4 (&pre)[2][kSlots], f32x4 (&acc)[3][3],
                                    const float* __restrict__ base, int rows, int n, const Item& it, const Thread& th,
                                    const Stage& stage, int k_begin = 0) {
  // registers -> LDS buffer `buf` for the step that starts at row k0
  auto store = [&](int buf, int k0) {
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      if (side == 1 && it.diag) break;
#pragma unroll
      for (int q = 0; q < kSlots; ++q)
        *reinterpret_cast<f32x4*>(&panel[buf][side][th.srow[q] * kLd + th.scol[q]]) =
            stage(side, k0 + th.srow[q], th.scol[q], pre[side][q]);
    }
  };
  store(0, k_begin);
  __syncthreads();

#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nks = (rows - k_begin + kKS - 1) / kKS;
  int cur = 0;
  for (int ks = 0; ks < nks; ++ks) {
    const bool more = ks + 1 < nks;
    if (more) load_panels<kVec>(pre, base, rows, n, k_begin + (ks + 1) * kKS, it, th);
    const float* __restrict__ pa = &panel[cur][0][th.frow * kLd + it.wr * 48 + th.fcol];
    const float* __restrict__ pb = &panel[cur][it.diag ? 0 : 1][th.frow * kLd + it.wc * 48 + th.fcol];
    if (it.mask == kAll) mma_step<kAll>(pa, pb, acc);
    else if (it.mask == kUpper) mma_step<kUpper>(pa, pb, acc);
    else if (it.mask == kFirst5) mma_step<kFirst5>(pa, pb, acc);
    else mma_step<kLast4>(pa, pb, acc);
    if (more) store(cur ^ 1, k_begin + (ks + 1) * kKS);
    __syncthreads();
    cur ^= 1;
  }
}

// Visit this wave's blocks: D[i][j] of a 16 x 16 block: lane l, register r holds i = 4 (l >> 4) + r, j = l & 15.
// f(a, b, tri, li0, gi0, gj): block acc[a][b]; tri = it lies on the diagonal of a diagonal tile (it holds its own
// mirror); register r is row li0 + r of tile bi = global row gi0 + r, at global column gj.
template <class F>
__device__ __forceinline__ void for_each_block(const Item& it, const Thread& th, const F& f) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (!((it.mask >> (3 * a + b)) & 1)) continue;          // another wave's, or below the diagonal
      const int rb = it.wr * 3 + a, cb = it.wc * 3 + b;       // block row / column inside the tile
      const int li0 = rb * 16 + 4 * th.frow;
      f(a, b, it.diag && rb == cb, li0, it.col0(0) + li0, it.col0(1) + cb * 16 + th.fcol);
    }
  }
}

}  // namespace gram
