// kendall.hip -- Kendall's tau-b of ranked ROI time series (include/cgnn_kendall.h).  Over the pairs
// k = (s < t) of kept frames of a unit, a_ik = sign(x_ti - x_si) in {-1, 0, 1} (the sign of the statement's, which
// A^T A does not see): G = A^T A holds concordant - discordant off the diagonal and the untied pairs on it, in exact
// int32, on the int8 matrix pipe.  Two kernels, no workspace, no atomics; integer sums, so no order changes a bit.
//
// k_kendall_counts   A persistent grid over gram_tile.h's items (unit, tile pair bi <= bj of 96 columns); the fp32 panel
//                    code of that header is not used, its item order and block ownership are.  Per item:
//   blocks     the frames go in blocks of kFb = 64 and the item walks the block pairs (a <= b).  Block a's keys are
//              staged frame-major (one s is read at a time, by adjacent columns), block b's column-major, 16 frames t of
//              a column being two 16-byte reads; a key is 16 bits, biased by -2^15 so that a saturating signed
//              subtraction orders every pair of keys.  A frame's kept flag is read from column 0 of the unit.
//   signs      a thread owns (column, chunk of 16 t) tasks and keeps their 16 keys and their kept mask in registers for
//              the whole block pair.  A step takes 2 frames s of block a (a censored s is skipped by a uniform branch):
//              per 4 signs two packed saturating subtractions, two packed minima with 1 and two byte permutes (the low
//              bytes, and 0xFF for a negative half), masked by the kept bytes of t (and, in a diagonal block pair, by
//              t > s); 16 sign bytes are stored once to the int8 panel [column][128 pairs] that all four waves share.
//   product    v_mfma_i32_16x16x64_i8: lane l reads "column l & 15, the 16 pairs of group l >> 4" for BOTH operands from
//              the same panel, so the order of the pairs inside an instruction cannot matter.  Block ownership and the
//              C/D layout (column l & 15, row 4 (l >> 4) + register) are gram_tile.h's.
//   epilogue   every entry and its mirror are stored from the same register; a NaN column gets its -1 and zeros here.
// k_kendall_tau      A workgroup per unit with a grid stride: the diagonal first (to LDS where n allows), then every
//                    off-diagonal entry read as int32 and written as fp32 at the same address by the same thread, in
//                    fp64 rounded once, and the diagonal last: which is what makes `out` in place of the counts safe.
#include "common.h"
#include "gram_tile.h"
#include "series_request.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = gram::kTile;
constexpr int kCols = 2 * kTile;              // columns of an item: tile bi | tile bj
constexpr int kFb = 64;                       // frames of a block
constexpr int kChunks = kFb / 16;             // chunks of 16 frames t
constexpr int kSStep = 2;                     // frames s of a step
constexpr int kPp = kSStep * kFb + 16;        // panel pitch in bytes: 16 columns x 16 bytes of a fragment read tile the banks
constexpr int kBp = kFb + 8;                  // pitch of block b's keys in halfwords, the same 144 bytes
constexpr int kTasks = kCols * kChunks / kThreads;   // (column, chunk) tasks of a thread
constexpr int kKeyBias = 32768;
constexpr int kTauDiag = 4096;                // diagonals up to this many columns are kept in LDS
// diagnostic A/B builds only (make variant DEFS=-DCGNN_KENDALL_LEAVE_OUT=..), never the product: 1 forms no signs (the
// panel is what it was), 2 issues no MFMAs.  Which of the two the kernel waits for is read off their timings.
#ifndef CGNN_KENDALL_LEAVE_OUT
#define CGNN_KENDALL_LEAVE_OUT 0
#endif
static_assert(kCols * kChunks % kThreads == 0 && kPp % 16 == 0 && (kBp * 2) % 16 == 0, "whole tasks, 16-byte rows");

typedef int v4i __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

struct Lds {
  short a[kFb][kCols];                        // block a, frame-major
  alignas(16) short b[kCols][kBp];            // block b, column-major
  alignas(16) unsigned char panel[kCols][kPp];
  alignas(16) unsigned char keptb[kFb];       // 0xFF: kept, 0x00: censored (or past L)
  unsigned char kepta[kFb];
  unsigned char nan[kCols];                   // a NaN in a kept frame of the column
};
static_assert(2 * sizeof(Lds) <= 160 * 1024, "two workgroups a CU");

// a kept frame's value in column 0: its key clamp(rint(2 v), 0, 65535) is not 0 (a NaN is kept)
__device__ __forceinline__ bool kept_of(float v0) { return !(rintf(2.0f * v0) <= 0.0f); }

__device__ __forceinline__ short key_of(float v) {
  const float t = fminf(fmaxf(rintf(2.0f * v), 0.0f), 65535.0f);      // a NaN reads as 0: its column is marked instead
  return (short)((int)t - kKeyBias);
}

// the kept flag of frame t of block blk: one thread per frame
__device__ __forceinline__ void flag_block(unsigned char* kept, const float* xu, int L, int n, int blk, int t) {
  const int f = blk * kFb + t;
  kept[t] = (f < L && kept_of(xu[(int64_t)f * n])) ? 0xFF : 0x00;
}

// block blk's keys of the item's columns into s.a (kA) or s.b; `kept` are that block's flags, already in LDS
template <bool kA>
__device__ __forceinline__ void stage_block(Lds& s, const unsigned char* kept, const float* xu, int L, int n, int blk,
                                            const gram::Item& it, int cols) {
  for (int e = threadIdx.x; e < kFb * kCols; e += kThreads) {
    const int f = e / kCols, c = e - f * kCols;
    if (c >= cols) continue;
    const int gc = c < kTile ? it.col0(0) + c : it.col0(1) + c - kTile;
    float v = 1.0f;
    if (kept[f] && gc < n) v = xu[(int64_t)(blk * kFb + f) * n + gc];  // a censored frame's value is never read
    if (v != v) s.nan[c] = 1;
    const short k = key_of(v);
    if (kA) s.a[f][c] = k;
    else s.b[c][f] = k;
  }
}

__device__ __forceinline__ uint32_t signs4(uint32_t lo, uint32_t hi, uint32_t s2) {
  const s16x2 one = {1, 1};
  const s16x2 sv = __builtin_bit_cast(s16x2, s2);
  // t - s, saturating, capped at 1: a half is 1, 0 or negative
  const s16x2 d0 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(__builtin_bit_cast(s16x2, lo), sv), one);
  const s16x2 d1 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(__builtin_bit_cast(s16x2, hi), sv), one);
  const uint32_t u0 = __builtin_bit_cast(uint32_t, d0), u1 = __builtin_bit_cast(uint32_t, d1);
  // the low bytes of the four halves (bytes 0, 2 of d0, then of d1), which are right for 1 and 0, under the bytes that
  // v_perm_b32's selectors 8 .. 11 make of the halves' sign bits: 0xFF, which is -1, for a negative half
  return __builtin_amdgcn_perm(u1, u0, 0x06040200u) | __builtin_amdgcn_perm(u1, u0, 0x0B0A0908u);
}

template <int kMask>
__device__ __forceinline__ void mma_half(const unsigned char* pa, const unsigned char* pb, v4i (&acc)[3][3]) {
  v4i fa[3], fb[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    fa[a] = (kMask >> (3 * a)) & 7 ? *reinterpret_cast<const v4i*>(pa + a * 16 * kPp) : v4i{0, 0, 0, 0};
    fb[a] = (kMask >> a) & 0x49 ? *reinterpret_cast<const v4i*>(pb + a * 16 * kPp) : v4i{0, 0, 0, 0};
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      if ((kMask >> (3 * a + b)) & 1)
        acc[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[a], fb[b], acc[a][b], 0, 0, 0);
}

// Every pair (s in block a, t in block b) of the staged blocks; kDiag: a == b, and only t > s counts.
template <bool kDiag>
__device__ __forceinline__ void block_pair(Lds& s, const gram::Item& it, const gram::Thread& th, int cols,
                                           v4i (&acc)[3][3]) {
  int tcol[kTasks], tchunk[kTasks];
  uint32_t kb[kTasks][8], km[kTasks][4];
#pragma unroll
  for (int q = 0; q < kTasks; ++q) {
    const int e = th.tid + kThreads * q;
    tchunk[q] = e / cols;                               // >= kChunks: no task (a diagonal tile has half the columns)
    tcol[q] = e - tchunk[q] * cols;
    if (tchunk[q] < kChunks) {
      const v4i* p = reinterpret_cast<const v4i*>(&s.b[tcol[q]][16 * tchunk[q]]);
      const v4i k0 = p[0], k1 = p[1];
      const v4i m = *reinterpret_cast<const v4i*>(&s.keptb[16 * tchunk[q]]);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        kb[q][d] = (uint32_t)k0[d];
        kb[q][4 + d] = (uint32_t)k1[d];
        km[q][d] = (uint32_t)m[d];
      }
    }
  }
  const unsigned char* pa = &s.panel[it.wr * 48 + th.fcol][16 * th.frow];
  const unsigned char* pb = &s.panel[(it.diag ? 0 : kTile) + it.wc * 48 + th.fcol][16 * th.frow];
  for (int s0 = 0; s0 < kFb; s0 += kSStep) {
    bool live[kSStep];
    bool any = false;
#pragma unroll
    for (int h = 0; h < kSStep; ++h) {
      const int sl = s0 + h;
      live[h] = cgnn_uniform(s.kepta[sl] != 0 && !(kDiag && sl == kFb - 1));
      any |= live[h];
    }
    if (!any) continue;                                 // uniform: the flags are the workgroup's
#pragma unroll
    for (int h = 0; h < kSStep; ++h) {
      if (!live[h] || CGNN_KENDALL_LEAVE_OUT == 1) continue;
      const int sl = s0 + h;
#pragma unroll
      for (int q = 0; q < kTasks; ++q) {
        if (tchunk[q] >= kChunks) continue;
        v4i w = {0, 0, 0, 0};
        const int t0 = 16 * tchunk[q];
        if (!kDiag || t0 + 15 > sl) {
          const uint32_t ks = (uint16_t)s.a[sl][tcol[q]];
          const uint32_t s2 = ks | (ks << 16);
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            uint32_t m = km[q][d];
            if (kDiag) {                                // the bytes of frames t <= s
              const int dead = sl + 1 - (t0 + 4 * d);
              m &= dead <= 0 ? 0xFFFFFFFFu : dead >= 4 ? 0u : 0xFFFFFFFFu << (8 * dead);
            }
            w[d] = (int)(signs4(kb[q][2 * d], kb[q][2 * d + 1], s2) & m);
          }
        }
        *reinterpret_cast<v4i*>(&s.panel[tcol[q]][kFb * h + t0]) = w;
      }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < kSStep; ++h) {
      if (!live[h] || CGNN_KENDALL_LEAVE_OUT == 2) continue;
      if (it.mask == gram::kAll) mma_half<gram::kAll>(pa + kFb * h, pb + kFb * h, acc);
      else if (it.mask == gram::kUpper) mma_half<gram::kUpper>(pa + kFb * h, pb + kFb * h, acc);
      else if (it.mask == gram::kFirst5) mma_half<gram::kFirst5>(pa + kFb * h, pb + kFb * h, acc);
      else mma_half<gram::kLast4>(pa + kFb * h, pb + kFb * h, acc);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void k_kendall_counts(const float* __restrict__ ranks, int64_t U, int L, int n,
                                                             int32_t* __restrict__ counts) {
  extern __shared__ __align__(16) unsigned char smem[];
  Lds& s = *reinterpret_cast<Lds*>(smem);
  const gram::Thread th;
  const int nt = gram::tiles_of(n);
  const int64_t items = U * gram::pairs_of(nt);
  const int nb = (L + kFb - 1) / kFb;
  for (int64_t item = gram::first_item(); item < items; item += gridDim.x) {
    const gram::Item it(item, nt, th.wave);
    const int cols = it.diag ? kTile : kCols;
    const float* __restrict__ xu = ranks + it.unit * L * n;
    v4i acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[a][b] = v4i{0, 0, 0, 0};
    if (th.tid < kCols) s.nan[th.tid] = 0;
    for (int a = 0; a < nb; ++a) {
      for (int b = a; b < nb; ++b) {
        __syncthreads();                                // the last pair's reads of the keys and the flags
        if (b == a && th.tid < kFb) flag_block(s.kepta, xu, L, n, a, th.tid);
        if (th.tid >= kFb && th.tid < 2 * kFb) flag_block(s.keptb, xu, L, n, b, th.tid - kFb);
        __syncthreads();
        if (b == a) stage_block<true>(s, s.kepta, xu, L, n, a, it, cols);
        stage_block<false>(s, s.keptb, xu, L, n, b, it, cols);
        __syncthreads();
        if (b == a) block_pair<true>(s, it, th, cols, acc);
        else block_pair<false>(s, it, th, cols, acc);
      }
    }
    int32_t* __restrict__ g = counts + it.unit * n * n;
    const int cbase = it.diag ? 0 : kTile;
    gram::for_each_block(it, th, [&](int a, int b, bool, int li0, int gi0, int gj) {
      const int lj = gj - it.col0(1);
      if (gj >= n) return;
      const bool nanc = s.nan[cbase + lj] != 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = gi0 + r;
        if (gi >= n) continue;
        int32_t v = acc[a][b][r];
        if (nanc || s.nan[li0 + r]) v = gi == gj ? -1 : 0;
        g[(int64_t)gi * n + gj] = v;
        g[(int64_t)gj * n + gi] = v;
      }
    });
    __syncthreads();                                    // the next item clears the NaN flags
  }
}

// g and out may be the same memory: every access is an int32 one, an entry is read and written by one thread, and
// the diagonal, which every entry reads, is written last.
__global__ __launch_bounds__(kThreads) void k_kendall_tau(const int32_t* g, int64_t U, int n, int absolute, float* out) {
  __shared__ int32_t diag[kTauDiag];
  const bool in_lds = n <= kTauDiag;
  const int nn = n * n;
  for (int64_t u = blockIdx.x; u < U; u += gridDim.x) {
    const int32_t* gu = g + u * nn;
    int32_t* ou = reinterpret_cast<int32_t*>(out) + u * nn;
    if (in_lds)
      for (int i = threadIdx.x; i < n; i += kThreads) diag[i] = gu[(int64_t)i * (n + 1)];
    __syncthreads();
    for (int e = threadIdx.x; e < nn; e += kThreads) {
      const int i = e / n, j = e - i * n;
      if (i == j) continue;
      const int32_t di = in_lds ? diag[i] : gu[(int64_t)i * (n + 1)];
      const int32_t dj = in_lds ? diag[j] : gu[(int64_t)j * (n + 1)];
      float t;
      if (di < 0 || dj < 0) t = __builtin_nanf("");
      else if (di == 0 || dj == 0) t = 0.0f;
      else {
        const double v = (double)gu[e] / sqrt((double)di * (double)dj);
        t = (float)(absolute ? fabs(v) : v);
      }
      ou[e] = __float_as_int(t);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kThreads) {
      const int32_t di = in_lds ? diag[i] : gu[(int64_t)i * (n + 1)];
      ou[(int64_t)i * (n + 1)] = __float_as_int(di < 0 ? __builtin_nanf("") : di == 0 ? 0.0f : 1.0f);
    }
    __syncthreads();                                    // the next unit's diagonal goes where this one is read
  }
}

}  // namespace

extern "C" int cgnn_ingest_kendall(const float* ranks, int64_t U, int32_t L, int32_t n, int32_t absolute,
                                   int32_t* counts, int64_t counts_bytes, float* out, int64_t out_bytes, void* stream) {
  if (cgnn_check_cohort(U, n) != CGNN_OK || L < 2 || L > CGNN_KENDALL_MAX_FRAMES) return CGNN_EINVAL;
  if (counts_bytes < 0 || out_bytes < 0) return CGNN_EINVAL;
  if (U == 0) return CGNN_OK;
  if (!ranks || (!counts && !out) || cgnn_misaligned({ranks, counts, out}, 3)) return CGNN_EINVAL;
  if (counts && !cgnn_holds_floats(counts_bytes, U * n, n)) return CGNN_EINVAL;    // (int32: the size of a float)
  if (out && !cgnn_holds_floats(out_bytes, U * n, n)) return CGNN_EINVAL;
  hipStream_t hs = cgnn_stream(stream);
  static bool attr[CGNN_MAX_DEVICES] = {};
  bool& done = attr[cgnn_device_ordinal()];
  if (!done) {                                          // dynamic LDS above 64 KB has to be allowed per kernel
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_kendall_counts), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)sizeof(Lds)) != hipSuccess)
      return CGNN_ELAUNCH;
    done = true;
  }
  int32_t* g = counts ? counts : reinterpret_cast<int32_t*>(out);
  const int64_t items = U * gram::pairs_of(gram::tiles_of(n));
  k_kendall_counts<<<cgnn_grid_for(items, 2), kThreads, sizeof(Lds), hs>>>(ranks, U, L, n, g);
  CGNN_CHECK_LAUNCH();
  if (out) {
    k_kendall_tau<<<cgnn_grid_for(U, 8), kThreads, 0, hs>>>(g, U, n, absolute, out);
    CGNN_CHECK_LAUNCH();
  }
  return CGNN_OK;
}
