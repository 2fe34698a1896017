// frame_mask.h -- the device side of a frame mask keep [S, T]: which frames of a unit count, for
// k_filter_mean and k_filter (filter.hip), k_corr_stats and k_corr (timeseries.hip), k_lw (shrinkage.hip) and
// k_confound_basis (confounds.hip); and the stream over the columns that the two statistics kernels share.
//
// A censored frame's values are loaded beside its flag (no load waits for another) and then left out by selection,
// never by multiplication: what it holds is never looked at.
#pragma once
#include "common.h"

// The frames [first, first + frames) of keep are a unit's; t below is relative to `first`.  Without a mask every frame
// of the unit counts: the type holds no pointer then, loads nothing and takes no ballot.
template <bool kMask>
struct cgnn_frame_mask;

template <>
struct cgnn_frame_mask<false> {
  int L;
  __device__ cgnn_frame_mask(const uint8_t*, int64_t, int frames) : L(frames) {}
  // frame t is inside the unit (and, under a mask, kept)
  __device__ bool kept(int t) const { return t < L; }
  // frame t, which the caller knows to be inside the unit, is left out
  __device__ bool censored(int) const { return false; }
  // under a mask: bit i, i < count <= 32, is kept(tb + step * i).  Without one no bits are formed: the frames of a
  // block that count are its first ones, which the callers find by arithmetic
  __device__ unsigned block(int, int, int, int) const { return 0u; }
};

template <>
struct cgnn_frame_mask<true> {
  const uint8_t* __restrict__ kp;
  int L;
  __device__ cgnn_frame_mask(const uint8_t* keep, int64_t first, int frames) : kp(keep + first), L(frames) {}
  __device__ bool kept(int t) const { return t < L && kp[t] != 0; }
  __device__ bool censored(int t) const { return kp[t] == 0; }
  // one load, lane i's of frame tb + step * i, and a ballot: every lane of the wave must be here
  __device__ unsigned block(int tb, int step, int count, int lane) const {
    return (unsigned)__ballot(lane < count && kept(tb + step * lane));
  }
};

// The first frame of unit u = s * W + w, frames [w * stride, w * stride + L) of subject s, as a row of ts [S T][n] and
// an index into keep [S T].
__device__ __forceinline__ int64_t cgnn_first_frame(int64_t u, int W, int T, int stride) {
  const int64_t s = u / W;
  const int w = (int)(u - s * W);
  return s * T + (int64_t)w * stride;
}

constexpr int kStreamCols = 64;               // columns of an item: a wave reads 256 consecutive bytes of a frame
constexpr int kStreamThreads = 256;
constexpr int kStreamWaves = kStreamThreads / 64;
constexpr int kStreamBlock = 8;               // frames of a block; a thread has the next block's loads in flight

// The stream of k_filter_mean and k_corr_stats over ts [S, T, n]: a workgroup of 4 waves per item (unit, 64 columns),
// grid stride; lane = column, wave = frame phase (wave w takes frames w, w + 4, ... of the unit, ascending), so every
// frame is read once.  Per item an Acc{} is made, block(acc, v, bits, frames) is called for each block of 8 of this
// wave's frames -- the next block's loads and flags are issued first -- and then finish(acc, u, col, act, lane, wave),
// which merges the waves and ends with every wave past its last read of what they share: the next item follows at once.
//   v[i]     frame t0 + 4 i of the column, 0 past the unit
//   bits     kMask: bit i says that v[i] is a kept frame of the unit (every lane takes part in the ballot, so the
//            lanes past n walk column 0 along under act == false and write nothing); 0 without a mask
//   frames   how many of the v[i] lie inside the unit, censored or not: the first `frames` of them
template <bool kMask, class Acc, class Block, class Finish>
__device__ __forceinline__ void cgnn_stream_columns(const float* __restrict__ ts, const uint8_t* __restrict__ keep,
                                                    int64_t U, int T, int n, int W, int L, int stride, Block block,
                                                    Finish finish) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = (n + kStreamCols - 1) / kStreamCols;
  const int64_t items = U * chunks;
  constexpr int kStep = kStreamWaves, kB = kStreamBlock;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t u = item / chunks;
    const int col = (int)(item - u * chunks) * kStreamCols + lane;
    const int64_t first = cgnn_first_frame(u, W, T, stride);
    const bool act = col < n;
    const float* __restrict__ x = ts + first * n + (act ? col : 0);
    const cgnn_frame_mask<kMask> mask(keep, first, L);
    Acc acc{};
    if (act || kMask) {
      float v[kB], nx[kB];
#pragma unroll
      for (int i = 0; i < kB; ++i) nx[i] = wave + kStep * i < L ? x[(int64_t)(wave + kStep * i) * n] : 0.0f;
      unsigned vk = 0, nk = mask.block(wave, kStep, kB, lane);
      for (int t0 = wave; t0 < L; t0 += kStep * kB) {
        vk = nk;
        nk = mask.block(t0 + kStep * kB, kStep, kB, lane);
#pragma unroll
        for (int i = 0; i < kB; ++i) {        // the next block's loads fly while this one is reduced
          const int t = t0 + kStep * (kB + i);
          v[i] = nx[i];
          nx[i] = t < L ? x[(int64_t)t * n] : 0.0f;
        }
        const int left = (L - t0 + kStep - 1) / kStep;
        block(acc, v, vk, left < kB ? left : kB);
      }
    }
    finish(acc, u, col, act, lane, wave);
  }
}
