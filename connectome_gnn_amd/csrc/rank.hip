// rank.hip -- the mid-ranks of ROI time series (include/cgnn_rank.h): what stands in front of
// cgnn_ingest_corr for a Spearman correlation.  One launch, no workspace, no atomics, nothing that depends on the data
// but the values themselves: every loop bound below is a function of L, n and the launch shape.
//
// A persistent workgroup of 4 waves takes items (unit, 4 adjacent columns) with a grid stride.
//   stage   all 256 threads read the item's L row segments of 16 bytes and store, per column, the 64-bit pairs
//           (order-preserving key << 32 | frame) in LDS, padded to P = 2^ceil(log2 L) with the pad key; a censored
//           frame gets the pad key too and its value is never looked at.  The whole column is in LDS before anything
//           is written, which is what makes `out == ts` safe.
//   sort    wave w sorts column w: a bitonic network whose strides are taken up to four at a time, 16 pairs in
//           registers between one LDS read and one LDS write (24 passes at P = 4096 instead of 78).  The pairs are
//           distinct (the frame breaks ties), so the order is a total one.
//   runs    a forward max-scan gives every sorted position the start of its run of equal keys, a backward min-scan
//           its end; 2 rank = start + end + 2 is kept beside the frame, and a third walk scatters it to the frame's
//           slot, all in the column's own LDS.
//   store   all 256 threads write the item's row segments, as they were read.
#include "common.h"
#include "frame_mask.h"
#include "series_request.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / CGNN_WAVE;
constexpr int kCols = kWaves;                 // columns of an item: a wave sorts one
constexpr int kSkew = 8;                      // pairs between the columns' arrays: their banks differ while staging
constexpr uint32_t kPadKey = 0xFFFFFFFFu;     // above every key of a number: +inf is 0xFF800000
constexpr uint32_t kNanKey = 0xFFC00000u;     // a NaN's key: its column is all NaN, only the pad key must differ
constexpr uint32_t kNoRun = 0xFFFFFFFEu;      // a run start that no position has
constexpr int kMaxLds = 160 * 1024;

// the pairs of a column live at a[slot(i)]: 16 consecutive pairs are permuted by the low bits of their block's index,
// so that lanes which hold 16 consecutive pairs each do not meet in one bank
__device__ __forceinline__ int slot(int i) { return i ^ ((i >> 4) & 15); }

__device__ __forceinline__ void wave_sync() {
  // the wave's LDS writes before its later reads, and its reads before its later writes
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// unsigned order of the keys == IEEE order of the floats; -0.0 and +0.0 share a key, subnormals keep theirs
__device__ __forceinline__ uint32_t key_of(uint32_t bits, bool& nan) {
  nan = (bits & 0x7FFFFFFFu) > 0x7F800000u;
  if ((bits << 1) == 0) bits = 0;
  const uint32_t key = bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
  return nan ? kNanKey : key;
}

// kS consecutive strides of the merge of size k, the smallest of them 1 << jlog: lane g's group is the 2^kS pairs
// whose indices differ in bits jlog .. jlog + kS - 1
template <int kS>
__device__ __forceinline__ void strides(uint64_t* a, int P, int k, int jlog, int lane) {
  constexpr int R = 1 << kS;
  const int groups = P >> kS;
  for (int g = lane; g < groups; g += CGNN_WAVE) {
    const int base = ((g >> jlog) << (jlog + kS)) | (g & ((1 << jlog) - 1));
    const bool asc = (base & k) == 0;
    uint64_t v[R];
#pragma unroll
    for (int e = 0; e < R; ++e) v[e] = a[slot(base + (e << jlog))];
#pragma unroll
    for (int st = R >> 1; st >= 1; st >>= 1) {
#pragma unroll
      for (int e = 0; e < R; ++e) {
        if (e & st) continue;
        const uint64_t lo = v[e], hi = v[e | st];
        const bool sw = (lo > hi) == asc;
        v[e] = sw ? hi : lo;
        v[e | st] = sw ? lo : hi;
      }
    }
#pragma unroll
    for (int e = 0; e < R; ++e) a[slot(base + (e << jlog))] = v[e];
  }
  wave_sync();
}

// ascending bitonic sort of the P = 1 << logp pairs of a, by one wave
__device__ __forceinline__ void sort_pairs(uint64_t* a, int logp, int lane) {
  const int P = 1 << logp;
  for (int m = 1; m <= logp; ++m) {
    const int k = 1 << m;
    for (int rem = m; rem > 0;) {
      const int s = rem < 4 ? rem : 4;
      rem -= s;
      if (s == 4) strides<4>(a, P, k, rem, lane);
      else if (s == 3) strides<3>(a, P, k, rem, lane);
      else if (s == 2) strides<2>(a, P, k, rem, lane);
      else strides<1>(a, P, k, rem, lane);
    }
  }
}

// The sorted pairs (key << 32 | frame) of a become, at the slot of frame f < L, the float bits of the rank of frame f
// in the high word: 0.0 for a censored frame.  The first L sorted positions hold every frame of the unit: the kept
// ones, then the censored ones by frame (their key is the pad's, and the padding's frames are L and above).
__device__ __forceinline__ void rank_runs(uint64_t* a, int L, bool nan, int lane) {
  uint32_t* w = reinterpret_cast<uint32_t*>(a);         // word 2 i: low half of pair i, word 2 i + 1: high half
  const int last = (L - 1) / CGNN_WAVE * CGNN_WAVE;
  // forward: high word <- the first position of the run of equal keys (the pad key stays what it is)
  uint32_t ckey = 0, cstart = 0;
  for (int c0 = 0; c0 <= last; c0 += CGNN_WAVE) {
    const int p = c0 + lane;
    const bool in = p < L;
    const uint32_t key = in ? w[2 * slot(p) + 1] : kPadKey;
    uint32_t prev = __shfl_up(key, 1, CGNN_WAVE);
    if (lane == 0) prev = ckey;
    uint32_t s = (p == 0 || key != prev) ? (uint32_t)p : 0u;
#pragma unroll
    for (int o = 1; o < CGNN_WAVE; o <<= 1) {
      const uint32_t t = __shfl_up(s, o, CGNN_WAVE);
      if (lane >= o && t > s) s = t;
    }
    if (cstart > s) s = cstart;
    ckey = __shfl(key, CGNN_WAVE - 1, CGNN_WAVE);
    cstart = __shfl(s, CGNN_WAVE - 1, CGNN_WAVE);
    if (in && key != kPadKey) w[2 * slot(p) + 1] = s;
  }
  wave_sync();
  // backward: low word <- frame | (start + end + 2) << 16, twice the rank (at most 2 L <= 8192); 0 for a censored frame
  uint32_t cnext = kNoRun, cend = 0;
  for (int c0 = last; c0 >= 0; c0 -= CGNN_WAVE) {
    const int p = c0 + lane;
    const bool in = p < L;
    const uint32_t s = in ? w[2 * slot(p) + 1] : kNoRun;
    uint32_t next = __shfl_down(s, 1, CGNN_WAVE);
    if (lane == CGNN_WAVE - 1) next = cnext;
    uint32_t e = s != next ? (uint32_t)p : 0x7FFFFFFFu;
#pragma unroll
    for (int o = 1; o < CGNN_WAVE; o <<= 1) {
      const uint32_t t = __shfl_down(e, o, CGNN_WAVE);
      if (lane + o < CGNN_WAVE && t < e) e = t;
    }
    if (e == 0x7FFFFFFFu) e = cend;                     // the run goes on in the chunk above, whose first run ends there
    cnext = __shfl(s, 0, CGNN_WAVE);
    cend = __shfl(e, 0, CGNN_WAVE);
    if (in) {
      const uint32_t twice = s == kPadKey ? 0u : s + e + 2u;
      w[2 * slot(p)] = (w[2 * slot(p)] & 0xFFFFu) | (twice << 16);
    }
  }
  wave_sync();
  // scatter: the high word of frame f's slot <- the rank of frame f (the run starts there are spent)
  for (int c0 = 0; c0 <= last; c0 += CGNN_WAVE) {
    const int p = c0 + lane;
    if (p < L) {
      const uint32_t v = w[2 * slot(p)];
      const int f = (int)(v & 0xFFFFu);
      const uint32_t twice = v >> 16;
      const float r = (twice != 0u && nan) ? __builtin_nanf("") : 0.5f * (float)twice;
      if (f < L) w[2 * slot(f) + 1] = __float_as_uint(r);
    }
  }
}

template <bool kMask>
__global__ __launch_bounds__(kThreads) void k_rank(const float* __restrict__ ts, const uint8_t* __restrict__ keep,
                                                   int64_t U, int T, int n, int W, int L, int stride, int logp,
                                                   float* out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int P = 1 << logp;
  const int pitch = P + kSkew;
  uint64_t* pairs = reinterpret_cast<uint64_t*>(smem);                              // [kCols][pitch]
  int* nans = reinterpret_cast<int*>(pairs + (size_t)kCols * pitch);                // [kWaves][kCols]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = threadIdx.x & (kCols - 1), f0 = threadIdx.x / kCols;               // staging: 4 threads per frame
  constexpr int kFrames = kThreads / kCols;
  const int chunks = (n + kCols - 1) / kCols;
  const int64_t items = U * chunks;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t u = item / chunks;
    const int col0 = (int)(item - u * chunks) * kCols;
    const int64_t first = cgnn_first_frame(u, W, T, stride);
    const cgnn_frame_mask<kMask> mask(keep, first, L);
    const bool act = col0 + c < n;
    const float* __restrict__ x = ts + first * n + (act ? col0 + c : 0);
    uint64_t* mycol = pairs + (size_t)c * pitch;
    bool seen = false;
#pragma unroll 4
    for (int f = f0; f < P; f += kFrames) {
      uint32_t key = kPadKey;
      if (f < L) {
        const uint32_t bits = __float_as_uint(x[(int64_t)f * n]);
        bool nan;
        const uint32_t k = key_of(bits, nan);
        if (!kMask || !mask.censored(f)) {              // by selection: a censored frame's value decides nothing
          key = k;
          seen |= nan;
        }
      }
      mycol[slot(f)] = ((uint64_t)key << 32) | (uint32_t)f;
    }
    // a NaN among the kept frames of column c, as this wave saw it: lanes c, c + 4, ...
    const unsigned long long saw = __ballot(seen && act);
    if (lane < kCols) nans[wave * kCols + lane] = (saw & (0x1111111111111111ull << lane)) != 0;
    __syncthreads();

    bool nan = false;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) nan |= nans[v * kCols + wave] != 0;
    uint64_t* a = pairs + (size_t)wave * pitch;
    sort_pairs(a, logp, lane);
    rank_runs(a, L, nan, lane);
    __syncthreads();

    if (act) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(mycol);
      float* __restrict__ o = out + u * L * n + col0 + c;
#pragma unroll 4
      for (int f = f0; f < L; f += kFrames) o[(int64_t)f * n] = __uint_as_float(w[2 * slot(f) + 1]);
    }
    __syncthreads();                                    // the next item's pairs go where these are read
  }
}

size_t lds_of(int logp) { return (size_t)kCols * ((1 << logp) + kSkew) * sizeof(uint64_t) + kWaves * kCols * sizeof(int); }

template <bool kMask>
int launch(const float* ts, const uint8_t* keep, const cgnn_units& un, int32_t T, int32_t n, float* out,
           hipStream_t hs) {
  static bool attr[CGNN_MAX_DEVICES] = {};
  bool& done = attr[cgnn_device_ordinal()];
  if (!done) {                                          // dynamic LDS above 64 KB has to be allowed per kernel
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_rank<kMask>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_of(12)) != hipSuccess)
      return CGNN_ELAUNCH;
    done = true;
  }
  int logp = 1;
  while ((1 << logp) < un.L) ++logp;
  const size_t lds = lds_of(logp);
  const int fit = (int)(kMaxLds / lds);                 // workgroups whose columns a CU's LDS holds: 1 at L > 2048
  const int per_cu = fit < 4 ? fit : 4;                 // and whose waves its registers hold (125 VGPRs: 4 per SIMD)
  const int64_t items = un.U * ((n + kCols - 1) / kCols);
  k_rank<kMask><<<cgnn_grid_for(items, per_cu), kThreads, lds, hs>>>(ts, keep, un.U, T, n, (int)un.W, un.L, un.st, logp,
                                                                     out);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

// what both entry points check and do; masked: keep [S, T] selects the frames
int rank_call(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride, const uint8_t* keep,
              int64_t keep_bytes, bool masked, float* out, int64_t out_bytes, void* stream) {
  cgnn_units un;
  if (cgnn_check_cohort(S, n) != CGNN_OK || cgnn_check_units(S, T, n, window, stride, &un) != CGNN_OK) return CGNN_EINVAL;
  if (un.L > CGNN_RANK_MAX_FRAMES || keep_bytes < 0 || out_bytes < 0) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (!ts || !out || cgnn_misaligned({ts, out}, 3) || (masked && !keep)) return CGNN_EINVAL;
  CGNN_NEED_BYTES(keep, keep_bytes, S * (int64_t)T);
  if (!cgnn_holds_floats(out_bytes, un.U * n, un.L)) return CGNN_EINVAL;           // out [U L][n]
  static_assert(kCols * (CGNN_RANK_MAX_FRAMES + kSkew) * 8 + 64 <= kMaxLds, "a unit's pairs must fit LDS");
  return masked ? launch<true>(ts, keep, un, T, n, out, cgnn_stream(stream))
                : launch<false>(ts, nullptr, un, T, n, out, cgnn_stream(stream));
}

}  // namespace

extern "C" int cgnn_ingest_rank(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride,
                                float* out, int64_t out_bytes, void* stream) {
  return rank_call(ts, S, T, n, window, stride, nullptr, 0, false, out, out_bytes, stream);
}

extern "C" int cgnn_ingest_rank_masked(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride,
                                       const uint8_t* keep, int64_t keep_bytes, float* out, int64_t out_bytes,
                                       void* stream) {
  return rank_call(ts, S, T, n, window, stride, keep, keep_bytes, true, out, out_bytes, stream);
}
