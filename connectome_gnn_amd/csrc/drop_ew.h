// drop_ew.h -- dropout, once for every kernel that draws, replays or advances it: the keys
// (make_drop), the device key word of graph replay (drop_resolve), the keyed counter hash of the keep
// bits (mix32, drop_bits: 4 bits per 4-column chunk, one byte per chunk in the masks) and the refresh of
// the device words between steps (rng_refresh).  One copy of each, because bit-equality is the contract:
// a fused consumer draws exactly the bits the stand-alone apply pass would, and cgnn_rng_advance, the
// one-launch finaliser and a producer's BatchNorm tail advance the words alike, so graph replay draws the
// masks an eager run would.  head.hip draws a stream of its own (its own keys, 16 bits per element) with
// the same mixer.  Held to this by tests/test_gpu_dropout.py (every draw site and advancer, bit for bit against
// the host model of tests/dropout_data.py) and tests/test_dropout_math.py (that model's statistics); DESIGN.md 4.2e.
#pragma once
#include "common.h"

namespace {

struct DropCfg {
  uint32_t thr16;     // keep iff 16-bit hash >= thr16  (thr16 = round(p * 65536))
  float scale;        // 1 / (1 - p)
  uint32_t key0, key1;
  const uint32_t* dev_key;   // optional device word XOR-ed into key1 (graph replay: a captured
                             // kernel advances it, so replays draw fresh masks)
};

__device__ __forceinline__ DropCfg drop_resolve(DropCfg d) {
  if (d.dev_key) d.key1 ^= d.dev_key[0];
  return d;
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}

// 4 keep-bits for chunk `chunk_index` (row * chunks per row + chunk); bit i <-> column 4*chunk + i.
// One keyed counter hash gives the first 32 random bits, a second round of the same mixer the other 32
// (chained, not a second counter: half the multiplies of two independent hashes).
__device__ __forceinline__ uint32_t drop_bits(const DropCfg& d, uint32_t chunk_index) {
  const uint32_t h0 = mix32((chunk_index ^ d.key0) + d.key1);
  const uint32_t h1 = mix32(h0 + 0x9E3779B9u);
  uint32_t b = 0;
  b |= ((h0 & 0xFFFFu) >= d.thr16) ? 1u : 0u;
  b |= ((h0 >> 16) >= d.thr16) ? 2u : 0u;
  b |= ((h1 & 0xFFFFu) >= d.thr16) ? 4u : 0u;
  b |= ((h1 >> 16) >= d.thr16) ? 8u : 0u;
  return b;
}

// device dropout word i of a graph-captured step, advanced to the next step's
__device__ __forceinline__ uint32_t rng_refresh(uint32_t word, uint32_t i) {
  return mix32(word + 0x9E3779B9u * (i + 1u));
}

// One element of BatchNorm's backward, dY = a * ((g*f - c1) - xhat*c2) with xhat = (y - mean) * invstd,
// in ONE fixed sequence of separately rounded operations: k_bn_act_apply<true> (elementwise.hip) and
// the aggregate that forms dY while staging (dense_aggregate_c16.hip) must produce the same bits, and
// neither `#pragma clang fp contract(off)` nor expression shape survives inlining into kernels that
// are otherwise compiled with contraction on -- so the operations are spelled as instructions.
__device__ __forceinline__ float ew_mul(float a, float b) {
  float r;
  asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float ew_sub(float a, float b) {
  float r;
  asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float bn_bwd_dy(float a, float g, float f, float c1, float y, float mean,
                                           float invstd, float c2) {
  const float xhat = ew_mul(ew_sub(y, mean), invstd);
  return ew_mul(a, ew_sub(ew_sub(ew_mul(g, f), c1), ew_mul(xhat, c2)));
}

// the reference's scale, 1/(1-p) (aten::native_dropout), not 1/(realised keep rate): with
// replayed keep bits the arithmetic then matches the oracle to rounding
inline float drop_scale(float p) { return p > 0.f ? (float)(1.0 / (1.0 - (double)p)) : 1.0f; }

// host: the set-up for dropout probability p, keys from `seed`; salt0/salt1 name the stream
inline DropCfg make_drop(float p, uint64_t seed, int* use_drop, uint32_t salt0 = 0x85EBCA6Bu,
                         uint32_t salt1 = 0xC2B2AE35u) {
  DropCfg d;
  *use_drop = (p > 0.f) ? 1 : 0;
  double thr = (double)p * 65536.0 + 0.5;
  if (thr > 65535.0) thr = 65535.0;
  d.thr16 = (uint32_t)thr;
  d.scale = drop_scale(p);
  d.key0 = (uint32_t)(seed & 0xFFFFFFFFu) * 0x9E3779B9u + salt0;
  d.key1 = (uint32_t)(seed >> 32) ^ salt1;
  d.dev_key = nullptr;
  return d;
}

}  // namespace
