// common.h -- shared device helpers for the gfx950 kernels (wave64, CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>
#include "../../include/cgnn.h"

#define CGNN_WAVE 64

#define CGNN_CHECK_LAUNCH()                                   \
  do {                                                        \
    if (hipGetLastError() != hipSuccess) return CGNN_ELAUNCH; \
  } while (0)

// ABI 2: every scratch / partial-sum buffer the library writes comes with its byte count; a call whose
// buffer is shorter than what the path it is about to take writes returns CGNN_EINVAL before any launch.
#define CGNN_NEED_BYTES(ptr, have, need)                                   \
  do {                                                                     \
    if ((ptr) && (int64_t)(have) < (int64_t)(need)) return CGNN_EINVAL;    \
  } while (0)

static inline hipStream_t cgnn_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Per-device lazily-initialised state (function attributes, CU counts) is indexed by the current
// device ordinal: one process may drive several GPUs.
#define CGNN_MAX_DEVICES 64
static inline int cgnn_device_ordinal() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= CGNN_MAX_DEVICES) return 0;
  return d;
}

static inline int64_t cgnn_align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// Whether the address of any of `ptrs` has a bit of `low_bits` set: 3 for floats, 15 for 16-byte accesses.  A null
// pointer is aligned; whether it may be null is the caller's check.
static inline bool cgnn_misaligned(std::initializer_list<const void*> ptrs, uintptr_t low_bits) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & low_bits) != 0;
}

// A persistent grid over `items` work items: at most per_cu workgroups per cgnn_fused_grid() (cgnn.h) unit.
static inline int cgnn_grid_for(int64_t items, int per_cu) {
  const int64_t cap = per_cu * (int64_t)cgnn_fused_grid();
  return (int)(items < cap ? items : cap);
}

// What every cohort entry point [S, n, n] requires before anything else: row and element indices of one subject
// and the row index S * n of the cohort fit an int32.  CGNN_OK or CGNN_EINVAL; S == 0 is valid (nothing to do).
static inline int cgnn_check_cohort(int64_t S, int32_t n) {
  constexpr int64_t kLimit = (int64_t)1 << 31;
  if (S < 0 || S >= kLimit || n <= 0) return CGNN_EINVAL;
  if ((int64_t)n * n >= kLimit || S * (int64_t)n >= kLimit) return CGNN_EINVAL;
  return CGNN_OK;
}

// What the tiled aggregations (aggregate_tiled.hip, aggregate_tiled_h16.hip) check before they launch, in the
// order their callers rely on: bad values (CGNN_EINVAL); then shapes the build does not cover (CGNN_EUNSUPPORTED:
// F not a multiple of 64, a row stride not a multiple of ld_mult elements, tiles of more than max_rows rows, a
// pointer that is not 16-byte aligned); then an empty batch (CGNN_OK with *launch = false); then the pointers a
// launch dereferences (CGNN_EINVAL).  lds: the row strides of the [*, F] arrays; ptr_bits: the OR of every
// pointer accessed 16 bytes at a time; X, Y: operand and result.
static inline int cgnn_check_agg_tiled(const cgnn_tiles* t, int32_t flags, int32_t F, std::initializer_list<int64_t> lds,
                                       uintptr_t ptr_bits, const void* X, const void* Y, int max_rows, int ld_mult,
                                       bool* launch) {
  *launch = false;
  if (!t || t->num_nodes < 0 || t->num_tiles < 0 || F <= 0) return CGNN_EINVAL;
  for (const int64_t ld : lds)
    if (ld < F) return CGNN_EINVAL;
  if (F % 64 || t->max_tile_rows > max_rows || (ptr_bits & 15)) return CGNN_EUNSUPPORTED;
  for (const int64_t ld : lds)
    if (ld % ld_mult) return CGNN_EUNSUPPORTED;
  if (t->num_nodes == 0 || t->num_tiles == 0) return CGNN_OK;
  const bool tr = flags & CGNN_AGG_TRANSPOSED;
  if (!X || !Y || !t->tile_ptr || !t->tile_blk || !(tr ? t->ent_src : t->ent_dst) ||
      !(tr ? t->blk_off_src : t->blk_off_dst))
    return CGNN_EINVAL;
  *launch = true;
  return CGNN_OK;
}

// Wave-uniform value made provably uniform for the compiler (-> SGPR, scalar loads).
__device__ __forceinline__ int cgnn_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ float cgnn_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double cgnn_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Block-wide fixed-order sum of v over 256 threads (4 waves); sh: 4 doubles of LDS.
__device__ __forceinline__ double block_sum256(double v, double* sh) {
  v = cgnn_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return t;
}

// Streamed data -- arrays a kernel reads or writes exactly once -- goes through non-temporal
// accesses: they do not allocate in the cache hierarchy the way default loads/stores do, and a
// streaming pass over 0.4 GB ran 24 % faster with them (k_pool_fwd 98 -> 74 us).  NOT for data
// that is re-read (tiles staged in LDS are fine: they are read from HBM once).
typedef float cgnn_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t cgnn_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t cgnn_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 ldnt4(const float* p) {
  const cgnn_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const cgnn_f32x4*>(p));
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void stnt4(float* p, const float4& v) {
  __builtin_nontemporal_store(cgnn_f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<cgnn_f32x4*>(p));
}
__device__ __forceinline__ float ldnt(const float* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ uint4 ldnt(const uint4* p) {
  const cgnn_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const cgnn_u32x4*>(p));
  return make_uint4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ uint2 ldnt(const uint2* p) {
  const cgnn_u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const cgnn_u32x2*>(p));
  return make_uint2(v[0], v[1]);
}
