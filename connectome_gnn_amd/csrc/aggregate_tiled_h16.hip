// aggregate_tiled_h16.hip -- fp16-storage / fp32-accumulate tiled aggregation for large dense
// parcellations (BASELINE config 5: 1000-ROI graphs at 10 % density, hidden 256).
//
//   Y[r,:] = post(r) * sum_{e in row r} w_e * pre(c_e) * X[c_e,:]   (+ bias)        X, Y: __half
//
// Same reduction as aggregate_tiled.hip (models.py:112-114 / :146-149 and their transposes), with
// two changes that the config forces:
//   * storage is fp16: a [<=1024 rows x 64 columns] slice of a graph is 128 KB of LDS, so a whole
//     1000-ROI graph fits one tile; products and sums are fp32 (v_fma_mix), only the staged
//     operand and the result are rounded to half;
//   * rows have ~100 neighbours: a block's blocked-ELL entries (up to 128 steps) sit in registers
//     as 8 batches of 16 steps, each batch refilled with the wave's next block as soon as it has
//     been consumed, and are broadcast with DPP.
// The reference has no fp16 path (.half() raises in both models); parity is checked
// against the fp32 oracle at fp16 resolution.
#include <hip/hip_fp16.h>
#include "common.h"

namespace {

constexpr int H_MAXR = 1024;
constexpr int H_NW = 8;
constexpr int H_THR = H_NW * 64;
constexpr int H_PF = H_MAXR / 64;              // 16-byte pieces per thread in the staging pass
constexpr int H_MB = 8;                        // metadata batches (16 steps each) held in registers

#define H_BC(v, S) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), 0x150 + (S), 0xf, 0xf, true))

__device__ __forceinline__ void fma4h(float4& acc, uint32_t wbits, const char* tb, uint32_t off) {
  const uint2 raw = *reinterpret_cast<const uint2*>(tb + (off >> 1));   // 4 halves of the row
  const float w = __uint_as_float(wbits);
  const __half2 lo = *reinterpret_cast<const __half2*>(&raw.x);
  const __half2 hi = *reinterpret_cast<const __half2*>(&raw.y);
  acc.x = fmaf(w, __low2float(lo), acc.x); acc.y = fmaf(w, __high2float(lo), acc.y);
  acc.z = fmaf(w, __low2float(hi), acc.z); acc.w = fmaf(w, __high2float(hi), acc.w);
}

// one step: the 4 entries (offset, weight) of this lane group's 4 rows sit in lane S of the group
#define H_STEP(M0, M1, S)                                                                   \
  {                                                                                         \
    const uint32_t o0 = H_BC(M0.x, S), w0 = H_BC(M0.y, S), o1 = H_BC(M0.z, S),              \
                   w1 = H_BC(M0.w, S), o2 = H_BC(M1.x, S), w2 = H_BC(M1.y, S),              \
                   o3 = H_BC(M1.z, S), w3 = H_BC(M1.w, S);                                  \
    fma4h(acc[0], w0, tb, o0); fma4h(acc[1], w1, tb, o1);                                   \
    fma4h(acc[2], w2, tb, o2); fma4h(acc[3], w3, tb, o3);                                   \
  }
#define H_STEP4(M0, M1, S)                                                                  \
  H_STEP(M0, M1, S) H_STEP(M0, M1, (S) + 1) H_STEP(M0, M1, (S) + 2) H_STEP(M0, M1, (S) + 3) \
  __builtin_amdgcn_sched_barrier(0);

__device__ __forceinline__ uint2 pack4(const float4& v) {
  const __half2 lo = __floats2half2_rn(v.x, v.y), hi = __floats2half2_rn(v.z, v.w);
  uint2 r;
  r.x = *reinterpret_cast<const uint32_t*>(&lo);
  r.y = *reinterpret_cast<const uint32_t*>(&hi);
  return r;
}

__global__ void __launch_bounds__(H_THR) k_agg_tiled_h16(
    cgnn_tiles t, int flags, const __half* __restrict__ X, int64_t ldx, int nslices,
    const float* __restrict__ pre, const float* __restrict__ post, const float* __restrict__ bias,
    __half* __restrict__ Y, int64_t ldy) {
  __shared__ __attribute__((aligned(16))) __half tile[H_MAXR * 64];   // 128 KB
  __shared__ float postl[H_MAXR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, j = lane & 15;
  const bool transposed = flags & CGNN_AGG_TRANSPOSED, pre_div = flags & CGNN_AGG_PRE_DIV;
  const bool post_div = flags & CGNN_AGG_POST_DIV;
  const uint4* ent = static_cast<const uint4*>(transposed ? t.ent_src : t.ent_dst);
  const int32_t* blk_off = transposed ? t.blk_off_src : t.blk_off_dst;
  const int units = t.num_tiles * nslices;
  const char* tb = reinterpret_cast<const char*>(tile) + 8 * j;      // this lane's 4 columns

  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int tid = u / nslices, slice = u - tid * nslices;
    const int base = t.tile_ptr[tid];
    const int n = t.tile_ptr[tid + 1] - base;
    const int nblk = (n + 15) >> 4;
    const int gb0 = t.tile_blk[tid];

    // ---- stage the slice: 8 threads x 16 bytes per row, 64 rows per pass
    {
      const int piece = threadIdx.x & 7, r0 = threadIdx.x >> 3;
      uint4 buf[H_PF];
#pragma unroll
      for (int k = 0; k < H_PF; ++k) {
        const int row = r0 + 64 * k;
        buf[k] = make_uint4(0u, 0u, 0u, 0u);
        if (row < n)
          buf[k] = *reinterpret_cast<const uint4*>(X + (int64_t)(base + row) * ldx + 64 * slice + 8 * piece);
      }
#pragma unroll
      for (int k = 0; k < H_PF; ++k) {
        const int row = r0 + 64 * k;
        if (row < nblk * 16) {
          uint4 v = buf[k];
          if (pre && row < n) {
            const float s = pre_div ? 1.0f / pre[base + row] : pre[base + row];
            __half2* h = reinterpret_cast<__half2*>(&v);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float2 f = __half22float2(h[i]);
              h[i] = __floats2half2_rn(f.x * s, f.y * s);
            }
          }
          *reinterpret_cast<uint4*>(tile + row * 64 + 8 * piece) = v;
          if (piece == 0) postl[row] = (post && row < n) ? post[base + row] : 1.f;
        }
      }
    }
    __syncthreads();

    // ---- aggregate 16-row blocks out of LDS
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bias) b4 = *reinterpret_cast<const float4*>(bias + 64 * slice + 4 * j);
    // metadata of a whole block (up to 128 steps = 8 batches of 16) sits in registers; as soon
    // as a batch has been consumed its registers are refilled with the same batch of the wave's
    // NEXT block, so every load has a whole block's worth of work to land behind (an HBM round
    // trip per 16 steps would dominate otherwise)
    uint4 cur[H_MB][2];
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
    int off_c = 0, wid_c = 0;
    if (wave < nblk) {
      off_c = blk_off[gb0 + wave];
      wid_c = (blk_off[gb0 + wave + 1] - off_c) >> 4;
      const uint4* mp = ent + (off_c >> 1);
#pragma unroll
      for (int k = 0; k < H_MB; ++k) {
        cur[k][0] = cur[k][1] = z4;
        if (16 * k + j < wid_c) {
          cur[k][0] = mp[8 * (16 * k + j) + 2 * q];
          cur[k][1] = mp[8 * (16 * k + j) + 2 * q + 1];
        }
      }
    }
    for (int b = wave; b < nblk; b += H_NW) {
      int off_n = 0, wid_n = 0;
      if (b + H_NW < nblk) {
        off_n = blk_off[gb0 + b + H_NW];
        wid_n = (blk_off[gb0 + b + H_NW + 1] - off_n) >> 4;
      }
      const uint4* mpn = ent + (off_n >> 1);
      float4 acc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      // padding steps past the width are (row 0, weight 0): harmless, so no per-step branch
#pragma unroll
      for (int k = 0; k < H_MB; ++k) {
        if (16 * k < wid_c) {
          H_STEP4(cur[k][0], cur[k][1], 0) H_STEP4(cur[k][0], cur[k][1], 4)
          if (16 * k + 8 < wid_c) { H_STEP4(cur[k][0], cur[k][1], 8) H_STEP4(cur[k][0], cur[k][1], 12) }
        }
        cur[k][0] = cur[k][1] = z4;
        if (16 * k + j < wid_n) {
          cur[k][0] = mpn[8 * (16 * k + j) + 2 * q];
          cur[k][1] = mpn[8 * (16 * k + j) + 2 * q + 1];
        }
      }
      {                                             // steps >= 128 (very dense rows): from global
        const uint4* mp = ent + (off_c >> 1);
        for (int st = 16 * H_MB; st < wid_c; ++st) {
          const uint4 e0 = mp[8 * st + 2 * q], e1 = mp[8 * st + 2 * q + 1];
          fma4h(acc[0], e0.y, tb, e0.x); fma4h(acc[1], e0.w, tb, e0.z);
          fma4h(acc[2], e1.y, tb, e1.x); fma4h(acc[3], e1.w, tb, e1.z);
        }
      }
      off_c = off_n; wid_c = wid_n;
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = 16 * b + 4 * q + it;
        if (row < n) {
          const float p = postl[row];
          float4 v = acc[it];
          if (post_div) { v.x /= p; v.y /= p; v.z /= p; v.w /= p; }
          else { v.x *= p; v.y *= p; v.z *= p; v.w *= p; }
          v.x += b4.x; v.y += b4.y; v.z += b4.z; v.w += b4.w;
          *reinterpret_cast<uint2*>(Y + (int64_t)(base + row) * ldy + 64 * slice + 4 * j) = pack4(v);
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int cgnn_aggregate_tiled_f16(const cgnn_tiles* t, int32_t flags, const void* X,
                                        int64_t ldx, int32_t F, const float* pre,
                                        const float* post, const float* bias, void* Y,
                                        int64_t ldy, void* stream) {
  bool launch;
  const int rc = cgnn_check_agg_tiled(t, flags, F, {ldx, ldy},
                                      reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y) |
                                          reinterpret_cast<uintptr_t>(bias),
                                      X, Y, H_MAXR, 8, &launch);
  if (!launch) return rc;
  k_agg_tiled_h16<<<cgnn_fused_grid(), H_THR, 0, cgnn_stream(stream)>>>(
      *t, flags, static_cast<const __half*>(X), ldx, F / 64, pre, post, bias,
      static_cast<__half*>(Y), ldy);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
