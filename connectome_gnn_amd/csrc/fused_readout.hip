// fused_readout.hip -- the fused GCN path's readout for gfx950 (hidden = 64, fp32): mean-pool with the
// last layer's BatchNorm + ReLU + dropout fused in, and its backward.
//
// Reference arithmetic replaced: global_mean_pool after the last layer's BatchNorm1d / ReLU / dropout
// (models.py:57-59, 209-211) and autograd's backward of it.  See include/cgnn.h ("FUSED PER-TILE GCN
// PATH") for the contract.  No atomics: per-workgroup partial sums go to slabs reduced in a fixed order
// (fused_support.hip).
#include "common.h"
#include "agg_block.h"   // ld4 / st4
#include "bn_coef.h"
#include "drop_ew.h"
#include "fused_common.h"

namespace {

constexpr int PTHR = 256;   // 16 row-lanes x 16 chunks

__global__ void __launch_bounds__(PTHR) k_pool_fwd(const float* __restrict__ Y,
                                                   const float* __restrict__ bn, DropCfg drop_in,
                                                   int use_drop, uint8_t* __restrict__ mask_out,
                                                   const int32_t* __restrict__ gptr, int B,
                                                   float* __restrict__ P, float* __restrict__ F1,
                                                   float* __restrict__ F2) {
  // F1/F2 (training): per graph and column, sum over the graph's rows of the factor f =
  // relu'(z) * keep / (1-p) and of f * xhat.  The readout's gradient is constant per graph
  // (dP[g] / (n_g + 1e-8)), so the BatchNorm-backward sums of the last layer are
  // sum_g dP[g]/n_g * F1[g] and sum_g dP[g]/n_g * F2[g]: the backward never re-reads Y.
  const DropCfg drop = drop_resolve(drop_in);
  __shared__ float red[3 * 16 * HID];
  const int j = threadIdx.x & 15, rr = threadIdx.x >> 4;
  const float4 a = ld4(bn + 4 * j), b = ld4(bn + HID + 4 * j);
  const float4 mean = ld4(bn + 2 * HID + 4 * j), is = ld4(bn + 3 * HID + 4 * j);
  for (int g = blockIdx.x; g < B; g += gridDim.x) {
    const int rbeg = gptr[g], rend = gptr[g + 1];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), f1 = s, f2 = s;
#define CGNN_POOL_U 4
    constexpr int U = CGNN_POOL_U;             // rows in flight per thread (latency-bound otherwise)
    for (int row0 = rbeg + rr; row0 < rend; row0 += 16 * U) {
      float4 yb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = row0 + 16 * u;
        yb[u] = row < rend ? ldnt4(Y + (int64_t)row * HID + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = row0 + 16 * u;
        if (row < rend) {
          uint32_t keep = 0xFu;
          if (use_drop) {
            keep = drop_bits(drop, (uint32_t)row * 16u + (uint32_t)j);
            if (mask_out) mask_out[(int64_t)row * 16 + j] = (uint8_t)keep;
          }
          float4 f;
          const float4 y = yb[u];
          const float4 x = act4(y, a, b, keep, drop.scale, f);
          s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
          if (F1) {
            f1.x += f.x; f1.y += f.y; f1.z += f.z; f1.w += f.w;
            f2.x = fmaf(f.x, (y.x - mean.x) * is.x, f2.x); f2.y = fmaf(f.y, (y.y - mean.y) * is.y, f2.y);
            f2.z = fmaf(f.z, (y.z - mean.z) * is.z, f2.z); f2.w = fmaf(f.w, (y.w - mean.w) * is.w, f2.w);
          }
        }
      }
    }
    st4(red + rr * HID + 4 * j, s);
    if (F1) {
      st4(red + (16 + rr) * HID + 4 * j, f1);
      st4(red + (32 + rr) * HID + 4 * j, f2);
    }
    __syncthreads();
    if (threadIdx.x < HID) {
      float tot = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) tot += red[k * HID + threadIdx.x];
      P[(int64_t)g * HID + threadIdx.x] = tot / ((float)(rend - rbeg) + 1e-8f);
    } else if (F1 && threadIdx.x < 3 * HID) {
      const int which = threadIdx.x / HID, col = threadIdx.x % HID;          // 1: F1, 2: F2
      double tot = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) tot += (double)red[(16 * which + k) * HID + col];
      (which == 1 ? F1 : F2)[(int64_t)g * HID + col] = (float)tot;
    }
    __syncthreads();
  }
}

// BatchNorm-backward sums of the last layer from the per-graph factor sums of k_pool_fwd:
// slab[wg][0..63] = sum_g dP[g]/(n_g+1e-8) * F1[g], slab[wg][64..127] = ... * F2[g]  (fp64).
__global__ void __launch_bounds__(128) k_pool_bwd_sums(const float* __restrict__ dP,
                                                       const float* __restrict__ F1,
                                                       const float* __restrict__ F2,
                                                       const int32_t* __restrict__ gptr, int B,
                                                       double* __restrict__ s_slab) {
  const int col = threadIdx.x & 63;
  const float* F = threadIdx.x < 64 ? F1 : F2;
  double acc = 0.0;
  for (int g = blockIdx.x; g < B; g += gridDim.x) {
    const float inv = 1.0f / ((float)(gptr[g + 1] - gptr[g]) + 1e-8f);
    acc += (double)(dP[(int64_t)g * HID + col] * inv) * (double)F[(int64_t)g * HID + col];
  }
  s_slab[(int64_t)blockIdx.x * 128 + threadIdx.x] = acc;
}

// The same sums folded over ALL graphs by one block per channel, finalised on the spot (per-rank
// BatchNorm: no exchange between the sums and the coefficients) -- k_pool_bwd_sums +
// k_bn_bwd_stats in one launch.
__global__ void __launch_bounds__(256) k_pool_bwd_finalize(const float* __restrict__ dP,
                                                           const float* __restrict__ F1,
                                                           const float* __restrict__ F2,
                                                           const int32_t* __restrict__ gptr, int B,
                                                           double count, int zero_coef,
                                                           float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta,
                                                           float* __restrict__ bwc) {
  __shared__ double sh[4];
  const int c = blockIdx.x;
  double a1 = 0.0, a2 = 0.0;
  for (int g = threadIdx.x; g < B; g += 256) {
    const float inv = 1.0f / ((float)(gptr[g + 1] - gptr[g]) + 1e-8f);
    const double d = (double)(dP[(int64_t)g * HID + c] * inv);
    a1 += d * (double)F1[(int64_t)g * HID + c];
    a2 += d * (double)F2[(int64_t)g * HID + c];
  }
  const double S1 = block_sum256(a1, sh), S2 = block_sum256(a2, sh);
  if (threadIdx.x == 0) bn_bwd_coef(S1, S2, count, zero_coef, dgamma, dbeta, bwc, HID, c);
}

constexpr int PBTHR = 1024;  // readout backward: 64 row-lanes x 16 chunks (16 waves per CU)

__global__ void __launch_bounds__(PBTHR) k_pool_bwd(const float* __restrict__ dP,
                                                   const float* __restrict__ Y,
                                                   const float* __restrict__ bn, DropCfg drop,
                                                   int use_drop, const uint8_t* __restrict__ mask,
                                                   const int32_t* __restrict__ gptr, int B,
                                                   float* __restrict__ dZ,
                                                   double* __restrict__ s_slab) {
  __shared__ double red[(PBTHR / 16) * 128];
  const int j = threadIdx.x & 15, rr = threadIdx.x >> 4;
  const float4 a = ld4(bn + 4 * j), b = ld4(bn + HID + 4 * j);
  const float4 mean = ld4(bn + 2 * HID + 4 * j), is = ld4(bn + 3 * HID + 4 * j);
  double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  for (int g = blockIdx.x; g < B; g += gridDim.x) {
    const int rbeg = gptr[g], rend = gptr[g + 1];
    const float inv = 1.0f / ((float)(rend - rbeg) + 1e-8f);
    float4 gp = ld4(dP + (int64_t)g * HID + 4 * j);
    gp.x *= inv; gp.y *= inv; gp.z *= inv; gp.w *= inv;
    constexpr int U = 3;                       // rows in flight per thread
    constexpr int RS = PBTHR / 16;             // row stride
    for (int row0 = rbeg + rr; row0 < rend; row0 += RS * U) {
      float4 yb[U];
      uint32_t kb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = row0 + RS * u;
        yb[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        kb[u] = 0u;
        if (row < rend) {
          yb[u] = ld4(Y + (int64_t)row * HID + 4 * j);
          kb[u] = use_drop ? mask[(int64_t)row * 16 + j] : 0xFu;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = row0 + RS * u;
        if (row < rend) {
          const float4 y = yb[u];
          float4 f;
          act4(y, a, b, kb[u], drop.scale, f);
          const float4 dz = make_float4(gp.x * f.x, gp.y * f.y, gp.z * f.z, gp.w * f.w);
          if (dZ) st4(dZ + (int64_t)row * HID + 4 * j, dz);
          s1[0] += dz.x; s1[1] += dz.y; s1[2] += dz.z; s1[3] += dz.w;
          s2[0] += (double)dz.x * ((y.x - mean.x) * is.x); s2[1] += (double)dz.y * ((y.y - mean.y) * is.y);
          s2[2] += (double)dz.z * ((y.z - mean.z) * is.z); s2[3] += (double)dz.w * ((y.w - mean.w) * is.w);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    red[rr * 128 + 4 * j + i] = s1[i];
    red[rr * 128 + 64 + 4 * j + i] = s2[i];
  }
  __syncthreads();
  if (threadIdx.x < 128) {
    double tot = 0.0;
    for (int k = 0; k < PBTHR / 16; ++k) tot += red[k * 128 + threadIdx.x];
    s_slab[(int64_t)blockIdx.x * 128 + threadIdx.x] = tot;
  }
}

}  // namespace

extern "C" {

int cgnn_gcn_fused_pool_fwd(const float* Y, const float* bn, float p_drop, uint64_t seed,
                            const uint32_t* seed_dev, uint8_t* mask_out, const int32_t* gptr,
                            int32_t num_graphs, float* P, float* F1, float* F2, void* stream) {
  if (num_graphs < 0 || p_drop < 0.f || p_drop >= 1.f) return CGNN_EINVAL;
  if (num_graphs == 0) return CGNN_OK;
  if (!Y || !bn || !gptr || !P || (!F1) != (!F2)) return CGNN_EINVAL;
  int use_drop;
  DropCfg d = make_drop(p_drop, seed, &use_drop);
  d.dev_key = seed_dev;
  const int grid = num_graphs < 8 * cgnn_fused_grid() ? num_graphs : 8 * cgnn_fused_grid();
  k_pool_fwd<<<grid, PTHR, 0, cgnn_stream(stream)>>>(Y, bn, d, use_drop, mask_out, gptr, num_graphs, P,
                                                     F1, F2);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

int cgnn_gcn_fused_pool_bwd_sums(const float* dP, const float* F1, const float* F2,
                                 const int32_t* gptr, int32_t num_graphs, double* s_slab, int64_t s_slab_bytes,
                                 void* stream) {
  if (num_graphs < 0 || !dP || !F1 || !F2 || !gptr || !s_slab) return CGNN_EINVAL;
  CGNN_NEED_BYTES(s_slab, s_slab_bytes, fused_stat_slab_bytes());
  // exactly cgnn_fused_grid() workgroups so that the slab has the documented row count
  k_pool_bwd_sums<<<cgnn_fused_grid(), 128, 0, cgnn_stream(stream)>>>(dP, F1, F2, gptr, num_graphs, s_slab);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

int cgnn_gcn_fused_pool_bwd(const float* dP, const float* Y, const float* bn, float p_drop,
                            const uint8_t* mask, const int32_t* gptr, int32_t num_graphs,
                            float* dZ, double* s_slab, int64_t s_slab_bytes, void* stream) {
  if (num_graphs < 0 || p_drop < 0.f || p_drop >= 1.f) return CGNN_EINVAL;
  if (!dP || !Y || !bn || !gptr || !s_slab) return CGNN_EINVAL;   /* dZ may be NULL: sums only */
  if (p_drop > 0.f && !mask) return CGNN_EINVAL;
  CGNN_NEED_BYTES(s_slab, s_slab_bytes, fused_stat_slab_bytes());
  int use_drop;
  DropCfg d = make_drop(p_drop, 0, &use_drop);
  // exactly cgnn_fused_grid() workgroups so that the slab has the documented row count
  k_pool_bwd<<<cgnn_fused_grid(), PBTHR, 0, cgnn_stream(stream)>>>(dP, Y, bn, d, use_drop, mask, gptr,
                                                             num_graphs, dZ, s_slab);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

int cgnn_gcn_fused_pool_bwd_finalize(const float* dP, const float* F1, const float* F2,
                                     const int32_t* gptr, int32_t num_graphs, double count,
                                     int32_t zero_coef, float* dgamma, float* dbeta, float* bwc,
                                     void* stream) {
  if (num_graphs < 0 || count <= 0.0 || !dP || !F1 || !F2 || !gptr || !dgamma || !dbeta || !bwc)
    return CGNN_EINVAL;
  k_pool_bwd_finalize<<<HID, 256, 0, cgnn_stream(stream)>>>(dP, F1, F2, gptr, num_graphs, count, zero_coef,
                                                           dgamma, dbeta, bwc);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

}  // extern "C"
