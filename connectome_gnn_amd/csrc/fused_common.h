// fused_common.h -- what more than one file of the fused GCN path (fused_gcn.hip, fused_readout.hip,
// fused_support.hip) needs: the hidden width, the activation whose bits the forward, the readout and both
// backwards must agree on, and the size of a statistics slab.
#pragma once
#include "common.h"

namespace {

constexpr int HID = CGNN_FUSED_HIDDEN;      // 64

// x = drop(relu(a*y + b)); returns x, and the combined (z>0 & keep) factor per component in f.
__device__ __forceinline__ float4 act4(const float4& y, const float4& a, const float4& b,
                                        uint32_t keep, float scale, float4& f) {
  float4 z, x;
  z.x = fmaf(a.x, y.x, b.x); z.y = fmaf(a.y, y.y, b.y);
  z.z = fmaf(a.z, y.z, b.z); z.w = fmaf(a.w, y.w, b.w);
  f.x = (z.x > 0.f && (keep & 1u)) ? scale : 0.f;
  f.y = (z.y > 0.f && (keep & 2u)) ? scale : 0.f;
  f.z = (z.z > 0.f && (keep & 4u)) ? scale : 0.f;
  f.w = (z.w > 0.f && (keep & 8u)) ? scale : 0.f;
  x.x = z.x * f.x; x.y = z.y * f.y; x.z = z.z * f.z; x.w = z.w * f.w;
  return x;
}

// bytes of a statistics slab: one row of 2 x 64 fp64 column sums per workgroup of the persistent grid
inline int64_t fused_stat_slab_bytes() { return (int64_t)cgnn_fused_grid() * 128 * (int64_t)sizeof(double); }

}  // namespace
