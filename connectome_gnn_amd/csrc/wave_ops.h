// wave_ops.h -- what the ingest kernels share of wave-level plumbing (knn.hip, mst.hip, modules.hip, pagerank.hip, core.hip;
// DESIGN.md 4.3u): the fence between a wave's own LDS accesses, and sums over the 64 lanes by a DPP scan in registers.
// Device code only.
#pragma once
#include "common.h"

// Between a wave's LDS accesses that other lanes of the same wave depend on: the hardware completes them in order, and
// this keeps the compiler from reordering them.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// v + (v moved across lanes by the DPP control kCtrl, on the rows of kRows), in registers; a lane without a source, or
// in a row outside kRows, adds 0
template <int kCtrl, int kRows>
__device__ __forceinline__ int dpp_add(int v) {
  return v + __builtin_amdgcn_update_dpp(0, v, kCtrl, kRows, 0xf, false);
}
template <int kCtrl, int kRows>
__device__ __forceinline__ double dpp_add(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), kCtrl, kRows, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), kCtrl, kRows, 0xf, false);
  return v + __hiloint2double(hi, lo);
}

// The inclusive prefix sum of v over the 64 lanes, in registers (no LDS round trips): sums within rows of 16 lanes by
// row_shr 1, 2, 4, 8, then lane 15 of a row into the next row (row_bcast:15 on rows 1 and 3) and lane 31 into the upper
// half (row_bcast:31 on rows 2 and 3).  The order of the additions is fixed.  Needs every lane active.
template <typename T>
__device__ __forceinline__ T wave_scan(T v) {
  v = dpp_add<0x111, 0xf>(v);
  v = dpp_add<0x112, 0xf>(v);
  v = dpp_add<0x114, 0xf>(v);
  v = dpp_add<0x118, 0xf>(v);
  v = dpp_add<0x142, 0xa>(v);
  return dpp_add<0x143, 0xc>(v);
}

// The sum of v over the 64 lanes, on every lane: the scan's last lane, read back.
__device__ __forceinline__ int wave_total(int v) { return __builtin_amdgcn_readlane(wave_scan(v), 63); }
__device__ __forceinline__ double wave_total(double v) {
  v = wave_scan(v);
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63),
                          __builtin_amdgcn_readlane(__double2loint(v), 63));
}
