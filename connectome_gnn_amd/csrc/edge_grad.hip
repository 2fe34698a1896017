// edge_grad.hip -- gradients of the loss w.r.t. the batch's edge weights (no atomics).
//
// Every aggregate of the layered path is Y = A_hat X' (+ b); the reference's autograd carries dY
// through models.py:94-114 (GCN) and :146-149 (SAGE) back to edge_weight.  Per edge e = (s -> d):
//
//   g_e = <dY[d,:], X'[s,:]>                                   the SDDMM over the dst-sorted CSR
//   GCN : dw_e = g_e dis_s dis_d - 1/2 dis_s^3 ddis_s,
//         ddis_i = sum_{e: src=i} g_e w_e dis_dst + sum_{e: dst=i} g_e w_e dis_src + 2 dis_i <dY[i], X'[i]>
//   SAGE: dw_e = (g_e - <dY[d], agg[d]>) / (wsum_d + 1e-8)
//
// SDDMM: one wave per destination row, the wave split into four 16-lane groups, one edge per group
// (eight to sixteen edges in flight per wave): a group reads a whole neighbour row (16 lanes x float4 per 64
// columns) and folds its partial dot products in four butterfly steps.  dY[r] stays in registers.
// Each output is one fixed-order reduction, so two runs are bit-identical.
#include "common.h"

namespace {

__device__ __forceinline__ float group16_sum(float v) {
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 1, 64);
  return v;
}

template <int V>
__device__ __forceinline__ float dot_v(const float4 (&a)[V], const float4 (&b)[V]) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    s = fmaf(a[j].x, b[j].x, s);
    s = fmaf(a[j].y, b[j].y, s);
    s = fmaf(a[j].z, b[j].z, s);
    s = fmaf(a[j].w, b[j].w, s);
  }
  return s;
}

template <int V>
__device__ __forceinline__ void load_v(float4 (&a)[V], const float* row, int l) {
#pragma unroll
  for (int j = 0; j < V; ++j) a[j] = *reinterpret_cast<const float4*>(row + 64 * j + 4 * l);
}

// the slot's value: g_e (GCN, or any caller without rowdiv) or the whole SAGE dw_e
__device__ __forceinline__ float value(float s, float self, const float* rowdiv, float dv) {
  return rowdiv ? (s - self) / dv : s;
}

// F == 64*V, rows 16-byte aligned.  Block = 4 waves = 4 rows; XCD-aware row order as k_agg_wave_row
// (aggregate.hip): XCD x walks the x-th eighth of the rows, so a graph's X' is pulled into one L2.  A row's
// slot metadata (col, eid) is loaded 64 slots at a time, one per lane, with dY[r] (no load waits on another
// inside the slot loop); each pass then has U edges per group in flight (U*4 neighbour rows per wave).
template <int V>
__global__ void __launch_bounds__(256) k_sddmm_wave_row(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ eid,
    const float* __restrict__ dY, int64_t lddy, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ Xs, int64_t ldxs, const float* __restrict__ rowdiv,
    float* __restrict__ g, float* __restrict__ gself, int64_t num_rows) {
  constexpr int U = V == 4 ? 2 : 4;
  const int lane = threadIdx.x & 63, q = lane >> 4, l = lane & 15;
  const int xcd = blockIdx.x & 7;
  const int64_t nrb = (num_rows + 3) / 4, per = (nrb + 7) / 8;
  for (int64_t i = blockIdx.x >> 3; i < per; i += gridDim.x >> 3) {
    const int64_t r = (xcd * per + i) * 4 + (threadIdx.x >> 6);
    if (r >= num_rows) continue;
    const int beg = cgnn_uniform(rowptr[r]);
    const int end = cgnn_uniform(rowptr[r + 1]);
    float4 dy[V];
    load_v<V>(dy, dY + r * lddy, l);
    float self = 0.f;
    if (Xs) {
      float4 xs[V];
      load_v<V>(xs, Xs + r * ldxs, l);
      self = group16_sum(dot_v<V>(dy, xs));
    }
    if (gself && lane == 0) gself[r] = self;
    const float dv = rowdiv ? rowdiv[r] : 1.f;
    for (int cb = beg; cb < end; cb += 64) {
      const int cnt = min(64, end - cb);
      int mycol = (int)r, myeid = cb + lane;           // lanes past the row: their own row, never written
      if (lane < cnt) {
        mycol = col[cb + lane];
        if (eid) myeid = eid[cb + lane];
      }
      for (int j = 0; j < cnt; j += 4 * U) {
        float4 a[U][V];
        int kk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          kk[u] = j + 4 * u + q;
          load_v<V>(a[u], X + (int64_t)__shfl(mycol, kk[u] & 63, 64) * ldx, l);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float sv = group16_sum(dot_v<V>(dy, a[u]));
          const int dst = __shfl(myeid, kk[u] & 63, 64);
          if (l == 0 && kk[u] < cnt) g[dst] = value(sv, self, rowdiv, dv);
        }
      }
    }
  }
}

// Any F (layer 0 runs at in_channels: 1, 5, 7, 12, ...): same layout, lane l of a group takes columns
// l, l+16, ...; dY[r] is re-read per edge (an L1 hit).
__global__ void __launch_bounds__(256) k_sddmm_any(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ eid,
    const float* __restrict__ dY, int64_t lddy, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ Xs, int64_t ldxs, const float* __restrict__ rowdiv,
    float* __restrict__ g, float* __restrict__ gself, int64_t num_rows, int F) {
  constexpr int U = 4;
  const int lane = threadIdx.x & 63, q = lane >> 4, l = lane & 15;
  const int xcd = blockIdx.x & 7;
  const int64_t nrb = (num_rows + 3) / 4, per = (nrb + 7) / 8;
  for (int64_t i = blockIdx.x >> 3; i < per; i += gridDim.x >> 3) {
    const int64_t r = (xcd * per + i) * 4 + (threadIdx.x >> 6);
    if (r >= num_rows) continue;
    const int beg = cgnn_uniform(rowptr[r]);
    const int end = cgnn_uniform(rowptr[r + 1]);
    const float* dyr = dY + r * lddy;
    float self = 0.f;
    if (Xs) {
      const float* xr = Xs + r * ldxs;
      for (int f = l; f < F; f += 16) self = fmaf(dyr[f], xr[f], self);
      self = group16_sum(self);
    }
    if (gself && lane == 0) gself[r] = self;
    const float dv = rowdiv ? rowdiv[r] : 1.f;
    for (int cb = beg; cb < end; cb += 64) {
      const int cnt = min(64, end - cb);
      int mycol = (int)r, myeid = cb + lane;
      if (lane < cnt) {
        mycol = col[cb + lane];
        if (eid) myeid = eid[cb + lane];
      }
      for (int j = 0; j < cnt; j += 4 * U) {
        const float* xp[U];
        float sv[U];
        int kk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          kk[u] = j + 4 * u + q;
          xp[u] = X + (int64_t)__shfl(mycol, kk[u] & 63, 64) * ldx;
          sv[u] = 0.f;
        }
        for (int f = l; f < F; f += 16) {
          const float d = dyr[f];
#pragma unroll
          for (int u = 0; u < U; ++u) sv[u] = fmaf(d, xp[u][f], sv[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float t = group16_sum(sv[u]);
          const int dst = __shfl(myeid, kk[u] & 63, 64);
          if (l == 0 && kk[u] < cnt) g[dst] = value(t, self, rowdiv, dv);
        }
      }
    }
  }
}

// ddis_i: 16 lanes per node walk its dst row and its src row (g and w in COO order), fixed-order fold
__global__ void __launch_bounds__(256) k_gcn_ddis(
    const int32_t* __restrict__ rowptr_dst, const int32_t* __restrict__ col_dst, const int32_t* __restrict__ eid_dst,
    const int32_t* __restrict__ rowptr_src, const int32_t* __restrict__ col_src, const int32_t* __restrict__ eid_src,
    const float* __restrict__ w, const float* __restrict__ dis, const float* __restrict__ g,
    const float* __restrict__ gself, int64_t nn, float* __restrict__ ddis) {
  const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int l = threadIdx.x & 15;
  float sum = 0.f;
  if (i < nn) {
    for (int s = rowptr_dst[i] + l, e = rowptr_dst[i + 1]; s < e; s += 16) {
      const int k = eid_dst[s];
      sum = fmaf(g[k] * w[k], dis[col_dst[s]], sum);
    }
    for (int s = rowptr_src[i] + l, e = rowptr_src[i + 1]; s < e; s += 16) {
      const int k = eid_src[s];
      sum = fmaf(g[k] * w[k], dis[col_src[s]], sum);
    }
  }
  sum = group16_sum(sum);
  if (i < nn && l == 0) ddis[i] = sum + 2.f * dis[i] * gself[i];
}

// dw_e = g_e dis_s dis_d - 1/2 dis_s^3 ddis_s, walked by destination rows (16 lanes per row)
__global__ void __launch_bounds__(256) k_gcn_dw(
    const int32_t* __restrict__ rowptr_dst, const int32_t* __restrict__ col_dst, const int32_t* __restrict__ eid_dst,
    const float* __restrict__ dis, const float* __restrict__ g, const float* __restrict__ ddis, int64_t nn,
    float* __restrict__ dw) {
  const int64_t d = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (d >= nn) return;
  const float dd = dis[d];
  for (int s = rowptr_dst[d] + (threadIdx.x & 15), e = rowptr_dst[d + 1]; s < e; s += 16) {
    const int k = eid_dst[s];
    const int c = col_dst[s];
    const float ds = dis[c];
    dw[k] = g[k] * ds * dd - 0.5f * ds * ds * ds * ddis[c];
  }
}

inline unsigned blocks16(int64_t n) { return (unsigned)((n + 15) / 16); }

}  // namespace

static bool sddmm_vec_ok(const float* p, int64_t ld) {
  return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % 4 == 0;
}

extern "C" {

int cgnn_sddmm_f32(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* dY, int64_t lddy,
                   const float* X, int64_t ldx, const float* Xself, int64_t ldxs, const float* rowdiv, float* g,
                   float* gself, int64_t num_rows, int32_t F, void* stream) {
  if (num_rows < 0 || F <= 0 || lddy < F || ldx < F) return CGNN_EINVAL;
  if (Xself && ldxs < F) return CGNN_EINVAL;
  if ((rowdiv || gself) && !Xself) return CGNN_EINVAL;
  if (num_rows == 0) return CGNN_OK;
  if (!rowptr || !dY || !X) return CGNN_EINVAL;             // col / g: read and written per slot only
  const int64_t per = ((num_rows + 3) / 4 + 7) / 8;          // 4-row blocks per XCD
  const unsigned grid = (unsigned)(8 * (per < 2048 ? per : 2048));
  hipStream_t st = cgnn_stream(stream);
  const bool vec = (F == 64 || F == 128 || F == 256) && sddmm_vec_ok(dY, lddy) && sddmm_vec_ok(X, ldx) &&
                   (!Xself || sddmm_vec_ok(Xself, ldxs));
  if (vec && F == 64)
    k_sddmm_wave_row<1><<<grid, 256, 0, st>>>(rowptr, col, eid, dY, lddy, X, ldx, Xself, ldxs, rowdiv, g, gself, num_rows);
  else if (vec && F == 128)
    k_sddmm_wave_row<2><<<grid, 256, 0, st>>>(rowptr, col, eid, dY, lddy, X, ldx, Xself, ldxs, rowdiv, g, gself, num_rows);
  else if (vec)
    k_sddmm_wave_row<4><<<grid, 256, 0, st>>>(rowptr, col, eid, dY, lddy, X, ldx, Xself, ldxs, rowdiv, g, gself, num_rows);
  else
    k_sddmm_any<<<grid, 256, 0, st>>>(rowptr, col, eid, dY, lddy, X, ldx, Xself, ldxs, rowdiv, g, gself, num_rows, F);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

int64_t cgnn_gcn_norm_bwd_workspace_bytes(int64_t num_nodes) {
  return num_nodes < 0 ? 0 : cgnn_align_up(num_nodes * (int64_t)sizeof(float), 16);
}

int cgnn_gcn_norm_bwd(const int32_t* rowptr_dst, const int32_t* col_dst, const int32_t* eid_dst,
                      const int32_t* rowptr_src, const int32_t* col_src, const int32_t* eid_src,
                      const float* edge_weight, const float* dis, const float* g, const float* gself,
                      int64_t num_nodes, int64_t num_edges, float* dw, void* workspace,
                      int64_t workspace_bytes, void* stream) {
  if (num_nodes < 0 || num_edges < 0) return CGNN_EINVAL;
  if (num_edges == 0) return CGNN_OK;                         // nothing to write: dw is empty
  if (num_nodes == 0) return CGNN_EINVAL;
  if (!rowptr_dst || !col_dst || !eid_dst || !rowptr_src || !col_src || !eid_src || !edge_weight || !dis ||
      !g || !gself || !dw || !workspace)
    return CGNN_EINVAL;
  CGNN_NEED_BYTES(workspace, workspace_bytes, cgnn_gcn_norm_bwd_workspace_bytes(num_nodes));
  hipStream_t st = cgnn_stream(stream);
  float* ddis = static_cast<float*>(workspace);
  k_gcn_ddis<<<blocks16(num_nodes), 256, 0, st>>>(rowptr_dst, col_dst, eid_dst, rowptr_src, col_src, eid_src,
                                                  edge_weight, dis, g, gself, num_nodes, ddis);
  CGNN_CHECK_LAUNCH();
  k_gcn_dw<<<blocks16(num_nodes), 256, 0, st>>>(rowptr_dst, col_dst, eid_dst, dis, g, ddis, num_nodes, dw);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

}  // extern "C"
