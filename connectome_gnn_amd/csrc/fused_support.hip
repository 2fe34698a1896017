// fused_support.hip -- what every fused path calls around its tile kernels (gfx950): the workgroup count
// of the persistent grids (cgnn_fused_grid), the fixed-order reductions of the per-workgroup slabs, the
// 64-wide BatchNorm finalisers and the refresh of the device dropout words.
//
// Reference arithmetic replaced: the batch statistics and affine coefficients of BatchNorm1d and of its
// backward (models.py:203-211), and the sums over nodes that autograd forms for the weight and bias
// gradients of GCNLayer (models.py:84-114) -- here sums over per-workgroup partials, in a fixed order.
#include "common.h"
#include "bn_coef.h"
#include "drop_ew.h"
#include "fused_common.h"

namespace {

template <typename T>
__global__ void __launch_bounds__(256) k_slab_reduce(const T* __restrict__ slab, int rows,
                                                     int width, double* __restrict__ out_d,
                                                     float* __restrict__ out_f, int out_cols,
                                                     int take_cols, int ld_out,
                                                     float* __restrict__ out_tail = nullptr, int split = 0) {
  // one block per 4 output elements: 64 threads (one wave) per element, fixed-order tree
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  if (e < width)
    for (int r = lane; r < rows; r += 64) s += (double)slab[(int64_t)r * width + e];
  s = cgnn_wave_sum(s);
  if (e < width && lane == 0) {
    if (out_d) out_d[e] = s;
    if (out_tail && e >= split) {
      out_tail[e - split] = (float)s;
    } else if (out_f) {
      const int rr = e / out_cols, cc = e % out_cols;
      if (cc < take_cols) out_f[(int64_t)rr * ld_out + cc] = (float)s;
    }
  }
}

// several f64 slab -> f32 vector reductions in one launch (blockIdx.y = job): the bias gradients of
// all layers of a backward pass.  (The loop is k_slab_reduce<double>'s, written out: as a shared function it
// changes the instructions of k_slab_reduce)
__global__ void __launch_bounds__(256) k_slab_reduce_multi(cgnn_reduce_jobs jobs) {
  const int jb = blockIdx.y;
  const int width = jobs.width[jb], rows = jobs.rows[jb];
  const double* __restrict__ slab = jobs.slab[jb];
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (e >= width) return;                                  // (wave-uniform)
  double s = 0.0;
  for (int r = lane; r < rows; r += 64) s += slab[(int64_t)r * width + e];
  s = cgnn_wave_sum(s);
  if (lane == 0) jobs.out[jb][e] = (float)s;
}

__global__ void k_bn_finalize(const double* __restrict__ sums, double count,
                              const double* __restrict__ count_dev,
                              const float* __restrict__ gamma, const float* __restrict__ beta,
                              float* __restrict__ rmean, float* __restrict__ rvar, float momentum,
                              float eps, int training, float* __restrict__ bn_out,
                              const float* __restrict__ mean_offset) {
  const int c = threadIdx.x;
  if (c >= HID) return;
  if (count_dev) count = count_dev[0];
  // mean_offset (nullable): the statistics are those of y - mean_offset[c] (the factored layer 0 is
  // handed on without its constant term); the module's running mean is that of y.  sums: NULL in eval
  const double S1 = training ? sums[c] : 0.0, S2 = training ? sums[HID + c] : 0.0;
  bn_fwd_coef(training, S1, S2, count, gamma, beta, rmean, rvar, momentum, eps,
              mean_offset ? mean_offset[c] : 0.f, bn_out, HID, c);
}

__global__ void k_bn_bwd_finalize(const double* __restrict__ sums, double count,
                                  const double* __restrict__ count_dev, int zero_coef,
                                  float* __restrict__ dgamma, float* __restrict__ dbeta,
                                  float* __restrict__ bwc) {
  const int c = threadIdx.x;
  if (c >= HID) return;
  if (count_dev) count = count_dev[0];
  bn_bwd_coef(sums[c], sums[HID + c], count, zero_coef, dgamma, dbeta, bwc, HID, c);
}

// ---- merged "reduce the per-workgroup partials + finalise" kernels (single-GPU fast path) ----

// one block per channel c: S1 = sum_r slab[r][c], S2 = sum_r slab[r][64+c], then finalise
// (thread i adds rows i, i + 256, ...; block_sum256 folds the 256 partials in a fixed order)
__device__ __forceinline__ void slab_pair_sum256(const double* __restrict__ slab, int rows, int c, double* sh,
                                                 double& S1, double& S2) {
  double a1 = 0.0, a2 = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) {
    a1 += slab[(int64_t)r * 128 + c];
    a2 += slab[(int64_t)r * 128 + HID + c];
  }
  S1 = block_sum256(a1, sh);
  S2 = block_sum256(a2, sh);
}

__global__ void __launch_bounds__(256) k_bn_fwd_stats(
    const double* __restrict__ slab, int rows, double count, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar,
    float momentum, float eps, long long* __restrict__ tracked, float* __restrict__ bn_out,
    uint32_t* __restrict__ rng_state, int rng_n, const float* __restrict__ mean_offset) {
  __shared__ double sh[4];
  const int c = blockIdx.x;
  // graph replay: refresh the device dropout words here -- this launch runs after every consumer of
  // the previous step's words and before the first of this one
  if (rng_state && c == 0 && (int)threadIdx.x < rng_n)
    rng_state[threadIdx.x] = rng_refresh(rng_state[threadIdx.x], threadIdx.x);
  double S1, S2;
  slab_pair_sum256(slab, rows, c, sh, S1, S2);
  if (threadIdx.x == 0) {
    bn_fwd_coef(true, S1, S2, count, gamma, beta, rmean, rvar, momentum, eps,
                mean_offset ? mean_offset[c] : 0.f, bn_out, HID, c);
    if (c == 0 && tracked) *tracked += 1;
  }
}

__global__ void __launch_bounds__(256) k_bn_bwd_stats(const double* __restrict__ slab, int rows,
                                                      double count, int zero_coef,
                                                      float* __restrict__ dgamma,
                                                      float* __restrict__ dbeta,
                                                      float* __restrict__ bwc) {
  __shared__ double sh[4];
  const int c = blockIdx.x;
  double S1, S2;
  slab_pair_sum256(slab, rows, c, sh, S1, S2);
  if (threadIdx.x == 0) bn_bwd_coef(S1, S2, count, zero_coef, dgamma, dbeta, bwc, HID, c);
}

// dW (f32 slab [rows][64*out_cols]) and db (f64 slab [rows][64]) in one launch.  A block folds
// RD_C consecutive output elements: thread (cc, rg) adds rows rg, rg + RD_G, ... of element cc
// (every load instruction reads 64-byte row pieces, up to 16 in flight per thread; 64 row groups, since
// the layer-0 slab has 2048 rows and the fold is a latency chain), then the RD_G partials are
// combined in fixed order.  [one wave per element with lane = row touched 64 lines
// per load: 32 us for the three layers of a step]
constexpr int RD_C = 16, RD_G = 64;      // 1024 threads
__host__ __device__ inline int dw_db_blocks(int out_cols) { return (HID * out_cols + HID) / RD_C; }
__device__ __forceinline__ void dw_db_reduce_block(const float* __restrict__ dw_slab,
                                                   const double* __restrict__ db_slab, int rows,
                                                   int out_cols, int take_cols,
                                                   float* __restrict__ dW, int ldw,
                                                   float* __restrict__ db, int block) {
  __shared__ double sh[RD_G][RD_C];
  const int nw = HID * out_cols;                    // a multiple of RD_C: a block is all dW or all db
  const int cc = threadIdx.x % RD_C, rg = threadIdx.x / RD_C;
  const int e = block * RD_C + cc;
  double s = 0.0;
  if (e < nw) {
    int r = rg;
    for (; r + 15 * RD_G < rows; r += 16 * RD_G) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = dw_slab[(int64_t)(r + u * RD_G) * nw + e];
#pragma unroll
      for (int u = 0; u < 16; ++u) s += (double)v[u];
    }
    for (; r + 3 * RD_G < rows; r += 4 * RD_G) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = dw_slab[(int64_t)(r + u * RD_G) * nw + e];
#pragma unroll
      for (int u = 0; u < 4; ++u) s += (double)v[u];
    }
    for (; r < rows; r += RD_G) s += (double)dw_slab[(int64_t)r * nw + e];
  } else {
    int r = rg;
    for (; r + 7 * RD_G < rows; r += 8 * RD_G) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = db_slab[(int64_t)(r + u * RD_G) * HID + (e - nw)];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; r < rows; r += RD_G) s += db_slab[(int64_t)r * HID + (e - nw)];
  }
  sh[rg][cc] = s;
  __syncthreads();
  __shared__ double sh2[RD_G / 8][RD_C];
  if (rg < RD_G / 8) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += sh[8 * rg + k][cc];
    sh2[rg][cc] = t;
  }
  __syncthreads();
  if (rg == 0) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < RD_G / 8; ++k) t += sh2[k][cc];
    if (e < nw) {
      const int o = e / out_cols, c2 = e % out_cols;
      if (c2 < take_cols) dW[(int64_t)o * ldw + c2] = (float)t;
    } else {
      db[e - nw] = (float)t;
    }
  }
}

// several layers' slabs in ONE launch (the reductions do not feed the backward chain, so they can
// all wait for its end: one launch instead of one per layer)
__global__ void __launch_bounds__(RD_C * RD_G) k_dw_db_reduce_multi(cgnn_dw_jobs jobs) {
  int block = blockIdx.x;
#pragma unroll
  for (int i = 0; i < CGNN_DW_MAX_JOBS; ++i) {
    if (i >= jobs.n) return;
    const int nb = dw_db_blocks(jobs.out_cols[i]);
    if (block < nb) {
      dw_db_reduce_block(jobs.dw_slab[i], jobs.db_slab[i], jobs.rows[i], jobs.out_cols[i], jobs.take_cols[i],
                         jobs.dW[i], jobs.take_cols[i], jobs.db[i], block);
      return;
    }
    block -= nb;
  }
}

int g_grid_cache[CGNN_MAX_DEVICES] = {};
int g_grid_override = 0;   // cgnn_set_fused_grid (test hook): > 0 replaces the CU count

int fused_grid() {
  if (g_grid_override > 0) return g_grid_override;
  const int dev = cgnn_device_ordinal();
  if (g_grid_cache[dev] == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      return 256;
    g_grid_cache[dev] = cus;
  }
  return g_grid_cache[dev];
}

__global__ void k_rng_advance(uint32_t* state, int n) {
  const int i = threadIdx.x;
  if (i < n) state[i] = rng_refresh(state[i], i);
}

}  // namespace

extern "C" {

int cgnn_fused_grid(void) { return fused_grid(); }

int cgnn_set_fused_grid(int32_t workgroups) {
  if (workgroups < 0 || workgroups > 65535) return CGNN_EINVAL;
  g_grid_override = workgroups;
  return CGNN_OK;
}

int cgnn_rng_advance(uint32_t* state, int32_t n, void* stream) {
  if (!state || n <= 0 || n > 64) return CGNN_EINVAL;
  k_rng_advance<<<1, 64, 0, cgnn_stream(stream)>>>(state, n);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

int cgnn_bn_reduce(const double* slab, int32_t rows, int32_t width, double* sums, void* stream) {
  if (!slab || !sums || rows <= 0 || width <= 0) return CGNN_EINVAL;
  k_slab_reduce<double><<<(width + 3) / 4, 256, 0, cgnn_stream(stream)>>>(slab, rows, width, sums,
                                                                        nullptr, 1, 1, 1);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

int cgnn_bn_finalize(const double* sums, double count, const double* count_dev, const float* gamma,
                     const float* beta, float* running_mean, float* running_var, float momentum,
                     float eps, int32_t training, float* bn_out, const float* mean_offset, void* stream) {
  if (!gamma || !beta || !running_mean || !running_var || !bn_out) return CGNN_EINVAL;
  if (training && (!sums || (!count_dev && count <= 0.0))) return CGNN_EINVAL;
  k_bn_finalize<<<1, 64, 0, cgnn_stream(stream)>>>(sums, count, count_dev, gamma, beta, running_mean,
                                                   running_var, momentum, eps, training, bn_out, mean_offset);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

int cgnn_bn_bwd_finalize(const double* sums, double count, const double* count_dev,
                         int32_t zero_coef, float* dgamma, float* dbeta, float* bwc, void* stream) {
  if (!sums || !dgamma || !dbeta || !bwc || (!count_dev && count <= 0.0)) return CGNN_EINVAL;
  k_bn_bwd_finalize<<<1, 64, 0, cgnn_stream(stream)>>>(sums, count, count_dev, zero_coef, dgamma, dbeta, bwc);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

int cgnn_bn_stats_finalize_rng(const double* slab, int32_t rows, double count, const float* gamma,
                               const float* beta, float* running_mean, float* running_var,
                               float momentum, float eps, int64_t* num_batches_tracked, float* bn_out,
                               uint32_t* rng_state, int32_t rng_n, const float* mean_offset, void* stream) {
  if (!slab || rows <= 0 || count <= 0.0 || !gamma || !beta || !running_mean || !running_var || !bn_out)
    return CGNN_EINVAL;
  if (rng_n < 0 || rng_n > 64 || (rng_n > 0 && !rng_state)) return CGNN_EINVAL;
  k_bn_fwd_stats<<<HID, 256, 0, cgnn_stream(stream)>>>(
      slab, rows, count, gamma, beta, running_mean, running_var, momentum, eps,
      reinterpret_cast<long long*>(num_batches_tracked), bn_out, rng_state, rng_n, mean_offset);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

int cgnn_bn_bwd_stats_finalize(const double* slab, int32_t rows, double count, int32_t zero_coef,
                               float* dgamma, float* dbeta, float* bwc, void* stream) {
  if (!slab || rows <= 0 || count <= 0.0 || !dgamma || !dbeta || !bwc) return CGNN_EINVAL;
  k_bn_bwd_stats<<<HID, 256, 0, cgnn_stream(stream)>>>(slab, rows, count, zero_coef, dgamma, dbeta, bwc);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

int cgnn_dw_db_reduce_multi(const cgnn_dw_jobs* jobs, void* stream) {
  if (!jobs || jobs->n < 1 || jobs->n > CGNN_DW_MAX_JOBS) return CGNN_EINVAL;
  int total = 0;
  for (int i = 0; i < jobs->n; ++i) {
    if (!jobs->dw_slab[i] || !jobs->db_slab[i] || !jobs->dW[i] || !jobs->db[i] || jobs->rows[i] <= 0 ||
        jobs->out_cols[i] <= 0 || jobs->take_cols[i] <= 0 || jobs->take_cols[i] > jobs->out_cols[i])
      return CGNN_EINVAL;
    total += (HID * jobs->out_cols[i] + HID) / RD_C;
  }
  k_dw_db_reduce_multi<<<total, RD_C * RD_G, 0, cgnn_stream(stream)>>>(*jobs);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

int cgnn_slab_reduce_f32(const float* slab, int32_t rows, int32_t out_rows, int32_t out_cols,
                         int32_t take_cols, float* out, int32_t ld_out, void* stream) {
  if (!slab || !out || rows <= 0 || out_rows <= 0 || out_cols <= 0 || take_cols <= 0 ||
      take_cols > out_cols || ld_out < take_cols)
    return CGNN_EINVAL;
  const int width = out_rows * out_cols;
  k_slab_reduce<float><<<(width + 3) / 4, 256, 0, cgnn_stream(stream)>>>(
      slab, rows, width, nullptr, out, out_cols, take_cols, ld_out);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

int cgnn_slab_reduce_f32_split(const float* slab, int32_t rows, int32_t width, int32_t split, float* out,
                               float* out_tail, void* stream) {
  if (!slab || !out || !out_tail || rows <= 0 || width <= 0 || split <= 0 || split >= width) return CGNN_EINVAL;
  k_slab_reduce<float><<<(width + 3) / 4, 256, 0, cgnn_stream(stream)>>>(slab, rows, width, nullptr, out, width,
                                                                        width, width, out_tail, split);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

int cgnn_slab_reduce_f64_multi(const cgnn_reduce_jobs* jobs, void* stream) {
  if (!jobs || jobs->n < 0 || jobs->n > CGNN_REDUCE_MAX_JOBS) return CGNN_EINVAL;
  if (jobs->n == 0) return CGNN_OK;
  int wmax = 0;
  for (int j = 0; j < jobs->n; ++j) {
    if (!jobs->slab[j] || !jobs->out[j] || jobs->rows[j] <= 0 || jobs->width[j] <= 0) return CGNN_EINVAL;
    wmax = jobs->width[j] > wmax ? jobs->width[j] : wmax;
  }
  k_slab_reduce_multi<<<dim3((wmax + 3) / 4, jobs->n), 256, 0, cgnn_stream(stream)>>>(*jobs);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

}  // extern "C"
