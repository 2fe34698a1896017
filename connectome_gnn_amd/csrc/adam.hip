// adam.hip -- the optimizer update of a training step as ONE launch (gfx950).
//
// The reference trains with torch.optim.Adam(lr, weight_decay) (train.py / demo.py:105-134); torch's
// fused multi-tensor Adam is two launches (step counters += 1, then the update) and takes 7-43 us
// for the 15 k - 400 k parameters of these models.  Here every parameter tensor of a group is
// updated by one grid (1024 elements per workgroup), and the shared step counter is advanced by
// the same launch: every workgroup reads the counter, announces that it has (one atomic), and the
// last one to arrive writes counter + 1 -- nothing else of the launch reads it afterwards.
//
// Arithmetic = torch's Adam, L2 weight decay (not decoupled), no amsgrad:
//   g += wd * p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2
//   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// or torch's AdamW (decoupled weight decay):  p *= 1 - lr wd  first, then the update above with g untouched.
//
// Two entries share one body.  cgnn_adam_step takes the hyper-parameters by value: a captured launch keeps the
// values it was captured with.  cgnn_adam_step_dev reads them from a row of doubles on the device WHEN IT RUNS
// (cgnn_optim.h), so a replayed launch follows a learning-rate schedule; with equal values the two give equal bits.
#include "common.h"

namespace {

constexpr int ADAM_THR = 256;
constexpr int ADAM_PER_BLOCK = 4 * ADAM_THR;

// Thread 0 reads the step counter for the workgroup and, with `advance`, takes part in advancing it.  The caller's
// __syncthreads() publishes *s_step.
__device__ __forceinline__ void adam_read_step(float* __restrict__ step, uint32_t* __restrict__ arrivals, int advance,
                                               float* s_step) {
  if (threadIdx.x == 0) {
    const float s = __uint_as_float(__atomic_load_n(reinterpret_cast<uint32_t*>(step), __ATOMIC_RELAXED));
    *s_step = s;
    if (advance) {
      __threadfence();                              // the read above is complete before we announce it
      const uint32_t old = atomicAdd(arrivals, 1u);
      if (old == gridDim.x - 1) {                   // every workgroup has read `step`
        __atomic_store_n(reinterpret_cast<uint32_t*>(step), __float_as_uint(s + 1.0f), __ATOMIC_RELAXED);
        __atomic_store_n(arrivals, 0u, __ATOMIC_RELAXED);
      }
    }
  }
}

template <bool DECOUPLED>
__device__ __forceinline__ void adam_update(const cgnn_adam_jobs& jobs, float s_step, double lr_d, double b1_d,
                                            double b2_d, double eps_d, double wd_d) {
  // hyper-parameters arrive as the host's doubles and are rounded where torch rounds them:
  // beta -> float for the multiply, (1 - beta) computed in double THEN rounded (1 - 0.999f is
  // 1.3e-5 off 0.001f), the bias corrections and lr / bc1 in double
  const double t = (double)s_step + 1.0;
  const float b2 = (float)b2_d, w1 = (float)(1.0 - b1_d), w2 = (float)(1.0 - b2_d);
  const float bc2_sqrt = (float)sqrt(1.0 - pow(b2_d, t));
  const float step_size = (float)(lr_d / (1.0 - pow(b1_d, t)));
  const float eps = (float)eps_d, wd = (float)wd_d;
  // AdamW: 1 - lr * wd as torch forms it, a product and a difference of doubles, rounded to float once
  const float shrink = (float)(1.0 - __dmul_rn(lr_d, wd_d));

  int block = blockIdx.x;
#pragma unroll 1
  for (int i = 0; i < jobs.n; ++i) {
    const int64_t n = jobs.numel[i];
    const int nb = (int)((n + ADAM_PER_BLOCK - 1) / ADAM_PER_BLOCK);
    if (block < nb) {
      float* __restrict__ p = jobs.param[i];
      const float* __restrict__ g = jobs.grad[i];
      float* __restrict__ m = jobs.exp_avg[i];
      float* __restrict__ v = jobs.exp_avg_sq[i];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t e = (int64_t)block * ADAM_PER_BLOCK + u * ADAM_THR + threadIdx.x;
        if (e < n) {
          // (__fmul_rn: the decayed parameter is rounded before the update is subtracted, as p.mul_() rounds it)
          const float pe = DECOUPLED ? __fmul_rn(p[e], shrink) : p[e];
          const float ge = DECOUPLED ? g[e] : fmaf(wd, pe, g[e]);
          const float m0 = m[e];
          const float me = fmaf(w1, ge - m0, m0);                 // lerp(m, g, 1 - b1)
          const float ve = fmaf(w2 * ge, ge, b2 * v[e]);
          m[e] = me;
          v[e] = ve;
          p[e] = pe - step_size * me / (sqrtf(ve) / bc2_sqrt + eps);
        }
      }
      return;
    }
    block -= nb;
  }
}

__global__ void __launch_bounds__(ADAM_THR) k_adam(cgnn_adam_jobs jobs, float* __restrict__ step,
                                                   uint32_t* __restrict__ arrivals, int advance,
                                                   double lr_d, double b1_d, double b2_d, float eps, float wd) {
  __shared__ float s_step;
  adam_read_step(step, arrivals, advance, &s_step);
  __syncthreads();
  adam_update<false>(jobs, s_step, lr_d, b1_d, b2_d, (double)eps, (double)wd);
}

// The hyper-parameters from a row {lr, beta1, beta2, eps, weight_decay} of doubles on the device.  Every thread issues
// the five reads of the row (one address per instruction: a broadcast) BEFORE thread 0 issues its read of the counter,
// and nobody waits in between: neither address depends on the other's data, both are vector loads that return in
// order, so the workgroup waits for one trip to memory, not two.  (Loads of device scope, as for the counter: the row
// was written by an earlier command of the stream.  As plain loads they became scalar loads, which share their wait
// counter with the kernel arguments: thread 0 then waited for the row before it could issue the counter's read.
// Lanes 0-4 reading and the workgroup sharing through LDS measured 0.01-0.02 us above this form.)  Nothing in the
// launch writes the row.
template <bool DECOUPLED>
__global__ void __launch_bounds__(ADAM_THR) k_adam_dev(cgnn_adam_jobs jobs, float* __restrict__ step,
                                                       uint32_t* __restrict__ arrivals, int advance,
                                                       const double* __restrict__ hyper) {
  __shared__ float s_step;
  double h[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) h[i] = __hip_atomic_load(hyper + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  adam_read_step(step, arrivals, advance, &s_step);
  __syncthreads();
  adam_update<DECOUPLED>(jobs, s_step, h[0], h[1], h[2], h[3], h[4]);
}

// What both entries require of the pointers and the jobs; *blocks: the grid.
int adam_grid(const cgnn_adam_jobs* jobs, const float* step, const uint32_t* arrivals, int64_t* blocks) {
  if (!jobs || jobs->n < 1 || jobs->n > CGNN_ADAM_MAX_JOBS || !step || !arrivals) return CGNN_EINVAL;
  int64_t nb = 0;
  for (int i = 0; i < jobs->n; ++i) {
    if (jobs->numel[i] < 0 || !jobs->param[i] || !jobs->grad[i] || !jobs->exp_avg[i] || !jobs->exp_avg_sq[i])
      return CGNN_EINVAL;
    nb += (jobs->numel[i] + ADAM_PER_BLOCK - 1) / ADAM_PER_BLOCK;
  }
  if (nb == 0) nb = 1;                               // still advances the counter
  if (nb > 0x7fffffff) return CGNN_EUNSUPPORTED;
  *blocks = nb;
  return CGNN_OK;
}

}  // namespace

extern "C" int cgnn_adam_step(const cgnn_adam_jobs* jobs, float* step, uint32_t* arrivals,
                              int32_t advance, double lr, double beta1, double beta2, double eps,
                              double weight_decay, void* stream) {
  if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
    return CGNN_EINVAL;
  int64_t blocks = 0;
  const int rc = adam_grid(jobs, step, arrivals, &blocks);
  if (rc != CGNN_OK) return rc;
  k_adam<<<(unsigned)blocks, ADAM_THR, 0, cgnn_stream(stream)>>>(*jobs, step, arrivals, advance ? 1 : 0, lr,
                                                                 beta1, beta2, (float)eps, (float)weight_decay);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

extern "C" int cgnn_adam_step_dev(const cgnn_adam_jobs* jobs, float* step, uint32_t* arrivals, int32_t advance,
                                  const double* hyper, int32_t decoupled, void* stream) {
  if (!hyper || cgnn_misaligned({hyper}, 7) || (decoupled != 0 && decoupled != 1)) return CGNN_EINVAL;
  int64_t blocks = 0;
  const int rc = adam_grid(jobs, step, arrivals, &blocks);
  if (rc != CGNN_OK) return rc;
  const auto kernel = decoupled ? k_adam_dev<true> : k_adam_dev<false>;
  kernel<<<(unsigned)blocks, ADAM_THR, 0, cgnn_stream(stream)>>>(*jobs, step, arrivals, advance ? 1 : 0, hyper);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
