// confounds.hip -- the orthonormal basis of every subject's confounds (float [S, T, q], one row per frame), which
// cgnn_ingest_regress (filter.hip) projects out of the ROI time series: cgnn_ingest_confound_basis.
//
// Per subject, in fp64: m_j = the mean of column j, cc_j = c_j - m_j, s_j = sqrt(sum_t cc_j[t]^2); a column with
// s_j == 0 is dropped, the others are u_j = cc_j / s_j.  Gram-Schmidt in the given order: r_j = u_j minus its
// projections on the kept q_k, k < j; d_j = |r_j|^2; kept iff d_j > CGNN_CONFOUND_RANK_TOL, and then q_j = r_j / sqrt(d_j).
// Q is float [T, qpad], qpad = q rounded up to 32: fl32(q_j) in a kept column, exactly 0 in a dropped one and in the
// padding.  A subject with a non-finite s_j (a NaN or Inf anywhere in its confounds) gets an all-NaN Q and rank -1.
//
// cgnn_ingest_confound_basis_masked is the same with a frame mask keep [S, T]: every mean, norm, inner
// product and pivot over the subject's kept frames, zero rows of Q at the censored ones.  The mask is a template argument
// of the kernel and the predicate of frame_mask.h in the two norm passes, where u is staged and in the final write.
//
// The kernel computes that Q by CholeskyQR2: nothing it keeps in LDS depends on T.
//   k_confound_basis<kQ>  kQ = qpad.  A persistent grid over the subjects, a workgroup of 4 waves per subject, grid
//                   stride.  Five passes over the subject's confounds (q / n of what the frames are):
//     means, norms    lane = column, 256 / kQ frame phases; a thread's frames in ascending order, the phases merged
//                     in phase order
//     G = U^T U       the frames 32 at a time (the next block's loads in flight): u centred and scaled into LDS, every
//                     pair (j, k) owned by one thread (a block of kQ / 16 x kQ / 16 pairs), summed over the frames in
//                     ascending order
//     R1              the q x q Cholesky factor G = R1^T R1 in LDS, right-looking; its pivot of column j IS d_j, and
//                     the rank rule is applied to it.  A dropped column leaves a zero row and takes no part.
//     W1 = R1^-1      back-substitution, a thread per column (the dropped rows and columns are zero)
//     G2, R2, W2      the same on Q1 = U W1, formed block by block in LDS, with the kept set held fixed: one pass leaves
//                     |Q1^T Q1 - I| near 1e-11 on motion-like regressors, the second brings it to 1e-15
//     Q = fl32(U (W1 W2))  written [T, kQ] with its zeros
// LDS: 3 matrices of q4 x (q4 + 1) doubles (q4 = q rounded up to 4) and two blocks of 32 x q4: 29 KB at q = 24, 133 KB
// at q = 64.  No atomics, every sum in a fixed order, no work assignment depends on the grid: the same bits on every
// run and for every grid.  Element offsets are 64-bit.
#include <math.h>

#include "frame_mask.h"
#include "measure_request.h"
#include "series_request.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFB = 32;                       // frames of a block
constexpr int kLdsBytes = 160 * 1024;

constexpr int pad_of(int q) { return (q + 31) / 32 * 32; }
constexpr int q4_of(int q) { return (q + 3) / 4 * 4; }

// doubles: mu | inv | s | part [256] | A | W1 | W2 | ub | qb ; then kept [kQ] ints
constexpr size_t lds_of(int kQ, int q) {
  const int q4 = q4_of(q);
  return sizeof(double) * (size_t)(3 * kQ + kThreads + 3 * q4 * (q4 + 1) + 2 * kFB * q4) + sizeof(int) * kQ;
}
static_assert(lds_of(64, CGNN_CONFOUND_MAX) <= (size_t)kLdsBytes, "the widest basis fits the LDS of a CU");

// R (upper, A = R^T R) over the leading q x q of a, in place and right-looking.  first: the rank rule decides kept[]
// (a column whose norm was zero stays dropped); otherwise kept[] is given.  A dropped column leaves a zero row.
__device__ void cholesky(double* a, int ld, int q, int* kept, bool first, int tid) {
  for (int j = 0; j < q; ++j) {
    const double d = a[j * ld + j];           // d_j: what the kept columns before j leave of u_j
    const bool keep = first ? (kept[j] != 0 && d > CGNN_CONFOUND_RANK_TOL) : kept[j] != 0;
    __syncthreads();                          // everyone has read the pivot
    if (tid == 0) kept[j] = keep;
    const double r = sqrt(d);
    for (int k = j + tid; k < q; k += kThreads) a[j * ld + k] = !keep ? 0.0 : (k == j ? r : a[j * ld + k] / r);
    __syncthreads();
    if (keep) {
      const int m = q - j - 1;
      for (int e = tid; e < m * m; e += kThreads) {
        const int i = j + 1 + e / m, k = j + 1 + e % m;
        if (k >= i) a[i * ld + k] -= a[j * ld + i] * a[j * ld + k];
      }
    }
    __syncthreads();
  }
}

// w = r^-1 (upper) over the kept rows and columns, zero elsewhere: a thread per column, sums in ascending order
__device__ void invert(const double* r, double* w, int ld, int q, int q4, const int* kept, int tid) {
  for (int e = tid; e < q4 * ld; e += kThreads) w[e] = 0.0;
  __syncthreads();
  if (tid < q && kept[tid]) {
    const int j = tid;
    w[j * ld + j] = 1.0 / r[j * ld + j];
    for (int i = j - 1; i >= 0; --i) {
      if (!kept[i]) continue;
      double sum = 0.0;
      for (int k = i + 1; k <= j; ++k) sum += r[i * ld + k] * w[k * ld + j];
      w[i * ld + j] = -sum / r[i * ld + i];
    }
  }
  __syncthreads();
}

// kMask: `keep` [S, T] selects the frames.  Every mean, norm, inner product and pivot runs over the
// kept frames Tk of the subject; a censored frame's values are loaded beside its flag (no load waits for another) and
// left out by selection: it is a zero row of u and an exact zero row of Q.
template <int kQ, bool kMask>
__global__ __launch_bounds__(kThreads) void k_confound_basis(const float* __restrict__ conf, int64_t S, int T, int q,
                                                             float* __restrict__ basis, int32_t* __restrict__ rank,
                                                             const uint8_t* __restrict__ keep) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr int kG = kThreads / kQ;           // frame phases of the means and norms
  constexpr int kB = kQ / 16;                 // a thread owns kB x kB pairs of G
  constexpr int kSlots = kFB * kQ / kThreads; // entries of a block of frames per thread
  const int q4 = q4_of(q), ld = q4 + 1;
  double* mu = reinterpret_cast<double*>(lds);          // [kQ]
  double* inv = mu + kQ;                      // [kQ] 1 / s_j, 0 for a dropped column and past q
  double* sn = inv + kQ;                      // [kQ] s_j
  double* part = sn + kQ;                     // [kG][kQ]
  double* A = part + kThreads;                // [q4][ld] G, then R, at last W1 W2
  double* W1 = A + q4 * ld;
  double* W2 = W1 + q4 * ld;
  double* ub = W2 + q4 * ld;                  // [kFB][q4] a block of u
  double* qb = ub + kFB * q4;                 // [kFB][q4] the same block of Q1
  int* kept = reinterpret_cast<int*>(qb + kFB * q4);    // [kQ]

  const int tid = threadIdx.x;
  const int col = tid % kQ, phase = tid / kQ;
  const int r0 = kB * (tid / 16), c0 = kB * (tid % 16);
  const bool owner = r0 < q4 && c0 < q4;      // (q4 is a multiple of 4, kB divides 4: a block is inside or outside)

  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const float* __restrict__ c = conf + s * T * q;
    float* __restrict__ out = basis + s * T * kQ;
    const cgnn_frame_mask<kMask> mask(keep, s * T, T);
    double frames = (double)T;                // Tk: what the means divide by
    if constexpr (kMask) {                    // counted by everyone, merged through `part` (an integer sum: exact)
      int cnt = 0;
      for (int t = tid; t < T; t += kThreads) cnt += mask.kept(t);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
      if ((tid & 63) == 0) part[tid >> 6] = (double)cnt;
      __syncthreads();
      frames = ((part[0] + part[1]) + part[2]) + part[3];
      __syncthreads();                        // the passes below overwrite part
    }

    // ---- means, then centred norms ----
    for (int pass = 0; pass < 2; ++pass) {
      double sum = 0.0;
      if (col < q) {
        const double m = pass ? mu[col] : 0.0;
#pragma unroll 8
        for (int t = phase; t < T; t += kG) {
          const double v = (double)c[(int64_t)t * q + col] - m;
          sum += !mask.kept(t) ? 0.0 : pass ? v * v : v;
        }
      }
      part[phase * kQ + col] = sum;
      __syncthreads();
      if (tid < kQ) {
        double total = part[tid];
        for (int g = 1; g < kG; ++g) total += part[g * kQ + tid];
        if (!pass) {
          mu[tid] = kMask && frames == 0.0 ? 0.0 : total / frames;
        } else {
          const double sj = sqrt(total);
          sn[tid] = sj;
          inv[tid] = tid < q && sj != 0.0 ? 1.0 / sj : 0.0;
          kept[tid] = tid < q && sj != 0.0;
        }
      }
      __syncthreads();
    }
    bool finite = true;
    for (int j = 0; j < q; ++j) finite = finite && isfinite(sn[j]);
    if (!finite) {                            // never "nothing regressed": the subject's output is NaN
      for (int64_t e = tid; e < (int64_t)T * kQ; e += kThreads)
        out[e] = mask.censored((int)(e / kQ)) ? 0.0f : __builtin_nanf("");
      if (tid == 0) rank[s] = -1;
      __syncthreads();                        // (the next subject overwrites sn)
      continue;
    }

    // a block of frames: 32 rows of c are 32 q consecutive floats, loaded into registers a block ahead, then centred
    // and scaled into ub; frames past T are zeros, and so are the columns past q, which nobody writes again
    float pv[kSlots];
    bool pk[kSlots];                          // kMask: the frame of pv[i] is kept
    auto load = [&](int t0) {
#pragma unroll
      for (int i = 0; i < kSlots; ++i) {
        const int e = tid + kThreads * i;
        const bool in = e < kFB * q && t0 + e / q < T;
        pk[i] = in && mask.kept(t0 + e / q);
        pv[i] = in ? c[(int64_t)t0 * q + e] : 0.0f;
      }
    };
    auto store = [&](int t0) {
#pragma unroll
      for (int i = 0; i < kSlots; ++i) {
        const int e = tid + kThreads * i;
        if (e < kFB * q) {
          const int f = e / q, j = e - f * q;
          ub[f * q4 + j] = (kMask ? pk[i] : t0 + f < T) ? ((double)pv[i] - mu[j]) * inv[j] : 0.0;
        }
      }
    };
    for (int e = tid; e < kFB * q4; e += kThreads)
      if (e % q4 >= q) ub[e] = 0.0;
    // this thread's pairs of src^T src over the block
    double acc[kB][kB];
    auto clear = [&]() {
#pragma unroll
      for (int x = 0; x < kB; ++x)
#pragma unroll
        for (int y = 0; y < kB; ++y) acc[x][y] = 0.0;
    };
    auto accumulate = [&](const double* src) {
      if (!owner) return;
      for (int f = 0; f < kFB; ++f) {
        double a[kB], b[kB];
#pragma unroll
        for (int x = 0; x < kB; ++x) a[x] = src[f * q4 + r0 + x];
#pragma unroll
        for (int y = 0; y < kB; ++y) b[y] = src[f * q4 + c0 + y];
#pragma unroll
        for (int x = 0; x < kB; ++x)
#pragma unroll
          for (int y = 0; y < kB; ++y) acc[x][y] = fma(a[x], b[y], acc[x][y]);
      }
    };
    auto store_gram = [&]() {
      if (owner) {
#pragma unroll
        for (int x = 0; x < kB; ++x)
#pragma unroll
          for (int y = 0; y < kB; ++y) A[(r0 + x) * ld + c0 + y] = acc[x][y];
      }
      __syncthreads();
    };
    // dst[f][j] = sum_{k <= j} ub[f][k] w[k][j], k ascending (a dropped k has a zero row)
    auto apply = [&](const double* w, int e) {
      const int f = e / q4, j = e - f * q4;
      double sum = 0.0;
      for (int k = 0; k <= j; ++k) sum = fma(ub[f * q4 + k], w[k * ld + j], sum);
      return sum;
    };

    // ---- G = U^T U, R1, W1 ----
    clear();
    load(0);
    for (int t0 = 0; t0 < T; t0 += kFB) {
      store(t0);
      __syncthreads();
      if (t0 + kFB < T) load(t0 + kFB);       // in flight while this block is summed
      accumulate(ub);
      __syncthreads();
    }
    store_gram();
    cholesky(A, ld, q, kept, true, tid);
    invert(A, W1, ld, q, q4, kept, tid);

    // ---- G2 = Q1^T Q1 with Q1 = U W1, R2, W2 ----
    clear();
    load(0);
    for (int t0 = 0; t0 < T; t0 += kFB) {
      store(t0);
      __syncthreads();
      if (t0 + kFB < T) load(t0 + kFB);
      for (int e = tid; e < kFB * q4; e += kThreads) qb[e] = apply(W1, e);
      __syncthreads();
      accumulate(qb);
    }
    __syncthreads();
    store_gram();
    cholesky(A, ld, q, kept, false, tid);
    invert(A, W2, ld, q, q4, kept, tid);

    // ---- W = W1 W2 (over A), Q = fl32(U W) ----
    for (int e = tid; e < q4 * q4; e += kThreads) {
      const int i = e / q4, j = e - i * q4;
      double v = 0.0;
      for (int k = i; k <= j; ++k) v = fma(W1[i * ld + k], W2[k * ld + j], v);
      A[i * ld + j] = v;
    }
    __syncthreads();
    load(0);
    for (int t0 = 0; t0 < T; t0 += kFB) {
      store(t0);
      __syncthreads();
      if (t0 + kFB < T) load(t0 + kFB);
      for (int e = tid; e < kFB * kQ; e += kThreads) {
        const int f = e / kQ, j = e - f * kQ;
        if (t0 + f < T)
          out[(int64_t)(t0 + f) * kQ + j] = j < q && kept[j] && mask.kept(t0 + f) ? (float)apply(A, f * q4 + j) : 0.0f;
      }
      __syncthreads();
    }
    if (tid == 0) {
      int r = 0;
      for (int j = 0; j < q; ++j) r += kept[j];
      rank[s] = r;
    }
    __syncthreads();                          // the next subject overwrites kept and mu
  }
}

int check(int64_t S, int32_t T, int32_t q) {
  if (S < 0 || S >= ((int64_t)1 << 31) || T < 2 || T > CGNN_MAX_FRAMES) return CGNN_EINVAL;
  return q < 1 || q > CGNN_CONFOUND_MAX ? CGNN_EINVAL : CGNN_OK;
}

template <int kQ, bool kMask>
int launch(const float* conf, int64_t S, int32_t T, int32_t q, const uint8_t* keep, float* basis, int32_t* rank,
           hipStream_t hs) {
  const size_t lds = lds_of(kQ, q);
  if (!cgnn_raise_lds_limit<k_confound_basis<kQ, kMask>>(kLdsBytes)) return CGNN_ELAUNCH;
  const int grid = cgnn_grid_for(S, cgnn_wg_per_cu_by_lds(lds, kLdsBytes));
  k_confound_basis<kQ, kMask><<<grid, kThreads, lds, hs>>>(conf, S, T, q, basis, rank, keep);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

// what both entry points check and do; keep == nullptr: every frame
int basis_call(const float* confounds, int64_t S, int32_t T, int32_t q, const uint8_t* keep, int64_t keep_bytes,
               bool masked, float* basis, int64_t basis_bytes, int32_t* rank, int64_t rank_bytes, void* stream) {
  if (check(S, T, q) != CGNN_OK || basis_bytes < 0 || rank_bytes < 0 || keep_bytes < 0) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (!confounds || !basis || !rank || cgnn_misaligned({confounds, rank}, 3) || cgnn_misaligned({basis}, 15))
    return CGNN_EINVAL;
  if (masked && !keep) return CGNN_EINVAL;
  CGNN_NEED_BYTES(keep, keep_bytes, S * T);
  CGNN_NEED_BYTES(basis, basis_bytes, cgnn_ingest_confound_basis_bytes(S, T, q));
  CGNN_NEED_BYTES(rank, rank_bytes, S * (int64_t)sizeof(int32_t));
  hipStream_t hs = cgnn_stream(stream);
  if (masked)
    return pad_of(q) == 32 ? launch<32, true>(confounds, S, T, q, keep, basis, rank, hs)
                           : launch<64, true>(confounds, S, T, q, keep, basis, rank, hs);
  return pad_of(q) == 32 ? launch<32, false>(confounds, S, T, q, nullptr, basis, rank, hs)
                         : launch<64, false>(confounds, S, T, q, nullptr, basis, rank, hs);
}

}  // namespace

extern "C" int64_t cgnn_ingest_confound_basis_bytes(int64_t S, int32_t T, int32_t q) {
  if (check(S, T, q) != CGNN_OK) return CGNN_EINVAL;
  return S * T * pad_of(q) * (int64_t)sizeof(float);    // (S < 2^31, T <= 2^30, 256: below 2^63)
}

extern "C" int cgnn_ingest_confound_basis(const float* confounds, int64_t S, int32_t T, int32_t q, float* basis,
                                          int64_t basis_bytes, int32_t* rank, int64_t rank_bytes, void* stream) {
  return basis_call(confounds, S, T, q, nullptr, 0, false, basis, basis_bytes, rank, rank_bytes, stream);
}

// frame censoring: the same launch over the frames keep [S, T] selects
extern "C" int cgnn_ingest_confound_basis_masked(const float* confounds, int64_t S, int32_t T, int32_t q,
                                                 const uint8_t* keep, int64_t keep_bytes, float* basis,
                                                 int64_t basis_bytes, int32_t* rank, int64_t rank_bytes, void* stream) {
  return basis_call(confounds, S, T, q, keep, keep_bytes, true, basis, basis_bytes, rank, rank_bytes, stream);
}
