// wpaths.hip -- weighted shortest-path node measures of a device-resident cohort of dense connectivity matrices
// (float [S, n, n]) at the thresholds of cgnn_ingest_select / cgnn_ingest_count:
// cgnn_ingest_wpaths, cgnn_ingest_wpaths_workspace_bytes.
//
// Per subject with matrix A and threshold t: e_ij iff i != j, A_ij > t and A_ij > 0 (ingest_rows.h); nothing is
// symmetrised.  wmax = max_{e_ij} A_ij; l_ij = wmax / A_ij where e_ij (one correctly rounded fp32 division: every
// length is >= 1, the strongest edge has length exactly 1), else +inf.  dw_ij = the smallest sum of lengths along a
// directed path i -> ... -> j of kept edges, dw_ii = 0, +inf without a path; R_i = { j != i : dw_ij finite },
// r_i = |R_i|.
//   weighted_nodal_efficiency  (1 / (n - 1)) sum_{j in R_i} 1 / dw_ij                     (0 for n == 1)
//   weighted_closeness         (r_i / (n - 1)) (r_i / sum_{j in R_i} dw_ij)               (0 for r_i == 0)
//   weighted_eccentricity      max_{j in R_i} dw_ij / (n - 1)                             (0 for r_i == 0 or n == 1)
//
//   k_wpaths<B>  one launch: a batched blocked Floyd-Warshall (min-plus).  A workgroup of 8 waves owns a subject, grid
//                stride; its distance slab D [npad][npad] fp32, npad = ceil(n / B) B, is workgroup blockIdx.x's slice of
//                the workspace (one slab per workgroup of the launch, not per subject) and stays in L2.
//     block    B = 32 while npad <= 512, B = 16 beyond (to n = 1024): the two panels of a round, 2 B npad floats, and the
//              diagonal tile in both layouts take 136 KB of LDS at the largest n of either rule.
//     build    a wave per row, two passes over A: wmax (fmaxf: no order), then l_ij, +inf or the zero diagonal; the
//              padding is +inf.
//     rounds   over the diagonal blocks K, nt = npad / B of them:
//       1  the diagonal tile in LDS, B steps of Floyd-Warshall over all 512 threads (a barrier a step); it is left in
//          LDS row-major and transposed.
//       2  the row panel D[K, :] and the column panel D[:, K], a wave per B x B tile: D[K, J] = min(D[K, J],
//          D[K, K] (x) D[K, J]) and D[I, K] = min(D[I, K], D[I, K] (x) D[K, K]) (the closed diagonal tile makes the
//          out-of-place product the in-place relaxation).  Both panels stay in LDS, the column panel transposed
//          ([k][i]: a lane's rows are consecutive floats), and go back to the slab.
//       3  every other tile D[I, J] = min(D[I, J], D[I, K] (x) D[K, J]): a wave per tile, the tile in registers
//          ((B / 8)^2 per lane: lane (r, c) = (lane / 8, lane % 8) owns rows r B/8 .., columns c B/8 ..), the panels
//          from LDS (two 16-byte reads per k), two k per v_min3_f32; the next tile of the wave is loaded before the
//          current one is relaxed.  Only these tiles cross L2 in a round.
//     epilogue a wave per row of the finished slab: r_i, sum 1 / dw, sum dw, max dw, in fp64; the row copied to `dist`
//              if that is asked for.
// Arithmetic: distances are fp32 sums of fp32 lengths (every candidate is a sum of positive terms; a min keeps one of
// them).  The three row reductions are taken in fp64 -- lane l over the columns l, l + 64, .. ascending, the lanes
// folded by a butterfly -- and rounded to fp32 once.  No atomics, and no work assignment depends on the grid: the
// same bits on every run and for every grid.  The round count is fixed, so a kept non-finite weight cannot hang the
// call.  Element offsets into `matrices`, `x`, `dist` and the workspace are 64-bit.
// The request (0 to 3 distinct ids, distinct columns below ldx), the cohort's size (n <= CGNN_WPATH_MAX_NODES) and
// its buffers are checked by measure_request.h, which also holds the LDS rules of the launch.
#include <math.h>

#include "ingest_rows.h"
#include "measure_request.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kLdsBytes = 160 * 1024;
constexpr int kWideNodes = 512;               // npad up to here: blocks of 32; beyond: of 16

enum {
  kNodal = CGNN_WPATH_NODAL_EFFICIENCY,
  kCloseness = CGNN_WPATH_CLOSENESS,
  kEccentricity = CGNN_WPATH_ECCENTRICITY
};

typedef cgnn_columns<CGNN_NUM_WPATH_MEASURES> Columns;

// the block rule, and what follows from it
inline int block_of(int n) { return ((n + 31) & ~31) <= kWideNodes ? 32 : 16; }
inline int padded(int n, int B) { return (n + B - 1) / B * B; }
inline size_t lds_of(int npad, int B) { return ((size_t)2 * B * npad + 2 * B * B) * sizeof(float); }
inline int64_t slab_bytes(int npad) { return (int64_t)npad * npad * (int64_t)sizeof(float); }

__device__ __forceinline__ float min3(float a, float b, float c) { return fminf(fminf(a, b), c); }

__device__ __forceinline__ void wave_sync() {
  // the wave's LDS writes before its later reads, and its reads before its later writes
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One lane's E x E piece of a B x B tile of the slab: rows r0 .., columns c0 .. (E = 4: 16-byte accesses)
template <int E>
__device__ __forceinline__ void load_tile(const float* D, int npad, int r0, int c0, float (&d)[E][E]) {
#pragma unroll
  for (int a = 0; a < E; ++a) {
    const float* p = D + (int64_t)(r0 + a) * npad + c0;
    if constexpr (E == 4) {
      const cgnn_f32x4 v = *reinterpret_cast<const cgnn_f32x4*>(p);
#pragma unroll
      for (int b = 0; b < 4; ++b) d[a][b] = v[b];
    } else {
#pragma unroll
      for (int b = 0; b < E; ++b) d[a][b] = p[b];
    }
  }
}
template <int E>
__device__ __forceinline__ void store_tile(float* D, int npad, int r0, int c0, const float (&d)[E][E]) {
#pragma unroll
  for (int a = 0; a < E; ++a) {
    float* p = D + (int64_t)(r0 + a) * npad + c0;
    if constexpr (E == 4) {
      *reinterpret_cast<cgnn_f32x4*>(p) = cgnn_f32x4{d[a][0], d[a][1], d[a][2], d[a][3]};
    } else {
#pragma unroll
      for (int b = 0; b < E; ++b) p[b] = d[a][b];
    }
  }
}

// d[a][b] = min(d[a][b], min_k colT[k][a] + row[k][b]) over the B values of k, two per min3.  colT and row point at
// the lane's first row / column of the two LDS operands, ldc / ldr are their strides in floats.
template <int B>
__device__ __forceinline__ void relax(float (&d)[B / 8][B / 8], const float* colT, int ldc, const float* row, int ldr) {
  constexpr int E = B / 8;
  typedef float vec __attribute__((ext_vector_type(E)));  // (every operand address is a multiple of E floats)
  // the operands of the next two k are read before the current two are used
  vec a0 = *reinterpret_cast<const vec*>(colT), a1 = *reinterpret_cast<const vec*>(colT + ldc);
  vec b0 = *reinterpret_cast<const vec*>(row), b1 = *reinterpret_cast<const vec*>(row + ldr);
#pragma unroll
  for (int k = 0; k < B; k += 2) {
    vec na0 = a0, na1 = a1, nb0 = b0, nb1 = b1;
    if (k + 2 < B) {
      na0 = *reinterpret_cast<const vec*>(colT + (k + 2) * ldc), na1 = *reinterpret_cast<const vec*>(colT + (k + 3) * ldc);
      nb0 = *reinterpret_cast<const vec*>(row + (k + 2) * ldr), nb1 = *reinterpret_cast<const vec*>(row + (k + 3) * ldr);
    }
#pragma unroll
    for (int a = 0; a < E; ++a)
#pragma unroll
      for (int b = 0; b < E; ++b) d[a][b] = min3(d[a][b], a0[a] + b0[b], a1[a] + b1[b]);
    a0 = na0, a1 = na1, b0 = nb0, b1 = nb1;
  }
}

template <int B>
__global__ __launch_bounds__(kThreads) void k_wpaths(const float* __restrict__ matrices, int64_t S, int n,
                                                     const float* __restrict__ thr, Columns cols, float* slabs,
                                                     float* __restrict__ x, float* __restrict__ dist) {
  constexpr int E = B / 8;                    // rows and columns of a tile a lane owns
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int npad = (n + B - 1) / B * B, nt = npad / B;
  float* rowp = reinterpret_cast<float*>(lds);            // [B][npad]  D[K b + k][j]
  float* colT = rowp + B * npad;                          // [B][npad]  D[i][K b + k] at [k][i]
  float* dkk = colT + B * npad;                           // [B][B]     the diagonal tile
  float* dkkT = dkk + B * B;                              // [B][B]     transposed
  float* wave_max = dkk;                                  // [kWaves]   of the build, before any round
  float* D = slabs + (int64_t)blockIdx.x * npad * npad;
  const int lr = (lane >> 3) * E, lc = (lane & 7) * E;    // the lane's first row and column inside a tile

  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const float* __restrict__ A = matrices + s * (int64_t)n * n;
    const float thr_s = thr[s];

    // ---- build: wmax, then the lengths ----
    float mx = 0.0f;
    for (int i = wave; i < n; i += kWaves) {
      int cnt;
      float sum, m;
      cgnn_row_kept<true>(A + (int64_t)i * n, i, n, thr_s, lane, cnt, sum, m);
      mx = fmaxf(mx, m);
    }
    if (lane == 0) wave_max[wave] = mx;
    __syncthreads();
    float wmax = wave_max[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) wmax = fmaxf(wmax, wave_max[w]);
    for (int i = wave; i < npad; i += kWaves) {
      const float* __restrict__ row = A + (int64_t)i * n;
      for (int j = lane; j < npad; j += 64) {
        float v = INFINITY;
        if (i < n && j < n) {
          const float a = row[j];
          if (j == i) v = 0.0f;
          else if (cgnn_kept(a, thr_s)) v = wmax / a;
        }
        D[(int64_t)i * npad + j] = v;
      }
    }
    __syncthreads();

    // ---- rounds ----
    for (int K = 0; K < nt; ++K) {
      const int kb = K * B;
      // 1: the diagonal tile
      for (int e = t; e < B * B; e += kThreads) dkk[e] = D[(int64_t)(kb + e / B) * npad + kb + e % B];
      __syncthreads();
      for (int k = 0; k < B; ++k) {
        // (row k and column k do not change in step k: d_kk >= 0)
        for (int e = t; e < B * B; e += kThreads) {
          const int i = e / B, j = e % B;
          dkk[e] = fminf(dkk[e], dkk[i * B + k] + dkk[k * B + j]);
        }
        __syncthreads();
      }
      for (int e = t; e < B * B; e += kThreads) {
        const int i = e / B, j = e % B;
        const float v = dkk[e];
        dkkT[j * B + i] = v;
        D[(int64_t)(kb + i) * npad + kb + j] = v;
      }
      __syncthreads();

      // 2: the panels, a wave per tile; jobs 0 .. nt - 2 are the row panel's, the rest the column panel's
      for (int q = wave; q < 2 * (nt - 1); q += kWaves) {
        const bool is_row = q < nt - 1;
        int T = is_row ? q : q - (nt - 1);
        T += T >= K;                                      // the tiles besides K
        const int r0 = (is_row ? kb : T * B) + lr, c0 = (is_row ? T * B : kb) + lc;
        float d[E][E];
        load_tile<E>(D, npad, r0, c0, d);
        if (is_row) {
#pragma unroll
          for (int a = 0; a < E; ++a)
#pragma unroll
            for (int b = 0; b < E; ++b) rowp[(lr + a) * npad + T * B + lc + b] = d[a][b];
          wave_sync();
          relax<B>(d, dkkT + lr, B, rowp + T * B + lc, npad);
          wave_sync();
#pragma unroll
          for (int a = 0; a < E; ++a)
#pragma unroll
            for (int b = 0; b < E; ++b) rowp[(lr + a) * npad + T * B + lc + b] = d[a][b];
        } else {
#pragma unroll
          for (int a = 0; a < E; ++a)
#pragma unroll
            for (int b = 0; b < E; ++b) colT[(lc + b) * npad + T * B + lr + a] = d[a][b];
          wave_sync();
          relax<B>(d, colT + T * B + lr, npad, dkk + lc, B);
          wave_sync();
#pragma unroll
          for (int a = 0; a < E; ++a)
#pragma unroll
            for (int b = 0; b < E; ++b) colT[(lc + b) * npad + T * B + lr + a] = d[a][b];
        }
        store_tile<E>(D, npad, r0, c0, d);
      }
      __syncthreads();

      // 3: every tile outside row K and column K, a wave per tile, the next tile in flight
      const int jobs = (nt - 1) * (nt - 1);
      float d[E][E], nx[E][E];
      int In = 0, Jn = 0;
      if (wave < jobs) {
        In = wave / (nt - 1), Jn = wave % (nt - 1);
        In += In >= K, Jn += Jn >= K;
        load_tile<E>(D, npad, In * B + lr, Jn * B + lc, nx);
      }
      for (int q = wave; q < jobs; q += kWaves) {
        const int I = In, J = Jn, qn = q + kWaves;
#pragma unroll
        for (int a = 0; a < E; ++a)
#pragma unroll
          for (int b = 0; b < E; ++b) d[a][b] = nx[a][b];
        if (qn < jobs) {
          In = qn / (nt - 1), Jn = qn % (nt - 1);
          In += In >= K, Jn += Jn >= K;
          load_tile<E>(D, npad, In * B + lr, Jn * B + lc, nx);
        }
        relax<B>(d, colT + I * B + lr, npad, rowp + J * B + lc, npad);
        store_tile<E>(D, npad, I * B + lr, J * B + lc, d);
      }
      __syncthreads();
    }

    // ---- epilogue: a wave per row ----
    const bool want_x = cols.col[kNodal] >= 0 || cols.col[kCloseness] >= 0 || cols.col[kEccentricity] >= 0;
    for (int i = wave; i < n; i += kWaves) {
      const float* Di = D + (int64_t)i * npad;
      float* __restrict__ out = dist ? dist + (s * n + i) * (int64_t)n : nullptr;
      int r = 0;
      double inv = 0.0, sum = 0.0, far = 0.0;
      for (int j = lane; j < n; j += 64) {
        const float v = Di[j];
        if (out) out[j] = v;
        if (j != i && v < INFINITY) {
          const double dv = (double)v;
          ++r;
          inv += 1.0 / dv;
          sum += dv;
          far = fmax(far, dv);
        }
      }
      if (!want_x) continue;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        r += __shfl_xor(r, o, 64);
        far = fmax(far, __shfl_xor(far, o, 64));
      }
      inv = cgnn_wave_sum(inv);
      sum = cgnn_wave_sum(sum);
      if (lane == 0) {
        float* __restrict__ o = x + (s * n + i) * (int64_t)cols.ldx;
        const double nm1 = (double)(n - 1);
        if (cols.col[kNodal] >= 0) o[cols.col[kNodal]] = n > 1 ? (float)(inv / nm1) : 0.0f;
        if (cols.col[kCloseness] >= 0)
          o[cols.col[kCloseness]] = r > 0 ? (float)(((double)r / nm1) * ((double)r / sum)) : 0.0f;
        if (cols.col[kEccentricity] >= 0) o[cols.col[kEccentricity]] = r > 0 ? (float)(far / nm1) : 0.0f;
      }
    }
    __syncthreads();                          // the next subject's build overwrites the slab
  }
}

// (CGNN_OK, the columns) of a valid call: the cohort's size, then 0 to 3 distinct ids and, with_cols, their columns
int check(int64_t S, int32_t n, const int32_t* measures, int32_t num, const int32_t* cols, int32_t ldx, bool with_cols,
          Columns* c) {
  if (cgnn_check_cohort_upto(S, n, CGNN_WPATH_MAX_NODES) != CGNN_OK) return CGNN_EINVAL;
  return cgnn_check_request(measures, num, 0, cols, ldx, with_cols, c);
}

// the launch's workgroups: one per subject, as many as the CUs hold
int grid_of(int64_t S, size_t lds) { return cgnn_grid_for(S, cgnn_wg_per_cu_by_lds(lds, kLdsBytes)); }

}  // namespace

extern "C" int64_t cgnn_ingest_wpaths_workspace_bytes(int64_t S, int32_t n, const int32_t* measures,
                                                      int32_t num_measures) {
  Columns c;
  if (check(S, n, measures, num_measures, nullptr, 0, false, &c) != CGNN_OK) return CGNN_EINVAL;
  const int B = block_of(n), npad = padded(n, B);
  return grid_of(S, lds_of(npad, B)) * slab_bytes(npad);       // a slab per workgroup of the launch
}

extern "C" int cgnn_ingest_wpaths(const float* matrices, int64_t S, int32_t n, const float* thr,
                                  const int32_t* measures, int32_t num_measures, const int32_t* cols, int32_t ldx,
                                  void* workspace, int64_t workspace_bytes, float* x, int64_t x_bytes, float* dist,
                                  int64_t dist_bytes, void* stream) {
  Columns c;
  if (check(S, n, measures, num_measures, cols, ldx, true, &c) != CGNN_OK) return CGNN_EINVAL;
  if (workspace_bytes < 0 || (reinterpret_cast<uintptr_t>(workspace) & 15)) return CGNN_EINVAL;
  if (x_bytes < 0 || dist_bytes < 0) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  // x [S n][ldx] if measures are asked for, dist [S n][n] if given (n <= 1024: by division too); one of the two
  if (cgnn_check_cohort_buffers(matrices, thr, workspace, x, x_bytes, num_measures > 0, S * n, c.ldx) != CGNN_OK ||
      cgnn_check_cohort_buffers(matrices, thr, workspace, dist, dist_bytes, dist != nullptr, S * n, n) != CGNN_OK ||
      (num_measures == 0 && !dist))
    return CGNN_EINVAL;
  const int B = block_of(n), npad = padded(n, B);
  const size_t lds = lds_of(npad, B);
  if (lds > (size_t)kLdsBytes) return CGNN_EINVAL;          // (n <= CGNN_WPATH_MAX_NODES fits: 136 KB at 512 and 1024)
  const int grid = grid_of(S, lds);
  if (!workspace || workspace_bytes < grid * slab_bytes(npad)) return CGNN_EINVAL;
  if (!(B == 32 ? cgnn_raise_lds_limit<k_wpaths<32>>(kLdsBytes) : cgnn_raise_lds_limit<k_wpaths<16>>(kLdsBytes)))
    return CGNN_ELAUNCH;
  float* slabs = static_cast<float*>(workspace);
  float* xs = num_measures > 0 ? x : nullptr;
  if (B == 32)
    k_wpaths<32><<<grid, kThreads, lds, cgnn_stream(stream)>>>(matrices, S, n, thr, c, slabs, xs, dist);
  else
    k_wpaths<16><<<grid, kThreads, lds, cgnn_stream(stream)>>>(matrices, S, n, thr, c, slabs, xs, dist);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
