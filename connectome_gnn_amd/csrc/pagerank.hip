// pagerank.hip -- PageRank centrality of a device-resident cohort of dense connectivity matrices (float [S, n, n]) at the
// thresholds of cgnn_ingest_select / cgnn_ingest_count (include/cgnn_pagerank.h): cgnn_ingest_pagerank,
// cgnn_ingest_pagerank_workspace_bytes.
//
// Per subject with matrix A and threshold t: e_ij iff i != j, A_ij > t and A_ij > 0 (ingest_rows.h); nothing is
// symmetrised; entry (i, j) is an edge j -> i.  w_ij = A_ij (weighted) or 1 (binary) where e_ij; c_j = sum_i w_ij;
// x_i = d (sum_j w_ij x_j / c_j + (sum_{c_j == 0} x_j) / n) + (1 - d) / n.
//
//   k_pagerank  one launch; a workgroup of 8 waves owns a subject, grid stride.  Everything of a subject lives in LDS.
//     staging   columns   a thread per column (n <= 256: the rows in 512 / npad slices, npad = n rounded up to 64;
//                         the slices are folded in ascending order) adds the kept entries of its column in ascending
//                         row order (16 loads in flight): c_j of both kinds as doubles, kept as 1 / c_j (0 for a
//                         dangling j).  A c_j that is not finite (a kept +inf) marks the subject: its weighted column
//                         is NaN and is not iterated.
//               rows      a wave per 4 rows counts the kept entries by ballots; wave 0 scans the counts to row offsets.
//               compact   E = the subject's kept entries.  If 2 E bytes fit the space beside the vectors, a wave per
//                         row writes the kept columns (16-bit) behind the row's offset in ascending order; if 6 E
//                         bytes (rounded to 4) fit, the weights (float) too.  Both tests depend on n and E alone.
//     iteration fp64, x = 1 / n at the start; y_j = x_j (1 / c_j) (0 for a dangling j) is kept beside x, twice (the step
//               reads one copy and writes the other: one barrier per step).  A row goes to a fixed group of lanes: 8
//               lanes over the row's compacted entries p = l, l + 8, .. when they are in LDS, else the 64 lanes of a
//               wave over the row itself (columns l, l + 64, .., edge test in flight; the rows come from L2).  The
//               group's partial sums fold in registers (DPP: neighbour, pair, quad; a whole wave by modules.hip's
//               scan); its first lane forms x_i, |x_i - x_i'| and the dangling mass.  Those two are summed over the
//               workgroup in a fixed order: the scan in each wave, then the 8 waves ascending, on every thread alike;
//               the stop test is therefore uniform.  A STEP IS TWO PRODUCTS x -> T(T(x)) and the change is taken
//               between the ends of two steps: a bipartite graph (a star) contracts at exactly d with an error that
//               alternates in sign, and a one-product step would then need more than K_max steps for its change to
//               meet the rule; with two, step K_max changes by at most 2 (1 + d) d^(2 K - 1), far below (1 - d) 2^-42
//               for every d <= 0.99, so the cap cannot be reached in exact arithmetic.
//               The binary and the weighted measure run one after the other off the same staging pass.
// No atomics, and neither the order of any sum nor the assignment of work depends on the grid, the run or on which
// measures are asked for: the same bits on every run, for every grid and every request.  Element offsets into
// `matrices` and `x` are 64-bit.
#include <math.h>

#include "ingest_rows.h"
#include "measure_request.h"
#include "wave_ops.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kLdsBytes = 160 * 1024;
constexpr int kVectors = 5;                   // doubles per node: x, y (twice), 1 / c weighted, 1 / c binary
constexpr int kScratch = 2 * kThreads;        // doubles: the column sums of the row slices, both kinds
constexpr int kRed = 2 * kWaves * 2;          // doubles: (change, dangling mass) per wave, twice
constexpr int kSparseLanes = 8;               // lanes on a row whose entries are in LDS (group8_total)
constexpr int kBatch = 16;                    // entries of a column a thread loads before it adds them
constexpr int kRows = 4;                      // rows a wave of the staging passes has in flight

typedef cgnn_columns<CGNN_NUM_PAGERANK_MEASURES> Columns;

// bytes in front of the entries; a multiple of 4
inline size_t fixed_bytes(int n) {
  return sizeof(double) * ((size_t)kVectors * n + kScratch + kRed) + sizeof(int32_t) * ((size_t)n + 1);
}
// what a launch asks for: room for every off-diagonal entry where that fits, else everything
inline size_t lds_of(int n) {
  const size_t all = fixed_bytes(n) + 6 * (size_t)n * (n - 1) + 4;
  return all < (size_t)kLdsBytes ? all : (size_t)kLdsBytes;
}

struct Params {
  double d, tol;                              // damping; (1 - d) 2^-42
  int kmax;
  int space;                                  // bytes of LDS behind the fixed part
};

// The sum of v over each aligned group of 8 lanes, on every lane of the group: the neighbour (quad_perm [1,0,3,2]), the
// other pair (quad_perm [2,3,0,1]), the other quad (row_half_mirror).  Needs every lane active.
__device__ __forceinline__ double group8_total(double v) {
  v = dpp_add<0xB1, 0xf>(v);
  v = dpp_add<0x4E, 0xf>(v);
  return dpp_add<0x141, 0xf>(v);
}

// (a, b) summed over the workgroup in a fixed order, on every thread; `red` is this call's half of the buffer
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red, int lane, int wave) {
  a = wave_total(a);
  b = wave_total(b);
  if (lane == 0) {
    red[2 * wave] = a;
    red[2 * wave + 1] = b;
  }
  __syncthreads();
  a = 0.0;
  b = 0.0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    a += red[2 * w];
    b += red[2 * w + 1];
  }
}

// The iteration of one measure of one subject; x holds the result after it.  Returns the number of steps.
template <bool kWeighted, bool kSparse>
__device__ int iterate(const float* __restrict__ A, int n, float thr, const Params& p, double* x, double* y0, double* y1,
                       const double* rc, double* red, const int32_t* rowptr, const uint16_t* ecol, const float* ewt) {
  constexpr int G = kSparse ? kSparseLanes : 64;
  constexpr int kGroups = kThreads / G;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = t / G, l = t % G;
  const double inv_n = 1.0 / (double)n, base = (1.0 - p.d) / (double)n;

  double unused = 0.0, dang = 0.0;
  for (int i = t; i < n; i += kThreads) {
    const double ri = rc[i];
    x[i] = inv_n;
    y0[i] = inv_n * ri;
    if (ri == 0.0) dang += inv_n;
  }
  block_sum2(unused, dang, red, lane, wave);  // (its barrier publishes x and y0)

  double* ycur = y0;
  double* ynext = y1;
  int steps = 0;
  for (int k = 1; k <= p.kmax; ++k) {
    double change = 0.0;
    for (int half = 0; half < 2; ++half) {     // a step is two products; x keeps the step's start until the second
      double dnext = 0.0;
      const double spread = dang * inv_n;
      for (int i0 = 0; i0 < n; i0 += kGroups) {
        const int i = i0 + g;
        double sum = 0.0;
        if (i < n) {
          if (kSparse) {
            const int end = rowptr[i + 1];
            for (int q = rowptr[i] + l; q < end; q += G)
              sum += (kWeighted ? (double)ewt[q] : 1.0) * ycur[ecol[q]];
          } else {
            const float* __restrict__ row = A + (int64_t)i * n;
            for (int j = l; j < n; j += G) {
              const float v = row[j];
              if (j != i && cgnn_kept(v, thr)) sum += (kWeighted ? (double)v : 1.0) * ycur[j];
            }
          }
        }
        sum = kSparse ? group8_total(sum) : wave_total(sum);
        if (i < n && l == 0) {
          const double xn = p.d * (sum + spread) + base, ri = rc[i];
          if (half) {
            change += fabs(xn - x[i]);
            x[i] = xn;
          }
          ynext[i] = xn * ri;
          if (ri == 0.0) dnext += xn;
        }
      }
      block_sum2(change, dnext, red + (1 - half) * 2 * kWaves, lane, wave);
      dang = dnext;
      double* s = ycur;
      ycur = ynext;
      ynext = s;
    }
    steps = k;
    if (change <= p.tol) break;               // (the same doubles on every thread)
  }
  return steps;
}

__global__ __launch_bounds__(kThreads) void k_pagerank(const float* __restrict__ matrices, int64_t S, int n,
                                                       const float* __restrict__ thr, Columns cols,
                                                       float* __restrict__ xout, int32_t* __restrict__ iterations,
                                                       Params p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double* x = reinterpret_cast<double*>(lds);                         // [n]
  double* y0 = x + n;                                                 // [n]
  double* y1 = y0 + n;                                                // [n]
  double* cw = y1 + n;                                                // [n] 1 / out-strength, 0 for a dangling node
  double* cb = cw + n;                                                // [n] 1 / out-degree, likewise
  double* scratch = cb + n;                                           // [kScratch]
  double* red = scratch + kScratch;                                   // [kRed]
  int32_t* rowptr = reinterpret_cast<int32_t*>(red + kRed);           // [n + 1]
  unsigned char* entries = reinterpret_cast<unsigned char*>(rowptr + n + 1);

  const int npad64 = (n + 63) & ~63;
  const int npad = npad64 < kThreads ? npad64 : kThreads;             // columns a slice of threads covers at a time
  const int slices = kThreads / npad;                                 // (1 for n > 256)
  const int chunk = (n + slices - 1) / slices;                        // rows of a slice

  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const float thr_s = thr[s];
    const float* __restrict__ A = matrices + s * n * (int64_t)n;

    // ---- the column sums ----
    bool bad = false;                                                 // a c_j that is not finite
    {
      const int sl = t / npad, j0 = t - sl * npad;
      if (sl < slices) {
        const int r0 = sl * chunk, r1 = r0 + chunk < n ? r0 + chunk : n;
        for (int j = j0; j < n; j += npad) {
          double sw = 0.0, sb = 0.0;
          const float* __restrict__ colp = A + j;
          int i = r0;
          for (; i + kBatch <= r1; i += kBatch) {                     // kBatch loads in flight, added in row order
            float v[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) v[u] = colp[(int64_t)(i + u) * n];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
              if (i + u != j && cgnn_kept(v[u], thr_s)) {
                sw += (double)v[u];
                sb += 1.0;
              }
            }
          }
          for (; i < r1; ++i) {
            const float v = colp[(int64_t)i * n];
            if (i != j && cgnn_kept(v, thr_s)) {
              sw += (double)v;
              sb += 1.0;
            }
          }
          if (slices == 1) {
            cw[j] = sw > 0.0 ? 1.0 / sw : 0.0;
            cb[j] = sb > 0.0 ? 1.0 / sb : 0.0;
            bad |= !(sw <= 1.7976931348623157e308);
          } else {
            scratch[sl * n + j] = sw;                                 // (slices * n <= kThreads)
            scratch[kThreads + sl * n + j] = sb;
          }
        }
      }
      if (slices > 1) {
        __syncthreads();
        if (t < n) {
          double sw = 0.0, sb = 0.0;
          for (int q = 0; q < slices; ++q) {
            sw += scratch[q * n + t];
            sb += scratch[kThreads + q * n + t];
          }
          cw[t] = sw > 0.0 ? 1.0 / sw : 0.0;
          cb[t] = sb > 0.0 ? 1.0 / sb : 0.0;
          bad |= !(sw <= 1.7976931348623157e308);
        }
      }
    }
    int32_t* flags = reinterpret_cast<int32_t*>(red);                 // (free until the first iteration)
    const bool wave_bad = __ballot(bad) != 0ull;
    if (lane == 0) flags[wave] = wave_bad;
    __syncthreads();                                                  // (publishes cw and cb)
    bool nonfinite = false;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) nonfinite |= flags[w] != 0;

    // ---- the rows' counts and offsets ----
    for (int i0 = wave * kRows; i0 < n; i0 += kWaves * kRows) {       // a wave takes kRows rows at a time
      int cnt[kRows] = {};
      for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        float v[kRows];
#pragma unroll
        for (int u = 0; u < kRows; ++u) v[u] = i0 + u < n && j < n ? A[(int64_t)(i0 + u) * n + j] : -INFINITY;
#pragma unroll
        for (int u = 0; u < kRows; ++u) cnt[u] += __popcll(__ballot(j != i0 + u && cgnn_kept(v[u], thr_s)));
      }
#pragma unroll
      for (int u = 0; u < kRows; ++u)
        if (lane == 0 && i0 + u < n) rowptr[i0 + u + 1] = cnt[u];
    }
    __syncthreads();
    if (wave == 0) {
      int carry = 0;
      for (int b = 0; b < n; b += 64) {
        const int i = b + lane;
        int v = i < n ? rowptr[i + 1] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int u = __shfl_up(v, o, 64);
          if (lane >= o) v += u;
        }
        if (i < n) rowptr[i + 1] = carry + v;
        carry += __shfl(v, 63, 64);
      }
      if (lane == 0) rowptr[0] = 0;
    }
    __syncthreads();
    const int E = rowptr[n];
    const int wt_at = (2 * E + 3) & ~3;                               // where the weights start
    const bool cols_fit = 2 * (int64_t)E <= p.space, all_fit = wt_at + 4 * (int64_t)E <= p.space;
    uint16_t* ecol = reinterpret_cast<uint16_t*>(entries);
    float* ewt = reinterpret_cast<float*>(entries + wt_at);

    // ---- the kept entries, behind their rows' offsets ----
    if (E > 0 && cols_fit) {
      const uint64_t below = (1ull << lane) - 1ull;
      for (int i0 = wave * kRows; i0 < n; i0 += kWaves * kRows) {
        int at[kRows];
#pragma unroll
        for (int u = 0; u < kRows; ++u) at[u] = i0 + u < n ? rowptr[i0 + u] : 0;
        for (int j0 = 0; j0 < n; j0 += 64) {
          const int j = j0 + lane;
          float v[kRows];
#pragma unroll
          for (int u = 0; u < kRows; ++u) v[u] = i0 + u < n && j < n ? A[(int64_t)(i0 + u) * n + j] : -INFINITY;
#pragma unroll
          for (int u = 0; u < kRows; ++u) {
            const bool kept = j != i0 + u && cgnn_kept(v[u], thr_s);
            const uint64_t m = __ballot(kept);
            if (kept) {
              const int q = at[u] + __popcll(m & below);
              ecol[q] = (uint16_t)j;
              if (all_fit) ewt[q] = v[u];
            }
            at[u] += __popcll(m);
          }
        }
      }
    }
    __syncthreads();

    // ---- the measures ----
    int slowest = 0;
    for (int kind = 0; kind < 2; ++kind) {                            // 0: binary, 1: weighted
      const int col = cols.col[kind ? CGNN_PAGERANK_WEIGHTED : CGNN_PAGERANK];
      if (col < 0) continue;
      float* __restrict__ o = xout + s * n * (int64_t)cols.ldx + col;
      if (E == 0 || (kind && nonfinite)) {                            // no edge: 1 / n; a kept +inf: NaN
        const float v = E == 0 ? (float)(1.0 / (double)n) : __int_as_float(0x7fc00000);
        for (int i = t; i < n; i += kThreads) o[(int64_t)i * cols.ldx] = v;
        if (E == 0 && slowest < 1) slowest = 1;
        continue;
      }
      int steps;
      if (kind == 0) {
        steps = cols_fit ? iterate<false, true>(A, n, thr_s, p, x, y0, y1, cb, red, rowptr, ecol, ewt)
                         : iterate<false, false>(A, n, thr_s, p, x, y0, y1, cb, red, rowptr, ecol, ewt);
      } else {
        steps = all_fit ? iterate<true, true>(A, n, thr_s, p, x, y0, y1, cw, red, rowptr, ecol, ewt)
                        : iterate<true, false>(A, n, thr_s, p, x, y0, y1, cw, red, rowptr, ecol, ewt);
      }
      if (steps > slowest) slowest = steps;
      for (int i = t; i < n; i += kThreads) o[(int64_t)i * cols.ldx] = (float)x[i];
      __syncthreads();                        // the next iteration, or the next subject, overwrites x
    }
    if (iterations && t == 0) iterations[s] = slowest;
    __syncthreads();                         // the next subject's staging overwrites everything
  }
}

// (CGNN_OK, the columns) of a valid call: the cohort's size, then 1 or 2 distinct ids and, with_cols, their columns
int check(int64_t S, int32_t n, const int32_t* measures, int32_t num, const int32_t* cols, int32_t ldx, bool with_cols,
          Columns* c) {
  if (cgnn_check_cohort_upto(S, n, CGNN_PAGERANK_MAX_NODES) != CGNN_OK) return CGNN_EINVAL;
  return cgnn_check_request(measures, num, 1, cols, ldx, with_cols, c);
}

// K_max(d) = ceil(43 ln 2 / -ln d) + 2 steps of two products: d^(K - 2) <= 2^-43, so the change of step K, at most
// 2 (1 + d) d^(2 K - 1), meets the stopping rule for every d <= 0.99
int max_steps(double d) { return d > 0.0 ? (int)ceil(43.0 * log(2.0) / -log(d)) + 2 : 2; }

}  // namespace

extern "C" int64_t cgnn_ingest_pagerank_workspace_bytes(int64_t S, int32_t n, const int32_t* measures,
                                                        int32_t num_measures) {
  Columns c;
  if (check(S, n, measures, num_measures, nullptr, 0, false, &c) != CGNN_OK) return CGNN_EINVAL;
  return 0;                                   // the state of the one kernel is LDS
}

extern "C" int cgnn_ingest_pagerank(const float* matrices, int64_t S, int32_t n, const float* thr,
                                    const int32_t* measures, int32_t num_measures, const int32_t* cols, int32_t ldx,
                                    double damping, void* workspace, int64_t workspace_bytes, float* x, int64_t x_bytes,
                                    int32_t* iterations, int64_t iterations_bytes, void* stream) {
  Columns c;
  if (check(S, n, measures, num_measures, cols, ldx, true, &c) != CGNN_OK) return CGNN_EINVAL;
  if (!(damping >= 0.0 && damping <= CGNN_PAGERANK_MAX_DAMPING)) return CGNN_EINVAL;        // (a NaN fails both)
  if (cgnn_check_byte_counts(workspace, {workspace_bytes, x_bytes, iterations_bytes}) != CGNN_OK) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (cgnn_check_cohort_buffers(matrices, thr, workspace, x, x_bytes, true, S * n, c.ldx) != CGNN_OK) return CGNN_EINVAL;
  if (cgnn_misaligned({iterations}, 3)) return CGNN_EINVAL;
  if (iterations && iterations_bytes / (int64_t)sizeof(int32_t) < S) return CGNN_EINVAL;
  const size_t lds = lds_of(n);
  Params p;
  p.d = damping;
  p.tol = (1.0 - damping) * 0x1p-42;
  p.kmax = max_steps(damping);
  p.space = (int)(lds - fixed_bytes(n));
  if (lds > 64 * 1024 && !cgnn_raise_lds_limit<k_pagerank>(kLdsBytes)) return CGNN_ELAUNCH;
  const int grid = cgnn_grid_for(S, cgnn_wg_per_cu_by_lds(lds, kLdsBytes));
  k_pagerank<<<grid, kThreads, lds, cgnn_stream(stream)>>>(matrices, S, n, thr, c, x, iterations, p);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
