// paths.hip -- shortest-path node measures of a device-resident cohort of dense connectivity matrices
// (float [S, n, n]) at the thresholds of cgnn_ingest_select / cgnn_ingest_count:
// cgnn_ingest_paths, cgnn_ingest_paths_workspace_bytes.
//
// Per subject with matrix A and threshold t: e_ij iff i != j, A_ij > t and A_ij > 0 (ingest_rows.h); nothing is
// symmetrised.  d_ij = edges on a shortest directed path i -> j along kept edges (out-neighbours of a row), infinite
// without one; R_i = { j != i : d_ij finite }, r_i = |R_i|; N_i = { j : e_ij }, k_i = |N_i|; d^(i) = distances in the
// subgraph induced on N_i.
//   nodal_efficiency  (1 / (n - 1)) sum_{j in R_i} 1 / d_ij                               (0 for n == 1)
//   closeness         (r_i / (n - 1)) (r_i / sum_{j in R_i} d_ij)                         (0 for r_i == 0)
//   eccentricity      max_{j in R_i} d_ij / (n - 1)                                       (0 for r_i == 0 or n == 1)
//   local_efficiency  (1 / (k_i (k_i - 1))) sum_{j != h in N_i} 1 / d^(i)_jh              (0 for k_i < 2)
//
//   k_paths   one launch.  A workgroup of 8 waves owns a subject, grid stride.
//     build   a wave per row: lane l tests column 64 c + l, one ballot is the 64-bit word c of the row's out-neighbour
//             bitset; adj [n][nw] words in LDS, nw = ceil(n / 64) (16 KB at 360, 128 KB at 1024).  Four loads of a row
//             are in flight per wave.  (A ballot over 4-byte lanes yields the word in column order; 16-byte lanes would
//             yield four words of every fourth column.)
//     bfs     a GROUP of nwp = 2^ceil(log2 nw) consecutive lanes owns a source, lane w of the group word w of
//             `visited` and `frontier`: 64 / nwp sources per wave (8 at 360, 32 at 84, 4 at 1024).  Level by level:
//             the group's lanes pass the frontier words round (one shuffle per word), every lane ORs word w of adj[u]
//             for each u of the frontier -- consecutive lanes read consecutive words of a row -- then
//             next &= ~visited, the popcounts are summed over the group: the level's count.  Every node is expanded
//             once per source.  A wave leaves the loop when all its groups met an empty frontier.
//     global  sources i = 0 .. n - 1 over the 8 x 64 / nwp groups of the workgroup; the group writes node i's columns.
//     local   a wave per node i: the wave lists N_i in LDS (n x 2 bytes per wave).  64 / nwp < k_i <= 128: N_i is
//             renumbered 0 .. k - 1 in list order and its induced subgraph written as a bitset of its own, [k][kw]
//             words with kw = ceil(k / 64) (2 KB per wave; a ballot of "bit list[b] of row list[a]" per word), and the
//             same bfs runs on it with kw lanes a source: all of 64 neighbours at once, one per lane.  Otherwise (one
//             round of groups covers N_i, or k_i > 128) the groups take the sources j in N_i in list order on adj
//             itself, visited preset to ~N_i, which confines the bfs to edges with both ends in N_i.  Either way a
//             neighbour is expanded at most once per source: ~ n k^2 row reads per subject against n^2 for the global
//             pass -- this pass grows with the density.
// Arithmetic: level counts, r_i, sum d and the eccentricity are exact integers (sum d <= n (n - 1) / 2 < 2^24);
// eccentricity is one correctly rounded fp32 quotient of two of them; the other three are formed in fp64 from the
// integers (sum_l count_l / l in ascending l; local: per source, sources in list order per group, groups folded in
// lane order) and rounded to fp32 once.  No atomics, and no work assignment depends on the grid: the same bits on
// every run and for every grid.  Element offsets into `matrices` and `x` are 64-bit.
// The request (1 to 4 distinct ids, distinct columns below ldx), the cohort's size (n <= CGNN_PATH_MAX_NODES) and its
// buffers are checked by measure_request.h, which also holds the LDS rules of the launch.
#include <math.h>

#include "ingest_rows.h"
#include "measure_request.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kLdsBytes = 160 * 1024;
constexpr int kSubNodes = 128;                // a neighbourhood of up to 128 nodes is renumbered: 2 words a row,
constexpr int kSubWords = kSubNodes * 2;      // 2 KB of LDS per wave

typedef unsigned long long u64;

enum {
  kNodal = CGNN_PATH_NODAL_EFFICIENCY,
  kCloseness = CGNN_PATH_CLOSENESS,
  kEccentricity = CGNN_PATH_ECCENTRICITY,
  kLocal = CGNN_PATH_LOCAL_EFFICIENCY
};

typedef cgnn_columns<CGNN_NUM_PATH_MEASURES> Columns;

// words of a bitset row, and the entries of a wave's neighbour list (a multiple of 4: the lists stay 8-byte aligned)
inline __host__ __device__ int words_of(int n) { return (n + 63) >> 6; }
inline __host__ __device__ int list_stride(int n) { return (n + 3) & ~3; }
size_t lds_of(int n) {
  return ((size_t)n * words_of(n) + kWaves * kSubWords) * sizeof(u64) + (size_t)kWaves * list_stride(n) * sizeof(uint16_t);
}

struct Levels {
  int r, sum_d, ecc;                          // reached nodes, the sum of their distances, the largest distance
  double eff;                                 // sum_l count_l / l, ascending l
};

// One source per group of nwp lanes (gbase: the group's first lane, w: this lane's word).  A lane with w >= nw and a
// group without a source hold visited = ~0 and frontier = 0: they read nothing and count nothing.  `others` is the
// number of nodes besides the source: once all are reached the last level is not expanded (it could find nothing).
__device__ __forceinline__ Levels bfs(const u64* __restrict__ adj, int nw, int nwp, int gbase, int w, u64 visited,
                                      u64 frontier, int others) {
  Levels o = {0, 0, 0, 0.0};
  const bool real = w < nw;
  int level = 0;
  while (true) {
    u64 next = 0;
    for (int q = 0; q < nw; ++q) {
      u64 f = __shfl(frontier, gbase + q, 64);
      while (f) {
        const int u = (q << 6) + __builtin_ctzll(f);
        f &= f - 1;
        if (real) next |= adj[u * nw + w];
      }
    }
    next &= ~visited;
    int cnt = __popcll(next);
    for (int d = 1; d < nwp; d <<= 1) cnt += __shfl_xor(cnt, d, 64);
    if (!__any(cnt != 0)) break;
    ++level;
    visited |= next;
    frontier = next;
    if (cnt) {
      o.r += cnt;
      o.sum_d += level * cnt;
      o.ecc = level;
      o.eff += (double)cnt / (double)level;
      if (o.r == others) frontier = 0;
    }
  }
  return o;
}

__global__ __launch_bounds__(kThreads) void k_paths(const float* __restrict__ matrices, int64_t S, int n,
                                                    const float* __restrict__ thr, Columns cols,
                                                    float* __restrict__ x) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nw = words_of(n);
  int nwp = 1;
  while (nwp < nw) nwp <<= 1;
  const int groups = 64 / nwp;                // sources a wave runs at once
  const int g = lane / nwp, w = lane - g * nwp, gbase = g * nwp;
  u64* __restrict__ adj = reinterpret_cast<u64*>(lds);
  u64* __restrict__ sub = adj + n * nw + wave * kSubWords;
  uint16_t* __restrict__ list = reinterpret_cast<uint16_t*>(adj + n * nw + kWaves * kSubWords) + wave * list_stride(n);
  const bool global = cols.col[kNodal] >= 0 || cols.col[kCloseness] >= 0 || cols.col[kEccentricity] >= 0;
  const bool local = cols.col[kLocal] >= 0;

  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const float* __restrict__ A = matrices + s * (int64_t)n * n;
    float* __restrict__ xs = x + s * (int64_t)n * cols.ldx;
    const float thr_s = thr[s];

    // ---- build: adj[i][c] bit l <=> e_{i, 64 c + l} ----
    for (int i = wave; i < n; i += kWaves) {
      const float* __restrict__ row = A + (int64_t)i * n;
      u64 mine = 0;
      for (int c0 = 0; c0 < nw; c0 += 4) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = ((c0 + e) << 6) + lane;
          v[e] = col < n ? row[col] : -INFINITY;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = ((c0 + e) << 6) + lane;
          const u64 word = __ballot(col != i && cgnn_kept(v[e], thr_s));
          if (lane == c0 + e) mine = word;
        }
      }
      if (lane < nw) adj[i * nw + lane] = mine;
    }
    __syncthreads();

    // ---- global: a group per source ----
    if (global) {
      for (int base = 0; base < n; base += kWaves * groups) {
        const int i = base + wave * groups + g;
        const bool active = i < n;
        const u64 bit = active && w == (i >> 6) ? 1ull << (i & 63) : 0;
        const Levels L = bfs(adj, nw, nwp, gbase, w, active && w < nw ? bit : ~0ull, bit, n - 1);
        if (active && w == 0) {
          float* __restrict__ o = xs + (int64_t)i * cols.ldx;
          const double nm1 = (double)(n - 1);
          if (cols.col[kNodal] >= 0) o[cols.col[kNodal]] = n > 1 ? (float)(L.eff / nm1) : 0.0f;
          if (cols.col[kCloseness] >= 0)
            o[cols.col[kCloseness]] =
                L.r > 0 ? (float)(((double)L.r / nm1) * ((double)L.r / (double)L.sum_d)) : 0.0f;
          if (cols.col[kEccentricity] >= 0)
            o[cols.col[kEccentricity]] = n > 1 ? (float)L.ecc / (float)(n - 1) : 0.0f;
        }
      }
    }

    // ---- local: a wave per node, a group per source j in N_i ----
    if (local) {
      for (int i = wave; i < n; i += kWaves) {
        const u64 mask = w < nw ? adj[i * nw + w] : 0;
        // the wave's earlier reads of the list are done before it is rewritten, the writes before it is read
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        int k = 0;
        for (int q = 0; q < nw; ++q) {
          const u64 word = __shfl(mask, q, 64);           // lane q is lane w = q of group 0
          if ((word >> lane) & 1) list[k + __popcll(word & ((1ull << lane) - 1))] = (uint16_t)((q << 6) + lane);
          k += __popcll(word);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        double sum = 0.0;
        // Three forms, chosen by (k, n) alone.  Shapes of tests/test_gpu_paths.py that reach each:
        //   renumbered, 1 word  (groups < k <= 64):   recipe n = 360 keep 0.1 (k ~ 36, groups 8); cliques at 129, 130
        //                                             (k = 63, 64, groups 16); recipe 97 keep 0.5 (k ~ 48, groups 32);
        //                                             Watts-Strogatz at 1024 (k ~ 6, groups 4)
        //   renumbered, 2 words (64 < k <= 128):      recipe 84 and 97 keep 1.0; complete graph at 129 (k = 128)
        //   on adj, one round   (k <= groups):        every n <= 64; recipe 84 .. 130 keep 0.1; ring and path at 1024
        //   on adj, k > 128:                          complete graph at 130 (k = 129); recipe 130 keep 1.0
        if (k > groups && k <= kSubNodes) {
          // N_i renumbered 0 .. k - 1 in list order: sub[a][c] bit l <=> e_{list[a], list[64 c + l]}, kw = 1 or 2 words
          // a row, and kw lanes own a source: one round runs 64 / kw sources
          const int kw = (k + 63) >> 6;
          for (int c = 0; c < kw; ++c) {
            const int b = (c << 6) + lane;
            const int jb = b < k ? list[b] : 0;
#pragma unroll 4
            for (int a = 0; a < k; ++a) {
              const u64 word = __ballot(b < k && ((adj[list[a] * nw + (jb >> 6)] >> (jb & 63)) & 1));
              if (lane == 0) sub[a * kw + c] = word;
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          const int sg = lane / kw, sw = lane - sg * kw;
          const int valid = k - (sw << 6);                // nodes of word sw: the bits from `valid` on are no nodes
          const u64 none = valid >= 64 ? 0 : ~0ull << (valid > 0 ? valid : 0);
          for (int base = 0; base < k; base += 64 / kw) {
            const int a = base + sg;
            const bool active = a < k;
            const u64 bit = active && sw == (a >> 6) ? 1ull << (a & 63) : 0;
            const Levels L = bfs(sub, kw, kw, sg * kw, sw, active ? none | bit : ~0ull, bit, k - 1);
            sum += L.eff;
          }
          for (int d = kw; d < 64; d <<= 1) sum += __shfl_xor(sum, d, 64);
        } else if (k >= 2) {
          for (int base = 0; base < k; base += groups) {
            const int m = base + g;
            const bool active = m < k;
            const int j = active ? list[m] : 0;
            const u64 bit = active && w == (j >> 6) ? 1ull << (j & 63) : 0;
            const Levels L = bfs(adj, nw, nwp, gbase, w, active && w < nw ? ~mask | bit : ~0ull, bit, k - 1);
            sum += L.eff;
          }
          for (int d = nwp; d < 64; d <<= 1) sum += __shfl_xor(sum, d, 64);
        }
        if (lane == 0)
          xs[(int64_t)i * cols.ldx + cols.col[kLocal]] = k >= 2 ? (float)(sum / ((double)k * (double)(k - 1))) : 0.0f;
      }
    }
    __syncthreads();                          // the next subject's build overwrites adj
  }
}

// (CGNN_OK, the columns) of a valid call: the cohort's size, then 1 to 4 distinct ids and, with_cols, their columns
int check(int64_t S, int32_t n, const int32_t* measures, int32_t num, const int32_t* cols, int32_t ldx, bool with_cols,
          Columns* c) {
  if (cgnn_check_cohort_upto(S, n, CGNN_PATH_MAX_NODES) != CGNN_OK) return CGNN_EINVAL;
  return cgnn_check_request(measures, num, 1, cols, ldx, with_cols, c);
}

}  // namespace

extern "C" int64_t cgnn_ingest_paths_workspace_bytes(int64_t S, int32_t n, const int32_t* measures,
                                                     int32_t num_measures) {
  Columns c;
  if (check(S, n, measures, num_measures, nullptr, 0, false, &c) != CGNN_OK) return CGNN_EINVAL;
  return 0;                                   // the one kernel keeps its state in LDS and registers
}

extern "C" int cgnn_ingest_paths(const float* matrices, int64_t S, int32_t n, const float* thr,
                                 const int32_t* measures, int32_t num_measures, const int32_t* cols, int32_t ldx,
                                 void* workspace, int64_t workspace_bytes, float* x, int64_t x_bytes, void* stream) {
  Columns c;
  if (check(S, n, measures, num_measures, cols, ldx, true, &c) != CGNN_OK) return CGNN_EINVAL;
  if (workspace_bytes < 0 || (reinterpret_cast<uintptr_t>(workspace) & 15)) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (cgnn_check_cohort_buffers(matrices, thr, workspace, x, x_bytes, true, S * n, ldx) != CGNN_OK) return CGNN_EINVAL;
  const size_t lds = lds_of(n);
  if (lds > (size_t)kLdsBytes) return CGNN_EINVAL;            // (n <= CGNN_PATH_MAX_NODES fits: 160 KB at 1024)
  if (!cgnn_raise_lds_limit<k_paths>(kLdsBytes)) return CGNN_ELAUNCH;
  const int per_cu = cgnn_wg_per_cu_by_lds(lds, kLdsBytes);
  k_paths<<<cgnn_grid_for(S, per_cu), kThreads, lds, cgnn_stream(stream)>>>(matrices, S, n, thr, c, x);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
