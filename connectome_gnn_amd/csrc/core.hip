// core.hip -- the core decomposition of a device-resident cohort of dense connectivity matrices (float [S, n, n]) at the
// thresholds of cgnn_ingest_select / cgnn_ingest_count (include/cgnn_core.h): cgnn_ingest_cores,
// cgnn_ingest_cores_workspace_bytes.
//
// Per subject with matrix A and threshold t: e_ij iff i != j, A_ij > t and A_ij > 0 (ingest_rows.h); nothing is
// symmetrised; rows are what is summed.  For the alive set H: k_i(H) = |{j in H: e_ij}|, s_i(H) = sum_{j in H, e_ij} A_ij.
// Peeling in rounds: L = max(L, min over alive u of p_u(alive)); every alive u with p_u(alive) <= L leaves together with
// value L and the round's number as its layer.  p = k: the k-core number and the onion layer; p = s: the s-core level.
//
//   k_cores   one launch; a workgroup of 8 waves owns a subject, grid stride.  Everything of a subject lives in LDS and
//             registers.
//     build   paths.hip's: a ballot per 64 columns of a row is a word of adj [n][nw], nw = ceil(n / 64) (16 KB at 360,
//             128 KB at 1024); a wave takes 4 rows at a time, four loads of each in flight.  A kept entry that is not
//             finite marks the subject: its s_coreness column is NaN and is not peeled.
//     entries (s_coreness only) pagerank.hip's: the rows' popcounts, scanned by wave 0 to row offsets (wave_ops.h);
//             E = the subject's kept entries.  If 6 E bytes (the columns rounded to 4) fit the space behind the offsets
//             a wave per row writes the kept columns (16-bit) and weights (float) behind the row's offset in ascending
//             column order, at the ranks the bitset's words give.  Else the peeling reads the kept entries from the
//             matrix rows (L2), found by the bitset.  The test depends on n and E alone.
//     peel    thread t owns row t, and row t + 512 above 512 nodes: wave w's ballot of "still alive" IS word w (and word
//             w + 8) of the alive mask, its ballot of "left in this round" that word of the removed mask.  A round:
//             the rows update p (k: minus the popcount of the row against the removed words, exact integers; s: a row
//             whose bitset meets the removed mask is summed AGAIN from 0.0 over its alive kept entries in ascending
//             column order, fp64 -- never a subtraction from a running sum; a row that does not meet it would add the
//             same terms in the same order and keeps its value; a byte per node beside the mask answers "is column j
//             alive" for the entries in LDS); the minimum over alive rows, in each wave by DPP,
//             then the 8 waves ascending, the same value on every thread; barrier; the rows at or below the level take
//             their value and layer and the ballots are written; barrier.  Two barriers a round.  The loop ends when the
//             minimum finds no alive row, which every thread sees alike, and after n rounds at the latest: a round
//             removes at least one node.
//             The binary and the weighted pass run one after the other off the same bitset.
// No atomics, and neither the order of any sum nor the assignment of work depends on the grid, the run or on which
// measures are asked for: the same bits on every run, for every grid and every request.  Element offsets into
// `matrices`, `x` and `levels` are 64-bit.
#include <float.h>
#include <limits.h>
#include <math.h>

#include <type_traits>

#include "ingest_rows.h"
#include "measure_request.h"
#include "wave_ops.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kLdsBytes = 160 * 1024;
constexpr int kMaxWords = CGNN_CORE_MAX_NODES / 64;   // words of the alive and the removed mask
constexpr int kOwned = CGNN_CORE_MAX_NODES / kThreads;   // rows a thread owns at the most
constexpr int kRed = 2 * kWaves;                      // doubles: a minimum and a maximum per wave
constexpr int kRows = 4;                              // rows a wave of the staging passes has in flight
constexpr int kLoads = 8;                             // entries of a row a thread loads before it adds them

typedef unsigned long long u64;
typedef cgnn_columns<CGNN_NUM_CORE_MEASURES> Columns;

enum { kCoreness = CGNN_CORE_CORENESS, kOnion = CGNN_CORE_ONION_LAYER, kScore = CGNN_CORE_S_CORENESS };

inline __host__ __device__ int words_of(int n) { return (n + 63) >> 6; }
// bytes in front of the entries; a multiple of 4
inline size_t fixed_bytes(int n) {
  return sizeof(u64) * ((size_t)n * words_of(n) + 2 * kMaxWords) + sizeof(double) * kRed +
         sizeof(int32_t) * (2 * kWaves + (size_t)n + 1) + (((size_t)n + 3) & ~(size_t)3);
}
// what a launch asks for: with s_coreness, room for every off-diagonal entry where that fits, else everything
inline size_t lds_of(int n, bool weighted) {
  const size_t fixed = fixed_bytes(n);
  if (!weighted) return fixed;
  const size_t all = fixed + 6 * (size_t)n * (n - 1) + 4;
  return all < (size_t)kLdsBytes ? all : (size_t)kLdsBytes;
}

// v moved across lanes by the DPP control kCtrl on the rows of kRows; a lane without a source, or in a row outside
// kRows, keeps its own v
template <int kCtrl, int kRows>
__device__ __forceinline__ int dpp_or_own(int v) {
  return __builtin_amdgcn_update_dpp(v, v, kCtrl, kRows, 0xf, false);
}
template <int kCtrl, int kRows>
__device__ __forceinline__ double dpp_or_own(double v) {
  const int lo = dpp_or_own<kCtrl, kRows>(__double2loint(v)), hi = dpp_or_own<kCtrl, kRows>(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
template <bool kMax, typename T>
__device__ __forceinline__ T pick(T a, T b) {
  return (kMax ? b > a : b < a) ? b : a;
}
// The minimum (kMax: the maximum) of v over the 64 lanes, on every lane, in registers: wave_ops.h's scan with the sum
// replaced (row_shr 1, 2, 4, 8, then row_bcast:15 and row_bcast:31), its last lane read back.  Needs every lane active.
template <bool kMax, typename T>
__device__ __forceinline__ T wave_extreme(T v) {
  v = pick<kMax>(v, dpp_or_own<0x111, 0xf>(v));
  v = pick<kMax>(v, dpp_or_own<0x112, 0xf>(v));
  v = pick<kMax>(v, dpp_or_own<0x114, 0xf>(v));
  v = pick<kMax>(v, dpp_or_own<0x118, 0xf>(v));
  v = pick<kMax>(v, dpp_or_own<0x142, 0xa>(v));
  return pick<kMax>(v, dpp_or_own<0x143, 0xc>(v));
}
__device__ __forceinline__ int wave_min(int v) { return __builtin_amdgcn_readlane(wave_extreme<false>(v), 63); }
__device__ __forceinline__ double last_lane(double v) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63),
                          __builtin_amdgcn_readlane(__double2loint(v), 63));
}
__device__ __forceinline__ double wave_min(double v) { return last_lane(wave_extreme<false>(v)); }
__device__ __forceinline__ double wave_max(double v) { return last_lane(wave_extreme<true>(v)); }
// the minimum over no row
__device__ __forceinline__ int none_of(int) { return INT_MAX; }
__device__ __forceinline__ double none_of(double) { return INFINITY; }

// What a subject's staging left in LDS.
struct Staged {
  const u64* adj;                             // [n][nw]
  u64* alive;                                 // [kMaxWords]
  u64* removed;                               // [kMaxWords]
  double* redd;                               // [kRed]
  int32_t* redi;                              // [kWaves]
  const int32_t* rowptr;                      // [n + 1], s_coreness only
  uint8_t* alive8;                            // [n] 1 while the node is alive, s_coreness only
  const uint16_t* ecol;                       // the kept columns behind rowptr, when they fit
  const float* ewt;                           // their weights
  bool fits;
};

// s_u(alive): from 0.0, the kept entries of row u at alive columns in ascending column order.  A removed neighbour adds
// +0.0, which changes no bit of a sum that is never negative.
// From LDS: the row's compacted entries, one after the other; the columns and weights of kLoads entries are loaded, then
// their columns' alive bytes, then they are added: two LDS round trips for kLoads entries instead of two for each.
__device__ __forceinline__ double row_sum_lds(const Staged& st, int at, int end) {
  const uint16_t* __restrict__ ecol = st.ecol;
  const float* __restrict__ ewt = st.ewt;
  const uint8_t* __restrict__ alive8 = st.alive8;
  double sum = 0.0;
  for (int q0 = at; q0 < end; q0 += kLoads) {
    int col[kLoads];
    float v[kLoads];
    bool on[kLoads];
#pragma unroll
    for (int e = 0; e < kLoads; ++e) {        // (a slot past the row's end reads its last entry again and adds +0.0)
      const int q = q0 + e < end ? q0 + e : end - 1;
      col[e] = ecol[q];
      v[e] = ewt[q];
    }
#pragma unroll
    for (int e = 0; e < kLoads; ++e) on[e] = alive8[col[e]] != 0 && q0 + e < end;
#pragma unroll
    for (int e = 0; e < kLoads; ++e) sum += on[e] ? (double)v[e] : 0.0;
  }
  return sum;
}
// From the matrix row: kLoads alive entries of a word of the bitset are located and loaded before they are added.
__device__ __forceinline__ double row_sum_matrix(const float* __restrict__ row, const u64* __restrict__ bits, int nw,
                                                 const Staged& st) {
  double sum = 0.0;
  for (int w = 0; w < nw; ++w) {
    u64 live = bits[w] & st.alive[w];
    while (live) {
      float v[kLoads];
#pragma unroll
      for (int e = 0; e < kLoads; ++e) {
        const bool on = live != 0;
        const int b = on ? __builtin_ctzll(live) : 0;
        live &= live - 1;                     // (0 stays 0)
        v[e] = on ? row[(w << 6) + b] : 0.0f;
      }
#pragma unroll
      for (int e = 0; e < kLoads; ++e) sum += (double)v[e];
    }
  }
  return sum;
}

// The peeling of one subject for p = k (int) or p = s (double).  Of row t + h * kThreads: val[h] is the core value,
// layer[h] the round it left in.  top: max_i s_i(all) (kWeighted).  Ends behind a barrier.
template <bool kWeighted>
__device__ void peel(const float* __restrict__ A, int n, int nw, const Staged& st,
                     typename std::conditional<kWeighted, double, int>::type (&val)[kOwned], int (&layer)[kOwned],
                     double& top) {
  typedef typename std::conditional<kWeighted, double, int>::type T;
  const T kNone = none_of(T());
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  bool al[kOwned];
  T p[kOwned];
#pragma unroll
  for (int h = 0; h < kOwned; ++h) {
    const int u = t + h * kThreads, word = wave + h * kWaves;
    al[h] = u < n;
    p[h] = 0;
    val[h] = 0;
    layer[h] = 0;
    const u64 m = __ballot(al[h]);
    if (lane == 0 && word < nw) st.alive[word] = m;
    if (kWeighted && al[h]) st.alive8[u] = 1;
    if (!kWeighted && al[h]) {
      int k = 0;
      for (int w = 0; w < nw; ++w) k += __popcll(st.adj[u * nw + w]);
      p[h] = (T)k;
    }
  }
  __syncthreads();

  T level = 0;
  top = 0.0;
  for (int round = 1; round <= n; ++round) {   // (a round removes at least one node: n bounds them whatever the masks hold)
    T m = kNone;
#pragma unroll
    for (int h = 0; h < kOwned; ++h) {
      if (!al[h]) continue;
      const int u = t + h * kThreads;
      const u64* __restrict__ bits = st.adj + u * nw;
      if (kWeighted) {
        bool touched = round == 1;
        for (int w = 0; w < nw && !touched; ++w) touched = (bits[w] & st.removed[w]) != 0;
        if (touched)
          p[h] = (T)(st.fits ? row_sum_lds(st, st.rowptr[u], st.rowptr[u + 1])
                             : row_sum_matrix(A + (int64_t)u * n, bits, nw, st));
      } else if (round > 1) {
        int gone = 0;
        for (int w = 0; w < nw; ++w) {
          const u64 r = st.removed[w];
          if (r) gone += __popcll(bits[w] & r);
        }
        p[h] -= (T)gone;
      }
      m = p[h] < m ? p[h] : m;
    }
    m = wave_min(m);
    if (kWeighted) {
      if (round == 1) {                       // every row is alive: p is s_i(all)
        double mx = 0.0;
#pragma unroll
        for (int h = 0; h < kOwned; ++h)
          if (al[h] && (double)p[h] > mx) mx = (double)p[h];
        mx = wave_max(mx);
        if (lane == 0) st.redd[kWaves + wave] = mx;
      }
      if (lane == 0) st.redd[wave] = (double)m;
    } else if (lane == 0) {
      st.redi[wave] = (int)m;
    }
    __syncthreads();
    m = kNone;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const T v = kWeighted ? (T)st.redd[w] : (T)st.redi[w];
      m = v < m ? v : m;
    }
    if (kWeighted && round == 1) {
#pragma unroll
      for (int w = 0; w < kWaves; ++w) top = st.redd[kWaves + w] > top ? st.redd[kWaves + w] : top;
    }
    if (m == kNone) break;                    // no row is alive (the same value on every thread)
    level = m > level ? m : level;
#pragma unroll
    for (int h = 0; h < kOwned; ++h) {
      const int word = wave + h * kWaves;
      const bool gone = al[h] && p[h] <= level;
      if (gone) {
        val[h] = level;
        layer[h] = round;
        al[h] = false;
        if (kWeighted) st.alive8[t + h * kThreads] = 0;
      }
      const u64 a = __ballot(al[h]), g = __ballot(gone);
      if (lane == 0 && word < nw) {
        st.alive[word] = a;
        st.removed[word] = g;
      }
    }
    __syncthreads();
  }
  __syncthreads();                            // the reductions' slots are free again
}

__global__ __launch_bounds__(kThreads) void k_cores(const float* __restrict__ matrices, int64_t S, int n,
                                                    const float* __restrict__ thr, Columns cols,
                                                    float* __restrict__ xout, int32_t* __restrict__ levels, int space) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nw = words_of(n);
  u64* __restrict__ adj = reinterpret_cast<u64*>(lds);                // [n][nw]
  u64* alive = adj + n * nw;                                          // [kMaxWords]
  u64* removed = alive + kMaxWords;                                   // [kMaxWords]
  double* redd = reinterpret_cast<double*>(removed + kMaxWords);      // [kRed]
  int32_t* redi = reinterpret_cast<int32_t*>(redd + kRed);            // [kWaves]
  int32_t* flags = redi + kWaves;                                     // [kWaves]
  int32_t* rowptr = flags + kWaves;                                   // [n + 1]
  uint8_t* alive8 = reinterpret_cast<uint8_t*>(rowptr + n + 1);       // [n], rounded up to 4
  unsigned char* entries = alive8 + ((n + 3) & ~3);                   // [space]
  const bool binary = cols.col[kCoreness] >= 0 || cols.col[kOnion] >= 0;
  const bool weighted = cols.col[kScore] >= 0;

  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const float* __restrict__ A = matrices + s * (int64_t)n * n;
    float* __restrict__ xs = xout + s * (int64_t)n * cols.ldx;
    int32_t* __restrict__ ls = levels ? levels + s * (int64_t)n * 3 : nullptr;
    const float thr_s = thr[s];

    // ---- build: adj[i][c] bit l <=> e_{i, 64 c + l} ----
    bool bad = false;                                                 // a kept entry that is not finite
    for (int i0 = wave * kRows; i0 < n; i0 += kWaves * kRows) {       // a wave takes kRows rows at a time
      u64 mine[kRows] = {};
      for (int c0 = 0; c0 < nw; c0 += 4) {
        float v[kRows][4];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int col = ((c0 + e) << 6) + lane;
            v[r][e] = i0 + r < n && col < n ? A[(int64_t)(i0 + r) * n + col] : -INFINITY;
          }
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int col = ((c0 + e) << 6) + lane;
            const bool kept = col != i0 + r && cgnn_kept(v[r][e], thr_s);
            bad |= kept && !(v[r][e] <= FLT_MAX);
            const u64 word = __ballot(kept);
            if (lane == c0 + e) mine[r] = word;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < kRows; ++r)
        if (i0 + r < n && lane < nw) adj[(i0 + r) * nw + lane] = mine[r];
    }
    const bool wave_bad = __ballot(bad) != 0ull;
    if (lane == 0) flags[wave] = wave_bad;
    __syncthreads();

    Staged st = {adj, alive, removed, redd, redi, rowptr, alive8, nullptr, nullptr, false};

    // ---- the binary pass ----
    if (binary) {
      int val[kOwned], layer[kOwned];
      double unused;
      peel<false>(A, n, nw, st, val, layer, unused);
#pragma unroll
      for (int h = 0; h < kOwned; ++h) {
        const int u = t + h * kThreads;
        if (u >= n) continue;
        float* __restrict__ o = xs + (int64_t)u * cols.ldx;
        if (cols.col[kCoreness] >= 0) o[cols.col[kCoreness]] = n > 1 ? (float)val[h] / (float)(n - 1) : 0.0f;
        if (cols.col[kOnion] >= 0) o[cols.col[kOnion]] = (float)layer[h] / (float)n;
        if (ls) {
          ls[(int64_t)u * 3] = val[h];
          ls[(int64_t)u * 3 + 1] = layer[h];
        }
      }
    } else if (ls) {
      for (int u = t; u < n; u += kThreads) {
        ls[(int64_t)u * 3] = -1;
        ls[(int64_t)u * 3 + 1] = -1;
      }
    }

    // ---- the weighted pass ----
    if (weighted) {
      bool nonfinite = false;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) nonfinite |= flags[w] != 0;
      float* __restrict__ o = xs + cols.col[kScore];
      if (nonfinite) {
        for (int u = t; u < n; u += kThreads) {
          o[(int64_t)u * cols.ldx] = __int_as_float(0x7fc00000);
          if (ls) ls[(int64_t)u * 3 + 2] = -1;
        }
      } else {
        // the rows' counts and offsets
        for (int u = t; u < n; u += kThreads) {
          int k = 0;
          for (int w = 0; w < nw; ++w) k += __popcll(adj[u * nw + w]);
          rowptr[u + 1] = k;
        }
        __syncthreads();
        if (wave == 0) {
          int carry = 0;
          for (int b = 0; b < n; b += 64) {
            const int i = b + lane;
            const int v = wave_scan(i < n ? rowptr[i + 1] : 0);
            if (i < n) rowptr[i + 1] = carry + v;
            carry += __builtin_amdgcn_readlane(v, 63);
          }
          if (lane == 0) rowptr[0] = 0;
        }
        __syncthreads();
        const int E = rowptr[n];
        const int wt_at = (2 * E + 3) & ~3;                           // where the weights start
        st.fits = wt_at + 4 * (int64_t)E <= (int64_t)space;
        uint16_t* ecol = reinterpret_cast<uint16_t*>(entries);
        float* ewt = reinterpret_cast<float*>(entries + wt_at);
        st.ecol = ecol;
        st.ewt = ewt;
        // the kept weights, behind their rows' offsets: the q-th set bit of a row owns the q-th float
        if (st.fits && E > 0) {
          const u64 below = (1ull << lane) - 1ull;
          for (int i = wave; i < n; i += kWaves) {
            const float* __restrict__ row = A + (int64_t)i * n;
            int at = rowptr[i];
            for (int c0 = 0; c0 < nw; c0 += 4) {                      // four loads of a row in flight, as in the build
              u64 word[4];
              float v[4];
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                word[e] = c0 + e < nw ? adj[i * nw + c0 + e] : 0ull;
                v[e] = (word[e] >> lane) & 1ull ? row[((c0 + e) << 6) + lane] : 0.0f;
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                if ((word[e] >> lane) & 1ull) {
                  const int q = at + __popcll(word[e] & below);
                  ecol[q] = (uint16_t)(((c0 + e) << 6) + lane);
                  ewt[q] = v[e];
                }
                at += __popcll(word[e]);
              }
            }
          }
        }
        __syncthreads();

        double val[kOwned], top;
        int layer[kOwned];
        peel<true>(A, n, nw, st, val, layer, top);
        const double scale = top + 1e-8;
#pragma unroll
        for (int h = 0; h < kOwned; ++h) {
          const int u = t + h * kThreads;
          if (u >= n) continue;
          o[(int64_t)u * cols.ldx] = (float)(val[h] / scale);
          if (ls) ls[(int64_t)u * 3 + 2] = layer[h];
        }
      }
    } else if (ls) {
      for (int u = t; u < n; u += kThreads) ls[(int64_t)u * 3 + 2] = -1;
    }
    __syncthreads();                          // the next subject's build overwrites adj and the flags
  }
}

// (CGNN_OK, the columns) of a valid call: the cohort's size, then 1 to 3 distinct ids and, with_cols, their columns
int check(int64_t S, int32_t n, const int32_t* measures, int32_t num, const int32_t* cols, int32_t ldx, bool with_cols,
          Columns* c) {
  if (cgnn_check_cohort_upto(S, n, CGNN_CORE_MAX_NODES) != CGNN_OK) return CGNN_EINVAL;
  return cgnn_check_request(measures, num, 1, cols, ldx, with_cols, c);
}

}  // namespace

extern "C" int64_t cgnn_ingest_cores_workspace_bytes(int64_t S, int32_t n, const int32_t* measures,
                                                     int32_t num_measures) {
  Columns c;
  if (check(S, n, measures, num_measures, nullptr, 0, false, &c) != CGNN_OK) return CGNN_EINVAL;
  return 0;                                   // the state of the one kernel is LDS and registers
}

extern "C" int cgnn_ingest_cores(const float* matrices, int64_t S, int32_t n, const float* thr, const int32_t* measures,
                                 int32_t num_measures, const int32_t* cols, int32_t ldx, void* workspace,
                                 int64_t workspace_bytes, float* x, int64_t x_bytes, int32_t* levels,
                                 int64_t levels_bytes, void* stream) {
  Columns c;
  if (check(S, n, measures, num_measures, cols, ldx, true, &c) != CGNN_OK) return CGNN_EINVAL;
  if (cgnn_check_byte_counts(workspace, {workspace_bytes, x_bytes, levels_bytes}) != CGNN_OK) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (cgnn_check_cohort_buffers(matrices, thr, workspace, x, x_bytes, true, S * n, c.ldx) != CGNN_OK) return CGNN_EINVAL;
  if (cgnn_misaligned({levels}, 3)) return CGNN_EINVAL;
  if (levels && levels_bytes / (int64_t)sizeof(int32_t) / 3 < S * n) return CGNN_EINVAL;
  const size_t lds = lds_of(n, c.col[kScore] >= 0);
  if (lds > (size_t)kLdsBytes) return CGNN_EINVAL;            // (n <= CGNN_CORE_MAX_NODES fits: 133 KB at 1024)
  if (lds > 64 * 1024 && !cgnn_raise_lds_limit<k_cores>(kLdsBytes)) return CGNN_ELAUNCH;
  const int grid = cgnn_grid_for(S, cgnn_wg_per_cu_by_lds(lds, kLdsBytes));
  k_cores<<<grid, kThreads, lds, cgnn_stream(stream)>>>(matrices, S, n, thr, c, x, levels, (int)(lds - fixed_bytes(n)));
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
