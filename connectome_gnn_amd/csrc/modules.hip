// modules.hip -- module-aware node measures of a device-resident cohort of dense connectivity matrices (float [S, n, n])
// at the thresholds of cgnn_ingest_select / cgnn_ingest_count, for one partition of the ROIs into M modules (DESIGN.md
// 4.3q, include/cgnn_modules.h): cgnn_ingest_modules, cgnn_ingest_modules_workspace_bytes.
//
// Per subject with matrix A and threshold t: e_ij iff i != j, A_ij > t and A_ij > 0 (ingest_rows.h); nothing is
// symmetrised.  With c_j the module of column j: k_i(m) = |{ j : e_ij, c_j = m }|, s_i(m) = sum of those A_ij;
// k_i = sum_m k_i(m), s_i = sum_m s_i(m); kappa_i = k_i(c_i), sigma_i = s_i(c_i).
//
//   k_modules<R>  one launch; a workgroup of 8 waves owns a subject, grid stride.  R = ceil(n / 64) (rounded up to an
//                 instantiated value): lane l holds columns l, l + 64, .. of a row in registers, and their module ids
//                 beside them, loaded once per workgroup; the wave's next row is loaded while the current one is worked on.
//     rows      a wave per row.
//       k_i(m)  lane m owns module m: one ballot of the edge test per 64 columns, ANDed with the lane's own mask of
//               module m's columns (formed once per workgroup), popcounts.  Exact integers; no reduction.
//       s_i(m)  per-lane slots in the wave's own LDS, double [modules of the pass][65]: lane l adds its kept entries
//               to slot [c_j][l] in ascending j (its own slots: plain read-add-write, no atomic), then module q's 64
//               slots are summed by 64 / P lanes, P = the power of two >= min(M, 32): lane q + P p adds slots
//               p P .. p P + P - 1 in ascending order, and the parts are folded by a butterfly over the lane bits
//               above P.  The row stride of 65 doubles keeps both half waves of the read on 32 different pairs of
//               banks.  The lane then clears the slots it used.  M > 32 takes two passes of 32 modules (the slots of
//               eight waves at M = 64 would not fit LDS).  The total of module m ends in lane m.
//       row     k_i, s_i and the sums over m of the ratios are sums over the lanes (lanes >= M hold zeros), by a DPP
//               scan in registers (wave_total); participation, weighted participation and diversity are written by
//               lane 0, the profile entries by lanes 0 .. M - 1 (M consecutive floats), kappa_i and sigma_i go to LDS
//               as doubles.
//     z-scores  only if one is asked for: a workgroup barrier, then a wave per module: the members' sum, the test "all
//               compare equal to the first member", the squared deviations from the mean (lane l over nodes l, l + 64,
//               .. ascending, the lanes by the same scan; the member count and the first member are formed once per
//               workgroup); a barrier; a thread per node writes its z-score; a barrier before the next subject
//               overwrites kappa and sigma.
// Everything after the fp32 edge test is fp64 and is rounded to fp32 once.  No atomics anywhere, and neither the order
// of any sum nor the assignment of work depends on the grid, the run or the wave that took a row: the same bits on
// every run and for every grid.  Element offsets into `matrices`, `x` and `profile` are 64-bit.
// A module id outside [0, M) is SKIPPED: such a column belongs to no module (it adds to no k_i(m) or s_i(m), hence to
// neither k_i nor s_i), and a row whose own id is outside has kappa = sigma = 0 and z-scores 0.
#include <math.h>

#include "ingest_rows.h"
#include "measure_request.h"
#include "wave_ops.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kLdsBytes = 160 * 1024;
constexpr int kPass = 32;                     // modules whose slots a wave keeps at a time
constexpr int kSlotLd = 65;                   // doubles between two modules' slots
constexpr int kStat = 6;                      // doubles per module: (mean, deviation, all equal) of kappa, of sigma

enum {
  kPart = CGNN_MODULE_PARTICIPATION,
  kWPart = CGNN_MODULE_WEIGHTED_PARTICIPATION,
  kZ = CGNN_MODULE_ZSCORE,
  kWZ = CGNN_MODULE_WEIGHTED_ZSCORE,
  kDiversity = CGNN_MODULE_DIVERSITY
};

typedef cgnn_columns<CGNN_NUM_MODULE_MEASURES> Columns;

inline int pass_of(int M) { return M < kPass ? M : kPass; }
inline size_t lds_of(int n, int M) {
  return sizeof(double) * ((size_t)kWaves * pass_of(M) * kSlotLd + 2 * (size_t)n + kStat * (size_t)M) +
         sizeof(int32_t) * ((size_t)n + 2 * (size_t)M);
}

template <int R>
__global__ __launch_bounds__(kThreads) void k_modules(const float* __restrict__ matrices, int64_t S, int n,
                                                      const float* __restrict__ thr,
                                                      const int32_t* __restrict__ modules, int M, Columns cols,
                                                      float* __restrict__ x, float* __restrict__ profile, int flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int mpass = M < kPass ? M : kPass;
  int P = 1, lg = 0;                          // the power of two >= mpass, and its logarithm
  while (P < mpass) P <<= 1, ++lg;
  double* slots = reinterpret_cast<double*>(lds) + (size_t)wave * mpass * kSlotLd;   // the wave's own
  double* kappa = reinterpret_cast<double*>(lds) + (size_t)kWaves * mpass * kSlotLd;  // [n]
  double* sigma = kappa + n;                                                          // [n]
  double* stat = sigma + n;                                                           // [M][kStat]
  int32_t* cid = reinterpret_cast<int32_t*>(stat + kStat * M);                        // [n]: the id, -1 if outside
  int32_t* modinfo = cid + n;                                                         // [M][2]: members, the first one

  const bool binary = flags & CGNN_MODULE_PROFILE_BINARY, normalize = flags & CGNN_MODULE_PROFILE_NORMALIZE;
  const bool want_z[2] = {cols.col[kZ] >= 0, cols.col[kWZ] >= 0};
  const bool need_b = cols.col[kPart] >= 0 || want_z[0] || (profile && binary);
  const bool need_w = cols.col[kWPart] >= 0 || cols.col[kDiversity] >= 0 || want_z[1] || (profile && !binary);

  // ---- once per workgroup: the ids, the lane's columns' ids, lane m's masks of module m's columns, zero slots ----
  for (int i = t; i < n; i += kThreads) {
    const int32_t c = modules[i];
    cid[i] = c >= 0 && c < M ? c : -1;
  }
  for (int q = 0; q < mpass; ++q) slots[q * kSlotLd + lane] = 0.0;
  __syncthreads();
  if (want_z[0] || want_z[1]) {               // a module's member count and first member, read after a barrier
    for (int m = wave; m < M; m += kWaves) {
      int cnt = 0, first = -1;
      for (int i0 = 0; i0 < n; i0 += 64) {
        const uint64_t b = __ballot(i0 + lane < n && cid[i0 + lane] == m);
        if (first < 0 && b) first = i0 + __ffsll((unsigned long long)b) - 1;
        cnt += __popcll(b);
      }
      if (lane == 0) {
        modinfo[2 * m] = cnt;
        modinfo[2 * m + 1] = first;
      }
    }
  }
  int ids[R];
  uint64_t mm[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int j = lane + 64 * r;
    ids[r] = j < n ? cid[j] : -1;
    mm[r] = 0ull;
    if (need_b) {
      for (int m = 0; m < M; ++m) {
        const uint64_t b = __ballot(ids[r] == m);
        if (lane == m) mm[r] = b;
      }
    }
  }
  const int rq = lane & (P - 1), rpart = lane >> lg;                 // the read of the slots: module, part

  // the lane's entries of row i of subject s; columns >= n read as -inf (never kept)
  auto load_row = [&](int64_t s, int i, float (&dst)[R]) {
    const float* __restrict__ row = matrices + (s * n + i) * (int64_t)n;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = lane + 64 * r;
      dst[r] = j < n ? row[j] : -INFINITY;
    }
  };
  float next[R];                              // the wave's next row is loaded while the current one is worked on
  if ((int64_t)blockIdx.x < S && wave < n) load_row(blockIdx.x, wave, next);

  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const float thr_s = thr[s];

    for (int i = wave; i < n; i += kWaves) {
      float v[R];
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = next[r];
      if (i + kWaves < n) load_row(s, i + kWaves, next);
      else if (s + gridDim.x < S) load_row(s + gridDim.x, wave, next);       // (wave < n: this wave has rows)
      bool kept[R];
#pragma unroll
      for (int r = 0; r < R; ++r) kept[r] = lane + 64 * r != i && cgnn_kept(v[r], thr_s);

      int km = 0, k = 0;                                             // k_i(lane), k_i
      if (need_b) {
#pragma unroll
        for (int r = 0; r < R; ++r) km += __popcll(__ballot(kept[r]) & mm[r]);
        k = wave_total(km);
      }
      double sm = 0.0, ssum = 0.0;                                   // s_i(lane), s_i
      if (need_w) {
        for (int base = 0; base < M; base += kPass) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const unsigned q = (unsigned)(ids[r] - base);
            if (kept[r] && q < (unsigned)mpass) slots[q * kSlotLd + lane] += (double)v[r];
          }
          wave_lds_fence();
          double part = 0.0;
          if (rq < mpass && base + rq < M) {
            const double* p = slots + rq * kSlotLd + rpart * P;
            for (int j = 0; j < P; ++j) part += p[j];
          }
          for (int o = P; o < 64; o <<= 1) part += __shfl_xor(part, o, 64);
          wave_lds_fence();
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const unsigned q = (unsigned)(ids[r] - base);
            if (kept[r] && q < (unsigned)mpass) slots[q * kSlotLd + lane] = 0.0;
          }
          if (lane < M && lane >= base && lane < base + kPass) sm = part;   // module `lane` is base + rq here
        }
        ssum = wave_total(sm);
      }

      const int ci = cid[i];
      float* __restrict__ o = x ? x + (s * n + i) * (int64_t)cols.ldx : nullptr;
      if (cols.col[kPart] >= 0) {
        const double r = (double)km / (double)k;                     // (not used when k == 0)
        const double sq = wave_total(k > 0 ? r * r : 0.0);
        if (lane == 0) o[cols.col[kPart]] = k > 0 ? (float)(1.0 - sq) : 0.0f;
      }
      if (cols.col[kWPart] >= 0 || cols.col[kDiversity] >= 0) {
        const double p = lane < M ? sm / ssum : 0.0;                 // (not used when s == 0)
        if (cols.col[kWPart] >= 0) {
          const double sq = wave_total(p * p);
          if (lane == 0) o[cols.col[kWPart]] = ssum == 0.0 ? 0.0f : (float)(1.0 - sq);
        }
        if (cols.col[kDiversity] >= 0) {
          const bool zero = ssum == 0.0 || M == 1;
          const double h = wave_total(zero || p == 0.0 ? 0.0 : p * log(p));
          if (lane == 0) o[cols.col[kDiversity]] = zero ? 0.0f : (float)(-h / log((double)M));
        }
      }
      if (want_z[0] || want_z[1]) {
        const int src = cgnn_uniform(ci >= 0 ? ci : 0);
        const int kap = __builtin_amdgcn_readlane(km, src);
        const double sig = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(sm), src),
                                            __builtin_amdgcn_readlane(__double2loint(sm), src));
        if (lane == 0) {
          kappa[i] = ci >= 0 ? (double)kap : 0.0;
          sigma[i] = ci >= 0 ? sig : 0.0;
        }
      }
      if (profile && lane < M) {
        double val = binary ? (double)km : sm;
        if (normalize) {
          const double tot = binary ? (double)k : ssum;
          val = tot == 0.0 ? 0.0 : val / tot;
        }
        profile[(s * n + i) * (int64_t)M + lane] = (float)val;
      }
    }

    if (want_z[0] || want_z[1]) {
      __syncthreads();                        // every kappa and sigma of the subject is in LDS
      for (int m = wave; m < M; m += kWaves) {
        const int cnt = modinfo[2 * m], first = modinfo[2 * m + 1];
        if (cnt == 0) continue;               // (wave-uniform) a label without nodes: nobody reads its statistics
        for (int kind = 0; kind < 2; ++kind) {
          if (!want_z[kind]) continue;
          const double* val = kind ? sigma : kappa;
          const double f = val[first];
          double sum = 0.0;
          bool differs = false;
          for (int i = lane; i < n; i += 64) {
            if (cid[i] == m) {
              sum += val[i];
              differs |= !(val[i] == f);
            }
          }
          sum = wave_total(sum);
          const bool all_equal = __ballot(differs) == 0ull;
          const double mean = sum / (double)cnt;
          double ss = 0.0;
          for (int i = lane; i < n; i += 64) {
            if (cid[i] == m) {
              const double d = val[i] - mean;
              ss += d * d;
            }
          }
          ss = wave_total(ss);
          if (lane == 0) {
            stat[m * kStat + 3 * kind + 0] = mean;
            stat[m * kStat + 3 * kind + 1] = sqrt(ss / (double)cnt);
            stat[m * kStat + 3 * kind + 2] = all_equal ? 1.0 : 0.0;
          }
        }
      }
      __syncthreads();
      for (int i = t; i < n; i += kThreads) {
        const int c = cid[i];
        float* __restrict__ o = x + (s * n + i) * (int64_t)cols.ldx;
#pragma unroll
        for (int kind = 0; kind < 2; ++kind) {
          if (!want_z[kind]) continue;
          double z = 0.0;
          if (c >= 0 && stat[c * kStat + 3 * kind + 2] == 0.0) {
            const double val = kind ? sigma[i] : kappa[i];
            z = (val - stat[c * kStat + 3 * kind + 0]) / stat[c * kStat + 3 * kind + 1];
          }
          o[cols.col[kind ? kWZ : kZ]] = (float)z;
        }
      }
      __syncthreads();                        // the next subject's rows overwrite kappa and sigma
    }
  }
}

// (CGNN_OK, the columns) of a valid call: the cohort's size, then 0 to 5 distinct ids and, with_cols, their columns
int check(int64_t S, int32_t n, const int32_t* measures, int32_t num, const int32_t* cols, int32_t ldx, bool with_cols,
          Columns* c) {
  if (cgnn_check_cohort_upto(S, n, CGNN_MODULE_MAX_NODES) != CGNN_OK) return CGNN_EINVAL;
  return cgnn_check_request(measures, num, 0, cols, ldx, with_cols, c);
}

template <int R>
int launch(int grid, size_t lds, hipStream_t st, const float* matrices, int64_t S, int n, const float* thr,
           const int32_t* modules, int M, const Columns& c, float* x, float* profile, int flags) {
  if (lds > 64 * 1024 && !cgnn_raise_lds_limit<k_modules<R>>(kLdsBytes)) return CGNN_ELAUNCH;
  k_modules<R><<<grid, kThreads, lds, st>>>(matrices, S, n, thr, modules, M, c, x, profile, flags);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

}  // namespace

extern "C" int64_t cgnn_ingest_modules_workspace_bytes(int64_t S, int32_t n, const int32_t* measures,
                                                       int32_t num_measures) {
  Columns c;
  if (check(S, n, measures, num_measures, nullptr, 0, false, &c) != CGNN_OK) return CGNN_EINVAL;
  return 0;                                   // the state of the one kernel is registers and LDS
}

extern "C" int cgnn_ingest_modules(const float* matrices, int64_t S, int32_t n, const float* thr,
                                   const int32_t* modules, int32_t M, const int32_t* measures, int32_t num_measures,
                                   const int32_t* cols, int32_t ldx, void* workspace, int64_t workspace_bytes, float* x,
                                   int64_t x_bytes, float* profile, int64_t profile_bytes, int32_t profile_flags,
                                   void* stream) {
  Columns c;
  if (check(S, n, measures, num_measures, cols, ldx, true, &c) != CGNN_OK) return CGNN_EINVAL;
  if (M < 1 || M > CGNN_MODULE_MAX || M > n) return CGNN_EINVAL;
  if (profile_flags & ~(CGNN_MODULE_PROFILE_BINARY | CGNN_MODULE_PROFILE_NORMALIZE)) return CGNN_EINVAL;
  if (cgnn_check_byte_counts(workspace, {workspace_bytes, x_bytes, profile_bytes}) != CGNN_OK) return CGNN_EINVAL;
  if (num_measures == 0 && !profile) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  // x [S n][ldx] if measures are asked for, profile [S n][M] if given; one of the two
  if (!modules || cgnn_misaligned({modules}, 3)) return CGNN_EINVAL;
  if (cgnn_check_cohort_buffers(matrices, thr, workspace, x, x_bytes, num_measures > 0, S * n, c.ldx) != CGNN_OK ||
      cgnn_check_cohort_buffers(matrices, thr, workspace, profile, profile_bytes, profile != nullptr, S * n, M) !=
          CGNN_OK)
    return CGNN_EINVAL;
  const size_t lds = lds_of(n, M);
  if (lds > (size_t)kLdsBytes) return CGNN_EINVAL;            // (157184 bytes at n = 1024, M = 64: every valid call fits)
  const int grid = cgnn_grid_for(S, cgnn_wg_per_cu_by_lds(lds, kLdsBytes));
  hipStream_t st = cgnn_stream(stream);
  float* xs = num_measures > 0 ? x : nullptr;
  const int chunks = (n + 63) / 64;
#define CGNN_MODULES_LAUNCH(R) \
  return launch<R>(grid, lds, st, matrices, S, n, thr, modules, M, c, xs, profile, profile_flags)
  if (chunks <= 1) CGNN_MODULES_LAUNCH(1);
  if (chunks <= 2) CGNN_MODULES_LAUNCH(2);
  if (chunks <= 3) CGNN_MODULES_LAUNCH(3);
  if (chunks <= 4) CGNN_MODULES_LAUNCH(4);
  if (chunks <= 6) CGNN_MODULES_LAUNCH(6);
  if (chunks <= 8) CGNN_MODULES_LAUNCH(8);
  if (chunks <= 12) CGNN_MODULES_LAUNCH(12);
  CGNN_MODULES_LAUNCH(16);
#undef CGNN_MODULES_LAUNCH
}
