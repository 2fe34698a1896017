// partial.hip -- partial-correlation matrices of a device-resident cohort of correlation matrices (float [U, n, n] ->
// float [U, n, n], in place if asked): cgnn_ingest_partial, cgnn_ingest_partial_each (a shrinkage per
// unit, read on the device: DESIGN.md 4.3i), cgnn_ingest_partial_workspace_bytes.
//
// Per unit with matrix R, read from its UPPER triangle (i <= j) only: ROI i is excluded iff R_ii == 0 (the zero row
// and column k_corr writes for a constant column); C = (1 - a) R + a I over the others, a = shrinkage, and the
// identity on the excluded ones; P = C^-1; out_ij = -P_ij / sqrt(P_ii P_jj) clamped to [-1, 1], out_ii = 1, zero rows
// and columns (diagonal included) for the excluded ROIs, |.| if asked.  A unit whose factorisation meets a pivot
// that is not > 0 (a NaN is not), or a P_ii that is not finite and > 0, is all NaN; so is, with a shrinkage per unit,
// a unit whose own is not in [0, 1] (the kernel is its first reader).
//
//   k_partial   one launch.  A workgroup of 4 waves owns a unit, grid stride; its slab [npad][npad] fp32, npad = n
//               rounded up to the block of 32, is workgroup blockIdx.x's slice of the workspace (one slab per workgroup
//               of the launch, not per unit).  With C = U^T U (U upper) and W = U^-T (lower), P = W^T W.
//     build     the upper block triangle of the slab <- C (padding: the identity), the rest <- 0.  Every read of R
//               happens here, before the first write of `out`: the call works in place.
//     rounds    over the diagonal blocks K, npad / 32 of them, right-looking on the augmented matrix [C | I]: the
//               upper block triangle of the slab holds what is left of C, the strictly lower one what is left of I,
//               which ends as W (block row I of it is the identity's until round I: the diagonal blocks need no room).
//       1  the diagonal tile in LDS, 32 steps of the unblocked factorisation over all threads (a barrier a step);
//          1 / u_kk is formed in fp64 and rounded once; its strictly lower transpose L_KK stays in LDS.
//       2  block row K of [U | W]: a thread per column solves L_KK y = (the column of the slab, or of the identity in
//          block K) by forward substitution in registers, k ascending.  The row panel [32][npad] stays in LDS; its W
//          part (columns up to block K) goes back to the slab, over the dead diagonal tile too, and its squares are
//          added to the column's P_ii = sum_k W_ki^2 (fp64, in LDS).
//       3  the trailing update, a wave per 32 x 32 tile: [C | I][I, J] -= U[K, I]^T [U | W][K, J] for I > K and
//          J <= K or J >= I (W[K, J] is zero between), on v_mfma_f32_16x16x4_f32 with both fragments read from the
//          panel (the fragment form of gram_tile.h); the tile is the accumulator, read and written 16 bytes a lane,
//          and the wave's next tile is loaded before the current one is updated.
//     scales    d_i = 1 / sqrt(P_ii), P_ii summed in fp64, k ascending, rounded once; 0 for an excluded ROI.
//     product   P = W^T W on the tile walk of gram_tile.h over the unit's tile pairs, from row 96 bj on (W is zero
//               above its diagonal).  Stage: entries above the diagonal (what is left of C) become zeros, column i is
//               scaled by d_i.  Epilogue: 0 - acc, clamp, |.|, the diagonal, the mirror store: k_corr's.
// Storage and products are fp32, every sum k ascending.  No atomics, and no work assignment depends on the grid: the
// same bits on every run and for every grid.  The round counts are fixed: the call returns whatever R holds.
// Element offsets into `matrices`, `out` and the workspace are 64-bit.
#include <math.h>

#include "gram_tile.h"
#include "measure_request.h"

namespace {

using namespace gram;

constexpr int kB = 32;                        // block of the factorisation: one K-step of the matrix pipe
constexpr int kTileLd = kB + 1;               // row stride of the diagonal tile in LDS
constexpr int kPanelPad = 16;                 // the row panel's stride npad + 16 is 16 or 48 (mod 64): disjoint banks
constexpr int kMisc = 36;                     // 1 / u_kk [32], the failure flag, padding to 16 bytes
constexpr int kLdsBytes = 160 * 1024;
static_assert(kB == kKS && kTile % kB == 0, "a round is one K-step; a tile of the product starts on a block row");

inline int padded(int n) { return (n + kB - 1) / kB * kB; }
inline int64_t slab_bytes(int npad) { return (int64_t)npad * npad * (int64_t)sizeof(float); }
// P_ii fp64 [npad] | d [tiles * 96] | misc | diagonal tile | L_KK | the row panel or, after the rounds, the product's
// panels
inline size_t lds_of(int n) {
  const int npad = padded(n);
  const size_t panel = (size_t)kB * (npad + kPanelPad), product = sizeof(Panels) / sizeof(float);
  return npad * sizeof(double) +
         ((size_t)tiles_of(n) * kTile + kMisc + kB * kTileLd + kB * kB + (panel > product ? panel : product)) *
             sizeof(float);
}

template <bool kVecOut, bool kEach>
__global__ __launch_bounds__(kThreads, 2) void k_partial(const float* matrices, int64_t U, int n, double shrinkage,
                                                      const double* __restrict__ alphas, int absolute, float* slabs,
                                                      float* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int frow = lane >> 4, fcol = lane & 15;           // a lane's row and column in a fragment (gram_tile.h)
  const int npad = (n + kB - 1) / kB * kB, nb = npad / kB, ldp = npad + kPanelPad;
  const int nt = tiles_of(n), nd = nt * kTile;
  double* pii = reinterpret_cast<double*>(lds);           // [npad]     P_ii = sum_k W_ki^2 as the rounds go
  float* scale = reinterpret_cast<float*>(pii + npad);    // [nd]       d_i; until the scales: 0 excluded, 1 not
  float* rinv = scale + nd;                               // [kB]       1 / u_kk of the round
  int* bad = reinterpret_cast<int*>(rinv + kB);           //            the unit failed
  float* tile = rinv + kMisc;                             // [kB][kB+1] the diagonal tile, upper
  float* lkk = tile + kB * kTileLd;                       // [kB][kB]   L_KK[r][k] = u_kr, k < r
  float* panel = lkk + kB * kB;                           // [kB][ldp]  block row K of [U | W]
  Panels& prod = *reinterpret_cast<Panels*>(panel);
  float* D = slabs + (int64_t)blockIdx.x * npad * npad;

  for (int64_t u = blockIdx.x; u < U; u += gridDim.x) {
    const float* R = matrices + u * (int64_t)n * n;       // (may be `o`: not restrict)
    float* o = out + u * (int64_t)n * n;
    // the unit's own shrinkage, if there is one per unit: nobody has read it before now, so a value that is not in
    // [0, 1] (a NaN is not) is refused here, by the failure path's all-NaN matrix
    const double alpha = kEach ? alphas[u] : shrinkage;
    const float om = (float)(1.0 - alpha);
    if (kEach && !(alpha >= 0.0 && alpha <= 1.0)) {
      for (int64_t e = t; e < (int64_t)n * n; e += kThreads) o[e] = NAN;
      continue;                               // (uniform: the whole workgroup leaves, no LDS is touched)
    }

    // ---- build ----
    for (int i = t; i < nd; i += kThreads) scale[i] = i < n && R[(int64_t)i * n + i] != 0.0f ? 1.0f : 0.0f;
    for (int i = t; i < npad; i += kThreads) pii[i] = 0.0;
    if (t == 0) *bad = 0;
    __syncthreads();
    for (int i = wave; i < npad; i += kThreads / 64) {
      const bool in_i = i < n && scale[i < n ? i : 0] != 0.0f;
      for (int j = lane; j < npad; j += 64) {
        float v = 0.0f;
        if (j == i) {
          v = in_i ? (float)((1.0 - alpha) * (double)R[(int64_t)i * n + i] + alpha) : 1.0f;
        } else if (j > i && in_i && j < n && scale[j] != 0.0f) {
          v = om * R[(int64_t)i * n + j];
        }
        D[(int64_t)i * npad + j] = v;
      }
    }
    __syncthreads();

    // ---- rounds ----
    for (int K = 0; K < nb; ++K) {
      const int kb = K * kB;
      // 1: the diagonal tile
      for (int e = t; e < kB * kB; e += kThreads)
        tile[(e / kB) * kTileLd + e % kB] = D[(int64_t)(kb + e / kB) * npad + kb + e % kB];
      __syncthreads();
      for (int k = 0; k < kB; ++k) {
        // (row k is final after step k - 1; it is scaled as it is read, and for good when L_KK is formed)
        const float p = tile[k * kTileLd + k];
        const float ri = (float)(1.0 / sqrt((double)p));
        if (t == k) {
          rinv[k] = ri;
          if (!(p > 0.0f)) *bad = 1;
        }
        for (int e = t; e < kB * kB; e += kThreads) {
          const int i = e / kB, j = e % kB;
          if (k < i && i <= j) tile[i * kTileLd + j] -= (tile[k * kTileLd + i] * ri) * (tile[k * kTileLd + j] * ri);
        }
        __syncthreads();
      }
      for (int e = t; e < kB * kB; e += kThreads) {
        const int r = e / kB, k = e % kB;
        lkk[e] = k < r ? tile[k * kTileLd + r] * rinv[k] : 0.0f;
      }
      __syncthreads();

      // 2: block row K of [U | W], a thread per column
      for (int c = t; c < npad; c += kThreads) {
        const int cb = c / kB;
        // (a uniform row pointer and a 32-bit column: 32 rows cost scalar registers, not 64 vector ones)
        const unsigned cu = c;
        __builtin_assume(cu < 2048u);
        float* const rows = D + (int64_t)kb * npad;
        float y[kB];
#pragma unroll
        for (int r = 0; r < kB; ++r) y[r] = (rows + (int64_t)r * npad)[cu];
        if (cb == K) {
#pragma unroll
          for (int r = 0; r < kB; ++r) y[r] = r == c - kb ? 1.0f : 0.0f;
        }
#pragma unroll
        for (int r = 0; r < kB; ++r) {
          float s = y[r];
#pragma unroll
          for (int k = 0; k < r; ++k) s = fmaf(-lkk[r * kB + k], y[k], s);
          y[r] = s * rinv[r];
          __builtin_amdgcn_sched_barrier(0);  // (row r + 1 of L_KK is read when it is used, not 32 rows ahead)
        }
#pragma unroll
        for (int r = 0; r < kB; ++r) panel[r * ldp + c] = y[r];
        if (cb <= K) {
          // rows kb .. kb + 31 of column c of W, and their part of P_cc (this thread's alone: c = t mod 256)
          double q = pii[c];
#pragma unroll
          for (int r = 0; r < kB; ++r) {
            (rows + (int64_t)r * npad)[cu] = y[r];
            q += (double)y[r] * (double)y[r];
          }
          pii[c] = q;
        }
      }
      __syncthreads();

      // 3: the trailing tiles (I, J), I > K, J in 0 .. K and I .. nb - 1, in row-major order: a wave per tile.  The
      // product is taken transposed (A from block J, B from block I), so a lane's 4 results are consecutive columns.
      // The next tile of the wave is loaded before the current one is updated.
      int total = 0;
      for (int i = K + 1; i < nb; ++i) total += K + 1 + nb - i;
      int In = K + 1, Jn = 0, base = 0;
      // (In, Jn) <- the tile of job q; q only grows
      auto seek = [&](int q) {
        while (q - base >= K + 1 + nb - In) {
          base += K + 1 + nb - In;
          ++In;
        }
        const int jj = q - base;
        Jn = jj <= K ? jj : In + (jj - K - 1);
      };
      // this lane's 16 bytes of block (a, b) of tile (I, J)
      auto at = [&](int I, int J, int a, int b) {
        return reinterpret_cast<f32x4*>(&D[(int64_t)(I * kB + b * 16 + fcol) * npad + J * kB + a * 16 + 4 * frow]);
      };
      f32x4 nx[2][2];
      if (wave < total) {
        seek(wave);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) nx[a][b] = *at(In, Jn, a, b);
      }
      for (int q = wave; q < total; q += kThreads / 64) {
        const int I = In, J = Jn, qn = q + kThreads / 64;
        f32x4 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = nx[a][b];
        if (qn < total) {
          seek(qn);
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) nx[a][b] = *at(In, Jn, a, b);
        }
        const float* pj = &panel[frow * ldp + J * kB + fcol];
        const float* pi = &panel[frow * ldp + I * kB + fcol];
#pragma unroll
        for (int kk = 0; kk < kB / 4; ++kk) {
          float fj[2], fi[2];
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            fj[a] = pj[kk * 4 * ldp + a * 16];
            fi[a] = -pi[kk * 4 * ldp + a * 16];
          }
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
              acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fj[a], fi[b], acc[a][b], 0, 0, 0);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) *at(I, J, a, b) = acc[a][b];
      }
      __syncthreads();
    }

    // ---- scales: d_i = 1 / sqrt(P_ii) ----
    for (int i = t; i < n; i += kThreads) {
      const double s = pii[i];
      if (scale[i] != 0.0f) {
        if (!(s > 0.0 && s < (double)INFINITY)) *bad = 1;
        scale[i] = (float)(1.0 / sqrt(s));
      }
    }
    __syncthreads();
    const bool failed = *bad != 0;

    if (failed) {
      for (int64_t e = t; e < (int64_t)n * n; e += kThreads) o[e] = NAN;
    } else {
      // ---- product ----
      const Thread th;
      for (int pair = 0; pair < pairs_of(nt); ++pair) {
        const Item it(pair, nt, wave);
        const int k0 = it.bj * kTile;
        f32x4 pre[2][kSlots], acc[3][3];
        load_panels<true>(pre, D, n, npad, k0, it, th);
        // W is lower triangular: above its diagonal the slab holds what is left of C; column i is scaled by d_i
        run<true>(prod, pre, acc, D, n, npad, it, th, [&](int side, int k, int c, f32x4 v) {
          const int col = it.col0(side) + c;
          const f32x4 d = *reinterpret_cast<const f32x4*>(&scale[col]);
          f32x4 z;
#pragma unroll
          for (int e = 0; e < 4; ++e) z[e] = col + e <= k ? v[e] * d[e] : 0.0f;
          return z;
        }, k0);

        for_each_block(it, th, [&](int a, int b, bool tri, int li0, int gi0, int gj) {
          f32x4 v = acc[a][b];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float c = 0.0f - v[r];
            c = c > 1.0f ? 1.0f : (c < -1.0f ? -1.0f : c);
            if (absolute) c = fabsf(c);
            if (tri && gi0 + r == gj) c = scale[gj] == 0.0f ? 0.0f : 1.0f;
            v[r] = c;
          }
          if (gj >= n) return;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (gi0 + r < n && (!tri || gi0 + r <= gj)) o[(int64_t)(gi0 + r) * n + gj] = v[r];
          if (kVecOut && !tri) {
            if (gi0 < n) *reinterpret_cast<f32x4*>(&o[(int64_t)gj * n + gi0]) = v;
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (gi0 + r < n && (!tri || gi0 + r < gj)) o[(int64_t)gj * n + gi0 + r] = v[r];
          }
        });
      }
    }
    __syncthreads();                          // the next unit's build overwrites d and the slab
  }
}

int check(int64_t U, int32_t n) { return cgnn_check_cohort_upto(U, n, CGNN_PARTIAL_MAX_NODES); }

// the launch's workgroups: one per unit, as many as the CUs hold
int grid_of(int64_t U, size_t lds) { return cgnn_grid_for(U, cgnn_wg_per_cu_by_lds(lds, kLdsBytes)); }

template <bool kVecOut, bool kEach>
int launch_as(int grid, size_t lds, const float* matrices, int64_t U, int32_t n, double shrinkage, const double* alphas,
              int32_t absolute, float* slabs, float* out, void* stream) {
  if (!cgnn_raise_lds_limit<k_partial<kVecOut, kEach>>(kLdsBytes)) return CGNN_ELAUNCH;
  k_partial<kVecOut, kEach><<<grid, kThreads, lds, cgnn_stream(stream)>>>(matrices, U, n, shrinkage, alphas, absolute,
                                                                         slabs, out);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}

// Both entry points: the checks, then the one launch.  each: alphas[u] is unit u's shrinkage; else `shrinkage` is all's.
int launch(const float* matrices, int64_t U, int32_t n, double shrinkage, const double* alphas, bool each,
           int32_t absolute, void* workspace, int64_t workspace_bytes, float* out, int64_t out_bytes, void* stream) {
  if (check(U, n) != CGNN_OK || !(shrinkage >= 0.0 && shrinkage <= 1.0)) return CGNN_EINVAL;
  if (workspace_bytes < 0 || out_bytes < 0 || (reinterpret_cast<uintptr_t>(workspace) & 15)) return CGNN_EINVAL;
  if (U == 0) return CGNN_OK;
  if (!matrices || !out || !workspace) return CGNN_EINVAL;
  if ((reinterpret_cast<uintptr_t>(matrices) | reinterpret_cast<uintptr_t>(out)) & 3) return CGNN_EINVAL;
  if (each && (!alphas || (reinterpret_cast<uintptr_t>(alphas) & 7))) return CGNN_EINVAL;
  // out [U n][n] (U * n < 2^31 and n <= 1024: the byte count fits, and is compared by division as its neighbours do)
  if (out_bytes / (int64_t)sizeof(float) / n < U * n) return CGNN_EINVAL;
  const size_t lds = lds_of(n);
  if (lds > (size_t)kLdsBytes) return CGNN_EINVAL;            // (n <= CGNN_PARTIAL_MAX_NODES fits: 151 KB at 1024)
  const int grid = grid_of(U, lds);
  if (workspace_bytes < grid * slab_bytes(padded(n))) return CGNN_EINVAL;
  const bool vec = n % 4 == 0 && !(reinterpret_cast<uintptr_t>(out) & 15);
  float* slabs = static_cast<float*>(workspace);
  const auto go = each ? (vec ? launch_as<true, true> : launch_as<false, true>)
                       : (vec ? launch_as<true, false> : launch_as<false, false>);
  return go(grid, lds, matrices, U, n, shrinkage, alphas, absolute, slabs, out, stream);
}

}  // namespace

extern "C" int64_t cgnn_ingest_partial_workspace_bytes(int64_t U, int32_t n) {
  if (check(U, n) != CGNN_OK) return CGNN_EINVAL;
  return grid_of(U, lds_of(n)) * slab_bytes(padded(n));       // a slab per workgroup of the launch
}

extern "C" int cgnn_ingest_partial(const float* matrices, int64_t U, int32_t n, double shrinkage, int32_t absolute,
                                   void* workspace, int64_t workspace_bytes, float* out, int64_t out_bytes,
                                   void* stream) {
  return launch(matrices, U, n, shrinkage, nullptr, false, absolute, workspace, workspace_bytes, out, out_bytes,
                stream);
}

extern "C" int cgnn_ingest_partial_each(const float* matrices, int64_t U, int32_t n, const double* shrinkage,
                                        int32_t absolute, void* workspace, int64_t workspace_bytes, float* out,
                                        int64_t out_bytes, void* stream) {
  return launch(matrices, U, n, 0.0, shrinkage, true, absolute, workspace, workspace_bytes, out, out_bytes, stream);
}
