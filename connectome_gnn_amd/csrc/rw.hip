// rw.hip -- the random-walk structural encoding of a device-resident cohort of dense connectivity matrices (float
// [S, n, n]) at the thresholds of cgnn_ingest_select / cgnn_ingest_count (include/cgnn_rw.h):
// cgnn_ingest_rw, cgnn_ingest_rw_workspace_bytes.
//
// Per subject with matrix A and threshold t: e_ij iff i != j, A_ij > t and A_ij > 0 (ingest_rows.h); nothing is
// symmetrised; rows are what is summed.  a_ij = A_ij on edges (1 with CGNN_RW_BINARY), s_i = sum_j a_ij,
// P_ij = a_ij / s_i (an exact zero row where s_i == 0), and step k is r_k(i) = ((P)^k)_ii.
//
//   k_rw      one launch; a workgroup of 4 waves owns a subject, grid stride.  Its intermediates M2 = P P, M3 = P M2 and
//             M4 = M2 M2 (as far as the largest requested step needs them) are slabs [npad][npad] fp32,
//             npad = 96 ceil(n / 96), in workgroup blockIdx.x's slice of the workspace: a slab set per workgroup of the
//             launch, not per subject.  A slab is written whole, its padding with the exact zeros that zero operands
//             give, so nothing reads what a previous subject left.
//     operand what a product or a sum reads is an Operand: the kept values a, P, or a slab.  P is never stored: wherever
//             a panel or an entry of it is wanted it is formed from the matrix row, the threshold and the fp32 s_i,
//             which live in LDS.
//     walk    the row walk that the sums s_i and r_k share: thread t owns row i0 + t of a block of 256 rows; a tile
//             [256 rows][32 columns] of the left operand is loaded with 16-byte accesses along the rows and stored to
//             LDS with rows of 33 floats, so that a thread reads ITS row without a bank conflict (the transposition of
//             what is read against the thread grain goes tile-wise through LDS); the right operand's entry (M_b)_ji is
//             read from row j at consecutive i by consecutive threads.  One fp64 accumulator per row, columns
//             ascending: s_i = sum_j a_ij; r_k(i) = sum_j (M_a)_ij (M_b)_ji, every product exact in fp64.  Rounded to
//             fp32 once.
//     product a plain tiled C = X Y on v_mfma_f32_16x16x4_f32, 96 x 96 tiles, K-steps of 32, 2 x 2 waves of 3 x 3
//             blocks as in gram_tile.h.  The right panel Y [32 k][96 j] is gram_tile.h's (rows of 112 floats).  X is NOT
//             symmetric, so the left panel is X [96 i][32 k] as it lies in memory, rows of 34 floats, and lane l reads
//             its fragment entry A[i = l & 15][k = l >> 4] transposed: a 4-byte LDS read is served in halves of 32
//             lanes over 32 banks, and 34 i + k = 2 i + k (mod 32) is a different bank for each lane of a half (k is
//             0, 1 in the first and 2, 3 in the second).  The next step's loads are issued before this step's MFMAs;
//             two buffers, one barrier a step; k ascending.
// A kept entry that is not finite (weights only) marks the subject: its columns for k >= 2 are NaN and no product is
// formed.  No atomics, and neither the order of any sum nor the assignment of work depends on the grid, the run or on
// which steps are asked for: the same bits on every run, for every grid and every request.  Offsets inside a subject
// and inside a slab are below 2^31 (n <= 1024); a subject's and a workgroup's base offsets are 64-bit.
#include <float.h>
#include <math.h>

#include "ingest_rows.h"
#include "measure_request.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 96;                             // output tile of a product
constexpr int kKS = 32;                               // k per K-step
constexpr int kLdL = 34;                              // left panel [kTile i][kKS k]: 34 i + k (mod 32) is a bank per lane
constexpr int kLdR = 112;                             // right panel [kKS k][kTile j]: gram_tile.h's
constexpr int kSlots = kTile * kKS / 4 / kThreads;    // float4 slots of either panel per thread
constexpr int kPanel = kTile * kLdL + kKS * kLdR;     // floats of a buffer: left | right
constexpr int kWalkRows = kThreads;                   // rows of a walk's block: one per thread
constexpr int kWalkCols = 32;                         // columns of a walk's tile
constexpr int kWalkLd = kWalkCols + 1;
constexpr int kWalkSlots = kWalkRows * kWalkCols / 4 / kThreads;
constexpr int kLdsFloats = 2 * kPanel > kWalkRows * kWalkLd ? 2 * kPanel : kWalkRows * kWalkLd;
constexpr int kWgPerCu = 2;                           // 58 KB of LDS each, at most 256 registers a thread
static_assert(kSlots * kThreads * 4 == kTile * kKS, "a panel is a whole number of slots per thread");
static_assert((kLdsFloats + CGNN_RW_MAX_NODES) * sizeof(float) <= 63 * 1024, "static LDS");

typedef cgnn_f32x4 f32x4;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef cgnn_columns<CGNN_RW_MAX_STEPS> Columns;

inline __host__ __device__ int npad_of(int n) { return (n + kTile - 1) / kTile * kTile; }
// the slabs a request needs, by its largest step k: M2 from 3 on, M3 from 5 on, M4 from 7 on
inline __host__ __device__ int slabs_of(int top) { return top >= 7 ? 3 : top >= 5 ? 2 : top >= 3 ? 1 : 0; }
inline int64_t slab_bytes(int npad) { return (int64_t)npad * npad * (int64_t)sizeof(float); }

enum { kValues = 0, kWalkP = 1, kSlab = 2 };          // what an Operand is: a, P, or a stored M

// What does not change while a subject is worked on (all of it the same on every thread).
struct Subject {
  const float* s;                                     // LDS: s_i in fp32
  int n;
  float thr;
  bool binary;
};

// Rows of `ld` floats from p on, `rows` of them: the subject's matrix (kValues, kWalkP: ld = rows = n) or a slab
// (ld = rows = npad).  A slab's pointer is a plain one: it is written and read back inside the launch.
struct Operand {
  const float* p;
  int ld, rows, kind;
};

// entry (row, col) of a or P from the loaded matrix entry v
template <bool kNormalised>
__device__ __forceinline__ float value_of(const Subject& sj, float v, int row, int col, float si) {
  if (col == row || !cgnn_kept(v, sj.thr)) return 0.0f;
  const float a = sj.binary ? 1.0f : v;
  if (!kNormalised) return a;
  return si > 0.0f ? a / si : 0.0f;
}

// 4 consecutive columns (col a multiple of 4; below ld for a slab) of row `row` of `op`; rows and columns outside the
// operand read as 0.  bad: a kept weight that is not finite was seen (kValues only).
__device__ __forceinline__ f32x4 op_load4(const Subject& sj, const Operand& op, int row, int col, bool& bad) {
  f32x4 out = {0.f, 0.f, 0.f, 0.f};
  if (row >= op.rows) return out;
  const float* at = op.p + row * op.ld;
  if (op.kind == kSlab) return *reinterpret_cast<const f32x4*>(at + col);
  const f32x4 v = cgnn_load_row4(at, col, sj.n);      // columns >= n: -inf, never kept
  const float si = op.kind == kWalkP ? sj.s[row] : 1.0f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    out[e] = op.kind == kWalkP ? value_of<true>(sj, v[e], row, col + e, si) : value_of<false>(sj, v[e], row, col + e, si);
    if (op.kind == kValues) bad |= !sj.binary && col + e != row && cgnn_kept(v[e], sj.thr) && !(v[e] <= FLT_MAX);
  }
  return out;
}

// entry (row, col) of P or of a slab, col below n; a row outside the operand reads as 0
__device__ __forceinline__ float op_load1(const Subject& sj, const Operand& op, int row, int col) {
  if (row >= op.rows) return 0.0f;
  const float v = op.p[row * op.ld + col];
  return op.kind == kSlab ? v : value_of<true>(sj, v, row, col, sj.s[row]);
}

// The row walk (`walk` above) over every row block of a subject.  kDot: out(i) = sum_j (opa)_ij (opb)_ji, else
// out(i) = sum_j (opa)_ij; out(i) is rounded once and written to out[i * stride], i < n.  Ends behind a barrier.
template <bool kDot>
__device__ __forceinline__ void walk(const Subject& sj, const Operand& opa, const Operand& opb, float* tile, bool& bad,
                                     float* out, int stride) {
  const int t = threadIdx.x;
  const int n = sj.n;
  const int trow = t / (kWalkCols / 4), tcol = 4 * (t % (kWalkCols / 4));   // slot q: row trow + 32 q
  for (int i0 = 0; i0 < n; i0 += kWalkRows) {
    const int i = i0 + t;
    double acc = 0.0;
    for (int j0 = 0; j0 < n; j0 += kWalkCols) {
      f32x4 v[kWalkSlots];
#pragma unroll
      for (int q = 0; q < kWalkSlots; ++q)
        v[q] = op_load4(sj, opa, i0 + trow + q * (kThreads / (kWalkCols / 4)), j0 + tcol, bad);
#pragma unroll
      for (int q = 0; q < kWalkSlots; ++q) {
        float* p = tile + (trow + q * (kThreads / (kWalkCols / 4))) * kWalkLd + tcol;
#pragma unroll
        for (int c = 0; c < 4; ++c) p[c] = v[q][c];
      }
      __syncthreads();
      if (i < n) {
        const float* mine = tile + t * kWalkLd;
        if (kDot) {
#pragma unroll 1
          for (int c0 = 0; c0 < kWalkCols; c0 += 8) {
            float b[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) b[c] = op_load1(sj, opb, j0 + c0 + c, i);
#pragma unroll
            for (int c = 0; c < 8; ++c) acc += (double)mine[c0 + c] * (double)b[c];
          }
        } else {
#pragma unroll
          for (int c = 0; c < kWalkCols; ++c) acc += (double)mine[c];
        }
      }
      __syncthreads();
    }
    if (i < n) out[(int64_t)i * stride] = (float)acc;
  }
}

// C = (opa) (opb) for a slab C [npad][npad], whole tiles (`product` above).  Ends behind a barrier: C can be read.
__device__ __forceinline__ void product(const Subject& sj, float* C, int npad, const Operand& opa, const Operand& opb,
                                        float* lds) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int frow = lane >> 4, fcol = lane & 15, wr = wave >> 1, wc = wave & 1;
  const int nt = npad / kTile;
  const int ksteps = (sj.n + kKS - 1) / kKS;          // rows k >= n of either operand are zeros
  // slot q of the left panel: row lrow + 32 q, columns lcol ..; of the right panel: row rrow + q', columns rcol ..
  const int lrow = t / (kKS / 4), lcol = 4 * (t % (kKS / 4));
  bool unused = false;
  for (int tile = 0; tile < nt * nt; ++tile) {
    const int i0 = tile / nt * kTile, j0 = tile % nt * kTile;
    f32x4 pl[kSlots], pr[kSlots];
    auto load = [&](int k0) {
#pragma unroll
      for (int q = 0; q < kSlots; ++q) {
        const int e = t + kThreads * q;
        pl[q] = op_load4(sj, opa, i0 + lrow + q * (kThreads / (kKS / 4)), k0 + lcol, unused);
        pr[q] = op_load4(sj, opb, k0 + e / (kTile / 4), j0 + 4 * (e % (kTile / 4)), unused);
      }
    };
    auto store = [&](int buf) {
      float* L = lds + buf * kPanel;
      float* R = L + kTile * kLdL;
#pragma unroll
      for (int q = 0; q < kSlots; ++q) {
        const int e = t + kThreads * q;
        float* l = L + (lrow + q * (kThreads / (kKS / 4))) * kLdL + lcol;      // (rows of 34 floats: 8-byte aligned)
        *reinterpret_cast<f32x2*>(l) = f32x2{pl[q][0], pl[q][1]};
        *reinterpret_cast<f32x2*>(l + 2) = f32x2{pl[q][2], pl[q][3]};
        *reinterpret_cast<f32x4*>(R + (e / (kTile / 4)) * kLdR + 4 * (e % (kTile / 4))) = pr[q];
      }
    };
    f32x4 acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    load(0);
    store(0);
    __syncthreads();
    int cur = 0;
    for (int ks = 0; ks < ksteps; ++ks) {
      const bool more = ks + 1 < ksteps;
      if (more) load((ks + 1) * kKS);
      const float* pa = lds + cur * kPanel + (wr * 48 + fcol) * kLdL + frow;
      const float* pb = lds + cur * kPanel + kTile * kLdL + frow * kLdR + wc * 48 + fcol;
#pragma unroll
      for (int kk = 0; kk < kKS / 4; ++kk) {
        float fa[3], fb[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          fa[a] = pa[a * 16 * kLdL + kk * 4];
          fb[a] = pb[kk * 4 * kLdR + a * 16];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a], fb[b], acc[a][b], 0, 0, 0);
      }
      if (more) store(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
    // D[i][j] of a block: lane l, register r holds i = 4 (l >> 4) + r, j = l & 15
    float* c = C + (i0 + wr * 48 + 4 * frow) * npad + j0 + wc * 48 + fcol;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) c[(a * 16 + r) * npad + b * 16] = acc[a][b][r];
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads, 2) void k_rw(const float* __restrict__ matrices, int64_t S, int n,
                                                    const float* __restrict__ thr, Columns cols, int binary, int top,
                                                    float* slabs, float* __restrict__ xout) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  __shared__ float s_row[CGNN_RW_MAX_NODES];
  __shared__ int s_col[CGNN_RW_MAX_STEPS];            // the columns, where a step that is not a constant can index them
  __shared__ int s_bad;
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < CGNN_RW_MAX_STEPS; ++k)
    if (t == k) s_col[k] = cols.col[k];
  if (t == 0) s_bad = 0;
  __syncthreads();
  const int npad = npad_of(n);
  const int nslabs = slabs_of(top);
  float* mine = slabs + (int64_t)blockIdx.x * nslabs * npad * npad;   // M2 | M3 | M4
  const float nan = __int_as_float(0x7fc00000);

  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const float* __restrict__ A = matrices + s * (int64_t)n * n;
    const Subject sj = {s_row, n, thr[s], binary != 0};
    float* __restrict__ xs = xout + s * (int64_t)n * cols.ldx;
    const Operand values = {A, n, n, kValues}, P = {A, n, n, kWalkP};

    bool bad = false;
    walk<false>(sj, values, values, lds, bad, s_row, 1);
    if (bad) s_bad = 1;                               // (every writer writes the same value)
    __syncthreads();                                  // s_row and the mark are there
    const bool nonfinite = s_bad != 0;

    if (cols.col[0] >= 0)
      for (int i = t; i < n; i += kThreads) xs[(int64_t)i * cols.ldx + cols.col[0]] = 0.0f;
    if (nonfinite) {
      for (int k = 2; k <= CGNN_RW_MAX_STEPS; ++k) {
        const int col = s_col[k - 1];
        if (col < 0) continue;
        for (int i = t; i < n; i += kThreads) xs[(int64_t)i * cols.ldx + col] = nan;
      }
      __syncthreads();                                // every thread has read the mark
      if (t == 0) s_bad = 0;
      continue;                                       // (the next walk's barriers stand before the mark is set again)
    }
    // M2 = P P, M3 = P M2, M4 = M2 M2
    for (int p = 0; p < nslabs; ++p) {
      const Operand m2 = {mine, npad, npad, kSlab};
      product(sj, mine + p * npad * npad, npad, p == 2 ? m2 : P, p == 0 ? P : m2, lds);
    }
    // r_k(i) = sum_j (M_a)_ij (M_b)_ji, a = floor(k / 2), b = ceil(k / 2)
    for (int k = 2; k <= CGNN_RW_MAX_STEPS; ++k) {
      const int col = s_col[k - 1];
      if (col < 0) continue;
      const int a = k / 2, b = (k + 1) / 2;
      const Operand ma = {a == 1 ? A : mine + (a - 2) * npad * npad, a == 1 ? n : npad, a == 1 ? n : npad,
                          a == 1 ? kWalkP : kSlab};
      const Operand mb = {b == 1 ? A : mine + (b - 2) * npad * npad, b == 1 ? n : npad, b == 1 ? n : npad,
                          b == 1 ? kWalkP : kSlab};
      bool unused = false;
      walk<true>(sj, ma, mb, lds, unused, xs + col, cols.ldx);
    }
    __syncthreads();                                  // the next subject's walk overwrites s_row
  }
}

// (CGNN_OK, the columns, the largest step) of a valid call
int check(int64_t S, int32_t n, const int32_t* steps, int32_t num, const int32_t* cols, int32_t ldx, bool with_cols,
          Columns* c, int* top) {
  if (cgnn_check_cohort_upto(S, n, CGNN_RW_MAX_NODES) != CGNN_OK) return CGNN_EINVAL;
  if (cgnn_check_request(steps, num, 1, cols, ldx, with_cols, c) != CGNN_OK) return CGNN_EINVAL;
  *top = 0;
  for (int k = 1; k <= CGNN_RW_MAX_STEPS; ++k)
    if (c->col[k - 1] >= 0) *top = k;
  return CGNN_OK;
}

int grid_of(int64_t S) { return cgnn_grid_for(S, kWgPerCu); }

}  // namespace

extern "C" int64_t cgnn_ingest_rw_workspace_bytes(int64_t S, int32_t n, const int32_t* steps, int32_t num_steps) {
  Columns c;
  int top;
  if (check(S, n, steps, num_steps, nullptr, 0, false, &c, &top) != CGNN_OK) return CGNN_EINVAL;
  return grid_of(S) * slabs_of(top) * slab_bytes(npad_of(n));   // a slab set per workgroup of the launch
}

extern "C" int cgnn_ingest_rw(const float* matrices, int64_t S, int32_t n, const float* thr, const int32_t* steps,
                              int32_t num_steps, const int32_t* cols, int32_t ldx, int32_t flags, void* workspace,
                              int64_t workspace_bytes, float* x, int64_t x_bytes, void* stream) {
  Columns c;
  int top;
  if (check(S, n, steps, num_steps, cols, ldx, true, &c, &top) != CGNN_OK) return CGNN_EINVAL;
  if (flags & ~CGNN_RW_BINARY) return CGNN_EINVAL;
  if (cgnn_check_byte_counts(workspace, {workspace_bytes, x_bytes}) != CGNN_OK) return CGNN_EINVAL;
  if (S == 0) return CGNN_OK;
  if (cgnn_check_cohort_buffers(matrices, thr, workspace, x, x_bytes, true, S * n, c.ldx) != CGNN_OK) return CGNN_EINVAL;
  const int grid = grid_of(S);
  const int64_t need = grid * slabs_of(top) * slab_bytes(npad_of(n));
  if (need > 0 && (!workspace || workspace_bytes < need)) return CGNN_EINVAL;
  k_rw<<<grid, kThreads, 0, cgnn_stream(stream)>>>(matrices, S, n, thr, c, flags & CGNN_RW_BINARY, top,
                                                  static_cast<float*>(workspace), x);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
