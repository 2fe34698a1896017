// collate.hip -- on-device collate of a batch's COO from a device-resident dataset whose subjects keep
// different numbers of edges (cgnn_collate_edges; the host loop it replaces is graph.py:143-167).
//
// The dataset stores every subject's edges as one run of flat arrays (edge_ptr [S+1]); a batch is b
// subject ids.  Two kernels on the caller's stream behind one entry point:
//
//   k_collate_scan   one workgroup: eptr[g] = sum_{h<g} (edge_ptr[ids[h]+1] - edge_ptr[ids[h]]), int32 [b+1]
//                    -- the offsets cgnn_csr_build_grouped wants, so the batch needs no upload of them.
//   k_collate_copy   the copies.  The work is the FLAT edge range [0, eptr[b]) of the batch cut into chunks
//                    of CGNN_COLLATE_CHUNK edges that a persistent grid walks with a grid stride; a thread
//                    owns CGNN_COLLATE_VEC consecutive edges, finds their graph by a binary search over
//                    eptr (held in LDS up to CGNN_COLLATE_LDS_GRAPHS graphs, read from L2 beyond) and moves
//                    the weights (one 16-byte access), and the two index rows (two 16-byte accesses each,
//                    + g * n).  How the edges are spread over the subjects does not matter: a subject ten
//                    times the size of the others is just more chunks.
//
// Accesses: a thread's destination starts at a multiple of 4 edges, so weight and source-row stores are
// 16-byte aligned (the destination-row ones when the edge count is even, else 8); the source of a run starts
// wherever the subject's run does (any 4-byte / 8-byte offset).  Both are 16 bytes wide, declared at element
// alignment where that is all that is known -- gfx950 serves them as one global_load/store_dwordx4.  A thread whose 4 edges straddle graphs (every run's tail/head) or
// the end of the batch moves them one by one.  Vector memory instructions only; no atomics; no scratch.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kVec = CGNN_COLLATE_VEC;
constexpr int kChunk = CGNN_COLLATE_CHUNK;
static_assert(kChunk == kThreads * kVec, "a chunk is one pass of a workgroup");
static_assert(kVec == 4, "the vector forms below move 4 edges");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
// the same vectors at element alignment: where a subject's run starts inside the dataset arrays, and the
// destination row of an odd-sized batch
typedef f32x4 f32x4_e __attribute__((aligned(4)));
typedef i64x2 i64x2_e __attribute__((aligned(8)));

// eptr[0] = 0, eptr[g+1] = eptr[g] + edges of subject ids[g]; a subject id outside the dataset or a run
// outside the edge arrays counts as empty, and the running sum stops at `cap` (the edge count the output
// buffers were sized for), so the copy below stays inside both whatever the arrays hold.
__global__ __launch_bounds__(kThreads) void k_collate_scan(const int64_t* __restrict__ edge_ptr, int64_t num_subjects,
                                                           int64_t ds_edges, const int64_t* __restrict__ ids, int b,
                                                           int64_t cap, int32_t* __restrict__ eptr) {
  __shared__ int64_t part[kThreads];
  const int t = threadIdx.x;
  for (int g = t; g < b; g += kThreads) {
    const int64_t id = ids[g];
    int64_t cnt = 0;
    if (id >= 0 && id < num_subjects) {
      const int64_t lo = edge_ptr[id], hi = edge_ptr[id + 1];
      if (lo >= 0 && hi >= lo && hi <= ds_edges) cnt = hi - lo;
    }
    eptr[g + 1] = (int32_t)(cnt < cap ? cnt : cap);
  }
  __syncthreads();
  const int per = (b + kThreads - 1) / kThreads;
  const int g0 = t * per < b ? t * per : b, g1 = g0 + per < b ? g0 + per : b;
  int64_t sum = 0;
  for (int g = g0; g < g1; ++g) sum += eptr[g + 1];
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < kThreads; o <<= 1) {          // inclusive scan of the 256 slice sums
    const int64_t add = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int64_t run = part[t] - sum;
  for (int g = g0; g < g1; ++g) {
    run += eptr[g + 1];
    eptr[g + 1] = (int32_t)(run < cap ? run : cap);
  }
  if (t == 0) eptr[0] = 0;
}

template <bool kLds>
__global__ __launch_bounds__(kThreads) void k_collate_copy(
    const int64_t* __restrict__ loc0, const int64_t* __restrict__ loc1, const float* __restrict__ w_ds,
    const int64_t* __restrict__ edge_ptr, const int64_t* __restrict__ ids, int b, int64_t n,
    const int32_t* __restrict__ eptr, int64_t* __restrict__ out0, int64_t* __restrict__ out1,
    float* __restrict__ outw) {
  extern __shared__ __align__(16) int32_t sh_eptr[];
  const int t = threadIdx.x;
  if (kLds) {
    for (int i = t; i <= b; i += kThreads) sh_eptr[i] = eptr[i];
    __syncthreads();
  }
  auto at = [&](int i) -> int32_t { return kLds ? sh_eptr[i] : eptr[i]; };
  const int64_t E = at(b);
  const int64_t chunks = (E + kChunk - 1) / kChunk;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t p0 = c * kChunk + (int64_t)t * kVec;
    if (p0 >= E) continue;
    int lo = 0, hi = b;                               // eptr[lo] <= p0 < eptr[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (at(mid) <= p0) lo = mid; else hi = mid;
    }
    int g = lo;                                       // the (non-empty) graph of edge p0
    const int64_t gbeg = at(g), gend = at(g + 1);
    if (p0 + kVec <= gend) {
      const int64_t s = edge_ptr[ids[g]] + (p0 - gbeg);
      const int64_t off = (int64_t)g * n;
      const f32x4 w = __builtin_nontemporal_load(reinterpret_cast<const f32x4_e*>(w_ds + s));
      const i64x2 a0 = __builtin_nontemporal_load(reinterpret_cast<const i64x2_e*>(loc0 + s));
      const i64x2 a1 = __builtin_nontemporal_load(reinterpret_cast<const i64x2_e*>(loc0 + s + 2));
      const i64x2 b0 = __builtin_nontemporal_load(reinterpret_cast<const i64x2_e*>(loc1 + s));
      const i64x2 b1 = __builtin_nontemporal_load(reinterpret_cast<const i64x2_e*>(loc1 + s + 2));
      *reinterpret_cast<f32x4*>(outw + p0) = w;
      *reinterpret_cast<i64x2*>(out0 + p0) = a0 + off;
      *reinterpret_cast<i64x2*>(out0 + p0 + 2) = a1 + off;
      *reinterpret_cast<i64x2_e*>(out1 + p0) = b0 + off;       // (row 1 starts 8 * num_edges bytes into the buffer)
      *reinterpret_cast<i64x2_e*>(out1 + p0 + 2) = b1 + off;
    } else {
      // the run ends (or the batch does) inside this thread's edges: one by one, stepping over empty graphs
      for (int j = 0; j < kVec; ++j) {
        const int64_t p = p0 + j;
        if (p >= E) break;
        while (p >= at(g + 1)) ++g;
        const int64_t s = edge_ptr[ids[g]] + (p - at(g));
        const int64_t off = (int64_t)g * n;
        outw[p] = w_ds[s];
        out0[p] = loc0[s] + off;
        out1[p] = loc1[s] + off;
      }
    }
  }
}

}  // namespace

extern "C" int cgnn_collate_edges(const int64_t* edge_local, const float* edge_weight_ds, const int64_t* edge_ptr,
                                  int64_t num_subjects, int64_t ds_edges, const int64_t* ids, int32_t b, int32_t n,
                                  int64_t num_edges, int64_t* edge_index, int64_t edge_index_bytes,
                                  float* edge_weight, int64_t edge_weight_bytes, int32_t* eptr, int64_t eptr_bytes,
                                  void* stream) {
  if (b < 0 || n <= 0 || num_edges < 0 || num_edges >= INT32_MAX || num_subjects < 0 || ds_edges < 0)
    return CGNN_EINVAL;
  if ((int64_t)b * n >= INT32_MAX) return CGNN_EINVAL;      // node ids of a batch are int32 inside the library
  if (b == 0 || num_edges == 0) return CGNN_OK;             // nothing to copy: eptr is all zeros, not written
  if (!edge_local || !edge_weight_ds || !edge_ptr || !ids || !edge_index || !edge_weight || !eptr)
    return CGNN_EINVAL;
  CGNN_NEED_BYTES(edge_index, edge_index_bytes, 2 * num_edges * (int64_t)sizeof(int64_t));
  CGNN_NEED_BYTES(edge_weight, edge_weight_bytes, num_edges * (int64_t)sizeof(float));
  CGNN_NEED_BYTES(eptr, eptr_bytes, ((int64_t)b + 1) * (int64_t)sizeof(int32_t));
  if ((reinterpret_cast<uintptr_t>(edge_index) & 15) || (reinterpret_cast<uintptr_t>(edge_weight) & 15) ||
      (reinterpret_cast<uintptr_t>(edge_local) & 7) || (reinterpret_cast<uintptr_t>(edge_weight_ds) & 3))
    return CGNN_EINVAL;
  hipStream_t st = cgnn_stream(stream);
  k_collate_scan<<<1, kThreads, 0, st>>>(edge_ptr, num_subjects, ds_edges, ids, b, num_edges, eptr);
  CGNN_CHECK_LAUNCH();
  const int64_t chunks = (num_edges + kChunk - 1) / kChunk;
  const int64_t cap = 4 * (int64_t)cgnn_fused_grid();       // persistent: 16 waves per CU stream the copies
  const int grid = (int)(chunks < cap ? chunks : cap);
  int64_t* out1 = edge_index + num_edges;
  if (b <= CGNN_COLLATE_LDS_GRAPHS)
    k_collate_copy<true><<<grid, kThreads, ((size_t)b + 1) * sizeof(int32_t), st>>>(
        edge_local, edge_local + ds_edges, edge_weight_ds, edge_ptr, ids, b, n, eptr, edge_index, out1, edge_weight);
  else
    k_collate_copy<false><<<grid, kThreads, 0, st>>>(edge_local, edge_local + ds_edges, edge_weight_ds, edge_ptr, ids,
                                                     b, n, eptr, edge_index, out1, edge_weight);
  CGNN_CHECK_LAUNCH();
  return CGNN_OK;
}
