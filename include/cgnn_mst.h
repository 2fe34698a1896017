/* cgnn_mst.h -- part of the C ABI of libcgnn_hip.so (cgnn.h, whose conventions and return codes hold here and which
 * includes this file): the maximum-spanning-tree backbone of a matrix cohort.  It is additive: CGNN_ABI_VERSION stays 2.
 *
 * Backbone: one threshold per subject and the k-NN graph both leave a modular connectome in pieces.
 * The maximum spanning forest of a subject's positive weights is the sparsest graph that connects whatever its positive
 * entries connect; united with a threshold it gives a connected graph at any density.  What is dropped becomes an exact
 * +0.0, so that cgnn_ingest_count / _fill / _measures / _paths / _wpaths / _modules at the threshold 0.0 see exactly the
 * united graph.  matrices: float [S, n, n], contiguous, any sign, not necessarily symmetric.  Per subject with matrix A:
 *   p(x) = x if x > 0 else 0.  A NaN is not positive.  +inf is positive.  A subnormal is positive.
 *   The pair {i, j}, i < j, has weight w_ij = max(p(A_ij), p(A_ji)).  It is a candidate iff w_ij > 0.
 *   Order: the pair (i, j) comes before (i', j') iff w > w', or w == w' and (i, j) is lexicographically lower.  This is
 *     a strict total order.
 *   F is the maximum spanning forest under that order.  Kruskal takes a pair iff its ends lie in different components.
 *     F is unique.  It has n - c pairs, where c is the number of components of the candidate graph.
 *     Any correct algorithm that compares edges by this strict order finds the same F.  That includes Prim with restarts
 *     from the lowest unvisited node, Boruvka and Kruskal.  The all-0.5 matrix gives the star at node 0.
 *   kept_ij iff i != j, A_ij > 0 and ({i, j} in F or A_ij > t_s).  t_s is the subject's threshold.  No thresholds means
 *     t_s = +inf, the tree alone.
 *     A tree pair whose reverse entry is not positive keeps only the positive direction.  knn's "union" mode does the
 *     same.
 *   out_ij is the bits of A_ij where kept and +0.0 elsewhere.  The diagonal and every NaN become +0.0 too.
 *   out may be `matrices` itself and gives the same bits.  Any other overlap is refused.
 * One launch on `stream`: min(S, 2 * cgnn_fused_grid()) workgroups of 4 waves, a workgroup per subject with a grid
 * stride.  Phase 0 writes W = max(p(A), p(A)^T) into the workgroup's slab of the workspace (pairs of 32 x 32 tiles across
 * the diagonal, exchanged transposed through padded LDS), so that the tree phase reads rows only.  Phase 1 is Prim with
 * restarts: every node outside the tree keeps, in registers, the 64-bit key of its best pair into the tree -- the bits
 * of w above the pair's inverted (i, j) -- so that the integer maximum is the order above and no subnormal is flushed;
 * each of the n steps is a workgroup maximum (lanes, then waves through LDS), one coalesced read of row u of the slab and
 * the relaxation; parent[] stays in LDS.  A workgroup barrier: every decision exists before anything is written.
 * Phase 2, a wave per row: an entry is read, decided (A_ij > 0 and (A_ij > t_s or parent[i] == j or parent[j] == i)) and
 * written by the same lane.  No atomics, nothing depends on the grid: the same bits on every run, for every grid, in
 * place and out of place.
 * workspace: cgnn_ingest_mst_workspace_bytes(S, n) bytes, 16-byte aligned: one slab per workgroup of the launch, not per
 * subject (the answer depends on the device's grid); CGNN_EINVAL (negative) for arguments the call refuses.
 * thresholds: float [S] or NULL.
 * S < 0, n < 1 or S * n >= 2^31 return CGNN_EINVAL and n > CGNN_MST_MAX_NODES returns CGNN_EUNSUPPORTED (a lane owns 4
 * nodes of the tree phase); then S == 0 returns CGNN_OK with nothing launched; then a NULL or misaligned `matrices` or
 * `out`, a misaligned `thresholds`, a NULL or misaligned workspace, a short out_bytes (4 S n n is needed) or
 * workspace_bytes, an `out` that overlaps `matrices` without being equal to it, a workspace that overlaps `matrices` or
 * `out` and thresholds that overlap `out` return CGNN_EINVAL, all before any launch.  Element offsets are 64-bit.  No
 * allocation or synchronisation inside.
 * ------------------------------------------------------------------------------------- */
#ifndef CGNN_MST_H
#define CGNN_MST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_MST_MAX_NODES 1024
int64_t cgnn_ingest_mst_workspace_bytes(int64_t S, int32_t n);
int cgnn_ingest_mst(const float* matrices, int64_t S, int32_t n, const float* thresholds /* [S] or NULL */,
                    void* workspace, int64_t workspace_bytes, float* out, int64_t out_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGNN_MST_H */
