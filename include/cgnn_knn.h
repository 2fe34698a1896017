/* cgnn_knn.h -- part of the C ABI of libcgnn_hip.so (cgnn.h, whose conventions and return codes hold here and which
 * includes this file): the k-nearest-neighbour sparsification of a matrix cohort.  It is additive: CGNN_ABI_VERSION
 * stays 2.
 *
 * k-NN sparsification: every ROI keeps its k strongest positive connections, the picks are symmetrised
 * as `mode` says, and what is dropped becomes an exact +0.0 -- so that cgnn_ingest_count / _fill / _measures / _paths /
 * _wpaths at the threshold 0.0 see exactly the k-NN graph.  matrices: float [S, n, n], contiguous, any sign, not
 * necessarily symmetric.  Per subject with matrix A:
 *   candidates P_i = { j != i : A_ij > 0 }, p_i = |P_i|: a NaN is not positive, +inf is; the diagonal is never one
 *   order      within a row j comes before j' iff A_ij > A_ij', or A_ij == A_ij' and j < j' (the stable descending sort)
 *   picks      D_i = the first min(k, p_i) members of P_i in that order; d_ij iff j in D_i.  A row gets EXACTLY
 *              min(k, p_i) picks: a tie class that straddles the cut is cut by column.  (Not the "strictly above the
 *              rank-k value" rule of cgnn_ingest_select: the minimum degree is what this call is for.)
 *   mode       CGNN_KNN_DIRECTED  kept_ij = d_ij
 *              CGNN_KNN_UNION     kept_ij = d_ij or (d_ji and A_ij > 0)
 *              CGNN_KNN_MUTUAL    kept_ij = d_ij and d_ji
 *   out        float [S, n, n]: out_ij = the bits of A_ij where kept_ij, +0.0 elsewhere (the diagonal and every NaN
 *              too).  out may be `matrices` itself, with the same bits; any other overlap is refused.
 * A row's picks are two numbers, the value v_i and the column c_i of its last pick (+inf and -1 for a row without one):
 *   d_ij  iff  A_ij > 0 and (A_ij > v_i or (A_ij == v_i and j <= c_i)).
 * One launch on `stream`: min(S, 2 * cgnn_fused_grid()) workgroups of 8 waves, a workgroup per subject with a grid
 * stride.  Phase 1, a wave per row with the row in registers: the bits of a positive float order as the floats do, so
 * v_i is the candidate of descending rank min(k, p_i) - 1 by an exact radix select on those bits (four 8-bit digits from
 * the top, a histogram per wave in LDS, the prefix sum over its bins in registers), and c_i comes from ballots and lane
 * prefixes over the tie class; (v, c) stay in LDS.  A workgroup barrier.  Phase 2: DIRECTED masks row by row; UNION and MUTUAL give every wave pairs of 32 x 32
 * tiles (bi, bj) and (bj, bi), bi <= bj, which it loads whole, exchanges transposed through padded LDS of its own,
 * decides and stores -- no entry is read after another wave may have written it.  No atomics on global memory (the
 * histogram counts are integer adds in LDS, whose order does not matter), nothing depends on the grid: the same bits on every run, for every grid, in place and out of place.
 * S < 0, n < 1, k < 0, a mode other than the three or S * n >= 2^31 return CGNN_EINVAL and n > CGNN_KNN_MAX_NODES
 * returns CGNN_EUNSUPPORTED (the row lives in 16 registers per lane); then S == 0 returns CGNN_OK with nothing launched;
 * then a NULL or misaligned pointer, a short out_bytes (4 S n n is needed) or an `out` that overlaps `matrices` without
 * being equal to it return CGNN_EINVAL, all before any launch.  Element offsets are 64-bit.  No allocation or
 * synchronisation inside.
 * ------------------------------------------------------------------------------------- */
#ifndef CGNN_KNN_H
#define CGNN_KNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_KNN_DIRECTED 0
#define CGNN_KNN_UNION 1
#define CGNN_KNN_MUTUAL 2
#define CGNN_KNN_MAX_NODES 1024
int cgnn_ingest_knn(const float* matrices, int64_t S, int32_t n, int64_t k, int32_t mode, float* out, int64_t out_bytes,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGNN_KNN_H */
