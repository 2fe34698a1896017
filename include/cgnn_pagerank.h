/* cgnn_pagerank.h -- part of the C ABI of libcgnn_hip.so (cgnn.h, whose conventions and return codes hold here and which
 * includes this file): PageRank centrality of a matrix cohort as node features.  It is additive: CGNN_ABI_VERSION stays 2.
 *
 * PageRank.  matrices: float [S, n, n] and thr: float [S] as for cgnn_ingest_measures.  Per subject
 * with matrix A and threshold t, and the existing edge test: e_ij iff i != j, A_ij > t and A_ij > 0 (compared as floats;
 * a NaN, a zero or a negative entry is never an edge).  Nothing is symmetrised.  Entry (i, j) is an edge j -> i.
 *   w_ij = A_ij (CGNN_PAGERANK_WEIGHTED) or 1 (CGNN_PAGERANK) where e_ij, else 0
 *   c_j = sum_i w_ij, the out-strength of node j: a column sum, added in fp64 in a fixed order
 *   node j is dangling iff c_j == 0; its mass is spread uniformly
 *   x is the solution of  x_i = d (sum_j w_ij x_j / c_j + (sum_{j dangling} x_j) / n) + (1 - d) / n,  sum_i x_i = 1
 * Arithmetic
 *   Everything after the fp32 edge test is fp64; the result is rounded to fp32 once.  With T(x) the right-hand side
 *   above, a step is TWO products, x_k = T(T(x_(k-1))), from x_0 = 1 / n.  The iteration stops at the first step k with
 *   ||x_k - x_(k-1)||_1 <= (1 - d) 2^-42 (a step contracts at rate d^2, which then gives ||x_k - x||_1 <= 2^-42), at the
 *   latest after K_max(d) = ceil(43 ln 2 / -ln d) + 2 steps (2 for d == 0).  The change of step K_max is at most
 *   2 (1 + d) d^(2 K_max - 1) <= 2^-84, so in exact arithmetic the cap is never reached; a subject that reaches it is
 *   written all the same.  (With one product a step, a bipartite graph such as a star, whose error alternates in sign
 *   and shrinks by exactly d, would run past K_max before its change met the rule.)  No atomics;
 *   no order of summation and no assignment of work depends on the grid or the run: the same bits on every run, for
 *   every grid, and for every subset and order of the two measures.
 *   A subject without kept entries is exactly (float)(1.0 / n) everywhere.  A kept +inf makes every value of that
 *   subject's CGNN_PAGERANK_WEIGHTED column NaN and touches nothing else; CGNN_PAGERANK does not see weights.
 * Arguments
 *   measures   HOST array of num_measures distinct ids, 1 <= num_measures <= CGNN_NUM_PAGERANK_MEASURES
 *   cols, ldx  as for cgnn_ingest_paths: measure m of node i of subject s is written to
 *              x[(s * n + i) * ldx + cols[m]]; the other columns of x are not touched
 *   damping    d, finite, 0 <= d <= CGNN_PAGERANK_MAX_DAMPING
 *   workspace  cgnn_ingest_pagerank_workspace_bytes(S, n, measures, num_measures) bytes, 16-byte aligned.  The one
 *              kernel keeps its state in LDS: the count is 0 today and workspace may then be NULL.
 *   iterations int32 [S] on the device or NULL: the number of steps of the slowest of the measures asked for (0 for a
 *              weighted column that a kept +inf made NaN, 1 for a subject without kept entries)
 * One launch on `stream`: min(S, w * cgnn_fused_grid()) workgroups of 8 waves (w = what the LDS of a CU admits, at
 * most 4), a workgroup per subject with a grid stride.  A subject's kept entries are compacted into LDS when they fit
 * beside the fp64 vectors (columns as 16-bit, weights as floats: n <= CGNN_PAGERANK_MAX_NODES); when only the columns
 * fit, CGNN_PAGERANK runs on them and CGNN_PAGERANK_WEIGHTED reads the matrix rows with the edge test in flight; when
 * neither fits both do.
 * n > CGNN_PAGERANK_MAX_NODES, a NULL, misaligned or short buffer, S < 0, n <= 0, S * n >= 2^31, num_measures outside
 * [1, CGNN_NUM_PAGERANK_MEASURES], an unknown or repeated id, ldx < 1, a column outside [0, ldx) or a repeated column, or
 * a damping that is not a finite number of [0, CGNN_PAGERANK_MAX_DAMPING] return CGNN_EINVAL before any launch (the
 * byte count: a negative value); S == 0 returns CGNN_OK with nothing launched (buffers are looked at after it).
 * Element offsets are 64-bit.  No allocation or synchronisation inside.
 * ------------------------------------------------------------------------------------- */
#ifndef CGNN_PAGERANK_H
#define CGNN_PAGERANK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_PAGERANK 0
#define CGNN_PAGERANK_WEIGHTED 1
#define CGNN_NUM_PAGERANK_MEASURES 2
#define CGNN_PAGERANK_MAX_NODES 1024
#define CGNN_PAGERANK_MAX_DAMPING 0.99
int64_t cgnn_ingest_pagerank_workspace_bytes(int64_t S, int32_t n, const int32_t* measures, int32_t num_measures);
int cgnn_ingest_pagerank(const float* matrices, int64_t S, int32_t n, const float* thr, const int32_t* measures,
                         int32_t num_measures, const int32_t* cols, int32_t ldx, double damping, void* workspace,
                         int64_t workspace_bytes, float* x, int64_t x_bytes, int32_t* iterations,
                         int64_t iterations_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGNN_PAGERANK_H */
