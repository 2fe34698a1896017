/* cgnn_core.h -- part of the C ABI of libcgnn_hip.so (cgnn.h, whose conventions and return codes hold here and which
 * includes this file): the core decomposition of a matrix cohort as node features.  It is additive: CGNN_ABI_VERSION
 * stays 2.
 *
 * Cores.  matrices: float [S, n, n] and thr: float [S] as for cgnn_ingest_measures.  Per subject with
 * matrix A and threshold t, and the existing edge test: e_ij iff i != j, A_ij > t and A_ij > 0 (compared as floats; a
 * NaN, a zero or a negative entry is never an edge).  Nothing is symmetrised and rows are what is summed.
 *   b_ij = 1 and a_ij = A_ij where e_ij, else 0
 *   for a node set H:  k_i(H) = sum_{j in H} b_ij,  s_i(H) = sum_{j in H} a_ij;  both are monotone in H
 *   the generalised core value (Batagelj & Zaversnik) of p = k or p = s:
 *     c(i) = max over H containing i of min_{u in H} p_u(H)
 *   which peeling in rounds computes, along with a layer:  L = 0, r = 0, every node alive;  while a node is alive:
 *     r += 1;  L = max(L, min over alive u of p_u(alive));  every alive u with p_u(alive) <= L is removed TOGETHER,
 *     with value L and layer r.
 *   p = k: the value is the k-core number k_i and the layer r_i the onion layer (Hebert-Dufresne et al.); on a
 *   symmetric kept set these are networkx.core_number and networkx.onion_layers, an isolated node in layer 1 of core 0.
 *   p = s: the value sigma_i is the s-core level (BCT's score_wu) and the layer is rho_i.
 *   CGNN_CORE_CORENESS     k_i / (n - 1), 0 for n == 1: one correctly rounded fp32 quotient of two exact integers;
 *                          pointwise at most the degree
 *   CGNN_CORE_ONION_LAYER  r_i / n, formed the same way
 *   CGNN_CORE_S_CORENESS   sigma_i / (max_i s_i(all) + 1e-8), the strength's normaliser; pointwise at most the strength
 * Arithmetic
 *   k and r are exact integers.  Everything of s after the fp32 edge test is fp64, the result is rounded to fp32 once.
 *   Every s_u(alive) is formed anew from the subject's kept entries: from 0.0, the row's kept entries of alive columns
 *   in ascending column order.  A removed neighbour is left out of an otherwise unchanged order (it would add +0.0);
 *   nothing is ever subtracted from a running sum, so the rounded s is still monotone in H and the peeling computes
 *   exactly its generalised core.  No atomics; no order of summation and no assignment of work depends on the grid or
 *   the run: the same bits on every run, for every grid, and for every subset and order of the three measures.
 *   A kept +inf makes every value of that subject's CGNN_CORE_S_CORENESS column NaN and touches nothing else.
 * Arguments
 *   measures   HOST array of num_measures distinct ids, 1 <= num_measures <= CGNN_NUM_CORE_MEASURES
 *   cols, ldx  as for cgnn_ingest_paths: measure m of node i of subject s is written to
 *              x[(s * n + i) * ldx + cols[m]]; the other columns of x are not touched
 *   workspace  cgnn_ingest_cores_workspace_bytes(S, n, measures, num_measures) bytes, 16-byte aligned.  The one kernel
 *              keeps its state in LDS and registers: the count is 0 today and workspace may then be NULL.
 *   levels     int32 [S, n, 3] on the device or NULL: column 0 is k_i and column 1 is r_i, written when
 *              CGNN_CORE_CORENESS or CGNN_CORE_ONION_LAYER is asked for; column 2 is rho_i, written when
 *              CGNN_CORE_S_CORENESS is.  A column whose pass did not run holds -1, and so does column 2 of a subject
 *              whose CGNN_CORE_S_CORENESS is NaN.
 * One launch on `stream`: min(S, w * cgnn_fused_grid()) workgroups of 8 waves (w = what the LDS of a CU admits, at
 * most 4), a workgroup per subject with a grid stride.  A subject's adjacency bitset lives in LDS (n <=
 * CGNN_CORE_MAX_NODES); for CGNN_CORE_S_CORENESS its kept entries are compacted beside it (row offsets, columns as
 * 16-bit, weights as floats) when they fit, else they are read from the matrix rows; which of the two depends on n and
 * the subject's kept count alone.
 * n > CGNN_CORE_MAX_NODES, a NULL, misaligned or short buffer, S < 0, n <= 0, S * n >= 2^31, num_measures outside
 * [1, CGNN_NUM_CORE_MEASURES], an unknown or repeated id, ldx < 1, a column outside [0, ldx) or a repeated column return
 * CGNN_EINVAL before any launch (the byte count: a negative value); S == 0 returns CGNN_OK with nothing launched (buffers
 * are looked at after it).  Element offsets are 64-bit.  No allocation or synchronisation inside.
 * ------------------------------------------------------------------------------------- */
#ifndef CGNN_CORE_H
#define CGNN_CORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_CORE_CORENESS 0
#define CGNN_CORE_ONION_LAYER 1
#define CGNN_CORE_S_CORENESS 2
#define CGNN_NUM_CORE_MEASURES 3
#define CGNN_CORE_MAX_NODES 1024
int64_t cgnn_ingest_cores_workspace_bytes(int64_t S, int32_t n, const int32_t* measures, int32_t num_measures);
int cgnn_ingest_cores(const float* matrices, int64_t S, int32_t n, const float* thr, const int32_t* measures,
                      int32_t num_measures, const int32_t* cols, int32_t ldx, void* workspace, int64_t workspace_bytes,
                      float* x, int64_t x_bytes, int32_t* levels, int64_t levels_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGNN_CORE_H */
