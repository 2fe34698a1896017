/* cgnn_rw.h -- part of the C ABI of libcgnn_hip.so (cgnn.h, whose conventions and return codes hold here and which
 * includes this file): the random-walk structural encoding of a matrix cohort as node features.  It is additive:
 * CGNN_ABI_VERSION stays 2.
 *
 * Random-walk encodings.  matrices: float [S, n, n] and thr: float [S] as for cgnn_ingest_measures.
 * Per subject with matrix A and threshold t, and the existing edge test: e_ij iff i != j, A_ij > t and A_ij > 0
 * (compared as floats; a NaN, a zero or a negative entry is never an edge).  Nothing is symmetrised and rows are what is
 * summed.
 *   a_ij = A_ij where e_ij (1 where e_ij with CGNN_RW_BINARY), else 0
 *   s_i  = sum_j a_ij
 *   P_ij = a_ij / s_i, an exact zero row where s_i == 0
 *   step k (id k - 1):  r_k(i) = ((P)^k)_ii, the probability that a k-step walk from i is back at i
 * This is the definition for asymmetric input too; on a symmetric kept set it is PyG's AddRandomWalkPE (Dwivedi et al.
 * 2022).  Every value lies in [0, 1].
 * Exact facts: r_1 is exactly 0.0 (it is written, not computed); an isolated node's row, a subject without edges and
 * n == 1 are all 0.0; on a bipartite kept set every odd step is exactly 0.0 (every term of every sum has an exact zero
 * factor).  A kept +inf (without CGNN_RW_BINARY, where a weight is never read as a number) makes every value of that
 * subject's columns for k >= 2 NaN; it touches no other subject and no r_1.
 * Arithmetic, u = 2^-24
 *   1  s_i is summed in fp64 in ascending column order and rounded to fp32 once
 *   2  P_ij is one fp32 division
 *   3  M2 = P P, M3 = P M2, M4 = M2 M2: fp32 products on the matrix pipe (v_mfma_f32_16x16x4_f32), k ascending
 *   4  r_k(i) = sum_j (M_a)_ij (M_b)_ji with a = floor(k / 2), b = ceil(k / 2) and M1 = P: every product exact in
 *      fp64, accumulated in fp64 in ascending j, rounded to fp32 once
 *   5  only the products the largest requested step needs are formed: none up to 2, M2 up to 4, M3 up to 6, else all
 *   6  every M and every r_k has the bits it has in the full call: the same bits for every subset and order of the
 *      steps, every run and every grid.  No atomics.
 *   |r_k - fp64 statement| <= 1.01 ((k - 2) n + 2 k + 1) 2^-24 |r_k| + 2^-40 for k >= 2 (DESIGN.md 4.3x derives it).
 * Arguments
 *   steps      HOST array of num_steps distinct ids k - 1, 1 <= num_steps <= CGNN_RW_MAX_STEPS
 *   cols, ldx  as for cgnn_ingest_paths: step steps[m] of node i of subject s is written to
 *              x[(s * n + i) * ldx + cols[m]]; the other columns of x are not touched
 *   flags      0 or CGNN_RW_BINARY
 *   workspace  cgnn_ingest_rw_workspace_bytes(S, n, steps, num_steps) bytes, 16-byte aligned: one set of slabs
 *              [npad][npad] fp32, npad = 96 ceil(n / 96), per WORKGROUP of the launch (0 to 3 of them: M2, M3, M4 as
 *              far as the request needs them).  The count depends on the grid, n and the largest step, and on S only
 *              where S is smaller than the grid; it is 0 for steps up to 2 and workspace may then be NULL.
 * One launch on `stream`: min(S, 2 * cgnn_fused_grid()) persistent workgroups of 4 waves, a workgroup per subject with a
 * grid stride.  P is never stored: it is formed from the matrix rows, the threshold and the fp32 s_i (LDS) as panels are
 * staged.
 * n > CGNN_RW_MAX_NODES, a NULL, misaligned or short buffer, S < 0, n <= 0, S * n >= 2^31, num_steps outside
 * [1, CGNN_RW_MAX_STEPS], an unknown or repeated id, ldx < 1, a column outside [0, ldx), a repeated column or an unknown
 * flag return CGNN_EINVAL before any launch (the byte count: a negative value); S == 0 returns CGNN_OK with nothing
 * launched (buffers are looked at after it).  Element offsets are 64-bit.  No allocation or synchronisation inside.
 * ------------------------------------------------------------------------------------- */
#ifndef CGNN_RW_H
#define CGNN_RW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_RW_MAX_STEPS 8
#define CGNN_RW_MAX_NODES 1024
#define CGNN_RW_BINARY 1
int64_t cgnn_ingest_rw_workspace_bytes(int64_t S, int32_t n, const int32_t* steps, int32_t num_steps);
int cgnn_ingest_rw(const float* matrices, int64_t S, int32_t n, const float* thr, const int32_t* steps,
                   int32_t num_steps, const int32_t* cols, int32_t ldx, int32_t flags, void* workspace,
                   int64_t workspace_bytes, float* x, int64_t x_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGNN_RW_H */
