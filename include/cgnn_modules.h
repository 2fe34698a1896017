/* cgnn_modules.h -- part of the C ABI of libcgnn_hip.so (cgnn.h, whose conventions and return codes hold here and which
 * includes this file): module-aware node measures of a matrix cohort from a partition of its ROIs.  It is additive:
 * CGNN_ABI_VERSION stays 2.
 *
 * Module measures.  matrices: float [S, n, n] and thr: float [S] as for cgnn_ingest_measures.  Per
 * subject with matrix A and threshold t, and the existing edge test: e_ij iff i != j, A_ij > t and A_ij > 0 (compared
 * as floats; a NaN is never an edge).  Nothing is symmetrised: rows are what is summed.
 *   a_ij = A_ij, b_ij = 1 where e_ij, else 0
 *   modules    int32 [n] on the DEVICE: c_j in 0 .. M - 1, the module of ROI j; one partition for the whole cohort
 *   k_i(m) = sum_{j: c_j = m} b_ij,  s_i(m) = sum_{j: c_j = m} a_ij  (lane l of a wave adds columns l, l + 64, ..
 *            ascending; the lanes are folded in a fixed order)
 *   k_i = sum_m k_i(m),  s_i = sum_m s_i(m),  kappa_i = k_i(c_i),  sigma_i = s_i(c_i)
 * Measures
 *   CGNN_MODULE_PARTICIPATION           1 - sum_m (k_i(m) / k_i)^2; 0 if k_i == 0
 *   CGNN_MODULE_WEIGHTED_PARTICIPATION  1 - sum_m (s_i(m) / s_i)^2; 0 if s_i == 0
 *   CGNN_MODULE_ZSCORE                  (kappa_i - mean) / std over the nodes of module c_i, std the population
 *                                       standard deviation; 0 if all kappa of that module compare equal (that test, not
 *                                       std == 0: the mean of equal doubles need not be that double)
 *   CGNN_MODULE_WEIGHTED_ZSCORE         the same on sigma_i
 *   CGNN_MODULE_DIVERSITY               -sum_{m: p != 0} p ln p / ln M with p = s_i(m) / s_i; 0 if s_i == 0 or M == 1
 * Arithmetic
 *   Everything after the fp32 edge test is fp64 in a fixed order (the binary sums are exact integers) and every
 *   result is rounded to fp32 once.  No atomics; no order of summation and no assignment of work depends on the
 *   grid, the run or the wave that took a row: the same bits on every run and for every grid.
 *   A kept +inf follows the formulas: NaN in that row's weighted columns and in the weighted z-scores of its module
 *   (unless every sigma of the module compares equal); the binary columns do not see weights.
 * Network profile
 *   profile    float [S, n, M] or NULL: profile[s][i][m] = s_i(m) -- a node's kept strength into every module.
 *   profile_flags  CGNN_MODULE_PROFILE_BINARY: k_i(m) instead.  CGNN_MODULE_PROFILE_NORMALIZE: divided by the row's
 *              total (s_i, or k_i), an exact 0 row where that total is 0.
 * Arguments
 *   measures   HOST array of num_measures distinct ids, 0 <= num_measures <= CGNN_NUM_MODULE_MEASURES; 0 (measures,
 *              cols and x may then be NULL) when only `profile` is asked for.  At least one of x and profile.
 *   cols, ldx  as for cgnn_ingest_paths: measure m of node i of subject s is written to
 *              x[(s * n + i) * ldx + cols[m]]; the other columns of x are not touched
 *   workspace  cgnn_ingest_modules_workspace_bytes(S, n, measures, num_measures) bytes, 16-byte aligned.  The one
 *              kernel keeps its state in LDS and registers: the count is 0 today and workspace may then be NULL.
 *   modules    the kernel TRUSTS 0 <= modules[j] < M (the caller has checked it).  An id outside that range is
 *              SKIPPED, not clamped: the column belongs to no module (it adds to no k_i(m), s_i(m), k_i or s_i), and a
 *              row whose own id is outside has kappa = sigma = 0 and z-scores 0.  Nothing is written outside the
 *              row's own outputs either way.
 * One launch on `stream`: min(S, w * cgnn_fused_grid()) workgroups of 8 waves (w = what the LDS of a CU admits, at
 * most 4), a workgroup per subject with a grid stride, a wave per row with the row in registers (lane l holds columns
 * l, l + 64, ..: n <= CGNN_MODULE_MAX_NODES).  The z-scores take a second phase per subject over kappa and sigma in
 * LDS, which runs only when one of them is asked for.
 * n > CGNN_MODULE_MAX_NODES, a NULL, misaligned or short buffer, S < 0, n <= 0, S * n >= 2^31, num_measures outside
 * [0, CGNN_NUM_MODULE_MEASURES], an unknown or repeated id, ldx < 1, a column outside [0, ldx) or a repeated column,
 * M < 1, M > CGNN_MODULE_MAX, M > n, unknown bits in profile_flags, or neither x nor profile return CGNN_EINVAL before
 * any launch (the byte count: a negative value); S == 0 returns CGNN_OK with nothing launched (buffers are looked at
 * after it).  Element offsets are 64-bit.  No allocation or synchronisation inside.
 * ------------------------------------------------------------------------------------- */
#ifndef CGNN_MODULES_H
#define CGNN_MODULES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_MODULE_PARTICIPATION 0
#define CGNN_MODULE_WEIGHTED_PARTICIPATION 1
#define CGNN_MODULE_ZSCORE 2
#define CGNN_MODULE_WEIGHTED_ZSCORE 3
#define CGNN_MODULE_DIVERSITY 4
#define CGNN_NUM_MODULE_MEASURES 5
#define CGNN_MODULE_MAX 64
#define CGNN_MODULE_MAX_NODES 1024
#define CGNN_MODULE_PROFILE_BINARY 1
#define CGNN_MODULE_PROFILE_NORMALIZE 2
int64_t cgnn_ingest_modules_workspace_bytes(int64_t S, int32_t n, const int32_t* measures, int32_t num_measures);
int cgnn_ingest_modules(const float* matrices, int64_t S, int32_t n, const float* thr, const int32_t* modules,
                        int32_t M, const int32_t* measures, int32_t num_measures, const int32_t* cols, int32_t ldx,
                        void* workspace, int64_t workspace_bytes, float* x, int64_t x_bytes, float* profile,
                        int64_t profile_bytes, int32_t profile_flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGNN_MODULES_H */
