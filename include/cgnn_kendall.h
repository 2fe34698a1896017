/* cgnn_kendall.h -- part of the C ABI of libcgnn_hip.so (cgnn.h, whose conventions and return codes hold here and which
 * includes this file): Kendall's tau-b of ROI time series from their mid-ranks (cgnn_rank.h).  It is additive:
 * CGNN_ABI_VERSION stays 2.
 *
 * Kendall's tau.  ranks: float [U, L, n], what cgnn_ingest_rank writes: per unit and column the
 * mid-ranks over the unit's kept frames, exactly 0.0 at a censored frame.  Over the pairs k = (s < t) of kept frames of a
 * unit, with a_ik = sign(x_si - x_ti) in {-1, 0, 1}, G = A^T A is an integer matrix:
 *   G_ij = concordant - discordant pairs of columns i and j            (i != j)
 *   G_ii = L_u (L_u - 1) / 2 - n1_i, the pairs not tied in column i    (L_u kept frames, n1_i tied pairs)
 *   tau_b(i, j) = G_ij / sqrt(G_ii G_jj)
 * The input is defined totally, so nothing is undefined for data that no ranking wrote:
 *   key        a value v reads as the 16-bit key clamp(rint(2 v), 0, 65535); comparisons are those of the keys, and so,
 *              for ranks, the ranking's: IEEE order, -0.0 == +0.0, +-inf ordinary values, subnormals distinct
 *   censored   a frame whose key in COLUMN 0 of its unit is 0 is censored for every column of the unit: it takes part in
 *              no pair and its values are never compared (the ranking writes 0.0 in every column of a censored frame
 *              and at least 1 in every column of a kept one); frames are not censored by other columns' keys
 *   NaN        a NaN in a kept frame marks its column (in column 0 it does not censor the frame)
 * counts (int32 [U, n, n])
 *   1  G is exact and bit-symmetric; G_ii >= 0; a unit with fewer than two kept frames is all zeros
 *   2  a marked column has G_ii = -1 and zeros elsewhere in its row and column of that unit; no other column and no other
 *      unit is touched
 * out (float [U, n, n])
 *   3  tau_ij = fp32( (double)G_ij / sqrt((double)G_ii * (double)G_jj) ): the product is below 2^46 and exact, the square
 *      root and the quotient are IEEE fp64, and the value is rounded to fp32 once; |tau| <= 1
 *   4  the diagonal is exactly 1 where G_ii > 0; a column that is constant over its kept frames (G_ii == 0) is an exact
 *      zero row and column, diagonal included: cgnn_ingest_corr's constant-ROI rule (scipy.stats.kendalltau gives NaN)
 *   5  a marked column is NaN in its row and column of its unit
 *   6  bit-symmetric; absolute != 0 gives |tau|
 * The same bits on every run and for every grid: the counts are integer sums, which no order changes.  No atomics, no
 * workspace.
 * Arguments
 *   counts     int32 [U, n, n] or NULL (counts_bytes 0)
 *   out        float [U, n, n] or NULL (out_bytes 0).  At least one of the two is given.  With `out` alone the counts
 *              are written into out's own bytes and normalised in place: there is no second cohort-sized buffer.
 * Launches on `stream`: k_kendall_counts, a persistent grid of at most 2 workgroups of 4 waves per cgnn_fused_grid() unit
 * over the items (unit, tile pair bi <= bj of 96 columns); then, if `out` is given, k_kendall_tau, a workgroup per unit
 * with a grid stride.
 * L < 2, L > CGNN_KENDALL_MAX_FRAMES, a NULL `ranks`, both outputs NULL, a misaligned or short buffer, U < 0, n <= 0,
 * U * n >= 2^31 or n * n >= 2^31 return CGNN_EINVAL before any launch (the byte count: a negative value); U == 0 returns
 * CGNN_OK with nothing launched (buffers are looked at after it).  Element offsets are 64-bit.  No allocation or
 * synchronisation inside.
 * ------------------------------------------------------------------------------------- */
#ifndef CGNN_KENDALL_H
#define CGNN_KENDALL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_KENDALL_MAX_FRAMES 4096
int cgnn_ingest_kendall(const float* ranks, int64_t U, int32_t L, int32_t n, int32_t absolute, int32_t* counts,
                        int64_t counts_bytes, float* out, int64_t out_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGNN_KENDALL_H */
