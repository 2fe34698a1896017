/* cgnn_rank.h -- part of the C ABI of libcgnn_hip.so (cgnn.h, whose conventions and return codes hold here and which
 * includes this file): the mid-ranks of ROI time series, what stands in front of cgnn_ingest_corr for a Spearman
 * correlation.  It is additive: CGNN_ABI_VERSION stays 2.
 *
 * Ranks.  ts: float [S, T, n], window and stride as for cgnn_ingest_corr, which defines the units:
 * unit u = s W + w is frames [w stride, w stride + L) of subject s; L = T and W = 1 for window == 0.  Per unit and
 * column, over the unit's kept frames K (every frame of the unit without a mask), with v_t the column's values:
 *   rank(t) = 1 + #{t' in K : v_t' < v_t} + (#{t' in K : v_t' == v_t} - 1) / 2        for t in K
 * the mid-rank: scipy.stats.rankdata(method="average").  Spearman's rho of a unit is cgnn_ingest_corr of the output.
 * Exact facts
 *   1  < and == are the IEEE comparisons of the fp32 values, taken on order-preserving integer keys: -0.0 == +0.0,
 *      +-inf are ordinary values, and subnormals are distinct values that are never flushed
 *   2  a NaN in a kept frame makes every kept frame of that column of that unit NaN (scipy's nan_policy="propagate")
 *      and touches no other column and no other unit
 *   3  a censored frame is written as exactly 0.0 and its value is never looked at: a NaN, an Inf or 1e30 there changes
 *      no bit of the output
 *   4  a column that is constant over its L_u kept frames is (L_u + 1) / 2 there: cgnn_ingest_corr's constant-ROI rule
 *      then gives it an exact zero row and column
 *   5  every value is a multiple of 1/2 and at most CGNN_RANK_MAX_FRAMES: exact in fp32.  The output is the fp32 cast of
 *      the statement, bit for bit, on every run and for every grid.  No atomics, no workspace.
 * Arguments
 *   keep       (masked form) uint8 [S, T], non-zero: the frame is kept; keep_bytes >= S T
 *   out        float [U, L, n], U = S W: unit u's frame t is row u L + t.  Without a window that is [S, T, n], and out
 *              may then be `ts` itself, with the same bits: a workgroup holds all L frames of its columns in LDS before
 *              it writes the first.  Any other overlap is not checked.
 * One launch on `stream`: a persistent grid of at most 4 workgroups of 4 waves per cgnn_fused_grid() unit (as many as
 * the LDS of a CU holds: two for L > 1024, one for L > 2048) over the items (unit, 4 adjacent columns).  The item's columns are staged in
 * LDS as 64-bit pairs (key << 32 | frame), padded to a power of two with a key above every number's, which a censored
 * frame gets too; a wave sorts a column (a bitonic network, four strides per pass over LDS), finds the runs of equal keys
 * by neighbour comparison and two scans, and the workgroup stores the item's row segments.  8 P bytes of LDS per column,
 * P = L rounded up to a power of two: 128 KB an item at L = 4096.
 * L > CGNN_RANK_MAX_FRAMES, a NULL, misaligned or short buffer, S < 0, n <= 0, T < 2, window outside {0} u [2, T],
 * stride < 1 with a window, U * n >= 2^31 or n * n >= 2^31 return CGNN_EINVAL before any launch (the byte count: a negative
 * value); S == 0 returns CGNN_OK with nothing launched (buffers are looked at after it).  Element offsets are 64-bit.
 * No allocation or synchronisation inside.
 * ------------------------------------------------------------------------------------- */
#ifndef CGNN_RANK_H
#define CGNN_RANK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_RANK_MAX_FRAMES 4096
int cgnn_ingest_rank(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride, float* out,
                     int64_t out_bytes, void* stream);
int cgnn_ingest_rank_masked(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride,
                            const uint8_t* keep, int64_t keep_bytes, float* out, int64_t out_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGNN_RANK_H */
