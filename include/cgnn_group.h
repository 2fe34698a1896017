/* cgnn_group.h -- part of the C ABI of libcgnn_hip.so (cgnn.h, whose conventions and return codes hold here and which
 * includes this file): the group-level matrix of a matrix cohort and the mask that gives every subject the group's edge
 * set.  It is additive: CGNN_ABI_VERSION stays 2.
 *
 * Group-consensus edges: the edge set is chosen once, on a group matrix G [n, n], and every subject
 * carries that topology with its own weights.  matrices: float [S, n, n], contiguous, any sign, not necessarily
 * symmetric; a subject is a *unit*.
 *
 * cgnn_ingest_group: out = G, float [n, n].
 *   among      bytes [S] or NULL: unit s is *included* iff among is NULL or among[s] != 0.  An excluded unit's matrix is
 *              never read: whatever it holds (NaN, Inf, 1e30) changes no bit.  N is the number of included units.
 *   the sum    per entry (i, j), in fp64, in this order, which depends on neither the grid nor the run: the units are cut
 *              into slices of CGNN_GROUP_SLICE consecutive units, slice c holding the units c * CGNN_GROUP_SLICE ..
 *              min(S, (c + 1) * CGNN_GROUP_SLICE) - 1; a slice's partial starts at 0.0 and adds the terms of its included
 *              units in ascending order; the partials are folded in ascending slice order from 0.0.  N is the sum of
 *              the slices' counts, an exact integer.
 *   CGNN_GROUP_MEAN         the term of unit s is double(A_sij);  G_ij = float(sum / N)
 *   CGNN_GROUP_FISHER_MEAN  the term is atanh(double(A_sij));     G_ij = float(tanh(sum / N)), fp64 atanh and tanh
 *   CGNN_GROUP_CONSISTENCY  the term is 1 if i != j and A_sij > thr[s] and A_sij > 0 (the edge predicate of
 *                           cgnn_ingest_count, both comparisons strict, a NaN fails both), else 0: an exact integer
 *                           count;                                G_ij = float(count / N)
 *   One fp64 division and one rounding to fp32 per entry.  Nothing is special-cased: N == 0 gives NaN everywhere (0 / 0);
 *   a NaN in an included unit makes that entry NaN (not under CONSISTENCY, where a NaN is not an edge); +inf and -inf in
 *   the same entry give NaN; |r| == 1 goes through atanh as +-inf; the diagonal is reduced like any entry, except that
 *   CONSISTENCY counts nothing there (0 / N: 0, and NaN for N == 0); a bit-symmetric cohort gives a bit-symmetric G.
 *   thr        float [S], the units' own thresholds, with CGNN_GROUP_CONSISTENCY; NULL with the other two statistics.
 *   workspace  cgnn_ingest_group_workspace_bytes(S, n) bytes, 16-byte aligned: the partials, fp64 [slices][n * n], and the
 *              slices' counts, fp64 [slices]; it depends on S and n only and is 2 / CGNN_GROUP_SLICE = 1 / 32 of the cohort.
 *              CGNN_EINVAL (negative) for sizes the call refuses; 0 for S == 0, and the workspace may then be NULL.
 *   Two launches on `stream`.  The first streams the cohort once: the work items are (slice, block of 1024 consecutive
 *   entries), walked with a grid stride by at most 8 * cgnn_fused_grid() workgroups of 4 waves; a lane owns 4 consecutive
 *   entries with their fp64 accumulators in registers and reads a unit's 4 entries as one 16-byte load at element
 *   alignment (a unit's base is only 4-byte aligned when n * n is odd); `among` and the edge predicate are tests inside
 *   the loop.  The second folds the partials and the counts, divides and rounds, a thread per entry.  No atomics, no
 *   read-back, no cohort-sized temporary, no bound on n beyond n * n < 2^31.
 *   S < 0, n < 1, an unknown statistic, S * n >= 2^31 or n * n >= 2^31, thr given or missing against the statistic, a
 *   NULL `out`, a NULL `matrices` or workspace where S > 0, a pointer that is not 4-byte aligned (the workspace: 16-byte),
 *   a short out_bytes (4 n n is needed) or workspace_bytes, an `out` that overlaps `matrices` without starting where they
 *   do, and a workspace, thr or among that overlaps `out` or (the workspace) `matrices` return CGNN_EINVAL, all before any
 *   launch.  S == 0 is valid: the statistic of no units is the all-NaN matrix, which the second launch writes.
 *
 * cgnn_ingest_group_mask: out = the cohort masked to the group's edge set, float [S, n, n].
 *   E          = { (i, j) : i != j and group_ij > thr[0] and group_ij > 0 }, the edge predicate on the group matrix at
 *              the one threshold thr [1], which is read on the device.  A NaN group entry is never an edge.
 *   out_sij    the bits of A_sij if (i, j) is in E and A_sij > 0; +0.0 otherwise (the diagonal, every NaN and -0.0 too) --
 *              so that cgnn_ingest_count / _fill / _measures / _paths / _wpaths / _modules / _pagerank at the threshold
 *              0.0 see exactly the group's edges that are positive in the subject.
 *   One launch on `stream`: the cohort is copied once under that predicate, in the order a copy walks it.  The work
 *   items are (unit, span of 4 blocks of 1024 consecutive entries; a unit of at most 8 blocks is one item), walked with a
 *   grid stride by at most 8 * cgnn_fused_grid() workgroups of 4 waves; a lane reads 16 bytes of the unit and of the
 *   group matrix (n * n floats, which stay in cache) per block, all of an item's loads in flight together, and writes
 *   after its last load.  Every entry is read and written by the same lane: out may be `matrices` itself, with the same
 *   bits.  No atomics, nothing depends on the grid.
 *   S < 0, n < 1, S * n >= 2^31 or n * n >= 2^31 return CGNN_EINVAL; then S == 0 returns CGNN_OK with nothing launched;
 *   then a NULL or misaligned pointer, a short out_bytes (4 S n n is needed), an `out` that overlaps `matrices` without
 *   being equal to it and a `group` or `thr` that overlaps `out` return CGNN_EINVAL, all before any launch.
 * Element offsets are 64-bit.  No allocation or synchronisation inside.
 * ------------------------------------------------------------------------------------- */
#ifndef CGNN_GROUP_H
#define CGNN_GROUP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_GROUP_MEAN 0
#define CGNN_GROUP_FISHER_MEAN 1
#define CGNN_GROUP_CONSISTENCY 2
#define CGNN_GROUP_SLICE 64
int64_t cgnn_ingest_group_workspace_bytes(int64_t S, int32_t n);
int cgnn_ingest_group(const float* matrices, int64_t S, int32_t n, int32_t statistic, const float* thr /* [S] or NULL */,
                      const uint8_t* among /* [S] or NULL */, void* workspace, int64_t workspace_bytes,
                      float* out /* [n, n] */, int64_t out_bytes, void* stream);
int cgnn_ingest_group_mask(const float* matrices, int64_t S, int32_t n, const float* group /* [n, n] */,
                           const float* thr /* [1] */, float* out, int64_t out_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGNN_GROUP_H */
