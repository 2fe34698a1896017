/* cgnn_butterworth.h -- part of the C ABI of libcgnn_hip.so (cgnn.h, whose conventions and return codes hold here and
 * which includes this file): the entry points of the Butterworth band-pass.  They are additive: CGNN_ABI_VERSION stays 2.
 *
 * Zero-phase IIR filtering in second-order sections: every column of ts (float [S, T, n]; confounds
 * [S, T, q] are served alike) through scipy.signal.sosfiltfilt with its default padding (padtype="odd", padlen=None),
 * which is nilearn's signal.clean(filter="butterworth") when `sos` is a Butterworth design.
 *   sos        a HOST array of L rows (b0 b1 b2 a0 a1 a2) of doubles, 1 <= L <= CGNN_BUTTER_MAX_SECTIONS, a0 == 1, read
 *              before the call returns.  The entry point derives in fp64 what sosfilt_zi derives: per section
 *              g = (b0 + b1 + b2) / (1 + a1 + a2) and zi = scale (g - b0, b2 - a2 g), scale the product of g over the
 *              earlier sections; and edge = 3 (2 L + 1 - min(#sections with b2 == 0, #sections with a2 == 0)), scipy's
 *              default pad length.  T > edge is required, as scipy requires it.
 *   per column everything in fp64:  d[t] = double(x[t]) - double(x[0]);  the odd extension by `edge` frames at both ends,
 *              2 d[0] - d[edge - e] and 2 d[T-1] - d[2 (T-1) - (e - edge)], formed on load;  the sections forward over
 *              the T + 2 edge frames in transposed direct form II from zi * (the first frame), in the given order:
 *                y = fma(b0, x, z0);  z0 = fma(-a1, y, fma(b1, x, z1));  z1 = fma(-a2, y, b2 * x);
 *              the same backward over the forward outputs from zi * (the last of them); the value between the passes is
 *              never rounded to fp32
 *   add_level  1: out = fl32(w + double(x[0])), for a filter with unit gain at frequency 0 (a low-pass);  0: out = fl32(w),
 *              for one with zero gain there (a high- or band-pass).  The extension commutes with the shift by x[0] and zi
 *              makes a constant input give a constant output, so this is sosfiltfilt(x) in exact arithmetic, and a constant
 *              column comes out as exactly 0.0 (add_level 0) or exactly its value (1): all states are exactly zero.
 *   NaN        anywhere in a column makes that whole column NaN, and no other column of any subject
 *   out        float [S, T, n]; may be `ts` itself (a wave owns all T frames of the columns it writes, forms the right pad
 *              before it stores anything and loads a segment's frames before it stores them), with the same bits; any
 *              other overlap is not checked
 *   workspace  cgnn_ingest_butterworth_workspace_bytes(S, T, n, L) bytes, 16-byte aligned: per wave of the launch a slab
 *              fp64 [T / 48 + (47 + 3 (2 L + 1)) / 8 + 7][2 L][64] of the states at segment boundaries; the count depends
 *              on cgnn_fused_grid() as it is when the call is made
 * One launch on `stream`: a persistent grid of at most 2 * cgnn_fused_grid() workgroups of 4 independent waves over the
 * items (subject, 64 columns), a lane per column: a forward sweep that keeps the 2 L states at segment boundaries only
 * (chunks of 48 real frames from the first real frame on; segments of 8 and of 1 for the pads and the last real frames),
 * then the segments last to first, each formed again in registers from its boundary and run backward (two reads of x).
 * No atomics, nothing depends on the grid: the same bits on every run, for every grid, in place and out of place.
 * L outside 1 .. CGNN_BUTTER_MAX_SECTIONS, a0 != 1, a non-finite coefficient, 1 + a1 + a2 == 0, T <= edge, T < 2,
 * T > 2^30, S < 0, n <= 0, S * n >= 2^31, add_level not 0 or 1, a NULL (sos included), misaligned or short buffer return
 * CGNN_EINVAL before any launch (the byte count: a negative value); S == 0 returns CGNN_OK with nothing launched.  Element
 * offsets are 64-bit.  No allocation or synchronisation inside.
 * ------------------------------------------------------------------------------------- */
#ifndef CGNN_BUTTERWORTH_H
#define CGNN_BUTTERWORTH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_BUTTER_MAX_SECTIONS 8
int64_t cgnn_ingest_butterworth_workspace_bytes(int64_t S, int32_t T, int32_t n, int32_t L);
int cgnn_ingest_butterworth(const float* ts, int64_t S, int32_t T, int32_t n, const double* sos, int32_t L,
                            int32_t add_level, void* workspace, int64_t workspace_bytes, float* out, int64_t out_bytes,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGNN_BUTTERWORTH_H */
