/* cgnn_activity.h -- part of the C ABI of libcgnn_hip.so (cgnn.h, whose conventions and return codes hold here and which
 * includes this file): regional activity node features from ROI time series.  It is additive: CGNN_ABI_VERSION stays 2.
 *
 * Series features: per subject and column x[0 .. T-1] of ts (float [S, T, n], one row per frame), stated
 * in fp64 on the fp32 inputs:
 *   m = the mean, xc = x - m;  q = sum xc^2;  K = T / 2 (floor);
 *   X_k = sum_t xc[t] e^(-2 pi i k t / T) for k = 1 .. K;  a_k = 2 |X_k| / T;  w_k = 2, but w_K = 1 when T is even;
 *   the band is the bins k_lo .. k_hi, 1 <= k_lo <= k_hi <= K, which the caller derives from its frequencies.
 *   CGNN_ACTIVITY_STD            sqrt(q / (T - 1))
 *   CGNN_ACTIVITY_AUTOCORR1      sum_{t < T-1} xc[t] xc[t+1] / q
 *   CGNN_ACTIVITY_ALFF           the mean of a_k over the band
 *   CGNN_ACTIVITY_FALFF          sum_band a_k / sum_{k = 1 .. K} a_k
 *   CGNN_ACTIVITY_BAND_STD       sqrt(sum_band w_k |X_k|^2 / T / (T - 1)): the sample std of the ideally band-passed column
 *   CGNN_ACTIVITY_BAND_FRACTION  band_std / std
 * A zero denominator gives +0.0; a constant column has xc exactly 0 and is exactly +0.0 in every feature.  A NaN anywhere
 * in a column makes every feature of that column NaN and touches no other column of any subject.
 *   feature_ids  a HOST array of F distinct ids, 1 <= F <= CGNN_ACTIVITY_FEATURES, read before the call returns; feature
 *                feature_ids[f] of node i of subject s goes to out[(s n + i) F + f]
 *   k_lo, k_hi   looked at when an id from CGNN_ACTIVITY_ALFF on (a spectral id) is asked for; k_lo > k_hi is refused always
 *   out          float [S, n, F]
 *   workspace    cgnn_ingest_activity_workspace_bytes(S, T, n, bins) bytes, 16-byte aligned: the table and seven doubles
 *                per column.  bins = 0 without a spectral id; K with CGNN_ACTIVITY_FALFF; else k_hi - k_first + 1, where
 *                k_first = k_lo, less one if k_lo is even (a band's first table column is 16-byte aligned).
 * Launches on `stream`: k_activity_moments always (a workgroup per (subject, 64 columns), grid stride: the fp64 mean, then
 * q and the lag-1 sum in fp64 over a contiguous segment of frames per wave, merged in wave order); with a spectral id
 * k_activity_table before it (cos and sin of a bin in adjacent columns, fp64 cospi / sinpi of the exactly reduced argument
 * ((2 k t) mod 2 T) / T, rounded once) and k_activity_spectrum after it, once over the band and, with CGNN_ACTIVITY_FALFF,
 * once more over 1 .. K: a persistent grid over the items (subject, 64 columns), C = B^T xc on v_mfma_f32_16x16x4_f32
 * with xc = fl32(double(x) - m), bins in chunks of at most 128, |X_k|^2, its root and the sums in fp64 in registers; no
 * coefficient is stored.  No atomics, nothing depends on the grid, and a bin's place in the sums depends on the band
 * alone: the same bits on every run, for every grid and for every subset or order of ids.
 * F outside 1 .. 6, an unknown or repeated id, T < 2, T > 2^30, T > CGNN_ACTIVITY_MAX_FRAMES with a spectral id, S < 0,
 * n <= 0, S * n >= 2^31, k_lo > k_hi, a band outside 1 .. K with a spectral id, a NULL (feature_ids included),
 * misaligned or short buffer return CGNN_EINVAL before any launch (the byte count: a negative value); S == 0 returns
 * CGNN_OK with nothing launched.  Element offsets are 64-bit.  No allocation or synchronisation inside.
 * ------------------------------------------------------------------------------------- */
#ifndef CGNN_ACTIVITY_H
#define CGNN_ACTIVITY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_ACTIVITY_STD 0
#define CGNN_ACTIVITY_AUTOCORR1 1
#define CGNN_ACTIVITY_ALFF 2
#define CGNN_ACTIVITY_FALFF 3
#define CGNN_ACTIVITY_BAND_STD 4
#define CGNN_ACTIVITY_BAND_FRACTION 5
#define CGNN_ACTIVITY_FEATURES 6
#define CGNN_ACTIVITY_MAX_FRAMES 4096 /* the whole-spectrum table [T, 2 (T / 2)] of floats stays at or below 64 MB */
int64_t cgnn_ingest_activity_workspace_bytes(int64_t S, int32_t T, int32_t n, int32_t bins);
int cgnn_ingest_activity(const float* ts, int64_t S, int32_t T, int32_t n, const int32_t* feature_ids, int32_t F,
                         int32_t k_lo, int32_t k_hi, void* workspace, int64_t workspace_bytes, float* out,
                         int64_t out_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGNN_ACTIVITY_H */
