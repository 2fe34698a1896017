"""The host statement of ``connectome_gnn_amd.ingest.series_features`` in float64, the same statement on
the operands the device holds, and the seeded frames and cases its tests share.

Statement, per subject and column ``x[0 .. T-1]`` (fp32 in, everything else fp64): ``m`` the mean, ``xc = x - m``,
``q = sum xc^2``, ``X_k = sum_t xc[t] exp(-2 pi i k t / T)`` for ``k = 1 .. K = T // 2``, ``w_k = 2`` but ``w_K = 1`` for
even ``T``, the band ``k_lo = max(1, ceil(lo T t_r)) .. k_hi = min(K, floor(hi T t_r))``:

    std = sqrt(q / (T - 1))      autocorr1 = sum_{t < T-1} xc[t] xc[t+1] / q      alff = mean_band 2 |X_k| / T
    falff = sum_band |X_k| / sum_{1..K} |X_k|      band_std = sqrt(sum_band w_k |X_k|^2 / T / (T - 1))
    band_fraction = band_std / std                 a zero denominator gives +0.0

``host_features`` forms the spectrum by an explicit cos/sin product whose arguments are reduced in integers,
``pi ((2 k t) mod 2 T) / T``; ``rfft_features`` is the same statement through ``numpy.fft.rfft``.  ``host_features32``
is what the device's operands give: fp32 table values, ``xc`` rounded to fp32, the coefficients accumulated in fp32 in
ascending order of the frame (a chain, not a blocked product), everything after them in fp64.
"""
import functools
import math

import numpy as np
import torch

NAMES = ("std", "autocorr1", "alff", "falff", "band_std", "band_fraction")
SPECTRAL = NAMES[2:]
S = 5                                             # subjects of a case, one per kind of ``KINDS``
KINDS = ("unit", "offset100", "walk1e4", "ramp", "constcol")
CHUNK = 128                                       # csrc/activity.hip: bins of a chunk
# (T, n, t_r, lo, hi)
CASES = [(2, 3, 1.0, 0.0, 0.5),                   # one bin, which is the Nyquist bin
         (9, 5, 1.0, 0.1, 0.4),                   # odd T, scalar loads
         (33, 65, 2.0, 0.01, 0.1),                # a frame past a 32-frame step, a column past a 64-column item
         (64, 64, 1.0, 0.25, 0.5),                # even T with the Nyquist bin inside the band (w_K = 1)
         (130, 84, 0.72, 0.01, 0.1),
         (300, 360, 2.0, 0.01, 0.08),             # six column items, 16-byte loads, 150 bins: two chunks for falff
         (298, 12, 1.0, 0.3, 0.5),                # the band 90 .. 149 straddles the chunk boundary between bins 128 and 129
         (520, 12, 0.72, 0.01, 0.1)]              # 260 bins: three chunks
# The seed of a case's frames, by (T, n); 0 where none is named.  tests/test_activity_math.py holds every non-constant
# column to a band bin lost or counted twice and to a Nyquist bin of weight 2; where the seed-0 frames had a column whose
# amplitude at that one bin was too faint for that, the case was replaced by the same case on other frames.
SEEDS = {(64, 64): 3, (300, 360): 2}
EPS = 2.0 ** -24
CONST_COL = 3                                     # the constant column of subject "constcol" (column 0 where n <= 3)
CONST_VALUE = 101.3


def band_of(T, t_r, lo, hi):
    """The index rule, stated again here: (k_lo, k_hi)."""
    return max(1, math.ceil(lo * T * t_r)), min(T // 2, math.floor(hi * T * t_r))


def const_col(n):
    return CONST_COL if n > CONST_COL else 0


@functools.lru_cache(maxsize=None)
def frames(T, n, seed=None):
    """[S, T, n] fp32 (host, shared: do not modify), one subject per kind; the seed is the case's own (``SEEDS``)."""
    if seed is None:
        return frames(T, n, SEEDS.get((T, n), 0))
    g = torch.Generator().manual_seed(19000 + seed)
    x = torch.empty(S, T, n, dtype=torch.float64)
    x[0] = torch.randn(T, n, generator=g, dtype=torch.float64)
    x[1] = 100.0 + torch.randn(T, n, generator=g, dtype=torch.float64)
    x[2] = 1e4 + 50.0 * (torch.randn(T, n, generator=g, dtype=torch.float64).cumsum(0) / 4.0
                         + torch.randn(T, n, generator=g, dtype=torch.float64))
    t = torch.arange(T, dtype=torch.float64)[:, None]
    x[3] = torch.randn(n, generator=g, dtype=torch.float64) * 10.0 + t * torch.randn(n, generator=g, dtype=torch.float64)
    x[4] = 100.0 + 3.0 * torch.randn(T, n, generator=g, dtype=torch.float64)
    x[4, :, const_col(n)] = CONST_VALUE
    return x.float().contiguous()


def table(T):
    """(cos, sin) float64 [K, T] of the bins 1 .. K, the arguments reduced in integers."""
    k = np.arange(1, T // 2 + 1, dtype=np.int64)[:, None]
    t = np.arange(T, dtype=np.int64)[None, :]
    a = np.pi * ((2 * k * t) % (2 * T)).astype(np.float64) / T
    return np.cos(a), np.sin(a)


def centred(x):
    """float64 numpy [T, n]: x - mean (the fp64 sum of T equal fp32 values is exact: a constant column gives exactly 0)."""
    xd = x.double().numpy()
    return xd - xd.sum(0) / xd.shape[0]


def moments(xc):
    """(q, lag-1 sum) float64 [n]"""
    return (xc * xc).sum(0), (xc[:-1] * xc[1:]).sum(0)


def _ratio(num, den):
    """num / den, +0.0 where den == 0 (a NaN is not 0: it takes the division)."""
    with np.errstate(all="ignore"):
        return np.where(den == 0.0, 0.0, num / np.where(den == 0.0, 1.0, den))


def finish(p2, q, lag, T, k_lo, k_hi, names, mult=None, nyquist_weight=1.0):
    """float64 [n, len(names)] from the powers p2 = |X_k|^2 [K, n] of the bins 1 .. K and the moments.  ``mult`` [K, n]
    scales what each bin adds to the band's sums and ``nyquist_weight`` replaces w_K of an even T: the wrong statements
    that the tolerance must not hide."""
    K = T // 2
    w = np.full(K, 2.0)
    if T % 2 == 0:
        w[K - 1] = nyquist_weight
    inband = np.zeros((K, 1))
    inband[k_lo - 1:k_hi] = 1.0
    if mult is not None:
        inband = inband * mult
    with np.errstate(all="ignore"):
        amp = np.sqrt(p2)
        band_amp = (inband * amp)[k_lo - 1:k_hi].sum(0)
        band_pow = (inband * w[:, None] * p2)[k_lo - 1:k_hi].sum(0)
        sd = np.sqrt(q / (T - 1))
        bsd = np.sqrt(band_pow / T / (T - 1))
        cols = {"std": sd, "autocorr1": _ratio(lag, q), "alff": 2.0 * band_amp / T / (k_hi - k_lo + 1),
                "falff": _ratio(band_amp, amp.sum(0)), "band_std": bsd, "band_fraction": _ratio(bsd, sd)}
    return np.stack([cols[name] for name in names], axis=1)


def powers(x):
    """|X_k|^2 float64 [K, n] of one subject x [T, n] by the explicit product, and (xc, q, lag)."""
    xc = centred(x)
    c, s = table(x.shape[0])
    re, im = c @ xc, s @ xc
    return re * re + im * im, xc, *moments(xc)


def host_features(x, t_r, band, names=NAMES):
    """float64 [S, n, F] (or [n, F] of one subject [T, n]): the statement."""
    if x.dim() == 3:
        return torch.stack([host_features(x[s], t_r, band, names) for s in range(x.shape[0])])
    T = x.shape[0]
    k_lo, k_hi = band_of(T, t_r, *band)
    p2, _, q, lag = powers(x)
    return torch.from_numpy(finish(p2, q, lag, T, k_lo, k_hi, names))


def rfft_features(x, t_r, band, names=NAMES):
    """The same through numpy.fft.rfft, one subject [T, n] -> float64 [n, F]."""
    T = x.shape[0]
    k_lo, k_hi = band_of(T, t_r, *band)
    xc = centred(x)
    X = np.fft.rfft(xc, axis=0)[1:T // 2 + 1]
    q, lag = moments(xc)
    return torch.from_numpy(finish(np.abs(X) ** 2, q, lag, T, k_lo, k_hi, names))


def powers32(x):
    """|X_k|^2 float64 [K, n] from the device's operands: fp32 table values, fp32 xc, an fp32 chain over the frames."""
    T, n = x.shape
    xc32 = centred(x).astype(np.float32)
    c, s = table(T)
    c32, s32 = c.astype(np.float32), s.astype(np.float32)
    re = np.zeros((T // 2, n), dtype=np.float32)
    im = np.zeros((T // 2, n), dtype=np.float32)
    for t in range(T):                            # ascending frames; every product and every sum rounds to fp32
        re = re + c32[:, t, None] * xc32[None, t]
        im = im + s32[:, t, None] * xc32[None, t]
    re, im = re.astype(np.float64), im.astype(np.float64)
    return re * re + im * im


def host_features32(x, t_r, band, names=NAMES):
    """float64 [S, n, F] / [n, F]: the statement on the operands the device holds; the moments stay fp64."""
    if x.dim() == 3:
        return torch.stack([host_features32(x[s], t_r, band, names) for s in range(x.shape[0])])
    T = x.shape[0]
    k_lo, k_hi = band_of(T, t_r, *band)
    q, lag = moments(centred(x))
    return torch.from_numpy(finish(powers32(x), q, lag, T, k_lo, k_hi, names))


@functools.lru_cache(maxsize=None)
def host_case(T, n, t_r, lo, hi):
    """float64 [S, n, 6] (shared: do not modify)."""
    return host_features(frames(T, n), t_r, (lo, hi))


@functools.lru_cache(maxsize=None)
def host32_case(T, n, t_r, lo, hi):
    return host_features32(frames(T, n), t_r, (lo, hi))


def amplitude(x):
    """max_t |xc| per column of x [S, T, n] or [T, n], float64, the scale of alff and band_std."""
    xd = x.double()
    return (xd - xd.sum(-2, keepdim=True) / xd.shape[-2]).abs().max(-2).values


def scale_of(name, x):
    """What a spectral feature's error is measured in: 2^-24 max_t |xc| for the amplitudes, 2^-24 for the ratios."""
    amp = amplitude(x)
    return EPS * amp if name in ("alff", "band_std") else torch.full_like(amp, EPS)


def ratios(got, want, bound):
    """|got - want| / bound elementwise; where the bound is 0 the match must be exact (0 if it is, inf if not)."""
    err = (got.double() - want).abs()
    return torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                       torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
