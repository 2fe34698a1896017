"""The host statement of ``connectome_gnn_amd.ingest.filter_timeseries`` in float64, the same statement on the fp32
operands the device holds, and the seeded frames its tests share.

Statement, per subject with frames ``x`` ``[T, n]`` (fp32 inputs, everything below in fp64) and column ``i``:
``b_k[t] = sqrt(2 / T) cos(pi (2 t + 1) k / (2 T))`` for ``k = 1 .. T - 1`` (the orthonormal DCT-II, component ``k`` at
``k / (2 T t_r)`` Hz); ``m_i`` = the mean of column ``i``; ``xc = x - m``;

    k_lo = 1 without a high_pass, else floor(2 T t_r high_pass) + 1
    k_hi = T - 1 without a low_pass, else min(T - 1, floor(2 T t_r low_pass))
    y    = sum_{k = k_lo .. k_hi} b_k (b_k . xc)

which is ``idct(mask * dct(xc))`` of ``scipy.fft`` with ``type=2, norm="ortho"``.  The call multiplies by the smaller of
the kept set and its complement (``y = xc - sum_{k dropped} b_k (b_k . xc)``); ``host_filter`` is always the kept form.
"""
import functools
import math

import numpy as np
import torch

EPS = 2.0 ** -24                                  # the unit roundoff of fp32
MAX_COMPONENTS = 256
# (T, n, S, t_r, high_pass, low_pass): the smallest shapes at which the kernel can still go wrong
CASES = [
    (2, 3, 2, 1.0, None, None),                   # pure centring, no products
    (9, 5, 2, 1.0, 0.1, None),                    # complement with one component
    (33, 65, 2, 2.0, 0.01, 0.1),                  # a frame past a 32-frame step, a column past a 64-column tile, scalar
    (50, 64, 3, 0.72, 0.05, 0.4),                 # the two forms within one component of each other
    (67, 97, 2, 0.72, None, 0.3),
    (130, 84, 2, 0.72, 0.01, 0.1),                # keep 17
    (300, 360, 2, 2.0, 0.008, 0.09),              # six column tiles, keep 99, vector loads
    (600, 12, 1, 1.0, None, 0.2134),              # the keep form with exactly 256 components
    (520, 12, 1, 0.72, 0.01, None),               # the complement form with 7
]

# One case per specialisation of the kernel that CASES leave out (they take 32, 128 and 256 components padded): 64, 96,
# 160, 192 twice (the one whose chunks are 16 frames: complement with vector stores, keep with scalar stores) and 224.
# Shapes whose host32 ratio (at most 14.0) lies inside the 15.95 of CASES: the device tolerance is built on that one.
WIDE_CASES = [
    (140, 20, 1, 1.0, None, 0.15),                # keep 42
    (150, 20, 1, 1.0, None, 0.2334),              # keep 70
    (262, 72, 2, 1.0, None, 0.24714),             # keep 129
    (326, 72, 2, 1.0, None, 0.25077),             # complement with 162: 20 chunks of 16 frames and one of 6
    (326, 65, 2, 1.0, 0.25077, None),             # keep 162
    (400, 12, 1, 1.0, None, 0.2488),              # keep 199
]


def components(T, t_r, high_pass=None, low_pass=None):
    """(k_lo, k_hi): the index rule, in Python floats."""
    k_lo = 1 if high_pass is None else math.floor(2 * T * t_r * high_pass) + 1
    k_hi = T - 1 if low_pass is None else min(T - 1, math.floor(2 * T * t_r * low_pass))
    return k_lo, k_hi


def form(T, k_lo, k_hi):
    """(complement, the components the call multiplies by): the smaller of the kept set and the rest."""
    kept = list(range(k_lo, k_hi + 1))
    dropped = [k for k in range(1, T) if not k_lo <= k <= k_hi]
    return (True, dropped) if len(kept) > len(dropped) else (False, kept)


def basis(T, comps):
    """float64 [T, len(comps)]: b_k[t], the argument reduced exactly in integers."""
    t = np.arange(T, dtype=np.int64)[:, None]
    k = np.asarray(list(comps), dtype=np.int64).reshape(1, -1)
    arg = ((2 * t + 1) * k) % (4 * T)
    return torch.from_numpy(math.sqrt(2.0 / T) * np.cos(np.pi * arg.astype(np.float64) / (2.0 * T)))


def centred(x):
    """float64 [T, n]: x minus its column means."""
    x = x.double()
    return x - x.mean(0, keepdim=True)


def project(xc, B):
    return B @ (B.t() @ xc)


def host_filter(x, t_r, high_pass=None, low_pass=None):
    """The statement for one subject x [T, n]: float64 [T, n], always by the kept components."""
    T = x.shape[0]
    k_lo, k_hi = components(T, t_r, high_pass, low_pass)
    return project(centred(x), basis(T, range(k_lo, k_hi + 1)))


def host_complement(x, t_r, high_pass=None, low_pass=None):
    """The same function by the dropped components: xc - sum_{k dropped} b_k (b_k . xc), float64."""
    T = x.shape[0]
    k_lo, k_hi = components(T, t_r, high_pass, low_pass)
    xc = centred(x)
    return xc - project(xc, basis(T, [k for k in range(1, T) if not k_lo <= k <= k_hi]))


def host_filter32(x, t_r, high_pass=None, low_pass=None):
    """The statement on the operands the device holds: xc centred in fp64 and rounded to fp32, the basis rounded to
    fp32, the host's fp32 matmul, the form the call chooses.  float32 [T, n]."""
    T = x.shape[0]
    complement, comps = form(T, *components(T, t_r, high_pass, low_pass))
    xc = centred(x).float()
    if not comps:
        return xc
    B = basis(T, comps).float()
    p = B @ (B.t() @ xc)
    return xc - p if complement else p


@functools.lru_cache(maxsize=None)
def planted(S, T, n, seed=0):
    """(components int64 [S, n, 4], amplitudes float64 [S, n, 4]) of the cosines ``frames`` plants."""
    g = torch.Generator().manual_seed(3000 + seed)
    ks = torch.randint(1, T, (S, n, 4), generator=g)
    amps = 0.2 + torch.rand(S, n, 4, generator=g, dtype=torch.float64)
    return ks, amps


@functools.lru_cache(maxsize=None)
def frames(S, T, n, seed=0):
    """[S, T, n] fp32 (host, shared between tests: do not modify).  Each column: four planted cosines of random
    components with amplitudes in [0.2, 1.2) plus 0.3 white noise, times a per-ROI scale in [0.5, 2), plus a per-ROI
    offset of order 100, plus a linear drift of 0.01 t.  The large offset is the point: careless centring fails on it."""
    ks, amps = planted(S, T, n, seed)
    g = torch.Generator().manual_seed(4000 + seed)
    t = torch.arange(T, dtype=torch.float64)
    x = 0.3 * torch.randn(S, T, n, generator=g, dtype=torch.float64)
    for j in range(4):
        arg = math.pi * (2 * t[None, :, None] + 1) * ks[:, None, :, j].double() / (2 * T)
        x = x + amps[:, None, :, j] * torch.cos(arg)
    x = x * (0.5 + 1.5 * torch.rand(n, generator=g, dtype=torch.float64))
    x = x + 100.0 * (1.0 + torch.rand(n, generator=g, dtype=torch.float64)) + 0.01 * t[None, :, None]
    return x.float().contiguous()


def column_ratios(got, x, t_r, high_pass, low_pass):
    """Per column of one subject: max_t |got - host_filter| / (2^-24 max_t |xc|), float64 [n]."""
    want = host_filter(x, t_r, high_pass, low_pass)
    scale = centred(x).abs().max(0).values
    return (got.double() - want).abs().max(0).values / (EPS * scale)


def worst_host32_ratio(cases=None):
    """The largest ratio of ``host_filter32`` over CASES, subjects and columns: what fp32 operands alone cost."""
    worst = 0.0
    for T, n, S, t_r, hp, lp in CASES if cases is None else cases:
        for x in frames(S, T, n):
            worst = max(worst, float(column_ratios(host_filter32(x, t_r, hp, lp), x, t_r, hp, lp).max()))
    return worst


# ---- the point of the feature: two ROIs that share a slow drift ------------------------------------------------------
DRIFT = dict(S=2, T=300, n=8, t_r=2.0, high_pass=0.008, low_pass=0.09, seed=2)     # the band starts at component 10


@functools.lru_cache(maxsize=None)
def drift_pair(seed=DRIFT["seed"]):
    """[S, 300, 8] fp32: independent noise of deviation 0.5 in every ROI; ROIs 0 and 1 also carry component 1 with
    amplitude 5, the same drift in both."""
    S, T, n = DRIFT["S"], DRIFT["T"], DRIFT["n"]
    g = torch.Generator().manual_seed(5000 + seed)
    x = 0.5 * torch.randn(S, T, n, generator=g, dtype=torch.float64)
    t = torch.arange(T, dtype=torch.float64)
    x[:, :, :2] += 5.0 * torch.cos(math.pi * (2 * t + 1) / (2 * T))[None, :, None]
    return x.float().contiguous()


def corr01(x):
    """Pearson correlation of columns 0 and 1 of one subject, fp64."""
    d = centred(x)
    return float((d[:, 0] * d[:, 1]).sum() / torch.sqrt((d[:, 0] ** 2).sum() * (d[:, 1] ** 2).sum()))
