"""The host statement of ``connectome_gnn_amd.ingest.filter_timeseries(..., filter="butterworth")`` in
float64, the seeded frames and the cases its tests share, and a numpy model of how the kernel walks a column.

Statement, per subject and column: ``scipy.signal.sosfiltfilt(scipy.signal.butter(order, ..., output="sos", fs=1 / t_r),
float64(x))`` with scipy's defaults (``padtype="odd"``, ``padlen=None``), before the one rounding to fp32.  ``host`` knows
nothing of how the device does it; ``model`` does: the level shift by ``x[0]``, the odd extension formed on load, the
forward pass that keeps the states at segment boundaries only, and the backward pass that forms each segment's forward
outputs again (csrc/butterworth.hip).
"""
import functools

import numpy as np
import scipy.signal
import torch

S = 5                                             # subjects of a case, one per kind of ``KINDS``
KINDS = ("unit", "offset100", "walk1e4", "ramp", "constcol")
CHUNK, SHORT = 48, 8                              # csrc/butterworth.hip: frames of a chunk, of a short segment
# (T, n, t_r, high_pass, low_pass, order)
CASES = [(34, 65, 0.72, 0.01, 0.1, 5),            # T = edge + 1; n one past a wave
         (19, 1, 0.72, 0.01, None, 5),            # T = edge + 1 of a 3-section high-pass; one column
         (130, 84, 2.0, 0.008, 0.08, 5),
         (300, 360, 0.72, 0.01, 0.1, 5),
         (1201, 70, 0.72, 0.01, 0.1, 5),
         (300, 63, 0.72, None, 0.1, 5),           # low-pass, add_level
         (300, 64, 0.72, 0.01, 0.1, 1),           # one section, edge = 9
         (1201, 130, 0.72, 0.008, None, 6),
         (160, 64, 0.72, 0.01, 0.1, 8),           # eight sections, edge = 51
         (63, 66, 0.72, 0.01, 0.1, 5),            # T + edge = 96: a multiple of the chunk (of 48 frames)
         (64, 66, 0.72, 0.01, 0.1, 5)]            # .. and one more
BOUND = 2.0 ** -40                                # what two fp64 formulations are granted, x max_t |x|
CONST_COL = 3                                     # the constant column of subject "constcol" (column 0 where n <= 3)
CONST_VALUE = 101.3


def butter(t_r, high_pass, low_pass, order):
    """scipy's sections of the design."""
    if high_pass is not None and low_pass is not None:
        return scipy.signal.butter(order, [high_pass, low_pass], btype="bandpass", output="sos", fs=1.0 / t_r)
    if high_pass is not None:
        return scipy.signal.butter(order, high_pass, btype="highpass", output="sos", fs=1.0 / t_r)
    return scipy.signal.butter(order, low_pass, btype="lowpass", output="sos", fs=1.0 / t_r)


def edge_of(sos):
    """scipy's default pad length of ``sosfiltfilt``."""
    sos = np.asarray(sos)
    return 3 * (2 * len(sos) + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum())))


def host(x, t_r, hp, lp, order):
    """float64, the shape of x ([S, T, n] or [T, n] with time on axis -2)."""
    y = scipy.signal.sosfiltfilt(butter(t_r, hp, lp, order), x.double().numpy(), axis=x.dim() - 2)
    return torch.from_numpy(np.ascontiguousarray(y))


def const_col(n):
    return CONST_COL if n > CONST_COL else 0


@functools.lru_cache(maxsize=None)
def frames(T, n, seed=0):
    """[S, T, n] fp32 (host, shared: do not modify), one subject per kind."""
    g = torch.Generator().manual_seed(13000 + seed)
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


@functools.lru_cache(maxsize=None)
def host_case(T, n, t_r, hp, lp, order):
    """float64 [S, T, n] (shared: do not modify)."""
    return host(frames(T, n), t_r, hp, lp, order)


def scale(x):
    """max_t |x| per column of one subject, float64 [n]."""
    return x.double().abs().max(0).values


def column_ratios(got, want, x):
    """Per column of one subject: max over the frames of |got - want| / (2^-24 |want| + 2^-40 max_t |x|), float64 [n];
    where that bound is 0 the match must be exact (0 if it is, inf if not)."""
    err = (got.double() - want).abs()
    bound = 2.0 ** -24 * want.abs() + BOUND * scale(x)[None, :]
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return r.max(0).values


# ---- the kernel's walk, in numpy ------------------------------------------------------------------------------------------
def _zi(sos):
    """sosfilt_zi as the entry point derives it: [L, 2]."""
    zi, sc = np.zeros((len(sos), 2)), 1.0
    for l, (b0, b1, b2, _, a1, a2) in enumerate(sos):
        g = (b0 + b1 + b2) / (1.0 + a1 + a2)
        zi[l] = sc * (g - b0), sc * (b2 - a2 * g)
        sc *= g
    return zi


def _step(sos, z, v):
    """one frame [n] through the sections; z [L, 2, n] is updated in place"""
    for l, (b0, b1, b2, _, a1, a2) in enumerate(sos):
        y = b0 * v + z[l, 0]
        z[l, 0] = -a1 * y + (b1 * v + z[l, 1])
        z[l, 1] = -a2 * y + b2 * v
        v = y
    return v


def segments(T, edge, chunk=CHUNK, short=SHORT):
    """[(first frame f = e - edge, frames)] of the frames from e = edge on: T // chunk chunks of real frames, then the
    tail in segments of ``short`` and of one."""
    full = T // chunk
    segs = [(k * chunk, chunk) for k in range(full)]
    f, end = full * chunk, T + edge
    while f + short <= end:
        segs.append((f, short))
        f += short
    return segs + [(g, 1) for g in range(f, end)]


def model(x, sos, add_level, chunked=True):
    """x [T, n] fp32 -> float64 [T, n] before the one rounding, by the kernel's walk (``chunked``), or by the same
    recurrence over the whole extended run with every forward output kept."""
    sos = [tuple(float(v) for v in r) for r in np.asarray(sos)]
    T, n = x.shape
    edge = edge_of(sos)
    xd = x.double().numpy()
    x0 = xd[0].copy()
    dl = xd[T - 1] - x0

    def frame(f):                                 # frame e = f + edge as it is formed on load
        if f < 0:
            return 0.0 - (xd[-f] - x0)
        if f < T:
            return xd[f] - x0
        return 2.0 * dl - (xd[2 * (T - 1) - f] - x0)

    zi = _zi(sos)
    zf = zi[:, :, None] * frame(-edge)[None, None, :]
    for f in range(-edge, 0):
        _step(sos, zf, frame(f))
    out = np.zeros((T, n))
    lvl = x0 if add_level else 0.0
    if not chunked:
        y = [_step(sos, zf, frame(f)) for f in range(T + edge)]
        zb = zi[:, :, None] * y[-1][None, None, :]
        for f in range(T + edge - 1, -1, -1):
            w = _step(sos, zb, y[f])
            if f < T:
                out[f] = w + lvl
        return torch.from_numpy(out)
    segs = segments(T, edge)
    bounds, last = [], None
    for f0, cnt in segs:
        bounds.append(zf.copy())
        for f in range(f0, f0 + cnt):
            last = _step(sos, zf, frame(f))
    zb = zi[:, :, None] * last[None, None, :]
    for (f0, cnt), z in zip(reversed(segs), reversed(bounds)):
        z = z.copy()
        y = [_step(sos, z, frame(f)) for f in range(f0, f0 + cnt)]
        for i in range(cnt - 1, -1, -1):
            w = _step(sos, zb, y[i])
            if f0 + i < T:
                out[f0 + i] = w + lvl
    return torch.from_numpy(out)
