"""The host statement of ``ingest.kendall_counts`` and ``ingest.kendall_matrices`` and the seeded series
its tests share.

Statement, per unit over the pairs ``k = (s < t)`` of its kept frames: ``a_ik = sign(x_si - x_ti)`` by numpy's comparisons
of the float32 values (IEEE: ``-0.0 == +0.0``, ``+-inf`` are values, subnormals are values), ``G = A^T A`` accumulated in
float64 over chunks of at most 2^16 pairs -- exact: every partial sum is an integer below 2^23 -- and cast to int64.  A
column with a NaN in a kept frame has ``G_ii = -1`` and zeros elsewhere in its row and column.  ``tau_ij = G_ij /
sqrt(G_ii G_jj)`` in float64; a column with ``G_ii == 0`` is a zero row and column, diagonal included (scipy gives NaN
there), a NaN column is NaN in its row and column.  Formed, not sorted: nothing here knows how the device does it.

The series are ``tests/rank_data.py``'s (its constant, zeros, infs, subnormal, descending and NaN columns), the masks
``tests/censor_data.py``'s ten kinds; ``quantised`` rounds to half steps (heavy ties).
"""
import functools

import numpy as np
import torch

from tests import rank_data as RD
from tests import timeseries_data as TS

MAX_FRAMES = 4096
CHUNK = 2 ** 16


def unit_counts(x, kept=None):
    """int64 [n, n]: the statement for one unit x (float32 [L, n]) under kept (bool [L], None: every frame)."""
    x = np.asarray(x, dtype=np.float32)
    xk = x if kept is None else x[np.asarray(kept, dtype=bool)]
    n = x.shape[1]
    g = np.zeros((n, n), dtype=np.float64)
    i0, i1 = np.triu_indices(xk.shape[0], 1)
    with np.errstate(invalid="ignore"):
        for lo in range(0, i0.shape[0], CHUNK):
            xs, xt = xk[i0[lo:lo + CHUNK]], xk[i1[lo:lo + CHUNK]]
            a = (xs > xt).astype(np.float64) - (xs < xt).astype(np.float64)
            g += a.T @ a
    g = g.astype(np.int64)
    nan = np.isnan(xk).any(0)
    g[nan, :] = 0
    g[:, nan] = 0
    g[nan, nan] = -1
    return g


def host_counts(ts, keep=None, window=None, stride=None):
    """int64 [U, n, n] (numpy) for ts [S, T, n] (tensor or array), keep bool [S, T] or None; units as in
    ``timeseries_data``."""
    ts = ts.numpy() if isinstance(ts, torch.Tensor) else ts
    keep = keep.numpy() if isinstance(keep, torch.Tensor) else keep
    S, T, _ = ts.shape
    L = T if window is None else window
    st = L if stride is None else stride
    W = TS.num_windows(T, window, stride)
    return np.stack([unit_counts(ts[s, w * st:w * st + L], None if keep is None else keep[s, w * st:w * st + L])
                     for s in range(S) for w in range(W)])


def tau_of(g, absolute=False):
    """float64 [..., n, n]: the normalisation of counts g (int64 [..., n, n]) with the zero and NaN rules."""
    g = np.asarray(g, dtype=np.int64)
    d = np.diagonal(g, axis1=-2, axis2=-1)
    di, dj = d[..., :, None], d[..., None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = g.astype(np.float64) / np.sqrt(di.astype(np.float64) * dj.astype(np.float64))
    t = np.where((di == 0) | (dj == 0), 0.0, t)
    t = np.where((di < 0) | (dj < 0), np.nan, t)
    return np.abs(t) if absolute else t


def quantised(S, T, n, seed=0):
    """[S, T, n] fp32: normal deviates rounded to half steps, ``round(2 x)``: a dozen values, heavy ties."""
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.round(2.0 * torch.randn(S, T, n, generator=g)).contiguous()


@functools.lru_cache(maxsize=None)
def series_counts(S, T, n, seed=0, nan=True):
    """``host_counts(rank_data.series(...))``, computed once (shared: do not modify)."""
    return host_counts(RD.series(S, T, n, seed, nan))


def tie_pairs(v):
    """sum t (t - 1) / 2 over the runs of equal values of a column v (no NaN)."""
    _, counts = np.unique(np.asarray(v, dtype=np.float32), return_counts=True)
    return int((counts * (counts - 1) // 2).sum())


def ulps(got, want):
    """int64 array: how many fp32 steps lie between got (fp32) and fp32(want), both finite or both NaN (0 there)."""
    g = np.ascontiguousarray(np.asarray(got, dtype=np.float32))
    w = np.ascontiguousarray(np.asarray(want).astype(np.float32))
    nan = np.isnan(w)
    assert (np.isnan(g) == nan).all()

    def order(a):                                 # a monotone integer image of the floats, -0.0 and +0.0 together
        i = a.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    return np.where(nan, 0, np.abs(order(g) - order(w)))
