"""The host statement of ``ingest.rank_timeseries`` and the seeded series its tests share.

Statement, per unit and column over the unit's kept frames::

    rank(t) = 1 + #{kept t' : v_t' < v_t} + (#{kept t' : v_t' == v_t} - 1) / 2

with numpy's comparisons of the float32 values (IEEE: ``-0.0 == +0.0``, subnormals are values); a NaN among the kept
frames makes them all NaN; a censored frame is 0 and is never looked at.  Counted, not sorted: nothing here knows how the
device does it.

Recipe: normal deviates quantised to quarter steps, so that ties abound, with special columns planted where ``n`` has
room for them (``SPECIAL``: name -> column; the column of special ``k`` is ``k`` and it sits in subject ``k % S``) and one
NaN column (``nan_at``) for ``n >= 7``.  The masks are ``tests/censor_data.py``'s.
"""
import functools

import numpy as np
import torch

from tests import censor_data as CD
from tests import timeseries_data as TS

MAX_FRAMES = 4096
SPECIAL = {"constant": 0, "zeros": 1, "infs": 2, "subnormal": 3, "descending": 4}
TINY = np.float32(2.0 ** -149)                    # the smallest subnormal


def column_ranks(v, kept=None):
    """float64 [L]: the statement for one column v (float32 [L]) under kept (bool [L], None: every frame)."""
    v = np.asarray(v, dtype=np.float32)
    kept = np.ones(v.shape[0], dtype=bool) if kept is None else np.asarray(kept, dtype=bool)
    out = np.zeros(v.shape[0], dtype=np.float64)
    vk = v[kept]
    if np.isnan(vk).any():
        out[kept] = np.nan
        return out
    with np.errstate(invalid="ignore"):
        less = (vk[None, :] < vk[:, None]).sum(1)
        same = (vk[None, :] == vk[:, None]).sum(1)
    out[kept] = 1.0 + less + (same - 1) / 2.0
    return out


def unit_ranks(x, kept=None):
    """float64 [L, n] for one unit x [L, n]."""
    x = np.asarray(x, dtype=np.float32)
    return np.stack([column_ranks(x[:, i], kept) for i in range(x.shape[1])], 1)


def host_ranks(ts, keep=None, window=None, stride=None):
    """float64 [U, L, n] (numpy) for ts [S, T, n] (tensor or array), keep bool [S, T] or None; units as in
    ``timeseries_data``."""
    ts = ts.numpy() if isinstance(ts, torch.Tensor) else ts
    keep = keep.numpy() if isinstance(keep, torch.Tensor) else keep
    S, T, _ = ts.shape
    L = T if window is None else window
    st = L if stride is None else stride
    W = TS.num_windows(T, window, stride)
    return np.stack([unit_ranks(ts[s, w * st:w * st + L], None if keep is None else keep[s, w * st:w * st + L])
                     for s in range(S) for w in range(W)])


def nan_at(S, n):
    """(subject, column) of the recipe's NaN column, None where n has no room for it."""
    return (1 % S, n - 1) if n >= 7 else None


def plain(S, T, n, seed=0):
    """[S, T, n] fp32: quarter steps only, no special column."""
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.round(4.0 * torch.randn(S, T, n, generator=g)) / 4.0).contiguous()


@functools.lru_cache(maxsize=None)
def series(S, T, n, seed=0, nan=True):
    """[S, T, n] fp32 (host, shared between tests: do not modify).  ``nan=False``: the same without the NaN."""
    x = plain(S, T, n, seed).clone()
    t = torch.arange(T)
    for name, col in SPECIAL.items():
        if col >= n:
            continue
        s = col % S
        if name == "constant":
            x[s, :, col] = 2.5
        elif name == "zeros":                     # both zeros among the quarter steps
            x[s, 0::3, col] = -0.0
            x[s, 1::3, col] = 0.0
        elif name == "infs":
            x[s, 0, col] = float("inf")
            x[s, T - 1, col] = float("-inf")
            if T >= 5:
                x[s, T // 2, col] = float("inf")
        elif name == "subnormal":                 # distinct subnormals of both signs, and 0
            k = (t - T // 2).float()
            x[s, :, col] = torch.from_numpy((k.numpy() * TINY).astype(np.float32))
        elif name == "descending":
            x[s, :, col] = (T - t).float() * 0.5
    at = nan_at(S, n)
    if nan and at is not None:
        x[at[0], T // 3, at[1]] = float("nan")
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def series_ranks(S, T, n, seed=0, nan=True):
    """``host_ranks(series(...))``, computed once (shared: do not modify)."""
    return host_ranks(series(S, T, n, seed, nan))


def masks(S, T):
    """``censor_data.masks``: bool [S, T], subject s of kind ``censor_data.KINDS[s % 10]``."""
    return CD.masks(S, T)


def bits(a):
    """The int32 bit patterns of the fp32 cast of an array or a tensor."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a.astype(np.float32)).view(np.int32)


def same_bits(got, want):
    """Whether ``got`` (tensor, fp32) is the fp32 cast of ``want`` (float64 array) bit for bit, a NaN of ``want``
    matched by any NaN."""
    g = got.detach().cpu().numpy()
    w = np.asarray(want)
    if g.shape != w.shape:
        return False
    nan = np.isnan(w)
    if not (np.isnan(g) == nan).all():
        return False
    return bool((bits(g)[~nan] == bits(w)[~nan]).all())


def spike_pair():
    """The README's example (``confound_data.spike_pair``): [2, 300, 8] fp32, ROIs 0 and 1 share 20 spiky frames of 300
    and nothing else."""
    from tests import confound_data
    return confound_data.spike_pair()[0]


def spearman(x, kept=None):
    """float64 [n, n]: ``np.corrcoef`` of the statement's ranks of one unit x [L, n] over its kept frames."""
    r = unit_ranks(x, kept)
    return np.corrcoef(r if kept is None else r[np.asarray(kept, dtype=bool)], rowvar=False)
