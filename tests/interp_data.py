"""The host statement of ``connectome_gnn_amd.ingest.interpolate_censored`` in float64, and the seeded
masks and frames its tests share.  Nothing here knows how the device does it.

Statement, per subject with frames ``x`` ``[T, n]`` and mask ``keep`` ``[T]``, per column, everything in fp64:
``t_0 < .. < t_{m-1}`` are the kept frames, ``y_k = x[t_k]``, ``h_k = t_{k+1} - t_k``, ``delta_k = (y_{k+1} - y_k) / h_k``.

* a kept frame is its input; ``m == 0`` gives zeros, ``m == 1`` the one value everywhere;
* a censored frame before ``t_0`` takes ``x[t_0]``, one after ``t_{m-1}`` takes ``x[t_{m-1}]``;
* inside ``(t_k, t_{k+1})``, with ``u = (t - t_k) / h_k``,
  ``v = (1+2u)(1-u)^2 y_k + u(1-u)^2 h_k s_k + u^2(3-2u) y_{k+1} + u^2(u-1) h_k s_{k+1}``;
* the knot derivatives: ``m == 2``: ``s_0 = s_1 = delta_0``; ``m == 3``: ``s_0 + s_1 = 2 delta_0``,
  ``h_1 s_0 + 2(h_0+h_1) s_1 + h_0 s_2 = 3(h_1 delta_0 + h_0 delta_1)``, ``s_1 + s_2 = 2 delta_1``; ``m >= 4``: interior rows
  ``h_k s_{k-1} + 2(h_{k-1}+h_k) s_k + h_{k-1} s_{k+1} = 3(h_k delta_{k-1} + h_{k-1} delta_k)``, first row with
  ``d = t_2 - t_0``: ``h_1 s_0 + d s_1 = ((h_0 + 2d) h_1 delta_0 + h_0^2 delta_1) / d``, last row with
  ``d = t_{m-1} - t_{m-3}``: ``d s_{m-2} + h_{m-3} s_{m-1} = (h_{m-2}^2 delta_{m-3} + (2d + h_{m-2}) h_{m-3} delta_{m-2}) / d``.

``host_interpolate`` writes the matrix out densely and hands it to ``numpy.linalg.solve`` (LU with partial pivoting).

Masks: one kind per subject, ``KINDS`` = the ten of ``censor_data`` and four of this module's; where a kind is random its
seed is ``9000 + s`` as there.
"""
import functools

import numpy as np
import torch

from tests import censor_data as C

KINDS = C.KINDS + ("three", "four", "pairs", "longgap")
S = len(KINDS)                                    # 14: every kind occurs once
# (T, n): tiny runs (every special case of m); a one-column second panel; two sizes that are no multiple of anything;
# six panels; the production run length with every chunk boundary
CASES = [(9, 5), (33, 65), (67, 97), (130, 84), (300, 360), (1201, 70)]
BOUND = 2.0 ** -40                                # what two fp64 formulations of the same spline are granted, x max_K |x|


def mask_of(kind, T, s):
    """bool [T], True = kept: the mask of ``kind`` for subject ``s`` of a ``T``-frame run."""
    if kind in C.KINDS:
        return C.mask_of(kind, T, s)
    g = torch.Generator().manual_seed(9000 + s)
    keep = torch.zeros(T, dtype=torch.bool)
    if kind == "three":
        keep[torch.randperm(T, generator=g)[:3]] = True
    elif kind == "four":
        keep[torch.randperm(T, generator=g)[:4]] = True
    elif kind == "pairs":                         # two kept, a gap of 1 - 3, two kept, ..
        t = 0
        while t < T:
            keep[t:t + 2] = True
            t += 2 + int(torch.randint(1, 4, (1,), generator=g))
    else:
        assert kind == "longgap", kind            # one gap of T // 2 in the middle
        keep[:] = True
        keep[T // 4:T // 4 + T // 2] = False
    return keep


@functools.lru_cache(maxsize=None)
def masks(T):
    """bool [S, T] (host, shared between tests: do not modify): subject s has kind ``KINDS[s]``."""
    return torch.stack([mask_of(KINDS[s], T, s) for s in range(S)]).contiguous()


@functools.lru_cache(maxsize=None)
def frames(T, n, seed=0):
    """[S, T, n] fp32 (host, shared: do not modify): noise of deviation 3 on a per-column offset of deviation 100, so
    that a solve or an evaluation in fp32 shows."""
    g = torch.Generator().manual_seed(11000 + seed)
    x = 3.0 * torch.randn(S, T, n, generator=g, dtype=torch.float64)
    x = x + 100.0 * torch.randn(n, generator=g, dtype=torch.float64)
    return x.float().contiguous()


def knot_derivatives(t, y):
    """s [m, n] float64 of the knots t [m] (float64, ascending) and values y [m, n] (float64), m >= 2."""
    m = len(t)
    h = np.diff(t)
    delta = (y[1:] - y[:-1]) / h[:, None]
    if m == 2:
        return np.stack([delta[0], delta[0]])
    A = np.zeros((m, m))
    r = np.zeros_like(y)
    for k in range(1, m - 1):
        A[k, k - 1], A[k, k], A[k, k + 1] = h[k], 2.0 * (h[k - 1] + h[k]), h[k - 1]
        r[k] = 3.0 * (h[k] * delta[k - 1] + h[k - 1] * delta[k])
    if m == 3:
        A[0, 0] = A[0, 1] = A[2, 1] = A[2, 2] = 1.0
        r[0], r[2] = 2.0 * delta[0], 2.0 * delta[1]
    else:
        d = t[2] - t[0]
        A[0, 0], A[0, 1] = h[1], d
        r[0] = ((h[0] + 2.0 * d) * h[1] * delta[0] + h[0] ** 2 * delta[1]) / d
        d = t[m - 1] - t[m - 3]
        A[m - 1, m - 2], A[m - 1, m - 1] = d, h[m - 3]
        r[m - 1] = (h[m - 2] ** 2 * delta[m - 3] + (2.0 * d + h[m - 2]) * h[m - 3] * delta[m - 2]) / d
    return np.linalg.solve(A, r)


def host_interpolate(x, keep):
    """The statement for one subject: x [T, n] (fp32 as the device holds it, or fp64 as it is), keep [T] bool ->
    float64 [T, n], before the one rounding to fp32.  Censored rows of x are never read."""
    T, n = x.shape
    out = torch.zeros(T, n, dtype=torch.float64)
    idx = keep.nonzero().flatten()
    m = len(idx)
    if m == 0:
        return out
    y = x[idx].double().numpy()
    t = idx.double().numpy()
    v = out.numpy()                               # (shares out's memory)
    v[:int(idx[0])] = y[0]
    v[int(idx[-1]):] = y[-1]
    v[idx.numpy()] = y
    if m == 1:
        return out
    with np.errstate(invalid="ignore", over="ignore"):        # (a non-finite kept value stays in its column)
        s = knot_derivatives(t, y)
        for k in range(m - 1):
            t0, t1 = int(idx[k]), int(idx[k + 1])
            hk = float(t1 - t0)
            for f in range(t0 + 1, t1):
                u = (f - t0) / hk
                v[f] = ((1 + 2 * u) * (1 - u) ** 2 * y[k] + u * (1 - u) ** 2 * hk * s[k]
                        + u ** 2 * (3 - 2 * u) * y[k + 1] + u ** 2 * (u - 1) * hk * s[k + 1])
    return out


@functools.lru_cache(maxsize=None)
def host_case(T, n):
    """float64 [S, T, n] (shared: do not modify): ``host_interpolate`` of every subject of a case."""
    x, m = frames(T, n), masks(T)
    return torch.stack([host_interpolate(x[s], m[s]) for s in range(S)])


def scale(x, keep):
    """max_K |x| per column, float64 [n] (0 without a kept frame)."""
    if not bool(keep.any()):
        return torch.zeros(x.shape[1], dtype=torch.float64)
    return x[keep].double().abs().max(0).values


def column_ratios(got, want, x, keep):
    """Per column of one subject, with ``want = host_interpolate(x, keep)``: max over the censored frames of
    |got - want| / (2^-24 |want| + 2^-40 max_K |x|), float64 [n]; where that bound is 0 the match must be exact (0 if it
    is, inf if not).  No censored frame: zeros."""
    if bool(keep.all()):
        return torch.zeros(x.shape[1], dtype=torch.float64)
    err = (got.double() - want)[~keep].abs()
    bound = 2.0 ** -24 * want[~keep].abs() + BOUND * scale(x, keep)[None, :]
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return r.max(0).values
