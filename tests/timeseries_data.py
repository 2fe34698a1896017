"""The host statement of ``connectome_gnn_amd.ingest.correlation_matrices`` in float64, and the seeded time-series
recipes its tests share.

Statement, per unit with frames ``x`` ``[L, n]`` (fp32 inputs, everything below in fp64): ``m_i`` = the mean of
column ``i``; ``q_i = sum_t (x[t, i] - m_i)^2``; ``z[t, i] = (x[t, i] - m_i) / sqrt(q_i)`` with ``1 / sqrt(0)``
taken as 0; ``r = z^T z`` clamped to ``[-1, 1]``, its diagonal set to 1 where ``q_i > 0`` and 0 elsewhere;
``absolute`` takes ``|r|``.  Units: without a window one per subject; with ``window=L`` and ``stride=st``
(default ``L``) subject ``s`` has ``W = (T - L) // st + 1`` units and unit ``s * W + w`` covers frames
``[w * st, w * st + L)``.

Recipe (seeded): four latent signals shared by the ROIs of a subject, mixed with ``0.6 randn(4, n)``, plus
independent unit noise, smoothed over time by ``y[t] = 0.5 y[t - 1] + e[t]``, times a per-ROI scale in
``[0.5, 3.5]``, plus ``offset`` population standard deviations of each (subject, ROI) column.
"""
import functools

import torch


def num_windows(T, window=None, stride=None):
    if window is None:
        return 1
    return (T - window) // (window if stride is None else stride) + 1


def host_unit(x, absolute=False):
    """[n, n] float64: the statement for one unit, x [L, n]."""
    x = x.double()
    d = x - x.mean(0, keepdim=True)
    q = (d * d).sum(0)
    rs = torch.where(q == 0, torch.zeros_like(q), 1.0 / torch.sqrt(q))
    z = d * rs
    r = (z.t() @ z).clamp(-1.0, 1.0)
    r.fill_diagonal_(0.0)
    r = r + torch.diag((q != 0).double())
    return r.abs() if absolute else r


def host_corr(ts, window=None, stride=None, absolute=False):
    """[U, n, n] float64 for ts [S, T, n]."""
    S, T, _ = ts.shape
    L = T if window is None else window
    st = L if stride is None else stride
    W = num_windows(T, window, stride)
    return torch.stack([host_unit(ts[s, w * st:w * st + L], absolute) for s in range(S) for w in range(W)])


def kappa(ts, window=None, stride=None):
    """max |m_i| / std_i over every unit and every column that is not constant, in fp64."""
    S, T, _ = ts.shape
    L = T if window is None else window
    st = L if stride is None else stride
    worst = 0.0
    for s in range(S):
        for w in range(num_windows(T, window, stride)):
            x = ts[s, w * st:w * st + L].double()
            m, sd = x.mean(0), x.std(0, unbiased=False)
            ok = sd > 0
            if bool(ok.any()):
                worst = max(worst, float((m[ok].abs() / sd[ok]).max()))
    return worst


def atol(T, k):
    """Twice the first-order bound of T fp32 accumulations of products whose magnitudes sum to at most 1, the
    dropped terms of a split product, and the centring and scaling roundings (which grow with |m| / std)."""
    return (T + 32 + 4 * k) * 2.0 ** -23


def _signals(S, T, n, g, extra=None):
    lat = torch.randn(S, T, 4, generator=g, dtype=torch.float64)
    mix = 0.6 * torch.randn(4, n, generator=g, dtype=torch.float64)
    e = lat @ mix + torch.randn(S, T, n, generator=g, dtype=torch.float64)
    if extra is not None:
        e = e + extra
    y = torch.empty_like(e)
    y[:, 0] = e[:, 0]
    for t in range(1, T):
        y[:, t] = 0.5 * y[:, t - 1] + e[:, t]
    return y * (0.5 + 3.0 * torch.rand(n, generator=g, dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def recipe(S, T, n, seed=0, offset=0.0):
    """[S, T, n] fp32 (host, shared between tests: do not modify)."""
    g = torch.Generator().manual_seed(seed)
    x = _signals(S, T, n, g)
    if offset:
        x = x + offset * x.std(1, unbiased=False, keepdim=True)
    return x.float().contiguous()


@functools.lru_cache(maxsize=None)
def planted(S, T, n, seed=0, offset=0.0):
    """The recipe with, in its LAST subject and for n >= 5, column 1 constant (2.5) and column n - 2 all zeros."""
    x = recipe(S, T, n, seed, offset).clone()
    if n >= 5:
        x[-1, :, 1] = 2.5
        x[-1, :, n - 2] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def two_classes(S, T, n, seed=4):
    """([S, T, n] fp32, labels [S]): class 1 has one more signal shared by its first n // 3 ROIs."""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(S, dtype=torch.long) % 2
    extra = torch.zeros(S, T, n, dtype=torch.float64)
    extra[y == 1, :, : n // 3] = 1.5 * torch.randn(int((y == 1).sum()), T, 1, generator=g, dtype=torch.float64)
    return _signals(S, T, n, g, extra).float().contiguous(), y
