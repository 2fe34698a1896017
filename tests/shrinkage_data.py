"""The host statement of ``connectome_gnn_amd.ingest.ledoit_wolf_shrinkage`` in float64, the same statement on the
fp32 operands the device holds, the factor by which its quotient magnifies an error of its sums, and the seeded frames
its tests share.

Statement, per unit with frames ``x`` ``[L, n]`` (fp32 inputs, everything below in fp64): ``m_i`` = the mean of column
``i``; ``q_i = sum_t (x[t, i] - m_i)^2``; ``z[t, i] = (x[t, i] - m_i) / sqrt(q_i)`` with ``1 / sqrt(0)`` taken as 0;
``R = z^T z``;

    p   = the number of columns with q_i > 0
    s_t = sum_i z[t, i]^2                    B = L sum_t s_t^2
    O   = 2 sum_{i<j} R_ij^2                 F = p + O
    a   = 0 if O == 0, else (B - F) / (L O) clipped to [0, 1] (a NaN stays a NaN)

which is ``sklearn.covariance.ledoit_wolf_shrinkage(z sqrt(L), assume_centered=True)`` over the columns that are not
constant.  ``L == 2`` makes every ``z`` equal to ``+-1/sqrt(2)`` and every ``R_ij`` to ``+-1``: ``B - F`` is zero
identically, what is left of it is rounding and no estimate, so ``a = 0`` there (a NaN stays a NaN).
"""
import functools

import numpy as np
import torch

EPS = 2.0 ** -24                                  # the unit roundoff of fp32
# (L, n, S): odd frame counts around the 8-frame blocks of the streaming passes, the 64-lane boundary, the 96-wide
# tiles of the correlation kernel and the size limit
CASES = [(2, 5, 3), (7, 1, 2), (9, 33, 3), (40, 64, 2), (40, 65, 2), (66, 97, 3), (300, 84, 3), (120, 360, 2),
         (64, 1024, 1)]
KINDS = ("planted", "white")


def _sums(z, R, L):
    """(B, F, O) in fp64 of standardised frames z [L, n] and their product R [n, n], whatever precision they come in."""
    z, R = z.double(), R.double()
    p = float((z != 0).any(0).sum())              # (a column that is not constant has a nonzero z)
    s = (z * z).sum(1)
    B = L * float((s * s).sum())
    O = 2.0 * float((torch.triu(R, 1) ** 2).sum())
    return B, p + O, O


def _quotient(B, F, O, L):
    if O == 0.0:
        return 0.0
    r = (B - F) / (L * O)
    if r != r:
        return r
    return 0.0 if L == 2 else min(1.0, max(0.0, r))


def _standardised(x):
    x = x.double()
    d = x - x.mean(0, keepdim=True)
    q = (d * d).sum(0)
    rs = torch.where(q == 0, torch.zeros_like(q), 1.0 / torch.sqrt(q))
    return x.mean(0), rs, d * rs


def ratio(x):
    """(B - F) / (L O) before the clip, in fp64 (inf if O == 0)."""
    L = x.shape[0]
    _, _, z = _standardised(x)
    B, F, O = _sums(z, z.t() @ z, L)
    return (B - F) / (L * O) if O != 0.0 else float("inf")


def host_lw(x):
    """The statement for one unit x [L, n]: a Python float."""
    L = x.shape[0]
    _, _, z = _standardised(x)
    return _quotient(*_sums(z, z.t() @ z, L), L)


def host_lw32(x):
    """The statement with z and R as the device holds them: the statistics rounded to fp32, z = (x - m) rs in fp32,
    R = z^T z by the host's fp32 product, clamped to [-1, 1]; the sums and the quotient in fp64."""
    L = x.shape[0]
    m, rs, _ = _standardised(x)
    z = (x.float() - m.float()) * rs.float()
    R = (z.t() @ z).clamp(-1.0, 1.0)
    return _quotient(*_sums(z, R, L), L)


def cond(x):
    """(B + F) / (L O): by how much the quotient (B - F) / (L O) magnifies a relative error of B and F (0 if O == 0:
    the answer is then exactly 0)."""
    L = x.shape[0]
    _, _, z = _standardised(x)
    B, F, O = _sums(z, z.t() @ z, L)
    return (B + F) / (L * O) if O != 0.0 else 0.0


def host_cohort(ts, window=None, stride=None):
    """float64 [U] for ts [S, T, n], units as in ``timeseries_data.host_corr``."""
    S, T, _ = ts.shape
    L = T if window is None else window
    st = L if stride is None else stride
    W = 1 if window is None else (T - L) // st + 1
    return torch.tensor([host_lw(ts[s, w * st:w * st + L]) for s in range(S) for w in range(W)], dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def planted(S, L, n, seed=0):
    """[S, L, n] fp32 (host, shared between tests: do not modify): three latent signals shared by the ROIs plus unit
    noise, times a per-ROI scale, plus a per-ROI offset; for n >= 3 column n // 2 is constant (1.5) in every subject."""
    g = torch.Generator().manual_seed(1000 + seed)
    lat = torch.randn(S, L, 3, generator=g, dtype=torch.float64)
    mix = 0.8 * torch.randn(3, n, generator=g, dtype=torch.float64)
    x = lat @ mix + torch.randn(S, L, n, generator=g, dtype=torch.float64)
    x = x * (0.5 + 3.0 * torch.rand(n, generator=g, dtype=torch.float64)) + torch.randn(n, generator=g,
                                                                                       dtype=torch.float64)
    if n >= 3:
        x[:, :, n // 2] = 1.5
    return x.float().contiguous()


@functools.lru_cache(maxsize=None)
def white(S, L, n, seed=0):
    """[S, L, n] fp32 (host, shared: do not modify): white noise."""
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(S, L, n, generator=g, dtype=torch.float64).float().contiguous()


def frames(kind, S, L, n, seed=0):
    return {"planted": planted, "white": white}[kind](S, L, n, seed)


@functools.lru_cache(maxsize=None)
def clipped():
    """[1, 1000, 12] fp32: white noise whose unclipped ratio is about 1.34."""
    return torch.from_numpy(np.random.default_rng(1).standard_normal((1000, 12)).astype(np.float32))[None].contiguous()


def worst_host32_ratio():
    """The largest |host_lw32 - host_lw| / (2^-24 cond) over CASES x KINDS: what fp32 operands alone cost."""
    worst = 0.0
    for kind in KINDS:
        for L, n, S in CASES:
            for x in frames(kind, S, L, n):
                k = cond(x)
                if k > 0.0:
                    worst = max(worst, abs(host_lw32(x) - host_lw(x)) / (EPS * k))
    return worst
