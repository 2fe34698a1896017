"""The host statement of ``connectome_gnn_amd.ingest.confound_basis`` / ``regress_confounds`` in float64, the same
statement on the fp32 operands the device holds, and the seeded confounds and frames its tests share.

Statement, per subject with frames ``x`` ``[T, n]`` and confounds ``c`` ``[T, q]`` (fp32 inputs, everything below in fp64):

    m_j  = the mean of confound column j,  cc_j = c_j - m_j,  s_j = sqrt(sum_t cc_j[t]^2)
    s_j == 0: column j is dropped;  otherwise u_j = cc_j / s_j
    r_j  = u_j - sum_{k < j, kept} q_k (q_k . u_j),  d_j = |r_j|^2
    d_j > RANK_TOL: column j is kept, q_j = r_j / sqrt(d_j);  otherwise it is dropped
    a non-finite s_j: the whole Q is NaN and the rank is -1
    xc   = x - its column means;  out = xc - Q (Q^T xc)

``host_basis`` is that Gram-Schmidt, literally, column by column.
"""
import functools
import math

import numpy as np
import torch

from tests import filter_data as F

EPS = F.EPS
RANK_TOL = 1e-10
MAX_CONFOUNDS = 64
# (T, n, S, q): the smallest shapes at which the kernels can still go wrong
CASES = [
    (2, 3, 2, 3),                                 # rank 1: two frames leave one direction
    (9, 5, 2, 5),
    (33, 64, 3, 1),
    (33, 65, 2, 24),                              # a frame past a step, a column past a tile, the scalar path
    (67, 97, 2, 33),                              # qpad 64
    (130, 84, 2, 32),
    (300, 360, 2, 64),                            # six tiles, vector path, full width
]
NEAR_COPY = (130, 84, 2, 8)                       # its last column is fl32(3 c_0 - 1): d near 1e-13, dropped


@functools.lru_cache(maxsize=None)
def confounds(S, T, q, seed=0, near_copy=False):
    """[S, T, q] fp32 (host, shared between tests: do not modify).  The pool, in this order: six random-walk "motion"
    columns with offsets, their differences, the squares of both, two columns of order 500 +- 5, and white noise
    beyond these 26.  The dependent columns are exact: column 2 is a constant (q >= 4), the last column is a bit-exact
    copy of column 0 (q >= 5), the one before it is column 1 times 2 (q >= 6).  ``near_copy``: the last column is
    ``fl32(3 c_0 - 1)`` instead, which rounding leaves independent by about 1e-13 of its norm."""
    g = torch.Generator().manual_seed(7000 + seed)
    steps = 0.05 * torch.randn(S, T, 6, generator=g, dtype=torch.float64)
    walk = steps.cumsum(1) + (torch.rand(S, 1, 6, generator=g, dtype=torch.float64) - 0.5)
    diff = torch.cat([torch.zeros(S, 1, 6, dtype=torch.float64), walk[:, 1:] - walk[:, :-1]], 1)
    big = 500.0 + 5.0 * torch.randn(S, T, 2, generator=g, dtype=torch.float64)
    noise = torch.randn(S, T, max(q - 26, 1), generator=g, dtype=torch.float64)
    pool = torch.cat([walk, diff, walk ** 2, diff ** 2, big, noise], 2)[:, :, :q].float()
    if q >= 4:
        pool[:, :, 2] = 0.25
    if near_copy:
        pool[:, :, q - 1] = (3.0 * pool[:, :, 0].double() - 1.0).float()
    else:
        if q >= 5:
            pool[:, :, q - 1] = pool[:, :, 0]
        if q >= 6:
            pool[:, :, q - 2] = 2.0 * pool[:, :, 1]
    return pool.contiguous()


@functools.lru_cache(maxsize=None)
def frames(S, T, n, q, seed=0, near_copy=False):
    """[S, T, n] fp32 (host, shared: do not modify): ``filter_data.frames`` plus 3 x confound 0 in every ROI."""
    c0 = confounds(S, T, q, seed, near_copy)[:, :, :1].double()
    return (F.frames(S, T, n, seed).double() + 3.0 * c0).float().contiguous()


def host_basis(c):
    """The statement for one subject's confounds c [T, q] (fp32, or fp64 as they are): (Q float64 [T, q] with zero
    columns where dropped, kept: list of bool, d: list of pivots, NaN for a column dropped on its norm).  A non-finite
    norm gives (all-NaN Q, None, None): rank -1."""
    c = c.double().numpy()
    T, q = c.shape
    with np.errstate(invalid="ignore"):           # (an Inf minus its mean)
        cc = c - c.mean(0, keepdims=True)
        s = np.sqrt((cc * cc).sum(0))
    if not np.isfinite(s).all():
        return torch.full((T, q), float("nan"), dtype=torch.float64), None, None
    Q = np.zeros((T, q))
    kept, piv = [], []
    for j in range(q):
        if s[j] == 0.0:
            kept.append(False)
            piv.append(float("nan"))
            continue
        u = cc[:, j] / s[j]
        r = u.copy()
        for k in range(j):
            if kept[k]:
                r = r - Q[:, k] * float(Q[:, k] @ u)
        d = float(r @ r)
        piv.append(d)
        kept.append(d > RANK_TOL)
        if kept[-1]:
            Q[:, j] = r / math.sqrt(d)
    return torch.from_numpy(Q), kept, piv


def host_rank(c):
    kept = host_basis(c)[1]
    return -1 if kept is None else sum(kept)


def host_regress(x, c):
    """The statement for one subject: float64 [T, n]."""
    xc = F.centred(x)
    Q = host_basis(c)[0]
    return xc - Q @ (Q.t() @ xc)


def host_regress32(x, c):
    """The statement on the operands the device holds: xc centred in fp64 and rounded to fp32, Q rounded to fp32, the
    host's fp32 matmul.  float32 [T, n]."""
    xc = F.centred(x).float()
    Q = host_basis(c)[0].float()
    return xc - Q @ (Q.t() @ xc)


def column_ratios(got, x, c):
    """Per column of one subject: max_t |got - host_regress| / (2^-24 max_t |xc|), float64 [n]."""
    scale = F.centred(x).abs().max(0).values
    return (got.double() - host_regress(x, c)).abs().max(0).values / (EPS * scale)


def all_cases():
    """(T, n, S, q, near_copy) of CASES and of the near-copy case"""
    return [(*case, False) for case in CASES] + [(*NEAR_COPY, True)]


def worst_host32_ratio():
    """The largest ratio of ``host_regress32`` over the cases, subjects and columns: what fp32 operands alone cost."""
    worst = 0.0
    for T, n, S, q, near in all_cases():
        for x, c in zip(frames(S, T, n, q, 0, near), confounds(S, T, q, 0, near)):
            worst = max(worst, float(column_ratios(host_regress32(x, c), x, c).max()))
    return worst


# ---- filter_timeseries(confounds=): the statement of the composition -------------------------------------------------
BANDS = [(130, 84, 2, 32, 0.72, 0.01, None), (300, 360, 2, 24, 2.0, 0.008, 0.09)]   # (T, n, S, q, t_r, hp, lp)


def host_filter_regress(x, c, t_r, high_pass, low_pass):
    """filter, then regress the filtered confounds, all in fp64: float64 [T, n]."""
    y = F.host_filter(x, t_r, high_pass, low_pass)
    cf = F.host_filter(c, t_r, high_pass, low_pass)
    Q = host_basis(cf)[0]
    return y - Q @ (Q.t() @ y)


# ---- the point of the feature: two ROIs that share a motion artefact ----------------------------------------------------
SPIKES = dict(S=2, T=300, n=8, q=6, seed=4)


@functools.lru_cache(maxsize=None)
def spike_pair(seed=SPIKES["seed"]):
    """(frames [S, 300, 8], confounds [S, 300, 6]) fp32: independent noise of deviation 0.5 in every ROI; confound 0 is
    spiky (20 frames of a subject at +-2 to +-3, zero elsewhere) and ROIs 0 and 1 also carry 5 x it; the other confounds
    are random walks."""
    S, T, n, q = (SPIKES[k] for k in ("S", "T", "n", "q"))
    g = torch.Generator().manual_seed(8000 + seed)
    x = 0.5 * torch.randn(S, T, n, generator=g, dtype=torch.float64)
    c = (0.05 * torch.randn(S, T, q, generator=g, dtype=torch.float64)).cumsum(1)
    c[:, :, 0] = 0.0
    for s in range(S):
        at = torch.randperm(T, generator=g)[:20]
        sign = torch.where(torch.rand(20, generator=g) < 0.5, -1.0, 1.0).double()
        c[s, at, 0] = sign * (2.0 + torch.rand(20, generator=g, dtype=torch.float64))
    x[:, :, :2] += 5.0 * c[:, :, :1]
    return x.float().contiguous(), c.float().contiguous()
