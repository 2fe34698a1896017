"""The host statement of ``connectome_gnn_amd.ingest`` in plain torch, and the seeded matrix recipes its tests
share.

Statement, per subject with matrix ``A`` ``[n, n]`` fp32: the candidates are the ``m = n (n - 1)``
off-diagonal entries with NaN replaced by -inf; the threshold is the candidate at index ``k`` of their
descending sort (-inf when ``k >= m``); ``i -> j`` is an edge iff ``i != j``, ``A[i, j] > t`` and
``A[i, j] > 0``; edges are ``torch.nonzero`` of that mask (row-major).  The default node feature is
``strength_i / (max_i strength_i + 1e-8)`` with ``strength_i`` the sum over ``j`` of the kept ``A[i, j]``.

Recipe for one ``n`` (six subjects, seed 0, ``B = randn(n, n)``): 1 ``(B + B^T) / 2``, signed; 2
``max(Q, Q^T)`` with ``Q = round(8 rand) / 8`` (heavy ties); 3 all zeros; 4 ``rand(n, n)``, asymmetric; 5
subject 1 with NaN at (0,1) and (1,0) and +inf on a diagonal entry; 6 symmetric ``rand`` with +inf at (0,3)
and (3,0) and the subnormal 1e-40 at (1,2) and (2,1).  Entries that do not exist at a small ``n`` are left out.
"""
import functools

import torch

import connectome_gnn_amd as C

INF = float("inf")
# Edge counts of the n = 84 recipe from the statement above on the CPU.  keep = 0.1 (k = 697) shows an odd k on
# symmetric data, a tie class that empties a subject and an exact k; at keep = 1 every positive entry stays.
# (These depend on the generator calls only through subjects 1, 2 and 5 at keep = 1; the draw order is Q, subject 4,
# subject 6's R, then B.)
COUNTS_84 = {0.1: [696, 0, 0, 697, 696, 696], 1.0: [3426, 6952, 0, 6972, 3424, 6972]}


def rank_of(n, keep=None, num_edges=None):
    """The rank k of the threshold among the candidates."""
    return int(keep * n * (n - 1) + 0.5) if keep is not None else int(num_edges)


def _off_diagonal(n):
    return ~torch.eye(n, dtype=torch.bool)


def host_threshold(A, k):
    cand = A[_off_diagonal(A.shape[0])]
    cand = torch.where(torch.isnan(cand), torch.full_like(cand, -INF), cand)
    if k >= cand.numel():
        return -INF
    return float(torch.sort(cand, descending=True).values[k])


def host_thresholds(mats, k):
    return torch.tensor([host_threshold(A, k) for A in mats], dtype=torch.float32)


def host_sorted(A):
    """The candidates of A in descending order, for thresholds at several ranks: ``rank_value(c, k)``."""
    cand = A[_off_diagonal(A.shape[0])]
    return torch.sort(torch.where(torch.isnan(cand), torch.full_like(cand, -INF), cand), descending=True).values


def rank_value(cand_sorted, k):
    return -INF if k >= cand_sorted.numel() else float(cand_sorted[k])


def host_edges(A, t):
    """(edge_index int64 [2, e], edge_weight [e]) of one subject at threshold t."""
    mask = (A > t) & (A > 0) & _off_diagonal(A.shape[0])
    return torch.nonzero(mask).t().contiguous(), A[mask]


def host_strength_feature(A, t, dtype=torch.float64):
    """[n, 1]: the default node feature, computed in `dtype`."""
    mask = (A > t) & (A > 0) & _off_diagonal(A.shape[0])
    s = torch.where(mask, A, torch.zeros_like(A)).to(dtype).sum(1)
    return (s / (s.max() + 1e-8)).unsqueeze(1)


def host_graphs(mats, thr, x, labels):
    """The ConnectomeGraphs the statement gives: thr per subject (a sequence of floats), x [S, n, F]."""
    out = []
    for s, A in enumerate(mats):
        ei, w = host_edges(A, float(thr[s]))
        out.append(C.ConnectomeGraph(x[s], ei, w, labels[s], f"sub-{s:04d}"))
    return out


def _set(A, i, j, v):
    if i < A.shape[0] and j < A.shape[0]:
        A[i, j] = v


@functools.lru_cache(maxsize=None)
def recipe(n, seed=0):
    """[6, n, n] fp32 (host, shared between tests: do not modify)."""
    g = torch.Generator().manual_seed(seed)           # draws: the three uniform matrices, then B
    Q = torch.round(8 * torch.rand(n, n, generator=g)) / 8
    s4 = torch.rand(n, n, generator=g)
    R = torch.rand(n, n, generator=g)
    B = torch.randn(n, n, generator=g)
    s1 = (B + B.t()) / 2
    s2 = torch.maximum(Q, Q.t())
    s3 = torch.zeros(n, n)
    s5 = s1.clone()
    _set(s5, 0, 1, float("nan"))
    _set(s5, 1, 0, float("nan"))
    _set(s5, n // 2, n // 2, INF)
    s6 = torch.maximum(R, R.t())
    for i, j in ((0, 3), (3, 0)):
        _set(s6, i, j, INF)
    for i, j in ((1, 2), (2, 1)):
        _set(s6, i, j, 1e-40)
    return torch.stack([s1, s2, s3, s4, s5, s6]).contiguous()


@functools.lru_cache(maxsize=None)
def worst_cases(n, seed=2):
    """[4, n, n]: the radix select's worst cases -- a constant matrix, all entries in [1, 1 + 2^-12] (an 8-bit
    select's passes but the last land in one bin), an all-negative matrix, and all entries in [1, 1 + 2^-13]
    (the same for the 11/11/10-bit passes of csrc/ingest.hip) (host, shared: do not modify)."""
    g = torch.Generator().manual_seed(seed)
    const = torch.full((n, n), 0.5)
    narrow = 1.0 + torch.rand(n, n, generator=g) * 2.0 ** -12
    negative = -0.1 - torch.rand(n, n, generator=g)
    narrower = 1.0 + torch.rand(n, n, generator=g) * 2.0 ** -13
    return torch.stack([const, narrow, negative, narrower]).contiguous()


def features(S, n, F=5, seed=1):
    return torch.randn(S, n, F, generator=torch.Generator().manual_seed(seed))


def labels(S):
    return torch.arange(S, dtype=torch.long) % 2
