"""The host statement of ``connectome_gnn_amd.ingest.mst_backbone`` in plain torch, for its tests.

The statement, per subject, for a matrix ``A`` ``[n, n]`` fp32 of any sign that need not be symmetric:

- ``p(x) = x if x > 0 else 0``. A NaN is not positive. ``+inf`` is positive. A subnormal is positive.
- The pair ``{i, j}``, ``i < j``, has weight ``w_ij = max(p(A_ij), p(A_ji))``. It is a candidate iff ``w_ij > 0``.
- Order: the pair ``(i, j)`` comes before ``(i', j')`` iff ``w > w'``, or ``w == w'`` and ``(i, j)`` is lexicographically
  lower. This is a strict total order.
- ``F`` is the maximum spanning forest under that order. Kruskal takes a pair iff its ends lie in different components.
  ``F`` is unique. It has ``n - c`` pairs, where ``c`` is the number of components of the candidate graph.
  - Any correct algorithm that compares edges by this strict order finds the same ``F``. That includes Prim with
    restarts from the lowest unvisited node, Boruvka and Kruskal.
  - The all-0.5 matrix gives the star at node 0.
- ``kept_ij`` iff ``i != j``, ``A_ij > 0`` and (``{i, j}`` in ``F`` or ``A_ij > t_s``). ``t_s`` is the subject's
  threshold. No thresholds means ``t_s = +inf``, the tree alone.
  - A tree pair whose reverse entry is not positive keeps only the positive direction. ``knn``'s "union" mode does the
    same.
- ``out_ij`` is the bits of ``A_ij`` where kept and ``+0.0`` elsewhere. The diagonal and every NaN become ``+0.0`` too.
- ``out`` may be ``matrices`` itself and gives the same bits. Any other overlap is refused.

``host_forest`` is Kruskal, ``brute_forest`` Prim by the 64-bit key order; both return ``F`` as a symmetric bool matrix.
``cohort(n)`` is ``knn_data.cohort(n)`` plus ``chain(n)``, ``bridge(n)`` and ``modular(n, 4)``.
"""
import functools

import torch

from tests import knn_data as K

INF = float("inf")
bits = K.bits


def _off_diagonal(n):
    return ~torch.eye(n, dtype=torch.bool)


def pair_weights(A):
    """[n, n] symmetric: ``w_ij = max(p(A_ij), p(A_ji))`` (the diagonal holds p of itself and is never looked at)."""
    P = torch.where(A > 0, A, torch.zeros_like(A))
    return torch.maximum(P, P.t())


def _mask_of(n, pairs):
    F = torch.zeros(n, n, dtype=torch.bool)
    for i, j in pairs:
        F[i, j] = F[j, i] = True
    return F


def host_forest(A):
    """bool [n, n], symmetric: ``F`` by Kruskal over a stable descending sort of the upper-triangle candidates (which
    lie in lexicographic order) with union-find, stopping once ``n - 1`` pairs are taken."""
    n = A.shape[0]
    W = pair_weights(A)
    iu = torch.triu_indices(n, n, 1)
    w = W[iu[0], iu[1]]
    cand = torch.nonzero(w > 0).flatten()
    order = cand[torch.sort(w[cand], descending=True, stable=True).indices]
    ends = iu[:, order].t().tolist()
    root = list(range(n))

    def find(v):
        while root[v] != v:
            root[v] = root[root[v]]
            v = root[v]
        return v

    taken = []
    for i, j in ends:
        if len(taken) == n - 1:
            break
        a, b = find(i), find(j)
        if a != b:
            root[max(a, b)] = min(a, b)
            taken.append((i, j))
    return _mask_of(n, taken)


def brute_forest(A):
    """bool [n, n], symmetric: ``F`` by Prim with restarts from the lowest unvisited node.  Every node outside the tree
    holds the key ``(bits(w) << 32) | (0xFFFFFFFF - (i n + j))``, ``i < j``, of its best pair into the tree, -1 without
    one; the integer maximum of the keys is the next pair."""
    n = A.shape[0]
    wb = bits(pair_weights(A)).to(torch.int64)        # (non-negative floats: the bits order as the values do)
    nodes = torch.arange(n)
    key = torch.full((n,), -1, dtype=torch.int64)
    other = torch.full((n,), -1, dtype=torch.int64)
    inside = torch.zeros(n, dtype=torch.bool)
    taken = []
    for _ in range(n):
        best = torch.where(inside, torch.full_like(key, -2), key)
        u = int(torch.argmax(best))
        if int(best[u]) < 0:                          # no pair leaves the trees so far: a new root
            u = int(torch.nonzero(~inside)[0])
        else:
            taken.append((min(u, int(other[u])), max(u, int(other[u]))))
        inside[u] = True
        lo, hi = torch.minimum(nodes, torch.tensor(u)), torch.maximum(nodes, torch.tensor(u))
        new = (wb[u] << 32) | (0xFFFFFFFF - (lo * n + hi))
        better = ~inside & (wb[u] > 0) & (new > key)
        key = torch.where(better, new, key)
        other = torch.where(better, torch.tensor(u), other)
    return _mask_of(n, taken)


def host_kept(A, t=INF, F=None):
    """bool [n, n]: ``kept``; ``F`` is ``host_forest(A)`` if the caller has it already."""
    F = host_forest(A) if F is None else F
    return _off_diagonal(A.shape[0]) & (A > 0) & (F | (A > t))


def host_backbone(A, t=INF, F=None):
    """``out`` of one subject: the bits of ``A`` where kept, +0.0 elsewhere."""
    return torch.where(host_kept(A, t, F), A, torch.zeros_like(A))


def host_backbone_cohort(mats, thr=None, forests=None):
    """``thr``: a sequence of ``S`` floats, or None for the tree alone; ``forests``: ``host_forest`` of every subject."""
    if mats.shape[0] == 0:
        return torch.zeros_like(mats)
    return torch.stack([host_backbone(A, INF if thr is None else float(thr[s]), None if forests is None else forests[s])
                        for s, A in enumerate(mats)])


def chain(n, seed=5):
    """``A[i, i+1] = A[i+1, i] = 2 - i / n``, everything else ``1e-3 rand``: the tree is one long path."""
    A = 1e-3 * torch.rand(n, n, generator=torch.Generator().manual_seed(seed))
    for i in range(n - 1):
        A[i, i + 1] = A[i + 1, i] = 2 - i / n
    return A


def bridge(n, seed=6):
    """Two dense halves (0.1 + rand inside, -rand across) whose only link is ``A[n-1, 0] = 1e-3`` with
    ``A[0, n-1] = -1``: the pair is in ``F``, and only ``out[n-1, 0]`` is kept of it."""
    g = torch.Generator().manual_seed(seed)
    half = torch.arange(n) * 2 // max(n, 1)
    same = half[:, None] == half[None, :]
    A = torch.where(same, 0.1 + torch.rand(n, n, generator=g), -torch.rand(n, n, generator=g))
    if n > 1:
        A[n - 1, 0] = 1e-3
        A[0, n - 1] = -1.0
    return A


def modular(n, M, seed=11):
    """``M`` modules, within-module weights in [0.5, 1], between-module weights in [0, 0.1], symmetric."""
    R = torch.rand(n, n, generator=torch.Generator().manual_seed(seed))
    R = torch.maximum(R, R.t())
    labels = torch.arange(n) * M // n
    A = torch.where(labels[:, None] == labels[None, :], 0.5 + 0.5 * R, 0.1 * R)
    A.fill_diagonal_(1.0)
    return A


@functools.lru_cache(maxsize=None)
def cohort(n):
    """[13, n, n] (host, shared between tests: do not modify)."""
    return torch.cat([K.cohort(n), torch.stack([chain(n), bridge(n), modular(n, 4)])]).contiguous()


@functools.lru_cache(maxsize=None)
def forests(n):
    """``host_forest`` of every subject of ``cohort(n)`` (shared: do not modify)."""
    return [host_forest(A) for A in cohort(n)]
