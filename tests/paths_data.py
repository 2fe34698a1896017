"""The host statement of the shortest-path node measures of ``connectome_gnn_amd.ingest`` (``PATH_MEASURES``) in
fp64 / int64, on the thresholds and recipes of tests/ingest_data.py, and structured graphs with known distances.

Statement, per subject with matrix ``A`` ``[n, n]`` fp32 and threshold ``t``: ``e_ij`` iff ``i != j``, ``A_ij > t`` and
``A_ij > 0`` (``measures_data.kept_mask``); nothing is symmetrised.  ``d_ij`` is the number of edges on a shortest
directed path ``i -> ... -> j`` along kept edges (the out-neighbours of a row), infinite (-1 here) if there is none.
``R_i = {j != i : d_ij finite}``, ``r_i = |R_i|``; ``N_i = {j : e_ij}``, ``k_i = |N_i|``; ``d^(i)`` are the distances
inside the subgraph induced on ``N_i`` (only edges ``e_jh`` with both ends in ``N_i``).

* ``nodal_efficiency``: ``(1 / (n - 1)) sum_{j in R_i} 1 / d_ij``, 0 for ``n == 1``
* ``closeness``: ``(r_i / (n - 1)) (r_i / sum_{j in R_i} d_ij)`` if ``r_i > 0``, else 0 (Wasserman-Faust)
* ``eccentricity``: ``max_{j in R_i} d_ij / (n - 1)``, 0 if ``r_i == 0`` or ``n == 1``
* ``local_efficiency``: ``(1 / (k_i (k_i - 1))) sum_{j != h in N_i} 1 / d^(i)_jh`` if ``k_i >= 2``, else 0

Everything after the edge test is int64 or fp64; ``sum_{j in R_i} 1 / d_ij`` is formed as ``sum_l count_l / l`` over the
level counts in ascending ``l``.
"""
import functools

import numpy as np
import torch

from connectome_gnn_amd import synthetic
from tests.ingest_data import host_threshold, rank_of, recipe  # noqa: F401  (re-exported for the tests)
from tests.measures_data import kept_mask

PATH_MEASURES = ("nodal_efficiency", "closeness", "eccentricity", "local_efficiency")
STRUCTURED = ("ring", "directed_path", "path", "star", "cliques", "complete", "watts_strogatz")


def distances(mask):
    """int64 ``[n, n]``: ``d_ij`` along the out-neighbours ``mask[i]``, -1 where ``j`` is not reached, 0 on the
    diagonal.  All sources advance one level per step; a step costs what the frontiers' edges cost, and a source that
    has reached every node is not expanded again."""
    mask = np.asarray(mask, dtype=bool)
    n = mask.shape[0]
    deg = mask.sum(1)
    indptr = np.concatenate([[0], np.cumsum(deg)])
    indices = np.nonzero(mask)[1]
    D = np.full(n * n, -1, dtype=np.int64)
    D[np.arange(n) * (n + 1)] = 0
    src = u = np.arange(n)
    left = np.full(n, n - 1, dtype=np.int64)            # nodes a source has not reached yet
    level = 0
    while src.size:
        level += 1
        cnt = deg[u]
        total = int(cnt.sum())
        first = np.cumsum(cnt) - cnt                    # where (src, u)'s neighbours start in the expansion
        slot = np.arange(total) - np.repeat(first, cnt) + np.repeat(indptr[u], cnt)
        key = np.unique(np.repeat(src, cnt) * n + indices[slot])
        key = key[D[key] < 0]
        D[key] = level
        src, u = key // n, key % n
        left -= np.bincount(src, minlength=n)
        more = left[src] > 0
        src, u = src[more], u[more]
    return D.reshape(n, n)


def level_counts(D):
    """int64 ``[n, L + 1]``: ``counts[i, l]`` nodes at distance ``l`` from ``i`` (column 0 is the node itself)."""
    n = D.shape[0]
    L = int(D.max()) if n else 0
    counts = np.zeros((n, L + 1), dtype=np.int64)
    for i in range(n):
        counts[i] = np.bincount(D[i][D[i] >= 0], minlength=L + 1)
    return counts


def inverse_distance_sums(D):
    """fp64 ``[n]``: ``sum_l count_l / l``, ascending ``l``."""
    counts = level_counts(D)
    out = np.zeros(D.shape[0])
    for lvl in range(1, counts.shape[1]):
        out += counts[:, lvl] / float(lvl)
    return out


def exact_integers(D):
    """(r_i, sum_j d_ij, max_j d_ij) over the reached ``j != i``, int64 ``[n]`` each."""
    reached = D > 0
    return reached.sum(1), np.where(reached, D, 0).sum(1), np.where(reached, D, 0).max(1, initial=0)


def local_efficiency(mask, nodes=None):
    """fp64: the local efficiency of every node (or of ``nodes``)."""
    mask = np.asarray(mask, dtype=bool)
    nodes = range(mask.shape[0]) if nodes is None else nodes
    out = []
    for i in nodes:
        N = np.flatnonzero(mask[i])
        k = N.size
        if k < 2:
            out.append(0.0)
            continue
        out.append(float(inverse_distance_sums(distances(mask[np.ix_(N, N)])).sum()) / (k * (k - 1.0)))
    return np.asarray(out, dtype=np.float64)


def mask_measures(mask, measures=PATH_MEASURES, local_nodes=None):
    """fp64 ``[n, len(measures)]`` of one kept set; with ``local_nodes`` the local efficiency is computed for those
    nodes only and is NaN elsewhere."""
    mask = np.asarray(mask, dtype=bool)
    n = mask.shape[0]
    D = distances(mask)
    r, sum_d, ecc = exact_integers(D)
    cols = {}
    if n > 1:
        cols["nodal_efficiency"] = inverse_distance_sums(D) / (n - 1)
        cols["closeness"] = np.where(r > 0, (r / (n - 1)) * (r / np.where(r > 0, sum_d, 1)), 0.0)
        cols["eccentricity"] = ecc / (n - 1)
    else:
        cols["nodal_efficiency"] = cols["closeness"] = cols["eccentricity"] = np.zeros(n)
    if "local_efficiency" in measures:
        if local_nodes is None:
            cols["local_efficiency"] = local_efficiency(mask)
        else:
            cols["local_efficiency"] = np.full(n, np.nan)
            cols["local_efficiency"][list(local_nodes)] = local_efficiency(mask, local_nodes)
    return torch.from_numpy(np.stack([cols[m] for m in measures], 1).astype(np.float64))


def host_measures(A, t, measures=PATH_MEASURES):
    """fp64 ``[n, len(measures)]`` of one subject at threshold ``t``."""
    return mask_measures(kept_mask(A, t), measures)


def host_integers(A, t):
    """(r_i, sum d, ecc_i) as exact int64 ``[n]`` tensors."""
    return tuple(torch.from_numpy(v) for v in exact_integers(distances(kept_mask(A, t))))


def cohort_measures(mats, thr, measures=PATH_MEASURES):
    """fp64 ``[S, n, F]``: ``thr`` is a sequence of floats, one per subject."""
    return torch.stack([host_measures(A, float(t), measures) for A, t in zip(mats, thr)])


def unreachable_pairs(A, t):
    """The number of ordered pairs ``i != j`` without a path."""
    return int((distances(kept_mask(A, t)) < 0).sum())


# ---- structured graphs: distinct positive weights on the intended edges, 0 elsewhere; used at min_weight = 0 ----
def _pairs(kind, n):
    """(rows, columns) of the directed edges of one structured graph."""
    idx = np.arange(n)
    if kind == "ring":                                  # i <-> i + 1 mod n: diameter n // 2
        u, v = idx, (idx + 1) % n
    elif kind == "directed_path":                       # i -> i + 1 only: eccentricity n - 1 - i
        return idx[:-1], idx[1:]
    elif kind == "path":                                # i <-> i + 1: diameter n - 1, sum d at its maximum
        u, v = idx[:-1], idx[1:]
    elif kind == "star":                                # 0 <-> every other node
        u, v = np.zeros(n - 1, dtype=np.int64), idx[1:]
    elif kind == "cliques":                             # two disjoint cliques and the isolated node n - 1
        a = (n - 1) // 2
        parts = [np.arange(0, a), np.arange(a, n - 1)]
        u = np.concatenate([np.repeat(p, p.size) for p in parts])
        v = np.concatenate([np.tile(p, p.size) for p in parts])
    elif kind == "complete":
        u, v = np.repeat(idx, n), np.tile(idx, n)
    elif kind == "watts_strogatz":
        u, v = synthetic._ws_pairs(n, min(6, (n - 1) // 2 * 2), 0.2, np.random.default_rng(n))
    else:
        raise KeyError(kind)
    keep = u != v
    u, v = u[keep], v[keep]
    return np.concatenate([u, v]), np.concatenate([v, u])


@functools.lru_cache(maxsize=None)
def structured(kind, n):
    """``[n, n]`` fp32 (host, shared between tests: do not modify)."""
    A = torch.zeros(n, n)
    r, c = _pairs(kind, n)
    if r.size:
        A[torch.from_numpy(r), torch.from_numpy(c)] = 1.0
    edges = A > 0
    A[edges] = 0.25 + torch.arange(1, int(edges.sum()) + 1, dtype=torch.float32) / 2 ** 21     # distinct, exact
    return A.contiguous()


@functools.lru_cache(maxsize=None)
def structured_cohort(n):
    """``[7, n, n]``: every structured graph at one size, in the order of ``STRUCTURED``."""
    return torch.stack([structured(kind, n) for kind in STRUCTURED]).contiguous()
