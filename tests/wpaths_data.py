"""The host statement of the weighted shortest-path node measures of ``connectome_gnn_amd.ingest``
(``WEIGHTED_PATH_MEASURES``, ``path_lengths``) in fp64 from the fp32 inputs, on the thresholds and recipes of
tests/ingest_data.py, and structured graphs that carry random weights.

Statement, per subject with matrix ``A`` ``[n, n]`` fp32 and threshold ``t``: ``e_ij`` iff ``i != j``, ``A_ij > t`` and
``A_ij > 0`` (``measures_data.kept_mask``); nothing is symmetrised.  ``wmax = max_{e_ij} A_ij`` and
``l_ij = float64(wmax) / float64(A_ij)`` where ``e_ij``.  ``dw_ij`` is the smallest sum of lengths along a directed path
``i -> ... -> j`` of kept edges (``scipy.sparse.csgraph.dijkstra``, ``directed=True``), 0 on the diagonal, ``+inf``
without a path.  ``R_i = {j != i : dw_ij finite}``, ``r_i = |R_i|``.

* ``weighted_nodal_efficiency``: ``(1 / (n - 1)) sum_{j in R_i} 1 / dw_ij``, 0 for ``n == 1``
* ``weighted_closeness``: ``(r_i / (n - 1)) (r_i / sum_{j in R_i} dw_ij)`` if ``r_i > 0``, else 0 (Wasserman-Faust)
* ``weighted_eccentricity``: ``max_{j in R_i} dw_ij / (n - 1)``, 0 if ``r_i == 0`` or ``n == 1``

``H`` is the largest number of edges on the shortest paths Dijkstra found: what the fp32 error of a distance scales with.
"""
import functools

import numpy as np
import torch
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import dijkstra

from tests import paths_data as P
from tests.ingest_data import host_threshold, rank_of, recipe  # noqa: F401  (re-exported for the tests)
from tests.measures_data import kept_mask

WEIGHTED_PATH_MEASURES = ("weighted_nodal_efficiency", "weighted_closeness", "weighted_eccentricity")
SUBJECTS = (0, 3, 4)        # of ingest_data.recipe: symmetric, asymmetric, symmetric with NaN entries
SYMMETRIC, ASYMMETRIC = (0, 2), 1                    # positions in SUBJECTS


def lengths(A, t):
    """(mask bool ``[n, n]``, fp64 ``[n, n]`` lengths, ``+inf`` where there is no edge)."""
    mask = kept_mask(A, t)
    a = A.numpy().astype(np.float64)
    L = np.full(a.shape, np.inf)
    if mask.any():
        L[mask] = float(a[mask].max()) / a[mask]
    return mask, L


def distances(A, t):
    """(fp64 ``[n, n]`` ``dw``, ``H``)."""
    mask, L = lengths(A, t)
    n = mask.shape[0]
    r, c = np.nonzero(mask)
    graph = csr_matrix((L[r, c], (r, c)), shape=(n, n))
    D, pred = dijkstra(graph, directed=True, return_predecessors=True)
    D = np.asarray(D, dtype=np.float64).reshape(n, n)
    # edges on the paths found: hops[i, j] = hops[i, pred[i, j]] + 1, settled level by level
    hops = np.where(np.eye(n, dtype=bool), 0, -1)
    has = pred >= 0
    before = np.where(has, pred, 0)
    while True:
        via = np.take_along_axis(hops, before, 1)
        new = np.where(has & (via >= 0) & (hops < 0), via + 1, hops)
        if np.array_equal(new, hops):
            break
        hops = new
    assert np.array_equal(hops >= 0, np.isfinite(D))
    return D, int(hops.max(initial=0))


def measures_of(D):
    """fp64 ``[n, 3]`` from ``dw``."""
    n = D.shape[0]
    reached = np.isfinite(D) & ~np.eye(n, dtype=bool)
    r = reached.sum(1)
    if n == 1:
        return torch.zeros(1, 3, dtype=torch.float64)
    inv = np.where(reached, 1.0 / np.where(reached, D, 1.0), 0.0).sum(1)
    total = np.where(reached, D, 0.0).sum(1)
    far = np.where(reached, D, 0.0).max(1, initial=0.0)
    close = np.where(r > 0, (r / (n - 1)) * (r / np.where(r > 0, total, 1.0)), 0.0)
    return torch.from_numpy(np.stack([inv / (n - 1), close, far / (n - 1)], 1))


def host_statement(A, t):
    """(``dw`` fp64 ``[n, n]`` tensor, measures fp64 ``[n, 3]``, ``H``) of one subject at threshold ``t``."""
    D, H = distances(A, float(t))
    return torch.from_numpy(D), measures_of(D), H


@functools.lru_cache(maxsize=None)
def cohort(n):
    """``[3, n, n]`` fp32: the subjects ``SUBJECTS`` of the recipe (host, shared between tests: do not modify)."""
    return recipe(n)[list(SUBJECTS)].contiguous()


def thresholds(mats, keep):
    return [host_threshold(A, rank_of(mats.shape[1], keep=keep)) for A in mats]


@functools.lru_cache(maxsize=None)
def cohort_statement(n, keep):
    """[(dw, measures, H)] of ``cohort(n)`` at ``keep``, computed once."""
    mats = cohort(n)
    return [host_statement(A, t) for A, t in zip(mats, thresholds(mats, keep))]


# ---- structured graphs: the masks of paths_data.STRUCTURED carrying seeded random weights in [0.05, 1] ----
STRUCTURED = P.STRUCTURED


@functools.lru_cache(maxsize=None)
def structured(kind, n):
    """``[n, n]`` fp32, one weight per directed edge (host, shared between tests: do not modify); used at
    ``min_weight = 0``."""
    mask = P.structured(kind, n) > 0
    g = torch.Generator().manual_seed(1000 * STRUCTURED.index(kind) + n)
    w = 0.05 + 0.95 * torch.rand(n, n, generator=g)
    return torch.where(mask, w, torch.zeros(n, n)).contiguous()


@functools.lru_cache(maxsize=None)
def structured_cohort(n):
    """``[7, n, n]``: every structured graph at one size, in the order of ``STRUCTURED``."""
    return torch.stack([structured(kind, n) for kind in STRUCTURED]).contiguous()


def equal_weights(mats, thr, value=0.7):
    """The kept sets of ``mats`` at ``thr`` with one weight on every edge: ``[S, n, n]`` fp32, used at
    ``min_weight = 0``."""
    return torch.stack([torch.from_numpy(kept_mask(A, float(t))).float() * value for A, t in zip(mats, thr)]).contiguous()
