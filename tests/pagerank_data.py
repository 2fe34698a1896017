"""The host statement of ``connectome_gnn_amd.ingest.centrality_measures`` (``CENTRALITY_MEASURES``) in fp64, built on
tests/measures_data.py, a numpy model of the kernel's iteration, and the seeded cohorts that its tests share.

Statement, per subject with matrix ``A`` ``[n, n]`` fp32, threshold ``t`` and damping ``d``: ``e_ij`` and the value maps
are ``measures_data.value_maps``'s (the edge test compares fp32 values, nothing is symmetrised); entry ``(i, j)`` is an
edge ``j -> i``; ``w_ij = a_ij`` (``weighted_pagerank``) or ``b_ij`` (``pagerank``); ``c_j = sum_i w_ij``; a node with
``c_j == 0`` is dangling.  With the Google matrix ``G_ij = w_ij / c_j`` (``1 / n`` in the column of a dangling ``j``),
``x`` solves ``(I - d G) x = (1 - d) / n``: ``numpy.linalg.solve`` in fp64.  ``G`` is column stochastic, so ``x`` sums
to 1 and ``I - d G`` has condition number at most ``(1 + d) / (1 - d)`` in the 1-norm.

Cohort: ``cohort(n)`` is ``modules_data.cohort(n)`` (the six recipe subjects of tests/ingest_data.py with every positive
entry clamped into ``[2^-10, 1]``: a symmetric Gaussian matrix, ties, all zeros, an asymmetric uniform matrix, NaNs,
negatives) plus two more subjects: two disjoint cliques and an isolated node, and a star.
"""
import functools
import math

import numpy as np
import torch

from tests import measures_data as MD
from tests import modules_data as D

CENTRALITY_MEASURES = ("pagerank", "weighted_pagerank")
SIZES = D.SIZES
THRESHOLDS = D.THRESHOLDS
DAMPINGS = (0.5, 0.85)
SYMMETRIC = (0, 1, 4, 5, 6, 7)                # the subjects of ``cohort`` whose kept entries are symmetric
ALL_ZERO, ASYMMETRIC, CLIQUES, STAR = 2, 3, 6, 7


# ---- the statement ----
def weights(A, t, name):
    """fp64 ``[n, n]``: ``w_ij`` of one subject for one name."""
    a, b, _ = MD.value_maps(A, t)
    return a if name == "weighted_pagerank" else b.astype(np.float64)


def google_matrix(w):
    """fp64 ``[n, n]``, column stochastic: ``w_ij / c_j``, and ``1 / n`` in the column of a dangling node."""
    n = w.shape[0]
    c = w.sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(c[None, :] == 0, 1.0 / n, w / c[None, :])


def host_pagerank(A, t, d, name):
    """fp64 ``[n]`` of one subject: the solve."""
    n = A.shape[0]
    G = google_matrix(weights(A, t, name))
    return np.linalg.solve(np.eye(n) - d * G, np.full(n, (1.0 - d) / n))


def host_centrality(A, t, d, measures=CENTRALITY_MEASURES):
    """fp64 ``[n, len(measures)]`` of one subject at threshold ``t``."""
    return torch.from_numpy(np.stack([host_pagerank(A, t, d, m) for m in measures], 1))


@functools.lru_cache(maxsize=None)
def _cohort_statement(n, kw_key, d):
    mats = cohort(n)
    thr = host_thresholds(mats, dict(kw_key))
    out = torch.stack([host_centrality(A, t, d) for A, t in zip(mats, thr)])
    return out


def cohort_statement(n, kw, d):
    """fp64 ``[8, n, 2]`` of ``cohort(n)`` at one of THRESHOLDS (shared between tests: do not modify)."""
    return _cohort_statement(n, tuple(sorted(kw.items())), d)


# ---- the kernel's iteration, in numpy ----
def max_steps(d):
    """``K_max(d) = ceil(43 ln 2 / -ln d) + 2`` (2 for ``d == 0``).  A product contracts at rate ``d`` in L1 and the start
    is at most 2 away; a step is two products, so step ``K`` changes by at most ``2 (1 + d) d^(2 K - 1)``, which at
    ``K_max`` is below ``2^-84``: the stopping rule holds before the cap in exact arithmetic."""
    return int(math.ceil(43.0 * math.log(2.0) / -math.log(d))) + 2 if d > 0 else 2


def model(A, t, d, name):
    """(x fp64 [n], steps): fp64, start ``1 / n``, a step is two products ``x -> T(T(x))`` as in the kernel, stop at the
    first step whose L1 change is at most ``(1 - d) 2^-42``, at most ``max_steps(d)`` steps."""
    n = A.shape[0]
    w = weights(A, t, name)
    c = w.sum(0)
    dangling = c == 0
    x = np.full(n, 1.0 / n)
    tol = (1.0 - d) * 2.0 ** -42

    def product(v):
        with np.errstate(invalid="ignore", divide="ignore"):
            y = np.where(dangling, 0.0, v / c)
        return d * (w @ y + v[dangling].sum() / n) + (1.0 - d) / n

    for k in range(1, max_steps(d) + 1):
        new = product(product(x))
        change = np.abs(new - x).sum()
        x = new
        if change <= tol:
            break
    return x, k


# ---- the inputs ----
def _cliques(n):
    """Two disjoint cliques over nodes ``0 .. n - 2`` with different weights, node ``n - 1`` isolated."""
    A = torch.zeros(n, n)
    h = (n - 1) // 2
    A[:h, :h] = 0.75
    A[h:n - 1, h:n - 1] = 0.25
    A.fill_diagonal_(0.0)
    return A


def _star(n):
    """Node 0 joined to every other node, with weights that grow with the node."""
    A = torch.zeros(n, n)
    if n > 1:
        w = 0.25 + 0.5 * torch.arange(1, n, dtype=torch.float32) / n
        A[0, 1:] = w
        A[1:, 0] = w
    return A


@functools.lru_cache(maxsize=None)
def cohort(n, seed=0):
    """[8, n, n] fp32 (host, shared between tests: do not modify)."""
    return torch.cat([D.cohort(n, seed), torch.stack([_cliques(n), _star(n)])]).contiguous()


def host_thresholds(mats, kw):
    return D.host_thresholds(mats, kw)


def kept_entries(A, t):
    return int(MD.kept_mask(A, t).sum())
