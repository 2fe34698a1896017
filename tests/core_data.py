"""The host statement of ``connectome_gnn_amd.ingest.core_measures`` / ``core_levels`` (``CORE_MEASURES``) in fp64, built
on tests/measures_data.py, and the seeded cohorts that its tests share.

Statement, per subject with matrix ``A`` ``[n, n]`` fp32 and threshold ``t``: ``e_ij``, ``a_ij`` and ``b_ij`` are
``measures_data.value_maps``'s (the edge test compares fp32 values, nothing is symmetrised, rows are what is summed).  For
a node set ``H``: ``k_i(H) = sum_{j in H} b_ij`` and ``s_i(H) = sum_{j in H} a_ij``.  ``peel`` is the loop of the header:
``L = 0``, ``r = 0``, all alive; while a node is alive ``r += 1``, ``L = max(L, min over alive u of p_u(alive))``, and every
alive ``u`` with ``p_u(alive) <= L`` is removed together with value ``L`` and layer ``r``.  Every ``p_u(alive)`` is formed
anew from the kept entries (a masked row sum), never by subtraction.

* ``coreness``: ``k_i / (n - 1)`` (0 for ``n == 1``), ``k_i`` the value for ``p = k``
* ``onion_layer``: ``r_i / n``, ``r_i`` the layer for ``p = k``
* ``s_coreness``: ``sigma_i / (max_i s_i(all) + 1e-8)``, ``sigma_i`` the value for ``p = s``; ``rho_i`` is its layer

Cohort: ``cohort(n)`` is ``pagerank_data.cohort(n)`` (the six clamped recipe subjects, two cliques and an isolated node, a
star) plus a clique with a path hanging off it and a threshold graph.  Every positive entry lies in ``[2^-10, 1]``, so it
is a multiple of ``2^-33`` and a row's sum is below ``2^10``: fp64 sums of a row are exact in ANY order, and the device's
result must equal this statement's rounding bit for bit.
"""
import functools
import itertools

import numpy as np
import torch

from tests import measures_data as MD
from tests import modules_data as D
from tests import pagerank_data as PD

CORE_MEASURES = ("coreness", "onion_layer", "s_coreness")
SIZES = D.SIZES
THRESHOLDS = D.THRESHOLDS
SYMMETRIC = (0, 1, 4, 5, 6, 7, 8, 9)          # the subjects of ``cohort`` whose kept entries are symmetric
ALL_ZERO, ASYMMETRIC, CLIQUES, STAR, CLIQUE_PATH, THRESHOLD_GRAPH = 2, 3, 6, 7, 8, 9


# ---- the statement ----
def peel(v):
    """(value [n], layer int64 [n]) of the value map ``v`` [n, n] (fp64 weights or int64 indicators): the loop above with
    ``p_u(alive) = sum_{j alive} v_uj``.  The values have ``v``'s dtype."""
    n = v.shape[0]
    alive = np.ones(n, dtype=bool)
    value = np.zeros(n, dtype=v.dtype)
    layer = np.zeros(n, dtype=np.int64)
    level, r = v.dtype.type(0), 0
    while alive.any():
        r += 1
        assert r <= n, "a round removes at least one node"
        p = (v * alive[None, :]).sum(1)
        level = max(level, p[alive].min())
        gone = alive & (p <= level)
        value[gone], layer[gone] = level, r
        alive &= ~gone
    return value, layer


def host_levels(A, t):
    """(k int64 [n], r int64 [n], sigma fp64 [n], rho int64 [n], max_i s_i(all)) of one subject at threshold ``t``; with
    a kept non-finite weight sigma is NaN and rho is -1."""
    a, b, _ = MD.value_maps(A, t)
    n = A.shape[0]
    k, r = peel(b)
    if not np.isfinite(a).all():
        return k, r, np.full(n, np.nan), np.full(n, -1, dtype=np.int64), np.nan
    sigma, rho = peel(a)
    return k, r, sigma, rho, float(a.sum(1).max())


def host_cores(A, t, measures=CORE_MEASURES):
    """(fp32 ``[n, len(measures)]``: the statement's values, each rounded once; int32 ``[n, 3]``: k, r, rho)."""
    n = A.shape[0]
    k, r, sigma, rho, top = host_levels(A, t)
    with np.errstate(invalid="ignore"):
        cols = {
            # one correctly rounded fp32 quotient of two integers that fp32 holds exactly
            "coreness": (k.astype(np.float32) / np.float32(n - 1)) if n > 1 else np.zeros(n, dtype=np.float32),
            "onion_layer": r.astype(np.float32) / np.float32(n),
            "s_coreness": (sigma / (top + 1e-8)).astype(np.float32),
        }
    x = torch.from_numpy(np.stack([cols[m] for m in measures], 1))
    return x, torch.from_numpy(np.stack([k, r, rho], 1).astype(np.int32))


def host_s_coreness(A, t):
    """fp64 ``[n]``: the third column before its rounding."""
    _, _, sigma, _, top = host_levels(A, t)
    return torch.from_numpy(sigma / (top + 1e-8))


@functools.lru_cache(maxsize=None)
def _cohort_statement(n, kw_key):
    mats = cohort(n)
    thr = host_thresholds(mats, dict(kw_key))
    pairs = [host_cores(A, t) for A, t in zip(mats, thr)]
    return torch.stack([x for x, _ in pairs]), torch.stack([lv for _, lv in pairs])


def cohort_statement(n, kw):
    """(fp32 ``[10, n, 3]``, int32 ``[10, n, 3]``) of ``cohort(n)`` at one of THRESHOLDS (shared between tests: do not
    modify)."""
    return _cohort_statement(n, tuple(sorted(kw.items())))


def brute_core(v):
    """``c(i) = max over H containing i of min_{u in H} p_u(H)`` over all subsets (small n only)."""
    n = v.shape[0]
    best = np.zeros(n, dtype=v.dtype)
    for size in range(1, n + 1):
        for H in itertools.combinations(range(n), size):
            idx = list(H)
            low = v[np.ix_(idx, idx)].sum(1).min()
            for i in idx:
                best[i] = max(best[i], low)
    return best


# ---- the inputs ----
CLIQUE_WEIGHT, PATH_WEIGHT = 0.5, 0.25


def clique_size(n):
    return -(-n // 3)


def _clique_path(n):
    """A clique on the first ``ceil(n / 3)`` nodes and a path through the rest that hangs off node 0."""
    A = torch.zeros(n, n)
    c = clique_size(n)
    A[:c, :c] = CLIQUE_WEIGHT
    A.fill_diagonal_(0.0)
    chain = [0] + list(range(c, n))
    for u, v in zip(chain[:-1], chain[1:]):
        A[u, v] = A[v, u] = PATH_WEIGHT
    return A


def _threshold_graph(n):
    """``i ~ j`` iff ``i + j >= n``, with weights ``(1 + i + j) / (2 n)``: nested cores, every degree occurs."""
    i = torch.arange(n)
    total = i[:, None] + i[None, :]
    A = torch.where(total >= n, (1 + total).float() / (2 * n), torch.zeros(n, n))
    A.fill_diagonal_(0.0)
    return D.clamp_weights(A)


@functools.lru_cache(maxsize=None)
def cohort(n, seed=0):
    """[10, n, n] fp32 (host, shared between tests: do not modify)."""
    out = torch.cat([PD.cohort(n, seed), torch.stack([_clique_path(n), _threshold_graph(n)])]).contiguous()
    kept = out[out > 0]
    assert bool(((kept >= D.LOW) & (kept <= D.HIGH)).all())
    return out


def host_thresholds(mats, kw):
    return D.host_thresholds(mats, kw)


def kept_entries(A, t):
    return int(MD.kept_mask(A, t).sum())


# ---- closed forms, every positive entry kept (min_weight = 0) ----
def _ranked(groups, n):
    """Disconnected regular groups ``(nodes, p)``: a group's value is its own ``p`` and its layer the rank of ``p`` among
    the distinct ones."""
    value, layer = np.zeros(n), np.zeros(n, dtype=np.int64)
    order = sorted({p for nodes, p in groups if len(nodes)})
    for nodes, p in groups:
        value[list(nodes)] = p
        layer[list(nodes)] = order.index(p) + 1 if len(nodes) else 0
    return value, layer


def expected_cliques(n, weighted):
    """(value, layer) of ``pagerank_data._cliques(n)``."""
    h = (n - 1) // 2
    first, second, lone = range(h), range(h, n - 1), [n - 1]
    w1, w2 = (0.75, 0.25) if weighted else (1, 1)
    return _ranked([(first, w1 * max(h - 1, 0)), (second, w2 * max(n - 2 - h, 0)), (lone, 0)], n)


def expected_star(n, weighted):
    """(value, layer) of ``pagerank_data._star(n)``: the leaves leave at once (binary) or one a round in ascending weight,
    the hub with the last of them (weighted)."""
    if n == 1:
        return np.zeros(1), np.ones(1, dtype=np.int64)
    if not weighted:
        layer = np.ones(n, dtype=np.int64)
        layer[0] = 2 if n > 2 else 1
        return np.ones(n), layer
    w = PD.cohort(n)[PD.STAR][0].double().numpy()
    value, layer = w.copy(), np.arange(n, dtype=np.int64)
    value[0], layer[0] = w[n - 1], n - 1
    return value, layer


def expected_clique_path(n, weighted):
    """(value, layer) of ``_clique_path(n)`` for a clique of at least 3 nodes (``n >= 7``), else None: the path is eaten
    from its far end, one node a round, then the clique leaves together."""
    c = clique_size(n)
    if c < 3:
        return None
    m = n - c
    value, layer = np.zeros(n), np.zeros(n, dtype=np.int64)
    value[:c] = (CLIQUE_WEIGHT if weighted else 1) * (c - 1)
    layer[:c] = m + 1
    value[c:] = PATH_WEIGHT if weighted else 1
    layer[c:] = np.arange(m, 0, -1)
    return value, layer
