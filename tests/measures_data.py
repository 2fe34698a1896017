"""The host statement of ``connectome_gnn_amd.ingest.node_measures`` in fp64, on the thresholds and recipes of
tests/ingest_data.py.

Statement, per subject with matrix ``A`` ``[n, n]`` fp32 and threshold ``t``: ``e_ij`` iff ``i != j``, ``A_ij > t`` and
``A_ij > 0`` (``ingest_data.host_edges``); ``a_ij = A_ij`` and ``b_ij = 1`` where ``e_ij``, else 0; ``k_i = sum_j b_ij``;
``s_i = sum_j a_ij``; ``wmax = max a_ij``; ``u_ij = cbrt(a_ij / wmax)`` where ``e_ij``, else 0; for a value map ``v``,
``T_i(v) = sum_{j,k} v_ki v_kj v_ij``.

* ``strength``: ``s_i / (max_i s_i + 1e-8)``
* ``degree``: ``k_i / (n - 1)``, 0 for ``n == 1``
* ``mean_weight``: ``s_i / (k_i + 1e-8)``
* ``clustering``: ``T_i(b) / (k_i (k_i - 1))`` if ``k_i >= 2``, else 0
* ``weighted_clustering``: ``T_i(u) / (k_i (k_i - 1))`` if ``k_i >= 2``, else 0

Nothing is symmetrised: for an asymmetric ``A`` the formula is the definition.  Everything after the edge test (which
compares fp32 values) is fp64; ``k_i`` and ``T_i(b)`` are also given as exact integers.
"""
import numpy as np
import torch

from tests.ingest_data import host_threshold, rank_of, recipe  # noqa: F401  (re-exported for the tests)

MEASURES = ("strength", "degree", "mean_weight", "clustering", "weighted_clustering")
TILE = 96


def kept_mask(A, t):
    """bool [n, n]: the edge test of ``from_matrices`` (numpy, from an fp32 torch matrix)."""
    n = A.shape[0]
    return ((A > t) & (A > 0) & ~torch.eye(n, dtype=torch.bool)).numpy()


def triangles(V):
    """``T_i(v) = sum_{j,k} v_ki v_kj v_ij`` for a value map ``V`` ``[n, n]`` (fp64 or int64)."""
    return ((V.T @ V) * V).sum(1)


def value_maps(A, t):
    """(a, b, u): kept weights fp64, kept indicator int64, cube roots of the weights scaled by their maximum fp64."""
    mask = kept_mask(A, t)
    a = np.where(mask, A.numpy().astype(np.float64), 0.0)
    b = mask.astype(np.int64)
    wmax = a.max() if a.size else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(mask, np.cbrt(a / wmax), 0.0)
    return a, b, u


def host_measures(A, t, measures=MEASURES):
    """fp64 ``[n, len(measures)]`` of one subject at threshold ``t``."""
    n = A.shape[0]
    a, b, u = value_maps(A, t)
    k = b.sum(1).astype(np.float64)
    s = a.sum(1)
    pairs = k * (k - 1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        cols = {
            "strength": s / (s.max() + 1e-8),
            "degree": k / (n - 1) if n > 1 else np.zeros(n),
            "mean_weight": s / (k + 1e-8),
            "clustering": np.where(k >= 2, triangles(b).astype(np.float64) / np.where(k >= 2, pairs, 1.0), 0.0),
            "weighted_clustering": np.where(k >= 2, triangles(u) / np.where(k >= 2, pairs, 1.0), 0.0),
        }
    return torch.from_numpy(np.stack([cols[m] for m in measures], 1))


def host_counts(A, t):
    """(k_i, T_i(b)) as exact int64 ``[n]`` tensors."""
    _, b, _ = value_maps(A, t)
    return torch.from_numpy(b.sum(1)), torch.from_numpy(triangles(b))


def finite_weights(A, t):
    """True when no kept weight of the subject is non-finite (the weight-valued measures are then checked)."""
    return bool(np.isfinite(A.numpy()[kept_mask(A, t)]).all())


def cohort_measures(mats, thr, measures=MEASURES):
    """fp64 ``[S, n, F]``: ``thr`` is a sequence of floats, one per subject."""
    return torch.stack([host_measures(A, float(t), measures) for A, t in zip(mats, thr)])


def tiled_triangles(V, tile=TILE):
    """``T_i(v)`` the way csrc/measures.hip sums it: for every tile pair ``bi <= bj`` of ``G = V^T V`` the row sums
    of ``G_ij v_ij`` go to the nodes of ``bi``; off the diagonal the column sums of ``G_ij v_ji`` go to the nodes of
    ``bj`` (the mirrored pair is never formed).  Returns (T [n], slots written [nt, nt * tile] as counts)."""
    n = V.shape[0]
    nt = -(-n // tile)
    P = np.zeros((nt * tile, nt * tile), dtype=V.dtype)
    P[:n, :n] = V
    part = np.zeros((nt, nt * tile), dtype=V.dtype)
    written = np.zeros((nt, nt * tile), dtype=np.int64)
    for bi in range(nt):
        for bj in range(bi, nt):
            ri, rj = slice(bi * tile, (bi + 1) * tile), slice(bj * tile, (bj + 1) * tile)
            G = P[:, ri].T @ P[:, rj]
            part[bj, ri] += (G * P[ri, rj]).sum(1)
            written[bj, ri] += 1
            if bi != bj:
                part[bi, rj] += (G * P[rj, ri].T).sum(0)
                written[bi, rj] += 1
    return part.sum(0)[:n], written
