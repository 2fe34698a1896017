"""The host statement of ``connectome_gnn_amd.ingest.group_matrix`` / ``group_sparsify`` in plain torch, for their tests.

The statement (include/cgnn_group.h), for a cohort ``mats`` ``[S, n, n]`` fp32 of any sign; a subject is a *unit*:

- ``among`` (bool ``[S]`` or None) says which units are *included*; ``N`` is their number.  An excluded unit is never
  looked at.
- The sum, per entry ``(i, j)``, in fp64, in the header's order: the units are cut into slices of ``SLICE`` consecutive
  units; a slice's partial starts at ``0.0`` and adds the terms of its included units in ascending order; the partials
  are folded in ascending slice order from ``0.0``.
- ``mean``: the term is ``A_sij``; ``G_ij = sum / N``.
- ``fisher_mean``: the term is ``atanh(A_sij)``; ``G_ij = tanh(sum / N)``, fp64 ``atanh`` and ``tanh``.
- ``consistency``: the term is 1 iff ``i != j and A_sij > t_s and A_sij > 0`` (``ingest_data.host_edges``'s rule at the
  unit's own threshold ``t_s``, ``ingest_data.host_threshold``'s), an exact integer count; ``G_ij = count / N``.
- One fp64 division and one rounding to fp32.  Nothing is special-cased: ``N == 0`` gives NaN everywhere; a NaN in an
  included unit makes that entry NaN; ``+inf`` and ``-inf`` in the same entry give NaN; ``|r| == 1`` goes through ``atanh``
  as ``+-inf``; the diagonal is reduced like any entry, except that ``consistency`` leaves it at 0; a bit-symmetric cohort
  gives a bit-symmetric group matrix.
- The group edge set: the edge choice (one of the thresholds; or ``knn`` / ``knn_mode``; with or without the ``"mst"``
  backbone) applied to ``G`` as a cohort of one unit gives ``(G', t)``; ``E = {(i, j): i != j, G'_ij > t, G'_ij > 0}``.  A
  NaN group entry is never an edge.
- The mask: ``out_sij`` is the bits of ``A_sij`` if ``(i, j)`` is in ``E`` and ``A_sij > 0``, else ``+0.0`` (the diagonal,
  every NaN and ``-0.0`` too).
"""
import functools

import numpy as np
import torch

from connectome_gnn_amd._lib import GROUP_SLICE as SLICE    # CGNN_GROUP_SLICE of include/cgnn_group.h
from tests import ingest_data as D
from tests import knn_data as K
from tests import mst_data as M

INF = float("inf")
STATISTICS = ("mean", "fisher_mean", "consistency")
bits = K.bits


def _off_diagonal(n):
    return ~torch.eye(n, dtype=torch.bool)


def included(S, among=None):
    return [s for s in range(S) if among is None or bool(among[s])]


def host_sum(term, S, n, among=None, slice_=SLICE):
    """fp64 [n, n]: ``term(s)`` (fp64 [n, n]) over the included units in the header's order."""
    total = torch.zeros(n, n, dtype=torch.float64)
    for lo in range(0, S, slice_):
        partial = torch.zeros(n, n, dtype=torch.float64)
        for s in range(lo, min(S, lo + slice_)):
            if among is None or bool(among[s]):
                partial = partial + term(s)
        total = total + partial
    return total


def host_unit_thresholds(mats, keep=None, num_edges=None, min_weight=None):
    """``t_s`` of every unit for exactly one of the three, as ``from_matrices`` chooses them (a list of floats)."""
    n = mats.shape[1]
    if min_weight is not None:
        return [float(t) for t in min_weight] if isinstance(min_weight, torch.Tensor) else [float(min_weight)] * len(mats)
    k = D.rank_of(n, keep=keep, num_edges=num_edges)
    return [D.host_threshold(A, k) for A in mats]


def host_group(mats, statistic, thr=None, among=None, exact=False):
    """``G`` [n, n] fp32 (``exact``: fp64 before the one rounding); ``thr``: the units' thresholds, for the consistency."""
    S, n = int(mats.shape[0]), int(mats.shape[1])
    if statistic == "mean":
        term = lambda s: mats[s].double()
    elif statistic == "fisher_mean":
        term = lambda s: torch.atanh(mats[s].double())
    else:
        assert statistic == "consistency" and thr is not None, statistic
        off = _off_diagonal(n)
        term = lambda s: ((mats[s] > thr[s]) & (mats[s] > 0) & off).double()
    N = torch.tensor(float(len(included(S, among))), dtype=torch.float64)
    v = host_sum(term, S, n, among) / N
    if statistic == "fisher_mean":
        v = torch.tanh(v)
    return v if exact else v.float()


def host_edge_set(G, keep=None, num_edges=None, min_weight=None, knn=None, knn_mode="union", backbone=None):
    """bool [n, n]: ``E``, the edge choice on the group matrix as a cohort of one unit."""
    n = G.shape[0]
    t = None
    if min_weight is not None:
        t = float(min_weight[0]) if isinstance(min_weight, torch.Tensor) else float(min_weight)
    elif keep is not None or num_edges is not None:
        t = D.host_threshold(G, D.rank_of(n, keep=keep, num_edges=num_edges))
    if knn is not None:
        kept = K.host_kept(G, knn, knn_mode)
        return kept | M.host_kept(G, INF) if backbone else kept
    if backbone:
        return M.host_kept(G, INF if t is None else t)
    return (G > t) & (G > 0) & _off_diagonal(n)


def host_mask(mats, E):
    """[S, n, n]: every unit's bits where ``E`` holds and the entry is positive, +0.0 elsewhere."""
    return torch.where(E[None] & (mats > 0), mats, torch.zeros_like(mats))


def host_group_sparsify(mats, group="mean", **choice):
    G = host_group(mats, group) if isinstance(group, str) else group
    return host_mask(mats, host_edge_set(G, **choice))


@functools.lru_cache(maxsize=None)
def cohort(S, n, seed=3):
    """[S, n, n]: ``ingest_data.recipe(n)`` repeated with seeded noise.  The first six units (and the next six) are exact
    copies, so the NaN, the +inf, the subnormal and the heavy ties are there; one -inf meets the +inf of unit 5 where
    both exist (host, shared between tests: do not modify)."""
    g = torch.Generator().manual_seed(seed * 1000 + 7 * S + n)
    base = D.recipe(n).repeat((S + 5) // 6, 1, 1)[:S]
    mats = (base + 0.01 * torch.randn(S, n, n, generator=g)).contiguous()
    mats[:min(S, 12)] = base[:min(S, 12)]
    if n > 3 and S > 6:
        mats[6, 0, 3] = -INF
    return mats


@functools.lru_cache(maxsize=None)
def correlations(S, n, seed=5):
    """[S, n, n]: symmetric values in (-1, 1) with a unit diagonal, an exact -1 and an exact +1 off the diagonal
    (host, shared: do not modify)."""
    g = torch.Generator().manual_seed(seed * 1000 + 7 * S + n)
    R = torch.tanh(0.6 * torch.randn(S, n, n, generator=g))
    R = ((R + R.transpose(1, 2)) / 2).clamp(-0.999, 0.999)
    R[:, torch.arange(n), torch.arange(n)] = 1.0
    if n > 2:
        R[0, 0, 2] = R[0, 2, 0] = -1.0
        R[S - 1, 1, 2] = R[S - 1, 2, 1] = 1.0
    return R.contiguous()


@functools.lru_cache(maxsize=None)
def modular_series_cohort(S=12, T=120, n=84, modules=4, seed=0):
    """[S, n, n] fp32: Pearson correlations (fp64, rounded once) of ``0.6 * module signal + noise``, seeded (host,
    shared: do not modify)."""
    rng = np.random.default_rng(seed)
    labels = np.arange(n) * modules // n
    out = []
    for _ in range(S):
        x = 0.6 * rng.standard_normal((T, modules))[:, labels] + rng.standard_normal((T, n))
        out.append(np.corrcoef(x, rowvar=False))
    return torch.from_numpy(np.stack(out)).float().contiguous()


def jaccard(a, b):
    return float((a & b).sum()) / float((a | b).sum())
