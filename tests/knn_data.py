"""The host statement of ``connectome_gnn_amd.ingest.knn_sparsify`` in plain torch, for its tests.

Statement, per subject with matrix ``A`` ``[n, n]`` fp32: the candidates of row ``i`` are the ``j != i`` with
``A[i, j] > 0`` (a NaN is not positive, +inf is), ``p_i`` of them; they are sorted by descending value, the sort being
stable, so equal values stay in column order; the row's picks ``d[i]`` are the first ``min(k, p_i)``.  ``"directed"``
keeps ``d``, ``"union"`` ``d | (d^T & (A > 0))``, ``"mutual"`` ``d & d^T``; the output is ``A`` where kept and ``+0.0``
elsewhere.  The matrices are those of ``tests/ingest_data.py``: ``cohort(n)`` is its six recipe subjects followed by its
four worst cases.
"""
import functools

import torch

from tests import ingest_data as D

MODES = ("union", "mutual", "directed")
INF = float("inf")


def _off_diagonal(n):
    return ~torch.eye(n, dtype=torch.bool)


def candidates(A):
    """bool [n, n]: the positive off-diagonal entries."""
    return (A > 0) & _off_diagonal(A.shape[0])


def host_picks(A, k):
    """bool [n, n]: ``d``, by a stable descending sort of every row's candidates."""
    n = A.shape[0]
    cand = candidates(A)
    keyed = torch.where(cand, A, torch.full_like(A, -INF))            # (no candidate is -inf: they sort last)
    order = torch.sort(keyed, dim=1, descending=True, stable=True).indices
    position = torch.empty_like(order)
    position.scatter_(1, order, torch.arange(n).expand(n, n).contiguous())
    take = torch.clamp(cand.sum(1), max=min(int(k), n))
    return cand & (position < take[:, None])


def kept_of(A, d, mode):
    if mode == "directed":
        return d
    if mode == "union":
        return d | (d.t() & (A > 0))
    assert mode == "mutual", mode
    return d & d.t()


def host_kept(A, k, mode):
    return kept_of(A, host_picks(A, k), mode)


def host_knn(A, k, mode):
    """``B`` of one subject: the bits of ``A`` where kept, +0.0 elsewhere."""
    return torch.where(host_kept(A, k, mode), A, torch.zeros_like(A))


def host_knn_cohort(mats, k, mode):
    return torch.stack([host_knn(A, k, mode) for A in mats]) if mats.shape[0] else torch.zeros_like(mats)


def brute_picks(A, k):
    """bool [n, n], without a sort: ``j`` is picked iff it is a candidate and fewer than ``k`` candidates precede it."""
    n = A.shape[0]
    cand, a = candidates(A).tolist(), A.tolist()      # (Python floats: fp32 values compare exactly as doubles)
    d = [[False] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            if cand[i][j]:
                before = sum(1 for h in range(n) if cand[i][h] and
                             (a[i][h] > a[i][j] or (a[i][h] == a[i][j] and h < j)))
                d[i][j] = before < k
    return torch.tensor(d, dtype=torch.bool).reshape(n, n)


def last_picks(A, k):
    """(v [n], c [n]): the value and the column of every row's last pick; (+inf, -1) for a row without one."""
    n = A.shape[0]
    cand, a = candidates(A).tolist(), A.tolist()
    v, c = torch.full((n,), INF), torch.full((n,), -1, dtype=torch.long)
    for i in range(n):
        cols = [j for j in range(n) if cand[i][j]]
        cols.sort(key=lambda j: (-a[i][j], j))
        cols = cols[:min(int(k), len(cols))]
        if cols:
            v[i], c[i] = A[i, cols[-1]], cols[-1]
    return v, c


def picks_from_last(A, v, c):
    """``d`` from (v, c): ``A_ij > 0 and (A_ij > v_i or (A_ij == v_i and j <= c_i))``, off the diagonal."""
    n = A.shape[0]
    cols = torch.arange(n)[None, :]
    return candidates(A) & ((A > v[:, None]) | ((A == v[:, None]) & (cols <= c[:, None])))


@functools.lru_cache(maxsize=None)
def cohort(n):
    """[10, n, n] (host, shared between tests: do not modify)."""
    return torch.cat([D.recipe(n), D.worst_cases(n)]).contiguous()


def bits(t):
    return t.contiguous().view(torch.int32)
