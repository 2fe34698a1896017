"""The host statement of ``connectome_gnn_amd.ingest.random_walk_encodings`` in fp64, the fp32 model of the arithmetic
that include/cgnn_rw.h fixes, the bound between the two, and the seeded cohorts that the tests share.

Statement, per subject with matrix ``A`` ``[n, n]`` fp32 and threshold ``t``: ``e_ij`` is ``measures_data.kept_mask``'s
(the edge test compares fp32 values, nothing is symmetrised, rows are what is summed); ``a_ij = A_ij`` on edges (``1`` with
``binary``), ``s_i = sum_j a_ij``, ``P_ij = a_ij / s_i`` with an exact zero row where ``s_i == 0``, and the column of step
``k`` is ``diag(P^k)``, the powers formed explicitly in fp64.  A kept weight that is not finite (weights only) makes the
columns for ``k >= 2`` NaN; step 1 is 0 whatever the subject holds.

Model (``model``): ``s_i`` an fp64 sum in ascending column order rounded to fp32; ``P_ij`` one fp32 division;
``M2 = P P``, ``M3 = P M2``, ``M4 = M2 M2`` as chains of fp32 fused multiply-adds with ``k`` ascending (the product of two
fp32 numbers is exact in fp64; the sum is formed there and rounded to fp32, which is the fused operation up to a double
rounding); ``r_k(i) = sum_j (M_a)_ij (M_b)_ji`` with ``SPLIT[k] = (a, b)`` in fp64 in ascending ``j``, rounded to fp32.

Bound (``bound``), ``u = 2^-24``, every term non-negative so every error is relative: ``s_i`` carries ``u`` and the
division ``u``, so ``P`` is within ``2 u``; to first order an entry of a product carries its factors' errors plus
``n u`` for its sum, so ``M2`` is within ``(n + 4) u``, ``M3`` within ``(2 n + 6) u`` and ``M4`` within ``(3 n + 8) u``:
``M_m`` within ``((m - 1) n + 2 m) u``.  ``r_k`` carries the errors of ``M_a`` and ``M_b`` with ``a + b = k`` and one
rounding: ``((k - 2) n + 2 k + 1) u``.  1.01 absorbs the second-order terms and ``2^-40`` what lies below the fp32 normal
range.

Cohort: ``cohort(n)`` is ``modules_data.cohort(n)``, the six recipe subjects with every positive entry in ``[2^-10, 1]``
(two symmetric, an all-zero one, an asymmetric one, one with NaN entries, one more symmetric); ``shapes(n)`` are the
closed-form graphs.
"""
import functools

import numpy as np
import torch

from tests import measures_data as MD
from tests import modules_data as D

MAX_STEPS = 8
STEPS = tuple(range(1, MAX_STEPS + 1))
SPLIT = {2: (1, 1), 3: (1, 2), 4: (2, 2), 5: (2, 3), 6: (3, 3), 7: (3, 4), 8: (4, 4)}
U = 2.0 ** -24
ALL_ZERO, ASYMMETRIC, WITH_NAN = 2, 3, 4      # subjects of ``cohort``
SYMMETRIC = (0, 1, 4, 5)
MODEL_SIZES = (2, 5, 17, 96, 97, 193, 360, 1024)
GPU_SIZES = (1, 2, 5, 16, 17, 95, 96, 97, 193, 360)
KEEPS = (0.10, 0.30)


def bound(k, n, r):
    """The largest ``|device - statement|`` for step ``k >= 2`` at ``n`` nodes where the statement is ``r`` (module
    docstring)."""
    return 1.01 * ((k - 2) * n + 2 * k + 1) * U * np.abs(r) + 2.0 ** -40


# ---- the statement ----
def walk_weights(A, t, binary=False):
    """(a fp64 [n, n], finite): the kept weights, or indicators, and whether every one of them is a finite number."""
    mask = MD.kept_mask(A, t)
    if binary:
        return mask.astype(np.float64), True
    a = np.where(mask, A.numpy().astype(np.float64), 0.0)
    return a, bool(np.isfinite(a).all())


def transition(a):
    """``P`` fp64: the rows of ``a`` over their sums, an exact zero row where the sum is 0."""
    s = a.sum(1)
    return np.divide(a, s[:, None], out=np.zeros_like(a), where=s[:, None] > 0)


def statement(A, t, steps=STEPS, binary=False):
    """fp64 ``[n, len(steps)]``: ``diag(P^k)`` by explicit powers."""
    n = A.shape[0]
    a, finite = walk_weights(A, t, binary)
    cols = {1: np.zeros(n)}
    if not finite:
        cols.update({k: np.full(n, np.nan) for k in STEPS[1:]})
    else:
        P = transition(a)
        Pk = P
        for k in range(2, max(steps) + 1):
            Pk = Pk @ P
            cols[k] = np.diagonal(Pk).copy()
    return np.stack([cols[k] for k in steps], 1)


def host_encodings(A, t, steps=STEPS, binary=False):
    """fp32 torch ``[n, len(steps)]``: the statement, each value rounded once."""
    return torch.from_numpy(statement(A, t, steps, binary).astype(np.float32))


def split_statement(P, k):
    """fp64 ``[n]``: ``sum_j (P^a)_ij (P^b)_ji`` with ``(a, b) = SPLIT[k]``."""
    a, b = SPLIT[k]
    return (np.linalg.matrix_power(P, a) * np.linalg.matrix_power(P, b).T).sum(1)


# ---- the fp32 model ----
def _ascending(terms):
    """fp64 ``[n]``: the rows of ``terms`` summed from 0.0 in ascending column order."""
    return np.cumsum(terms, axis=1)[:, -1] if terms.shape[1] else np.zeros(terms.shape[0])


def _fma_product(X, Y):
    """fp32 ``X Y`` as a chain of fused multiply-adds, ``k`` ascending."""
    acc = np.zeros((X.shape[0], Y.shape[1]), dtype=np.float32)
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    for k in range(X.shape[1]):
        acc = (X64[:, k, None] * Y64[None, k, :] + acc).astype(np.float32)
    return acc


def model(A, t, binary=False):
    """fp32 numpy ``[n, 8]``: the arithmetic of the header, on a subject whose kept weights are finite."""
    n = A.shape[0]
    a, finite = walk_weights(A, t, binary)
    assert finite
    s = _ascending(a).astype(np.float32)
    a32 = a.astype(np.float32)                 # exact: fp32 weights, or 1
    with np.errstate(invalid="ignore", divide="ignore"):
        P = np.where(s[:, None] > 0, a32 / s[:, None], np.float32(0)).astype(np.float32)
    M = {1: P}
    M[2] = _fma_product(P, P)
    M[3] = _fma_product(P, M[2])
    M[4] = _fma_product(M[2], M[2])
    out = np.zeros((n, MAX_STEPS), dtype=np.float32)
    for k, (p, q) in SPLIT.items():
        out[:, k - 1] = _ascending(M[p].astype(np.float64) * M[q].T.astype(np.float64)).astype(np.float32)
    return out


def share_of_bound(got, want, n, steps=STEPS):
    """The largest ``|got - want| / bound`` over the columns of steps ``>= 2``; ``got`` and ``want`` are ``[.., n, len(steps)]``."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    worst = 0.0
    for c, k in enumerate(steps):
        if k >= 2:
            worst = max(worst, float((np.abs(got[..., c] - want[..., c]) / bound(k, n, want[..., c])).max()))
    return worst


# ---- the inputs ----
def cohort(n, seed=0):
    """[6, n, n] fp32 (host, shared between tests: do not modify)."""
    return D.cohort(n, seed)


def host_thresholds(mats, kw):
    return D.host_thresholds(mats, kw)


@functools.lru_cache(maxsize=None)
def cohort_statement(n, keep, binary):
    """fp64 numpy ``[6, n, 8]`` of ``cohort(n)`` at ``keep`` (shared between tests: do not modify)."""
    mats = cohort(n)
    thr = host_thresholds(mats, {"keep": keep})
    out = np.stack([statement(A, t, STEPS, binary) for A, t in zip(mats, thr)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def large(n):
    """[1, n, n] fp32: one asymmetric subject of uniform weights in ``[2^-10, 1]`` (shared: do not modify)."""
    g = torch.Generator().manual_seed(100 + n)
    return D.clamp_weights(torch.rand(1, n, n, generator=g))


def star(n):
    A = torch.zeros(n, n)
    A[0, 1:] = 0.5
    A[1:, 0] = 0.5
    return A


def complete(n, weight=0.25):
    A = torch.full((n, n), weight)
    A.fill_diagonal_(0.0)
    return A


def cycle(n, weight=0.5):
    A = torch.zeros(n, n)
    i = torch.arange(n)
    A[i, (i + 1) % n] = weight
    A[(i + 1) % n, i] = weight
    return A


def two_cliques(n):
    """Cliques on the first ``n // 2`` and on the other nodes, with different weights."""
    A = torch.zeros(n, n)
    h = n // 2
    A[:h, :h] = 0.75
    A[h:, h:] = 0.25
    A.fill_diagonal_(0.0)
    return A


def bipartite(n, seed=0):
    """Random weights in ``[2^-10, 1]`` between the even and the odd nodes only, asymmetric."""
    g = torch.Generator().manual_seed(seed)
    A = D.clamp_weights(torch.rand(n, n, generator=g))
    i = torch.arange(n)
    same = (i[:, None] % 2) == (i[None, :] % 2)
    return torch.where(same, torch.zeros(n, n), A).contiguous()


def expected_complete(n):
    """``r_k`` of any node of the complete graph on ``n >= 2`` nodes with equal weights: ``r_1 = 0``,
    ``r_{k + 1} = (1 - r_k) / (n - 1)`` (the walk returns from any other node with probability ``1 / (n - 1)``)."""
    r = [0.0]
    for _ in range(MAX_STEPS - 1):
        r.append((1.0 - r[-1]) / (n - 1))
    return np.array(r)
