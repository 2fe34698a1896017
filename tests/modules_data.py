"""The host statement of the module measures of ``connectome_gnn_amd.ingest`` (``MODULE_MEASURES``, ``module_profile``)
in fp64, built on tests/measures_data.py, and the seeded cohorts and partitions that its tests share.

Statement, per subject with matrix ``A`` ``[n, n]`` fp32, threshold ``t`` and partition ``c`` ``[n]`` with ``c_j`` in
``0 .. M - 1``: ``e_ij``, ``a_ij`` and ``b_ij`` are ``measures_data``'s (the edge test compares fp32 values, nothing is
symmetrised, rows are what is summed); ``k_i(m) = sum_{j: c_j = m} b_ij``, ``s_i(m) = sum_{j: c_j = m} a_ij``,
``k_i = sum_m k_i(m)``, ``s_i = sum_m s_i(m)`` (ascending ``m``), ``kappa_i = k_i(c_i)``, ``sigma_i = s_i(c_i)``.

* ``participation``: ``1 - sum_m (k_i(m) / k_i)^2``; 0 if ``k_i == 0``
* ``weighted_participation``: ``1 - sum_m (s_i(m) / s_i)^2``; 0 if ``s_i == 0``
* ``module_zscore``: ``(kappa_i - mean) / std`` over the nodes of module ``c_i``, ``std`` the population standard
  deviation; 0 if all ``kappa`` of that module compare equal (NOT ``std == 0``: the mean of three bit-equal doubles need
  not be that double)
* ``weighted_module_zscore``: the same on ``sigma_i``
* ``diversity``: ``-sum_m p ln p / ln M`` over the ``m`` with ``p = s_i(m) / s_i`` not 0 (a NaN ``p`` propagates); 0 if
  ``s_i == 0`` or ``M == 1``

Everything after the edge test is fp64.  The profile is ``s_i(m)`` (``k_i(m)`` if ``binary``), divided by the row total
if ``normalize``, with an exact zero row where that total is 0.

Cohorts: ``cohort(n)`` is ``ingest_data.recipe(n)`` with every positive entry clamped into ``[2^-10, 1]`` (a ``+inf``
becomes 1; a NaN, a zero or a negative entry is never kept and stays).  An fp32 value in that range is a multiple of
``2^-33``, and a row's sum is below ``2^10``: 43 bits, so fp64 sums of a row are exact in ANY order, and the device's and
the host's "all compare equal" tests see the same doubles.
"""
import functools
import math

import numpy as np
import torch

from tests import ingest_data as I
from tests import measures_data as MD

MODULE_MEASURES = ("participation", "weighted_participation", "module_zscore", "weighted_module_zscore", "diversity")
LOW, HIGH = 2.0 ** -10, 1.0


# ---- the statement ----
def module_sums(A, t, c):
    """(k_i(m) int64 [n, M], s_i(m) fp64 [n, M]) of one subject; ``c`` is an integer array [n]."""
    a, b, _ = MD.value_maps(A, t)
    c = np.asarray(c)
    M = int(c.max()) + 1
    km = np.stack([b[:, c == m].sum(1) for m in range(M)], 1)
    sm = np.stack([a[:, c == m].sum(1) for m in range(M)], 1)
    return km, sm


def _ascending_sum(cols):
    total = np.zeros(cols.shape[0], dtype=np.float64)
    for m in range(cols.shape[1]):
        total = total + cols[:, m]
    return total


def _participation(vm, total):
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = vm / total[:, None]
        return np.where(total == 0, 0.0, 1.0 - _ascending_sum(ratio * ratio))


def _diversity(sm, s):
    M = sm.shape[1]
    if M == 1:
        return np.zeros(sm.shape[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        p = sm / s[:, None]
        h = _ascending_sum(np.where(p == 0, 0.0, p * np.log(p)))
        return np.where(s == 0, 0.0, -h / math.log(M))


def module_stats(v, c, m):
    """(members, all compare equal, mean, population std) of the values ``v`` on module ``m``."""
    idx = np.nonzero(np.asarray(c) == m)[0]
    w = v[idx]
    equal = bool((w == w[0]).all())
    with np.errstate(invalid="ignore", over="ignore"):
        mean = w.sum() / len(w)
        std = float(np.sqrt(((w - mean) ** 2).sum() / len(w)))
    return idx, equal, mean, std


def _zscore(v, c):
    z = np.zeros(len(v), dtype=np.float64)
    for m in range(int(np.asarray(c).max()) + 1):
        idx, equal, mean, std = module_stats(v, c, m)
        if not equal:
            with np.errstate(invalid="ignore", divide="ignore"):
                z[idx] = (v[idx] - mean) / std
    return z


def host_module_measures(A, t, c, measures=MODULE_MEASURES):
    """fp64 ``[n, len(measures)]`` of one subject at threshold ``t`` for the partition ``c``."""
    c = np.asarray(c)
    km, sm = module_sums(A, t, c)
    k = km.sum(1).astype(np.float64)
    s = _ascending_sum(sm)
    rows = np.arange(len(c))
    kappa, sigma = km[rows, c].astype(np.float64), sm[rows, c]
    cols = {
        "participation": lambda: _participation(km.astype(np.float64), k),
        "weighted_participation": lambda: _participation(sm, s),
        "module_zscore": lambda: _zscore(kappa, c),
        "weighted_module_zscore": lambda: _zscore(sigma, c),
        "diversity": lambda: _diversity(sm, s),
    }
    return torch.from_numpy(np.stack([cols[m]() for m in measures], 1))


def host_profile(A, t, c, binary=False, normalize=False):
    """fp64 ``[n, M]``: the network profile of one subject."""
    km, sm = module_sums(A, t, c)
    v = km.astype(np.float64) if binary else sm
    if normalize:
        total = v.sum(1) if binary else _ascending_sum(v)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = np.where(total[:, None] == 0, 0.0, v / total[:, None])
    return torch.from_numpy(v)


def assert_conditioned(A, t, c):
    """The condition on the INPUTS under which the z-scores are checked to one rounding: every module's kappa and sigma
    either all compare equal or have a population std of at least 1e-3 of their largest magnitude.  The deviations are
    then formed from a mean that carries ``n 2^-53 max`` of error at the most, which moves a z-score by less than
    ``n 2^-53 / 1e-3 < 2^-33`` of itself at ``n <= 1024``.  Checked by the statement alone."""
    c = np.asarray(c)
    km, sm = module_sums(A, t, c)
    rows = np.arange(len(c))
    for name, v in (("kappa", km[rows, c].astype(np.float64)), ("sigma", sm[rows, c])):
        for m in range(int(c.max()) + 1):
            idx, equal, _, std = module_stats(v, c, m)
            assert equal or std >= 1e-3 * np.abs(v[idx]).max(), (name, m, std, np.abs(v[idx]).max())


def cohort_statement(mats, thr, c, measures=MODULE_MEASURES):
    """fp64 ``[S, n, F]`` for thresholds ``thr`` (a sequence of floats), after ``assert_conditioned`` on every subject."""
    out = []
    for A, t in zip(mats, thr):
        assert_conditioned(A, float(t), c)
        out.append(host_module_measures(A, float(t), c, measures))
    return torch.stack(out)


def cohort_profile(mats, thr, c, binary=False, normalize=False):
    return torch.stack([host_profile(A, float(t), c, binary, normalize) for A, t in zip(mats, thr)])


# ---- the inputs ----
def clamp_weights(mats):
    """Every positive entry into [2^-10, 1]; everything else as it is (module docstring)."""
    return torch.where(mats > 0, mats.clamp(LOW, HIGH), mats).contiguous()


@functools.lru_cache(maxsize=None)
def cohort(n, seed=0):
    """[6, n, n] fp32 (host, shared between tests: do not modify)."""
    out = clamp_weights(I.recipe(n, seed))
    kept = out[out > 0]
    assert bool(((kept >= LOW) & (kept <= HIGH)).all())
    return out


@functools.lru_cache(maxsize=None)
def _partition(n, M, seed, kind):
    assert 1 <= M <= n
    g = torch.Generator().manual_seed(1000 * seed + 17 * n + M)
    if kind == "blocks":                      # contiguous networks of uneven sizes, as an atlas lists them
        cuts = torch.randperm(n - 1, generator=g)[:M - 1].sort().values + 1
        c = torch.bucketize(torch.arange(n), cuts, right=True)
    else:                                     # scattered labels, every one used
        c = torch.randint(0, M, (n,), generator=g)
        c[torch.randperm(n, generator=g)[:M]] = torch.arange(M)
        if kind == "singleton" and M >= 2:    # module M - 1 keeps one node; the others of it move to module 0
            members = torch.nonzero(c == M - 1).flatten()
            c[members[1:]] = 0
    c = c.numpy().astype(np.int64)
    assert sorted(set(c.tolist())) == list(range(M)), "every label is used"
    c.setflags(write=False)
    return c


def partition(n, M, seed=0, kind="scattered"):
    """int64 numpy [n] with every label of 0 .. M - 1 used (shared: read-only).  ``kind``: "scattered", "singleton"
    (module M - 1 has exactly one node) or "blocks" (contiguous runs of uneven lengths)."""
    return _partition(n, M, seed, kind)


SIZES = (1, 2, 3, 5, 63, 64, 65, 84, 129, 257, 360)
THRESHOLDS = ({"keep": 0.1}, {"keep": 0.5}, {"min_weight": 0.0})
# (n, M) -> the partition's seed where seed 0 does not meet ``assert_conditioned`` on ``cohort(n)`` at every one of
# THRESHOLDS (two nodes of a small module with nearly the same sigma): the first seed that does, found on the host
SEEDS = {(84, 17): 1}


def module_counts(n):
    return sorted({M for M in (1, 2, 7, 17, min(n, 64)) if M <= n})


def kind_of(n, M):
    """A singleton module at M = 7, contiguous runs at M = 17, scattered labels elsewhere."""
    return "singleton" if M == 7 and n > 7 else "blocks" if M == 17 and n > 17 else "scattered"


def case_partition(n, M):
    return partition(n, M, SEEDS.get((n, M), 0), kind_of(n, M))


def host_thresholds(mats, kw):
    """The thresholds of one of THRESHOLDS, as floats."""
    if "min_weight" in kw:
        return [float(kw["min_weight"])] * len(mats)
    n = mats.shape[1]
    return [I.host_threshold(A, I.rank_of(n, kw["keep"])) for A in mats]


def has_singleton(c):
    return bool((np.bincount(c) == 1).any())


def straddles(c, boundary=64):
    """Some module has nodes on both sides of column ``boundary``."""
    c = np.asarray(c)
    return len(c) > boundary and bool(set(c[:boundary].tolist()) & set(c[boundary:].tolist()))
