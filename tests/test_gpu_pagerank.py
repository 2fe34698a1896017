"""PageRank centrality of connectome_gnn_amd.ingest on the device (csrc/pagerank.hip) against the fp64 host statement of
tests/pagerank_data.py (``numpy.linalg.solve`` on the Google matrix), on ``pagerank_data.cohort``.

The bound, derived and not taken from what the kernel gives: every value is within ``2^-24 |v| + 2^-36`` of the
statement, for ``d <= 0.9`` and ``n <= 1024``.

* The product ``T(x) = d G x + (1 - d) / n`` with a column-stochastic ``G`` contracts at rate ``d`` in L1; a step of the
  iteration is two products and contracts at ``d^2``.  It stops at the first step whose change is at most
  ``(1 - d) 2^-42``: then ``||x_k - x||_1 <= d^2 / (1 - d^2) * change < 2^-42``.  A subject that ran to the cap
  ``K_max = ceil(43 ln 2 / -ln d) + 2`` instead would be within ``2 d^(2 K_max) < 2^-42`` all the same, the start being at
  most 2 away; tests/test_pagerank_math.py shows why a step is two products and that no case of the cohort is capped.
* The fp64 chain: a row's sum of ``k`` products carries at most ``(k + 2) 2^-53`` of the sum of their magnitudes, the
  product ``x_j (1 / c_j)`` with the rounded reciprocal, the dangling mass and the affine step a few ``2^-53`` more, and
  ``c_j`` itself ``n 2^-53`` relative (a sum of up to ``n - 1`` positive terms).  The magnitudes of a step sum to 1, so a
  step adds at most ``(n + 8) 2^-53`` in L1 for its own sums and as much again for the ``c_j`` it divides by:
  ``(2 n + 8) 2^-53``, which the contraction accumulates to ``(2 n + 8) 2^-53 / (1 - d)``, below ``2^-38`` at
  ``n = 1024``, ``d = 0.9``.  (The issue states ``(n + 8) 2^-53 / (1 - d) < 2^-39``, which leaves the error of ``c_j``
  out; the constant proven here is twice that and the bound under test is unchanged, it has the room.)
* The statement's own solve is backward stable on a matrix of condition at most ``(1 + d) / (1 - d) <= 19``: some
  ``19 n 2^-53 < 2^-38``.
* Together below ``2^-37``: inside the ``2^-36`` term.  Then one rounding to fp32: half an ulp, which is ``2^-24 |v|``
  for a ``v`` just above a power of two.  That term is therefore tight: the measured maxima come close to 1.

The measured maxima are printed per size, in units of the bound.

Which staging path a case takes follows from byte counts alone (the C call reports none).  Beside the ``8 (5 n + 1056) +
4 (n + 1)`` bytes of vectors, scratch and row offsets a workgroup has ``space = min(6 n (n - 1) + 4, 160 KiB - that)``
bytes for a subject's ``E`` kept entries: 2 bytes per column, 4 per weight.  ``6 E`` fits: both names walk LDS.  Only
``2 E`` fits: ``pagerank`` walks LDS and ``weighted_pagerank`` reads the matrix rows.  Neither: both read the rows.  Up
to ``n = 129`` everything fits whatever is kept.  At ``n = 360`` ``space`` is 139548 bytes: ``keep=0.1`` keeps at most
12924 entries (77544 bytes: the first path), ``keep=0.5`` 64620 (129240 bytes of columns: the second), and
``min_weight=0.0`` up to 129240 on the dense subjects (258480 bytes of columns: the third).  ``_staging`` restates this
and ``test_the_three_staging_paths_are_all_taken`` asserts it on the kept counts of the cases of the parity test.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import cohort_kit as K
from tests import ingest_data as I
from tests import modules_data as D
from tests import pagerank_data as PD
from tests.cohort_kit import DEV, NAN_BITS, bits as _bits, thresholds as _thresholds

pytestmark = pytest.mark.gpu
NAMES = PD.CENTRALITY_MEASURES
IDS, COLS, LDX = [0, 1], [3, 1], 5                # the raw calls write into a wider x; columns 0, 2 and 4 stay
REQUESTS = [([0], [3]), ([1], [1]), ([1, 0], [1, 3]), ([0], [0]), ([1, 0], [4, 2])]


def _raw(dev, thr, d, ids=IDS, cols=COLS, ldx=LDX):
    """One cgnn_ingest_pagerank call into a NaN-filled x: (x [S, n, ldx], iterations [S])."""
    it = torch.full((int(dev.shape[0]),), -7, dtype=torch.int32, device=DEV)
    x, _ = K.raw("cgnn_ingest_pagerank", dev, thr, ids, cols, ldx, mid=(float(d),), tail=_lib.buf(it))
    return x, it


def _ratio(got, want):
    """The largest error of ``got`` (fp32, host) against ``want`` (fp64) in units of ``2^-24 |v| + 2^-36``."""
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(want).all())
    return float(((got.double() - want).abs() / (2.0 ** -24 * want.abs() + 2.0 ** -36)).max())


def _staging(n, E):
    """Which of the three staging paths a subject of ``E`` kept entries takes (module docstring)."""
    fixed = 8 * (5 * n + 1056) + 4 * (n + 1)
    space = min(6 * n * (n - 1) + 4, 160 * 1024 - fixed)
    if (2 * E + 3) // 4 * 4 + 4 * E <= space:
        return "all"
    return "columns" if 2 * E <= space else "rows"


def _check_cohort(n, dev, kw, d):
    """Both names of one (size, threshold choice, damping) through the C ABI into a NaN-filled wider x and through the
    Python call, every request against the full call, the exact values, the step counts.  Returns the largest error in
    units of the bound."""
    what = f"n={n} {kw} d={d}"
    mats = PD.cohort(n)
    thr, thr_h = _thresholds(dev, mats, kw)
    want = PD.cohort_statement(n, kw, d)
    x, it = _raw(dev, thr, d)
    x, it = x.cpu(), it.cpu()
    assert bool((_bits(x[:, :, [0, 2, 4]]) == NAN_BITS).all()), (what, "the columns that were not asked for keep their bits")
    got = x[:, :, COLS]
    worst = _ratio(got, want)
    assert worst <= 1.0, (what, worst)
    bound = 2.0 ** -24 * want.abs() + 2.0 ** -36
    assert bool((got.double() >= (1.0 - d) / n - bound).all()), (what, "the teleport term is a lower bound")
    assert bool(((got.double().sum(1) - 1.0).abs() <= n * 2.0 ** -24).all()), (what, "a subject sums to 1")
    uniform = torch.full((n,), np.float32(1.0 / n).item())
    for s in range(len(mats)):
        if PD.kept_entries(mats[s], thr_h[s]) == 0:
            for col in range(2):
                assert torch.equal(_bits(got[s, :, col]), _bits(uniform)), (what, s, "no kept entry: fp32(1 / n) exactly")
    assert PD.kept_entries(mats[PD.ALL_ZERO], thr_h[PD.ALL_ZERO]) == 0
    if n == 1:
        assert bool((got == 1.0).all())
    # the Python call, and every subset and order of the names
    api = ingest.centrality_measures(dev, damping=d, **kw)
    assert api.dtype == torch.float32 and api.is_contiguous() and tuple(api.shape) == (len(mats), n, 2)
    assert torch.equal(_bits(api.cpu()), _bits(got)), what
    for names in (NAMES[::-1], NAMES[:1], NAMES[1:]):
        part = ingest.centrality_measures(dev, damping=d, measures=names, **kw).cpu()
        assert torch.equal(_bits(part), _bits(got[:, :, [NAMES.index(m) for m in names]])), (what, names)
    for ids, cols in REQUESTS:
        ldx = max(cols) + 2
        y, it_y = _raw(dev, thr, d, ids, cols, ldx)
        y = y.cpu()
        assert torch.equal(_bits(y[:, :, cols]), _bits(got[:, :, ids])), (what, ids, cols)
        rest = [c for c in range(ldx) if c not in cols]
        assert bool((_bits(y[:, :, rest]) == NAN_BITS).all()), (what, ids, cols)
        if len(ids) == 2:
            assert torch.equal(it_y.cpu(), it), (what, "the step counts of both names in the other order")
    # the step counts: the slowest name's, at most the cap; the model's within one step on the symmetric subjects
    cap = PD.max_steps(d)
    assert ingest.pagerank_max_steps(d) == cap
    assert bool((it >= 1).all()) and bool((it <= cap).all()), (what, it.tolist(), cap)
    single = [_raw(dev, thr, d, [i], [0], 1)[1].cpu() for i in range(2)]
    assert torch.equal(torch.maximum(*single), it), (what, "the slowest of the names asked for")
    for s in PD.SYMMETRIC:
        for col, name in enumerate(NAMES):
            steps = min(PD.model(mats[s], thr_h[s], d, name)[1], cap)
            assert abs(int(single[col][s]) - steps) <= 1, (what, s, name, int(single[col][s]), steps)
    print(f"{what}: {worst:.3f} of the bound, steps {it.tolist()}")
    return worst


# ---- 1: parity at every size, threshold choice and damping ----
@pytest.mark.parametrize("n", PD.SIZES)
def test_parity_with_the_fp64_statement(n):
    dev = PD.cohort(n).to(DEV)
    worst = 0.0
    for kw, d in itertools.product(PD.THRESHOLDS, PD.DAMPINGS):
        worst = max(worst, _check_cohort(n, dev, kw, d))
    print(f"n={n}: largest error {worst:.3f} of 2^-24 |v| + 2^-36")


def test_the_three_staging_paths_are_all_taken():
    """By byte counts (module docstring): the cases of the parity test reach every path, and sizes up to 129 only the
    first."""
    taken = {}
    for n in (129, 257, 360):
        mats = PD.cohort(n)
        for kw in PD.THRESHOLDS:
            thr = PD.host_thresholds(mats, kw)
            taken[n, tuple(kw.values())] = [_staging(n, PD.kept_entries(A, t)) for A, t in zip(mats, thr)]
    assert set(taken[129, (0.1,)] + taken[129, (0.5,)] + taken[129, (0.0,)]) == {"all"}
    assert _staging(129, 129 * 128) == "all"
    dense = PD.ASYMMETRIC
    assert taken[360, (0.1,)][dense] == "all" and taken[360, (0.5,)][dense] == "columns"
    assert taken[360, (0.0,)][dense] == "rows"
    assert taken[257, (0.1,)][dense] == "all" and taken[257, (0.5,)][dense] == "columns"
    assert taken[257, (0.0,)][dense] == "columns"
    assert set(taken[360, (0.1,)]) == {"all"}, "360 ROIs at 10 % fit beside the vectors"


# ---- 2: more than 512 nodes: two columns per thread in the staging pass ----
@pytest.mark.parametrize("n", [600, 1024])
def test_the_largest_sizes(n):
    mats = D.cohort(n)[[3, 5]].contiguous()                 # asymmetric and symmetric uniform weights
    dev = mats.to(DEV)
    kw, d = {"keep": 0.05}, 0.85
    thr, thr_h = _thresholds(dev, mats, kw)
    want = torch.stack([PD.host_centrality(A, t, d) for A, t in zip(mats, thr_h)])
    x, it = _raw(dev, thr, d)
    got = x.cpu()[:, :, COLS]
    worst = _ratio(got, want)
    paths = [_staging(n, PD.kept_entries(A, t)) for A, t in zip(mats, thr_h)]
    print(f"n={n}: {worst:.3f} of the bound, steps {it.cpu().tolist()}, staging {paths}")
    assert worst <= 1.0, (n, worst)
    assert bool((it.cpu() <= PD.max_steps(d)).all())
    assert torch.equal(_bits(ingest.centrality_measures(dev, damping=d, **kw).cpu()), _bits(got))


def test_more_than_1024_nodes_are_refused():
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.centrality_measures(torch.zeros(1, 1025, 1025, device=DEV), keep=0.1)


# ---- 3: determinism ----
def test_a_grid_of_three_gives_the_bits_of_the_default_grid_and_of_a_second_run():
    """24 subjects at n = 84: the 8 of the cohort and two more seeds of them.  A workgroup takes at most 4 per unit of
    the grid: 12 workgroups at the most at a grid of 3, hence at least 2 subjects each."""
    n = 84
    mats = torch.cat([PD.cohort(n, seed) for seed in range(3)]).contiguous()
    assert mats.shape[0] == 24
    dev = mats.to(DEV)

    def run():
        thr = ingest.select_thresholds(dev, keep=0.1)
        x, it = _raw(dev, thr, 0.85)
        return x, it, ingest.centrality_measures(dev, keep=0.1)
    few, full = K.check_grid_of_three(run)
    alone = ingest.centrality_measures(PD.cohort(n).to(DEV), keep=0.1)
    assert torch.equal(_bits(full[2][:8]), _bits(alone)), "a subject's result does not depend on its cohort"
    tail = mats[-8:]
    want = torch.stack([PD.host_centrality(A, t, 0.85) for A, t in zip(tail, PD.host_thresholds(tail, {"keep": 0.1}))])
    assert _ratio(few[2][-8:].cpu(), want) <= 1.0


# ---- 4: a kept +inf ----
def test_a_kept_infinity_makes_the_weighted_column_nan_and_nothing_else():
    n, s = 84, 5
    raw = I.recipe(n)                                       # unclamped: subject 5 has +inf at (0, 3) and (3, 0)
    assert float(raw[s, 0, 3]) == float("inf") and float(raw[4, n // 2, n // 2]) == float("inf")
    got = ingest.centrality_measures(raw.to(DEV), min_weight=0.0).cpu()
    ref = ingest.centrality_measures(D.cohort(n).to(DEV), min_weight=0.0).cpu()
    assert bool(torch.isnan(got[s, :, 1]).all()), "the weighted column of the subject"
    assert int(torch.isnan(got).sum()) == n, "and nothing else: the +inf on a diagonal is never kept"
    assert torch.equal(_bits(got[:, :, 0]), _bits(ref[:, :, 0])), "the binary column does not see weights"
    others = [u for u in range(6) if u != s]
    want = torch.stack([PD.host_centrality(raw[u], 0.0, 0.85) for u in others])
    assert _ratio(got[others], want) <= 1.0
    thr = torch.zeros(6, device=DEV)
    both, only_b, only_w = (_raw(raw.to(DEV), thr, 0.85, ids, list(range(len(ids))), len(ids))[1].cpu()
                            for ids in ([0, 1], [0], [1]))
    assert int(only_w[s]) == 0 and int(both[s]) == int(only_b[s]) >= 1, "no step is taken on the NaN column"


# ---- 5: composition ----
def test_knn_and_the_backbone_are_the_call_on_the_sparsified_matrices():
    n = 84
    dev = PD.cohort(n).to(DEV)
    K.check_knn(ingest.centrality_measures, dev)
    got = K.check_backbone(ingest.centrality_measures, dev, damping=0.5)
    assert bool(torch.isfinite(got).all())


def test_the_two_columns_train_on_the_fused_path():
    mats, feats = K.check_trains_on_the_fused_path(lambda m: ingest.centrality_measures(m, keep=0.1), 2)
    assert bool(((feats.sum(1) - 1).abs() <= mats.shape[1] * 2.0 ** -24).all())


# ---- 6: an empty cohort ----
def test_no_subjects_give_an_empty_tensor_without_a_launch():
    n = 20
    K.check_no_subjects(lambda m: ingest.centrality_measures(m, keep=0.1), PD.cohort(n).to(DEV)[:0], 2)
    lib = _lib.load()
    assert lib.cgnn_ingest_pagerank(None, 0, n, None, (ctypes.c_int32 * 1)(1), 1, (ctypes.c_int32 * 1)(0), 1, 0.85,
                                    None, 0, None, 0, None, 0, _lib.stream_ptr()) == _lib.CGNN_OK
