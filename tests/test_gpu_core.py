"""The core decomposition of connectome_gnn_amd.ingest on the device (csrc/core.hip) against the fp64 host statement of
tests/core_data.py (the peeling loop in numpy), on ``core_data.cohort``.

What is asserted, derived and not taken from what the kernel gives:

* ``levels`` (``k_i``, ``r_i``, ``rho_i``) are integers and must equal the statement's; ``coreness`` and ``onion_layer``
  are one correctly rounded fp32 quotient of two integers below ``2^24`` and must equal ``numpy``'s fp32 quotient bit for
  bit.
* ``s_coreness`` on ``core_data.cohort``: every positive entry lies in ``[2^-10, 1]``, so it is a multiple of ``2^-33``
  and a sum of up to 1023 of them is below ``2^10``: 43 bits, exact in fp64 in any order.  The kernel and the statement
  then form the same doubles ``s_u(alive)`` in every round, make the same comparisons, and divide the same two doubles:
  the result must equal the statement's rounding bit for bit, and ``rho_i`` with it.
* ``s_coreness`` on unclamped weights: within ``2^-24 |v| + 2^-40`` of the statement, for ``n <= 1024``.  Every
  ``s_u(alive)`` is summed anew in a fixed order that depends on the subject's entries alone (a removed neighbour is left
  out of an otherwise unchanged order, never subtracted from a running sum), so the rounded function ``s~`` is still
  monotone in the alive set and the peeling computes exactly ITS generalised core ``max_H min_{u in H} s~_u(H)``.  That
  max-min form is 1-Lipschitz in the sup norm of ``p``; a sum of at most ``n - 1`` non-negative terms carries at most
  ``n 2^-53`` of itself, so ``sigma`` is within ``n 2^-53 max s`` of the exact value.  The statement's own sums (numpy's,
  pairwise) carry as much at the most.  The normaliser ``max s + 1e-8`` has the same relative error and the quotient one
  more rounding: together below ``(3 n + 2) 2^-53 <= 2^-41`` of a value that is at most 1 at ``n = 1024``, inside the
  ``2^-40`` term.  Then one rounding to fp32: half an ulp, at most ``2^-24 |v|``.  ``rho_i`` is not asserted there: two
  rows whose exact sums tie may leave a round apart.

The measured maxima are printed, in units of the bound.

Which staging path a subject takes for ``s_coreness`` follows from byte counts alone (the C call reports none).  Behind
the bitset (``8 n ceil(n / 64)`` bytes), the two masks (``2 x 128``), the reductions' slots (``128 + 64``), the row
offsets (``4 (n + 1)``) and a byte per node (``n`` rounded up to 4) a workgroup has ``space = min(6 n (n - 1) + 4,
160 KiB - that)`` bytes for the ``E`` kept entries of a subject: 2 bytes per column (rounded up to 4 in all), 4 per
weight.  They fit: the peeling walks LDS; else it reads the kept entries from the matrix rows.  Up to ``n = 129``
everything fits whatever is kept.  At ``n = 360`` ``space`` is 144308 bytes: ``keep=0.1`` keeps at most 12924 entries
(77544 bytes: LDS), ``keep=0.5`` 64620 (387720 bytes: the rows).
``_staging`` restates this and ``test_both_staging_paths_are_taken`` asserts it on the kept counts of the parity cases.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import cohort_kit as K
from tests import core_data as CD
from tests import ingest_data as I
from tests import modules_data as D
from tests import pagerank_data as PD
from tests.cohort_kit import DEV, NAN_BITS, bits as _bits, thresholds as _thresholds

pytestmark = pytest.mark.gpu
NAMES = CD.CORE_MEASURES
IDS, COLS, LDX = [0, 1, 2], [3, 1, 0], 5          # the raw calls write into a wider x; columns 2 and 4 stay
# every subset and order of the three names
REQUESTS = [list(p) for r in (1, 2, 3) for p in itertools.permutations(range(3), r)]


def _raw(dev, thr, ids=IDS, cols=COLS, ldx=LDX, want_levels=True):
    """One cgnn_ingest_cores call into a NaN-filled x: (x [S, n, ldx], levels [S, n, 3])."""
    S, n = int(dev.shape[0]), int(dev.shape[1])
    lv = torch.full((S, n, 3), -7, dtype=torch.int32, device=DEV) if want_levels else None
    x, _ = K.raw("cgnn_ingest_cores", dev, thr, ids, cols, ldx, tail=_lib.buf(lv))
    return x, lv


def _staging(n, E):
    """Which staging path a subject of ``E`` kept entries takes for s_coreness (module docstring)."""
    fixed = 8 * n * ((n + 63) // 64) + 2 * 128 + 128 + 64 + 4 * (n + 1) + (n + 3) // 4 * 4
    space = min(6 * n * (n - 1) + 4, 160 * 1024 - fixed)
    return "lds" if (2 * E + 3) // 4 * 4 + 4 * E <= space else "rows"


def _expect_levels(want, ids):
    out = want.clone()
    if 0 not in ids and 1 not in ids:
        out[:, :, :2] = -1
    if 2 not in ids:
        out[:, :, 2] = -1
    return out


def _check_cohort(n, dev, kw):
    """The three names of one (size, threshold choice) through the C ABI into a NaN-filled wider x and through the Python
    calls, every request against the full call, the levels."""
    what = f"n={n} {kw}"
    mats = CD.cohort(n)
    thr, _ = _thresholds(dev, mats, kw)
    want, want_lv = CD.cohort_statement(n, kw)
    x, lv = _raw(dev, thr)
    x, lv = x.cpu(), lv.cpu()
    assert bool((_bits(x[:, :, [2, 4]]) == NAN_BITS).all()), (what, "the columns that were not asked for keep their bits")
    got = x[:, :, COLS]
    assert torch.equal(lv, want_lv), (what, "k, r and rho are the host's integers")
    for col, name in enumerate(NAMES):
        assert torch.equal(_bits(got[:, :, col]), _bits(want[:, :, col])), (what, name)
    # the Python calls
    api = ingest.core_measures(dev, **kw)
    assert api.dtype == torch.float32 and api.is_contiguous() and tuple(api.shape) == (len(mats), n, 3)
    assert torch.equal(_bits(api.cpu()), _bits(got)), what
    levels = ingest.core_levels(dev, **kw)
    assert levels.dtype == torch.int32 and tuple(levels.shape) == (len(mats), n, 3)
    assert torch.equal(levels.cpu(), lv), (what, "core_levels is the raw call's levels")
    # every subset and order of the names: the bits of the full call; a pass that did not run leaves -1
    for ids in REQUESTS:
        cols = [4 - i for i in range(len(ids))]
        y, lv_y = _raw(dev, thr, ids, cols, 6)
        y = y.cpu()
        assert torch.equal(_bits(y[:, :, cols]), _bits(got[:, :, ids])), (what, ids)
        rest = [c for c in range(6) if c not in cols]
        assert bool((_bits(y[:, :, rest]) == NAN_BITS).all()), (what, ids)
        assert torch.equal(lv_y.cpu(), _expect_levels(want_lv, ids)), (what, ids)
        part = ingest.core_measures(dev, measures=tuple(NAMES[i] for i in ids), **kw)
        assert torch.equal(_bits(part.cpu()), _bits(got[:, :, ids])), (what, ids)
    no_levels, _ = _raw(dev, thr, want_levels=False)
    assert torch.equal(_bits(no_levels.cpu()), _bits(x)), (what, "levels may be NULL")
    rounds = lv[:, :, 1:].amax(1)
    print(f"{what}: rounds binary {rounds[:, 0].tolist()} weighted {rounds[:, 1].tolist()}")


# ---- 1: parity at every size and threshold choice ----
@pytest.mark.parametrize("n", CD.SIZES)
def test_parity_with_the_fp64_statement(n):
    dev = CD.cohort(n).to(DEV)
    for kw in CD.THRESHOLDS:
        _check_cohort(n, dev, kw)


def test_both_staging_paths_are_taken():
    """By byte counts (module docstring): the cases of the parity test reach both paths, and sizes up to 129 only LDS."""
    taken = {}
    for n in (129, 257, 360):
        mats = CD.cohort(n)
        for kw in CD.THRESHOLDS:
            thr = CD.host_thresholds(mats, kw)
            taken[n, tuple(kw.values())] = [_staging(n, CD.kept_entries(A, t)) for A, t in zip(mats, thr)]
    assert set(taken[129, (0.1,)] + taken[129, (0.5,)] + taken[129, (0.0,)]) == {"lds"}
    assert _staging(129, 129 * 128) == "lds"
    dense = CD.ASYMMETRIC
    assert set(taken[360, (0.1,)]) == {"lds"}, "360 ROIs at 10 % fit beside the bitset"
    assert taken[360, (0.5,)][dense] == "rows" and taken[360, (0.0,)][dense] == "rows"
    assert taken[257, (0.1,)][dense] == "lds" and taken[257, (0.5,)][dense] == "rows"
    assert _staging(360, 24051) == "lds" and _staging(360, 24052) == "rows"


# ---- 2: more than 512 nodes: two rows a thread, and the bitset filling LDS ----
@pytest.mark.parametrize("n", [600, 1024])
def test_the_largest_sizes(n):
    mats = D.cohort(n)[[3, 5]].contiguous()                 # asymmetric and symmetric uniform weights
    dev = mats.to(DEV)
    kw = {"keep": 0.05}
    thr, thr_h = _thresholds(dev, mats, kw)
    pairs = [CD.host_cores(A, t) for A, t in zip(mats, thr_h)]
    want, want_lv = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    x, lv = _raw(dev, thr)
    got, lv = x.cpu()[:, :, COLS], lv.cpu()
    paths = [_staging(n, CD.kept_entries(A, t)) for A, t in zip(mats, thr_h)]
    print(f"n={n}: rounds {lv[:, :, 1:].amax(1).tolist()}, staging {paths}")
    assert set(paths) == ({"lds"} if n == 600 else {"rows"})
    assert torch.equal(lv, want_lv)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(ingest.core_measures(dev, **kw).cpu()), _bits(got))


def test_more_than_1024_nodes_are_refused():
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.core_measures(torch.zeros(1, 1025, 1025, device=DEV), keep=0.1)
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.core_levels(torch.zeros(1, 1025, 1025, device=DEV), keep=0.1)


# ---- 3: unclamped weights, and a kept +inf ----
def test_unclamped_weights_stay_within_the_bound_and_a_kept_infinity_is_nan():
    n, s = 84, 5
    raw = I.recipe(n)                                       # unclamped: subject 5 has +inf at (0, 3) and (3, 0)
    assert float(raw[s, 0, 3]) == float("inf") and float(raw[4, n // 2, n // 2]) == float("inf")
    dev = raw.to(DEV)
    got = ingest.core_measures(dev, min_weight=0.0).cpu()
    lv = ingest.core_levels(dev, min_weight=0.0).cpu()
    ref = ingest.core_measures(D.cohort(n).to(DEV), min_weight=0.0).cpu()
    assert bool(torch.isnan(got[s, :, 2]).all()), "the weighted column of the subject"
    assert int(torch.isnan(got).sum()) == n, "and nothing else: the +inf on a diagonal is never kept"
    assert torch.equal(_bits(got[:, :, :2]), _bits(ref[:, :, :2])), "the binary columns do not see weights"
    assert bool((lv[s, :, 2] == -1).all()) and bool((lv[:, :, :2] >= 0).all())
    worst = 0.0
    for u in range(6):
        want, want_lv = CD.host_cores(raw[u], 0.0)
        assert torch.equal(lv[u, :, :2], want_lv[:, :2]), u
        assert torch.equal(_bits(got[u, :, :2]), _bits(want[:, :2])), u
        if u == s:
            continue
        v = CD.host_s_coreness(raw[u], 0.0)
        assert bool(torch.isfinite(got[u, :, 2]).all()) and bool((lv[u, :, 2] >= 1).all())
        ratio = float(((got[u, :, 2].double() - v).abs() / (2.0 ** -24 * v.abs() + 2.0 ** -40)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (u, ratio)
    print(f"unclamped n={n}: largest error {worst:.3f} of 2^-24 |v| + 2^-40")


# ---- 4: determinism ----
def test_a_grid_of_three_gives_the_bits_of_the_default_grid_and_of_a_second_run():
    """24 subjects at n = 84: the 8 of ``pagerank_data.cohort`` and two more seeds of them.  A workgroup takes at most 4
    per unit of the grid: 12 workgroups at the most at a grid of 3, hence at least 2 subjects each."""
    n = 84
    mats = torch.cat([PD.cohort(n, seed) for seed in range(3)]).contiguous()
    assert mats.shape[0] == 24
    dev = mats.to(DEV)

    def run():
        thr = ingest.select_thresholds(dev, keep=0.1)
        x, lv = _raw(dev, thr)
        return x, lv, ingest.core_measures(dev, keep=0.1)
    few, full = K.check_grid_of_three(run)
    alone = ingest.core_measures(PD.cohort(n).to(DEV), keep=0.1)
    assert torch.equal(_bits(full[2][:8]), _bits(alone)), "a subject's result does not depend on its cohort"
    tail = mats[-8:]
    want = torch.stack([CD.host_cores(A, t)[0] for A, t in zip(tail, CD.host_thresholds(tail, {"keep": 0.1}))])
    assert torch.equal(_bits(few[2][-8:].cpu()), _bits(want))


# ---- 5: composition ----
def test_knn_the_backbone_and_the_group_are_the_call_on_the_sparsified_matrices():
    n = 84
    dev = CD.cohort(n).to(DEV)
    for call in (ingest.core_measures, ingest.core_levels):
        K.check_knn(call, dev)
        K.check_backbone(call, dev)
        K.check_group(call, dev)
    tree = ingest.core_levels(dev, backbone="mst").cpu()
    assert int(tree[CD.STAR, :, 0].max()) == 1, "a tree has no 2-core"
    assert bool(torch.isfinite(ingest.core_measures(dev, backbone="mst", keep=0.1)).all())


def test_the_three_columns_train_on_the_fused_path():
    mats, feats = K.check_trains_on_the_fused_path(lambda m: ingest.core_measures(m, keep=0.1), 3)
    assert bool((feats >= 0).all()) and bool((feats <= 1).all())
    ref = ingest.node_measures(mats, keep=0.1, measures=("degree",))
    assert bool((feats[:, :, 0] <= ref[:, :, 0]).all()), "coreness <= degree: the same correctly rounded quotient"


# ---- 6: an empty cohort ----
def test_no_subjects_give_an_empty_tensor_without_a_launch():
    n = 20
    dev = CD.cohort(n).to(DEV)[:0]
    K.check_no_subjects(lambda m: ingest.core_measures(m, keep=0.1), dev, 3)
    K.check_no_subjects(lambda m: ingest.core_levels(m, keep=0.1), dev, 3, torch.int32)
    lib = _lib.load()
    assert lib.cgnn_ingest_cores(None, 0, n, None, (ctypes.c_int32 * 1)(2), 1, (ctypes.c_int32 * 1)(0), 1, None, 0,
                                 None, 0, None, 0, _lib.stream_ptr()) == _lib.CGNN_OK
