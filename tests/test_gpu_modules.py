"""The module measures of connectome_gnn_amd.ingest on the device (csrc/modules.hip) against the fp64 host statement
of tests/modules_data.py, on ``modules_data.cohort`` (the recipe subjects of tests/ingest_data.py with every positive
weight in ``[2^-10, 1]``, so that fp64 sums of a row are exact in any order).

Bounds, none of them taken from what the kernel gives:

* ``participation`` and the binary profile, normalised or not, equal the host's fp32 rounding BIT FOR BIT.  The counts
  are exact integers.  A normalised entry is one correctly rounded fp64 quotient of two of them on either side.  The
  participation is a rational with denominator ``k^2 <= 2^20``: where it is not an fp32 value or tie itself (``k`` a
  power of two: every term is then exact) it lies at least ``2^-45`` away from the nearest one, and the fp64 evaluation
  is within ``M 2^-52`` of it in whatever order the ``M`` terms are added, so both sides round alike.
* Every other value is within ``2^-24 |v| + 2^-30`` of the statement: the sums are exact, the fp64 chain after them
  differs from the host's by a few ``2^-53`` (the order of at most 64 terms, ``ln``), and there is one rounding to fp32.
  The z-scores add ``n 2^-53 max / std``, which ``modules_data.assert_conditioned`` keeps below ``2^-33`` by a condition on
  the inputs.

The measured maxima are printed per size, in units of the bound.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import cohort_kit as K
from tests import ingest_data as I
from tests import measures_data as MD
from tests import modules_data as D
from tests import paths_data as P
from tests import timeseries_data as TS
from tests import wpaths_data as W
from tests.cohort_kit import DEV, NAN_BITS, bits as _bits, thresholds as _thresholds

pytestmark = pytest.mark.gpu
NAMES = D.MODULE_MEASURES
ALL17 = MD.MEASURES + P.PATH_MEASURES + W.WEIGHTED_PATH_MEASURES + NAMES
IDS, COLS, LDX = [0, 1, 2, 3, 4], [5, 0, 3, 6, 1], 7       # the raw calls write into a wider x; columns 2 and 4 stay
FORMS = list(itertools.product((False, True), (False, True)))           # (binary, normalize)


def _labels(c):
    return torch.from_numpy(np.asarray(c).astype(np.int32)).to(DEV)


def _raw(dev, thr, c_dev, M, ids=(), cols=(), ldx=1, profile_flags=None):
    """One cgnn_ingest_modules call into NaN-filled outputs: (x [S, n, ldx] or None, profile [S, n, M] or None)."""
    S, n = int(dev.shape[0]), int(dev.shape[1])
    prof = torch.full((S, n, M), float("nan"), device=DEV) if profile_flags is not None else None
    x, _ = K.raw("cgnn_ingest_modules", dev, thr, ids, cols, ldx, head=(c_dev, M),
                 tail=_lib.buf(prof) + (profile_flags or 0,))
    return x, prof


def _ratio(got, want):
    """The largest error of ``got`` (fp32, host) against ``want`` (fp64) in units of ``2^-24 |v| + 2^-30``."""
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(want).all())
    if got.numel() == 0:
        return 0.0
    return float(((got.double() - want).abs() / (2.0 ** -24 * want.abs() + 2.0 ** -30)).max())


def _check_cohort(mats, dev, c, M, kw, what):
    """All five measures and the four profile forms of one (cohort, partition, threshold choice), through the C ABI
    into NaN-filled buffers and through the Python calls.  Returns the largest error in units of the bound."""
    c_dev = _labels(c)
    thr, thr_h = _thresholds(dev, mats, kw)
    want = D.cohort_statement(mats, thr_h, c)                          # asserts the condition on the inputs
    x, _ = _raw(dev, thr, c_dev, M, IDS, COLS, LDX)
    x = x.cpu()
    assert bool((_bits(x[:, :, [2, 4]]) == NAN_BITS).all()), (what, "the columns that were not asked for keep their bits")
    got = x[:, :, COLS]
    assert torch.equal(_bits(got[:, :, 0]), _bits(want[:, :, 0].float())), (what, "participation, bit for bit")
    worst = _ratio(got[:, :, 1:], want[:, :, 1:])
    print(f"{what}: measures {worst:.3f} of the bound")
    assert worst <= 1.0, (what, worst)
    api = ingest.node_measures(dev, measures=NAMES, modules=c, **kw)
    assert api.dtype == torch.float32 and api.is_contiguous() and torch.equal(_bits(api.cpu()), _bits(got)), what
    for binary, normalize in FORMS:
        flags = (1 if binary else 0) | (2 if normalize else 0)
        prof = _raw(dev, thr, c_dev, M, profile_flags=flags)[1].cpu()
        p_want = D.cohort_profile(mats, thr_h, c, binary, normalize)
        assert tuple(prof.shape) == (len(mats), mats.shape[1], M)
        if binary:
            assert torch.equal(_bits(prof), _bits(p_want.float())), (what, "binary profile, bit for bit", normalize)
        else:
            r = _ratio(prof, p_want)
            worst = max(worst, r)
            assert r <= 1.0, (what, "profile", normalize, r)
            assert torch.equal(prof == 0, p_want == 0), (what, "exact zeros")
        api = ingest.module_profile(dev, c, binary=binary, normalize=normalize, **kw)
        assert torch.equal(_bits(api.cpu()), _bits(prof)), (what, binary, normalize)
    return worst


# ---- 1: parity at every size and module count ----
@pytest.mark.parametrize("n", D.SIZES)
def test_parity_with_the_fp64_statement(n):
    mats = D.cohort(n)
    dev = mats.to(DEV)
    worst = 0.0
    for M in D.module_counts(n):
        c = D.case_partition(n, M)
        if (n, M) == (65, 7):
            assert D.has_singleton(c) and D.straddles(c), "a singleton module, and one across the 64-column boundary"
        if (n, M) == (84, 17):
            assert D.straddles(c) and len(set(np.bincount(c).tolist())) > 1, "contiguous runs of uneven lengths"
        for kw in D.THRESHOLDS:
            worst = max(worst, _check_cohort(mats, dev, c, M, kw, f"n={n} M={M} {kw}"))
    print(f"n={n}: largest error {worst:.3f} of 2^-24 |v| + 2^-30")


# ---- 2: full lane registers and the last partial chunk ----
@pytest.mark.parametrize("n", [1023, 1024])
def test_the_largest_sizes_with_64_modules(n):
    mats = D.cohort(n)[[1, 3]].contiguous()
    c = D.partition(n, 64)
    worst = _check_cohort(mats, mats.to(DEV), c, 64, {"keep": 0.1}, f"n={n} M=64")
    print(f"n={n}: largest error {worst:.3f} of the bound")


def test_more_than_1024_nodes_are_refused():
    big, c = torch.zeros(1, 1025, 1025, device=DEV), np.zeros(1025, dtype=np.int64)
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.node_measures(big, keep=0.1, measures=("diversity",), modules=c)
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.module_profile(big, c, keep=0.1)


# ---- 3: determinism ----
def test_a_grid_of_three_gives_the_bits_of_the_default_grid_and_of_a_second_run():
    n, M = 84, 7
    mats = torch.cat([D.cohort(n, seed) for seed in range(50)]).contiguous()
    assert mats.shape[0] == 300
    dev, c = mats.to(DEV), D.case_partition(n, M)

    def run():
        return (ingest.node_measures(dev, keep=0.1, measures=NAMES, modules=c),
                ingest.module_profile(dev, c, keep=0.1, normalize=True))
    few, full = K.check_grid_of_three(run)
    alone = ingest.node_measures(D.cohort(n).to(DEV), keep=0.1, measures=NAMES, modules=c)
    assert torch.equal(_bits(full[0][:6]), _bits(alone)), "a subject's result does not depend on its cohort"
    tail = mats[-6:]
    want = D.cohort_statement(tail, D.host_thresholds(tail, {"keep": 0.1}), c)
    assert _ratio(few[0][-6:].cpu()[:, :, 1:], want[:, :, 1:]) <= 1.0
    assert torch.equal(_bits(few[0][-6:].cpu()[:, :, 0]), _bits(want[:, :, 0].float()))


# ---- 4: mixed requests ----
MIXED = ("participation", "strength", "closeness", "module_zscore", "weighted_closeness", "diversity", "clustering",
         "weighted_participation", "local_efficiency", "weighted_module_zscore")


def test_any_mix_of_the_seventeen_names_is_the_columns_of_the_separate_calls():
    n, M = 84, 7
    dev, c = D.cohort(n).to(DEV), D.case_partition(n, M)
    full = torch.cat([ingest.node_measures(dev, keep=0.1), ingest.node_measures(dev, keep=0.1, measures=P.PATH_MEASURES),
                      ingest.node_measures(dev, keep=0.1, measures=W.WEIGHTED_PATH_MEASURES),
                      ingest.node_measures(dev, keep=0.1, measures=NAMES, modules=c)], 2)
    col = {name: i for i, name in enumerate(ALL17)}
    requests = [MIXED, ALL17, ALL17[::-1], NAMES[::-1], ("module_zscore",), ("weighted_module_zscore", "module_zscore"),
                ("diversity", "degree"), ("eccentricity", "participation")] + [(name,) for name in NAMES]
    for names in requests:
        got = ingest.node_measures(dev, keep=0.1, measures=names, modules=c)
        assert tuple(got.shape) == (6, n, len(names))
        assert torch.equal(_bits(got), _bits(full[:, :, [col[m] for m in names]])), names
    got = ingest.node_measures(dev, num_edges=I.rank_of(n, keep=0.1), measures=ALL17, modules=torch.tensor(c))
    assert torch.equal(_bits(got), _bits(full)), "num_edges=, and the partition as a CPU tensor"
    # a request that names no module measure is what it was
    assert torch.equal(_bits(ingest.node_measures(dev, keep=0.1, measures=ALL17[:12])), _bits(full[:, :, :12]))


def test_datasets_take_the_names_and_the_partition():
    n, M = 84, 7
    dev, y, c = D.cohort(n).to(DEV), I.labels(6).to(DEV), D.case_partition(n, M)
    plain = ingest.from_matrices(dev, y, keep=0.1)
    ds = ingest.from_matrices(dev, y, keep=0.1, measures=MIXED, modules=c)
    for name in ("edge_local", "edge_weight", "labels", "edge_ptr_dev"):
        assert torch.equal(getattr(ds, name), getattr(plain, name)), name
    assert ds.x.shape == (6, n, len(MIXED)) and ds.x.is_contiguous()
    assert torch.equal(_bits(ds.x), _bits(ingest.node_measures(dev, keep=0.1, measures=MIXED, modules=c)))
    S, T = 4, 40
    ts = TS.recipe(S, T, n).to(DEV)
    for window, stride in ((None, None), (20, 10)):
        tds = ingest.from_timeseries(ts, I.labels(S).to(DEV), keep=0.2, window=window, stride=stride, measures=MIXED,
                                     modules=c)
        mats = ingest.correlation_matrices(ts, window=window, stride=stride)
        assert tds.x.shape == (S * TS.num_windows(T, window, stride), n, len(MIXED))
        assert torch.equal(_bits(tds.x), _bits(ingest.node_measures(mats, keep=0.2, measures=MIXED, modules=c)))


@pytest.mark.parametrize("mode", ["union", "mutual"])
def test_knn_is_the_call_on_the_sparsified_matrices(mode):
    n, M = 84, 7
    dev, c = D.cohort(n).to(DEV), D.case_partition(n, M)
    sparse = ingest.knn_sparsify(dev, 8, mode=mode)
    got = ingest.node_measures(dev, knn=8, knn_mode=mode, measures=MIXED, modules=c)
    assert torch.equal(_bits(got), _bits(ingest.node_measures(sparse, min_weight=0.0, measures=MIXED, modules=c)))
    for binary, normalize in FORMS:
        got = ingest.module_profile(dev, c, knn=8, knn_mode=mode, binary=binary, normalize=normalize)
        assert torch.equal(_bits(got), _bits(ingest.module_profile(sparse, c, min_weight=0.0, binary=binary,
                                                                   normalize=normalize)))
    counts = ingest.module_profile(dev, c, knn=8, knn_mode="directed", binary=True).sum(2).cpu()
    positive = ((D.cohort(n) > 0) & ~torch.eye(n, dtype=torch.bool)).sum(2)
    assert torch.equal(counts, positive.clamp(max=8).float()), "the profile of the directed picks sums to min(k, p_i)"


# ---- 5: the profile as node features on the fused path ----
def test_the_normalised_profile_of_seven_networks_trains_on_the_fused_path():
    n, M = 84, 7
    c = D.case_partition(n, M)
    _, prof = K.check_trains_on_the_fused_path(lambda m: ingest.module_profile(m, c, keep=0.1, normalize=True), M)
    rows = prof.sum(2)
    assert bool(((rows - 1).abs() < 1e-6).logical_or(rows == 0).all())


# ---- 6: a kept +inf ----
def test_a_kept_infinity_follows_the_formulas():
    n, M, s = 84, 7, 3
    clean = D.cohort(n)
    c = D.case_partition(n, M)
    home = int(np.argmax(np.bincount(c)))
    members = np.nonzero(c == home)[0]
    assert len(members) >= 3
    i0, j0 = int(members[0]), int(members[1])               # row and column in the same module: sigma_i0 is +inf
    assert float(clean[s, i0, j0]) > 0, "the entry is kept either way: the binary structure does not change"
    mats = clean.clone()
    mats[s, i0, j0] = float("inf")
    got = ingest.node_measures(mats.to(DEV), min_weight=0.0, measures=NAMES, modules=c).cpu()
    ref = ingest.node_measures(clean.to(DEV), min_weight=0.0, measures=NAMES, modules=c).cpu()
    want = D.host_module_measures(mats[s], 0.0, c)
    others = [u for u in range(6) if u != s]
    assert torch.equal(_bits(got[others]), _bits(ref[others])), "every other subject is untouched"
    assert bool(torch.isnan(got[s, i0, [1, 4]]).all()), "the row's weighted participation and diversity"
    assert bool(torch.isnan(got[s, members, 3]).all()), "the weighted z-scores of its module"
    assert torch.equal(torch.isnan(got[s]), torch.isnan(want)), "NaN exactly where the statement has it"
    assert int(torch.isnan(got[s]).sum()) == 2 + len(members)
    assert torch.equal(_bits(got[s, :, 0]), _bits(want[:, 0].float())), "participation is still bit-exact"
    assert torch.equal(_bits(got[s][:, [0, 2]]), _bits(ref[s][:, [0, 2]])), "the binary columns do not see weights"
    rest = ~torch.isnan(got[s])
    assert torch.equal(_bits(got[s][rest]), _bits(ref[s][rest])), "every other value of the subject is untouched"
    for normalize in (False, True):
        a = ingest.module_profile(mats.to(DEV), c, min_weight=0.0, binary=True, normalize=normalize)
        b = ingest.module_profile(clean.to(DEV), c, min_weight=0.0, binary=True, normalize=normalize)
        assert torch.equal(_bits(a), _bits(b))
    prof = ingest.module_profile(mats.to(DEV), c, min_weight=0.0).cpu()
    assert float(prof[s, i0, home]) == float("inf") and int(torch.isinf(prof).sum()) == 1


# ---- 7: an empty cohort ----
def test_no_subjects_give_empty_tensors_without_a_launch():
    n, M = 20, 3
    dev, c = D.cohort(n).to(DEV)[:0], D.partition(n, M)
    K.check_no_subjects(lambda m: ingest.node_measures(m, keep=0.1, measures=MIXED, modules=c), dev, len(MIXED))
    K.check_no_subjects(lambda m: ingest.module_profile(m, c, keep=0.1, binary=True), dev, M)
    lib = _lib.load()
    assert lib.cgnn_ingest_modules(None, 0, n, None, None, M, (ctypes.c_int32 * 1)(4), 1, (ctypes.c_int32 * 1)(0), 1,
                                   None, 0, None, 0, None, 0, 0, _lib.stream_ptr()) == _lib.CGNN_OK
