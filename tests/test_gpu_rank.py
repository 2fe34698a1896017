"""connectome_gnn_amd.ingest.rank_timeseries (csrc/rank.hip) and ``rank=True`` of the connectivity calls on the device,
against the host statement (tests/rank_data.py).

The ranks are exact: every comparison below is of bit patterns, a NaN of the statement matched by ``isnan``.  The one
tolerance is the Spearman parity's, and it is the project's Pearson bound ``timeseries_data.atol(L, kappa)`` applied to
the ranked series (kappa about 1.7): ranking adds no error of its own.
"""
import functools

import numpy as np
import pytest
import scipy.stats
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib, ingest
from connectome_gnn_amd.resident import ResidentDataLoader
from tests import censor_data as CD
from tests import rank_data as RD
from tests import timeseries_data as TS

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 3
# the edges of a wave (64), of the padded power of two, of the 4 columns of an item (n = 1, 3, 5, 7, 17, 33 leave a
# partial item; 16, 20, 84 do not), of the LDS rule (1024 / 1025: 4 -> 2 workgroups a CU; 2048 / 2049: 2 -> 1)
SHAPES = [(2, 1), (3, 7), (63, 16), (64, 17), (65, 5), (127, 84), (128, 3), (129, 33), (300, 84), (1024, 4), (1025, 17),
          (1200, 20), (2048, 2), (2049, 5), (4096, 3)]
WINDOWS = [(200, 50, 10), (67, 33, 17)]
KINDS = [("correlation", 0.0), ("partial", 0.1), ("partial", "ledoit_wolf")]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(got, want, what=""):
    assert got.dtype == torch.float32 and got.device.type == "cuda", what
    assert RD.same_bits(got, want), what


def _unfold(m, L, st):
    return m.unfold(1, L, st).reshape(-1, L).contiguous()


@pytest.mark.parametrize("T,n", SHAPES)
def test_the_ranks_are_the_statements_bit_for_bit(T, n):
    x = RD.series(S, T, n)
    got = ingest.rank_timeseries(x.to(DEV))
    assert tuple(got.shape) == (S, T, n)
    want = RD.series_ranks(S, T, n)
    _same(got, want, (T, n))
    at = RD.nan_at(S, n)
    if at is not None:
        assert np.isnan(want[at[0], :, at[1]]).all() and np.isnan(want).sum() == T
    twice = 2.0 * got.cpu().double()
    twice = twice[~torch.isnan(twice)]
    assert bool((twice == twice.round()).all()) and float(twice.min()) >= 2.0 and float(twice.max()) <= 2.0 * T


def test_the_special_columns_are_exactly_as_stated():
    T, n = 129, 33
    x = RD.series(S, T, n)
    got = ingest.rank_timeseries(x.to(DEV)).cpu()
    col = RD.SPECIAL
    t = torch.arange(T)
    assert bool((got[col["constant"] % S, :, col["constant"]] == (T + 1) / 2).all())
    z = got[col["zeros"] % S, :, col["zeros"]]
    zeros = (x[col["zeros"] % S, :, col["zeros"]] == 0.0)
    assert int(zeros.sum()) >= 2 * (T // 3) and len(set(z[zeros].tolist())) == 1, "-0.0 and +0.0 share a rank"
    i = got[col["infs"] % S, :, col["infs"]]
    assert float(i[T - 1]) == 1.0 and float(i[0]) == float(i[T // 2]) == T - 0.5, "+-inf are ordinary values"
    sub = got[col["subnormal"] % S, :, col["subnormal"]]
    assert torch.equal(sub, (t + 1).float()), "2^-149 steps through 0 are distinct and ordered"
    assert torch.equal(got[col["descending"] % S, :, col["descending"]], (T - t).float())
    # the NaN column is NaN in its unit only; every other bit is that of the run without the NaN
    s, c = RD.nan_at(S, n)
    clean = ingest.rank_timeseries(RD.series(S, T, n, 0, False).to(DEV)).cpu()
    assert bool(torch.isnan(got[s, :, c]).all()) and not bool(torch.isnan(clean).any())
    got[s, :, c] = clean[s, :, c]
    assert torch.equal(_bits(got), _bits(clean))
    # the correlation's constant-ROI rule: an exact zero row and column
    r = ingest.correlation_matrices(RD.series(S, T, n, 0, False).to(DEV), rank=True).cpu()
    k = col["constant"]
    assert bool((r[k % S, k, :] == 0.0).all()) and bool((r[k % S, :, k] == 0.0).all())


@pytest.mark.parametrize("T", (67, 300))
def test_masks(T):
    num, n = len(CD.KINDS), 9
    x, m = RD.series(num, T, n), RD.masks(num, T)
    xd, md = x.to(DEV), m.to(DEV)
    got = ingest.rank_timeseries(xd, sample_mask=md)
    _same(got, RD.host_ranks(x, m), T)
    back = got.cpu()
    assert bool((back[~m] == 0.0).all()) and not bool(torch.signbit(back[~m]).any()), "censored frames are exactly 0.0"
    kept = back[m]
    assert bool(((kept >= 1.0) | torch.isnan(kept)).all())
    for poison in (float("nan"), float("inf"), 1e30):
        bad = x.clone()
        bad[~m] = poison
        assert torch.equal(_bits(ingest.rank_timeseries(bad.to(DEV), sample_mask=md)), _bits(got)), poison
    everything = torch.ones_like(md)
    assert torch.equal(_bits(ingest.rank_timeseries(xd, sample_mask=everything)), _bits(ingest.rank_timeseries(xd)))


@pytest.mark.parametrize("T,L,st", WINDOWS)
def test_windows(T, L, st):
    num, n = len(CD.KINDS), 9
    x, m = RD.series(num, T, n), RD.masks(num, T)
    W = TS.num_windows(T, L, st)
    for keep in (None, m):
        kd = None if keep is None else keep.to(DEV)
        got = ingest.rank_timeseries(x.to(DEV), window=L, stride=st, sample_mask=kd)
        assert tuple(got.shape) == (num * W, L, n)
        _same(got, RD.host_ranks(x, keep, L, st), (T, L, st))
        # ... which is ranking the unfolded units one by one
        units = x.unfold(1, L, st).permute(0, 1, 3, 2).reshape(num * W, L, n).contiguous()
        one_by_one = ingest.rank_timeseries(units.to(DEV), sample_mask=None if keep is None else _unfold(kd, L, st))
        assert torch.equal(_bits(got), _bits(one_by_one))
        out = torch.empty(num * W, L, n, dtype=torch.float32, device=DEV)
        assert ingest.rank_timeseries(x.to(DEV), window=L, stride=st, sample_mask=kd, out=out) is out
        assert torch.equal(_bits(out), _bits(got))


def test_in_place_every_grid_and_every_run_give_the_same_bits():
    num, T, n = 12, 129, 84
    x, m = RD.series(num, T, n), RD.masks(num, T)
    xd, md = x.to(DEV), m.to(DEV)
    full = ingest.rank_timeseries(xd)
    masked = ingest.rank_timeseries(xd, sample_mask=md)
    _same(full, RD.series_ranks(num, T, n))
    assert torch.equal(_bits(ingest.rank_timeseries(xd)), _bits(full)), "a second run"
    lib = _lib.load()
    try:
        assert lib.cgnn_set_fused_grid(3) == _lib.CGNN_OK
        few, few_masked = ingest.rank_timeseries(xd), ingest.rank_timeseries(xd, sample_mask=md)
    finally:
        lib.cgnn_set_fused_grid(0)
    assert torch.equal(_bits(few), _bits(full)) and torch.equal(_bits(few_masked), _bits(masked)), "3 workgroups"
    for keep, want in ((None, full), (md, masked)):
        place = xd.clone()
        assert ingest.rank_timeseries(place, sample_mask=keep, out=place) is place
        assert torch.equal(_bits(place), _bits(want)), "in place"
        try:
            assert lib.cgnn_set_fused_grid(3) == _lib.CGNN_OK
            place = xd.clone()
            ingest.rank_timeseries(place, sample_mask=keep, out=place)
        finally:
            lib.cgnn_set_fused_grid(0)
        assert torch.equal(_bits(place), _bits(want)), "in place, 3 workgroups"


@functools.lru_cache(maxsize=None)
def _cohort():
    """(series, labels, mask): 10 subjects; the mask kinds are those that leave every window more than two frames, so
    that no estimate below is a NaN by ``L_u <= 2``."""
    ts, y = TS.two_classes(10, 200, 20)
    m = torch.stack([CD.mask_of(CD.KINDS[s % 6], 200, s) for s in range(10)]).contiguous()
    return ts.to(DEV), y, m.to(DEV)


@pytest.mark.parametrize("kind,shrinkage", KINDS)
@pytest.mark.parametrize("window,stride", [(None, None), (60, 35)])
@pytest.mark.parametrize("masked", (False, True))
def test_rank_true_is_the_sequence_of_public_calls(kind, shrinkage, window, stride, masked):
    xd, y, md = _cohort()
    keep = md if masked else None
    kw = dict(kind=kind, shrinkage=shrinkage)
    ranked = ingest.rank_timeseries(xd, window=window, stride=stride, sample_mask=keep)
    unit_keep = None if keep is None else (keep if window is None else _unfold(keep, window, stride))
    want = ingest.correlation_matrices(ranked, sample_mask=unit_keep, **kw)
    got = ingest.correlation_matrices(xd, window=window, stride=stride, sample_mask=keep, rank=True, **kw)
    assert torch.equal(_bits(got), _bits(want)), "correlation_matrices"
    assert not torch.equal(_bits(got), _bits(ingest.correlation_matrices(xd, window=window, stride=stride,
                                                                         sample_mask=keep, **kw)))
    if kind == "partial":
        a = ingest.ledoit_wolf_shrinkage(xd, window=window, stride=stride, sample_mask=keep, rank=True)
        assert torch.equal(_bits(a), _bits(ingest.ledoit_wolf_shrinkage(ranked, sample_mask=unit_keep)))
    W = TS.num_windows(200, window, stride)
    ds = ingest.from_timeseries(xd, y, window=window, stride=stride, sample_mask=keep, rank=True, keep=0.1, **kw)
    ref = ingest.from_matrices(want, y.repeat_interleave(W), keep=0.1)
    for name in ("x", "edge_local", "edge_weight", "labels", "edge_ptr_dev"):
        assert torch.equal(getattr(ds, name), getattr(ref, name)), name
    # rank=False is the call without the argument
    plain = ingest.correlation_matrices(xd, window=window, stride=stride, sample_mask=keep, **kw)
    assert torch.equal(_bits(ingest.correlation_matrices(xd, window=window, stride=stride, sample_mask=keep, rank=False,
                                                         **kw)), _bits(plain))
    off = ingest.from_timeseries(xd, y, window=window, stride=stride, sample_mask=keep, rank=False, keep=0.1, **kw)
    base = ingest.from_timeseries(xd, y, window=window, stride=stride, sample_mask=keep, keep=0.1, **kw)
    for name in ("x", "edge_local", "edge_weight", "labels", "edge_ptr_dev"):
        assert torch.equal(getattr(off, name), getattr(base, name)), name
    assert torch.equal(_bits(ingest.ledoit_wolf_shrinkage(xd, window=window, stride=stride, sample_mask=keep,
                                                          rank=False)),
                       _bits(ingest.ledoit_wolf_shrinkage(xd, window=window, stride=stride, sample_mask=keep)))


@pytest.mark.parametrize("T,n", [(300, 84), (1200, 20)])
def test_parity_with_scipys_spearman(T, n):
    x = RD.plain(S, T, n)
    ranks = RD.host_ranks(x)
    assert (ranks.std(1) > 0).all(), "no column compared is constant"
    k = TS.kappa(torch.from_numpy(ranks).float())
    tol = TS.atol(T, k)
    got = ingest.correlation_matrices(x.to(DEV), rank=True).cpu().double().numpy()
    worst = 0.0
    for s in range(S):
        want = scipy.stats.spearmanr(x[s].double().numpy()).statistic
        worst = max(worst, float(np.abs(got[s] - want).max()))
    print(f"T={T} n={n}: kappa {k:.3f}, tol {tol:.3e}, largest error {worst:.3e}")
    assert 1.5 < k < 2.5 and worst <= tol, (worst, tol)


def test_ranks_remove_an_artefact_that_no_frame_list_names():
    """The README's example (``confound_data.spike_pair``): ROIs 0 and 1 share 20 spiky frames of 300 and nothing else.
    fp64 host values: Pearson 0.97576 and 0.97471 (subjects 0 and 1); Spearman, ``np.corrcoef`` of the statement's
    ranks and ``scipy.stats.spearmanr`` alike, 0.15388 and 0.14123 -- the 20 frames still rank together, the other 280
    decide.  Threshold: 0.2."""
    x = RD.spike_pair()
    host = [float(RD.spearman(x[s].numpy())[0, 1]) for s in range(2)]
    assert abs(host[0] - 0.15388) < 1e-5 and abs(host[1] - 0.14123) < 1e-5
    xd = x.to(DEV)
    pearson = ingest.correlation_matrices(xd).cpu()
    spearman = ingest.correlation_matrices(xd, rank=True).cpu()
    tol = TS.atol(300, TS.kappa(torch.from_numpy(RD.host_ranks(x)).float()))
    for s in range(2):
        assert float(pearson[s, 0, 1]) > 0.9
        assert float(spearman[s, 0, 1]) < 0.2
        assert abs(float(spearman[s, 0, 1]) - host[s]) <= tol, (s, float(spearman[s, 0, 1]), host[s], tol)


def test_abi_runs_what_python_runs_and_refuses_before_any_launch():
    lib = _lib.load()
    T, n = 66, 33
    x, m = RD.series(S, T, n), RD.masks(S, T)
    xd, md = x.to(DEV), m.to(DEV)
    sp = _lib.stream_ptr()
    out = torch.full((S, T, n), -7.0, dtype=torch.float32, device=DEV)
    good = [_lib.ptr(xd), S, T, n, 0, 0, _lib.ptr(out), _lib.nbytes(out), sp]
    bad = {"short out": (7, _lib.nbytes(out) - 1), "out NULL": (6, None), "ts NULL": (0, None), "T = 1": (2, 1),
           "out misaligned": (6, _lib.ptr(out) + 2), "window > T": (4, T + 1), "S < 0": (1, -1), "n = 0": (3, 0),
           "L = 4097": (2, 4097)}
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_rank(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    assert lib.cgnn_ingest_rank(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK                     # U == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "nothing was written"
    assert lib.cgnn_ingest_rank(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(out), _bits(ingest.rank_timeseries(xd)))
    L, st = 20, 7
    U = S * TS.num_windows(T, L, st)
    out = torch.full((U, L, n), -7.0, dtype=torch.float32, device=DEV)
    good = [_lib.ptr(xd), S, T, n, L, st, _lib.ptr(md), S * T, _lib.ptr(out), _lib.nbytes(out), sp]
    bad = {"short out": (9, _lib.nbytes(out) - 1), "keep NULL": (6, None), "short keep": (7, S * T - 1),
           "stride = 0": (5, 0), "window = 1": (4, 1)}
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_rank_masked(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    assert lib.cgnn_ingest_rank_masked(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "nothing was written"
    assert lib.cgnn_ingest_rank_masked(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(out), _bits(ingest.rank_timeseries(xd, window=L, stride=st, sample_mask=md)))
    empty = xd[:0]
    assert tuple(ingest.rank_timeseries(empty).shape) == (0, T, n)
    assert tuple(ingest.rank_timeseries(empty, window=L, stride=st).shape) == (0, L, n)
    assert tuple(ingest.correlation_matrices(empty, rank=True).shape) == (0, n, n)


def test_no_temporaries():
    """Above the resident input ``rank_timeseries`` allocates its output and nothing cohort-sized; in place nothing."""
    num, T, n = 60, 300, 360
    xd = RD.plain(2, T, n).repeat(num // 2, 1, 1).contiguous().to(DEV)
    ingest.rank_timeseries(xd)                                                    # (the kernel is loaded)
    size = 4 * num * T * n
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ingest.rank_timeseries(xd)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert size <= peak <= size + 2 ** 20, (peak, size)
    assert torch.equal(_bits(out[:2]), _bits(out[2:4]))
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ingest.rank_timeseries(xd, out=xd)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak <= 2 ** 20, peak


def test_spearman_connectivity_through_loader_and_trainer():
    ts, y = TS.two_classes(32, 200, 20)
    dev = ts.to(DEV)
    ds = ingest.from_timeseries(dev, y, rank=True, keep=0.2, measures=True)
    assert ds.x.shape == (32, 20, 5) and int(ds.edge_ptr[-1]) > 0
    ref = ingest.from_matrices(ingest.correlation_matrices(ingest.rank_timeseries(dev)), y, keep=0.2, measures=True)
    for name in ("x", "edge_local", "edge_weight", "labels", "edge_ptr_dev"):
        assert torch.equal(getattr(ds, name), getattr(ref, name)), name
    pearson = ingest.from_timeseries(dev, y, keep=0.2, measures=True)
    assert not torch.equal(ds.edge_weight, pearson.edge_weight)
    torch.manual_seed(3)
    m = C.GCNConnectome(5, 64, dropout=0.0)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2, weight_decay=1e-4, capturable=True)
    tr = C.Trainer(m, opt, device=DEV, graph=True)
    ld = ResidentDataLoader(ds, 16, shuffle=True, structure_cache=True)
    vl = ResidentDataLoader(ds, 16, shuffle=False, structure_cache=True)
    hist = tr.fit(ld, vl, num_epochs=2, patience=10, verbose=False)
    loss = hist["train_loss"]
    assert len(loss) == 2 and all(torch.isfinite(torch.tensor(v)).all() for v in hist.values())
    assert loss[1] < loss[0], loss
