"""connectome_gnn_amd.ingest on the device (csrc/ingest.hip) against its host statement (tests/ingest_data.py):
thresholds, the dataset arrays, the default strength feature, the grid stride, 64-bit offsets, the C ABI's
refusals, and the result served through ResidentDataLoader + Trainer.  Everything is compared bit for bit
unless a tolerance is stated."""
import functools

import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib, ingest
from connectome_gnn_amd.resident import ResidentDataLoader
from connectome_gnn_amd.synthetic import RaggedPackedDataset
from tests import ingest_data as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 2, 5, 20, 63, 64, 65, 84, 257, 360]
KEEPS = (0.1, 0.29, 0.5)


def _ranks(n):
    m = n * (n - 1)
    ks = [("num_edges", k) for k in (0, 1, m - 1, m, m + 7) if k >= 0]
    return ks + [("keep", f) for f in KEEPS]


@functools.lru_cache(maxsize=None)
def _cohort(n):
    """(host matrices [10, n, n] = the six recipes + the four worst cases, their sorted candidates, device copy)."""
    mats = torch.cat([D.recipe(n), D.worst_cases(n)]).contiguous()
    return mats, tuple(D.host_sorted(A) for A in mats), mats.to(DEV)


def _host_thr(n, kind, v):
    k = D.rank_of(n, **{kind: v})
    return torch.tensor([D.rank_value(c, k) for c in _cohort(n)[1]], dtype=torch.float32)


def _same_dataset(got, want):
    """got (device) == want (host RaggedPackedDataset), every field, dtypes and shapes included."""
    assert type(got) is RaggedPackedDataset
    for name in ("x", "edge_local", "edge_weight", "labels"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.device.type == "cuda" and a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, a.shape, b.shape)
        assert torch.equal(a.cpu(), b), name
    assert got.edge_ptr.device.type == "cpu" and got.edge_ptr.dtype == torch.long
    assert torch.equal(got.edge_ptr, want.edge_ptr)
    assert got.edge_ptr_dev.device.type == "cuda" and got.edge_ptr_dev.dtype == torch.long
    assert torch.equal(got.edge_ptr_dev.cpu(), want.edge_ptr)


def _want(mats, thr, x, y):
    return RaggedPackedDataset.from_graphs(D.host_graphs(mats, thr.tolist(), x, y))


@pytest.mark.parametrize("n", SIZES)
def test_thresholds_equal_the_host_statement(n):
    mats, _, dev = _cohort(n)
    for kind, v in _ranks(n):
        got = ingest.select_thresholds(dev, **{kind: v})
        assert got.device.type == "cuda" and got.dtype == torch.float32 and got.shape == (mats.shape[0],)
        want = _host_thr(n, kind, v)
        assert torch.equal(got.cpu(), want), (kind, v, got.cpu().tolist(), want.tolist())   # (-0.0 == 0.0)


@pytest.mark.parametrize("n", SIZES)
def test_dataset_equals_from_graphs_of_the_host_statement(n):
    mats, _, dev = _cohort(n)
    S = mats.shape[0]
    x, y = D.features(S, n), D.labels(S)
    xd = x.to(DEV)
    for kind, v in _ranks(n):
        got = ingest.from_matrices(dev, y if kind == "keep" else y.to(DEV), node_features=xd, **{kind: v})
        assert got.x is xd                                  # the caller's features, as they are
        _same_dataset(got, _want(mats, _host_thr(n, kind, v), x, y))
        if n == 84 and kind == "keep" and v == 0.1:
            assert (got.edge_ptr[1:7] - got.edge_ptr[:6]).tolist() == D.COUNTS_84[0.1]
            again = ingest.from_matrices(dev, y, node_features=xd, keep=v)     # two calls: identical bits
            for name in ("edge_local", "edge_weight", "edge_ptr_dev"):
                assert torch.equal(getattr(again, name), getattr(got, name)), name
    # absolute thresholds: a scalar, +-inf, and one per subject (host or device tensor)
    for t in (0.25, 0.0, -1.0, float("inf"), float("-inf")):
        got = ingest.from_matrices(dev, y, min_weight=t, node_features=xd)
        _same_dataset(got, _want(mats, torch.full((S,), t), x, y))
    per = torch.tensor([0.3, 0.5, float("-inf"), 0.9, float("inf"), 0.1, 0.5, 1.0001, -0.5, 1.0])
    for t in (per, per.to(DEV), per.double()):
        _same_dataset(ingest.from_matrices(dev, y, min_weight=t, node_features=xd), _want(mats, per, x, y))


@pytest.mark.parametrize("n", [1, 2, 5, 65, 84, 360])
def test_default_strength_feature(n):
    """Recipe subjects 1 to 4 (finite) against the fp64 statement, atol = (n + 2) 2^-23: twice the first-order
    bound of an fp32 sum of at most n - 1 positive terms in any order plus the division, on values in [0, 1]."""
    mats = D.recipe(n)[:4].contiguous()
    y = D.labels(4)
    for keep in (0.29, 1.0):
        k = D.rank_of(n, keep=keep)
        ds = ingest.from_matrices(mats.to(DEV), y, keep=keep)
        assert ds.x.shape == (4, n, 1) and ds.x.dtype == torch.float32
        want = torch.stack([D.host_strength_feature(A, D.host_threshold(A, k)) for A in mats])
        err = float((ds.x.cpu().double() - want).abs().max())
        assert err <= (n + 2) * 2.0 ** -23, (keep, err)
        assert torch.equal(ds.x[2].cpu(), torch.zeros(n, 1))               # the empty subject
        _same_dataset(ds, _want(mats, D.host_thresholds(mats, k), ds.x.cpu(), y))
    # the same call on the same matrices gives the same bits
    assert torch.equal(ingest.from_matrices(mats.to(DEV), y, keep=1.0).x, ds.x)


def test_many_subjects_walk_the_grid_stride():
    """300 subjects (the n = 84 recipe fifty times over, with noise) on 9 select / 24 fill workgroups, then on the
    default grid."""
    n, S = 84, 300
    g = torch.Generator().manual_seed(7)
    mats = (D.recipe(n).repeat(50, 1, 1) + 0.01 * torch.randn(S, n, n, generator=g)).contiguous()
    mats[6:12] = D.recipe(n)                                # one exact copy, ties and all
    x, y = D.features(S, n), D.labels(S)
    k = D.rank_of(n, keep=0.1)
    thr = D.host_thresholds(mats, k)
    want = _want(mats, thr, x, y)
    dev, xd = mats.to(DEV), x.to(DEV)
    lib = _lib.load()
    try:
        assert lib.cgnn_set_fused_grid(3) == _lib.CGNN_OK
        assert torch.equal(ingest.select_thresholds(dev, keep=0.1).cpu(), thr)
        _same_dataset(ingest.from_matrices(dev, y, keep=0.1, node_features=xd), want)
        few = ingest.from_matrices(dev, y, keep=0.1).x
    finally:
        lib.cgnn_set_fused_grid(0)
    assert torch.equal(ingest.select_thresholds(dev, keep=0.1).cpu(), thr)
    _same_dataset(ingest.from_matrices(dev, y, keep=0.1, node_features=xd), want)
    # (bits: the rows with an infinite weight have strength inf / inf = NaN)
    assert torch.equal(ingest.from_matrices(dev, y, keep=0.1).x.view(torch.int32), few.view(torch.int32))


def test_offsets_beyond_2_31_elements():
    """16,600 x 360 x 360 = 2.15 G elements (8.6 GB), generated on the device; keep = 0.01; subjects 0, S // 2 and
    S - 1 against the host statement."""
    S, n, keep = 16600, 360, 0.01
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip(f"needs 24 GB of free device memory, {free / 2 ** 30:.1f} GB are free")
    assert S * n * n > 2 ** 31
    torch.manual_seed(5)
    mats = torch.rand(S, n, n, device=DEV)
    y = torch.zeros(S, dtype=torch.long)
    k = D.rank_of(n, keep=keep)
    thr = ingest.select_thresholds(mats, keep=keep)
    ds = ingest.from_matrices(mats, y, keep=keep)
    assert ds.edge_ptr[0] == 0 and ds.edge_ptr.shape == (S + 1,) and torch.equal(ds.edge_ptr_dev.cpu(), ds.edge_ptr)
    counts = ds.edge_ptr[1:] - ds.edge_ptr[:-1]
    assert int(counts.max()) <= k and int(counts.min()) >= k - 8          # (rand: ties are rare)
    for s in (0, S // 2, S - 1):
        A = mats[s].cpu()
        t = D.host_threshold(A, k)
        assert float(thr[s]) == t, s
        ei, w = D.host_edges(A, t)
        lo, hi = int(ds.edge_ptr[s]), int(ds.edge_ptr[s + 1])
        assert torch.equal(ds.edge_local[:, lo:hi].cpu(), ei) and torch.equal(ds.edge_weight[lo:hi].cpu(), w), s
        want = D.host_strength_feature(A, t)
        assert float((ds.x[s].cpu().double() - want).abs().max()) <= (n + 2) * 2.0 ** -23, s
    del mats, ds


def _refusals(fn, good, written, required, scalars, sentinels):
    """Every bad form of `good` returns CGNN_EINVAL and leaves the sentinel-filled outputs alone.
    written: (pointer position, byte-count position) of each written buffer; required: positions of the pointers
    that may not be NULL; scalars: {name: (position, value)}."""
    bad = {}
    for p, nb in written:
        bad[f"buffer at {p} one byte short"] = good[:nb] + [good[nb] - 1] + good[nb + 1:]
    for p in required:
        bad[f"pointer at {p} NULL"] = good[:p] + [None] + good[p + 1:]
    for name, (p, v) in scalars.items():
        bad[name] = good[:p] + [v] + good[p + 1:]
    for name, args in bad.items():
        assert fn(*args) == _lib.CGNN_EINVAL, name
    torch.cuda.synchronize()
    for t, v in sentinels:
        assert bool((t == v).all())


def test_ingest_abi_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    n = 20
    mats = D.recipe(n)
    S = mats.shape[0]
    dev = mats.to(DEV)
    k = D.rank_of(n, keep=0.29)
    thr_h = D.host_thresholds(mats, k)
    edges = [D.host_edges(A, float(t)) for A, t in zip(mats, thr_h)]
    E = sum(w.numel() for _, w in edges)
    sp = _lib.stream_ptr()
    limits = {"S < 0": (1, -1), "n = 0": (2, 0), "n < 0": (2, -1), "S * n >= 2^31": (1, 2 ** 31 // n + 1),
              "n * n >= 2^31": (2, 46341)}

    def f32(numel):
        return torch.full((numel,), -7.0, dtype=torch.float32, device=DEV)

    # ---- select
    thr = f32(S)
    good = [_lib.ptr(dev), S, n, k, _lib.ptr(thr), _lib.nbytes(thr), sp]
    _refusals(lib.cgnn_ingest_select, good, [(4, 5)], [0, 4], dict(limits, **{"k < 0": (3, -1)}), [(thr, -7.0)])
    assert lib.cgnn_ingest_select(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK
    assert lib.cgnn_ingest_select(None, 0, n, k, None, 0, sp) == _lib.CGNN_OK
    torch.cuda.synchronize()
    assert bool((thr == -7.0).all())
    assert lib.cgnn_ingest_select(*good) == _lib.CGNN_OK
    assert torch.equal(thr.cpu(), thr_h)
    # ---- count (selecting, and with the thresholds given)
    rc = torch.full((S * n,), -7, dtype=torch.int32, device=DEV)
    st = f32(S * n)
    thr2 = f32(S)
    good = [_lib.ptr(dev), S, n, 1, k, _lib.ptr(thr2), _lib.nbytes(thr2), _lib.ptr(rc), _lib.nbytes(rc), _lib.ptr(st),
            _lib.nbytes(st), sp]
    _refusals(lib.cgnn_ingest_count, good, [(5, 6), (7, 8), (9, 10)], [0, 5, 7], dict(limits, **{"k < 0": (4, -1)}),
              [(thr2, -7.0), (rc, -7), (st, -7.0)])
    assert lib.cgnn_ingest_count(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK
    torch.cuda.synchronize()
    assert bool((thr2 == -7.0).all()) and bool((rc == -7).all()) and bool((st == -7.0).all())
    assert lib.cgnn_ingest_count(*good) == _lib.CGNN_OK
    want_rc = torch.cat([torch.bincount(ei[0], minlength=n) for ei, _ in edges]).int()
    assert torch.equal(thr2.cpu(), thr_h) and torch.equal(rc.cpu(), want_rc)
    rc2 = torch.full_like(rc, -7)
    assert lib.cgnn_ingest_count(_lib.ptr(dev), S, n, 0, 0, _lib.ptr(thr), _lib.nbytes(thr), _lib.ptr(rc2),
                                 _lib.nbytes(rc2), None, 0, sp) == _lib.CGNN_OK          # no strength wanted
    assert torch.equal(rc2, rc)
    # ---- fill
    row_off = torch.zeros(S * n + 1, dtype=torch.long, device=DEV)
    row_off[1:] = torch.cumsum(rc, 0)
    el = torch.full((2, E), -7, dtype=torch.long, device=DEV)
    ew = f32(E)
    good = [_lib.ptr(dev), S, n, _lib.ptr(thr), _lib.ptr(row_off), E, _lib.ptr(el), _lib.nbytes(el), _lib.ptr(ew),
            _lib.nbytes(ew), sp]
    _refusals(lib.cgnn_ingest_fill, good, [(6, 7), (8, 9)], [0, 3, 4, 6, 8],
              dict(limits, **{"num_edges < 0": (5, -1), "num_edges > S n (n - 1)": (5, S * n * (n - 1) + 1)}),
              [(el, -7), (ew, -7.0)])
    assert lib.cgnn_ingest_fill(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK
    assert lib.cgnn_ingest_fill(*(good[:5] + [0] + good[6:])) == _lib.CGNN_OK
    torch.cuda.synchronize()
    assert bool((el == -7).all()) and bool((ew == -7.0).all())
    assert lib.cgnn_ingest_fill(*good) == _lib.CGNN_OK
    assert torch.equal(el.cpu(), torch.cat([ei for ei, _ in edges], 1))
    assert torch.equal(ew.cpu(), torch.cat([w for _, w in edges]))


def _fit(ds, in_channels):
    torch.manual_seed(3)
    m = C.GCNConnectome(in_channels, 64, dropout=0.0)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
    tr = C.Trainer(m, opt, device=DEV, graph=True)
    ld = ResidentDataLoader(ds, 16, shuffle=True, structure_cache=True)
    vl = ResidentDataLoader(ds, 16, shuffle=False, structure_cache=True)
    hist = tr.fit(ld, vl, num_epochs=2, patience=10, verbose=False)
    return tr, hist, [p.detach().clone() for p in tr.model.parameters()]


def test_matrices_through_loader_and_trainer():
    """72 subjects x 84 nodes, symmetric matrices, keep = 0.1, explicit 5-wide features, two classes: Trainer.fit
    over ResidentDataLoader(structure_cache=True) on the dataset from_matrices built equals, bit for bit, the same
    run on RaggedPackedDataset.from_graphs of the host-built graphs; captured steps serve both batch sizes."""
    S, n = 72, 84
    g = torch.Generator().manual_seed(9)
    R = torch.rand(S, n, n, generator=g)
    mats = ((R + R.transpose(1, 2)) / 2).contiguous()
    y = D.labels(S)
    mats[y == 1, : n // 2, : n // 2] *= 1.5                   # a block the classes differ in (still symmetric)
    x = D.features(S, n)
    k = D.rank_of(n, keep=0.1)
    dev = mats.to(DEV)
    ds = ingest.from_matrices(dev, y, keep=0.1, node_features=x.to(DEV))
    ref = _want(mats, D.host_thresholds(mats, k), x, y)
    _same_dataset(ds, ref)
    assert int(ds.edge_ptr[-1]) > 0
    tr_a, hist_a, par_a = _fit(ds, 5)
    tr_b, hist_b, par_b = _fit(ref.to(DEV), 5)
    assert hist_a == hist_b and len(hist_a["train_loss"]) == 2
    assert all(torch.isfinite(torch.tensor(v)).all() for v in hist_a.values())
    for a, b in zip(par_a, par_b):
        assert torch.equal(a, b)
    for tr in (tr_a, tr_b):
        assert sorted(key[2] for key in tr._graphs if key[0] == "resident") == [8, 16]
    # the default strength feature: one input channel keeps the hidden-64 GCN on its fused path
    ds1 = ingest.from_matrices(dev, y, keep=0.1)
    assert ds1.x.shape == (S, n, 1)
    tr, hist, _ = _fit(ds1, 1)
    assert tr.model.impl_used == "fused"
    assert all(torch.isfinite(torch.tensor(v)).all() for v in hist.values())
