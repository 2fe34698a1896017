"""connectome_gnn_amd.ingest.knn_sparsify on the device (csrc/knn.hip) against its host statement (tests/knn_data.py):
every mode, size and k, in place and out of place, the grid stride, the C ABI's refusals, ``knn=`` of the four entry
points as the composition it stands for, the minimum degree it exists for, and the result served through
ResidentDataLoader + Trainer.  Everything is compared bit for bit."""
import functools

import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib, ingest
from connectome_gnn_amd.resident import ResidentDataLoader
from connectome_gnn_amd.synthetic import RaggedPackedDataset
from tests import ingest_data as D
from tests import knn_data as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (1, 2, 3, 5, 63, 64, 65, 84, 129, 257, 360)


def _ks(n):
    return sorted({k for k in (0, 1, 2, 5, n // 2, n - 2, n - 1, n, 2 ** 40) if k >= 0})


@functools.lru_cache(maxsize=None)
def _cohort(n):
    mats = K.cohort(n)
    return mats, mats.to(DEV)


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _check(dev, mats, k, modes=K.MODES):
    """knn_sparsify(dev, k) into a NaN-filled output against the host statement, every mode; the picks are sorted once."""
    picks = [K.host_picks(A, k) for A in mats]
    for mode in modes:
        want = torch.stack([torch.where(K.kept_of(A, d, mode), A, torch.zeros_like(A)) for A, d in zip(mats, picks)])
        out = _nan_like(dev)
        got = ingest.knn_sparsify(dev, k, mode=mode, out=out)
        assert got is out and got.dtype == torch.float32 and got.shape == dev.shape
        bad = torch.nonzero(K.bits(got.cpu()) != K.bits(want))
        assert bad.numel() == 0, (k, mode, bad.shape[0], bad[:4].tolist())


@pytest.mark.parametrize("n", SIZES)
def test_knn_equals_the_host_statement(n):
    mats, dev = _cohort(n)
    for k in _ks(n):
        _check(dev, mats, k)
    got = ingest.knn_sparsify(dev, 2)                                  # the defaults: a new tensor, "union"
    assert got.device == dev.device and got.data_ptr() != dev.data_ptr()
    assert torch.equal(K.bits(got.cpu()), K.bits(K.host_knn_cohort(mats, 2, "union")))
    assert torch.equal(K.bits(dev.cpu()), K.bits(mats))


@pytest.mark.parametrize("n", [1023, 1024])
def test_full_lane_registers_and_the_last_tile(n):
    """Subject 1 symmetric rand; subject 2 asymmetric with a block of equal values, larger than the rest, across every
    cut and across a 256-column chunk boundary."""
    g = torch.Generator().manual_seed(n)
    R = torch.rand(n, n, generator=g)
    sym = torch.maximum(R, R.t())
    asym = 0.5 * torch.rand(n, n, generator=g)
    asym[:, 200:300] = 0.75
    asym[n // 2:, 900:] = 0.75
    mats = torch.stack([sym, asym]).contiguous()
    dev = mats.to(DEV)
    for k in (1, 36, 1022):
        _check(dev, mats, k)


@pytest.mark.parametrize("n", [5, 84, 257])
def test_in_place_and_repeated_calls_give_the_same_bits(n):
    mats, dev = _cohort(n)
    for mode in K.MODES:
        for k in (1, 5, n // 2):
            out = _nan_like(dev)
            first = ingest.knn_sparsify(dev, k, mode=mode, out=out)
            assert torch.equal(K.bits(dev), K.bits(mats.to(DEV))), "a separate output leaves the matrices alone"
            again = ingest.knn_sparsify(dev, k, mode=mode)
            work = dev.clone()
            same = ingest.knn_sparsify(work, k, mode=mode, out=work)
            assert same is work
            assert torch.equal(K.bits(again), K.bits(first)) and torch.equal(K.bits(work), K.bits(first)), (mode, k)


def test_many_subjects_walk_the_grid_stride():
    """300 subjects (the n = 84 recipe fifty times over, with noise) on 6 workgroups, then on the default grid."""
    n, S = 84, 300
    g = torch.Generator().manual_seed(7)
    mats = (D.recipe(n).repeat(50, 1, 1) + 0.01 * torch.randn(S, n, n, generator=g)).contiguous()
    mats[6:12] = D.recipe(n)                                # one exact copy, ties and all
    dev = mats.to(DEV)
    want = {mode: K.bits(K.host_knn_cohort(mats, 8, mode)) for mode in K.MODES}
    lib = _lib.load()
    try:
        assert lib.cgnn_set_fused_grid(3) == _lib.CGNN_OK
        few = {mode: ingest.knn_sparsify(dev, 8, mode=mode, out=_nan_like(dev)) for mode in K.MODES}
    finally:
        lib.cgnn_set_fused_grid(0)
    for mode in K.MODES:
        assert torch.equal(K.bits(few[mode].cpu()), want[mode]), mode
        full = ingest.knn_sparsify(dev, 8, mode=mode, out=_nan_like(dev))
        assert torch.equal(K.bits(full.cpu()), want[mode]), mode


def test_knn_abi_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    n = 20
    mats = D.recipe(n)
    S = mats.shape[0]
    dev = mats.to(DEV)
    out = torch.full((S, n, n), -7.0, dtype=torch.float32, device=DEV)
    sp = _lib.stream_ptr()
    nbytes = _lib.nbytes(out)
    assert nbytes == 4 * S * n * n
    good = [_lib.ptr(dev), S, n, 4, _lib.KNN_UNION, _lib.ptr(out), nbytes, sp]

    def rc(at, v):
        return lib.cgnn_ingest_knn(*(good[:at] + [v] + good[at + 1:]))

    bad = {"matrices NULL": (0, None), "out NULL": (5, None), "S < 0": (1, -1), "n = 0": (2, 0), "k < 0": (3, -1),
           "mode 3": (4, 3), "out_bytes one byte short": (6, nbytes - 1), "S * n >= 2^31": (1, 2 ** 31 // n + 1)}
    for name, (at, v) in bad.items():
        assert rc(at, v) == _lib.CGNN_EINVAL, name
    assert rc(2, 1025) == _lib.CGNN_EUNSUPPORTED
    # an output one subject into the matrices overlaps them without being them
    big = torch.full((S + 1, n, n), -7.0, dtype=torch.float32, device=DEV)
    assert lib.cgnn_ingest_knn(_lib.ptr(big), S, n, 4, _lib.KNN_UNION, _lib.ptr(big[1:]), nbytes, sp) == _lib.CGNN_EINVAL
    assert lib.cgnn_ingest_knn(_lib.ptr(big[1:]), S, n, 4, _lib.KNN_UNION, _lib.ptr(big), nbytes, sp) == _lib.CGNN_EINVAL
    assert rc(1, 0) == _lib.CGNN_OK                         # no subjects: nothing launched
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((big == -7.0).all())
    assert lib.cgnn_ingest_knn(*good) == _lib.CGNN_OK       # the documented size is accepted
    assert torch.equal(K.bits(out.cpu()), K.bits(K.host_knn_cohort(mats, 4, "union")))


def _same_dataset(got, want):
    """got (device) == want (host RaggedPackedDataset), every field, dtypes and shapes included."""
    assert type(got) is RaggedPackedDataset
    for name in ("x", "edge_local", "edge_weight", "labels"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.device.type == "cuda" and a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, a.shape, b.shape)
        assert torch.equal(a.cpu(), b), name
    assert torch.equal(got.edge_ptr, want.edge_ptr) and torch.equal(got.edge_ptr_dev.cpu(), want.edge_ptr)


def _same_bits(a, b):
    """two device datasets, every field bit for bit"""
    for name in ("x", "edge_local", "edge_weight", "labels", "edge_ptr", "edge_ptr_dev"):
        u, v = getattr(a, name), getattr(b, name)
        assert u.dtype == v.dtype and u.shape == v.shape and u.device == v.device, name
        if u.dtype == torch.float32:
            u, v = K.bits(u), K.bits(v)
        assert torch.equal(u, v), name


@pytest.mark.parametrize("n", [5, 84])
def test_from_matrices_is_the_composition(n):
    mats, dev = _cohort(n)
    S = mats.shape[0]
    x, y = D.features(S, n), D.labels(S)
    xd = x.to(DEV)
    for k in (2, 8):
        for mode in K.MODES:
            B = K.host_knn_cohort(mats, k, mode)
            got = ingest.from_matrices(dev, y, knn=k, knn_mode=mode, node_features=xd)
            want = RaggedPackedDataset.from_graphs(D.host_graphs(B, [0.0] * S, x, y))
            _same_dataset(got, want)
            two = ingest.from_matrices(ingest.knn_sparsify(dev, k, mode=mode), y, min_weight=0.0, node_features=xd)
            _same_bits(got, two)
            # the default strength feature is the k-NN graph's
            got = ingest.from_matrices(dev, y, knn=k, knn_mode=mode)
            _same_bits(got, ingest.from_matrices(ingest.knn_sparsify(dev, k, mode=mode), y, min_weight=0.0))
            assert got.x.shape == (S, n, 1)
            _same_bits(got, ingest.from_matrices(B.to(DEV), y, min_weight=0.0))
            assert torch.equal(got.edge_ptr, want.edge_ptr)
            assert torch.equal(K.bits(dev.cpu()), K.bits(mats)), "the caller's matrices are untouched"
    got = ingest.from_matrices(dev, y, knn=3)                          # knn_mode defaults to "union"
    _same_bits(got, ingest.from_matrices(ingest.knn_sparsify(dev, 3), y, min_weight=0.0))


@pytest.mark.parametrize("n", [5, 84])
def test_measures_and_path_lengths_are_the_composition(n):
    mats, dev = _cohort(n)
    names = ingest.MEASURES + ingest.PATH_MEASURES + ingest.WEIGHTED_PATH_MEASURES
    for k, mode in ((2, "union"), (8, "mutual"), (3, "directed")):
        sparse = ingest.knn_sparsify(dev, k, mode=mode)
        got = ingest.node_measures(dev, knn=k, knn_mode=mode, measures=names)
        want = ingest.node_measures(sparse, min_weight=0.0, measures=names)
        assert got.shape == (mats.shape[0], n, len(names)) and torch.equal(K.bits(got), K.bits(want)), (k, mode)
        got = ingest.path_lengths(dev, knn=k, knn_mode=mode)
        assert torch.equal(K.bits(got), K.bits(ingest.path_lengths(sparse, min_weight=0.0))), (k, mode)
        ds = ingest.from_matrices(dev, D.labels(mats.shape[0]), knn=k, knn_mode=mode, measures=names)
        assert torch.equal(K.bits(ds.x), K.bits(want))
        assert torch.equal(K.bits(dev.cpu()), K.bits(mats)), "the caller's matrices are untouched"


def test_from_timeseries_is_the_composition():
    ts = torch.randn(6, 40, 20, generator=torch.Generator().manual_seed(4)).to(DEV)
    y = D.labels(6)
    before = ts.clone()
    for k, mode in ((3, "union"), (5, "mutual")):
        got = ingest.from_timeseries(ts, y, knn=k, knn_mode=mode)
        sparse = ingest.knn_sparsify(ingest.correlation_matrices(ts), k, mode=mode)
        _same_bits(got, ingest.from_matrices(sparse, y, min_weight=0.0))
        host = K.host_knn_cohort(ingest.correlation_matrices(ts).cpu(), k, mode)
        assert torch.equal(K.bits(sparse.cpu()), K.bits(host))
    got = ingest.from_timeseries(ts, y, knn=4, window=20, stride=10, absolute=True)      # 3 windows a subject
    sparse = ingest.knn_sparsify(ingest.correlation_matrices(ts, window=20, stride=10, absolute=True), 4)
    _same_bits(got, ingest.from_matrices(sparse, y.repeat_interleave(3), min_weight=0.0))
    assert torch.equal(ts, before)


def test_every_node_keeps_its_minimum_degree():
    """"union" at k = 8 on the finite symmetric recipe subjects at n = 84: every node has at least min(8, p_i) edges.
    Subject 2 (heavy ties) has p_i >= 80 everywhere and its k-NN graph 846 edges.  One threshold per subject does not
    get there.  At the usual keep = 0.10, a budget of 697 <= 846 edges, the tie class of the largest value straddles
    the cut and subject 2 keeps no edge at all: every node is isolated.  At the k-NN graph's own budget, num_edges = 846,
    the threshold keeps 818 edges and the weakest node one of them, against 8.  (Both were worked out from the host
    statement on the CPU and are asserted on it here, next to the device's answer.)"""
    n, k = 84, 8
    mats = D.recipe(n)[:3].contiguous()                     # signed symmetric, heavy ties, all zeros
    y = D.labels(3)
    dev = mats.to(DEV)
    ds = ingest.from_matrices(dev, y, knn=k)
    p = torch.stack([K.candidates(A).sum(1) for A in mats])
    for s in range(3):
        lo, hi = int(ds.edge_ptr[s]), int(ds.edge_ptr[s + 1])
        degree = torch.bincount(ds.edge_local[0, lo:hi].cpu(), minlength=n)
        assert bool((degree >= torch.clamp(p[s], max=k)).all()), s
    assert int(p[1].min()) >= k
    budget = int(ds.edge_ptr[2] - ds.edge_ptr[1])           # subject 2's k-NN edges
    assert budget == int(K.host_kept(mats[1], k, "union").sum()) == 846
    usual = D.rank_of(n, keep=0.10)
    assert usual == 697 <= budget
    for kind, v, edges, weakest in (("keep", 0.10, 0, 0), ("num_edges", budget, 818, 1)):
        ei, _ = D.host_edges(mats[1], D.host_threshold(mats[1], D.rank_of(n, **{kind: v})))   # the host statement
        assert ei.shape[1] == edges and int(torch.bincount(ei[0], minlength=n).min()) == weakest
        one = ingest.from_matrices(dev[1:2], y[:1], **{kind: v})
        assert int(one.edge_ptr[-1]) == edges
        assert int(torch.bincount(one.edge_local[0].cpu(), minlength=n).min()) == weakest < k


def test_knn_through_loader_and_trainer():
    """12 subjects x 84 nodes, knn = 8, the default strength feature: one epoch of a hidden-64 GCN over
    ResidentDataLoader(structure_cache=True) with captured steps runs on the fused path and its loss is finite."""
    S, n = 12, 84
    g = torch.Generator().manual_seed(9)
    R = torch.rand(S, n, n, generator=g)
    mats = ((R + R.transpose(1, 2)) / 2).contiguous()
    y = D.labels(S)
    ds = ingest.from_matrices(mats.to(DEV), y, knn=8)
    assert ds.x.shape == (S, n, 1) and int((ds.edge_ptr[1:] - ds.edge_ptr[:-1]).min()) >= 8 * n
    torch.manual_seed(3)
    m = C.GCNConnectome(1, 64, dropout=0.0)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
    tr = C.Trainer(m, opt, device=DEV, graph=True)
    ld = ResidentDataLoader(ds, 4, shuffle=True, structure_cache=True)
    vl = ResidentDataLoader(ds, 4, shuffle=False, structure_cache=True)
    hist = tr.fit(ld, vl, num_epochs=1, patience=10, verbose=False)
    assert tr.model.impl_used == "fused"
    assert len(hist["train_loss"]) == 1 and all(torch.isfinite(torch.tensor(v)).all() for v in hist.values())
