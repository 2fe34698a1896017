"""connectome_gnn_amd.ingest.mst_backbone on the device (csrc/mst.hip) against its host statement (tests/mst_data.py):
every size and choice of threshold, in place and out of place, the grid stride, the C ABI's refusals, ``backbone=`` of the
five entry points as the compositions it stands for, the connectedness it exists for, and the result served through
ResidentDataLoader + Trainer.  Everything is compared bit for bit; outputs are pre-filled with NaN."""
import functools

import pytest
import torch
from scipy.sparse.csgraph import connected_components

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib, ingest
from connectome_gnn_amd.resident import ResidentDataLoader
from connectome_gnn_amd.synthetic import RaggedPackedDataset
from tests import ingest_data as D
from tests import knn_data as K
from tests import mst_data as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
SIZES = (1, 2, 3, 5, 63, 64, 65, 84, 129, 257, 360)
CHOICES = (dict(), dict(keep=0.1), dict(keep=1.0), dict(num_edges=0), dict(min_weight=0.3))


@functools.lru_cache(maxsize=None)
def _cohort(n):
    mats = M.cohort(n)
    return mats, mats.to(DEV)


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _host_thresholds(mats, keep=None, num_edges=None, min_weight=None):
    """What the statement of ``select_thresholds`` / ``from_matrices`` gives for the choice; None for no choice."""
    n = mats.shape[1]
    if min_weight is not None:
        return [float(min_weight)] * mats.shape[0]
    if keep is None and num_edges is None:
        return None
    return [D.host_threshold(A, D.rank_of(n, keep=keep, num_edges=num_edges)) for A in mats]


def _assert_bits(got, want, what):
    bad = torch.nonzero(M.bits(got.cpu()) != M.bits(want))
    assert bad.numel() == 0, (what, bad.shape[0], bad[:4].tolist())


def _abi_call(dev, thr, out):
    """cgnn_ingest_mst through the C ABI with a workspace of the size its query names; the return code."""
    lib = _lib.load()
    S, n = dev.shape[0], dev.shape[1]
    need = lib.cgnn_ingest_mst_workspace_bytes(S, n)
    assert need > 0
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = lib.cgnn_ingest_mst(_lib.ptr(dev), S, n, _lib.ptr(thr), _lib.ptr(work), need, _lib.ptr(out), _lib.nbytes(out),
                             _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("n", SIZES)
def test_backbone_equals_the_host_statement(n):
    mats, dev = _cohort(n)
    forests = M.forests(n)
    for choice in CHOICES:
        want = M.host_backbone_cohort(mats, _host_thresholds(mats, **choice), forests)
        out = _nan_like(dev)
        got = ingest.mst_backbone(dev, out=out, **choice)
        assert got is out and got.dtype == torch.float32 and got.shape == dev.shape
        _assert_bits(got, want, choice)
    got = ingest.mst_backbone(dev)                                      # the defaults: a new tensor, the tree alone
    assert got.device == dev.device and got.data_ptr() != dev.data_ptr()
    _assert_bits(got, M.host_backbone_cohort(mats, None, forests), "defaults")
    assert torch.equal(M.bits(dev.cpu()), M.bits(mats))
    # thresholds of every kind through the C ABI: +inf (the tree alone), -inf (every positive entry), a number
    thr = torch.tensor([(INF, -INF, 0.3)[s % 3] for s in range(mats.shape[0])], dtype=torch.float32)
    out = _nan_like(dev)
    assert _abi_call(dev, thr.to(DEV), out) == _lib.CGNN_OK
    _assert_bits(out, M.host_backbone_cohort(mats, thr.tolist(), forests), "C ABI")


@pytest.mark.parametrize("n", [1023, 1024])
def test_every_lane_owns_four_nodes(n):
    """Subject 1 symmetric rand; subject 2 asymmetric with blocks of equal values, larger than the rest, that span the
    256-column boundaries: the order among equal weights is the pairs'."""
    g = torch.Generator().manual_seed(n)
    R = torch.rand(n, n, generator=g)
    sym = torch.maximum(R, R.t())
    asym = 0.5 * torch.rand(n, n, generator=g)
    asym[:, 200:300] = 0.75
    asym[n // 2:, 900:] = 0.75
    mats = torch.stack([sym, asym]).contiguous()
    dev = mats.to(DEV)
    forests = [M.host_forest(A) for A in mats]
    assert [int(F.sum()) for F in forests] == [2 * (n - 1)] * 2
    for choice in (dict(), dict(keep=0.1)):
        out = ingest.mst_backbone(dev, out=_nan_like(dev), **choice)
        _assert_bits(out, M.host_backbone_cohort(mats, _host_thresholds(mats, **choice), forests), choice)


@pytest.mark.parametrize("n", [5, 84, 257])
def test_in_place_and_repeated_calls_give_the_same_bits(n):
    mats, dev = _cohort(n)
    for choice in (dict(), dict(keep=0.1), dict(min_weight=0.3)):
        first = ingest.mst_backbone(dev, out=_nan_like(dev), **choice)
        assert torch.equal(M.bits(dev), M.bits(mats.to(DEV))), "a separate output leaves the matrices alone"
        again = ingest.mst_backbone(dev, **choice)
        work = dev.clone()
        same = ingest.mst_backbone(work, out=work, **choice)
        assert same is work
        assert torch.equal(M.bits(again), M.bits(first)) and torch.equal(M.bits(work), M.bits(first)), choice
        _assert_bits(first, M.host_backbone_cohort(mats, _host_thresholds(mats, **choice), M.forests(n)), choice)


def test_many_subjects_walk_the_grid_stride():
    """300 subjects (the n = 84 recipe fifty times over, with noise, and one exact copy) on 6 workgroups, then on the
    default grid: a workgroup's slab and its parent[] are reused from subject to subject."""
    n, S = 84, 300
    g = torch.Generator().manual_seed(7)
    mats = (D.recipe(n).repeat(50, 1, 1) + 0.01 * torch.randn(S, n, n, generator=g)).contiguous()
    mats[6:12] = D.recipe(n)                                # one exact copy, ties and all
    dev = mats.to(DEV)
    forests = [M.host_forest(A) for A in mats]
    choices = (dict(), dict(keep=0.1))
    want = [M.host_backbone_cohort(mats, _host_thresholds(mats, **c), forests) for c in choices]
    lib = _lib.load()
    try:
        assert lib.cgnn_set_fused_grid(3) == _lib.CGNN_OK
        assert lib.cgnn_ingest_mst_workspace_bytes(S, n) == 6 * n * n * 4
        few = [ingest.mst_backbone(dev, out=_nan_like(dev), **c) for c in choices]
    finally:
        lib.cgnn_set_fused_grid(0)
    for c, f, w in zip(choices, few, want):
        _assert_bits(f, w, ("6 workgroups", c))
        _assert_bits(ingest.mst_backbone(dev, out=_nan_like(dev), **c), w, ("the default grid", c))


def test_mst_abi_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    n = 20
    mats = D.recipe(n)
    S = mats.shape[0]
    dev = mats.to(DEV)
    out = torch.full((S, n, n), -7.0, dtype=torch.float32, device=DEV)
    thr = torch.full((S,), 0.25, dtype=torch.float32, device=DEV)
    sp = _lib.stream_ptr()
    nbytes = _lib.nbytes(out)
    need = lib.cgnn_ingest_mst_workspace_bytes(S, n)
    assert nbytes == 4 * S * n * n and need == min(S, 2 * lib.cgnn_fused_grid()) * n * n * 4
    work = torch.full((need // 4,), -7.0, dtype=torch.float32, device=DEV)
    good = [_lib.ptr(dev), S, n, _lib.ptr(thr), _lib.ptr(work), need, _lib.ptr(out), nbytes, sp]

    def rc(at, v):
        return lib.cgnn_ingest_mst(*(good[:at] + [v] + good[at + 1:]))

    bad = {"matrices NULL": (0, None), "out NULL": (6, None), "workspace NULL": (4, None), "S < 0": (1, -1),
           "n = 0": (2, 0), "out_bytes one byte short": (7, nbytes - 1), "workspace_bytes one byte short": (5, need - 1),
           "S * n >= 2^31": (1, 2 ** 31 // n + 1), "matrices misaligned": (0, _lib.ptr(dev) + 2),
           "out misaligned": (6, _lib.ptr(out) + 1), "workspace misaligned": (4, _lib.ptr(work) + 4),
           "the workspace is the matrices": (4, _lib.ptr(dev)), "the workspace is out": (4, _lib.ptr(out)),
           "the thresholds lie in out": (3, _lib.ptr(out))}
    for name, (at, v) in bad.items():
        assert rc(at, v) == _lib.CGNN_EINVAL, name
    assert rc(2, 1025) == _lib.CGNN_EUNSUPPORTED
    # an output one subject into the matrices overlaps them without being them
    big = torch.full((S + 1, n, n), -7.0, dtype=torch.float32, device=DEV)
    for a, b in ((big, big[1:]), (big[1:], big)):
        assert lib.cgnn_ingest_mst(_lib.ptr(a), S, n, None, _lib.ptr(work), need, _lib.ptr(b), nbytes, sp) == _lib.CGNN_EINVAL
    assert rc(1, 0) == _lib.CGNN_OK                         # no subjects: nothing launched
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((big == -7.0).all()) and bool((work == -7.0).all())
    assert lib.cgnn_ingest_mst(*good) == _lib.CGNN_OK       # the documented sizes are accepted
    _assert_bits(out, M.host_backbone_cohort(mats, [0.25] * S), "the documented sizes")
    assert rc(3, None) == _lib.CGNN_OK                      # no thresholds: the tree alone
    _assert_bits(out, M.host_backbone_cohort(mats), "no thresholds")


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
            u, v = M.bits(u), M.bits(v)
        assert torch.equal(u, v), name


THRESHOLDS = (dict(), dict(keep=0.1), dict(num_edges=7), dict(min_weight=0.3))
KNNS = ((2, "union"), (8, "mutual"))


def _united(dev, choice):
    """The matrices that ``backbone="mst"`` with ``choice`` stands for: (the composition, the entry point's arguments)."""
    if "knn" in choice:
        sparse = ingest.knn_sparsify(dev, choice["knn"], mode=choice["knn_mode"])
        return torch.maximum(sparse, ingest.mst_backbone(dev))
    return ingest.mst_backbone(dev, **choice)


def _all_choices():
    return THRESHOLDS + tuple(dict(knn=k, knn_mode=mode) for k, mode in KNNS)


@pytest.mark.parametrize("n", [5, 84])
def test_from_matrices_is_the_composition(n):
    mats, dev = _cohort(n)
    S = mats.shape[0]
    x, y = D.features(S, n), D.labels(S)
    xd = x.to(DEV)
    for choice in _all_choices():
        B = _united(dev, choice)
        got = ingest.from_matrices(dev, y, backbone="mst", node_features=xd, **choice)
        _same_bits(got, ingest.from_matrices(B, y, min_weight=0.0, node_features=xd))
        if "knn" not in choice:                             # ... and the host statement's graphs
            host = M.host_backbone_cohort(mats, _host_thresholds(mats, **choice), M.forests(n))
            _same_dataset(got, RaggedPackedDataset.from_graphs(D.host_graphs(host, [0.0] * S, x, y)))
        else:
            host = torch.maximum(K.host_knn_cohort(mats, choice["knn"], choice["knn_mode"]),
                                 M.host_backbone_cohort(mats, None, M.forests(n)))
            _assert_bits(B, host, choice)
        got = ingest.from_matrices(dev, y, backbone="mst", **choice)   # the default strength feature is the united graph's
        assert got.x.shape == (S, n, 1)
        _same_bits(got, ingest.from_matrices(B, y, min_weight=0.0))
        plain = dict(choice) if choice else None
        if plain is not None:                               # at most 2 (n - 1) entries more than the choice alone
            alone = ingest.from_matrices(dev, y, **plain)
            more = (got.edge_ptr[1:] - got.edge_ptr[:-1]) - (alone.edge_ptr[1:] - alone.edge_ptr[:-1])
            assert int(more.min()) >= 0 and int(more.max()) <= 2 * (n - 1), choice
        assert torch.equal(M.bits(dev.cpu()), M.bits(mats)), "the caller's matrices are untouched"


@pytest.mark.parametrize("n", [5, 84])
def test_measures_paths_and_profiles_are_the_composition(n):
    mats, dev = _cohort(n)
    S = mats.shape[0]
    names = ingest.MEASURES + ingest.PATH_MEASURES + ingest.WEIGHTED_PATH_MEASURES
    modules = (torch.arange(n) * 3 // n).tolist()
    for choice in _all_choices():
        B = _united(dev, choice)
        got = ingest.node_measures(dev, backbone="mst", measures=names, **choice)
        want = ingest.node_measures(B, min_weight=0.0, measures=names)
        assert got.shape == (S, n, len(names)) and torch.equal(M.bits(got), M.bits(want)), choice
        got = ingest.path_lengths(dev, backbone="mst", **choice)
        assert torch.equal(M.bits(got), M.bits(ingest.path_lengths(B, min_weight=0.0))), choice
        got = ingest.module_profile(dev, modules, backbone="mst", **choice)
        assert torch.equal(M.bits(got), M.bits(ingest.module_profile(B, modules, min_weight=0.0))), choice
        ds = ingest.from_matrices(dev, D.labels(S), backbone="mst", measures=names, **choice)
        assert torch.equal(M.bits(ds.x), M.bits(want)), choice
        assert torch.equal(M.bits(dev.cpu()), M.bits(mats)), "the caller's matrices are untouched"


def test_from_timeseries_is_the_composition():
    ts = torch.randn(6, 40, 20, generator=torch.Generator().manual_seed(4)).to(DEV)
    y = D.labels(6)
    before = ts.clone()
    cm = ingest.correlation_matrices(ts)
    for choice in (dict(), dict(keep=0.2), dict(num_edges=30), dict(min_weight=0.1), dict(knn=3, knn_mode="union"),
                   dict(knn=5, knn_mode="mutual")):
        got = ingest.from_timeseries(ts, y, backbone="mst", **choice)
        B = _united(cm, choice)
        _same_bits(got, ingest.from_matrices(B, y, min_weight=0.0))
        if "knn" not in choice:
            host = cm.cpu()
            _assert_bits(B, M.host_backbone_cohort(host, _host_thresholds(host, **choice)), choice)
    got = ingest.from_timeseries(ts, y, keep=0.2, backbone="mst", window=20, stride=10, absolute=True)   # 3 windows each
    B = ingest.mst_backbone(ingest.correlation_matrices(ts, window=20, stride=10, absolute=True), keep=0.2)
    _same_bits(got, ingest.from_matrices(B, y.repeat_interleave(3), min_weight=0.0))
    assert torch.equal(ts, before)


def _components_of(ds, s, n):
    lo, hi = int(ds.edge_ptr[s]), int(ds.edge_ptr[s + 1])
    ei = ds.edge_local[:, lo:hi].cpu()
    adj = torch.zeros(n, n, dtype=torch.bool)
    adj[ei[0], ei[1]] = True
    return int(connected_components(adj.numpy(), directed=False)[0]), hi - lo


def test_the_backbone_connects_what_a_threshold_and_knn_leave_apart():
    """The point of the feature, on ``modular(84, 4)``: 4 components at keep = 0.10 (696 entries) and at knn = 8 (772),
    one component with the tree added, at six entries more.  Components are counted from ``edge_local`` on the host and
    asserted next to the host statement's."""
    n = 84
    A = M.modular(n, 4)
    dev, y = A[None].contiguous().to(DEV), D.labels(1)
    F = M.host_forest(A)
    none = torch.zeros(n, n, dtype=torch.bool)
    t = D.host_threshold(A, D.rank_of(n, keep=0.10))
    knn = K.host_kept(A, 8, "union")
    host = {("keep", False): M.host_kept(A, t, none), ("keep", True): M.host_kept(A, t, F),
            ("knn", False): knn, ("knn", True): knn | M.host_kept(A, INF, F)}
    figures = {("keep", False): (4, 696), ("keep", True): (1, 702), ("knn", False): (4, 772), ("knn", True): (1, 778)}
    for (kind, tree), want in figures.items():
        choice = dict(keep=0.10) if kind == "keep" else dict(knn=8)
        ds = ingest.from_matrices(dev, y, backbone="mst" if tree else None, **choice)
        mask = host[(kind, tree)]
        assert (int(connected_components(mask.numpy(), directed=False)[0]), int(mask.sum())) == want
        assert _components_of(ds, 0, n) == want, (kind, tree)
        assert torch.equal(ds.edge_local.cpu(), torch.nonzero(mask).t())
    ecc = ingest.node_measures(dev, keep=0.10, backbone="mst", measures=("eccentricity",))
    assert ecc.shape == (1, n, 1) and bool(torch.isfinite(ecc).all()) and bool((ecc > 0).all())
    apart = ingest.node_measures(dev, keep=0.10, measures=("nodal_efficiency",))
    joined = ingest.node_measures(dev, keep=0.10, backbone="mst", measures=("nodal_efficiency",))
    assert bool((joined > apart).all()), "every node reaches the other modules"


def test_backbone_through_loader_and_trainer():
    """12 subjects x 84 nodes, keep = 0.10 with the backbone, the default strength feature: one epoch of a hidden-64 GCN
    over ResidentDataLoader(structure_cache=True) with captured steps runs on the fused path and its loss is finite."""
    S, n = 12, 84
    mats = torch.stack([M.modular(n, 4, seed=20 + s) for s in range(S)]).contiguous()
    y = D.labels(S)
    ds = ingest.from_matrices(mats.to(DEV), y, keep=0.10, backbone="mst")
    assert ds.x.shape == (S, n, 1)
    assert all(_components_of(ds, s, n)[0] == 1 for s in range(S))
    torch.manual_seed(3)
    m = C.GCNConnectome(1, 64, dropout=0.0)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
    tr = C.Trainer(m, opt, device=DEV, graph=True)
    ld = ResidentDataLoader(ds, 4, shuffle=True, structure_cache=True)
    vl = ResidentDataLoader(ds, 4, shuffle=False, structure_cache=True)
    hist = tr.fit(ld, vl, num_epochs=1, patience=10, verbose=False)
    assert tr.model.impl_used == "fused"
    assert len(hist["train_loss"]) == 1 and all(torch.isfinite(torch.tensor(v)).all() for v in hist.values())
