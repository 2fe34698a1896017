"""connectome_gnn_amd.ingest.group_matrix / group_sparsify on the device (csrc/group.hip) against their host statement
(tests/group_data.py): the three statistics at every size and slice count, ``among``, the grid, the mask for every edge
choice, in place and out of place, the C ABI's refusals, ``group=`` of the six entry points as the composition it stands
for, the common topology it exists for, and the result served through ResidentDataLoader + Trainer.  Bits are compared
unless a test says otherwise."""
import functools

import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib, ingest
from connectome_gnn_amd.resident import ResidentDataLoader
from connectome_gnn_amd.synthetic import RaggedPackedDataset
from tests import group_data as G
from tests import ingest_data as D
from tests import knn_data as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
UNITS = (1, 2, 3, G.SLICE - 1, G.SLICE, G.SLICE + 1, 2 * G.SLICE + 5)
SIZES = (1, 2, 3, 5, 63, 64, 65, 84)
CHOICES = (dict(keep=0.1), dict(num_edges=40), dict(min_weight=0.2), dict(knn=3), dict(knn=3, knn_mode="mutual"),
           dict(knn=2, knn_mode="directed"), dict(backbone="mst"), dict(keep=0.1, backbone="mst"),
           dict(num_edges=40, backbone="mst"), dict(min_weight=0.2, backbone="mst"), dict(knn=3, backbone="mst"))


def _nan_like(t):
    return torch.full_like(t, NAN)


def _same(got, want, what=None):
    """a device tensor and a host tensor, bit for bit"""
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == want.shape, what
    bad = torch.nonzero(K.bits(got.cpu()) != K.bits(want))
    assert bad.numel() == 0, (what, bad.shape[0], bad[:4].tolist())


def _fisher_close(got, want64, what=None):
    """|got - v| <= 2^-24 |v| + 2^-40 against the unrounded fp64 statement ``v``: one rounding to fp32, and an absolute
    term for a device and a host atanh / tanh that differ by a few fp64 ulp (|atanh| <= 8.7 for an fp32 |r| < 1 and tanh
    contracts: below 2^-47).  The NaN pattern and the exact +-1 are the host's."""
    got = got.cpu().double()
    nan = torch.isnan(want64)
    assert torch.equal(torch.isnan(got), nan), what
    assert torch.equal(got.abs() == 1, want64.float().abs() == 1) and torch.equal(got == 1, want64.float() == 1), what
    ok = ~nan
    err, bound = (got[ok] - want64[ok]).abs(), 2.0 ** -24 * want64[ok].abs() + 2.0 ** -40
    print(what, "fisher_mean: largest error / bound", float((err / bound).max()) if err.numel() else 0.0)
    assert bool((err <= bound).all()), (what, float((err / bound).max()))


def _consistency_choices(S):
    return (dict(keep=0.3), dict(num_edges=5), dict(min_weight=torch.linspace(-0.25, 0.75, S)))


def _check_statistics(S, n):
    mats = G.cohort(S, n)
    dev = mats.to(DEV)
    _same(ingest.group_matrix(dev), G.host_group(mats, "mean"), ("mean", S, n))
    for choice in _consistency_choices(S):
        on_dev = {k: v.to(DEV) if isinstance(v, torch.Tensor) else v for k, v in choice.items()}
        thr = G.host_unit_thresholds(mats, **choice)
        _same(ingest.group_matrix(dev, "consistency", **on_dev), G.host_group(mats, "consistency", thr),
              ("consistency", S, n, sorted(choice)))
    for cohort in (mats, G.correlations(S, n)):
        got = ingest.group_matrix(cohort.to(DEV), "fisher_mean")
        _fisher_close(got, G.host_group(cohort, "fisher_mean", exact=True), ("fisher_mean", S, n))
    assert torch.equal(K.bits(dev.cpu()), K.bits(mats)), "the caller's matrices are untouched"


@pytest.mark.parametrize("n", SIZES)
def test_the_statistics_equal_the_host_statement(n):
    for S in UNITS:
        _check_statistics(S, n)


@pytest.mark.parametrize("S,n", [(8, 360), (3, 1025)])
def test_the_statistics_on_wide_matrices(S, n):
    _check_statistics(S, n)


def test_a_symmetric_cohort_gives_a_symmetric_group_matrix():
    dev = G.correlations(G.SLICE + 1, 65).to(DEV)
    for stat, kw in (("mean", {}), ("fisher_mean", {}), ("consistency", dict(keep=0.2))):
        g = ingest.group_matrix(dev, stat, **kw)
        assert torch.equal(K.bits(g), K.bits(g.t().contiguous())), stat


@pytest.mark.parametrize("S,n", [(5, 5), (2 * G.SLICE + 5, 65)])
def test_among(S, n):
    mats = G.cohort(S, n)
    dev = mats.to(DEV)
    every = torch.ones(S, dtype=torch.bool, device=DEV)
    half = (torch.arange(S) % 2 == 0)
    ragged = torch.rand(S, generator=torch.Generator().manual_seed(S)) < 0.7
    poisoned = mats.clone()
    poisoned[~half] = torch.tensor([NAN, INF, 1e30, -INF, -1e30] * n)[:n]
    for stat, kw in (("mean", {}), ("fisher_mean", {}), ("consistency", dict(keep=0.3)),
                     ("consistency", dict(min_weight=torch.linspace(-0.25, 0.75, S).to(DEV)))):
        plain = ingest.group_matrix(dev, stat, **kw)
        assert torch.equal(K.bits(ingest.group_matrix(dev, stat, among=every, **kw)), K.bits(plain)), stat
        got = ingest.group_matrix(dev, stat, among=half.to(DEV), **kw)
        assert torch.equal(K.bits(ingest.group_matrix(poisoned.to(DEV), stat, among=half.to(DEV), **kw)), K.bits(got)), \
            (stat, "a unit left out is never looked at")
        assert bool(torch.isnan(ingest.group_matrix(dev, stat, among=~every, **kw)).all()), (stat, "no units: all NaN")
        if stat == "fisher_mean":
            continue
        host_kw = {k: v.cpu() if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
        thr = G.host_unit_thresholds(mats, **host_kw) if kw else None
        for among in (half, ragged):
            _same(ingest.group_matrix(dev, stat, among=among.to(DEV), **kw), G.host_group(mats, stat, thr, among),
                  (stat, S, n))
    ds = ingest.from_matrices(dev, D.labels(S), keep=0.2,
                              group=ingest.group_matrix(dev, among=torch.zeros(S, dtype=torch.bool, device=DEV)))
    assert int(ds.edge_ptr[-1]) == 0 and ds.edge_local.shape == (2, 0), "an all-NaN group matrix has no edges"


def test_every_grid_gives_the_same_bits():
    """300 subjects on 24 workgroups, then on the default grid: the statistic and the mask."""
    S, n = 300, 84
    mats = G.cohort(S, n)
    dev = mats.to(DEV)
    among = (torch.arange(S) % 3 != 0).to(DEV)
    grp = G.host_group(mats[:12], "mean").nan_to_num(0.0, 0.0, 0.0).contiguous().to(DEV)

    def run():
        return [ingest.group_matrix(dev), ingest.group_matrix(dev, "fisher_mean"),
                ingest.group_matrix(dev, "consistency", keep=0.1), ingest.group_matrix(dev, among=among),
                ingest.group_sparsify(dev, grp, keep=0.1, out=_nan_like(dev))]

    lib = _lib.load()
    try:
        assert lib.cgnn_set_fused_grid(3) == _lib.CGNN_OK
        few = run()
    finally:
        lib.cgnn_set_fused_grid(0)
    full = run()
    for a, b in zip(few, full):
        assert torch.equal(K.bits(a), K.bits(b))
    _same(full[0], G.host_group(mats, "mean"))
    _same(full[2], G.host_group(mats, "consistency", G.host_unit_thresholds(mats, keep=0.1)))
    _same(full[3], G.host_group(mats, "mean", among=among.cpu()))
    _same(full[4], G.host_mask(mats, G.host_edge_set(grp.cpu(), keep=0.1)))


@functools.lru_cache(maxsize=None)
def _mask_case(n):
    """(mats, a finite group matrix): the recipe cohort of 9 units and the symmetric mean of a correlation cohort"""
    return G.cohort(9, n), G.host_group(G.correlations(7, n), "mean")


@pytest.mark.parametrize("n", [5, 65, 84])
def test_the_mask_equals_the_host_statement_for_every_edge_choice(n):
    mats, grp = _mask_case(n)
    dev, grp_dev = mats.to(DEV), grp.to(DEV)
    mean = G.host_group(mats, "mean")                       # NaN and +-inf entries included
    for choice in CHOICES:
        for group, host in ((grp_dev, grp), ("mean", mean)):
            want = G.host_mask(mats, G.host_edge_set(host, **choice))
            out = _nan_like(dev)
            got = ingest.group_sparsify(dev, group, out=out, **choice)
            assert got is out
            _same(got, want, (choice, isinstance(group, str)))
    got = ingest.group_sparsify(dev, keep=0.1)              # the defaults: "mean", a new tensor
    assert got.data_ptr() != dev.data_ptr()
    _same(got, G.host_mask(mats, G.host_edge_set(mean, keep=0.1)))
    one = torch.tensor([0.2])
    _same(ingest.group_sparsify(dev, grp_dev, min_weight=one.to(DEV)), G.host_mask(mats, G.host_edge_set(grp, min_weight=one)))
    assert torch.equal(K.bits(dev.cpu()), K.bits(mats)), "the caller's matrices are untouched"


@pytest.mark.parametrize("S,n", [(1, 1025), (G.SLICE + 3, 65), (3, 33), (3, 45), (3, 55), (3, 64), (3, 75), (3, 90), (3, 91)])
def test_the_mask_past_one_block_and_one_slice(S, n):
    """A unit of 2, 3, 4, 6 and 8 blocks of 1024 entries is one work item of as many loads a lane (5 and 7: n = 65 and 84),
    91 nodes are the first to be cut into spans of 4 blocks, 1025 nodes take 257 spans and end in a short quad."""
    mats = G.cohort(S, n)
    grp = G.host_group(G.correlations(3, n), "mean")
    want = G.host_mask(mats, G.host_edge_set(grp, keep=0.2))
    _same(ingest.group_sparsify(mats.to(DEV), grp.to(DEV), keep=0.2), want)


@pytest.mark.parametrize("n", [5, 65])
def test_in_place_and_repeated_calls_give_the_same_bits(n):
    mats, grp = _mask_case(n)
    dev, grp_dev = mats.to(DEV), grp.to(DEV)
    for choice in (dict(keep=0.1), dict(knn=3), dict(keep=0.1, backbone="mst")):
        for group in (grp_dev, "mean"):
            first = ingest.group_sparsify(dev, group, out=_nan_like(dev), **choice)
            again = ingest.group_sparsify(dev, group, **choice)
            work = dev.clone()
            same = ingest.group_sparsify(work, group, out=work, **choice)
            assert same is work
            assert torch.equal(K.bits(again), K.bits(first)) and torch.equal(K.bits(work), K.bits(first)), choice
    assert torch.equal(K.bits(dev.cpu()), K.bits(mats))


def test_what_is_not_a_positive_entry_at_a_group_edge_becomes_plus_zero():
    n = 5
    mats = G.cohort(9, n).clone()
    mats[0, 2, 3] = -0.0
    mats[1, 2, 3] = NAN
    mats[2, 2, 3] = -INF
    grp = torch.full((n, n), 0.5)
    grp[0, 1] = NAN
    grp[4, 3] = -0.5
    out = ingest.group_sparsify(mats.to(DEV), grp.to(DEV), min_weight=0.0).cpu()
    _same(out.to(DEV), G.host_mask(mats, G.host_edge_set(grp, min_weight=0.0)))
    assert [int(K.bits(out)[s, 2, 3]) for s in range(3)] == [0, 0, 0]
    assert not bool(torch.isnan(out).any()) and not out[:, torch.arange(n), torch.arange(n)].any()
    assert not out[:, 0, 1].any() and not out[:, 4, 3].any(), "a NaN or negative group entry is never an edge"
    assert int(K.bits(out)[5, 1, 2]) == int(K.bits(mats)[5, 1, 2]) != 0 and float(out[5, 1, 2]) < 1e-38, "the subnormal"
    assert float(out[5, 3, 0]) == INF


def test_the_abi_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    n = 20
    mats = G.cohort(G.SLICE + 2, n)
    S = mats.shape[0]
    dev = mats.to(DEV)
    sp = _lib.stream_ptr()
    fill = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device=DEV)
    # the statistic
    out, thr = fill(n, n), torch.zeros(S, dtype=torch.float32, device=DEV)
    among = torch.ones(S, dtype=torch.bool, device=DEV)
    need = lib.cgnn_ingest_group_workspace_bytes(S, n)
    assert need == (2 * n * n + 2) * 8
    work = torch.full((need // 4,), -7.0, dtype=torch.float32, device=DEV)
    good = [dev, S, n, _lib.GROUP_MEAN, None, among, work, need, out, 4 * n * n, sp]

    def rc(at, v, base=good):
        return lib.cgnn_ingest_group(*(base[:at] + [v] + base[at + 1:]))

    bad = {"matrices NULL": (0, None), "out NULL": (8, None), "workspace NULL": (6, None), "S < 0": (1, -1),
           "n = 0": (2, 0), "statistic 3": (3, 3), "statistic -1": (3, -1), "thr with the mean": (4, thr),
           "out_bytes one byte short": (9, 4 * n * n - 1), "workspace_bytes short": (7, need - 1),
           "S * n >= 2^31": (1, 2 ** 31 // n + 1), "matrices misaligned": (0, _lib.ptr(dev) + 2),
           "workspace misaligned": (6, _lib.ptr(work) + 8), "out inside the matrices": (8, _lib.ptr(dev) + 4 * n * n),
           "out inside the workspace": (8, _lib.ptr(work) + 64), "among inside out": (5, _lib.ptr(out) + 4)}
    for name, (at, v) in bad.items():
        assert rc(at, v) == _lib.CGNN_EINVAL, name
    consistency = good[:3] + [_lib.GROUP_CONSISTENCY, thr] + good[5:]
    assert rc(4, None, consistency) == _lib.CGNN_EINVAL, "the consistency without thresholds"
    assert rc(4, out, consistency) == _lib.CGNN_EINVAL, "thr inside out"
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((work == -7.0).all())
    for stat, base in ((_lib.GROUP_MEAN, good), (_lib.GROUP_FISHER_MEAN, good), (_lib.GROUP_CONSISTENCY, consistency)):
        assert rc(3, stat, base) == _lib.CGNN_OK            # the documented sizes are accepted
    _same(out, G.host_group(mats, "consistency", [0.0] * S))
    empty = fill(n, n)
    assert lib.cgnn_ingest_group(None, 0, n, _lib.GROUP_MEAN, None, None, None, 0, empty, 4 * n * n, sp) == _lib.CGNN_OK
    assert bool(torch.isnan(empty).all()), "the statistic of no units is the all-NaN matrix"
    # the mask
    out, grp, one = fill(S, n, n), torch.full((n, n), 0.5, device=DEV), torch.zeros(1, device=DEV)
    nbytes = _lib.nbytes(out)
    good = [dev, S, n, grp, one, out, nbytes, sp]

    def rcm(at, v):
        return lib.cgnn_ingest_group_mask(*(good[:at] + [v] + good[at + 1:]))

    bad = {"matrices NULL": (0, None), "group NULL": (3, None), "thr NULL": (4, None), "out NULL": (5, None),
           "S < 0": (1, -1), "n = 0": (2, 0), "out_bytes one byte short": (6, nbytes - 1),
           "S * n >= 2^31": (1, 2 ** 31 // n + 1), "group misaligned": (3, _lib.ptr(grp) + 2),
           "group inside out": (3, _lib.ptr(out) + 4 * n * n), "thr inside out": (4, _lib.ptr(out) + nbytes - 4)}
    for name, (at, v) in bad.items():
        assert rcm(at, v) == _lib.CGNN_EINVAL, name
    big = fill(S + 1, n, n)                                 # an output one subject into the matrices overlaps them
    assert lib.cgnn_ingest_group_mask(big, S, n, grp, one, big[1:], nbytes, sp) == _lib.CGNN_EINVAL
    assert lib.cgnn_ingest_group_mask(big[1:], S, n, grp, one, big, nbytes, sp) == _lib.CGNN_EINVAL
    assert rcm(1, 0) == _lib.CGNN_OK                        # no subjects: nothing launched
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((big == -7.0).all())
    assert lib.cgnn_ingest_group_mask(*good) == _lib.CGNN_OK
    _same(out, G.host_mask(mats, G.host_edge_set(grp.cpu(), min_weight=0.0)))


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


def _groups(dev):
    """the three kinds of ``group=``: the two names and a tensor (the consistency of the even units)"""
    among = (torch.arange(dev.shape[0]) % 2 == 0).to(DEV)
    return ("mean", "fisher_mean", ingest.group_matrix(dev, "consistency", among=among, keep=0.3))


@pytest.mark.parametrize("n", [5, 84])
def test_from_matrices_is_the_composition(n):
    mats = G.correlations(10, n)
    dev = mats.to(DEV)
    S = mats.shape[0]
    x, y = D.features(S, n), D.labels(S)
    xd = x.to(DEV)
    for group in _groups(dev):
        for choice in (dict(keep=0.1), dict(num_edges=7), dict(min_weight=0.1), dict(knn=3, knn_mode="mutual"),
                       dict(keep=0.1, backbone="mst")):
            masked = ingest.group_sparsify(dev, group, **choice)
            got = ingest.from_matrices(dev, y, group=group, node_features=xd, **choice)
            _same_bits(got, ingest.from_matrices(masked, y, min_weight=0.0, node_features=xd))
            want = RaggedPackedDataset.from_graphs(D.host_graphs(masked.cpu(), [0.0] * S, x, y))
            _same_dataset(got, want)
            got = ingest.from_matrices(dev, y, group=group, **choice)      # the default strength feature
            _same_bits(got, ingest.from_matrices(masked, y, min_weight=0.0))
            if not isinstance(group, str) or group == "mean":               # (bit-exact group matrices on the host)
                host = group.cpu() if not isinstance(group, str) else G.host_group(mats, "mean")
                B = G.host_mask(mats, G.host_edge_set(host, **choice))
                _same_dataset(ingest.from_matrices(dev, y, group=group, node_features=xd, **choice),
                              RaggedPackedDataset.from_graphs(D.host_graphs(B, [0.0] * S, x, y)))
    assert torch.equal(K.bits(dev.cpu()), K.bits(mats)), "the caller's matrices are untouched"


@pytest.mark.parametrize("n", [5, 84])
def test_the_measure_calls_are_the_composition(n):
    mats = G.correlations(10, n)
    dev = mats.to(DEV)
    names = ingest.MEASURES + ingest.PATH_MEASURES + ingest.WEIGHTED_PATH_MEASURES
    modules = (torch.arange(n) * 4 // n).tolist() if n >= 4 else [0] * n
    for group in _groups(dev):
        for choice in (dict(keep=0.2), dict(knn=3), dict(min_weight=0.05, backbone="mst")):
            masked = ingest.group_sparsify(dev, group, **choice)
            for call, kw in ((ingest.node_measures, dict(measures=names)), (ingest.path_lengths, {}),
                             (ingest.centrality_measures, dict(damping=0.8)),
                             (lambda m, **k: ingest.module_profile(m, modules, **k), dict(normalize=True))):
                got = call(dev, group=group, **choice, **kw)
                want = call(masked, min_weight=0.0, **kw)
                assert got.shape == want.shape and torch.equal(K.bits(got), K.bits(want)), (choice, kw)
    assert torch.equal(K.bits(dev.cpu()), K.bits(mats)), "the caller's matrices are untouched"


def test_from_timeseries_is_the_composition():
    ts = torch.randn(6, 40, 20, generator=torch.Generator().manual_seed(4)).to(DEV)
    y = D.labels(6)
    before = ts.clone()
    windows = dict(window=20, stride=10)                    # 3 windows a subject: the units are the windows
    c = ingest.correlation_matrices(ts, **windows)
    for group in ("mean", "fisher_mean", ingest.group_matrix(c[::2].contiguous())):
        for choice in (dict(keep=0.2), dict(knn=4), dict(keep=0.1, backbone="mst")):
            got = ingest.from_timeseries(ts, y, group=group, **windows, **choice)
            masked = ingest.group_sparsify(c, group, **choice)
            _same_bits(got, ingest.from_matrices(masked, y.repeat_interleave(3), min_weight=0.0))
            assert got.x.shape[0] == 18
    got = ingest.from_timeseries(ts, y, group="mean", keep=0.2, absolute=True)      # one unit a subject
    masked = ingest.group_sparsify(ingest.correlation_matrices(ts, absolute=True), "mean", keep=0.2)
    _same_bits(got, ingest.from_matrices(masked, y, min_weight=0.0))
    assert torch.equal(ts, before)


def test_every_subject_carries_the_common_topology():
    n, S = 84, 12
    g = torch.Generator().manual_seed(9)
    R = 0.05 + torch.rand(S, n, n, generator=g)
    positive = ((R + R.transpose(1, 2)) / 2).contiguous()
    ds = ingest.from_matrices(positive.to(DEV), D.labels(S), group="mean", keep=0.1)
    counts = ds.edge_ptr[1:] - ds.edge_ptr[:-1]
    assert int(counts.min()) == int(counts.max()) == 696
    runs = ds.edge_local.cpu().reshape(2, S, 696)
    assert bool((runs == runs[:, :1]).all()), "the same edge_local run for every subject"
    # signed matrices: a subject drops the group edges at which it is not positive
    mats = G.modular_series_cohort()
    dev = mats.to(DEV)
    E = G.host_edge_set(G.host_group(mats, "mean"), keep=0.1)
    ds = ingest.from_matrices(dev, D.labels(S), group="mean", keep=0.1)
    counts = ds.edge_ptr[1:] - ds.edge_ptr[:-1]
    assert int(E.sum()) == 696 and 694 <= int(counts.min()) and int(counts.max()) <= 696
    for s in range(S):
        ei = ds.edge_local[:, int(ds.edge_ptr[s]):int(ds.edge_ptr[s + 1])].cpu()
        assert bool(E[ei[0], ei[1]].all()), s
    recipe = G.cohort(9, n)
    E = G.host_edge_set(G.host_group(recipe, "mean"), keep=0.1)
    ds = ingest.from_matrices(recipe.to(DEV), D.labels(9), group="mean", keep=0.1)
    for s in range(9):
        ei = ds.edge_local[:, int(ds.edge_ptr[s]):int(ds.edge_ptr[s + 1])].cpu()
        assert bool(E[ei[0], ei[1]].all()), s


def test_group_through_loader_and_trainer():
    """12 subjects x 84 nodes, group="mean" at keep = 0.1, the default strength feature: one epoch of a hidden-64 GCN
    over ResidentDataLoader(structure_cache=True) with captured steps runs on the fused path and its loss is finite."""
    S, n = 12, 84
    ds = ingest.from_matrices(G.modular_series_cohort().to(DEV), D.labels(S), group="mean", keep=0.1)
    assert ds.x.shape == (S, n, 1) and int((ds.edge_ptr[1:] - ds.edge_ptr[:-1]).min()) >= 694
    torch.manual_seed(3)
    m = C.GCNConnectome(1, 64, dropout=0.0)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
    tr = C.Trainer(m, opt, device=DEV, graph=True)
    ld = ResidentDataLoader(ds, 4, shuffle=True, structure_cache=True)
    vl = ResidentDataLoader(ds, 4, shuffle=False, structure_cache=True)
    hist = tr.fit(ld, vl, num_epochs=1, patience=10, verbose=False)
    assert tr.model.impl_used == "fused"
    assert len(hist["train_loss"]) == 1 and all(torch.isfinite(torch.tensor(v)).all() for v in hist.values())
