"""The shortest-path node measures of connectome_gnn_amd.ingest on the device (csrc/paths.hip) against the fp64 host
statement (tests/paths_data.py), on the recipe subjects of tests/ingest_data.py and on structured graphs.

Bounds, none of them taken from what the kernel gives:

* ``eccentricity`` is the correctly rounded fp32 quotient ``ecc_i / (n - 1)`` of two exact integers (bit-equal to the
  host's), and ``round(eccentricity * (n - 1))`` in fp64 is ``ecc_i`` exactly.
* ``nodal_efficiency``, ``closeness`` and ``local_efficiency`` are within ``2^-22`` relative of the fp64 statement: one
  fp32 rounding is ``2^-24``; the factor 4 allows the last quotient to be formed in fp32 from a rounded fp64 sum.
* Exact zeros where the statement is 0.

The measured maximum is printed per shape.
"""
import ctypes
import functools

import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib, ingest
from connectome_gnn_amd.resident import ResidentDataLoader
from tests import ingest_data as I
from tests import measures_data as M
from tests import paths_data as P
from tests import timeseries_data as TS
from tests.cohort_kit import DEV, bits as _bits, grid_of_three

pytestmark = pytest.mark.gpu
BOUND = 2.0 ** -22
SIZES = [1, 2, 3, 5, 20, 31, 32, 33, 63, 64, 65, 84, 96, 97, 130, 360]
# keep 1.0 at 84 and 97: neighbourhoods of 65 .. 128 nodes (two words a row once renumbered); at 130: beyond 128 as well
CASES = [(n, 0.1) for n in SIZES] + [(n, keep) for keep in (0.5, 1.0) for n in (84, 97)] + [(130, 1.0)]
MIN_WEIGHT = (0.3, 0.5, 0.0, 0.7, -1.0, 0.6)          # the per-subject min_weight= case of test_gpu_measures.py
COL = {name: c for c, name in enumerate(P.PATH_MEASURES)}
NINE = M.MEASURES + P.PATH_MEASURES


def _check(mats, thr, got, what, local_nodes=None):
    """`got` [S, n, 4] float32 (host) against the statement of every subject."""
    n = mats.shape[1]
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(mats), n, 4), what
    worst = 0.0
    for s, (A, t) in enumerate(zip(mats, thr)):
        mask = M.kept_mask(A, float(t))
        want = P.mask_measures(mask, local_nodes=local_nodes)
        _, _, ecc = P.exact_integers(P.distances(mask))
        ecc = torch.from_numpy(ecc)
        e = got[s, :, COL["eccentricity"]]
        assert torch.equal(_bits(e), _bits(ecc.float() / (n - 1) if n > 1 else torch.zeros(n))), (what, s)
        assert torch.equal(torch.round(e.double() * (n - 1)).long(), ecc if n > 1 else torch.zeros_like(ecc)), (what, s)
        for name in ("nodal_efficiency", "closeness", "local_efficiency"):
            g, w = got[s, :, COL[name]].double(), want[:, COL[name]]
            sel = ~torch.isnan(w)                         # (a sampled local efficiency)
            g, w = g[sel], w[sel]
            assert torch.equal(g[w == 0], w[w == 0]), (what, s, name, "exact zeros")
            rel = float(((g - w).abs() / w.clamp_min(1e-300)).max()) if g.numel() else 0.0
            worst = max(worst, rel)
            assert bool(((g - w).abs() <= BOUND * w).all()), (what, s, name, rel)
        assert float(got[s].min()) >= 0.0 and float(got[s].max()) <= 1.0, (what, s)
        if not mask.any():
            assert torch.equal(got[s], torch.zeros(n, 4)), (what, s, "a subject without edges")
    print(f"{what}: max relative error {worst:.3e}, bound {BOUND:.3e}")


def _paths(dev, **kw):
    return ingest.node_measures(dev, measures=P.PATH_MEASURES, **kw)


@functools.lru_cache(maxsize=None)
def _got(n, keep):
    return _paths(P.recipe(n).to(DEV), keep=keep).cpu()


@functools.lru_cache(maxsize=None)
def _classic(n, keep):
    return ingest.node_measures(P.recipe(n).to(DEV), keep=keep).cpu()


def _thresholds(mats, keep):
    return [P.host_threshold(A, P.rank_of(mats.shape[1], keep=keep)) for A in mats]


@pytest.mark.parametrize("n,keep", CASES)
def test_parity_with_the_fp64_statement(n, keep):
    mats = P.recipe(n)
    thr = _thresholds(mats, keep)
    if (n, keep) in ((20, 0.1), (84, 0.1)):               # both kinds of subject occur
        holes = [P.unreachable_pairs(mats[s], thr[s]) for s in (0, 3, 4, 5)]
        assert all(140 <= h <= 173 for h in holes) if n == 20 else holes == [0, 0, 0, 0]
    _check(mats, thr, _got(n, keep), f"n={n} keep={keep}")


def test_parity_at_per_subject_min_weight():
    mats = P.recipe(84)
    got = _paths(mats.to(DEV), min_weight=torch.tensor(MIN_WEIGHT, device=DEV)).cpu()
    _check(mats, list(MIN_WEIGHT), got, "n=84 min_weight=[S]")


@pytest.mark.parametrize("n", [5, 64, 65, 129, 130])          # complete: neighbourhoods of 63, 64, 128 and 129 nodes
def test_parity_on_structured_graphs(n):
    mats = P.structured_cohort(n)
    got = _paths(mats.to(DEV), min_weight=0.0).cpu()
    _check(mats, [0.0] * len(mats), got, f"structured n={n}")
    ring, dpath, path = (P.STRUCTURED.index(k) for k in ("ring", "directed_path", "path"))
    nm1 = float(n - 1)
    assert torch.equal(got[ring, :, COL["eccentricity"]], torch.full((n,), (n // 2) / nm1))
    assert torch.equal(got[dpath, :, COL["eccentricity"]], (n - 1 - torch.arange(n)).float() / nm1)
    assert got[dpath, n - 1].tolist() == [0.0, 0.0, 0.0, 0.0], "the last node reaches nothing"
    assert float(got[path, :, COL["eccentricity"]].max()) == 1.0, "diameter n - 1"


def test_1024_nodes_and_the_limit():
    """The largest n: ring (diameter 512) and undirected path (diameter 1023, sum d at its maximum n (n - 1) / 2)."""
    n = 1024
    mats = torch.stack([P.structured("ring", n), P.structured("path", n)]).contiguous()
    got = _paths(mats.to(DEV), min_weight=0.0).cpu()
    _check(mats, [0.0, 0.0], got, "n=1024 ring, path", local_nodes=(0, 1, 63, 64, 511, 1022, 1023))
    assert torch.equal(got[:, :, COL["local_efficiency"]], torch.zeros(2, n)), "no two neighbours are adjacent"
    assert float(got[1, 0, COL["eccentricity"]]) == 1.0
    # a denser graph at the limit, local efficiency on a sample of nodes
    ws = P.structured("watts_strogatz", n).unsqueeze(0).contiguous()
    _check(ws, [0.0], _paths(ws.to(DEV), min_weight=0.0).cpu(), "n=1024 watts-strogatz", local_nodes=range(0, n, 97))
    big = torch.zeros(1, 1025, 1025, device=DEV)
    with pytest.raises(ValueError, match="n <= 1024"):
        _paths(big, keep=0.1)
    assert tuple(ingest.node_measures(big, keep=0.1, measures=("degree",)).shape) == (1, 1025, 1)


@pytest.mark.parametrize("n", [33, 130])
def test_any_subset_in_any_order_is_the_columns_of_the_two_full_calls(n):
    dev = P.recipe(n).to(DEV)
    full = torch.cat([_classic(n, 0.1), _got(n, 0.1)], 2)
    col = {name: c for c, name in enumerate(NINE)}
    for names in (("local_efficiency",), ("eccentricity",), ("closeness", "nodal_efficiency"), P.PATH_MEASURES[::-1],
                  ("eccentricity", "local_efficiency", "closeness"), NINE, NINE[::-1],
                  ("closeness", "degree"), ("clustering", "local_efficiency", "strength", "nodal_efficiency"),
                  ("degree", "weighted_clustering", "eccentricity", "mean_weight", "closeness", "strength",
                   "local_efficiency", "clustering"), ("weighted_clustering", "degree"), M.MEASURES):
        got = ingest.node_measures(dev, keep=0.1, measures=names).cpu()
        assert tuple(got.shape) == (6, n, len(names))
        assert torch.equal(_bits(got), _bits(full[:, :, [col[m] for m in names]])), names
    got = ingest.node_measures(dev, num_edges=P.rank_of(n, keep=0.1), measures=NINE).cpu()
    assert torch.equal(_bits(got), _bits(full))


def test_a_classic_request_gives_the_bits_of_cgnn_ingest_measures():
    n, S = 84, 6
    dev = P.recipe(n).to(DEV)
    lib = _lib.load()
    thr = ingest.select_thresholds(dev, keep=0.1)
    for names in (M.MEASURES, ("clustering", "strength")):
        ids = (ctypes.c_int32 * len(names))(*[M.MEASURES.index(m) for m in names])
        need = lib.cgnn_ingest_measures_workspace_bytes(S, n, ids, len(names))
        work = torch.empty(need, dtype=torch.uint8, device=DEV)
        x = torch.empty(S, n, len(names), device=DEV)
        assert lib.cgnn_ingest_measures(_lib.ptr(dev), S, n, _lib.ptr(thr), ids, len(names), _lib.ptr(work), need,
                                        _lib.ptr(x), _lib.nbytes(x), _lib.stream_ptr()) == _lib.CGNN_OK
        assert torch.equal(_bits(ingest.node_measures(dev, keep=0.1, measures=names)), _bits(x)), names
    assert torch.equal(_bits(ingest.node_measures(dev, keep=0.1).cpu()), _bits(_classic(n, 0.1)))


@pytest.mark.parametrize("n", [5, 97])
def test_subjects_without_edges_give_zeros(n):
    dev = P.recipe(n).to(DEV)
    assert torch.equal(_paths(dev, keep=0.0).cpu(), torch.zeros(6, n, 4))
    assert torch.equal(_got(n, 0.1)[2], torch.zeros(n, 4)), "the all-zero subject"
    assert torch.equal(_paths(dev, min_weight=float("inf")).cpu(), torch.zeros(6, n, 4))


@pytest.mark.parametrize("n", [84, 360])
def test_two_calls_give_the_same_bits(n):
    assert torch.equal(_bits(_paths(P.recipe(n).to(DEV), keep=0.1).cpu()), _bits(_got(n, 0.1)))


@pytest.mark.parametrize("S,n", [(40, 84), (12, 130)])
def test_many_subjects_walk_the_grid_stride(S, n):
    mats = torch.cat([P.recipe(n, seed=seed) for seed in range(-(-S // 6))])[:S].contiguous()
    dev = mats.to(DEV)
    with grid_of_three():
        few = _paths(dev, keep=0.1)
    full = _paths(dev, keep=0.1)
    assert torch.equal(_bits(few), _bits(full))
    assert torch.equal(_bits(full[:6].cpu()), _bits(_got(n, 0.1))), "a subject's result does not depend on its cohort"
    _check(mats[-6:], _thresholds(mats[-6:], 0.1), full[-6:].cpu(), f"S={S} n={n}, the last six subjects")


def test_offsets_beyond_2_31_elements():
    """16600 x 360 x 360 = 2.15 G matrix elements (8.6 GB), generated on the device in slices; subjects 0, S // 2 and
    S - 1 against the host statement."""
    Sb, n = 16600, 360
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        pytest.skip(f"needs 16 GB of free device memory, {free / 2 ** 30:.1f} GB are free")
    assert Sb * n * n > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(7)
    mats = torch.empty(Sb, n, n, device=DEV)
    for lo in range(0, Sb, 200):                         # in slices: no second cohort-sized temporary
        hi = min(lo + 200, Sb)
        r = torch.rand(hi - lo, n, n, device=DEV, generator=g)
        mats[lo:hi] = torch.maximum(r, r.transpose(1, 2))
    got = _paths(mats, keep=0.1)
    assert tuple(got.shape) == (Sb, n, 4)
    for s in (0, Sb // 2, Sb - 1):
        A = mats[s:s + 1].cpu()
        _check(A, _thresholds(A, 0.1), got[s:s + 1].cpu(), f"subject {s}")
    del mats, got


def test_paths_abi_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    n, S, ldx = 20, 6, 7
    dev = P.recipe(n).to(DEV)
    thr = ingest.select_thresholds(dev, keep=0.1)
    sp = _lib.stream_ptr()
    i32 = ctypes.c_int32
    ids, cols = (i32 * 4)(0, 1, 2, 3), (i32 * 4)(5, 1, 2, 4)
    need = lib.cgnn_ingest_paths_workspace_bytes(S, n, ids, 4)
    assert need >= 0
    work = torch.full((max(need, 16),), 7, dtype=torch.uint8, device=DEV)
    x = torch.full((S, n, ldx), -7.0, device=DEV)
    good = [_lib.ptr(dev), S, n, _lib.ptr(thr), ids, 4, cols, ldx, _lib.ptr(work), _lib.nbytes(work), _lib.ptr(x),
            _lib.nbytes(x), sp]
    bad = {"x one byte short": (11, _lib.nbytes(x) - 1), "matrices NULL": (0, None), "thr NULL": (3, None),
           "measures NULL": (4, None), "cols NULL": (6, None), "x NULL": (10, None), "S < 0": (1, -1), "n = 0": (2, 0),
           "n < 0": (2, -3), "n > 1024": (2, 1025), "S * n >= 2^31": (1, 2 ** 31 // n + 1), "no measure": (5, 0),
           "num_measures < 0": (5, -1), "five measures": (5, 5), "unknown id": (4, (i32 * 4)(0, 1, 2, 4)),
           "negative id": (4, (i32 * 4)(0, -1, 2, 3)), "repeated id": (4, (i32 * 4)(0, 1, 3, 3)),
           "column == ldx": (6, (i32 * 4)(5, 1, 2, 7)), "negative column": (6, (i32 * 4)(5, -1, 2, 4)),
           "repeated column": (6, (i32 * 4)(5, 1, 2, 5)), "ldx too small": (7, 5), "ldx = 0": (7, 0),
           "workspace bytes < 0": (9, -1), "misaligned workspace": (8, _lib.ptr(work) + 4),
           "misaligned matrices": (0, _lib.ptr(dev) + 2), "misaligned x": (10, _lib.ptr(x) + 2),
           "misaligned thr": (3, _lib.ptr(thr) + 2),
           # S * n * ldx * 4 would wrap 64 bits: the byte count is compared by division
           "ldx = 2^31 - 1": (7, 2 ** 31 - 1), "ldx = 2^30": (7, 2 ** 30)}
    if need > 0:
        bad.update({"workspace one byte short": (9, need - 1), "workspace NULL": (8, None)})
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_paths(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    for args in ((-1, n, ids, 4), (S, 0, ids, 4), (S, 1025, ids, 4), (S, n, None, 4), (S, n, ids, 0), (S, n, ids, 5),
                 (S, n, (i32 * 2)(3, 3), 2), (S, n, (i32 * 1)(4), 1), (2 ** 31 // n + 1, n, ids, 4)):
        assert lib.cgnn_ingest_paths_workspace_bytes(*args) < 0, args
    assert lib.cgnn_ingest_paths(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK                   # S == 0
    assert lib.cgnn_ingest_paths(None, 0, n, None, ids, 4, cols, ldx, None, 0, None, 0, sp) == _lib.CGNN_OK
    torch.cuda.synchronize()
    assert bool((work == 7).all()) and bool((x == -7.0).all()), "nothing was launched"
    # a good call into the middle of a wider tensor: columns 5, 1, 2, 4 are written, 0, 3 and 6 stay
    assert lib.cgnn_ingest_paths(*good) == _lib.CGNN_OK
    torch.cuda.synchronize()
    assert bool((work == 7).all())
    assert torch.equal(_bits(x[:, :, [5, 1, 2, 4]].cpu()), _bits(_got(n, 0.1)))
    assert bool((x[:, :, [0, 3, 6]] == -7.0).all()), "the other columns are untouched"
    # one measure, the last column
    x.fill_(-7.0)
    assert lib.cgnn_ingest_paths(_lib.ptr(dev), S, n, _lib.ptr(thr), (i32 * 1)(3), 1, (i32 * 1)(6), ldx, None, 0,
                                 _lib.ptr(x), _lib.nbytes(x), sp) == _lib.CGNN_OK
    assert torch.equal(_bits(x[:, :, 6].cpu()), _bits(_got(n, 0.1)[:, :, 3])) and bool((x[:, :, :6] == -7.0).all())
    assert tuple(_paths(dev[:0], keep=0.1).shape) == (0, n, 4)


def _same_but_x(got, want):
    for name in ("edge_local", "edge_weight", "labels", "edge_ptr_dev"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    assert torch.equal(got.edge_ptr, want.edge_ptr)


MIXED = ("strength", "closeness", "clustering", "local_efficiency", "nodal_efficiency")


@pytest.mark.parametrize("kw", [{"keep": 0.1}, {"num_edges": 500}, {"min_weight": 0.4}, {"min_weight": MIN_WEIGHT}],
                         ids=["keep", "num_edges", "min_weight", "min_weight[S]"])
def test_dataset_with_mixed_measures(kw):
    n = 84
    dev, y = P.recipe(n).to(DEV), I.labels(6).to(DEV)
    if isinstance(kw.get("min_weight"), tuple):
        kw = {"min_weight": torch.tensor(kw["min_weight"], device=DEV)}
    plain = ingest.from_matrices(dev, y, **kw)
    ds = ingest.from_matrices(dev, y, measures=MIXED, **kw)
    _same_but_x(ds, plain)
    assert ds.x.shape == (6, n, 5) and ds.x.is_contiguous() and ds.x.device.type == "cuda"
    assert torch.equal(_bits(ds.x), _bits(ingest.node_measures(dev, measures=MIXED, **kw)))
    assert torch.equal(_bits(ds.x[:, :, :1]), _bits(plain.x))
    only = ingest.from_matrices(dev, y, measures=P.PATH_MEASURES, **kw)
    _same_but_x(only, plain)
    assert torch.equal(_bits(only.x), _bits(_paths(dev, **kw)))
    assert torch.equal(_bits(only.x[:, :, [1, 3, 0]]), _bits(ds.x[:, :, [1, 3, 4]]))


@pytest.mark.parametrize("window,stride", [(None, None), (20, 10)])
def test_timeseries_hand_mixed_measures_through(window, stride):
    S, T, n = 4, 40, 84
    ts = TS.recipe(S, T, n).to(DEV)
    y = I.labels(S).to(DEV)
    W = TS.num_windows(T, window, stride)
    ds = ingest.from_timeseries(ts, y, keep=0.2, window=window, stride=stride, measures=MIXED)
    plain = ingest.from_timeseries(ts, y, keep=0.2, window=window, stride=stride)
    _same_but_x(ds, plain)
    mats = ingest.correlation_matrices(ts, window=window, stride=stride)
    assert ds.x.shape == (S * W, n, 5)
    assert torch.equal(_bits(ds.x), _bits(ingest.node_measures(mats, keep=0.2, measures=MIXED)))


def test_one_epoch_on_seven_features():
    """12 subjects x 84 ROI through ResidentDataLoader + Trainer with GCNConnectome(in_channels=7)."""
    S, n = 12, 84
    r = torch.rand(S, n, n, generator=torch.Generator().manual_seed(4))
    mats = torch.maximum(r, r.transpose(1, 2)).contiguous().to(DEV)
    names = ("strength", "degree", "clustering") + ingest.PATH_MEASURES
    ds = ingest.from_matrices(mats, I.labels(S).to(DEV), keep=0.1, measures=names)
    assert ds.x.shape == (S, n, 7) and bool(torch.isfinite(ds.x).all())
    torch.manual_seed(3)
    m = C.GCNConnectome(7, 64, dropout=0.0)
    before = [p.detach().clone() for p in m.parameters()]
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
    tr = C.Trainer(m, opt, device=DEV, graph=True)
    ld = ResidentDataLoader(ds, 6, shuffle=True, structure_cache=True)
    vl = ResidentDataLoader(ds, 6, shuffle=False, structure_cache=True)
    hist = tr.fit(ld, vl, num_epochs=1, patience=10, verbose=False)
    assert len(hist["train_loss"]) == 1
    assert all(torch.isfinite(torch.tensor(v)).all() for v in hist.values())
    after = [p.detach().cpu() for p in tr.model.parameters()]
    assert any(not torch.equal(a, b) for a, b in zip(after, before)), "the parameters moved"
    assert all(bool(torch.isfinite(a).all()) for a in after)
