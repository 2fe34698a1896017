"""connectome_gnn_amd.ingest.node_measures on the device (csrc/measures.hip) against the fp64 host statement
(tests/measures_data.py) on the six recipe subjects of tests/ingest_data.py.

Bounds, none of them taken from what the kernels give:

* ``degree`` is the correctly rounded fp32 quotient ``k_i / (n - 1)`` (bit-equal to the host's), and
  ``round(degree * (n - 1))`` in fp64 is ``k_i`` exactly.  (The product formed in fp32 is not always ``k_i`` --
  ``15 / 19 * 19`` is not 15 in fp32 -- so the round is taken in fp64.)
* ``clustering``: ``T_i(b)`` is a sum of products of 0 and 1 below ``2^24`` on the exact fp32 pipe, so
  ``round(clustering * k (k - 1))`` is the exact integer and the one division leaves at most ``2^-22`` relative.
* ``weighted_clustering``: ``|got - want| <= (2 n + 64) 2^-23 want`` -- twice the first-order bound of two chained
  fp32 accumulations of ``n`` non-negative terms, with slack for three cube roots, three divisions and the final
  quotient; on the subjects without non-finite kept weights.  The measured maximum is printed per shape.
* ``strength``: the bits of the default feature of ``from_matrices``.
* ``mean_weight``: ``n 2^-23`` relative (one fp32 accumulation of at most ``n`` non-negative terms and a division).
"""
import functools

import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib, ingest
from connectome_gnn_amd.resident import ResidentDataLoader
from tests import ingest_data as I
from tests import measures_data as M
from tests import timeseries_data as TS

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -23
SIZES = [1, 2, 3, 5, 20, 31, 32, 33, 84, 95, 96, 97, 130, 193, 360]
CASES = [(n, 0.1) for n in SIZES] + [(n, keep) for keep in (0.5, 1.0) for n in (84, 97)]
MIN_WEIGHT = (0.3, 0.5, 0.0, 0.7, -1.0, 0.6)          # the per-subject min_weight= case, n = 84
COL = {name: c for c, name in enumerate(M.MEASURES)}


def _bits(t):
    return t.contiguous().view(torch.int32)


class Case:
    """One cohort at one set of thresholds: the statement (computed once, shared) and the device result."""

    def __init__(self, mats, thr, got):
        self.mats, self.thr, self.got = mats, thr, got.cpu()
        self.n = mats.shape[1]
        self.want = M.cohort_measures(mats, thr)
        counts = [M.host_counts(A, float(t)) for A, t in zip(mats, thr)]
        self.k = torch.stack([c[0] for c in counts])
        self.T = torch.stack([c[1] for c in counts])
        self.finite = [M.finite_weights(A, float(t)) for A, t in zip(mats, thr)]


@functools.lru_cache(maxsize=None)
def _case(n, keep):
    mats = M.recipe(n)
    thr = [M.host_threshold(A, M.rank_of(n, keep=keep)) for A in mats]
    return Case(mats, thr, ingest.node_measures(mats.to(DEV), keep=keep))


@functools.lru_cache(maxsize=None)
def _min_weight_case():
    mats = M.recipe(84)
    thr = torch.tensor(MIN_WEIGHT)
    return Case(mats, list(MIN_WEIGHT), ingest.node_measures(mats.to(DEV), min_weight=thr.to(DEV)))


def _check(c, what):
    n, got, want = c.n, c.got, c.want
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(c.mats), n, 5), what
    k = c.k.double()
    pairs = k * (k - 1)
    # degree
    deg = got[:, :, COL["degree"]]
    assert torch.equal(_bits(deg), _bits(c.k.float() / (n - 1) if n > 1 else torch.zeros_like(deg))), what
    assert torch.equal(torch.round(deg.double() * (n - 1)).long(), c.k if n > 1 else torch.zeros_like(c.k)), what
    # clustering: exact integers, one rounding
    cl = got[:, :, COL["clustering"]].double()
    assert torch.equal(torch.round(cl * pairs).long(), torch.where(c.k >= 2, c.T, torch.zeros_like(c.T))), what
    wcl = want[:, :, COL["clustering"]]
    assert bool(((cl - wcl).abs() <= 2.0 ** -22 * wcl).all()), what
    assert int(c.T.max()) < 2 ** 24
    # mean_weight and weighted_clustering
    worst = 0.0
    for s in range(len(c.mats)):
        g, w = got[s, :, COL["mean_weight"]].double(), want[s, :, COL["mean_weight"]]
        fin = torch.isfinite(w)
        assert bool(((g - w).abs()[fin] <= n * EPS * w[fin]).all()), (what, s, "mean_weight")
        assert torch.equal(g[~fin], w[~fin]), (what, s, "a kept +inf propagates")
        if c.finite[s]:
            g, w = got[s, :, COL["weighted_clustering"]].double(), want[s, :, COL["weighted_clustering"]]
            rel = ((g - w).abs() / w.clamp_min(1e-300)).max() if bool((w > 0).any()) else torch.tensor(0.0)
            worst = max(worst, float(rel))
            assert bool(((g - w).abs() <= (2 * n + 64) * EPS * w).all()), (what, s, "weighted_clustering", float(rel))
    print(f"{what}: weighted_clustering max relative error {worst:.3e}, bound {(2 * n + 64) * EPS:.3e}")
    # subjects without edges
    for s in range(len(c.mats)):
        if int(c.k[s].sum()) == 0:
            assert torch.equal(got[s], torch.zeros(n, 5)), (what, s)


@pytest.mark.parametrize("n,keep", CASES)
def test_parity_with_the_fp64_statement(n, keep):
    c = _case(n, keep)
    if n >= 5 and keep == 1.0:
        assert int(c.k[3].min()) >= n - 2, "near-complete graphs"
    _check(c, f"n={n} keep={keep}")


def test_parity_at_per_subject_min_weight():
    c = _min_weight_case()
    assert int(c.k[4].sum()) > 0 and not c.finite[5]
    _check(c, "n=84 min_weight=[S]")


@pytest.mark.parametrize("n,keep", [(5, 0.1), (84, 0.1), (97, 0.5), (84, 1.0), (360, 0.1)])
def test_strength_is_the_default_feature_bit_for_bit(n, keep):
    ds = ingest.from_matrices(M.recipe(n).to(DEV), I.labels(6).to(DEV), keep=keep)
    assert torch.equal(_bits(_case(n, keep).got[:, :, :1]), _bits(ds.x.cpu()))


@pytest.mark.parametrize("n", [33, 130])
def test_any_subset_in_any_order_is_the_columns_of_the_full_call(n):
    dev = M.recipe(n).to(DEV)
    full = _case(n, 0.1).got
    for names in (("weighted_clustering",), ("clustering",), ("degree",), ("clustering", "strength"),
                  ("weighted_clustering", "mean_weight", "degree"), M.MEASURES[::-1],
                  ("mean_weight", "weighted_clustering", "clustering", "strength")):
        got = ingest.node_measures(dev, keep=0.1, measures=names).cpu()
        assert tuple(got.shape) == (6, n, len(names))
        assert torch.equal(_bits(got), _bits(full[:, :, [COL[m] for m in names]])), names
    assert torch.equal(_bits(ingest.node_measures(dev, num_edges=M.rank_of(n, keep=0.1)).cpu()), _bits(full))


@pytest.mark.parametrize("n", [5, 97])
def test_subjects_without_edges_give_zeros(n):
    dev = M.recipe(n).to(DEV)
    assert torch.equal(ingest.node_measures(dev, keep=0.0).cpu(), torch.zeros(6, n, 5))
    assert torch.equal(_case(n, 0.1).got[2], torch.zeros(n, 5)), "the all-zero subject"
    assert torch.equal(ingest.node_measures(dev, min_weight=float("inf")).cpu(), torch.zeros(6, n, 5))


@pytest.mark.parametrize("n", [84, 360])
def test_two_calls_give_the_same_bits(n):
    again = ingest.node_measures(M.recipe(n).to(DEV), keep=0.1)
    assert torch.equal(_bits(again.cpu()), _bits(_case(n, 0.1).got))


@pytest.mark.parametrize("S,n", [(40, 84), (12, 130)])
def test_many_subjects_walk_the_grid_stride(S, n):
    mats = torch.cat([M.recipe(n, seed=seed) for seed in range(-(-S // 6))])[:S].contiguous()
    dev = mats.to(DEV)
    lib = _lib.load()
    try:
        assert lib.cgnn_set_fused_grid(3) == _lib.CGNN_OK
        few = ingest.node_measures(dev, keep=0.1)
    finally:
        lib.cgnn_set_fused_grid(0)
    full = ingest.node_measures(dev, keep=0.1)
    assert torch.equal(_bits(few), _bits(full))
    first = _case(n, 0.1).got
    assert torch.equal(_bits(full[:6].cpu()), _bits(first)), "a subject's result does not depend on its cohort"
    thr = [M.host_threshold(A, M.rank_of(n, keep=0.1)) for A in mats[-6:]]
    _check(Case(mats[-6:], thr, full[-6:]), f"S={S} n={n}, the last six subjects")


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
    got = ingest.node_measures(mats, keep=0.1)
    assert tuple(got.shape) == (Sb, n, 5)
    k = M.rank_of(n, keep=0.1)
    for s in (0, Sb // 2, Sb - 1):
        A = mats[s:s + 1].cpu()
        _check(Case(A, [M.host_threshold(A[0], k)], got[s:s + 1]), f"subject {s}")
    del mats, got


def test_measures_abi_refuses_bad_arguments_before_any_launch():
    import ctypes
    lib = _lib.load()
    n, S = 20, 6
    mats = M.recipe(n)
    dev = mats.to(DEV)
    thr = ingest.select_thresholds(dev, keep=0.1)
    sp = _lib.stream_ptr()
    ids = (ctypes.c_int32 * 5)(0, 1, 2, 3, 4)
    need = lib.cgnn_ingest_measures_workspace_bytes(S, n, ids, 5)
    assert need >= 4 * (2 * S * n + 2 * S + 2 * S * 96)
    two = (ctypes.c_int32 * 2)(1, 0)
    assert 0 < lib.cgnn_ingest_measures_workspace_bytes(S, n, two, 2) < need, "no partial sums without clustering"
    work = torch.full((need,), 7, dtype=torch.uint8, device=DEV)
    x = torch.full((S, n, 5), -7.0, device=DEV)
    good = [_lib.ptr(dev), S, n, _lib.ptr(thr), ids, 5, _lib.ptr(work), need, _lib.ptr(x), _lib.nbytes(x), sp]
    bad = {"workspace one byte short": (7, need - 1), "x one byte short": (9, _lib.nbytes(x) - 1),
           "matrices NULL": (0, None), "thr NULL": (3, None), "measures NULL": (4, None), "workspace NULL": (6, None),
           "x NULL": (8, None), "S < 0": (1, -1), "n = 0": (2, 0), "n < 0": (2, -3),
           "S * n >= 2^31": (1, 2 ** 31 // n + 1), "n * n >= 2^31": (2, 46341), "no measure": (5, 0),
           "num_measures < 0": (5, -1), "six measures": (5, 6),
           "unknown id": (4, (ctypes.c_int32 * 5)(0, 1, 2, 3, 5)), "negative id": (4, (ctypes.c_int32 * 5)(0, -1, 2, 3, 4)),
           "repeated id": (4, (ctypes.c_int32 * 5)(0, 1, 2, 3, 3)), "misaligned workspace": (6, _lib.ptr(work) + 4),
           "misaligned matrices": (0, _lib.ptr(dev) + 2)}
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_measures(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    for args in ((-1, n, ids, 5), (S, 0, ids, 5), (S, n, None, 5), (S, n, ids, 0), (S, n, ids, 6),
                 (S, n, (ctypes.c_int32 * 2)(3, 3), 2), (2 ** 31 // n + 1, n, ids, 5), (S, 46341, ids, 5)):
        assert lib.cgnn_ingest_measures_workspace_bytes(*args) < 0, args
    assert lib.cgnn_ingest_measures(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK                # S == 0
    assert lib.cgnn_ingest_measures(None, 0, n, None, ids, 5, None, 0, None, 0, sp) == _lib.CGNN_OK
    torch.cuda.synchronize()
    assert bool((work == 7).all()) and bool((x == -7.0).all()), "nothing was launched"
    assert lib.cgnn_ingest_measures(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(x.cpu()), _bits(_case(n, 0.1).got))
    assert tuple(ingest.node_measures(dev[:0], keep=0.1).shape) == (0, n, 5)


def _same_but_x(got, want):
    for name in ("edge_local", "edge_weight", "labels", "edge_ptr_dev"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    assert torch.equal(got.edge_ptr, want.edge_ptr)


@pytest.mark.parametrize("kw", [{"keep": 0.1}, {"num_edges": 500}, {"min_weight": 0.4}, {"min_weight": MIN_WEIGHT}],
                         ids=["keep", "num_edges", "min_weight", "min_weight[S]"])
def test_dataset_with_measures(kw):
    n = 84
    dev, y = M.recipe(n).to(DEV), I.labels(6).to(DEV)
    if isinstance(kw["min_weight"] if "min_weight" in kw else None, tuple):
        kw = {"min_weight": torch.tensor(kw["min_weight"], device=DEV)}
    plain = ingest.from_matrices(dev, y, **kw)
    ds = ingest.from_matrices(dev, y, measures=True, **kw)
    _same_but_x(ds, plain)
    assert ds.x.shape == (6, n, 5) and ds.x.is_contiguous() and ds.x.device.type == "cuda"
    assert torch.equal(_bits(ds.x), _bits(ingest.node_measures(dev, **kw)))
    assert torch.equal(_bits(ds.x[:, :, :1]), _bits(plain.x))
    names = ("clustering", "degree")
    sub = ingest.from_matrices(dev, y, measures=names, **kw)
    _same_but_x(sub, plain)
    assert torch.equal(_bits(sub.x), _bits(ingest.node_measures(dev, measures=names, **kw)))


@pytest.mark.parametrize("window,stride", [(None, None), (20, 10)])
def test_timeseries_hand_measures_through(window, stride):
    S, T, n = 4, 40, 84
    ts = TS.recipe(S, T, n).to(DEV)
    y = I.labels(S).to(DEV)
    W = TS.num_windows(T, window, stride)
    ds = ingest.from_timeseries(ts, y, keep=0.2, window=window, stride=stride, measures=True)
    mats = ingest.correlation_matrices(ts, window=window, stride=stride)
    ref = ingest.from_matrices(mats, y.repeat_interleave(W), keep=0.2, measures=True)
    _same_but_x(ds, ref)
    assert ds.x.shape == (S * W, n, 5) and torch.equal(_bits(ds.x), _bits(ref.x))
    assert torch.equal(_bits(ds.x), _bits(ingest.node_measures(mats, keep=0.2)))


def test_one_epoch_on_five_measures():
    """12 subjects x 84 ROI through ResidentDataLoader + Trainer with GCNConnectome(in_channels=5)."""
    S, n = 12, 84
    r = torch.rand(S, n, n, generator=torch.Generator().manual_seed(4))
    mats = torch.maximum(r, r.transpose(1, 2)).contiguous().to(DEV)
    ds = ingest.from_matrices(mats, I.labels(S).to(DEV), keep=0.1, measures=True)
    assert ds.x.shape == (S, n, 5) and bool(torch.isfinite(ds.x).all())
    torch.manual_seed(3)
    m = C.GCNConnectome(5, 64, dropout=0.0)
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
