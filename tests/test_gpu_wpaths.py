"""The weighted shortest-path node measures of connectome_gnn_amd.ingest on the device (csrc/wpaths.hip) against the
fp64 host statement (tests/wpaths_data.py: lengths ``float64(wmax) / float64(A_ij)``, scipy's Dijkstra), on recipe
subjects of tests/ingest_data.py and on structured graphs that carry random weights.

Bound, not taken from what the kernel gives: every distance and every column is within a relative ``(n + 2) 2^-24`` of
the statement.  A path of ``h <= n - 1`` positive fp32 terms, each carrying one division rounding, summed in any
association, is within ``h 2^-24`` relative; a min over such candidates keeps that bound; sums of such distances and of
their reciprocals keep it too (all terms are positive); the fp64 reductions add one final rounding.  The reachability
pattern -- the positions of ``+inf`` and of the zeros -- must match exactly.

The measured maximum is printed per shape, in units of ``2^-24``, next to ``H``, the largest hop count of a shortest
path.
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
from tests import wpaths_data as W
from tests.cohort_kit import DEV, bits as _bits, grid_of_three

pytestmark = pytest.mark.gpu
U =2.0 ** -24
NAMES = W.WEIGHTED_PATH_MEASURES
TWELVE = M.MEASURES + P.PATH_MEASURES + NAMES
CASES = [(5, 0.5), (37, 0.1), (64, 0.3), (65, 0.1), (130, 0.1), (360, 0.1)]
MIN_WEIGHT = (0.3, 0.5, 0.0)


def _check_subject(dist, cols, want, what):
    """One subject: ``dist`` [n, n] and ``cols`` [n, 3] float32 (host) against ``want`` = (dw, measures, H).  Returns the
    largest relative error in units of 2^-24."""
    D, Mw, H = want
    n = D.shape[0]
    bound = (n + 2) * U
    worst = 0.0
    assert dist.dtype == torch.float32 and tuple(dist.shape) == (n, n), what
    assert cols.dtype == torch.float32 and tuple(cols.shape) == (n, 3), what
    assert torch.equal(torch.isinf(dist), torch.isinf(D)), (what, "the unreachable pairs")
    assert bool((dist >= 0).all()), (what, "no NaN, nothing negative")
    assert torch.equal(dist == 0, D == 0) and torch.equal(dist.diagonal(), torch.zeros(n)), (what, "the zero diagonal")
    fin = torch.isfinite(D) & (D > 0)
    if bool(fin.any()):
        rel = ((dist.double() - D).abs()[fin] / D[fin])
        worst = float(rel.max())
        assert worst <= bound, (what, "path_lengths", worst / U, H)
    for c, name in enumerate(NAMES):
        g, w = cols[:, c].double(), Mw[:, c]
        assert torch.equal(g[w == 0], w[w == 0]), (what, name, "exact zeros")
        assert bool((g[w > 0] > 0).all()), (what, name)
        if bool((w > 0).any()):
            rel = float(((g - w).abs()[w > 0] / w[w > 0]).max())
            worst = max(worst, rel)
            assert rel <= bound, (what, name, rel / U, H)
    return worst / U


def _check(mats, thr, dist, cols, what, statements=None):
    worst, Hs = 0.0, []
    for s, (A, t) in enumerate(zip(mats, thr)):
        want = statements[s] if statements is not None else W.host_statement(A, t)
        worst = max(worst, _check_subject(dist[s], cols[s], want, (what, s)))
        Hs.append(want[2])
    n = mats.shape[1]
    print(f"{what}: max relative error {worst:.2f} x 2^-24, bound {n + 2} x 2^-24, H = {Hs}")


def _cols(dev, **kw):
    return ingest.node_measures(dev, measures=NAMES, **kw)


@functools.lru_cache(maxsize=None)
def _got(n, keep):
    """(path_lengths, the three columns) of ``W.cohort(n)`` at ``keep``, on the host."""
    dev = W.cohort(n).to(DEV)
    return ingest.path_lengths(dev, keep=keep).cpu(), _cols(dev, keep=keep).cpu()


# ---- 1: parity on the random recipe, symmetric and asymmetric subjects ----
@pytest.mark.parametrize("n,keep", CASES)
def test_parity_with_the_fp64_statement(n, keep):
    mats = W.cohort(n)
    thr = W.thresholds(mats, keep)
    if n > 5:
        mask = M.kept_mask(mats[W.ASYMMETRIC], thr[W.ASYMMETRIC])
        assert (mask != mask.T).any(), "an asymmetric kept set"
    dist, cols = _got(n, keep)
    assert tuple(dist.shape) == (3, n, n) and tuple(cols.shape) == (3, n, 3)
    _check(mats, thr, dist, cols, f"n={n} keep={keep}", W.cohort_statement(n, keep))


# ---- 2: structured weighted graphs ----
@pytest.mark.parametrize("n", [5, 33, 130])
def test_parity_on_structured_weighted_graphs(n):
    mats = W.structured_cohort(n)
    dev = mats.to(DEV)
    dist, cols = ingest.path_lengths(dev, min_weight=0.0).cpu(), _cols(dev, min_weight=0.0).cpu()
    _check(mats, [0.0] * len(mats), dist, cols, f"structured n={n}")
    dpath, cliques = W.STRUCTURED.index("directed_path"), W.STRUCTURED.index("cliques")
    assert W.host_statement(mats[dpath], 0.0)[2] == n - 1, "a chain of n - 1 hops crosses every block round"
    assert cols[dpath, n - 1].tolist() == [0.0, 0.0, 0.0], "the last node reaches nothing"
    assert cols[cliques, n - 1].tolist() == [0.0, 0.0, 0.0], "the isolated node"
    assert bool(torch.isinf(dist[dpath][torch.tril(torch.ones(n, n), -1) > 0]).all()), "nothing runs backwards"


# ---- 3: equal kept weights reduce to the binary measures ----
@pytest.mark.parametrize("n,keep", [(37, 0.1), (84, 0.1), (130, 0.3)])
def test_equal_weights_give_the_hop_distances_and_the_binary_columns(n, keep):
    mats = W.cohort(n)
    thr = W.thresholds(mats, keep)
    flat = W.equal_weights(mats, thr)
    dev = flat.to(DEV)
    dist = ingest.path_lengths(dev, min_weight=0.0).cpu()
    for s in range(3):
        hops = torch.from_numpy(P.distances(M.kept_mask(mats[s], thr[s])))
        want = torch.where(hops < 0, torch.tensor(float("inf")), hops.float())
        assert torch.equal(dist[s], want), (n, keep, s, "integer hop distances, exactly")
    both = ingest.node_measures(dev, min_weight=0.0, measures=NAMES + P.PATH_MEASURES[:3]).cpu().double()
    w, b = both[:, :, :3], both[:, :, 3:]
    assert torch.equal(w == 0, b == 0)
    assert bool(((w - b).abs() <= (n + 2) * U * b).all()), float(((w - b).abs() / b.clamp_min(1e-300)).max()) / U


# ---- 4: scale invariance ----
@pytest.mark.parametrize("n,keep", [(37, 0.1), (130, 0.1)])
def test_scaling_the_matrices_by_four_gives_the_same_bits(n, keep):
    dist, cols = _got(n, keep)
    dev = (W.cohort(n) * 4).contiguous().to(DEV)
    assert torch.equal(_bits(ingest.path_lengths(dev, keep=keep).cpu()), _bits(dist))
    assert torch.equal(_bits(_cols(dev, keep=keep).cpu()), _bits(cols))


# ---- 5: degenerate sizes ----
def test_one_and_two_nodes():
    one = torch.tensor([[[0.7]], [[0.0]]], device=DEV)
    assert ingest.path_lengths(one, keep=0.5).tolist() == [[[0.0]], [[0.0]]]
    assert torch.equal(_cols(one, keep=0.5).cpu(), torch.zeros(2, 1, 3))
    two = torch.tensor([[[9.0, 0.5], [0.25, 9.0]], [[0.0, 0.0], [0.3, 0.0]]])
    dev = two.to(DEV)
    dist, cols = ingest.path_lengths(dev, min_weight=0.0).cpu(), _cols(dev, min_weight=0.0).cpu()
    inf = float("inf")
    assert dist.tolist() == [[[0.0, 1.0], [2.0, 0.0]], [[0.0, inf], [1.0, 0.0]]]
    assert cols.tolist() == [[[1.0, 1.0, 1.0], [0.5, 0.5, 2.0]], [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]], "eccentricity may exceed 1"
    _check(two, [0.0, 0.0], dist, cols, "n=2")


@pytest.mark.parametrize("n", [5, 97])
def test_subjects_without_edges(n):
    dev = W.cohort(n).to(DEV)
    empty = torch.where(torch.eye(n, dtype=torch.bool), 0.0, float("inf")).expand(3, n, n)
    for kw in ({"keep": 0.0}, {"min_weight": float("inf")}):
        assert torch.equal(_cols(dev, **kw).cpu(), torch.zeros(3, n, 3)), kw
        assert torch.equal(ingest.path_lengths(dev, **kw).cpu(), empty), kw
    zero = torch.zeros(2, n, n, device=DEV)
    assert torch.equal(_cols(zero, keep=0.3).cpu(), torch.zeros(2, n, 3))
    assert torch.equal(ingest.path_lengths(zero, keep=0.3).cpu(), empty[:2])


def test_parity_at_per_subject_min_weight():
    n = 84
    mats = W.cohort(n)
    dev, mw = mats.to(DEV), torch.tensor(MIN_WEIGHT, device=DEV)
    _check(mats, list(MIN_WEIGHT), ingest.path_lengths(dev, min_weight=mw).cpu(), _cols(dev, min_weight=mw).cpu(),
           "n=84 min_weight=[S]")


# ---- 6: the size limit ----
def test_1024_nodes_and_the_limit():
    n = 1024
    mats = W.structured("watts_strogatz", n).unsqueeze(0).contiguous()
    dev = mats.to(DEV)
    _check(mats, [0.0], ingest.path_lengths(dev, min_weight=0.0).cpu(), _cols(dev, min_weight=0.0).cpu(),
           "n=1024 watts-strogatz")
    big = torch.zeros(1, 1025, 1025, device=DEV)
    with pytest.raises(ValueError, match="n <= 1024"):
        _cols(big, keep=0.1)
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.path_lengths(big, keep=0.1)
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.node_measures(big, keep=0.1, measures=("degree", "weighted_closeness"))
    assert tuple(ingest.node_measures(big, keep=0.1, measures=("degree",)).shape) == (1, 1025, 1)


# ---- 7: column mixing ----
@pytest.mark.parametrize("n", [33, 130])
def test_any_subset_in_any_order_is_the_columns_of_the_separate_calls(n):
    dev = W.cohort(n).to(DEV)
    full = torch.cat([ingest.node_measures(dev, keep=0.1).cpu(),
                      ingest.node_measures(dev, keep=0.1, measures=P.PATH_MEASURES).cpu(), _got(n, 0.1)[1]], 2)
    col = {name: c for c, name in enumerate(TWELVE)}
    for names in (("weighted_closeness",), ("weighted_eccentricity", "weighted_nodal_efficiency"), NAMES[::-1], TWELVE,
                  TWELVE[::-1], ("weighted_closeness", "degree"), ("closeness", "weighted_closeness"),
                  ("clustering", "weighted_eccentricity", "local_efficiency", "strength", "weighted_nodal_efficiency"),
                  ("weighted_nodal_efficiency", "eccentricity", "weighted_clustering", "weighted_eccentricity")):
        got = ingest.node_measures(dev, keep=0.1, measures=names).cpu()
        assert tuple(got.shape) == (3, n, len(names))
        assert torch.equal(_bits(got), _bits(full[:, :, [col[m] for m in names]])), names
    got = ingest.node_measures(dev, num_edges=W.rank_of(n, keep=0.1), measures=TWELVE).cpu()
    assert torch.equal(_bits(got), _bits(full))


def test_a_request_without_weighted_names_gives_the_bits_of_the_c_abi_calls():
    n, S = 84, 3
    dev = W.cohort(n).to(DEV)
    lib = _lib.load()
    thr = ingest.select_thresholds(dev, keep=0.1)
    i32 = ctypes.c_int32
    classic = ("clustering", "strength", "weighted_clustering")
    ids = (i32 * 3)(*[M.MEASURES.index(m) for m in classic])
    need = lib.cgnn_ingest_measures_workspace_bytes(S, n, ids, 3)
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    xc = torch.empty(S, n, 3, device=DEV)
    assert lib.cgnn_ingest_measures(_lib.ptr(dev), S, n, _lib.ptr(thr), ids, 3, _lib.ptr(work), need, _lib.ptr(xc),
                                    _lib.nbytes(xc), _lib.stream_ptr()) == _lib.CGNN_OK
    assert torch.equal(_bits(ingest.node_measures(dev, keep=0.1, measures=classic)), _bits(xc))
    xp = torch.empty(S, n, 4, device=DEV)
    assert lib.cgnn_ingest_paths(_lib.ptr(dev), S, n, _lib.ptr(thr), (i32 * 4)(0, 1, 2, 3), 4, (i32 * 4)(0, 1, 2, 3), 4,
                                 None, 0, _lib.ptr(xp), _lib.nbytes(xp), _lib.stream_ptr()) == _lib.CGNN_OK
    assert torch.equal(_bits(ingest.node_measures(dev, keep=0.1, measures=P.PATH_MEASURES)), _bits(xp))
    mixed = ingest.node_measures(dev, keep=0.1, measures=("closeness", "strength", "local_efficiency", "clustering"))
    assert torch.equal(_bits(mixed), _bits(torch.stack([xp[:, :, 1], xc[:, :, 1], xp[:, :, 3], xc[:, :, 0]], 2)))


# ---- 8: determinism ----
@pytest.mark.parametrize("n", [84, 360])
def test_two_calls_give_the_same_bits(n):
    dev = W.cohort(n).to(DEV)
    dist, cols = _got(n, 0.1)
    assert torch.equal(_bits(ingest.path_lengths(dev, keep=0.1).cpu()), _bits(dist))
    assert torch.equal(_bits(_cols(dev, keep=0.1).cpu()), _bits(cols))


@pytest.mark.parametrize("S,n", [(40, 84), (12, 130)])
def test_a_grid_of_three_gives_the_bits_of_the_default_grid(S, n):
    mats = torch.cat([W.recipe(n, seed=seed)[list(W.SUBJECTS)] for seed in range(-(-S // 3))])[:S].contiguous()
    dev = mats.to(DEV)
    with grid_of_three():
        few, few_dist = _cols(dev, keep=0.1), ingest.path_lengths(dev, keep=0.1)
    full, full_dist = _cols(dev, keep=0.1), ingest.path_lengths(dev, keep=0.1)
    assert torch.equal(_bits(few), _bits(full)) and torch.equal(_bits(few_dist), _bits(full_dist))
    assert torch.equal(_bits(full[:3].cpu()), _bits(_got(n, 0.1)[1])), "a subject's result does not depend on its cohort"
    tail = mats[-3:]
    _check(tail, W.thresholds(tail, 0.1), few_dist[-3:].cpu(), few[-3:].cpu(), f"S={S} n={n} grid 3, the last three")


# ---- 9: the C ABI ----
def test_wpaths_abi_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    n, S, ldx = 20, 3, 6
    dev = W.cohort(n).to(DEV)
    thr = ingest.select_thresholds(dev, keep=0.3)
    sp = _lib.stream_ptr()
    i32 = ctypes.c_int32
    ids, cols = (i32 * 3)(0, 1, 2), (i32 * 3)(5, 1, 3)
    need = lib.cgnn_ingest_wpaths_workspace_bytes(S, n, ids, 3)
    assert need > 0 and need == lib.cgnn_ingest_wpaths_workspace_bytes(S, n, None, 0)
    work = torch.full((need,), 7, dtype=torch.uint8, device=DEV)
    x = torch.full((S, n, ldx), -7.0, device=DEV)
    dist = torch.full((S, n, n), -7.0, device=DEV)
    good = [_lib.ptr(dev), S, n, _lib.ptr(thr), ids, 3, cols, ldx, _lib.ptr(work), need, _lib.ptr(x), _lib.nbytes(x),
            _lib.ptr(dist), _lib.nbytes(dist), sp]
    bad = {"x one byte short": (11, _lib.nbytes(x) - 1), "dist one byte short": (13, _lib.nbytes(dist) - 1),
           "workspace one byte short": (9, need - 1), "workspace NULL": (8, None), "matrices NULL": (0, None),
           "thr NULL": (3, None), "measures NULL": (4, None), "cols NULL": (6, None), "x NULL": (10, None), "S < 0": (1, -1),
           "n = 0": (2, 0), "n < 0": (2, -3), "n > 1024": (2, 1025), "S * n >= 2^31": (1, 2 ** 31 // n + 1),
           "num_measures < 0": (5, -1), "four measures": (5, 4), "unknown id": (4, (i32 * 3)(0, 1, 3)),
           "negative id": (4, (i32 * 3)(0, -1, 2)), "repeated id": (4, (i32 * 3)(0, 2, 2)),
           "column == ldx": (6, (i32 * 3)(5, 1, 6)), "negative column": (6, (i32 * 3)(5, -1, 3)),
           "repeated column": (6, (i32 * 3)(5, 1, 5)), "ldx too small": (7, 5), "ldx = 0": (7, 0),
           "workspace bytes < 0": (9, -1), "x bytes < 0": (11, -1), "dist bytes < 0": (13, -1),
           "misaligned workspace": (8, _lib.ptr(work) + 4), "misaligned matrices": (0, _lib.ptr(dev) + 2),
           "misaligned x": (10, _lib.ptr(x) + 2), "misaligned dist": (12, _lib.ptr(dist) + 2),
           "misaligned thr": (3, _lib.ptr(thr) + 2),
           # S * n * ldx * 4 would wrap 64 bits: the byte count is compared by division
           "ldx = 2^31 - 1": (7, 2 ** 31 - 1), "ldx = 2^30": (7, 2 ** 30)}
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_wpaths(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    # neither x nor dist
    assert lib.cgnn_ingest_wpaths(*(good[:4] + [None, 0, None, 0] + good[8:10] + [None, 0, None, 0, sp])) == _lib.CGNN_EINVAL
    for args in ((-1, n, ids, 3), (S, 0, ids, 3), (S, 1025, ids, 3), (S, n, None, 3), (S, n, ids, 4), (S, n, ids, -1),
                 (S, n, (i32 * 2)(2, 2), 2), (S, n, (i32 * 1)(3), 1), (2 ** 31 // n + 1, n, ids, 3)):
        assert lib.cgnn_ingest_wpaths_workspace_bytes(*args) < 0, args
    assert lib.cgnn_ingest_wpaths(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK                  # S == 0
    assert lib.cgnn_ingest_wpaths(None, 0, n, None, ids, 3, cols, ldx, None, 0, None, 0, None, 0, sp) == _lib.CGNN_OK
    torch.cuda.synchronize()
    assert bool((work == 7).all()) and bool((x == -7.0).all()) and bool((dist == -7.0).all()), "nothing was launched"
    want_dist, want_cols = ingest.path_lengths(dev, keep=0.3), _cols(dev, keep=0.3)
    # a good call into the middle of a wider tensor: columns 5, 1, 3 are written, 0, 2 and 4 stay
    assert lib.cgnn_ingest_wpaths(*good) == _lib.CGNN_OK
    torch.cuda.synchronize()
    assert torch.equal(_bits(x[:, :, [5, 1, 3]]), _bits(want_cols)) and torch.equal(_bits(dist), _bits(want_dist))
    assert bool((x[:, :, [0, 2, 4]] == -7.0).all()), "the other columns are untouched"
    # dist alone: no measures, x NULL; and one measure without dist
    dist.fill_(-7.0)
    x.fill_(-7.0)
    assert lib.cgnn_ingest_wpaths(_lib.ptr(dev), S, n, _lib.ptr(thr), None, 0, None, 0, _lib.ptr(work), need, None, 0,
                                  _lib.ptr(dist), _lib.nbytes(dist), sp) == _lib.CGNN_OK
    assert lib.cgnn_ingest_wpaths(_lib.ptr(dev), S, n, _lib.ptr(thr), (i32 * 1)(2), 1, (i32 * 1)(4), ldx, _lib.ptr(work),
                                  need, _lib.ptr(x), _lib.nbytes(x), None, 0, sp) == _lib.CGNN_OK
    torch.cuda.synchronize()
    assert torch.equal(_bits(dist), _bits(want_dist))
    assert torch.equal(_bits(x[:, :, 4]), _bits(want_cols[:, :, 2])) and bool((x[:, :, [0, 1, 2, 3, 5]] == -7.0).all())
    assert tuple(_cols(dev[:0], keep=0.1).shape) == (0, n, 3) and tuple(ingest.path_lengths(dev[:0], keep=0.1).shape) == (0, n, n)
    _check(W.cohort(n), W.thresholds(W.cohort(n), 0.3), want_dist.cpu(), want_cols.cpu(), "n=20 keep=0.3")


# ---- 10: integration ----
MIXED = ("strength", "weighted_closeness", "closeness", "weighted_eccentricity", "clustering", "weighted_nodal_efficiency")


def _same_but_x(got, want):
    for name in ("edge_local", "edge_weight", "labels", "edge_ptr_dev"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    assert torch.equal(got.edge_ptr, want.edge_ptr)


@pytest.mark.parametrize("kw", [{"keep": 0.1}, {"num_edges": 500}, {"min_weight": MIN_WEIGHT}],
                         ids=["keep", "num_edges", "min_weight[S]"])
def test_dataset_with_mixed_measures(kw):
    n = 84
    dev, y = W.cohort(n).to(DEV), I.labels(3).to(DEV)
    if isinstance(kw.get("min_weight"), tuple):
        kw = {"min_weight": torch.tensor(kw["min_weight"], device=DEV)}
    plain = ingest.from_matrices(dev, y, **kw)
    ds = ingest.from_matrices(dev, y, measures=MIXED, **kw)
    _same_but_x(ds, plain)
    assert ds.x.shape == (3, n, 6) and ds.x.is_contiguous() and ds.x.device.type == "cuda"
    assert torch.equal(_bits(ds.x), _bits(ingest.node_measures(dev, measures=MIXED, **kw)))
    assert torch.equal(_bits(ds.x[:, :, :1]), _bits(plain.x))
    assert torch.equal(_bits(ds.x[:, :, [5, 1, 3]]), _bits(_cols(dev, **kw)))


@pytest.mark.parametrize("window,stride", [(None, None), (20, 10)])
def test_timeseries_hand_the_names_through(window, stride):
    S, T, n = 4, 40, 84
    ts = TS.recipe(S, T, n).to(DEV)
    y = I.labels(S).to(DEV)
    W_ = TS.num_windows(T, window, stride)
    ds = ingest.from_timeseries(ts, y, keep=0.2, window=window, stride=stride, measures=MIXED)
    _same_but_x(ds, ingest.from_timeseries(ts, y, keep=0.2, window=window, stride=stride))
    mats = ingest.correlation_matrices(ts, window=window, stride=stride)
    assert ds.x.shape == (S * W_, n, 6)
    assert torch.equal(_bits(ds.x), _bits(ingest.node_measures(mats, keep=0.2, measures=MIXED)))
    assert bool(torch.isfinite(ds.x).all())


def test_one_epoch_on_features_of_all_three_kinds():
    """12 subjects x 84 ROI through ResidentDataLoader + Trainer with GCNConnectome(in_channels=7)."""
    S, n = 12, 84
    r = torch.rand(S, n, n, generator=torch.Generator().manual_seed(4))
    mats = torch.maximum(r, r.transpose(1, 2)).contiguous().to(DEV)
    names = ("strength", "degree", "closeness", "local_efficiency") + ingest.WEIGHTED_PATH_MEASURES
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
