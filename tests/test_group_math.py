"""The host statement of the group-consensus edges (tests/group_data.py) against independent ones: exact rational sums
for the mean, integer counts for the consistency, numpy for the Fisher mean; the public argument checks of
``ingest.group_matrix``, ``ingest.group_sparsify`` and ``group=`` on CPU tensors; the header and the binding of
cgnn_ingest_group / cgnn_ingest_group_mask; and the seeded cohort that shows what a common topology is for.  No device is
touched."""
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

import connectome_gnn_amd
from connectome_gnn_amd import _lib, ingest
from tests import group_data as G
from tests import ingest_data as D
from tests import knn_data as K
from tests.abi_header import check_header

NAN, INF = float("nan"), float("inf")


def _finite_cohort(S, n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(S, n, n, generator=g) * 10 ** torch.randint(-3, 4, (S, n, n), generator=g).float()).contiguous()


def _round_fraction(q):
    """the fp32 nearest to fp64(q): the statement's two roundings, of an exact rational"""
    return torch.tensor(float(q), dtype=torch.float64).float()


@pytest.mark.parametrize("S,n", [(1, 2), (3, 3), (5, 4), (G.SLICE + 3, 2)])
def test_the_mean_is_the_rounded_exact_sum_where_the_sum_is_exact(S, n):
    """Values that are multiples of 2^-10 below 2^10: every fp64 partial sum is exact, so the statement's order plays no
    part and the result is the exact rational mean rounded to fp64 by the division and to fp32 once."""
    g = torch.Generator().manual_seed(S * 10 + n)
    mats = (torch.randint(-2 ** 20, 2 ** 20, (S, n, n), generator=g).float() / 1024).contiguous()
    for among in (None, torch.arange(S) % 2 == 0):
        got = G.host_group(mats, "mean", among=among)
        units = G.included(S, among)
        for i in range(n):
            for j in range(n):
                q = sum(Fraction(float(mats[s, i, j])) for s in units) / len(units)
                assert float(got[i, j]) == float(_round_fraction(q)), (i, j)


def test_the_order_of_the_sum_is_the_headers():
    """Where fp64 addition rounds the order matters: the statement's slices against a plain ascending sum."""
    S, n = 2 * G.SLICE + 5, 3
    mats = _finite_cohort(S, n)
    mats[0] = 1e30
    mats[G.SLICE] = -1e30                                   # cancels only after the first slice was rounded
    in_slices = G.host_sum(lambda s: mats[s].double(), S, n)
    partials = [sum((mats[s].double() for s in range(lo, min(S, lo + G.SLICE))), torch.zeros(n, n, dtype=torch.float64))
                for lo in range(0, S, G.SLICE)]
    assert torch.equal(in_slices, partials[0] + partials[1] + partials[2])
    plain = sum((mats[s].double() for s in range(S)), torch.zeros(n, n, dtype=torch.float64))
    assert not torch.equal(in_slices, plain)
    assert torch.equal(G.host_sum(lambda s: mats[s].double(), S, n, slice_=S), plain)


@pytest.mark.parametrize("n", [1, 2, 5, 20])
def test_the_consistency_is_an_integer_count(n):
    mats = G.cohort(9, n)
    S = mats.shape[0]
    for choice in (dict(keep=0.3), dict(num_edges=3), dict(min_weight=0.1),
                   dict(min_weight=torch.linspace(-0.5, 0.5, S))):
        thr = G.host_unit_thresholds(mats, **choice)
        for among in (None, torch.arange(S) % 3 != 1):
            got = G.host_group(mats, "consistency", thr, among)
            units = G.included(S, among)
            count = torch.zeros(n, n, dtype=torch.long)
            for s in units:
                ei, _ = D.host_edges(mats[s], thr[s])
                count[ei[0], ei[1]] += 1
            want = torch.tensor([[float(np.float32(np.float64(int(c)) / np.float64(len(units)))) for c in row]
                                 for row in count.tolist()]).reshape(n, n)
            assert torch.equal(got, want), choice
            assert not got.diagonal().any() and bool((got >= 0).all()) and bool((got <= 1).all())


@pytest.mark.parametrize("S,n", [(3, 5), (G.SLICE + 1, 4)])
def test_the_fisher_mean_against_numpy(S, n):
    mats = G.correlations(S, n)
    got = G.host_group(mats, "fisher_mean", exact=True).numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.tanh(np.arctanh(mats.numpy().astype(np.float64)).sum(0) / S)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 2.0 ** -40)             # (another order of the sum, another libm)
    assert got[0, 2] == -1.0 and got[1, 2] == 1.0, "|r| == 1 goes through atanh as an infinity"
    assert np.all(np.diag(got) == 1.0)
    a = mats.clone()
    a[0, 1, 2] = -1.0                                                    # -inf meets unit S - 1's +inf
    assert np.isnan(G.host_group(a, "fisher_mean").numpy()[1, 2])


def test_the_natural_consequences():
    mats = G.cohort(8, 5)
    none = torch.zeros(8, dtype=torch.bool)
    for stat, thr in (("mean", None), ("fisher_mean", None), ("consistency", [0.0] * 8)):
        assert bool(torch.isnan(G.host_group(mats, stat, thr, none)).all()), "no units: NaN everywhere"
        every = G.host_group(mats, stat, thr, ~none)
        assert torch.equal(K.bits(every), K.bits(G.host_group(mats, stat, thr)))
        poisoned = mats.clone()
        poisoned[1::2] = torch.tensor([NAN, INF, 1e30, -INF, NAN]).repeat(5, 1)
        half = torch.arange(8) % 2 == 0
        assert torch.equal(K.bits(G.host_group(poisoned, stat, thr, half)), K.bits(G.host_group(mats, stat, thr, half)))
    mean = G.host_group(mats, "mean")
    assert bool(torch.isnan(mean[0, 1])) and bool(torch.isnan(mean[0, 3]))       # a NaN; +inf and -inf
    assert float(mean[2, 2]) == INF                                        # the diagonal is reduced like any entry
    sym = G.correlations(7, 6)
    for stat, thr in (("mean", None), ("fisher_mean", None), ("consistency", [0.2] * 7)):
        g = G.host_group(sym, stat, thr)
        assert torch.equal(K.bits(g), K.bits(g.t().contiguous())), stat


def test_the_mask_and_the_edge_set():
    mats = G.cohort(8, 5).clone()
    grp = torch.full((5, 5), 0.5)
    grp[0, 1] = NAN
    grp[1, 0] = 0.25
    mats[0, 2, 3] = -0.0
    mats[1, 2, 3] = NAN
    E = G.host_edge_set(grp, min_weight=0.3)
    assert not E.diagonal().any() and not bool(E[0, 1]) and not bool(E[1, 0]) and int(E.sum()) == 18
    out = G.host_mask(mats, E)
    assert int(K.bits(out)[0, 2, 3]) == 0 and int(K.bits(out)[1, 2, 3]) == 0, "-0.0 and NaN at a group edge become +0.0"
    assert not bool(torch.isnan(out).any()) and not out[:, torch.arange(5), torch.arange(5)].any()
    assert int(K.bits(out)[5, 1, 2]) == int(K.bits(mats)[5, 1, 2]) != 0 and float(out[5, 1, 2]) < 1e-38   # the subnormal
    assert float(out[5, 3, 0]) == INF
    for s in range(8):
        ei, _ = D.host_edges(out[s], 0.0)
        assert bool(E[ei[0], ei[1]].all()), "a subject's edges are a subset of the group's"
    # every form of the choice gives a set inside the positive group entries, off the diagonal
    G5 = G.host_group(G.correlations(6, 20), "mean")
    for choice in (dict(keep=0.2), dict(num_edges=30), dict(min_weight=torch.tensor([0.05])), dict(knn=3),
                   dict(knn=3, knn_mode="mutual"), dict(backbone="mst"), dict(keep=0.1, backbone="mst"),
                   dict(knn=2, knn_mode="directed", backbone="mst")):
        E = G.host_edge_set(G5, **choice)
        assert bool(E.any()) and not bool((E & ~K.candidates(G5)).any()), choice


def _mats(n=5, S=3):
    return D.recipe(n)[:S].contiguous()


def test_group_matrix_checks_its_arguments_before_the_device():
    m = _mats()
    assert ingest.GROUP_STATISTICS == ("mean", "fisher_mean", "consistency") == G.STATISTICS
    assert not {"group_matrix", "group_sparsify", "GROUP_STATISTICS"} & set(connectome_gnn_amd.__all__)
    for bad in ("median", "MEAN", 0, None):
        with pytest.raises(ValueError, match=r"GROUP_STATISTICS = \('mean', 'fisher_mean', 'consistency'\)"):
            ingest.group_matrix(m, bad)
    for stat in ("mean", "fisher_mean"):
        for given in (dict(keep=0.1), dict(num_edges=3), dict(min_weight=0.0)):
            with pytest.raises(ValueError, match="takes none of them"):
                ingest.group_matrix(m, stat, **given)
    with pytest.raises(ValueError, match="give exactly one of keep=, num_edges= and min_weight="):
        ingest.group_matrix(m, "consistency")
    with pytest.raises(ValueError, match="give exactly one of keep=, num_edges= and min_weight="):
        ingest.group_matrix(m, "consistency", keep=0.1, min_weight=0.0)
    with pytest.raises(ValueError, match=r"min_weight tensor must be floating point \[S\] = \[3\]"):
        ingest.group_matrix(m, "consistency", min_weight=torch.zeros(1))
    with pytest.raises(TypeError, match="among must be bool"):
        ingest.group_matrix(m, among=torch.ones(3))
    with pytest.raises(TypeError, match="among must be bool"):
        ingest.group_matrix(m, among=torch.ones(3, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"among must be \[S\] = \[3\]"):
        ingest.group_matrix(m, among=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"among must be \[S\] = \[3\]"):
        ingest.group_matrix(m, among=torch.ones(3, 1, dtype=torch.bool))
    with pytest.raises(TypeError, match="among must be a torch.Tensor"):
        ingest.group_matrix(m, among=[True, True, False])
    with pytest.raises(TypeError, match="float32"):
        ingest.group_matrix(m.double())
    with pytest.raises(ValueError, match=r"\[S, n, n\]"):
        ingest.group_matrix(m[0])
    # valid arguments on CPU tensors get as far as the residency check, and no further
    for args, kw in ((("mean",), {}), (("fisher_mean",), dict(among=torch.ones(3, dtype=torch.bool))),
                     (("consistency",), dict(keep=0.1)), (("consistency",), dict(min_weight=torch.zeros(3))), ((), {})):
        with pytest.raises(RuntimeError, match="ROCm"):
            ingest.group_matrix(m, *args, **kw)


def _entry_points():
    m, y = _mats(), D.labels(3)
    ts = torch.randn(6, 40, 5, generator=torch.Generator().manual_seed(4))
    return {"group_sparsify": lambda group, **kw: ingest.group_sparsify(m, group, **kw),
            "from_matrices": lambda group, **kw: ingest.from_matrices(m, y, group=group, **kw),
            "node_measures": lambda group, **kw: ingest.node_measures(m, group=group, **kw),
            "module_profile": lambda group, **kw: ingest.module_profile(m, [0, 0, 1, 1, 1], group=group, **kw),
            "path_lengths": lambda group, **kw: ingest.path_lengths(m, group=group, **kw),
            "centrality_measures": lambda group, **kw: ingest.centrality_measures(m, group=group, **kw),
            "from_timeseries": lambda group, **kw: ingest.from_timeseries(ts, D.labels(6), group=group, **kw)}


@pytest.mark.parametrize("name", ["group_sparsify", "from_matrices", "node_measures", "module_profile", "path_lengths",
                                  "centrality_measures", "from_timeseries"])
def test_group_of_every_entry_point(name):
    call = _entry_points()[name]
    with pytest.raises(ValueError, match='group="consistency" needs a threshold choice of its own'):
        call("consistency", keep=0.1)
    for bad in ("median", "Mean"):
        with pytest.raises(ValueError, match="GROUP_STATISTICS"):
            call(bad, keep=0.1)
    for bad in (1, 0.5, True, np.zeros((5, 5), dtype=np.float32)):
        with pytest.raises(TypeError, match="group must be one of"):
            call(bad, keep=0.1)
    with pytest.raises(TypeError, match="a group tensor must be float32"):
        call(torch.zeros(5, 5, dtype=torch.float64), keep=0.1)
    for shape in ((5, 4), (25,), (1, 5, 5), (6, 6)):
        with pytest.raises(ValueError, match=r"a group tensor must be \[n, n\] = \[5, 5\]"):
            call(torch.zeros(shape), keep=0.1)
    with pytest.raises(ValueError, match="a group tensor must be contiguous"):
        call(torch.zeros(5, 10)[:, ::2], keep=0.1)
    # the choice is the group matrix's, a cohort of one unit, and validated by the same plan
    for units in (3, 6, 2):
        with pytest.raises(ValueError, match=r"min_weight tensor must be floating point \[the group matrix\] = \[1\]"):
            call("mean", min_weight=torch.zeros(units))
    with pytest.raises(ValueError, match="give exactly one of keep=, num_edges= and min_weight="):
        call("mean")
    with pytest.raises(ValueError, match="give exactly one of keep=, num_edges= and min_weight="):
        call("mean", keep=0.1, num_edges=3)
    with pytest.raises(ValueError, match="knn= is a fourth way"):
        call("mean", knn=2, keep=0.1)
    with pytest.raises(ValueError, match=r"BACKBONES = \('mst',\)"):
        call("mean", keep=0.1, backbone="tree")
    with pytest.raises(ValueError, match=r"keep must lie in \[0, 1\]"):
        call("fisher_mean", keep=1.5)
    for group in ("mean", "fisher_mean", torch.zeros(5, 5)):
        for kw in (dict(keep=0.1), dict(num_edges=4), dict(min_weight=0.2), dict(min_weight=torch.zeros(1)),
                   dict(knn=2), dict(knn=2, knn_mode="mutual"), dict(backbone="mst"), dict(keep=0.1, backbone="mst"),
                   dict(knn=2, backbone="mst")):
            with pytest.raises(RuntimeError, match="ROCm"):
                call(group, **kw)


def test_group_sparsify_checks_its_own_arguments():
    m = _mats()
    with pytest.raises(TypeError, match="group must be one of"):
        ingest.group_sparsify(m, None, keep=0.1)
    with pytest.raises(ValueError, match="out must be"):
        ingest.group_sparsify(m, keep=0.1, out=torch.empty(3, 5, 4))
    with pytest.raises(TypeError, match="out must be float32"):
        ingest.group_sparsify(m, keep=0.1, out=torch.empty(3, 5, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be contiguous"):
        ingest.group_sparsify(m, keep=0.1, out=torch.empty(3, 5, 5).transpose(1, 2))
    with pytest.raises(RuntimeError, match="ROCm"):
        ingest.group_sparsify(m, keep=0.1, out=m.clone())               # group defaults to "mean"
    # without group= the six entry points check what they always checked
    with pytest.raises(ValueError, match=r"min_weight tensor must be floating point \[S\] = \[3\]"):
        ingest.node_measures(m, min_weight=torch.zeros(1))
    with pytest.raises(RuntimeError, match="ROCm"):
        ingest.node_measures(m, min_weight=torch.zeros(3))


def test_the_prototypes_match_their_header_type_by_type():
    """The three entry points are declared in include/cgnn_group.h, which cgnn.h includes, and bound by
    ``_lib.GROUP_PROTOTYPES``: every type, the library's exports, the constants, and the comparison itself against a
    doctored header."""
    hdr = check_header("cgnn_group.h", _lib.GROUP_PROTOTYPES,
                       ["cgnn_ingest_group_workspace_bytes", "cgnn_ingest_group", "cgnn_ingest_group_mask"],
                       [("int64_t S, int32_t n)", "int32_t S, int32_t n)"), ("int32_t statistic, ", ""),
                        ("const float* group /* [n, n] */,", "")])
    assert len(_lib.PROTOTYPES) == 127, "the main table is as it was"
    for line in ("#define CGNN_GROUP_MEAN 0\n", "#define CGNN_GROUP_FISHER_MEAN 1\n", "#define CGNN_GROUP_CONSISTENCY 2\n",
                 f"#define CGNN_GROUP_SLICE {_lib.GROUP_SLICE}\n"):
        assert line in hdr, line
    assert (_lib.GROUP_MEAN, _lib.GROUP_FISHER_MEAN, _lib.GROUP_CONSISTENCY) == (0, 1, 2)
    assert [ingest.GROUP_STATISTICS.index(s) for s in ingest.GROUP_STATISTICS] == [0, 1, 2] and G.SLICE == _lib.GROUP_SLICE
    assert _lib.ABI_VERSION == 2, "the change is additive"


def test_the_entry_points_refuse_before_any_launch():
    """No device is present here: a call that went as far as a launch could not return these codes."""
    lib = _lib.load()
    fn, mask, query = lib.cgnn_ingest_group, lib.cgnn_ingest_group_mask, lib.cgnn_ingest_group_workspace_bytes
    S, n = 130, 21
    a, b, w, t, m, g = 1 << 20, 1 << 24, 1 << 28, 1 << 30, 1 << 31, 1 << 32    # addresses that nothing dereferences
    slices = -(-S // _lib.GROUP_SLICE)
    need = query(S, n)
    assert need == -(-(slices * n * n + slices) * 8 // 16) * 16, "the partials and the counts, rounded up to 16 bytes"
    assert query(0, n) == 0 and query(1, 1) == 16
    assert query(_lib.GROUP_SLICE, n) == query(1, n) < query(_lib.GROUP_SLICE + 1, n)
    for bad in ((-1, n), (S, 0), (S, -3), (2 ** 31 // n + 1, n), (1, 46341)):
        assert query(*bad) == _lib.CGNN_EINVAL, bad
    out_bytes = 4 * n * n
    good = [a, S, n, _lib.GROUP_MEAN, None, m, w, need, b, out_bytes, None]

    def rc(at, v, base=good):
        return fn(*(base[:at] + [v] + base[at + 1:]))

    for at, v in ((0, None), (8, None), (6, None), (0, a + 2), (8, b + 1), (6, w + 8), (1, -1), (2, 0), (2, -5),
                  (3, 3), (3, -1), (4, t), (9, out_bytes - 1), (7, need - 1), (7, 0), (1, 2 ** 31 // n + 1),
                  (8, a + 4), (8, a + 4 * S * n * n - 4), (8, a - 4),                 # out overlaps matrices
                  (6, a), (6, b - need + 16), (6, b + out_bytes - 16), (5, b + 4), (5, b - S + 1)):
        assert rc(at, v) == _lib.CGNN_EINVAL, (at, v)
    consistency = good[:3] + [_lib.GROUP_CONSISTENCY, t] + good[5:]
    assert rc(4, None, consistency) == _lib.CGNN_EINVAL, "the consistency needs the thresholds"
    assert rc(4, t + 2, consistency) == _lib.CGNN_EINVAL and rc(4, b, consistency) == _lib.CGNN_EINVAL
    # the mask
    nbytes = 4 * S * n * n
    good = [a, S, n, g, t, b, nbytes, None]

    def rcm(at, v):
        return mask(*(good[:at] + [v] + good[at + 1:]))

    for at, v in ((0, None), (3, None), (4, None), (5, None), (0, a + 2), (3, g + 1), (4, t + 2), (5, b + 3), (1, -1),
                  (2, 0), (2, -5), (6, nbytes - 1), (6, 0), (1, 2 ** 31 // n + 1),
                  (5, a + 4 * n * n), (5, a - 4), (5, a + nbytes - 4),              # out overlaps matrices
                  (3, b), (3, b + nbytes - 4), (3, b - 4 * n * n + 4), (4, b), (4, b + nbytes - 4)):
        assert rcm(at, v) == _lib.CGNN_EINVAL, (at, v)
    assert rcm(1, 0) == _lib.CGNN_OK and mask(None, 0, n, None, None, None, 0, None) == _lib.CGNN_OK


def test_a_common_topology_on_the_seeded_cohort():
    """12 subjects, 120 frames, 84 ROIs in 4 modules, series ``0.6 * module signal + noise``, Pearson correlation,
    ``keep=0.10`` (rank 697).  The subjects' own edge sets overlap by a quarter and share no edge; the cohort mean at the
    same rank keeps 696 entries, and every subject carries at least 694 of them as positive weights."""
    mats = G.modular_series_cohort()
    S, n = mats.shape[0], mats.shape[1]
    assert (S, n) == (12, 84) and D.rank_of(n, keep=0.10) == 697
    own = torch.stack([G.host_edge_set(A, keep=0.10) for A in mats])
    overlap = [G.jaccard(a, b) for a, b in itertools.combinations(own, 2)]
    assert max(overlap) < 0.34 and 0.2 < sum(overlap) / len(overlap) < 0.3
    assert int(own.all(0).sum()) == 0, "no edge is present in all 12 subjects"
    assert int((own.float().mean(0) > 0.6).sum()) < 150
    E = G.host_edge_set(G.host_group(mats, "mean"), keep=0.10)
    assert int(E.sum()) == 696
    masked = G.host_group_sparsify(mats, "mean", keep=0.10)
    kept = [(masked[s] != 0).sum().item() for s in range(S)]
    assert min(kept) >= 694 and max(kept) <= 696
    shared = torch.stack([masked[s] != 0 for s in range(S)])
    assert min(G.jaccard(a, b) for a, b in itertools.combinations(shared, 2)) > 0.99
