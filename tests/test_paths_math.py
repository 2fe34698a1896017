"""The shortest-path node measures of connectome_gnn_amd.ingest without a GPU: their fp64 host statement
(tests/paths_data.py) against networkx, against ``small_world_stats`` and against closed forms on structured graphs,
and every refusal of a request that names them."""
import numpy as np
import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import ingest
from connectome_gnn_amd.synthetic import small_world_stats
from tests import ingest_data as I
from tests import measures_data as M
from tests import paths_data as P

SYMMETRIC = (0, 1, 2, 4, 5)              # recipe subjects with a symmetric kept set (weights play no part)
ASYMMETRIC = 3
COL = {name: c for c, name in enumerate(P.PATH_MEASURES)}


def test_the_names_are_the_statement_s():
    assert ingest.PATH_MEASURES == P.PATH_MEASURES == ("nodal_efficiency", "closeness", "eccentricity",
                                                       "local_efficiency")
    assert ingest.MEASURES == M.MEASURES, "measures=True keeps meaning these five"
    assert ingest.PATH_MAX_NODES == 1024


def _against_networkx(nx, mask, what):
    n = mask.shape[0]
    assert (mask == mask.T).all(), what
    G = nx.from_numpy_array(mask.astype(np.int64))
    got = P.mask_measures(mask).numpy()
    close = nx.closeness_centrality(G, wf_improved=True)
    assert np.abs(got[:, COL["closeness"]] - np.array([close[v] for v in range(n)])).max() <= 1e-12, what
    local = np.array([nx.global_efficiency(G.subgraph(G[v])) for v in range(n)])
    assert np.abs(got[:, COL["local_efficiency"]] - local).max() <= 1e-12, what
    assert abs(got[:, COL["nodal_efficiency"]].mean() - nx.global_efficiency(G)) <= 1e-12, what
    # (networkx forms the same n subgraph efficiencies again for its mean: on the small graphs only)
    mean = nx.local_efficiency(G) if G.number_of_edges() < 1000 else local.mean()
    assert abs(got[:, COL["local_efficiency"]].mean() - mean) <= 1e-12, what
    lengths = dict(nx.all_pairs_shortest_path_length(G))
    ecc = np.array([max(lengths[v].values()) for v in range(n)])     # over the reachable nodes
    assert np.array_equal(got[:, COL["eccentricity"]], ecc / (n - 1)), what
    assert got.min() >= 0.0 and got.max() <= 1.0, what


@pytest.mark.parametrize("n", [20, 84])
@pytest.mark.parametrize("keep", [0.1, 0.5])
def test_statement_against_networkx_on_the_recipe(n, keep):
    nx = pytest.importorskip("networkx")
    mats = P.recipe(n)
    k = P.rank_of(n, keep=keep)
    for s in SYMMETRIC:
        _against_networkx(nx, M.kept_mask(mats[s], P.host_threshold(mats[s], k)), (n, keep, s))


@pytest.mark.parametrize("n", [5, 64, 65])
def test_statement_against_networkx_on_the_structured_graphs(n):
    nx = pytest.importorskip("networkx")
    for kind in P.STRUCTURED:
        if kind != "directed_path":
            _against_networkx(nx, M.kept_mask(P.structured(kind, n), 0.0), (kind, n))


@pytest.mark.parametrize("n", [20, 84])
@pytest.mark.parametrize("keep", [0.1, 0.5])
def test_asymmetric_closeness_is_networkx_s_on_the_reversed_graph(n, keep):
    nx = pytest.importorskip("networkx")
    A = P.recipe(n)[ASYMMETRIC]
    mask = M.kept_mask(A, P.host_threshold(A, P.rank_of(n, keep=keep)))
    assert (mask != mask.T).any()
    G = nx.from_numpy_array(mask.astype(np.int64), create_using=nx.DiGraph)
    assert G.number_of_edges() == int(mask.sum())
    close = nx.closeness_centrality(G.reverse(), wf_improved=True)
    got = P.mask_measures(mask, ("closeness",)).numpy()[:, 0]
    assert np.abs(got - np.array([close[v] for v in range(n)])).max() <= 1e-12
    D = P.distances(mask)
    lengths = dict(nx.all_pairs_shortest_path_length(G))
    for i in range(n):
        for j in range(n):
            assert D[i, j] == lengths[i].get(j, -1), "d_ij runs along the out-neighbours of row i"


@pytest.mark.filterwarnings("ignore:Mean of empty slice")
@pytest.mark.parametrize("n", [20, 84])
@pytest.mark.parametrize("keep", [0.1, 0.5])
def test_first_twenty_sources_are_small_world_stats_on_unit_weights(n, keep):
    mats = P.recipe(n)
    k = P.rank_of(n, keep=keep)
    for s in range(6):
        A = mats[s]
        t = P.host_threshold(A, k)
        ei, w = I.host_edges(A, t)
        if ei.shape[1] == 0:
            continue
        g = C.ConnectomeGraph(torch.zeros(n, 1), ei, torch.ones_like(w), torch.tensor(0), "sub")
        D = P.distances(M.kept_mask(A, t))[:min(20, n)]
        assert abs(float(D[D > 0].mean()) - small_world_stats([g])["mean_avg_path_length"]) <= 1e-12, s


@pytest.mark.parametrize("n", [5, 64, 65, 130])
def test_closed_forms(n):
    i = np.arange(n)
    # ring: 2 nodes at every distance below n / 2, one more at n / 2 when n is even
    m = P.mask_measures(M.kept_mask(P.structured("ring", n), 0.0)).numpy()
    half = (n - 1) // 2
    inv = 2 * sum(1.0 / d for d in range(1, half + 1)) + (2.0 / n if n % 2 == 0 else 0.0)
    total = 2 * sum(range(1, half + 1)) + (n // 2 if n % 2 == 0 else 0)
    assert np.abs(m[:, COL["nodal_efficiency"]] - inv / (n - 1)).max() <= 1e-12
    assert np.abs(m[:, COL["closeness"]] - (n - 1) / total).max() <= 1e-12
    assert np.array_equal(m[:, COL["eccentricity"]], np.full(n, (n // 2) / (n - 1)))
    assert np.array_equal(m[:, COL["local_efficiency"]], np.zeros(n)), "a ring's neighbours are not adjacent"
    # directed path: node i reaches i + 1 .. n - 1, the last node nothing; one out-neighbour: no local efficiency
    mask = M.kept_mask(P.structured("directed_path", n), 0.0)
    r, sum_d, ecc = P.exact_integers(P.distances(mask))
    assert np.array_equal(r, n - 1 - i) and np.array_equal(ecc, n - 1 - i)
    assert np.array_equal(sum_d, (n - 1 - i) * (n - i) // 2)
    m = P.mask_measures(mask).numpy()
    assert m[n - 1].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert np.array_equal(m[:, COL["local_efficiency"]], np.zeros(n))
    # undirected path: diameter n - 1, and sum d of an end node is the largest possible, n (n - 1) / 2
    r, sum_d, ecc = P.exact_integers(P.distances(M.kept_mask(P.structured("path", n), 0.0)))
    assert np.array_equal(ecc, np.maximum(i, n - 1 - i)) and int(sum_d.max()) == n * (n - 1) // 2 < 2 ** 24
    assert np.array_equal(sum_d, (i * (i + 1) + (n - 1 - i) * (n - i)) // 2)
    # star: the hub at distance 1 of all, the leaves at 1 of the hub and 2 of each other
    m = P.mask_measures(M.kept_mask(P.structured("star", n), 0.0)).numpy()
    assert m[0].tolist() == [1.0, 1.0, 1.0 / (n - 1), 0.0]
    leaf = [(1.0 + (n - 2) / 2.0) / (n - 1), (n - 1) / (1.0 + 2.0 * (n - 2)), 2.0 / (n - 1), 0.0]
    assert np.abs(m[1:] - np.array(leaf)).max() <= 1e-12
    # complete: everything at distance 1
    m = P.mask_measures(M.kept_mask(P.structured("complete", n), 0.0)).numpy()
    assert np.array_equal(m, np.stack([np.ones(n), np.ones(n), np.full(n, 1.0 / (n - 1)), np.ones(n)], 1))
    # two cliques of a and b nodes and an isolated node
    m = P.mask_measures(M.kept_mask(P.structured("cliques", n), 0.0)).numpy()
    a = (n - 1) // 2
    for lo, size in ((0, a), (a, n - 1 - a)):
        want = [(size - 1) / (n - 1), (size - 1) / (n - 1), (1.0 if size > 1 else 0.0) / (n - 1),
                1.0 if size > 2 else 0.0]
        assert np.abs(m[lo:lo + size] - np.array(want)).max() <= 1e-12
    assert m[n - 1].tolist() == [0.0, 0.0, 0.0, 0.0], "the isolated node"


def test_statement_edge_cases():
    mats = P.recipe(20)
    zeros = torch.zeros(20, 4, dtype=torch.float64)
    assert torch.equal(P.host_measures(mats[2], P.host_threshold(mats[2], 38)), zeros), "a subject without edges"
    assert torch.equal(P.host_measures(mats[0], float("inf")), zeros)
    assert torch.equal(P.host_measures(torch.ones(1, 1), -1.0), torch.zeros(1, 4, dtype=torch.float64)), "n = 1"
    # NaN entries are never edges; a kept +inf is an ordinary edge
    s6 = mats[5]
    assert M.kept_mask(s6, 0.5)[0, 3] and bool(torch.isfinite(P.host_measures(s6, 0.5)).all())
    assert not M.kept_mask(mats[4], -float("inf"))[0, 1]
    # both kinds of subject occur at keep 0.1: unreachable pairs at n = 20, none at n = 84
    for n, lo, hi in ((20, 140, 173), (84, 0, 0)):
        k = P.rank_of(n, keep=0.1)
        for s in (0, 3, 4, 5):
            A = P.recipe(n)[s]
            assert lo <= P.unreachable_pairs(A, P.host_threshold(A, k)) <= hi, (n, s)
    # level counts: row sums are r_i + 1, and they carry the three integers
    A = P.recipe(20)[3]
    D = P.distances(M.kept_mask(A, P.host_threshold(A, P.rank_of(20, keep=0.1))))
    counts = P.level_counts(D)
    r, sum_d, ecc = P.exact_integers(D)
    lv = np.arange(counts.shape[1])
    assert np.array_equal(counts[:, 0], np.ones(20, dtype=np.int64)) and np.array_equal(counts.sum(1), r + 1)
    assert np.array_equal((counts * lv).sum(1), sum_d)
    assert np.array_equal(np.where(counts > 0, lv, 0).max(1), ecc)


def test_measure_names_are_refused_in_mixed_requests():
    m, y = P.recipe(5), I.labels(6)
    for bad, exc, msg in (((), ValueError, "empty"),
                          (("closeness", "betweenness"), ValueError, "unknown measure"),
                          (("betweenness",), ValueError, "unknown measure"),
                          (("degree", "closeness", "strength", "closeness"), ValueError, "named twice"),
                          (("local_efficiency", "degree", "degree"), ValueError, "named twice"),
                          ("closeness", TypeError, "tuple of names")):
        with pytest.raises(exc, match=msg):
            ingest.node_measures(m, keep=0.1, measures=bad)
        with pytest.raises(exc, match=msg):
            ingest.from_matrices(m, y, keep=0.1, measures=bad)
        with pytest.raises(exc, match=msg):
            ingest.from_timeseries(torch.zeros(6, 4, 5), y, keep=0.1, measures=bad)
    with pytest.raises(ValueError, match="either measures= or node_features="):
        ingest.from_matrices(m, y, keep=0.1, measures=("closeness",), node_features=I.features(6, 5))


def test_more_than_1024_nodes_are_refused_for_path_measures_only():
    big, y = torch.zeros(1, 1025, 1025), I.labels(1)
    for names in (("eccentricity",), ("degree", "local_efficiency"), P.PATH_MEASURES):
        with pytest.raises(ValueError, match="n <= 1024"):
            ingest.node_measures(big, keep=0.1, measures=names)
        with pytest.raises(ValueError, match="n <= 1024"):
            ingest.from_matrices(big, y, keep=0.1, measures=names)
        with pytest.raises(ValueError, match="n <= 1024"):
            ingest.from_timeseries(torch.zeros(1, 4, 1025), y, keep=0.1, measures=names)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # the five have no such limit
        ingest.node_measures(big, keep=0.1, measures=("degree",))
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # 1024 itself is taken
        ingest.node_measures(torch.zeros(1, 1024, 1024), keep=0.1, measures=P.PATH_MEASURES)


def test_cpu_tensors_are_refused():
    m, y = P.recipe(5), I.labels(6)
    for names in (P.PATH_MEASURES, ("closeness",), ("strength", "local_efficiency", "clustering")):
        for kw in ({"keep": 0.1}, {"num_edges": 3}, {"min_weight": 0.5}, {"min_weight": torch.zeros(6)}):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                ingest.node_measures(m, measures=names, **kw)
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                ingest.from_matrices(m, y, measures=names, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ingest.from_timeseries(torch.zeros(6, 4, 5), y, keep=0.1, measures=names)
