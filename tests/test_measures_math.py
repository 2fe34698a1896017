"""connectome_gnn_amd.ingest.node_measures without a GPU: its fp64 host statement (tests/measures_data.py) against
networkx and against ``small_world_stats``, the tile algebra of csrc/measures.hip in numpy, and every refusal of
``node_measures`` / ``from_matrices(measures=...)`` / ``from_timeseries(measures=...)``."""
import numpy as np
import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import ingest
from connectome_gnn_amd.synthetic import small_world_stats
from tests import ingest_data as I
from tests import measures_data as M

SYMMETRIC_FINITE = (0, 1, 2, 4)          # recipe subjects with A == A^T and no kept +inf


def test_the_names_are_the_statement_s():
    assert ingest.MEASURES == M.MEASURES == ("strength", "degree", "mean_weight", "clustering", "weighted_clustering")


@pytest.mark.parametrize("n", [20, 84])
@pytest.mark.parametrize("keep", [0.1, 0.5])
def test_statement_against_networkx(n, keep):
    nx = pytest.importorskip("networkx")
    mats = M.recipe(n)
    k = M.rank_of(n, keep=keep)
    for s in SYMMETRIC_FINITE:
        A = mats[s]
        t = M.host_threshold(A, k)
        a, b, _ = M.value_maps(A, t)
        assert (b == b.T).all()
        G = nx.from_numpy_array(a)                     # zero entries are no edges
        assert G.number_of_edges() * 2 == int(b.sum())
        want_b = np.array([v for _, v in sorted(nx.clustering(G).items())])
        want_w = np.array([v for _, v in sorted(nx.clustering(G, weight="weight").items())])
        got = M.host_measures(A, t, ("clustering", "weighted_clustering")).numpy()
        assert np.abs(got[:, 0] - want_b).max() <= 1e-12, (s, "binary")
        assert np.abs(got[:, 1] - want_w).max() <= 1e-12, (s, "weighted")
        deg = np.array([d for _, d in sorted(G.degree())])
        assert np.array_equal(M.host_counts(A, t)[0].numpy(), deg)
        assert np.array_equal(M.host_measures(A, t, ("degree",)).numpy()[:, 0], deg / (n - 1))


@pytest.mark.filterwarnings("ignore:Mean of empty slice")          # the path length of the subject without edges
@pytest.mark.parametrize("n", [20, 84])
@pytest.mark.parametrize("keep", [0.1, 0.5])
def test_binary_clustering_is_small_world_stats_on_unit_weights(n, keep):
    mats = M.recipe(n)
    k = M.rank_of(n, keep=keep)
    for s in SYMMETRIC_FINITE:
        A = mats[s]
        t = M.host_threshold(A, k)
        ei, w = I.host_edges(A, t)
        g = C.ConnectomeGraph(torch.zeros(n, 1), ei, torch.ones_like(w), torch.tensor(0), "sub")
        mean = float(M.host_measures(A, t, ("clustering",)).mean())
        assert abs(mean - small_world_stats([g])["mean_clustering"]) <= 1e-12, s


@pytest.mark.parametrize("n", [5, 96, 97, 200])
@pytest.mark.parametrize("symmetric", [True, False])
def test_upper_tile_pairs_and_mirrored_column_sums_give_T(n, symmetric):
    g = np.random.default_rng(n)
    V = g.random((n, n)) * (g.random((n, n)) < 0.3)
    if symmetric:
        V = np.maximum(V, V.T)
    np.fill_diagonal(V, 0.0)
    want = np.einsum("ki,kj,ij->i", V, V, V)
    got, written = M.tiled_triangles(V)
    assert (written == 1).all(), "every slot [b][i] is written exactly once"
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, want.max())
    assert np.abs(M.triangles(V) - want).max() <= 1e-12 * max(1.0, want.max())
    if symmetric:
        assert np.abs(want - np.diag(V @ V @ V)).max() <= 1e-12 * max(1.0, want.max())
    B = (V > 0).astype(np.int64)
    got_b, _ = M.tiled_triangles(B)
    assert np.array_equal(got_b, np.einsum("ki,kj,ij->i", B, B, B)) and got_b.max() < 2 ** 24


def test_statement_edge_cases():
    mats = M.recipe(20)
    zeros = M.host_measures(mats[2], M.host_threshold(mats[2], 38))
    assert torch.equal(zeros, torch.zeros(20, 5, dtype=torch.float64)), "a subject without edges"
    assert torch.equal(M.host_measures(mats[0], float("inf")), torch.zeros(20, 5, dtype=torch.float64))
    assert torch.equal(M.host_measures(torch.ones(1, 1), -1.0), torch.zeros(1, 5, dtype=torch.float64)), "n = 1"
    tri = torch.tensor([[0.0, 2.0, 1.0], [2.0, 0.0, 0.5], [1.0, 0.5, 0.0]])
    m = M.host_measures(tri, 0.0)
    assert torch.equal(m[:, 1], torch.ones(3, dtype=torch.float64)) and torch.equal(m[:, 3], m[:, 1])
    # one triangle: T_i(u) = 2 u01 u02 u12 with u = cbrt(w / 2), over k (k - 1) = 2
    assert torch.allclose(m[:, 4], torch.full((3,), float(np.cbrt(1.0 * 0.5 * 0.25)), dtype=torch.float64), atol=1e-15)
    assert torch.allclose(m[:, 2], torch.tensor([1.5, 1.25, 0.75], dtype=torch.float64), atol=1e-7)
    # NaN entries are never edges; the +inf of subject 6 reaches the weight-valued measures only
    s5, s6 = mats[4], mats[5]
    assert not M.kept_mask(s5, -float("inf"))[0, 1] and M.finite_weights(s5, -float("inf"))
    assert not M.finite_weights(s6, 0.5)
    m6 = M.host_measures(s6, 0.5)
    assert bool(torch.isfinite(m6[:, 1]).all()) and bool(torch.isfinite(m6[:, 3]).all())
    assert not bool(torch.isfinite(m6[:, 2]).all())
    # asymmetric: the formula is the definition, and is not bounded by 1
    asym = torch.tensor([[0.0, 1.0, 1.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 0.0], [1.0, 1.0, 1.0, 0.0]])
    k, T = M.host_counts(asym, 0.0)
    B = (asym > 0).long().numpy()
    assert T.tolist() == np.einsum("ki,kj,ij->i", B, B, B).tolist() and k.tolist() == [2, 1, 1, 3]


def test_measure_names_are_refused():
    m, y = M.recipe(5), I.labels(6)
    for bad, exc, msg in (((), ValueError, "empty"), ([], ValueError, "empty"),
                          (("strength", "betweenness"), ValueError, "unknown measure"),
                          (("degree", "strength", "degree"), ValueError, "named twice"),
                          ("degree", TypeError, "tuple of names"), (3, TypeError, "tuple of names")):
        with pytest.raises(exc, match=msg):
            ingest.node_measures(m, keep=0.1, measures=bad)
        with pytest.raises(exc, match=msg):
            ingest.from_matrices(m, y, keep=0.1, measures=bad)
        with pytest.raises(exc, match=msg):
            ingest.from_timeseries(torch.zeros(6, 4, 5), y, keep=0.1, measures=bad)


def test_measures_with_node_features_are_refused():
    m, y = M.recipe(5), I.labels(6)
    for measures in (True, ("degree",)):
        with pytest.raises(ValueError, match="either measures= or node_features="):
            ingest.from_matrices(m, y, keep=0.1, measures=measures, node_features=I.features(6, 5))
        with pytest.raises(ValueError, match="either measures= or node_features="):
            ingest.from_timeseries(torch.zeros(6, 4, 5), y, keep=0.1, measures=measures,
                                   node_features=I.features(6, 5))


def test_node_measures_threshold_arguments_are_refused():
    m = M.recipe(5)
    for kw in ({}, {"keep": 0.1, "num_edges": 3}, {"keep": 0.1, "min_weight": 0.2},
               {"keep": 0.1, "num_edges": 3, "min_weight": 0.2}):
        with pytest.raises(ValueError, match="exactly one"):
            ingest.node_measures(m, **kw)
    for keep in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"keep must lie in \[0, 1\]"):
            ingest.node_measures(m, keep=keep)
    with pytest.raises(ValueError, match="num_edges must be >= 0"):
        ingest.node_measures(m, num_edges=-1)
    with pytest.raises(TypeError, match="num_edges must be an int"):
        ingest.node_measures(m, num_edges=2.5)
    for bad in (torch.zeros(5), torch.zeros(6, 1), torch.zeros(6, dtype=torch.long)):
        with pytest.raises(ValueError, match="min_weight tensor"):
            ingest.node_measures(m, min_weight=bad)
    with pytest.raises(TypeError, match="float32"):
        ingest.node_measures(m.double(), keep=0.1)
    with pytest.raises(ValueError, match=r"\[S, n, n\]"):
        ingest.node_measures(m[0], keep=0.1)
    with pytest.raises(ValueError, match="contiguous"):
        ingest.node_measures(m.transpose(1, 2), keep=0.1)


def test_cpu_tensors_are_refused():
    m, y = M.recipe(5), I.labels(6)
    for kw in ({"keep": 0.1}, {"num_edges": 3}, {"min_weight": 0.5}, {"min_weight": torch.zeros(6)}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ingest.node_measures(m, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ingest.node_measures(m, measures=("clustering",), **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ingest.from_matrices(m, y, measures=True, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.from_timeseries(torch.zeros(6, 4, 5), y, keep=0.1, measures=True)
