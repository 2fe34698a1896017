"""connectome_gnn_amd.ingest without a GPU: the properties of its host statement (tests/ingest_data.py) on the
seeded recipes, the rank formula, and every refusal of ``from_matrices`` / ``select_thresholds``."""
import pytest
import torch

from connectome_gnn_amd import ingest
from tests import ingest_data as D

KEEPS = (0.0, 0.1, 0.29, 0.5, 1.0)
SYMMETRIC = (0, 1, 2, 4, 5)              # recipe subjects with A == A^T (NaN positions included)


def _edges(n, k):
    mats = D.recipe(n)
    return mats, [D.host_edges(A, D.host_threshold(A, k)) for A in mats]


@pytest.mark.parametrize("n", [5, 20, 84])
@pytest.mark.parametrize("keep", KEEPS)
def test_statement_properties(n, keep):
    k = D.rank_of(n, keep=keep)
    mats, edges = _edges(n, k)
    for s, (A, (ei, w)) in enumerate(zip(mats, edges)):
        e = ei.shape[1]
        assert e <= k and w.shape == (e,) and ei.dtype == torch.long
        assert bool((ei[0] != ei[1]).all()), "no diagonal edge"
        assert bool((w > 0).all()) and not bool(torch.isnan(w).any()), "no NaN or non-positive edge"
        assert torch.equal(w, A[ei[0], ei[1]])
        flat = ei[0] * n + ei[1]
        assert bool((flat[1:] > flat[:-1]).all()), "row-major order, no edge twice"
        if s in SYMMETRIC:
            back = torch.sort(ei[1] * n + ei[0]).values
            assert torch.equal(back, flat), "symmetric input gives a symmetric edge set"


@pytest.mark.parametrize("keep", KEEPS)
def test_rank_formula_and_recipe_counts(keep):
    n = 84
    k = ingest._rank(n, keep, None)
    assert k == D.rank_of(n, keep=keep) == {0.0: 0, 0.1: 697, 0.29: 2022, 0.5: 3486, 1.0: 6972}[keep]
    assert ingest._rank(n, None, k) == k
    _, edges = _edges(n, k)
    counts = [w.numel() for _, w in edges]
    assert all(c <= k for c in counts)
    if keep in D.COUNTS_84:
        assert counts == D.COUNTS_84[keep]
    if keep == 0.0:
        assert counts == [0] * 6


def test_threshold_of_nan_and_of_ranks_beyond_the_candidates():
    A = torch.tensor([[9.0, float("nan"), 2.0], [1.0, 9.0, float("nan")], [3.0, -1.0, 9.0]])
    # candidates, descending: 3, 2, 1, -1, -inf (NaN), -inf (NaN)
    assert [D.host_threshold(A, k) for k in range(8)] == [3.0, 2.0, 1.0, -1.0, -D.INF, -D.INF, -D.INF, -D.INF]
    ei, w = D.host_edges(A, D.host_threshold(A, 6))
    assert ei.tolist() == [[0, 1, 2], [2, 0, 0]] and w.tolist() == [2.0, 1.0, 3.0]


def test_default_feature_statement():
    A = D.recipe(20)[3]
    t = D.host_threshold(A, 40)
    x = D.host_strength_feature(A, t)
    ei, w = D.host_edges(A, t)
    deg = torch.zeros(20, dtype=torch.float64).index_add_(0, ei[0], w.double())     # ConnectomeGraph.degree()
    assert torch.allclose(x[:, 0], deg / (deg.max() + 1e-8), rtol=0, atol=1e-15)
    assert float(x.max()) <= 1.0 and float(x.min()) >= 0.0
    assert torch.equal(D.host_strength_feature(D.recipe(20)[2], 0.0), torch.zeros(20, 1, dtype=torch.float64))


def test_cpu_matrices_are_refused():
    m, y = D.recipe(5), D.labels(6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.from_matrices(m, y, keep=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.from_matrices(m, y, min_weight=0.5, node_features=D.features(6, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.select_thresholds(m, num_edges=3)


def _huge(shape):
    return torch.zeros(1).expand(*shape)      # no storage behind it


BAD_MATRICES = [
    ("dtype", lambda: D.recipe(5).double(), TypeError, "float32"),
    ("not a tensor", lambda: D.recipe(5).numpy(), TypeError, "torch.Tensor"),
    ("rank", lambda: D.recipe(5)[0], ValueError, r"\[S, n, n\]"),
    ("not square", lambda: D.recipe(5)[:, :, :4], ValueError, r"\[S, n, n\]"),
    ("n = 0", lambda: torch.zeros(3, 0, 0), ValueError, r"\[S, n, n\]"),
    ("S * n >= 2^31", lambda: _huge((2 ** 29, 4, 4)), ValueError, r"S \* n"),
    ("n * n >= 2^31", lambda: _huge((1, 46341, 46341)), ValueError, r"n \* n"),
    ("not contiguous", lambda: D.recipe(5).transpose(1, 2), ValueError, "contiguous"),
]


@pytest.mark.parametrize("name,make,exc,msg", BAD_MATRICES, ids=[b[0] for b in BAD_MATRICES])
def test_malformed_matrices_are_refused(name, make, exc, msg):
    m = make()
    y = torch.zeros(m.shape[0] if hasattr(m, "shape") and m.shape[0] < 100 else 1, dtype=torch.long)
    with pytest.raises(exc, match=msg):
        ingest.from_matrices(m, y, keep=0.1)
    with pytest.raises(exc, match=msg):
        ingest.select_thresholds(m, keep=0.1)


def test_threshold_arguments_are_refused():
    m, y = D.recipe(5), D.labels(6)
    for kw in ({}, {"keep": 0.1, "num_edges": 3}, {"keep": 0.1, "min_weight": 0.2},
               {"num_edges": 3, "min_weight": 0.2}, {"keep": 0.1, "num_edges": 3, "min_weight": 0.2}):
        with pytest.raises(ValueError, match="exactly one"):
            ingest.from_matrices(m, y, **kw)
    for kw in ({}, {"keep": 0.1, "num_edges": 3}):
        with pytest.raises(ValueError, match="exactly one"):
            ingest.select_thresholds(m, **kw)
    for keep in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"keep must lie in \[0, 1\]"):
            ingest.from_matrices(m, y, keep=keep)
        with pytest.raises(ValueError, match=r"keep must lie in \[0, 1\]"):
            ingest.select_thresholds(m, keep=keep)
    with pytest.raises(ValueError, match="num_edges must be >= 0"):
        ingest.from_matrices(m, y, num_edges=-1)
    with pytest.raises(ValueError, match="num_edges must be >= 0"):
        ingest.select_thresholds(m, num_edges=-1)
    with pytest.raises(TypeError, match="num_edges must be an int"):
        ingest.from_matrices(m, y, num_edges=2.5)
    for bad in (torch.zeros(5), torch.zeros(6, 1), torch.zeros(6, dtype=torch.long)):
        with pytest.raises(ValueError, match="min_weight tensor"):
            ingest.from_matrices(m, y, min_weight=bad)


def test_labels_and_features_are_refused():
    m, y = D.recipe(5), D.labels(6)
    for bad in (y.int(), y.float(), y[:5], y.view(6, 1), y.tolist()):
        with pytest.raises(ValueError, match=r"labels must be an int64 tensor \[S\]"):
            ingest.from_matrices(m, bad, keep=0.1)
    for bad in (D.features(6, 5).double(), D.features(5, 5), D.features(6, 4), D.features(6, 5)[:, :, 0]):
        with pytest.raises(ValueError, match=r"node_features must be a float32 tensor \[S, n, F\]"):
            ingest.from_matrices(m, y, keep=0.1, node_features=bad)
