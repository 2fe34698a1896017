"""RaggedPackedDataset / pack_graphs / threshold_edges (synthetic.py): the host side of the device-resident
path for same-atlas datasets whose subjects keep different numbers of edges.  No GPU needed."""
import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd.synthetic import PackedDataset, RaggedPackedDataset, pack_graphs, threshold_edges
from tests import ragged_data as R


def _same_graph(a, b):
    return (torch.equal(a.node_features, b.node_features) and torch.equal(a.edge_index, b.edge_index)
            and a.edge_index.dtype == b.edge_index.dtype and a.edge_index.shape == b.edge_index.shape
            and torch.equal(a.edge_weight, b.edge_weight) and torch.equal(a.label, b.label))


@pytest.mark.parametrize("S,n,k", R.SHAPES)
def test_from_graphs_round_trips_bit_exactly(S, n, k):
    graphs = R.ragged_graphs(S, n, k)
    ds = RaggedPackedDataset.from_graphs(list(graphs))
    assert ds.num_subjects == S
    assert ds.x.shape == (S, n, 5) and ds.labels.shape == (S,) and ds.labels.dtype == torch.long
    counts = [g.num_edges for g in graphs]
    assert ds.edge_ptr.device.type == "cpu" and ds.edge_ptr.dtype == torch.long
    assert ds.edge_ptr.tolist() == [sum(counts[:i]) for i in range(S + 1)]
    assert ds.edge_local.shape == (2, sum(counts)) and ds.edge_weight.shape == (sum(counts),)
    for i, g in enumerate(graphs):
        assert _same_graph(ds.graph(i), g), i
    assert ds.graph(R.EMPTY).num_edges == 0 and ds.graph(R.EMPTY).edge_index.shape == (2, 0)
    assert ds.graph(S - 1).num_edges == n * k
    moved = ds.to("cpu")
    assert isinstance(moved, RaggedPackedDataset) and torch.equal(moved.edge_ptr, ds.edge_ptr)
    assert torch.equal(moved.edge_ptr_dev, ds.edge_ptr)
    # the collate that matches is collate_graphs': the packed arrays ARE its concatenation
    ref = C.collate_graphs(list(graphs))
    assert torch.equal(ds.edge_weight, ref.edge_weight) and torch.equal(ds.edge_ptr, ref._eptr)


def test_pack_graphs_picks_the_layout():
    regular = C.generate_dataset(5, 20, 4, seed=1)
    dense = pack_graphs(regular)
    want = PackedDataset.from_graphs(regular)
    assert type(dense) is PackedDataset
    for name in ("x", "edge_local", "edge_weight", "labels"):
        assert torch.equal(getattr(dense, name), getattr(want, name))
    ragged = pack_graphs(list(R.ragged_graphs(8, 20, 4)))
    assert type(ragged) is RaggedPackedDataset
    with pytest.raises(ValueError):
        pack_graphs([])


def test_from_graphs_refuses_what_it_cannot_hold():
    graphs = list(R.ragged_graphs(8, 20, 4))
    other_atlas = C.generate_dataset(1, 21, 4, seed=1)
    with pytest.raises(ValueError):
        RaggedPackedDataset.from_graphs(graphs + other_atlas)
    with pytest.raises(ValueError):
        pack_graphs(graphs + other_atlas)
    g = graphs[0]
    wider = C.ConnectomeGraph(torch.zeros(20, 6), g.edge_index, g.edge_weight, g.label)
    with pytest.raises(ValueError):
        RaggedPackedDataset.from_graphs(graphs + [wider])
    unlabelled = C.ConnectomeGraph(g.node_features, g.edge_index, g.edge_weight, None)
    with pytest.raises(ValueError):
        RaggedPackedDataset.from_graphs(graphs + [unlabelled])
    with pytest.raises(ValueError):
        RaggedPackedDataset.from_graphs([])


def test_threshold_edges_keeps_the_edges_above_in_order():
    g = C.generate_dataset(1, 84, 8, seed=5)[0]
    for thr in (0.0, 0.2, 0.35, 2.0):
        t = threshold_edges(g, thr)
        keep = [j for j in range(g.num_edges) if float(g.edge_weight[j]) > thr]
        assert t.num_edges == len(keep)
        assert torch.equal(t.edge_index, g.edge_index[:, keep]) and torch.equal(t.edge_weight, g.edge_weight[keep])
        assert t.node_features is g.node_features and t.label is g.label and t.subject_id == g.subject_id
    assert threshold_edges(g, 0.2).num_edges < g.num_edges
    assert threshold_edges(g, 2.0).num_edges == 0
    # strictly greater: an edge AT the threshold goes
    w0 = float(g.edge_weight[0])
    assert threshold_edges(g, w0).num_edges == int((g.edge_weight > w0).sum())


@pytest.mark.parametrize("S,n,k", R.SHAPES[:2])
def test_relabel_by_degree_is_an_isomorphism_per_subject(S, n, k):
    graphs = R.ragged_graphs(S, n, k)
    ds = RaggedPackedDataset.from_graphs(list(graphs))
    rel = ds.relabel_by_degree()
    assert isinstance(rel, RaggedPackedDataset) and torch.equal(rel.edge_ptr, ds.edge_ptr)
    assert torch.equal(rel.labels, ds.labels)
    for i, g in enumerate(graphs):
        deg = torch.zeros(n, dtype=torch.long)
        one = torch.ones(g.num_edges, dtype=torch.long)
        deg.index_add_(0, g.edge_index[1], one).index_add_(0, g.edge_index[0], one)
        perm = torch.argsort(deg, descending=True, stable=True)              # new id -> old id
        r = rel.graph(i)
        assert torch.equal(r.node_features, g.node_features[perm])
        new_deg = torch.zeros(n, dtype=torch.long)
        new_deg.index_add_(0, r.edge_index[1], one).index_add_(0, r.edge_index[0], one)
        assert bool((new_deg[:-1] >= new_deg[1:]).all())                    # decreasing degree
        back = perm[r.edge_index]                                            # mapped back to the old ids
        mine = sorted(zip(back[0].tolist(), back[1].tolist(), r.edge_weight.tolist()))
        want = sorted(zip(g.edge_index[0].tolist(), g.edge_index[1].tolist(), g.edge_weight.tolist()))
        assert mine == want
        assert torch.equal(back, g.edge_index)                               # (COO order is kept too)


def test_relabel_by_degree_agrees_with_the_dense_layout():
    regular = C.generate_dataset(5, 20, 4, seed=1)
    dense = PackedDataset.from_graphs(regular).relabel_by_degree()
    flat = RaggedPackedDataset.from_graphs(regular).relabel_by_degree()
    for i in range(5):
        assert _same_graph(dense.graph(i), flat.graph(i))
