"""Same-atlas datasets with per-subject edge counts for the ragged resident path's tests.

Recipe: Watts-Strogatz subjects (``generate_dataset(S, n, k, seed=5)``), subject i keeps the edges with
weight > 0.2 + 0.05 * (i % 5).  The generator's graphs are symmetric, so those counts are all even and every
run would start at an even offset: every subject with i % 3 == 0 also loses its first remaining edge (odd
counts, odd run offsets).  Subject 1 is emptied completely, the last subject is left whole."""
import functools

import torch

import connectome_gnn_amd as C
from connectome_gnn_amd.synthetic import threshold_edges

SHAPES = [(8, 20, 4), (12, 84, 8), (6, 360, 14)]
EMPTY = 1


def _drop_first(g):
    return C.ConnectomeGraph(g.node_features, g.edge_index[:, 1:], g.edge_weight[1:], g.label, g.subject_id)


def thresholded(graphs):
    """The thresholding + odd-count part of the recipe on any list of symmetric graphs."""
    out = []
    for i, g in enumerate(graphs):
        t = threshold_edges(g, 0.2 + 0.05 * (i % 5))
        out.append(_drop_first(t) if i % 3 == 0 and t.num_edges else t)
    return out


@functools.lru_cache(maxsize=None)
def ragged_graphs(S, n, k):
    """The recipe's graphs (host, shared between tests: do not modify)."""
    base = C.generate_dataset(S, n, k, seed=5)
    out = thresholded(base)
    out[EMPTY] = threshold_edges(base[EMPTY], float("inf"))
    out[S - 1] = base[S - 1]
    assert out[EMPTY].num_edges == 0 and out[S - 1].num_edges == n * k
    assert any(g.num_edges % 2 for g in out)
    return tuple(out)


def host_eptr(graphs, ids):
    e = torch.zeros(len(ids) + 1, dtype=torch.long)
    if len(ids):
        e[1:] = torch.cumsum(torch.tensor([graphs[i].num_edges for i in ids], dtype=torch.long), 0)
    return e
