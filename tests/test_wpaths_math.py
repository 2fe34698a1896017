"""The weighted shortest-path node measures of connectome_gnn_amd.ingest without a GPU: their fp64 host statement
(tests/wpaths_data.py) against networkx and against the binary statement, and what the package checks before it
needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import ingest_data as I
from tests import measures_data as M
from tests import paths_data as P
from tests import wpaths_data as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_names_are_the_statement_s():
    assert ingest.WEIGHTED_PATH_MEASURES == W.WEIGHTED_PATH_MEASURES == (
        "weighted_nodal_efficiency", "weighted_closeness", "weighted_eccentricity")
    assert ingest.WEIGHTED_PATH_MAX_NODES == 1024
    assert ingest.MEASURES == M.MEASURES and ingest.PATH_MEASURES == P.PATH_MEASURES, "the nine stay as they are"
    assert callable(ingest.path_lengths)


@pytest.mark.parametrize("n,keep", [(20, 0.3), (37, 0.1), (84, 0.1)])
def test_statement_against_networkx_on_a_symmetric_case(n, keep):
    nx = pytest.importorskip("networkx")
    mats = W.cohort(n)
    for s in W.SYMMETRIC:
        A, t = mats[s], W.thresholds(mats, keep)[s]
        mask, L = W.lengths(A, t)
        assert (mask == mask.T).all() and mask.any()
        G = nx.Graph()
        G.add_nodes_from(range(n))
        G.add_weighted_edges_from([(i, j, L[i, j]) for i, j in zip(*np.nonzero(mask))], weight="length")
        D, got, H = W.host_statement(A, t)
        got = got.numpy()
        assert 1 <= H <= n - 1
        close = nx.closeness_centrality(G, distance="length", wf_improved=True)
        assert np.abs(got[:, 1] - np.array([close[v] for v in range(n)])).max() <= 1e-12, (n, s)
        dist = dict(nx.all_pairs_dijkstra_path_length(G, weight="length"))
        eff = np.array([sum(1.0 / d for j, d in dist[v].items() if j != v) for v in range(n)]) / (n - 1)
        assert np.abs(got[:, 0] - eff).max() <= 1e-12, (n, s)
        # networkx's eccentricity wants a connected graph: per component, a single node has none
        ecc = np.zeros(n)
        for comp in nx.connected_components(G):
            if len(comp) > 1:
                for v, e in nx.eccentricity(G.subgraph(comp), weight="length").items():
                    ecc[v] = e
        assert np.abs(got[:, 2] - ecc / (n - 1)).max() <= 1e-12, (n, s)
        for v in range(n):
            for j in range(n):
                want = dist[v].get(j, np.inf)
                assert abs(float(D[v, j]) - want) <= 1e-12 * max(want, 1.0) if np.isfinite(want) else float(D[v, j]) == want


@pytest.mark.parametrize("n,keep", [(20, 0.1), (37, 0.1), (84, 0.1), (84, 0.5)])
def test_equal_weights_give_the_binary_statement(n, keep):
    mats = W.cohort(n)
    thr = W.thresholds(mats, keep)
    for s, A in enumerate(W.equal_weights(mats, thr)):
        D, got, H = W.host_statement(A, 0.0)
        mask = M.kept_mask(mats[s], thr[s])
        hops = P.distances(mask)
        assert np.array_equal(D.numpy(), np.where(hops < 0, np.inf, hops.astype(np.float64))), "every length is exactly 1"
        assert H == int(hops.max(initial=0))
        want = P.mask_measures(mask, P.PATH_MEASURES[:3])
        assert float((got - want).abs().max()) <= 1e-12, (n, keep, s)


@pytest.mark.parametrize("n", [5, 33])
def test_statement_on_structured_weighted_graphs(n):
    for kind in W.STRUCTURED:
        A = W.structured(kind, n)
        assert torch.equal(A > 0, P.structured(kind, n) > 0)
        kept = A[A > 0]
        assert float(kept.min()) >= 0.05 and float(kept.max()) <= 1.0 and kept.unique().numel() > 1
        D, got, H = W.host_statement(A, 0.0)
        hops = P.distances(M.kept_mask(A, 0.0))
        assert np.array_equal(np.isfinite(D.numpy()), hops >= 0), "the same reachable set as the binary statement"
        assert bool((D.numpy()[hops > 0] >= hops[hops > 0]).all()), "every length is >= 1"
        if kind == "directed_path":
            assert H == n - 1 and got[n - 1].tolist() == [0.0, 0.0, 0.0]
        if kind == "cliques":
            assert got[n - 1].tolist() == [0.0, 0.0, 0.0], "the isolated node"


def test_statement_is_invariant_under_scaling():
    for n, keep in ((20, 0.3), (37, 0.1)):
        mats = W.cohort(n)
        for A, t in zip(mats, W.thresholds(mats, keep)):
            D, got, H = W.host_statement(A, t)
            D4, got4, H4 = W.host_statement(A * 4, t * 4)
            assert torch.equal(D, D4) and torch.equal(got, got4) and H == H4


def test_statement_edge_cases():
    zeros = torch.zeros(20, 3, dtype=torch.float64)
    D, got, H = W.host_statement(I.recipe(20)[2], 0.0)                  # the all-zero subject
    assert torch.equal(got, zeros) and H == 0
    assert torch.equal(D, torch.where(torch.eye(20, dtype=torch.bool), 0.0, float("inf")).double())
    D, got, H = W.host_statement(torch.ones(1, 1), -1.0)
    assert D.tolist() == [[0.0]] and got.tolist() == [[0.0, 0.0, 0.0]]
    # NaN entries are never edges
    A = W.cohort(20)[2]
    assert bool(torch.isnan(A[0, 1])) and not M.kept_mask(A, -float("inf"))[0, 1]
    assert bool(torch.isfinite(W.host_statement(A, 0.0)[1]).all())


def test_weighted_names_are_refused_like_the_others():
    m, y = I.recipe(5), I.labels(6)
    for bad, msg in ((("weighted_closeness", "weighted_betweenness"), "unknown measure"),
                     (("weighted_local_efficiency",), "unknown measure"),
                     (("degree", "weighted_closeness", "closeness", "weighted_closeness"), "named twice"),
                     (("weighted_eccentricity", "weighted_eccentricity"), "named twice")):
        with pytest.raises(ValueError, match=msg):
            ingest.node_measures(m, keep=0.1, measures=bad)
        with pytest.raises(ValueError, match=msg):
            ingest.from_matrices(m, y, keep=0.1, measures=bad)
        with pytest.raises(ValueError, match=msg):
            ingest.from_timeseries(torch.zeros(6, 4, 5), y, keep=0.1, measures=bad)
    with pytest.raises(ValueError, match="either measures= or node_features="):
        ingest.from_matrices(m, y, keep=0.1, measures=("weighted_closeness",), node_features=I.features(6, 5))
    with pytest.raises(ValueError, match="exactly one of"):
        ingest.path_lengths(m, keep=0.1, min_weight=0.2)
    with pytest.raises(ValueError, match="exactly one of"):
        ingest.path_lengths(m)


def test_more_than_1024_nodes_are_refused_on_a_cpu_tensor():
    big, y = torch.zeros(1, 1025, 1025), I.labels(1)
    for names in (("weighted_closeness",), ("degree", "weighted_eccentricity"), W.WEIGHTED_PATH_MEASURES,
                  ("closeness", "weighted_nodal_efficiency")):
        with pytest.raises(ValueError, match="n <= 1024"):
            ingest.node_measures(big, keep=0.1, measures=names)
        with pytest.raises(ValueError, match="n <= 1024"):
            ingest.from_matrices(big, y, keep=0.1, measures=names)
        with pytest.raises(ValueError, match="n <= 1024"):
            ingest.from_timeseries(torch.zeros(1, 4, 1025), y, keep=0.1, measures=names)
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.path_lengths(big, keep=0.1)
    # 1024 itself is taken: the next refusal is the device's
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.node_measures(torch.zeros(1, 1024, 1024), keep=0.1, measures=W.WEIGHTED_PATH_MEASURES)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.path_lengths(torch.zeros(1, 1024, 1024), keep=0.1)


def test_cpu_tensors_are_refused():
    m, y = I.recipe(5), I.labels(6)
    for names in (W.WEIGHTED_PATH_MEASURES, ("weighted_closeness",), ("strength", "weighted_eccentricity", "closeness")):
        for kw in ({"keep": 0.1}, {"num_edges": 3}, {"min_weight": 0.5}, {"min_weight": torch.zeros(6)}):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                ingest.node_measures(m, measures=names, **kw)
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                ingest.from_matrices(m, y, measures=names, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ingest.from_timeseries(torch.zeros(6, 4, 5), y, keep=0.1, measures=names)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.path_lengths(m, keep=0.1)


def test_header_exports_and_prototypes_agree_for_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, args in (("cgnn_ingest_wpaths_workspace_bytes", 4), ("cgnn_ingest_wpaths", 15)):
        decl = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert decl, f"{name} is not declared in cgnn.h"
        assert len(decl.group(2).split(",")) == args
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib.PROTOTYPES[name]
        assert len(argtypes) == args
        assert restype is (ctypes.c_int64 if decl.group(1) == "int64_t" else ctypes.c_int)
    for macro, value in (("CGNN_WPATH_NODAL_EFFICIENCY", 0), ("CGNN_WPATH_CLOSENESS", 1), ("CGNN_WPATH_ECCENTRICITY", 2),
                         ("CGNN_NUM_WPATH_MEASURES", 3), ("CGNN_WPATH_MAX_NODES", 1024)):
        assert re.search(rf"#define {macro} {value}\b", code), macro
    assert [f"weighted_{m}" for m in P.PATH_MEASURES[:3]] == list(ingest.WEIGHTED_PATH_MEASURES), "the ids line up"
    # the byte count needs no device for its refusals
    loaded = _lib.load()
    i32 = ctypes.c_int32
    for args in ((-1, 20, (i32 * 1)(0), 1), (6, 0, (i32 * 1)(0), 1), (6, 1025, (i32 * 1)(0), 1), (6, 20, None, 1),
                 (6, 20, (i32 * 1)(3), 1), (6, 20, (i32 * 2)(1, 1), 2), (6, 20, (i32 * 4)(0, 1, 2, 0), 4),
                 (6, 20, (i32 * 1)(0), -1), (2 ** 31 // 20 + 1, 20, (i32 * 1)(0), 1)):
        assert loaded.cgnn_ingest_wpaths_workspace_bytes(*args) < 0, args
