"""The host statement of the maximum-spanning-tree backbone (tests/mst_data.py): Kruskal against Prim, the forest's size
and weight against scipy, the star of a constant matrix, the connectedness the feature exists for; the public argument
checks of ``ingest.mst_backbone`` and of ``backbone=`` on CPU tensors; the header and the binding of cgnn_ingest_mst.  No
device is touched."""
import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components, minimum_spanning_tree

from connectome_gnn_amd import _lib, ingest
from tests import ingest_data as D
from tests import knn_data as K
from tests import mst_data as M
from tests.abi_header import check_header

NAN, INF = float("nan"), float("inf")
SIZES = (1, 2, 3, 5, 20, 84)


def _components(mask):
    """the number of components of the undirected graph with an edge where ``mask`` [n, n] is set in either direction"""
    return int(connected_components(mask.numpy(), directed=False)[0])


def _upper(F):
    return torch.triu(F, 1)


@pytest.mark.parametrize("n", SIZES)
def test_kruskal_agrees_with_prim(n):
    for s, A in enumerate(M.cohort(n)):
        F = M.host_forest(A)
        assert torch.equal(F, M.brute_forest(A)), s
        assert torch.equal(F, F.t()) and not F.diagonal().any()
        assert not (F & ~(M.pair_weights(A) > 0)).any(), "a pair of the forest is a candidate"


@pytest.mark.parametrize("n", SIZES)
def test_the_forest_spans_every_component_of_the_candidates(n):
    for s, A in enumerate(M.cohort(n)):
        cand = (M.pair_weights(A) > 0) & ~torch.eye(n, dtype=torch.bool)
        F = M.forests(n)[s]
        c = _components(cand)
        assert int(_upper(F).sum()) == n - c, s
        assert _components(F) == c, "the forest connects what the candidates connect"


@pytest.mark.parametrize("n", SIZES)
def test_the_weight_is_that_of_scipys_tree(n):
    """scipy's minimum spanning tree of ``max + 1 - W`` over the candidates, for the subjects whose weights are finite.
    scipy breaks ties differently, so the pair count and the total weight are compared, the weight within what rounding
    ``max + 1 - W`` to fp64 can move it: n ulps of ``max + 1`` (a tie that fp64 creates swaps pairs that close)."""
    for s, A in enumerate(M.cohort(n)):
        W = M.pair_weights(A).double()
        iu = torch.triu_indices(n, n, 1)
        w = W[iu[0], iu[1]]
        if not bool(torch.isfinite(w).all()) or not bool((w > 0).any()):
            continue
        on = w > 0
        top = float(w.max())
        cost = coo_matrix(((top + 1 - w[on]).numpy(), (iu[0][on].numpy(), iu[1][on].numpy())), shape=(n, n))
        tree = minimum_spanning_tree(cost.tocsr()).tocoo()
        F = _upper(M.forests(n)[s])
        assert tree.nnz == int(F.sum()), s
        theirs = float(np.sum(top + 1 - tree.data))
        assert abs(float(W[F].sum()) - theirs) <= n * 2.0 ** -50 * (top + 1), s


def test_a_constant_matrix_gives_the_star_at_node_0():
    for n in (2, 5, 20):
        F = M.host_forest(D.worst_cases(n)[0])
        want = torch.zeros(n, n, dtype=torch.bool)
        want[0, 1:] = want[1:, 0] = True
        assert torch.equal(F, want)
        assert not M.host_forest(D.worst_cases(n)[2]).any()            # all negative: no candidates, no forest


def test_a_hand_written_example():
    A = torch.tensor([[9.0, 0.5, -1.0, 0.0],
                      [0.25, 0.0, NAN, 0.75],
                      [0.5, 0.5, 0.0, 0.75],
                      [0.0, 0.5, 1e-40, 7.0]])
    # weights: (0,1) .5  (0,2) .5  (0,3) 0  (1,2) .5  (1,3) .75  (2,3) .75: the forest is (1,3) (2,3) then (0,1)
    tree = [[0, .5, 0, 0], [.25, 0, 0, .75], [0, 0, 0, .75], [0, .5, 1e-40, 0]]
    assert torch.equal(M.bits(M.host_backbone(A)), M.bits(torch.tensor(tree, dtype=torch.float32)))
    half = [[0, .5, 0, 0], [.25, 0, 0, .75], [.5, .5, 0, .75], [0, .5, 1e-40, 0]]
    assert torch.equal(M.bits(M.host_backbone(A, 0.25)), M.bits(torch.tensor(half, dtype=torch.float32)))
    assert torch.equal(M.host_kept(A, -INF), K.candidates(A))           # every positive off-diagonal entry


def test_the_bridge_keeps_only_its_positive_direction():
    for n in (2, 5, 84):
        A = M.bridge(n)
        F = M.host_forest(A)
        assert bool(F[0, n - 1]) and bool(F[n - 1, 0])
        out = M.host_backbone(A, INF, F)
        assert float(out[n - 1, 0]) == float(A[n - 1, 0]) > 0 and M.bits(out)[0, n - 1] == 0
        assert _components(M.host_kept(A, INF, F)) == 1
    n = 20
    path = _upper(M.host_forest(M.chain(n)))
    assert torch.equal(torch.nonzero(path), torch.stack([torch.arange(n - 1), torch.arange(1, n)], 1))


def test_the_backbone_connects_a_modular_matrix():
    """84 ROIs in 4 modules, within-module weights in [0.5, 1], between-module weights in [0, 0.1]: a threshold and the
    k-NN graph both leave the 4 modules apart, and the tree joins them at six entries more."""
    n = 84
    A = M.modular(n, 4)
    F = M.host_forest(A)
    none = torch.zeros(n, n, dtype=torch.bool)
    t = D.host_threshold(A, D.rank_of(n, keep=0.10))
    plain, united = M.host_kept(A, t, none), M.host_kept(A, t, F)
    assert (_components(plain), int(plain.sum())) == (4, 696)
    assert (_components(united), int(united.sum())) == (1, 702)
    knn = K.host_kept(A, 8, "union")
    both = knn | M.host_kept(A, INF, F)
    assert (_components(knn), int(knn.sum())) == (4, 772)
    assert (_components(both), int(both.sum())) == (1, 778)
    assert int(united.sum()) - int(plain.sum()) <= 2 * (n - 1)
    # the composition that backbone="mst" with knn= stands for is exact: a maximum of positive bits and +0.0
    B = torch.maximum(K.host_knn(A, 8, "union"), M.host_backbone(A, INF, F))
    assert torch.equal(M.bits(B), M.bits(torch.where(both, A, torch.zeros_like(A))))


def _mats(n=5, S=3):
    return D.recipe(n)[:S].contiguous()


def test_mst_backbone_checks_its_arguments_before_the_device():
    m = _mats()
    assert ingest.BACKBONES == ("mst",) and ingest.MST_MAX_NODES == 1024
    for two in (dict(keep=0.1, num_edges=3), dict(keep=0.1, min_weight=0.2), dict(num_edges=3, min_weight=0.0)):
        with pytest.raises(ValueError, match="at most one of keep=, num_edges= and min_weight="):
            ingest.mst_backbone(m, **two)
    with pytest.raises(ValueError, match=r"keep must lie in \[0, 1\]"):
        ingest.mst_backbone(m, keep=1.5)
    with pytest.raises(TypeError, match="num_edges must be an int"):
        ingest.mst_backbone(m, num_edges=2.0)
    with pytest.raises(ValueError, match="min_weight tensor"):
        ingest.mst_backbone(m, min_weight=torch.zeros(4))
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.mst_backbone(torch.zeros(1, 1025, 1025))
    with pytest.raises(TypeError, match="float32"):
        ingest.mst_backbone(m.double())
    with pytest.raises(ValueError, match=r"\[S, n, n\]"):
        ingest.mst_backbone(m[:, :, :4])
    with pytest.raises(ValueError, match="out must be"):
        ingest.mst_backbone(m, out=torch.empty(3, 5, 4))
    with pytest.raises(TypeError, match="out must be float32"):
        ingest.mst_backbone(m, out=torch.empty(3, 5, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be contiguous"):
        ingest.mst_backbone(m, out=torch.empty(3, 5, 5).transpose(1, 2))
    with pytest.raises(TypeError, match="out must be a torch.Tensor"):
        ingest.mst_backbone(m, out=[0.0])
    # valid arguments on CPU tensors get as far as the residency check, and no further
    for kw in (dict(), dict(keep=0.1), dict(num_edges=0), dict(min_weight=0.3), dict(min_weight=torch.zeros(3)),
               dict(out=torch.empty_like(m)), dict(keep=1.0, out=m.clone())):
        with pytest.raises(RuntimeError, match="ROCm"):
            ingest.mst_backbone(m, **kw)


def _entry_points():
    m, y = _mats(), D.labels(3)
    ts = torch.randn(6, 40, 20, generator=torch.Generator().manual_seed(4))
    return {"from_matrices": lambda **kw: ingest.from_matrices(m, y, **kw),
            "node_measures": lambda **kw: ingest.node_measures(m, **kw),
            "module_profile": lambda **kw: ingest.module_profile(m, [0, 0, 1, 1, 1], **kw),
            "path_lengths": lambda **kw: ingest.path_lengths(m, **kw),
            "from_timeseries": lambda **kw: ingest.from_timeseries(ts, D.labels(6), **kw)}


@pytest.mark.parametrize("name", ["from_matrices", "node_measures", "module_profile", "path_lengths", "from_timeseries"])
def test_backbone_of_every_entry_point(name):
    call = _entry_points()[name]
    for bad in ("MST", "tree", 1, True):
        with pytest.raises(ValueError, match=r"BACKBONES = \('mst',\)"):
            call(keep=0.1, backbone=bad)
    with pytest.raises(ValueError, match="at most one of keep=, num_edges= and min_weight="):
        call(keep=0.1, min_weight=0.0, backbone="mst")
    with pytest.raises(ValueError, match="knn= is a fourth way"):
        call(knn=2, keep=0.1, backbone="mst")
    with pytest.raises(ValueError, match="give exactly one of keep=, num_edges= and min_weight="):
        call()                                         # without backbone= the check is as strict as it was
    with pytest.raises(ValueError, match=r"keep must lie in \[0, 1\]"):
        call(keep=-0.5, backbone="mst")
    for kw in (dict(backbone="mst"), dict(keep=0.1, backbone="mst"), dict(num_edges=4, backbone="mst"),
               dict(min_weight=0.2, backbone="mst"), dict(knn=2, backbone="mst"),
               dict(knn=3, knn_mode="mutual", backbone="mst"), dict(keep=0.1), dict(knn=2)):
        with pytest.raises(RuntimeError, match="ROCm"):
            call(**kw)


def test_backbone_refuses_more_than_1024_nodes_in_every_matrix_entry_point():
    big = torch.zeros(1, 1025, 1025)
    for call in (lambda: ingest.from_matrices(big, D.labels(1), keep=0.1, backbone="mst"),
                 lambda: ingest.node_measures(big, backbone="mst"),
                 lambda: ingest.path_lengths(big, num_edges=3, backbone="mst")):
        with pytest.raises(ValueError, match="n <= 1024"):
            call()


def test_the_prototypes_match_their_header_type_by_type():
    """cgnn_ingest_mst and its workspace query are declared in include/cgnn_mst.h, which cgnn.h includes, and bound by
    ``_lib.MST_PROTOTYPES``: every type, the library's exports, the constant, and the comparison itself against a
    doctored header."""
    hdr = check_header("cgnn_mst.h", _lib.MST_PROTOTYPES, ["cgnn_ingest_mst_workspace_bytes", "cgnn_ingest_mst"],
                       [("int64_t S, int32_t n)", "int32_t S, int32_t n)"), ("void* workspace, ", "")])
    assert "#define CGNN_MST_MAX_NODES 1024\n" in hdr
    assert _lib.ABI_VERSION == 2, "the change is additive"


def test_the_entry_point_refuses_before_any_launch():
    """No device is present here: a call that went as far as a launch could not return these codes."""
    lib = _lib.load()
    fn, query = lib.cgnn_ingest_mst, lib.cgnn_ingest_mst_workspace_bytes
    S, n = 3, 21
    a, b, w, t = 1 << 20, 1 << 24, 1 << 28, 1 << 30    # addresses that nothing dereferences
    nbytes = 4 * S * n * n
    need = query(S, n)
    assert need == S * n * 24 * 4, "a slab per workgroup, rows rounded up to 16 bytes"
    assert query(10 ** 6, n) == query(10 ** 5, n) > need, "per workgroup of the launch, not per subject"
    assert query(0, n) == 0
    for bad in ((-1, n), (S, 0), (S, 1025), (2 ** 31 // n + 1, n)):
        assert query(*bad) == _lib.CGNN_EINVAL, bad
    good = [a, S, n, t, w, need, b, nbytes, None]

    def rc(at, v):
        return fn(*(good[:at] + [v] + good[at + 1:]))

    for at, v in ((0, None), (6, None), (4, None), (0, a + 2), (6, b + 1), (3, t + 2), (4, w + 8), (1, -1), (2, 0),
                  (2, -5), (7, nbytes - 1), (5, need - 1), (5, 0), (1, 2 ** 31 // n + 1),
                  (6, a + 4 * n * n), (6, a - 4), (6, a + nbytes - 4),              # out overlaps matrices
                  (4, a), (4, a + nbytes - 16), (4, b - need + 16), (4, b + nbytes - 16),   # the workspace overlaps
                  (3, b), (3, b + nbytes - 4)):                                     # the thresholds lie in out
        assert rc(at, v) == _lib.CGNN_EINVAL, (at, v)
    assert rc(2, 1025) == _lib.CGNN_EUNSUPPORTED
    assert fn(a, -1, 1025, t, w, need, b, nbytes, None) == _lib.CGNN_EINVAL       # a bad value comes first
    assert rc(1, 0) == _lib.CGNN_OK and fn(None, 0, n, None, None, 0, None, 0, None) == _lib.CGNN_OK
