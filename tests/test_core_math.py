"""The host statement of the core decomposition (tests/core_data.py): the peeling against ``networkx.core_number`` and
``networkx.onion_layers``, against the brute-force max-min over all subsets, against closed forms and against the degree and
the strength; the argument checks of ``ingest.core_measures`` / ``core_levels``; the header and the binding of
cgnn_ingest_cores and the refusals of the C entry point, none of which reaches a launch.  No device is touched."""
import ctypes

import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import core_data as CD
from tests import measures_data as MD
from tests.abi_header import check_header

NAMES = CD.CORE_MEASURES
HOST_SIZES = (1, 2, 3, 5, 63, 84, 129, 360)


def test_the_names_and_constants():
    assert ingest.CORE_MEASURES == NAMES == ("coreness", "onion_layer", "s_coreness")
    assert ingest.CORE_MAX_NODES == 1024
    assert not set(NAMES) & set(ingest._ALL_MEASURES) and not set(NAMES) & set(ingest.CENTRALITY_MEASURES)
    assert ingest._CORE not in ingest._FAMILIES and len(ingest._ALL_MEASURES) == 17
    import connectome_gnn_amd
    assert "core_measures" not in connectome_gnn_amd.__all__


# ---- the statement ----
@pytest.mark.parametrize("n", HOST_SIZES)
def test_the_peeling_is_networkx_on_symmetric_subjects(n):
    nx = pytest.importorskip("networkx")
    mats = CD.cohort(n)
    for kw in CD.THRESHOLDS:
        thr = CD.host_thresholds(mats, kw)
        _, levels = CD.cohort_statement(n, kw)
        for s in CD.SYMMETRIC:
            mask = MD.kept_mask(mats[s], thr[s])
            assert (mask == mask.T).all(), (n, kw, s)
            g = nx.from_numpy_array(mask.astype(np.int64))
            assert g.number_of_nodes() == n
            core, onion = nx.core_number(g), nx.onion_layers(g)
            assert levels[s, :, 0].tolist() == [core[i] for i in range(n)], (n, kw, s)
            assert levels[s, :, 1].tolist() == [onion[i] for i in range(n)], (n, kw, s)


def test_the_peeling_is_the_max_min_over_all_subsets():
    """30 asymmetric graphs of 7 nodes; the weights are multiples of 1 / 16, so every sum is exact."""
    g = torch.Generator().manual_seed(11)
    for trial in range(30):
        n = 7
        mask = (torch.rand(n, n, generator=g) < 0.2 + 0.02 * trial) & ~torch.eye(n, dtype=torch.bool)
        w = torch.randint(1, 17, (n, n), generator=g).double() / 16
        b = mask.long().numpy()
        a = torch.where(mask, w, torch.zeros(n, n, dtype=torch.float64)).numpy()
        assert not (b == b.T).all() or trial < 3
        for v in (b, a):
            value, layer = CD.peel(v)
            assert (value == CD.brute_core(v)).all(), (trial, v.dtype)
            assert layer.min() >= 1 and layer.max() <= n
            # a later layer never has a smaller value: the level only grows
            order = np.argsort(layer, kind="stable")
            assert (np.diff(value[order]) >= 0).all()


@pytest.mark.parametrize("n", HOST_SIZES)
def test_coreness_is_at_most_the_degree_and_s_coreness_at_most_the_strength(n):
    mats = CD.cohort(n)
    for kw in CD.THRESHOLDS:
        thr = CD.host_thresholds(mats, kw)
        x, levels = CD.cohort_statement(n, kw)
        for s, (A, t) in enumerate(zip(mats, thr)):
            ref = MD.host_measures(A, t, ("degree", "strength"))
            assert bool((x[s, :, 0].double() <= ref[:, 0] + 2.0 ** -24).all()), (n, kw, s)
            assert bool((x[s, :, 2].double() <= ref[:, 1] * (1 + 2.0 ** -24)).all()), (n, kw, s)
            k, r, sigma, rho, top = CD.host_levels(A, t)
            a, b, _ = MD.value_maps(A, t)
            assert (k <= b.sum(1)).all() and (sigma <= a.sum(1)).all()
            assert (r >= 1).all() and (rho >= 1).all() and r.max() <= n and rho.max() <= n
            assert bool((x[s] >= 0).all()) and bool((x[s] <= 1).all())
        assert not levels[CD.ALL_ZERO, :, 0].any() and bool((levels[CD.ALL_ZERO, :, 1:] == 1).all()), "no edge: layer 1 of core 0"


@pytest.mark.parametrize("n", (1, 2, 3, 5, 7, 20, 63, 84))
def test_the_closed_forms(n):
    mats = CD.cohort(n)
    for s, expected in ((CD.CLIQUES, CD.expected_cliques), (CD.STAR, CD.expected_star),
                        (CD.CLIQUE_PATH, CD.expected_clique_path)):
        k, r, sigma, rho, _ = CD.host_levels(mats[s], 0.0)
        for weighted, value, layer in ((False, k, r), (True, sigma, rho)):
            want = expected(n, weighted)
            if want is None:
                assert s == CD.CLIQUE_PATH and n < 7
                continue
            assert (value == want[0]).all() and (layer == want[1]).all(), (n, s, weighted)
    # the small sizes degrade sensibly: one node is isolated, two nodes are one edge
    k, r, sigma, rho, _ = CD.host_levels(mats[CD.CLIQUE_PATH], 0.0)
    if n == 1:
        assert k.tolist() == [0] and r.tolist() == [1] and rho.tolist() == [1]
    if n in (2, 3):
        assert set(k.tolist()) == {1}
    k, r, _, _, _ = CD.host_levels(mats[CD.THRESHOLD_GRAPH], 0.0)
    if n > 3:
        degree = MD.value_maps(mats[CD.THRESHOLD_GRAPH], 0.0)[1].sum(1)
        assert set(degree.tolist()) == set(range(n - 1)), "every degree occurs"
        assert len(set(k.tolist())) > 1 and (np.diff(k) >= 0).all(), "nested cores"
    if n == 1:
        assert k.tolist() == [0]


def test_a_hand_written_example():
    """A triangle 0-1-2 with a tail 2-3-4 and an isolated node 5; the weights make the weighted layers differ."""
    A = torch.zeros(6, 6)
    for u, v, w in ((0, 1, 0.5), (1, 2, 0.5), (0, 2, 1.0), (2, 3, 0.25), (3, 4, 0.125)):
        A[u, v] = A[v, u] = w
    k, r, sigma, rho, top = CD.host_levels(A, 0.0)
    assert k.tolist() == [2, 2, 2, 1, 1, 0] and r.tolist() == [4, 4, 4, 3, 2, 1]
    # s = 1.5, 1, 1.75, 0.375, 0.125, 0: node 3 leaves at its own 0.25, node 1 at 1.0, and nodes 0 and 2 a round later
    assert sigma.tolist() == [1.0, 1.0, 1.0, 0.25, 0.125, 0.0] and rho.tolist() == [5, 4, 5, 3, 2, 1]
    assert top == 1.75
    x, levels = CD.host_cores(A, 0.0)
    assert x[:, 0].tolist() == [np.float32(v / 5).item() for v in (2, 2, 2, 1, 1, 0)]
    assert x[:, 1].tolist() == [np.float32(np.float32(v) / np.float32(6)).item() for v in (4, 4, 4, 3, 2, 1)]
    assert levels.tolist() == [[2, 4, 5], [2, 4, 4], [2, 4, 5], [1, 3, 3], [1, 2, 2], [0, 1, 1]]
    A[0, 1] = float("inf")
    k2, r2, sigma2, rho2, _ = CD.host_levels(A, 0.0)
    assert k2.tolist() == k.tolist() and r2.tolist() == r.tolist()
    assert np.isnan(sigma2).all() and (rho2 == -1).all()


# ---- the Python arguments ----
def test_core_measures_checks_its_arguments():
    mats = CD.cohort(5)[:3].contiguous()
    for call in (ingest.core_measures, ingest.core_levels):
        with pytest.raises(ValueError, match=rf"{call.__name__} takes n <= 1024 nodes"):
            call(torch.zeros(1, 1025, 1025), keep=0.1)
        with pytest.raises(ValueError, match="exactly one of keep=, num_edges= and min_weight="):
            call(mats)
        with pytest.raises(ValueError, match="exactly one of keep=, num_edges= and min_weight="):
            call(mats, keep=0.1, min_weight=0.0)
        with pytest.raises(ValueError, match="knn= is a fourth way"):
            call(mats, keep=0.1, knn=3)
        with pytest.raises(ValueError, match="unknown backbone"):
            call(mats, keep=0.1, backbone="tree")
        with pytest.raises(TypeError, match="float32"):
            call(mats.double(), keep=0.1)
        with pytest.raises(TypeError, match="torch.Tensor"):
            call(mats.numpy(), keep=0.1)
        with pytest.raises(ValueError, match=r"\[S, n, n\]"):
            call(mats[:, :, :4], keep=0.1)
        # a valid request gets as far as the device check: there is no CPU path
        for kw in (dict(keep=0.1), dict(min_weight=0.0), dict(knn=3), dict(backbone="mst"), dict(num_edges=7),
                   dict(keep=0.5, group="mean")):
            with pytest.raises(RuntimeError, match="ROCm"):
                call(mats, **kw)
    with pytest.raises(ValueError, match="unknown measure 'k_core': the core measures are"):
        ingest.core_measures(mats, keep=0.2, measures=("coreness", "k_core"))
    with pytest.raises(ValueError, match="unknown measure 'degree'"):
        ingest.core_measures(mats, keep=0.2, measures=("degree",))
    with pytest.raises(ValueError, match="unknown measure 'pagerank'"):
        ingest.core_measures(mats, keep=0.2, measures=("pagerank",))
    with pytest.raises(ValueError, match="'onion_layer' is named twice"):
        ingest.core_measures(mats, keep=0.2, measures=("onion_layer", "onion_layer"))
    with pytest.raises(ValueError, match="measures is empty"):
        ingest.core_measures(mats, keep=0.2, measures=())
    with pytest.raises(TypeError, match="tuple of names"):
        ingest.core_measures(mats, keep=0.2, measures="coreness")
    with pytest.raises(ValueError, match="unknown measure 'coreness'"):
        ingest.node_measures(mats, keep=0.2, measures=("coreness",))
    for kw in (dict(keep=0.1, measures=("s_coreness",)), dict(min_weight=0.0, measures=NAMES[::-1])):
        with pytest.raises(RuntimeError, match="ROCm"):
            ingest.core_measures(mats, **kw)


# ---- the C ABI ----
def test_the_prototypes_match_their_header_type_by_type():
    hdr = check_header("cgnn_core.h", _lib.CORE_PROTOTYPES, ["cgnn_ingest_cores_workspace_bytes", "cgnn_ingest_cores"],
                       [("int32_t* levels", "int32_t levels"), ("int64_t levels_bytes, ", "")])
    assert len(_lib.PROTOTYPES) == 127
    lib = _lib.load()
    for name, value in (("CGNN_CORE_CORENESS", 0), ("CGNN_CORE_ONION_LAYER", 1), ("CGNN_CORE_S_CORENESS", 2),
                        ("CGNN_NUM_CORE_MEASURES", 3), ("CGNN_CORE_MAX_NODES", 1024)):
        assert f"#define {name} {value}\n" in hdr
    assert _lib.ABI_VERSION == 2 and lib.cgnn_abi_version() == 2, "the change is additive"


_i32 = ctypes.c_int32
_A, _M4, _A2 = 0x1000, 0x1004, 0x1002      # 16-byte aligned / 4-byte aligned only / not 4-byte aligned: never dereferenced
_INV, _OK = _lib.CGNN_EINVAL, _lib.CGNN_OK
_CALL, _QUERY = "cgnn_ingest_cores", "cgnn_ingest_cores_workspace_bytes"
_ID3, _COL3 = (_i32 * 3)(0, 1, 2), (_i32 * 3)(3, 1, 0)
_BIG_S = 2 ** 31 // 20 + 1                 # S * n >= 2^31 at n = 20
# defaults that pass every check: S = 6 subjects of n = 20 nodes, the three measures into a [S, n, 4] x, and the levels
_DEFAULTS = {
    _QUERY: dict(S=6, n=20, measures=_ID3, num=3),
    _CALL: dict(matrices=_A, S=6, n=20, thr=_A, measures=_ID3, num=3, cols=_COL3, ldx=4, workspace=None,
                workspace_bytes=0, x=_A, x_bytes=1920, levels=_A, levels_bytes=1440, stream=None),
}
_EMPTY = dict(matrices=None, S=0, thr=None, x=None, x_bytes=0, levels=None, levels_bytes=0)
_CALLS = [
    # ---- the byte count: no slab, whatever is asked for
    (_QUERY, dict(), 0),
    (_QUERY, dict(measures=(_i32 * 1)(2), num=1), 0),
    (_QUERY, dict(S=0), 0),
    (_QUERY, dict(n=1024), 0),
    (_QUERY, dict(n=1025), _INV),
    (_QUERY, dict(S=-1), _INV),
    (_QUERY, dict(n=0), _INV),
    (_QUERY, dict(measures=None), _INV),
    (_QUERY, dict(measures=None, num=0), _INV),
    (_QUERY, dict(num=4), _INV),
    (_QUERY, dict(num=-1), _INV),
    (_QUERY, dict(measures=(_i32 * 2)(1, 1), num=2), _INV),
    (_QUERY, dict(measures=(_i32 * 1)(3), num=1), _INV),
    (_QUERY, dict(S=_BIG_S), _INV),
    # ---- the call: the request and the cohort (measure_request.h)
    (_CALL, dict(S=-1), _INV),
    (_CALL, dict(n=0), _INV),
    (_CALL, dict(n=-3), _INV),
    (_CALL, dict(n=1025, x_bytes=2 ** 30, levels_bytes=2 ** 30), _INV),
    (_CALL, dict(S=_BIG_S), _INV),
    (_CALL, dict(num=0), _INV),
    (_CALL, dict(num=-1), _INV),
    (_CALL, dict(num=4), _INV),
    (_CALL, dict(measures=None), _INV),
    (_CALL, dict(cols=None), _INV),
    (_CALL, dict(measures=(_i32 * 3)(0, 1, 3)), _INV),
    (_CALL, dict(measures=(_i32 * 3)(-1, 1, 2)), _INV),
    (_CALL, dict(measures=(_i32 * 3)(1, 2, 1)), _INV),
    (_CALL, dict(cols=(_i32 * 3)(3, 4, 0)), _INV),                    # a column == ldx
    (_CALL, dict(cols=(_i32 * 3)(-1, 1, 0)), _INV),
    (_CALL, dict(cols=(_i32 * 3)(1, 0, 1)), _INV),
    (_CALL, dict(ldx=3), _INV),
    (_CALL, dict(ldx=0), _INV),
    # ---- the buffers
    (_CALL, dict(x_bytes=1919), _INV),
    (_CALL, dict(x_bytes=-1), _INV),
    (_CALL, dict(x=None), _INV),
    (_CALL, dict(x=_A2), _INV),
    (_CALL, dict(matrices=None), _INV),
    (_CALL, dict(matrices=_A2), _INV),
    (_CALL, dict(thr=None), _INV),
    (_CALL, dict(thr=_A2), _INV),
    (_CALL, dict(workspace=_M4), _INV),
    (_CALL, dict(workspace_bytes=-1), _INV),
    (_CALL, dict(levels=_A2), _INV),
    (_CALL, dict(levels_bytes=1439), _INV),
    (_CALL, dict(levels_bytes=-1), _INV),
    (_CALL, dict(ldx=2 ** 31 - 1), _INV),                             # S * n * ldx * 4 would wrap 64 bits
    (_CALL, dict(ldx=2 ** 30), _INV),
    # ---- S == 0: CGNN_OK before any buffer is looked at; the request comes before it
    (_CALL, dict(S=0), _OK),
    (_CALL, dict(_EMPTY), _OK),
    (_CALL, dict(_EMPTY, n=1024), _OK),
    (_CALL, dict(_EMPTY, measures=(_i32 * 1)(2), num=1, cols=(_i32 * 1)(0), ldx=1), _OK),
    (_CALL, dict(_EMPTY, n=1025), _INV),
    (_CALL, dict(_EMPTY, num=0), _INV),
    (_CALL, dict(_EMPTY, cols=None), _INV),
    (_CALL, dict(_EMPTY, workspace=_M4), _INV),
    (_CALL, dict(_EMPTY, workspace_bytes=-1), _INV),
    (_CALL, dict(_EMPTY, x_bytes=-1), _INV),
    (_CALL, dict(_EMPTY, levels_bytes=-1), _INV),
]


def test_the_entry_points_check_their_arguments_before_any_launch():
    """No device is present here: a call that went as far as a launch could not return these codes."""
    lib = _lib.load()
    got = []
    for name, change, want in _CALLS:
        args = dict(_DEFAULTS[name])
        unknown = set(change) - set(args)
        assert not unknown, (name, unknown)
        args.update(change)
        got.append((name, change, want, getattr(lib, name)(*args.values())))
    wrong = [(n, c, w, g) for n, c, w, g in got if g != w]
    assert not wrong, wrong
