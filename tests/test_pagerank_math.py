"""PageRank centrality of connectome_gnn_amd.ingest without a device: the fp64 host statement of tests/pagerank_data.py
against ``networkx.pagerank``, the numpy model of the kernel's iteration against the statement, the argument rules of
``centrality_measures``, and the refusals of the C entry point (include/cgnn_pagerank.h), none of which reaches a launch.

Why a step of the iteration is two products.  The cap ``K_max(d) = ceil(43 ln 2 / -ln d) + 2`` is 186 at ``d = 0.85``.  A
product contracts at rate ``d`` and the first change is at most ``2 d``, so with one product a step the stopping rule
``change <= (1 - d) 2^-42`` needs ``2 d^k <= (1 - d) 2^-42``, which ``K_max`` implies only for ``d^2 <= 1 - d``
(``d <= 0.618``).  The star of the cohort attains the rate: it is bipartite, its error alternates in sign and shrinks by
exactly ``d`` a product, and at ``d = 0.85`` a one-product model needs 192 to 196 steps on it (``one_product_steps``
below measures that).  With two products a step the change of step ``K`` is at most ``2 (1 + d) d^(2 K - 1)``, which at
``K_max`` is below ``2^-84`` for every ``d <= 0.99``: the rule holds before the cap in exact arithmetic, and the model
stops before it on every case (at most 93 steps at ``d = 0.85``, 23 at ``d = 0.5``).
"""
import ctypes

import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import pagerank_data as PD
from tests.abi_header import check_header

NAMES = PD.CENTRALITY_MEASURES


# ---- the statement ----
def _networkx(A, t, d, name):
    import networkx as nx
    w = PD.weights(A, t, name)
    n = w.shape[0]
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    G.add_weighted_edges_from((int(j), int(i), float(w[i, j])) for i, j in zip(*np.nonzero(w)))
    pr = nx.pagerank(G, alpha=d, tol=1e-15, max_iter=10 ** 4)
    return np.array([pr[i] for i in range(n)])


@pytest.mark.parametrize("d", PD.DAMPINGS)
@pytest.mark.parametrize("n", [5, 64, 84])
def test_the_statement_is_networkx_pagerank(n, d):
    mats = PD.cohort(n)
    worst = 0.0
    for kw in PD.THRESHOLDS:
        want = PD.cohort_statement(n, kw, d).numpy()
        for s, (A, t) in enumerate(zip(mats, PD.host_thresholds(mats, kw))):
            for col, name in enumerate(NAMES):
                err = float(np.abs(_networkx(A, t, d, name) - want[s, :, col]).max())
                worst = max(worst, err)
                assert err <= 1e-12, (n, d, kw, s, name, err)
    print(f"n={n} d={d}: statement against networkx, largest difference {worst:.3e}")


def test_the_case_worked_by_hand():
    """Entry (i, j) is an edge j -> i: with A[1, 0] alone, node 0 points at node 1 and node 1 is dangling."""
    A = torch.zeros(2, 2)
    A[1, 0] = 0.5
    d = 0.5
    # x0 = d x1 / 2 + (1 - d) / 2, x1 = d (x0 + x1 / 2) + (1 - d) / 2  ->  x0 = 0.4, x1 = 0.6
    for name in NAMES:
        assert np.allclose(PD.host_pagerank(A, 0.0, d, name), [0.4, 0.6], rtol=0, atol=1e-15)
        assert np.allclose(PD.model(A, 0.0, d, name)[0], [0.4, 0.6], rtol=0, atol=1e-13)
    assert np.allclose(PD.host_pagerank(A.t().contiguous(), 0.0, d, "pagerank"), [0.6, 0.4], rtol=0, atol=1e-15)
    assert np.allclose(PD.host_pagerank(A, 0.5, d, "pagerank"), [0.5, 0.5], rtol=0, atol=1e-15), "the threshold is strict"


def test_the_cohort_holds_what_the_cases_need():
    n = 84
    mats = PD.cohort(n)
    assert tuple(mats.shape) == (8, n, n)
    assert not mats[PD.ALL_ZERO].any()
    assert not torch.equal(mats[PD.ASYMMETRIC], mats[PD.ASYMMETRIC].t())
    for s in PD.SYMMETRIC:
        m = PD.MD.kept_mask(mats[s], 0.0)
        assert np.array_equal(m, m.T), s
    w = PD.weights(mats[PD.CLIQUES], 0.0, "pagerank")
    assert not w[n - 1].any() and not w[:, n - 1].any(), "an isolated node"
    h = (n - 1) // 2
    assert w[:h, :h].sum() == h * (h - 1) and not w[:h, h:].any() and not w[h:, :h].any(), "two disjoint cliques"
    w = PD.weights(mats[PD.STAR], 0.0, "pagerank")
    assert w[0, 1:].all() and w[1:, 0].all() and not w[1:, 1:].any()
    # the asymmetric subject tells the j -> i convention from its transpose
    A, d = mats[PD.ASYMMETRIC], 0.85
    for name, t in (("weighted_pagerank", 0.0), ("pagerank", 0.9)):
        assert np.abs(PD.host_pagerank(A, t, d, name) - PD.host_pagerank(A.t().contiguous(), t, d, name)).max() > 1e-4


def test_the_cap_at_085_is_186():
    assert PD.max_steps(0.85) == 186 and ingest.pagerank_max_steps(0.85) == 186
    assert PD.max_steps(0.5) == 45 and ingest.pagerank_max_steps(0.5) == 45
    assert ingest.pagerank_max_steps(0.0) == 2 and ingest.pagerank_max_steps(0) == 2
    for d in (0.1, 0.5, 0.85, 0.9, 0.99):
        K = ingest.pagerank_max_steps(d)
        assert K == PD.max_steps(d) and 2.0 * d ** K <= 2.0 ** -42, "the error bound at the cap"
        assert 2.0 * (1.0 + d) * d ** (2 * K - 1) <= (1.0 - d) * 2.0 ** -42, "the stopping rule holds at the cap"


def one_product_steps(A, t, d, name, limit=400):
    """The steps a model with ONE product a step would take to meet the same rule (module docstring)."""
    n = A.shape[0]
    w = PD.weights(A, t, name)
    c = w.sum(0)
    x = np.full(n, 1.0 / n)
    for k in range(1, limit + 1):
        with np.errstate(invalid="ignore", divide="ignore"):
            y = np.where(c == 0, 0.0, x / c)
        new = d * (w @ y + x[c == 0].sum() / n) + (1.0 - d) / n
        change, x = np.abs(new - x).sum(), new
        if change <= (1.0 - d) * 2.0 ** -42:
            break
    return k


def test_a_star_is_why_a_step_is_two_products():
    d, n = 0.85, 84
    A = PD.cohort(n)[PD.STAR]
    for name in NAMES:
        single = one_product_steps(A, 0.0, d, name)
        assert single > PD.max_steps(d), (name, single, "one product a step runs past the cap on a bipartite graph")
        x, steps = PD.model(A, 0.0, d, name)
        assert steps < PD.max_steps(d) and 2 * steps <= single + 2, (name, steps, single)
        assert np.abs(x - PD.host_pagerank(A, 0.0, d, name)).sum() <= 2.0 ** -40


def _model_cases(d):
    for n in PD.SIZES:
        mats = PD.cohort(n)
        for kw in PD.THRESHOLDS:
            want = PD.cohort_statement(n, kw, d).numpy()
            for s, (A, t) in enumerate(zip(mats, PD.host_thresholds(mats, kw))):
                for col, name in enumerate(NAMES):
                    yield (n, tuple(kw.items()), s, name), PD.model(A, t, d, name), want[s, :, col]


@pytest.mark.parametrize("d", PD.DAMPINGS)
def test_the_model_of_the_iteration_meets_the_statement(d):
    worst, most = 0.0, 0
    for case, (x, steps), want in _model_cases(d):
        assert abs(float(want.sum()) - 1.0) <= 1e-14, (case, "the statement sums to 1")
        assert float(want.min()) >= (1.0 - d) / len(want) * (1 - 1e-12), (case, "the teleport term is a lower bound")
        err = float(np.abs(x - want).sum())
        worst, most = max(worst, err), max(most, steps)
        assert err <= 2.0 ** -40, (case, err)
        assert steps <= PD.max_steps(d), case
    print(f"d={d}: model against the solve, largest L1 error {worst / 2.0 ** -40:.3f} of 2^-40, most steps {most}")


@pytest.mark.parametrize("d", PD.DAMPINGS)
def test_the_model_stops_before_the_cap_on_every_case(d):
    """Checked here so that no device test can hide a capped subject."""
    cap = PD.max_steps(d)
    steps = {case: k for case, (_, k), _ in _model_cases(d)}
    capped = sorted(case for case, k in steps.items() if k >= cap)
    rest = max((k for case, k in steps.items() if case not in capped), default=0)
    print(f"d={d}: cap {cap}, {len(capped)} of {len(steps)} cases ran to the cap, the others took at most {rest} steps")
    assert not capped, (cap, capped)


# ---- the argument rules, without a device ----
def test_the_names_and_the_limits():
    assert ingest.CENTRALITY_MEASURES == NAMES == ("pagerank", "weighted_pagerank")
    assert ingest.PAGERANK_MAX_NODES == 1024 and ingest.PAGERANK_MAX_DAMPING == 0.99
    assert not set(NAMES) & set(ingest._ALL_MEASURES), "a call of its own: the family table is as it was"
    assert len(ingest._FAMILIES) == 4 and len(ingest._ALL_MEASURES) == 17


def test_centrality_measures_checks_its_arguments():
    n = 12
    mats = PD.cohort(n)[:3].contiguous()
    with pytest.raises(ValueError, match="unknown measure 'eigenvector'.*weighted_pagerank"):
        ingest.centrality_measures(mats, keep=0.2, measures=("pagerank", "eigenvector"))
    with pytest.raises(ValueError, match="unknown measure 'degree'"):
        ingest.centrality_measures(mats, keep=0.2, measures=("degree",))
    with pytest.raises(ValueError, match="'pagerank' is named twice"):
        ingest.centrality_measures(mats, keep=0.2, measures=("pagerank", "pagerank"))
    with pytest.raises(ValueError, match="measures is empty"):
        ingest.centrality_measures(mats, keep=0.2, measures=())
    with pytest.raises(TypeError, match="tuple of names"):
        ingest.centrality_measures(mats, keep=0.2, measures="pagerank")
    for bad in (-0.1, 0.995, 1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"damping must lie in \[0, 0.99\]"):
            ingest.centrality_measures(mats, keep=0.2, damping=bad)
    for bad in (True, False, "0.85", None):
        with pytest.raises(TypeError, match="damping must be a number"):
            ingest.centrality_measures(mats, keep=0.2, damping=bad)
    with pytest.raises(ValueError, match=r"centrality_measures takes n <= 1024 nodes"):
        ingest.centrality_measures(torch.zeros(1, 1025, 1025), keep=0.1)
    with pytest.raises(ValueError, match="exactly one of keep=, num_edges= and min_weight="):
        ingest.centrality_measures(mats)
    with pytest.raises(ValueError, match="exactly one of keep=, num_edges= and min_weight="):
        ingest.centrality_measures(mats, keep=0.1, min_weight=0.0)
    with pytest.raises(ValueError, match="exactly one of keep=, num_edges= and min_weight="):
        ingest.centrality_measures(mats, keep=0.1, num_edges=5)
    with pytest.raises(ValueError, match="knn= is a fourth way"):
        ingest.centrality_measures(mats, keep=0.1, knn=3)
    with pytest.raises(ValueError, match="unknown backbone"):
        ingest.centrality_measures(mats, keep=0.1, backbone="tree")
    with pytest.raises(TypeError, match="float32"):
        ingest.centrality_measures(mats.double(), keep=0.1)
    # a valid request gets as far as the device check: there is no CPU path
    for kw in (dict(keep=0.1), dict(min_weight=0.0, measures=("weighted_pagerank",)), dict(knn=3, damping=0),
               dict(backbone="mst", damping=0.99), dict(num_edges=7, measures=NAMES[::-1], damping=0.5)):
        with pytest.raises(RuntimeError, match="ROCm"):
            ingest.centrality_measures(mats, **kw)


# ---- the C ABI ----
def test_the_prototypes_match_their_header_type_by_type():
    hdr = check_header("cgnn_pagerank.h", _lib.PAGERANK_PROTOTYPES,
                       ["cgnn_ingest_pagerank_workspace_bytes", "cgnn_ingest_pagerank"],
                       [("double damping", "float damping")])
    lib = _lib.load()
    for name, value in (("CGNN_PAGERANK", 0), ("CGNN_PAGERANK_WEIGHTED", 1), ("CGNN_NUM_PAGERANK_MEASURES", 2),
                        ("CGNN_PAGERANK_MAX_NODES", 1024), ("CGNN_PAGERANK_MAX_DAMPING", 0.99)):
        assert f"#define {name} {value}\n" in hdr
    assert _lib.PAGERANK_MAX_DAMPING == 0.99
    assert _lib.ABI_VERSION == 2 and lib.cgnn_abi_version() == 2, "the change is additive"


_i32 = ctypes.c_int32
_A, _M4, _A2 = 0x1000, 0x1004, 0x1002      # 16-byte aligned / 4-byte aligned only / not 4-byte aligned: never dereferenced
_INV, _OK = _lib.CGNN_EINVAL, _lib.CGNN_OK
_CALL, _QUERY = "cgnn_ingest_pagerank", "cgnn_ingest_pagerank_workspace_bytes"
_ID2, _COL2 = (_i32 * 2)(0, 1), (_i32 * 2)(3, 1)
_BIG_S = 2 ** 31 // 20 + 1                 # S * n >= 2^31 at n = 20
# defaults that pass every check: S = 6 subjects of n = 20 nodes, both measures into a [S, n, 4] x, and the step counts
_DEFAULTS = {
    _QUERY: dict(S=6, n=20, measures=_ID2, num=2),
    _CALL: dict(matrices=_A, S=6, n=20, thr=_A, measures=_ID2, num=2, cols=_COL2, ldx=4, damping=0.85, workspace=None,
                workspace_bytes=0, x=_A, x_bytes=1920, iterations=_A, iterations_bytes=24, stream=None),
}
_EMPTY = dict(matrices=None, S=0, thr=None, x=None, x_bytes=0, iterations=None, iterations_bytes=0)
_CALLS = [
    # ---- the byte count: no slab, whatever is asked for
    (_QUERY, dict(), 0),
    (_QUERY, dict(measures=(_i32 * 1)(1), num=1), 0),
    (_QUERY, dict(S=0), 0),
    (_QUERY, dict(n=1024), 0),
    (_QUERY, dict(n=1025), _INV),
    (_QUERY, dict(S=-1), _INV),
    (_QUERY, dict(n=0), _INV),
    (_QUERY, dict(measures=None), _INV),
    (_QUERY, dict(measures=None, num=0), _INV),
    (_QUERY, dict(num=3), _INV),
    (_QUERY, dict(num=-1), _INV),
    (_QUERY, dict(measures=(_i32 * 2)(1, 1)), _INV),
    (_QUERY, dict(measures=(_i32 * 1)(2), num=1), _INV),
    (_QUERY, dict(S=_BIG_S), _INV),
    # ---- the call: the request and the cohort (measure_request.h)
    (_CALL, dict(S=-1), _INV),
    (_CALL, dict(n=0), _INV),
    (_CALL, dict(n=-3), _INV),
    (_CALL, dict(n=1025, x_bytes=2 ** 30), _INV),
    (_CALL, dict(S=_BIG_S), _INV),
    (_CALL, dict(num=0), _INV),
    (_CALL, dict(num=-1), _INV),
    (_CALL, dict(num=3), _INV),
    (_CALL, dict(measures=None), _INV),
    (_CALL, dict(cols=None), _INV),
    (_CALL, dict(measures=(_i32 * 2)(0, 2)), _INV),
    (_CALL, dict(measures=(_i32 * 2)(-1, 1)), _INV),
    (_CALL, dict(measures=(_i32 * 2)(1, 1)), _INV),
    (_CALL, dict(cols=(_i32 * 2)(3, 4)), _INV),                       # a column == ldx
    (_CALL, dict(cols=(_i32 * 2)(-1, 1)), _INV),
    (_CALL, dict(cols=(_i32 * 2)(1, 1)), _INV),
    (_CALL, dict(ldx=3), _INV),
    (_CALL, dict(ldx=0), _INV),
    # ---- the damping
    (_CALL, dict(damping=-0.01), _INV),
    (_CALL, dict(damping=0.991), _INV),
    (_CALL, dict(damping=1.0), _INV),
    (_CALL, dict(damping=float("nan")), _INV),
    (_CALL, dict(damping=float("inf")), _INV),
    (_CALL, dict(damping=float("-inf")), _INV),
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
    (_CALL, dict(iterations=_A2), _INV),
    (_CALL, dict(iterations_bytes=23), _INV),
    (_CALL, dict(iterations_bytes=-1), _INV),
    (_CALL, dict(ldx=2 ** 31 - 1), _INV),                             # S * n * ldx * 4 would wrap 64 bits
    (_CALL, dict(ldx=2 ** 30), _INV),
    # ---- S == 0: CGNN_OK before any buffer is looked at; the request and the damping come before it
    (_CALL, dict(S=0), _OK),
    (_CALL, dict(_EMPTY), _OK),
    (_CALL, dict(_EMPTY, n=1024, damping=0.0), _OK),
    (_CALL, dict(_EMPTY, n=1024, damping=0.99), _OK),
    (_CALL, dict(_EMPTY, n=1025), _INV),
    (_CALL, dict(_EMPTY, damping=1.5), _INV),
    (_CALL, dict(_EMPTY, num=0), _INV),
    (_CALL, dict(_EMPTY, cols=None), _INV),
    (_CALL, dict(_EMPTY, workspace=_M4), _INV),
    (_CALL, dict(_EMPTY, workspace_bytes=-1), _INV),
    (_CALL, dict(_EMPTY, x_bytes=-1), _INV),
    (_CALL, dict(_EMPTY, iterations_bytes=-1), _INV),
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
