"""The host statement of the random-walk encodings (tests/rw_data.py): against networkx's transition matrix, against closed
forms, the split table of the header against ``diag(P^k)``, the fp32 model of the fixed arithmetic against the derived
bound; the argument checks of ``ingest.random_walk_encodings``; the header and the binding of cgnn_ingest_rw and the
refusals of the C entry point, none of which reaches a launch.  No device is touched."""
import ctypes

import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import measures_data as MD
from tests import rw_data as RD
from tests.abi_header import check_header


def test_the_constants():
    assert ingest.RW_MAX_STEPS == RD.MAX_STEPS == 8 and ingest.RW_MAX_NODES == 1024
    assert ingest._RW not in ingest._FAMILIES and len(ingest._ALL_MEASURES) == 17
    assert ingest._RW.names == RD.STEPS, "step k has id k - 1"
    assert set(RD.SPLIT) == set(range(2, 9))
    assert all(a + b == k and a == k // 2 and a >= 1 and b <= 4 for k, (a, b) in RD.SPLIT.items())
    import connectome_gnn_amd
    assert "random_walk_encodings" not in connectome_gnn_amd.__all__


# ---- the statement ----
@pytest.mark.parametrize("n", (2, 5, 17, 63))
def test_the_statement_is_networkx_on_symmetric_subjects(n):
    nx = pytest.importorskip("networkx")
    mats = RD.cohort(n)
    for keep in RD.KEEPS + (1.0,):
        thr = RD.host_thresholds(mats, {"keep": keep})
        for s in RD.SYMMETRIC:
            for binary in (False, True):
                a, finite = RD.walk_weights(mats[s], thr[s], binary)
                assert finite and (a == a.T).all(), (n, keep, s)
                g = nx.from_numpy_array(a)
                assert g.number_of_nodes() == n
                W = nx.to_numpy_array(g, nodelist=range(n), weight="weight")
                deg = np.array([g.degree(i, weight="weight") for i in range(n)])
                P = np.divide(W, deg[:, None], out=np.zeros_like(W), where=deg[:, None] > 0)
                want = np.stack([np.diagonal(np.linalg.matrix_power(P, k)) for k in RD.STEPS], 1)
                got = RD.statement(mats[s], thr[s], RD.STEPS, binary)
                assert np.allclose(got, want, rtol=1e-12, atol=1e-15), (n, keep, s, binary)
                assert (got >= 0).all() and (got <= 1 + 1e-12).all() and not got[:, 0].any()


@pytest.mark.parametrize("n", (2, 3, 6, 20, 63))
def test_the_closed_forms(n):
    hub_leaf = RD.statement(RD.star(n), 0.0)
    assert np.allclose(hub_leaf[0], [0, 1, 0, 1, 0, 1, 0, 1], atol=1e-15), "the hub is back after every even step"
    leaf = [0, 1 / (n - 1)] * 4
    assert np.allclose(hub_leaf[1:], np.tile(leaf, (n - 1, 1)), rtol=1e-13, atol=0)
    assert not hub_leaf[:, 0::2].any(), "a star is bipartite: exact zeros"
    for binary in (False, True):
        k_n = RD.statement(RD.complete(n), 0.0, binary=binary)
        assert np.allclose(k_n, np.tile(RD.expected_complete(n), (n, 1)), rtol=1e-12, atol=0), n
    if n % 2 == 0 and n > 2:
        ring = RD.statement(RD.cycle(n), 0.0)
        assert not ring[:, 0::2].any(), "an even cycle is bipartite"
        assert np.allclose(ring[:, 1], 0.5) and (ring[:, 1::2] > 0).all()
    if n >= 4:
        h = n // 2
        pair = RD.statement(RD.two_cliques(n), 0.0)
        assert np.allclose(pair[:h], np.tile(RD.expected_complete(h), (h, 1)), rtol=1e-12, atol=0)
        assert np.allclose(pair[h:], np.tile(RD.expected_complete(n - h), (n - h, 1)), rtol=1e-12, atol=0)


def test_the_exact_zeros_and_the_infinity_of_the_statement():
    n = 9
    assert not RD.statement(torch.zeros(n, n), 0.0).any(), "no edge"
    assert RD.statement(torch.zeros(1, 1), 0.0).tolist() == [[0.0] * 8], "one node"
    A = RD.complete(n)
    A[4, :] = 0.0
    A[:, 4] = 0.0
    assert not RD.statement(A, 0.0)[4].any(), "an isolated node"
    odd = RD.statement(RD.bipartite(n), 0.0)[:, 0::2]
    assert not odd.any() and not np.signbit(odd).any()
    A = RD.complete(n)
    A[2, 5] = float("nan")
    with_nan = RD.statement(A, 0.0)
    assert np.isfinite(with_nan).all(), "a NaN is never an edge"
    B = RD.complete(n)
    B[2, 5] = 0.0
    assert (with_nan == RD.statement(B, 0.0)).all()
    A[2, 5] = float("inf")
    r = RD.statement(A, 0.0)
    assert not r[:, 0].any() and np.isnan(r[:, 1:]).all()
    assert np.isfinite(RD.statement(A, 0.0, binary=True)).all(), "binary never reads a weight as a number"
    A[2, 5] = 0.0
    A[3, 3] = float("inf")
    assert np.isfinite(RD.statement(A, 0.0)).all(), "the diagonal is never kept"


@pytest.mark.parametrize("n", (2, 5, 17, 40))
def test_the_split_table_gives_the_diagonal_of_the_power_on_asymmetric_matrices(n):
    mats = RD.cohort(n)
    A = mats[RD.ASYMMETRIC]
    for keep in RD.KEEPS + (1.0,):
        t = RD.host_thresholds(mats, {"keep": keep})[RD.ASYMMETRIC]
        for binary in (False, True):
            a, _ = RD.walk_weights(A, t, binary)
            if keep == 1.0 and n > 2 and not binary:
                assert not (a == a.T).all()
            P = RD.transition(a)
            want = RD.statement(A, t, RD.STEPS, binary)
            for k in RD.SPLIT:
                assert np.allclose(RD.split_statement(P, k), want[:, k - 1], rtol=1e-12, atol=1e-300), (n, keep, k)
    # any subset and order of the steps is a selection of columns
    sub = RD.statement(A, 0.0, (8, 3))
    assert (sub == RD.statement(A, 0.0)[:, [7, 2]]).all()


# ---- the fp32 model against the bound ----
def _model_cases(n):
    if n == 1024:                                       # one asymmetric subject: the model's loop is the cost
        return [(RD.large(n)[0], 0.05, False)]
    mats = RD.cohort(n)
    cases = [(mats[s], keep, binary) for s in (0, RD.ASYMMETRIC) for keep in (0.05, 0.30, 0.60) for binary in (False, True)]
    return cases if n <= 193 else cases[::3]


@pytest.mark.parametrize("n", RD.MODEL_SIZES)
def test_the_fp32_model_stays_inside_the_bound(n):
    worst = 0.0
    for A, keep, binary in _model_cases(n):
        t = RD.host_thresholds(A[None], {"keep": keep})[0]
        want = RD.statement(A, t, RD.STEPS, binary)
        got = RD.model(A, t, binary)
        assert not got[:, 0].any()
        share = RD.share_of_bound(got, want, n)
        worst = max(worst, share)
        assert share <= 1.0, (n, keep, binary, share)
    print(f"n={n}: the fp32 model's largest error is {worst:.3f} of the bound")


def test_the_model_keeps_the_exact_zeros():
    n = 17
    odd = RD.model(RD.bipartite(n), 0.0)[:, 0::2]
    assert not odd.any() and not np.signbit(odd).any()
    assert not RD.model(torch.zeros(n, n), 0.0).any()


# ---- the Python arguments ----
def test_random_walk_encodings_checks_its_arguments():
    mats = RD.cohort(5)[:3].contiguous()
    call = ingest.random_walk_encodings
    with pytest.raises(ValueError, match="random_walk_encodings takes n <= 1024 nodes"):
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
    for steps in (0, 9, -1, (0,), (1, 9), [3, -2]):
        with pytest.raises(ValueError, match=r"a step must lie in 1 \.\. RW_MAX_STEPS = 8"):
            call(mats, keep=0.1, steps=steps)
    for steps in (2.0, True, "8", None, (1, 2.0), (True,), ("3",), np.arange(1, 4)):
        with pytest.raises(TypeError, match="steps must be an int or a tuple of ints"):
            call(mats, keep=0.1, steps=steps)
    with pytest.raises(ValueError, match="step 3 is named twice"):
        call(mats, keep=0.1, steps=(3, 1, 3))
    with pytest.raises(ValueError, match="steps is empty"):
        call(mats, keep=0.1, steps=())
    with pytest.raises(TypeError, match="binary must be a bool"):
        call(mats, keep=0.1, binary=1)
    # a valid request gets as far as the device check: there is no CPU path
    for kw in (dict(keep=0.1), dict(min_weight=0.0), dict(knn=3), dict(backbone="mst"), dict(num_edges=7),
               dict(keep=0.5, group="mean"), dict(keep=0.1, steps=4), dict(keep=0.1, steps=(8, 3), binary=True),
               dict(keep=0.1, steps=[2, 1])):
        with pytest.raises(RuntimeError, match="ROCm"):
            call(mats, **kw)
    assert ingest._check_steps(3) == [0, 1, 2] and ingest._check_steps((8, 3)) == [7, 2]
    assert ingest._check_steps(8) == list(range(8)) and ingest._check_steps([5]) == [4]


# ---- the C ABI ----
def test_the_prototypes_match_their_header_type_by_type():
    hdr = check_header("cgnn_rw.h", _lib.RW_PROTOTYPES, ["cgnn_ingest_rw_workspace_bytes", "cgnn_ingest_rw"],
                       [("int32_t flags, ", ""), ("const int32_t* steps", "int32_t steps")])
    assert len(_lib.PROTOTYPES) == 127
    lib = _lib.load()
    for name, value in (("CGNN_RW_MAX_STEPS", ingest.RW_MAX_STEPS), ("CGNN_RW_MAX_NODES", ingest.RW_MAX_NODES),
                        ("CGNN_RW_BINARY", _lib.RW_BINARY)):
        assert f"#define {name} {value}\n" in hdr
    assert _lib.ABI_VERSION == 2 and lib.cgnn_abi_version() == 2, "the change is additive"


_i32 = ctypes.c_int32
_A, _M4, _A2 = 0x1000, 0x1004, 0x1002      # 16-byte aligned / 4-byte aligned only / not 4-byte aligned: never dereferenced
_INV, _OK = _lib.CGNN_EINVAL, _lib.CGNN_OK
_CALL, _QUERY = "cgnn_ingest_rw", "cgnn_ingest_rw_workspace_bytes"
_ID8, _COL8 = (_i32 * 8)(*range(8)), (_i32 * 8)(8, 7, 6, 5, 4, 3, 2, 0)
_ID2, _COL2 = (_i32 * 2)(1, 0), (_i32 * 2)(0, 8)
_BIG_S = 2 ** 31 // 20 + 1                 # S * n >= 2^31 at n = 20
_SLAB = 96 * 96 * 4                        # a slab at n = 20
# defaults that pass every check but the workspace's: S = 6 subjects of n = 20 nodes, all steps into a [S, n, 9] x;
# a grid of 6 workgroups with 3 slabs each
_DEFAULTS = {
    _QUERY: dict(S=6, n=20, steps=_ID8, num=8),
    _CALL: dict(matrices=_A, S=6, n=20, thr=_A, steps=_ID8, num=8, cols=_COL8, ldx=9, flags=0, workspace=_A,
                workspace_bytes=6 * 3 * _SLAB - 1, x=_A, x_bytes=4320, stream=None),
}
_EMPTY = dict(matrices=None, S=0, thr=None, workspace=None, workspace_bytes=0, x=None, x_bytes=0)
_CALLS = [
    # ---- the byte count: a slab set per workgroup, as many slabs as the largest step needs
    (_QUERY, dict(), 6 * 3 * _SLAB),
    (_QUERY, dict(steps=(_i32 * 1)(6), num=1), 6 * 3 * _SLAB),
    (_QUERY, dict(steps=(_i32 * 2)(5, 0), num=2), 6 * 2 * _SLAB),
    (_QUERY, dict(steps=(_i32 * 1)(4), num=1), 6 * 2 * _SLAB),
    (_QUERY, dict(steps=(_i32 * 1)(3), num=1), 6 * _SLAB),
    (_QUERY, dict(steps=(_i32 * 1)(2), num=1), 6 * _SLAB),
    (_QUERY, dict(steps=_ID2, num=2), 0),
    (_QUERY, dict(S=0), 0),
    (_QUERY, dict(S=1, n=1024), 3 * 1056 * 1056 * 4),
    (_QUERY, dict(S=1, n=96), 3 * _SLAB),
    (_QUERY, dict(S=1, n=97), 3 * 4 * _SLAB),
    (_QUERY, dict(n=1025), _INV),
    (_QUERY, dict(S=-1), _INV),
    (_QUERY, dict(n=0), _INV),
    (_QUERY, dict(steps=None), _INV),
    (_QUERY, dict(steps=None, num=0), _INV),
    (_QUERY, dict(num=9), _INV),
    (_QUERY, dict(num=-1), _INV),
    (_QUERY, dict(steps=(_i32 * 2)(1, 1), num=2), _INV),
    (_QUERY, dict(steps=(_i32 * 1)(8), num=1), _INV),
    (_QUERY, dict(S=_BIG_S), _INV),
    # ---- the call: everything is in order but the workspace, which is one byte short
    (_CALL, dict(), _INV),
    (_CALL, dict(workspace=None, workspace_bytes=0), _INV),
    (_CALL, dict(workspace_bytes=0), _INV),
    (_CALL, dict(steps=(_i32 * 8)(7, 6, 5, 4, 3, 2, 1, 0), workspace_bytes=6 * 2 * _SLAB), _INV),
    # ---- the call: the request and the cohort (measure_request.h)
    (_CALL, dict(S=-1), _INV),
    (_CALL, dict(n=0), _INV),
    (_CALL, dict(n=-3), _INV),
    (_CALL, dict(n=1025, x_bytes=2 ** 30, workspace_bytes=2 ** 40), _INV),
    (_CALL, dict(S=_BIG_S), _INV),
    (_CALL, dict(num=0), _INV),
    (_CALL, dict(num=-1), _INV),
    (_CALL, dict(num=9), _INV),
    (_CALL, dict(steps=None), _INV),
    (_CALL, dict(cols=None), _INV),
    (_CALL, dict(steps=(_i32 * 2)(0, 8), num=2, cols=_COL2), _INV),
    (_CALL, dict(steps=(_i32 * 2)(-1, 1), num=2, cols=_COL2), _INV),
    (_CALL, dict(steps=(_i32 * 2)(1, 1), num=2, cols=_COL2), _INV),
    (_CALL, dict(steps=_ID2, num=2, cols=(_i32 * 2)(0, 9)), _INV),    # a column == ldx
    (_CALL, dict(steps=_ID2, num=2, cols=(_i32 * 2)(-1, 1)), _INV),
    (_CALL, dict(steps=_ID2, num=2, cols=(_i32 * 2)(1, 1)), _INV),
    (_CALL, dict(ldx=8), _INV),
    (_CALL, dict(ldx=0), _INV),
    (_CALL, dict(flags=2, workspace_bytes=2 ** 40), _INV),
    (_CALL, dict(flags=-1, workspace_bytes=2 ** 40), _INV),
    # ---- the buffers, with a workspace that is long enough: the refusal is theirs
    (_CALL, dict(workspace_bytes=2 ** 40, x_bytes=4319), _INV),
    (_CALL, dict(workspace_bytes=2 ** 40, x_bytes=-1), _INV),
    (_CALL, dict(workspace_bytes=2 ** 40, x=None), _INV),
    (_CALL, dict(workspace_bytes=2 ** 40, x=_A2), _INV),
    (_CALL, dict(workspace_bytes=2 ** 40, matrices=None), _INV),
    (_CALL, dict(workspace_bytes=2 ** 40, matrices=_A2), _INV),
    (_CALL, dict(workspace_bytes=2 ** 40, thr=None), _INV),
    (_CALL, dict(workspace_bytes=2 ** 40, thr=_A2), _INV),
    (_CALL, dict(workspace_bytes=2 ** 40, workspace=_M4), _INV),
    (_CALL, dict(workspace_bytes=-1), _INV),
    (_CALL, dict(workspace_bytes=2 ** 40, ldx=2 ** 31 - 1), _INV),    # S * n * ldx * 4 would wrap 64 bits
    (_CALL, dict(workspace_bytes=2 ** 40, ldx=2 ** 30), _INV),
    # ---- S == 0: CGNN_OK before any buffer is looked at; the request comes before it
    (_CALL, dict(S=0), _OK),
    (_CALL, dict(_EMPTY), _OK),
    (_CALL, dict(_EMPTY, n=1024), _OK),
    (_CALL, dict(_EMPTY, flags=1), _OK),
    (_CALL, dict(_EMPTY, steps=(_i32 * 1)(7), num=1, cols=(_i32 * 1)(0), ldx=1), _OK),
    (_CALL, dict(_EMPTY, n=1025), _INV),
    (_CALL, dict(_EMPTY, num=0), _INV),
    (_CALL, dict(_EMPTY, cols=None), _INV),
    (_CALL, dict(_EMPTY, flags=4), _INV),
    (_CALL, dict(_EMPTY, workspace=_M4), _INV),
    (_CALL, dict(_EMPTY, workspace_bytes=-1), _INV),
    (_CALL, dict(_EMPTY, x_bytes=-1), _INV),
]


def test_the_entry_points_check_their_arguments_before_any_launch():
    """No device is present here: a call that went as far as a launch could not return these codes.  (Every refused call
    keeps a workspace that is too short or has another argument out of order, so none can reach the launch on a machine
    that has a device either.)"""
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
