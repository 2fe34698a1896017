"""The module measures of connectome_gnn_amd.ingest without a device: the fp64 host statement of tests/modules_data.py
pinned on a case worked by hand, against independent one-line numpy forms and on its properties; ``_check_modules`` and
the argument rules of ``modules=``; and the refusals of the C entry point (include/cgnn_modules.h), none of which
reaches a launch.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import ingest_data as I
from tests import modules_data as D
from tests import timeseries_data as TS
from tests.abi_header import check_header

NAMES = D.MODULE_MEASURES


def _random_subject(n, seed, density=0.4, symmetric=True):
    g = torch.Generator().manual_seed(seed)
    A = torch.rand(n, n, generator=g)
    if symmetric:
        A = torch.maximum(A, A.t())
    A = torch.where(torch.rand(n, n, generator=g) < density, A, torch.zeros(n, n))
    return D.clamp_weights(A)


# ---- the statement ----
def test_the_case_worked_by_hand():
    A = torch.zeros(4, 4)
    for i, j, w in ((0, 1, 1.0), (0, 2, 1.0), (2, 3, 2.0)):
        A[i, j] = A[j, i] = w
    c = [0, 0, 1, 1]
    got = D.host_module_measures(A, 0.0, c).numpy()
    h = -(1 / 3 * math.log(1 / 3) + 2 / 3 * math.log(2 / 3)) / math.log(2)
    want = {"participation": [0.5, 0.0, 0.5, 0.0], "weighted_participation": [0.5, 0.0, 4 / 9, 0.0],
            "module_zscore": [0.0] * 4, "weighted_module_zscore": [0.0] * 4, "diversity": [1.0, 0.0, h, 0.0]}
    for col, name in enumerate(NAMES):
        assert np.allclose(got[:, col], want[name], rtol=0, atol=1e-15), (name, got[:, col])
    assert got[:, 2].tolist() == [0.0] * 4 and got[:, 3].tolist() == [0.0] * 4, "every module's values are equal: exactly 0"
    assert D.host_profile(A, 0.0, c).tolist() == [[1, 1], [1, 0], [1, 2], [0, 2]]
    assert D.host_profile(A, 0.0, c, binary=True).tolist() == [[1, 1], [1, 0], [1, 1], [0, 1]]
    assert D.host_profile(A, 0.0, c, normalize=True).tolist() == [[0.5, 0.5], [1, 0], [1 / 3, 2 / 3], [0, 1]]
    assert D.host_profile(A, 1.0, c).tolist() == [[0, 0], [0, 0], [0, 2], [0, 2]], "the threshold is strict"


@pytest.mark.parametrize("n,M,symmetric", [(9, 3, True), (20, 7, False), (33, 17, True), (40, 40, False), (12, 1, True)])
def test_the_statement_against_one_line_numpy_forms(n, M, symmetric):
    A = _random_subject(n, seed=n + M, symmetric=symmetric)
    c = D.partition(n, M, seed=3)
    t = 0.2
    mask = ((A > t) & (A > 0) & ~torch.eye(n, dtype=torch.bool)).numpy()
    a = np.where(mask, A.numpy().astype(np.float64), 0.0)
    onehot = np.eye(M)[c]
    km, sm = mask.astype(np.float64) @ onehot, a @ onehot
    got_k, got_s = D.module_sums(A, t, c)
    assert np.array_equal(got_k, km) and np.array_equal(got_s, sm), "weights in [2^-10, 1]: the sums are exact"
    got = D.host_module_measures(A, t, c).numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        k, s = km.sum(1), sm.sum(1)
        part = np.where(k > 0, 1 - ((km / k[:, None]) ** 2).sum(1), 0.0)
        wpart = np.where(s > 0, 1 - ((sm / s[:, None]) ** 2).sum(1), 0.0)
        p = sm / s[:, None]
        div = np.where(s > 0, -np.where(p > 0, p * np.log(p), 0.0).sum(1) / (math.log(M) if M > 1 else 1.0), 0.0)
    if M == 1:
        div = np.zeros(n)
    kappa, sigma = km[np.arange(n), c], sm[np.arange(n), c]
    for col, want in ((0, part), (1, wpart), (4, div)):
        assert np.allclose(got[:, col], want, rtol=1e-13, atol=1e-15), NAMES[col]
    for col, v in ((2, kappa), (3, sigma)):
        for m in range(M):
            idx = np.nonzero(c == m)[0]
            sd = np.std(v[idx])
            want = (v[idx] - v[idx].mean()) / sd if sd > 1e-12 else np.zeros(len(idx))
            assert np.allclose(got[idx, col], want, rtol=1e-11, atol=1e-13), (NAMES[col], m)
    for binary in (False, True):
        v = km if binary else sm
        assert np.array_equal(D.host_profile(A, t, c, binary).numpy(), v)
        with np.errstate(invalid="ignore", divide="ignore"):
            norm = np.where(v.sum(1, keepdims=True) > 0, v / v.sum(1, keepdims=True), 0.0)
        assert np.allclose(D.host_profile(A, t, c, binary, True).numpy(), norm, rtol=1e-15, atol=0)


def test_one_module_gives_zero_participation_and_diversity():
    A = _random_subject(15, seed=1)
    got = D.host_module_measures(A, 0.1, np.zeros(15, dtype=np.int64)).numpy()
    assert not got[:, [0, 1, 4]].any()
    assert got[:, 2].any() and got[:, 3].any(), "the z-scores are those of the whole graph"


def test_a_singleton_module_has_zscore_zero():
    n, M = 30, 5
    c = D.partition(n, M, seed=2, kind="singleton")
    assert D.has_singleton(c)
    alone = int(np.nonzero(c == M - 1)[0][0])
    got = D.host_module_measures(_random_subject(n, seed=5), 0.1, c).numpy()
    assert got[alone, 2] == 0.0 and got[alone, 3] == 0.0
    assert got[:, 2].any() and got[:, 3].any()


def test_three_bit_equal_values_are_all_equal_whatever_their_mean():
    v = np.array([0.1, 0.1, 0.1, 0.7])
    c = np.array([0, 0, 0, 1])
    assert v[:3].sum() / 3 != 0.1, "the mean of three equal doubles is not that double"
    assert D._zscore(v, c).tolist() == [0.0] * 4


def test_an_isolated_node_is_zero_everywhere():
    n, M = 20, 4
    A = _random_subject(n, seed=7)
    A[5, :] = 0.0
    c = D.partition(n, M, seed=1)
    got = D.host_module_measures(A, 0.0, c).numpy()
    km, _ = D.module_sums(A, 0.0, c)
    assert not km[5].any()
    assert got[5, [0, 1, 4]].tolist() == [0.0, 0.0, 0.0]
    for binary in (False, True):
        assert not D.host_profile(A, 0.0, c, binary, True)[5].any()
        assert not D.host_profile(A, 0.0, c, binary, False)[5].any()
    # with every node of its module isolated, the z-scores are 0 too
    members = np.nonzero(c == c[5])[0]
    A[members, :] = 0.0
    got = D.host_module_measures(A, 0.0, c).numpy()
    assert not got[members].any()


@pytest.mark.parametrize("n,M", [(24, 6), (33, 17)])
def test_relabelling_the_modules_permutes_the_profile_and_nothing_else(n, M):
    A = _random_subject(n, seed=11, symmetric=False)
    c = D.partition(n, M, seed=4)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(5)).numpy()
    c2 = perm[c]
    a, b = D.host_module_measures(A, 0.3, c).numpy(), D.host_module_measures(A, 0.3, c2).numpy()
    assert np.array_equal(a[:, [2, 3]], b[:, [2, 3]]), "the z-scores see one module at a time"
    assert np.allclose(a, b, rtol=0, atol=1e-14), "the sums over m run in another order"
    for binary in (False, True):
        for normalize in (False, True):
            p, p2 = D.host_profile(A, 0.3, c, binary, normalize).numpy(), D.host_profile(A, 0.3, c2, binary, normalize).numpy()
            assert np.array_equal(p2[:, perm], p), (binary, normalize)


def test_the_shared_cohorts_meet_the_condition_of_the_one_rounding_bound():
    for n, M in ((5, 2), (65, 7), (84, 17)):
        mats, c = D.cohort(n), D.case_partition(n, M)
        for kw in D.THRESHOLDS:
            got = D.cohort_statement(mats, D.host_thresholds(mats, kw), c)
            assert tuple(got.shape) == (6, n, 5) and bool(torch.isfinite(got).all())
    assert D.kind_of(65, 7) == "singleton" and D.kind_of(84, 17) == "blocks" and D.kind_of(84, 64) == "scattered"
    assert D.has_singleton(D.case_partition(65, 7)) and D.straddles(D.case_partition(65, 7))
    lengths = np.bincount(D.case_partition(84, 17))
    assert len(lengths) == 17 and lengths.min() >= 1 and len(set(lengths.tolist())) > 1
    with pytest.raises(AssertionError, match="sigma"):
        D.cohort_statement(D.cohort(84), D.host_thresholds(D.cohort(84), {"keep": 0.5}), D.partition(84, 17, 0, "blocks"))


# ---- _check_modules ----
def test_check_modules_takes_sequences_arrays_and_cpu_tensors():
    want = [0, 2, 1, 1, 0]
    for given in (want, tuple(want), np.array(want), np.array(want, dtype=np.int16), torch.tensor(want),
                  torch.tensor(want, dtype=torch.int32), torch.tensor(want, dtype=torch.uint8)):
        labels, M = ingest._check_modules(given, 5)
        assert M == 3 and labels.dtype == torch.int32 and labels.device.type == "cpu" and labels.is_contiguous()
        assert labels.tolist() == want
    labels, M = ingest._check_modules(range(64), 64)
    assert M == ingest.MODULE_MAX == 64 and labels.tolist() == list(range(64))
    assert ingest._check_modules(torch.tensor([0, 9, 1, 9, 2, 9])[::2], 3)[0].tolist() == [0, 1, 2], "a strided tensor"


@pytest.mark.parametrize("given,n,error,match", [
    ([0, 1, 1], 4, ValueError, r"\[n\] = \[4\].*\(3,\)"),
    ([[0, 1], [1, 0]], 4, ValueError, r"\[n\] = \[4\].*\(2, 2\)"),
    ([], 3, ValueError, r"\[n\] = \[3\]"),
    ([0, 1, -1], 3, ValueError, "0 .. M - 1, got -1"),
    ([0, 2, 2], 3, ValueError, r"\[1\] have no ROI"),
    ([1, 2, 4, 4], 4, ValueError, r"\[0, 3\] have no ROI"),
    (list(range(65)), 65, ValueError, "M = 65 modules: at most MODULE_MAX = 64"),
    ([0.0, 1.0], 2, TypeError, "integer labels, got float64"),
    ([True, False], 2, TypeError, "integer labels, got bool"),
    (np.array([0.5, 1.0]), 2, TypeError, "integer labels, got float64"),
    (torch.tensor([0.0, 1.0]), 2, TypeError, "integer labels, got torch.float32"),
    (torch.tensor([True, False]), 2, TypeError, "integer labels, got torch.bool"),
    ("01", 2, TypeError, "got str"),
    (3, 2, TypeError, "got int"),
    ({0: 1}, 1, TypeError, "got dict"),
], ids=lambda v: None)
def test_check_modules_names_the_offender(given, n, error, match):
    with pytest.raises(error, match=match):
        ingest._check_modules(given, n)


def test_check_modules_refuses_a_device_tensor_and_says_why():
    with pytest.raises(ValueError, match="modules are on meta.*read-back"):
        ingest._check_modules(torch.zeros(4, dtype=torch.int64, device="meta"), 4)


# ---- the argument rules, without a device ----
def test_the_families_and_their_names():
    assert ingest.MODULE_MEASURES == NAMES and ingest.MODULE_MAX == 64 and ingest.MODULE_MAX_NODES == 1024
    fam = ingest._FAMILIES[3]
    assert fam.names is ingest.MODULE_MEASURES and fam.call == "cgnn_ingest_modules" and fam.cols and fam.modules
    assert not fam.dist and fam.max_nodes == 1024
    assert [f.modules for f in ingest._FAMILIES] == [False, False, False, True]
    assert ingest._ALL_MEASURES == ingest.MEASURES + ingest.PATH_MEASURES + ingest.WEIGHTED_PATH_MEASURES + NAMES
    assert len(ingest._ALL_MEASURES) == 17
    with pytest.raises(ValueError, match="unknown measure 'modularity'.*weighted_module_zscore"):
        ingest._measure_ids(("modularity",))
    assert ingest._measure_ids(("diversity", "degree", "participation")) == [(fam, 4), (ingest._FAMILIES[0], 1), (fam, 0)]


def _entry_points(n=12, S=3):
    mats, y = D.cohort(n)[:S].contiguous(), I.labels(S)
    ts = TS.recipe(S, 30, n)
    return {
        "node_measures": lambda **kw: ingest.node_measures(mats, keep=0.2, **kw),
        "from_matrices": lambda **kw: ingest.from_matrices(mats, y, keep=0.2, **kw),
        "from_timeseries": lambda **kw: ingest.from_timeseries(ts, y, keep=0.2, **kw),
    }


@pytest.mark.parametrize("entry", ["node_measures", "from_matrices", "from_timeseries"])
def test_modules_go_with_module_measures_and_only_with_them(entry):
    n = 12
    call = _entry_points(n)[entry]
    c = D.partition(n, 3)
    with pytest.raises(ValueError, match=r"\('participation',\) need the partition: give modules="):
        call(measures=("degree", "participation"))
    with pytest.raises(ValueError, match=r"\('diversity', 'module_zscore'\) need the partition"):
        call(measures=("diversity", "closeness", "module_zscore"))
    with pytest.raises(ValueError, match="modules= was given but no measure of MODULE_MEASURES"):
        call(measures=("degree", "closeness"), modules=c)
    if entry != "node_measures":
        with pytest.raises(ValueError, match="modules= was given but no measure of MODULE_MEASURES"):
            call(modules=c)
        with pytest.raises(ValueError, match="modules= was given but no measure of MODULE_MEASURES"):
            call(measures=True, modules=c)                  # True still means the five classic names
    with pytest.raises(ValueError, match=r"\[n\] = \[12\]"):
        call(measures=("participation",), modules=c[:-1])
    with pytest.raises(ValueError, match=r"\[2\] have no ROI"):
        call(measures=("participation",), modules=np.where(c == 2, 3, c))
    with pytest.raises(TypeError, match="integer labels"):
        call(measures=("participation",), modules=c.astype(np.float32))
    with pytest.raises(ValueError, match="named twice"):
        call(measures=("participation", "participation"), modules=c)
    # a valid request gets as far as the device check: there is no CPU path
    for names in (NAMES, ("module_zscore",), ("weighted_closeness", "diversity", "strength", "local_efficiency")):
        with pytest.raises(RuntimeError, match="ROCm"):
            call(measures=names, modules=c)
        with pytest.raises(RuntimeError, match="ROCm"):
            call(measures=names, modules=torch.tensor(c))


def test_module_profile_checks_its_arguments():
    n = 12
    mats, c = D.cohort(n)[:3].contiguous(), D.partition(n, 3)
    with pytest.raises(ValueError, match="exactly one of keep=, num_edges= and min_weight="):
        ingest.module_profile(mats, c)
    with pytest.raises(ValueError, match="knn= is a fourth way"):
        ingest.module_profile(mats, c, keep=0.1, knn=3)
    with pytest.raises(ValueError, match=r"\[n\] = \[12\]"):
        ingest.module_profile(mats, c[:5], keep=0.1)
    with pytest.raises(TypeError, match="got NoneType"):
        ingest.module_profile(mats, None, keep=0.1)
    with pytest.raises(ValueError, match="module_profile takes n <= 1024 nodes"):
        ingest.module_profile(torch.zeros(1, 1025, 1025), np.zeros(1025, dtype=np.int64), keep=0.1)
    for kw in (dict(keep=0.1), dict(min_weight=0.0, binary=True), dict(knn=3, normalize=True)):
        with pytest.raises(RuntimeError, match="ROCm"):
            ingest.module_profile(mats, c, **kw)


def test_module_measures_refuse_more_than_1024_nodes():
    big, c = torch.zeros(1, 1025, 1025), np.zeros(1025, dtype=np.int64)
    with pytest.raises(ValueError, match=r"module measures .* take n <= 1024 nodes \(a row lives in 16 registers"):
        ingest.node_measures(big, keep=0.1, measures=("degree", "diversity"), modules=c)
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.from_matrices(big, I.labels(1), keep=0.1, measures=("participation",), modules=c)


# ---- the C ABI ----
def test_the_prototypes_match_their_header_type_by_type():
    """The two entry points are declared in include/cgnn_modules.h, which cgnn.h includes, and bound by
    ``_lib.MODULE_PROTOTYPES``: every type, the library's exports, the constants, and the comparison itself against a
    doctored header."""
    hdr = check_header("cgnn_modules.h", _lib.MODULE_PROTOTYPES,
                       ["cgnn_ingest_modules_workspace_bytes", "cgnn_ingest_modules"],
                       [("int32_t M, const", "int64_t M, const")])
    lib = _lib.load()
    for name, value in (("CGNN_NUM_MODULE_MEASURES", 5), ("CGNN_MODULE_MAX", 64), ("CGNN_MODULE_MAX_NODES", 1024),
                        ("CGNN_MODULE_PROFILE_BINARY", 1), ("CGNN_MODULE_PROFILE_NORMALIZE", 2)):
        assert f"#define {name} {value}\n" in hdr
    for i, name in enumerate(NAMES):
        macro = {"module_zscore": "ZSCORE", "weighted_module_zscore": "WEIGHTED_ZSCORE"}.get(name, name.upper())
        assert f"#define CGNN_MODULE_{macro} {i}\n" in hdr
    assert (_lib.MODULE_PROFILE_BINARY, _lib.MODULE_PROFILE_NORMALIZE) == (1, 2)
    assert _lib.ABI_VERSION == 2 and lib.cgnn_abi_version() == 2, "the change is additive"


_i32 = ctypes.c_int32
_A, _M4, _A2 = 0x1000, 0x1004, 0x1002      # 16-byte aligned / 4-byte aligned only / not 4-byte aligned: never dereferenced
_INV, _OK = _lib.CGNN_EINVAL, _lib.CGNN_OK
_CALL, _QUERY = "cgnn_ingest_modules", "cgnn_ingest_modules_workspace_bytes"
_ID5, _COL5 = (_i32 * 5)(0, 1, 2, 3, 4), (_i32 * 5)(6, 0, 3, 5, 1)
_BIG_S = 2 ** 31 // 20 + 1                 # S * n >= 2^31 at n = 20
# defaults that pass every check: S = 6 subjects of n = 20 nodes, M = 7, all five measures into a [S, n, 7] x and a profile
_DEFAULTS = {
    _QUERY: dict(S=6, n=20, measures=_ID5, num=5),
    _CALL: dict(matrices=_A, S=6, n=20, thr=_A, modules=_A, M=7, measures=_ID5, num=5, cols=_COL5, ldx=7, workspace=None,
                workspace_bytes=0, x=_A, x_bytes=3360, profile=_A, profile_bytes=3360, flags=3, stream=None),
}
_NOTHING = dict(measures=None, num=0, cols=None, ldx=0, x=None, x_bytes=0)          # no measure: the profile alone
_EMPTY = dict(matrices=None, S=0, thr=None, modules=None, x=None, x_bytes=0, profile=None, profile_bytes=0)
_CALLS = [
    # ---- the byte count: no slab, whatever is asked for
    (_QUERY, dict(), 0),
    (_QUERY, dict(measures=None, num=0), 0),
    (_QUERY, dict(measures=(_i32 * 1)(2), num=1), 0),
    (_QUERY, dict(S=0), 0),
    (_QUERY, dict(n=1024), 0),
    (_QUERY, dict(n=1025), _INV),
    (_QUERY, dict(S=-1), _INV),
    (_QUERY, dict(n=0), _INV),
    (_QUERY, dict(measures=None), _INV),
    (_QUERY, dict(num=6), _INV),
    (_QUERY, dict(num=-1), _INV),
    (_QUERY, dict(measures=(_i32 * 2)(3, 3), num=2), _INV),
    (_QUERY, dict(measures=(_i32 * 1)(5), num=1), _INV),
    (_QUERY, dict(S=_BIG_S), _INV),
    # ---- the call: the request and the cohort (measure_request.h)
    (_CALL, dict(S=-1), _INV),
    (_CALL, dict(n=0), _INV),
    (_CALL, dict(n=-3), _INV),
    (_CALL, dict(n=1025, M=7), _INV),                                 # what the other families return for it
    (_CALL, dict(S=_BIG_S), _INV),
    (_CALL, dict(num=-1), _INV),
    (_CALL, dict(num=6), _INV),
    (_CALL, dict(measures=None), _INV),
    (_CALL, dict(cols=None), _INV),
    (_CALL, dict(measures=(_i32 * 5)(0, 1, 2, 3, 5)), _INV),
    (_CALL, dict(measures=(_i32 * 5)(0, -1, 2, 3, 4)), _INV),
    (_CALL, dict(measures=(_i32 * 5)(0, 1, 2, 3, 3)), _INV),
    (_CALL, dict(cols=(_i32 * 5)(6, 0, 3, 5, 7)), _INV),              # a column == ldx
    (_CALL, dict(cols=(_i32 * 5)(6, -1, 3, 5, 1)), _INV),
    (_CALL, dict(cols=(_i32 * 5)(6, 0, 3, 6, 1)), _INV),
    (_CALL, dict(ldx=6), _INV),
    (_CALL, dict(ldx=0), _INV),
    # ---- the partition
    (_CALL, dict(M=0), _INV),
    (_CALL, dict(M=-1), _INV),
    (_CALL, dict(M=21), _INV),                                        # M > n
    (_CALL, dict(n=100, M=65, x_bytes=2 ** 30, profile_bytes=2 ** 30), _INV),       # M > 64
    (_CALL, dict(modules=None), _INV),
    (_CALL, dict(modules=_A2), _INV),
    # ---- the profile and its flags
    (_CALL, dict(profile_bytes=3359), _INV),
    (_CALL, dict(profile_bytes=-1), _INV),
    (_CALL, dict(profile=_A2), _INV),
    (_CALL, dict(flags=4), _INV),
    (_CALL, dict(flags=-1), _INV),
    (_CALL, dict(flags=7), _INV),
    (_CALL, dict(_NOTHING, profile=None, profile_bytes=0), _INV),     # neither measures nor a profile
    (_CALL, dict(_NOTHING, profile_bytes=3359), _INV),
    # ---- the other buffers
    (_CALL, dict(x_bytes=3359), _INV),
    (_CALL, dict(x_bytes=-1), _INV),
    (_CALL, dict(x=None), _INV),
    (_CALL, dict(x=_A2), _INV),
    (_CALL, dict(matrices=None), _INV),
    (_CALL, dict(matrices=_A2), _INV),
    (_CALL, dict(thr=None), _INV),
    (_CALL, dict(thr=_A2), _INV),
    (_CALL, dict(workspace=_M4), _INV),
    (_CALL, dict(workspace_bytes=-1), _INV),
    (_CALL, dict(ldx=2 ** 31 - 1), _INV),                             # S * n * ldx * 4 would wrap 64 bits
    (_CALL, dict(ldx=2 ** 30), _INV),
    # ---- S == 0: CGNN_OK before any buffer is looked at; the request, M and the flags come before it
    (_CALL, dict(S=0), _OK),
    (_CALL, dict(_EMPTY), _OK),
    (_CALL, dict(_EMPTY, n=1024, M=64), _OK),
    (_CALL, dict(_EMPTY, n=1025, M=64), _INV),
    (_CALL, dict(_EMPTY, **_NOTHING, profile=_A), _OK),               # the profile alone
    (_CALL, dict(_EMPTY, **_NOTHING), _INV),                          # neither
    (_CALL, dict(_EMPTY, M=0), _INV),
    (_CALL, dict(_EMPTY, M=65, n=100), _INV),
    (_CALL, dict(_EMPTY, flags=8), _INV),
    (_CALL, dict(_EMPTY, cols=None), _INV),
    (_CALL, dict(_EMPTY, workspace=_M4), _INV),
    (_CALL, dict(_EMPTY, workspace_bytes=-1), _INV),
    (_CALL, dict(_EMPTY, x_bytes=-1), _INV),
    (_CALL, dict(_EMPTY, profile_bytes=-1), _INV),
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
