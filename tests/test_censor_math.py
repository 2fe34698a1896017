"""Frame censoring (``sample_mask=`` of connectome_gnn_amd.ingest) without a GPU: the host statement by
compaction (tests/censor_data.py) on the properties that define it and against numpy's least squares on the kept rows,
every refusal of a malformed mask on CPU tensors, the new functions of the C ABI, and the constants the device tests
build their tolerances on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import censor_data as C
from tests import confound_data as D
from tests import filter_data as F
from tests import shrinkage_data as W
from tests import timeseries_data as TS

_OK, _INV = _lib.CGNN_OK, _lib.CGNN_EINVAL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST32_RATIO = 23.42                              # measured here; tests/test_gpu_censor.py takes 4 x this
LW32_RATIO = 0.5711                               # the same for the Ledoit-Wolf estimate of the connectivity cases


# ---- the masks --------------------------------------------------------------------------------------------------------
def test_the_masks_are_what_their_names_say():
    m = C.masks(C.S, 67)
    kept = {k: m[s] for s, k in enumerate(C.KINDS)}
    assert bool(kept["all"].all()) and not bool(kept["none"].any())
    assert (~kept["ends"]).nonzero().flatten().tolist() == [0, 66]
    assert not bool(kept["random"][66]) and 30 <= int(kept["random"].sum()) <= 60
    assert (~kept["phase"]).nonzero().flatten().tolist() == list(range(1, 67, 4))
    assert (~kept["head32"]).nonzero().flatten().tolist() == list(range(32))
    assert (~kept["block8"]).nonzero().flatten().tolist() == list(range(2, 31, 4))
    assert [int(kept[k].sum()) for k in ("few", "two", "one")] == [20, 2, 1]
    assert (~C.masks(C.S, 9)[4]).nonzero().flatten().tolist() == list(range(8)), "head32 of a short run leaves one frame"
    assert m.dtype == torch.bool and m.is_contiguous() and C.S == 10


def test_the_cases_drop_the_cosines_they_are_there_for():
    counts = [len(C.dropped_components(T, t_r, hp)) + q for T, n, q, t_r, hp in C.REGRESSION_CASES]
    assert counts == [6, 25, 37, 33, 33, 64]
    assert all(c <= ingest.CONFOUND_MAX for c in counts)
    for T, n, q, t_r, hp in C.REGRESSION_CASES[:5]:
        k_lo, k_hi = ingest.filter_components(T, t_r, hp, None)
        assert C.dropped_components(T, t_r, hp) == list(range(1, k_lo)) and k_hi == T - 1


# ---- the statement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.REGRESSION_CASES)
def test_no_case_sits_on_the_rank_tolerance(case):
    """Every kept pivot is at least 9.4e-5 and every dropped one at most 5.1e-24 (measured): the rule can decide only one
    way, the rank-saturated subjects (few, two, 33 x random, 67 x head32) included."""
    for x, d, keep, kind in C.regression_subjects(case):
        _, kept, piv = C.host_basis(d, keep)
        tk = int(keep.sum())
        assert sum(kept) <= max(tk - 1, 0), (kind, "at most Tk - 1 centred columns are independent")
        assert all(p > 9.4e-5 for k, p in zip(kept, piv) if k), (kind, [p for k, p in zip(kept, piv) if k])
        assert all(p < 1e-20 for k, p in zip(kept, piv) if not k and p == p), (kind, piv)


def test_the_saturated_subjects_are_saturated():
    ranks = {}
    for case in C.REGRESSION_CASES:
        for x, d, keep, kind in C.regression_subjects(case):
            ranks[(case[0], case[1], kind)] = (int(keep.sum()), sum(C.host_basis(d, keep)[1]))
    assert ranks[(33, 65, "random")] == (16, 15) and ranks[(67, 97, "head32")] == (35, 34)
    assert all(ranks[(T, n, "few")] == (20, 19) for T, n, *_ in C.REGRESSION_CASES[1:])
    assert all(ranks[(T, n, "two")] == (2, 1) and ranks[(T, n, "one")] == (1, 0) and ranks[(T, n, "none")] == (0, 0)
               for T, n, *_ in C.REGRESSION_CASES)


@pytest.mark.parametrize("case", C.REGRESSION_CASES)
def test_the_statement_equals_least_squares_on_the_kept_rows(case):
    """The residual of x[K] on [1 | design[K]], by numpy; exact zeros at the censored frames."""
    for x, d, keep, kind in C.regression_subjects(case):
        got = C.host_regress(x, d, keep)
        assert bool((got[~keep] == 0.0).all()), kind
        if not bool(keep.any()):
            continue
        xk, dk = x[keep].double().numpy(), d[keep].double().numpy()
        A = np.concatenate([np.ones((len(xk), 1)), dk], 1)
        A = A / np.sqrt((A * A).sum(0))
        want = torch.from_numpy(xk - A @ np.linalg.lstsq(A, xk, rcond=None)[0])
        scale = float(C.host_centred(x, keep).abs().max())
        assert float((got[keep] - want).abs().max()) <= 1e-10 * max(scale, 1.0), kind


def test_an_all_true_mask_reproduces_the_unmasked_statements():
    T, n, q, t_r, hp = C.REGRESSION_CASES[1]
    x, c = D.frames(C.S, T, n, q)[0], D.confounds(C.S, T, q)[0]
    keep = torch.ones(T, dtype=torch.bool)
    assert torch.equal(C.host_regress(x, c, keep), D.host_regress(x, c))
    assert torch.equal(C.host_regress32(x, c, keep), D.host_regress32(x, c))
    assert torch.equal(C.host_basis(c, keep)[0], D.host_basis(c)[0]) and C.host_basis(c, keep)[1] == D.host_basis(c)[1]
    assert torch.equal(C.host_centred(x, keep), F.centred(x)) and torch.equal(C.host_regress(x, None, keep), F.centred(x))
    ts = TS.planted(2, 33, 65)
    every = torch.ones(2, 33, dtype=torch.bool)
    for window, stride in ((None, None), (8, 4)):
        us = C.units(ts, every, window, stride)
        assert torch.equal(torch.stack([C.host_unit(u) for u in us]), TS.host_corr(ts, window, stride))
        assert [C.host_lw(u) for u in us] == W.host_cohort(ts, window, stride).tolist()


def test_censored_values_play_no_part_in_the_statement():
    T, n, q, t_r, hp = C.REGRESSION_CASES[2]
    for x, d, keep, kind in C.regression_subjects(C.REGRESSION_CASES[2])[1:6]:
        bad_x, bad_d = x.clone(), d.clone()
        bad_x[~keep] = float("nan")
        bad_d[~keep] = 1e30
        assert torch.equal(C.host_regress(bad_x, bad_d, keep), C.host_regress(x, d, keep)), kind


def test_units_with_fewer_than_two_kept_frames_are_empty():
    T, n, window, stride = C.CONNECTIVITY_CASES[1]
    us = C.connectivity_units(C.CONNECTIVITY_CASES[1])
    W_ = TS.num_windows(T, window, stride)
    assert len(us) == C.S * W_
    head = us[4 * W_:5 * W_]                      # head32 of 33 frames keeps frame 32 alone, which no window reaches
    assert [u.shape[0] for u in head] == [0] * W_
    for u in head + us[8 * W_:]:                  # and the kinds one and none
        assert u.shape[0] < 2 and not bool(C.host_unit(u).any()) and C.host_lw(u) == 0.0 and C.cond(u) == 0.0
    two = us[7 * W_:8 * W_]
    assert sorted(u.shape[0] for u in two)[-1] <= 2 and all(C.host_lw(u) == 0.0 for u in two), "L_u <= 2 gives exactly 0"


def test_the_spike_example_is_what_the_device_test_needs():
    """Regression cannot replace censoring: the artefact lives in 20 frames, and only dropping them removes it."""
    x, c = D.spike_pair()
    for s in range(x.shape[0]):
        keep = c[s, :, 0] == 0
        assert int(keep.sum()) == 280
        assert F.corr01(x[s]) > 0.9 and abs(F.corr01(x[s][keep])) < 0.2
        r = C.host_unit(x[s][keep])
        assert abs(float(r[0, 1]) - F.corr01(x[s][keep])) < 1e-12


# ---- what the device tests build their tolerances on ---------------------------------------------------------------------
def test_the_fp32_statement_is_at_the_quoted_ratio():
    """4 x this ratio is the device tolerance of the outputs: measured on the host alone, never against the kernel."""
    worst, at = C.worst_host32_ratio()
    print(f"worst max_t |host_regress32 - host_regress| / (2^-24 max_K |xc|) = {worst:.4f} at {at}")
    assert round(worst, 2) == HOST32_RATIO and at == ((300, 72, 64, None, None), "block8")
    assert 4 * HOST32_RATIO * C.EPS < 1e-5


def test_the_fp32_estimate_is_at_the_quoted_ratio():
    worst = C.worst_lw32_ratio()
    print(f"worst |host_lw32 - host_lw| / (2^-24 cond) over the censored units = {worst:.4f}")
    assert round(worst, 4) == LW32_RATIO


# ---- refusals: on CPU tensors, before the residency check ------------------------------------------------------------------
def _ts(T=30, n=20):
    return F.frames(3, T, n)


def _cf(T=30, q=6):
    return D.confounds(3, T, q)


def _mask(S=3, T=30):
    return torch.ones(S, T, dtype=torch.bool)


def _calls():
    y = torch.zeros(3, dtype=torch.long)
    return (("confound_basis", lambda m: ingest.confound_basis(_cf(), sample_mask=m)),
            ("regress_confounds", lambda m: ingest.regress_confounds(_ts(), _cf(), sample_mask=m)),
            ("filter_timeseries", lambda m: ingest.filter_timeseries(_ts(), t_r=1.0, high_pass=0.05, sample_mask=m)),
            ("filter_timeseries", lambda m: ingest.filter_timeseries(_ts(), t_r=1.0, confounds=_cf(), sample_mask=m)),
            ("correlation_matrices", lambda m: ingest.correlation_matrices(_ts(), sample_mask=m)),
            ("correlation_matrices", lambda m: ingest.correlation_matrices(_ts(), window=10, stride=5, kind="partial",
                                                                           shrinkage="ledoit_wolf", sample_mask=m)),
            ("ledoit_wolf_shrinkage", lambda m: ingest.ledoit_wolf_shrinkage(_ts(), sample_mask=m)),
            ("from_timeseries", lambda m: ingest.from_timeseries(_ts(), y, keep=0.2, sample_mask=m)))


def test_valid_requests_reach_the_residency_check():
    for name, call in _calls():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(_mask())


def test_a_malformed_mask_is_refused_by_every_entry_point():
    for name, call in _calls():
        for bad, exc, msg in ((_mask().numpy(), TypeError, "sample_mask must be a torch.Tensor or None"),
                              (_mask().to(torch.uint8), TypeError, "sample_mask must be bool"),
                              (_mask().float(), TypeError, "sample_mask must be bool"),
                              (_mask(3, 29), ValueError, r"sample_mask must be \[S, T\] = \[3, 30\]"),
                              (_mask(2, 30), ValueError, r"sample_mask must be \[S, T\] = \[3, 30\]"),
                              (_mask()[0], ValueError, r"sample_mask must be \[S, T\]"),
                              (_mask(30, 3).t(), ValueError, "sample_mask must be contiguous"),
                              (_mask().to("meta"), ValueError, "sample_mask is on meta")):
            with pytest.raises(exc, match=msg):
                call(bad)


def test_sample_mask_is_by_keyword():
    with pytest.raises(TypeError):
        ingest.confound_basis(_cf(), _mask())
    with pytest.raises(TypeError):
        ingest.regress_confounds(_ts(), _cf(), _mask())


def test_a_band_that_needs_too_many_regressors_is_refused():
    ts = F.frames(3, 300, 20)
    m = _mask(3, 300)
    with pytest.raises(ValueError, match=r"drops 269 components, and with 0 confound columns.*CONFOUND_MAX = 64.*"
                                         "interpolated, which is not built"):
        ingest.filter_timeseries(ts, t_r=1.0, low_pass=0.05, sample_mask=m)
    with pytest.raises(ValueError, match="drops 60 components, and with 6 confound columns"):
        ingest.filter_timeseries(ts, t_r=1.0, high_pass=0.1, confounds=D.confounds(3, 300, 6), sample_mask=m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # 58 + 6 fit, and so does a low_pass that fits
        ingest.filter_timeseries(ts, t_r=1.0, high_pass=0.098, confounds=D.confounds(3, 300, 6), sample_mask=m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.filter_timeseries(ts, t_r=1.0, low_pass=0.4, sample_mask=m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # masked centring
        ingest.filter_timeseries(ts, t_r=1.0, sample_mask=m)
    with pytest.raises(ValueError, match="holds no component"):        # the band's own refusals come first
        ingest.filter_timeseries(ts, t_r=1.0, high_pass=0.2, low_pass=0.2001, sample_mask=m)


# ---- the binding and the C ABI: refusals return before any launch, so they need no device -------------------------------
_NEW = (("cgnn_ingest_confound_basis_masked", 11), ("cgnn_ingest_regress_masked", 14), ("cgnn_ingest_corr_masked", 14),
        ("cgnn_ingest_shrinkage_masked", 15), ("cgnn_ingest_design_bytes", 4), ("cgnn_ingest_design", 9))


def test_header_exports_and_prototypes_agree_for_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name, args in _NEW:
        decl = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert decl, f"{name} is not declared in cgnn.h"
        assert len(decl.group(2).split(",")) == args
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib.PROTOTYPES[name]
        assert len(argtypes) == args
        assert restype is (ctypes.c_int64 if decl.group(1) == "int64_t" else ctypes.c_int)
    assert _lib.ABI_VERSION == 2 and lib.cgnn_abi_version() == 2, "the change is additive"


_A, _A2, _A8 = 0x1000, 0x1002, 0x1008             # 16-byte aligned; not 4-byte aligned; not 16-byte aligned


def _wrong(fn, base, cases, want):
    out = []
    for change in cases:
        args = dict(base)
        args.update(change)
        if fn(*args.values()) != want:
            out.append(change)
    return out


def test_the_design_byte_count():
    q = _lib.load().cgnn_ingest_design_bytes
    assert q(6, 30, 9, 24) == 6 * 30 * 33 * 4 and q(6, 30, 0, 1) == q(6, 30, 1, 0) == 6 * 30 * 4
    assert q(0, 30, 9, 24) == 0 and q(4096, 1200, 17, 24) == 4096 * 1200 * 41 * 4 and q(6, 30, 40, 24) == 6 * 30 * 64 * 4
    for bad in ((6, 30, 0, 0), (6, 30, 41, 24), (6, 30, -1, 24), (6, 30, 9, -1), (6, 1, 9, 24), (-1, 30, 9, 24),
                (6, 2 ** 30 + 1, 9, 24), (2 ** 31, 30, 9, 24)):
        assert q(*bad) < 0, bad


def test_the_masked_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    basis = dict(confounds=_A, S=6, T=30, q=24, keep=_A2, keep_bytes=180, basis=_A, basis_bytes=6 * 30 * 32 * 4, rank=_A,
                 rank_bytes=24, stream=None)
    bad = [dict(keep=None), dict(keep_bytes=179), dict(keep_bytes=-1), dict(basis_bytes=6 * 30 * 32 * 4 - 1),
           dict(rank_bytes=23), dict(q=33), dict(confounds=None), dict(basis=None), dict(rank=None), dict(confounds=_A2),
           dict(rank=_A2), dict(basis=_A8), dict(q=0), dict(q=65), dict(T=1), dict(T=2 ** 30 + 1), dict(S=-1),
           dict(S=2 ** 31), dict(S=0, q=65), dict(S=0, keep_bytes=-1)]
    assert not _wrong(lib.cgnn_ingest_confound_basis_masked, basis, bad, _INV)
    ok = [dict(S=0), dict(S=0, confounds=None, keep=None, basis=None, rank=None, keep_bytes=0, basis_bytes=0, rank_bytes=0)]
    assert not _wrong(lib.cgnn_ingest_confound_basis_masked, basis, ok, _OK)

    regress = dict(ts=_A, S=6, T=30, n=20, keep=_A2, keep_bytes=180, basis=_A, basis_bytes=6 * 30 * 32 * 4, qpad=32,
                   workspace=_A, workspace_bytes=6 * 20 * 8, out=_A, out_bytes=6 * 30 * 20 * 4, stream=None)
    bad = [dict(keep=None), dict(keep_bytes=179), dict(keep_bytes=-1), dict(basis_bytes=6 * 30 * 32 * 4 - 1),
           dict(workspace_bytes=6 * 20 * 8 - 1), dict(out_bytes=6 * 30 * 20 * 4 - 1), dict(basis_bytes=-1),
           dict(workspace_bytes=-1), dict(out_bytes=-1), dict(qpad=64), dict(qpad=48), dict(qpad=96), dict(qpad=-32),
           dict(qpad=0), dict(basis=None), dict(ts=None), dict(workspace=None), dict(out=None), dict(ts=_A2), dict(out=_A2),
           dict(basis=_A8), dict(workspace=_A8), dict(T=1), dict(T=2 ** 30 + 1), dict(S=-1), dict(n=0),
           dict(S=2 ** 31 // 20 + 1), dict(S=0, qpad=48), dict(S=0, T=1), dict(S=0, keep_bytes=-1)]
    assert not _wrong(lib.cgnn_ingest_regress_masked, regress, bad, _INV), "qpad == 0 goes with a NULL basis, and only it"
    ok = [dict(S=0), dict(S=0, qpad=0), dict(S=0, ts=None, keep=None, basis=None, workspace=None, out=None, keep_bytes=0,
                                             basis_bytes=0, workspace_bytes=0, out_bytes=0)]
    assert not _wrong(lib.cgnn_ingest_regress_masked, regress, ok, _OK)

    corr = dict(ts=_A, S=6, T=30, n=20, window=10, stride=5, absolute=0, keep=_A2, keep_bytes=180, stats=_A,
                stats_bytes=30 * 20 * 8, out=_A, out_bytes=30 * 400 * 4, stream=None)
    bad = [dict(keep=None), dict(keep_bytes=179), dict(keep_bytes=-1), dict(stats_bytes=30 * 20 * 8 - 1),
           dict(out_bytes=30 * 400 * 4 - 1), dict(ts=None), dict(stats=None), dict(out=None), dict(ts=_A2), dict(stats=_A2),
           dict(out=_A2), dict(T=1), dict(window=1), dict(window=31), dict(stride=0), dict(S=-1), dict(n=0),
           dict(S=0, window=31), dict(S=0, keep_bytes=-1)]
    assert not _wrong(lib.cgnn_ingest_corr_masked, corr, bad, _INV)
    ok = [dict(S=0), dict(S=0, ts=None, keep=None, stats=None, out=None, keep_bytes=0, stats_bytes=0, out_bytes=0)]
    assert not _wrong(lib.cgnn_ingest_corr_masked, corr, ok, _OK)

    lw = dict(ts=_A, S=6, T=30, n=20, window=10, stride=5, keep=_A2, keep_bytes=180, stats=_A, stats_bytes=30 * 20 * 8,
              matrices=_A, matrices_bytes=30 * 400 * 4, alpha=_A, alpha_bytes=30 * 8, stream=None)
    bad = [dict(keep=None), dict(keep_bytes=179), dict(keep_bytes=-1), dict(stats_bytes=30 * 20 * 8 - 1),
           dict(matrices_bytes=30 * 400 * 4 - 1), dict(alpha_bytes=30 * 8 - 1), dict(stats_bytes=-1), dict(matrices_bytes=-1),
           dict(alpha_bytes=-1), dict(ts=None), dict(stats=None), dict(matrices=None), dict(alpha=None), dict(ts=_A2),
           dict(stats=_A2), dict(matrices=_A2), dict(alpha=0x1004), dict(T=1), dict(window=1), dict(window=31),
           dict(stride=0), dict(S=-1), dict(n=0), dict(n=1025), dict(S=0, n=1025), dict(S=0, alpha_bytes=-1)]
    assert not _wrong(lib.cgnn_ingest_shrinkage_masked, lw, bad, _INV)
    ok = [dict(S=0), dict(S=0, ts=None, keep=None, stats=None, matrices=None, alpha=None, keep_bytes=0, stats_bytes=0,
                          matrices_bytes=0, alpha_bytes=0)]
    assert not _wrong(lib.cgnn_ingest_shrinkage_masked, lw, ok, _OK)


def test_the_design_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    comps = (ctypes.c_int32 * 3)(1, 2, 5)
    design = dict(confounds=_A, S=6, T=30, q=24, comps=comps, K=3, design=_A, design_bytes=6 * 30 * 27 * 4, stream=None)
    bad = [dict(design_bytes=6 * 30 * 27 * 4 - 1), dict(design_bytes=-1), dict(design=None), dict(design=_A2),
           dict(confounds=None), dict(confounds=_A2), dict(comps=None), dict(q=0), dict(q=62), dict(q=-1), dict(K=-1),
           dict(K=0, q=0, confounds=None), dict(comps=(ctypes.c_int32 * 3)(1, 2, 30)), dict(comps=(ctypes.c_int32 * 3)(0, 2, 5)),
           dict(comps=(ctypes.c_int32 * 3)(1, 5, 5)), dict(comps=(ctypes.c_int32 * 3)(2, 1, 5)), dict(T=1),
           dict(T=2 ** 30 + 1), dict(S=-1), dict(S=2 ** 31), dict(S=0, q=62), dict(S=0, confounds=None),
           dict(S=0, design_bytes=-1)]
    assert not _wrong(lib.cgnn_ingest_design, design, bad, _INV), "confounds is NULL iff q == 0"
    ok = [dict(S=0), dict(S=0, design=None, design_bytes=0), dict(S=0, q=0, confounds=None),
          dict(S=0, K=0, comps=None)]
    assert not _wrong(lib.cgnn_ingest_design, design, ok, _OK)
