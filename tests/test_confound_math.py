"""connectome_gnn_amd.ingest.confound_basis / regress_confounds / filter_timeseries(confounds=) without a GPU: the host
statement (tests/confound_data.py) on the properties that define it and against numpy's least squares, every refusal of
the new calls on CPU tensors, the new functions of the C ABI, and the constant the device tests build their tolerance
on."""
import ctypes

import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import confound_data as D
from tests import filter_data as F

_OK, _INV = _lib.CGNN_OK, _lib.CGNN_EINVAL
HOST32_RATIO = 11.09                              # measured here; tests/test_gpu_confounds.py takes 4 x this


def _subjects(case):
    T, n, S, q, near = case
    return zip(D.frames(S, T, n, q, 0, near), D.confounds(S, T, q, 0, near))


# ---- the statement ----------------------------------------------------------------------------------------------
def test_the_constants_are_the_modules():
    assert D.RANK_TOL == ingest.CONFOUND_RANK_TOL == 1e-10 and D.MAX_CONFOUNDS == ingest.CONFOUND_MAX == 64


@pytest.mark.parametrize("case", D.all_cases())
def test_no_case_sits_on_the_rank_tolerance(case):
    for _, c in _subjects(case):
        _, kept, piv = D.host_basis(c)
        assert all(d > 1e-4 for k, d in zip(kept, piv) if k), [d for k, d in zip(kept, piv) if k]
        assert all(d < 1e-12 for k, d in zip(kept, piv) if not k and d == d), piv


def test_the_cases_have_the_ranks_they_are_there_for():
    ranks = [[D.host_rank(c) for c in D.confounds(S, T, q, 0, near)] for T, n, S, q, near in D.all_cases()]
    assert ranks == [[1, 1], [3, 3], [1, 1, 1], [21, 21], [30, 30], [29, 29], [61, 61], [6, 6]]
    c = D.confounds(2, 130, 8, 0, True)[0]
    _, kept, piv = D.host_basis(c)
    assert kept == [True, True, False, True, True, True, True, False]       # the constant and the near-copy
    assert 1e-18 < piv[7] < 1e-12, "rounding leaves the near-copy independent, far below the tolerance"


@pytest.mark.parametrize("case", D.all_cases())
def test_the_host_basis_is_orthonormal(case):
    for _, c in _subjects(case):
        Q, kept, _ = D.host_basis(c)
        K = [j for j, k in enumerate(kept) if k]
        assert float((Q[:, K].t() @ Q[:, K] - torch.eye(len(K), dtype=torch.float64)).abs().max()) <= 1e-13
        assert float(Q.sum(0).abs().max()) <= 1e-13 * Q.shape[0]             # orthogonal to the constant
        dropped = [j for j, k in enumerate(kept) if not k]
        assert bool((Q[:, dropped] == 0.0).all())
        u = F.centred(c)[:, K]
        assert all(float(Q[:, j] @ u[:, i]) > 0.0 for i, j in enumerate(K)), "a positive coefficient on u_j"


@pytest.mark.parametrize("case", [(*c, False) for c in D.CASES])
def test_the_statement_equals_least_squares_residuals(case):
    """On the cases whose dependent columns are exact; the near-copy is left to the statement alone."""
    for x, c in _subjects(case):
        xc, cc = F.centred(x).numpy(), F.centred(c).numpy()
        norm = np.sqrt((cc * cc).sum(0))
        u = cc / np.where(norm > 0.0, norm, 1.0)
        coef = np.linalg.lstsq(u, xc, rcond=None)[0]
        want = torch.from_numpy(xc - u @ coef)
        scale = float(F.centred(x).abs().max())
        assert float((D.host_regress(x, c) - want).abs().max()) <= 1e-10 * scale


@pytest.mark.parametrize("T,n,S,q,t_r,hp,lp", D.BANDS)
def test_filter_then_regress_is_the_joint_regression(T, n, S, q, t_r, hp, lp):
    """Frisch-Waugh-Lovell: the residual of x on [1 | dropped cosines | confounds], in fp64."""
    k_lo, k_hi = F.components(T, t_r, hp, lp)
    dropped = F.basis(T, [k for k in range(1, T) if not k_lo <= k <= k_hi]).numpy()
    for x, c in zip(D.frames(S, T, n, q), D.confounds(S, T, q)):
        cc = F.centred(c).numpy()
        norm = np.sqrt((cc * cc).sum(0))
        design = np.concatenate([dropped, cc / np.where(norm > 0.0, norm, 1.0)], 1)
        xc = F.centred(x).numpy()
        want = torch.from_numpy(xc - design @ np.linalg.lstsq(design, xc, rcond=None)[0])
        got = D.host_filter_regress(x, c, t_r, hp, lp)
        assert float((got - want).abs().max()) <= 1e-10 * float(F.centred(x).abs().max())


def test_non_finite_confounds_give_a_nan_basis_and_rank_minus_one():
    c = D.confounds(2, 33, 24)[0].clone()
    for bad in (float("nan"), float("inf"), float("-inf")):
        c[17, 5] = bad
        Q, kept, _ = D.host_basis(c)
        assert kept is None and D.host_rank(c) == -1 and bool(torch.isnan(Q).all())
        assert bool(torch.isnan(D.host_regress(D.frames(2, 33, 65, 24)[0], c)).all())


def test_the_spike_example_is_what_the_device_test_needs():
    x, c = D.spike_pair()
    for s in range(x.shape[0]):
        assert F.corr01(x[s]) > 0.95
        assert abs(F.corr01(D.host_regress(x[s], c[s]))) < 0.2


# ---- refusals: on CPU tensors, before the residency check -------------------------------------------------------------
def _ts(T=30, n=20):
    return F.frames(3, T, n)


def _cf(T=30, q=6):
    return D.confounds(3, T, q)


def test_valid_requests_reach_the_residency_check():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.confound_basis(_cf())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.confound_basis(D.confounds(3, 30, 64))
    for kw in (dict(), dict(out=torch.empty(3, 30, 20))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ingest.regress_confounds(_ts(), _cf(), **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ingest.filter_timeseries(_ts(), t_r=1.0, high_pass=0.05, confounds=_cf(), **kw)


def _calls():
    return (("confound_basis", lambda c: ingest.confound_basis(c)),
            ("regress_confounds", lambda c: ingest.regress_confounds(_ts(), c)),
            ("filter_timeseries", lambda c: ingest.filter_timeseries(_ts(), t_r=1.0, high_pass=0.05, confounds=c)))


def test_malformed_confounds_are_refused():
    wide = torch.zeros(1).expand(3, 30, 65)
    for name, call in _calls():
        for bad, exc, msg in ((_cf().numpy(), TypeError, "confounds must be a torch.Tensor"),
                              (_cf().double(), TypeError, "confounds must be float32"),
                              (_cf()[0], ValueError, r"confounds must be \[S, T, q\]"),
                              (_cf()[:, :, :0], ValueError, "q = 0 columns: 1 <= q <= CONFOUND_MAX = 64"),
                              (wide, ValueError, "q = 65 columns: 1 <= q <= CONFOUND_MAX = 64"),
                              (_cf().transpose(0, 1).contiguous().transpose(0, 1), ValueError,
                               "confounds must be contiguous"),
                              (_cf().to("meta"), ValueError if name != "confound_basis" else RuntimeError,
                               "confounds are on meta")):
            with pytest.raises(exc, match=msg):
                call(bad)


def test_confounds_must_go_with_the_time_series():
    for name, call in _calls()[1:]:
        for bad in (D.confounds(2, 30, 6), D.confounds(3, 29, 6), D.confounds(3, 31, 6)):
            with pytest.raises(ValueError, match=r"confounds must be \[S, T, q\] = \[3, 30, q\]"):
                call(bad)
    with pytest.raises(ValueError, match="T >= 2"):
        ingest.confound_basis(_cf()[:, :1].contiguous())


def test_malformed_time_series_and_out_are_refused_by_regress_confounds():
    for bad, exc, msg in ((_ts().numpy(), TypeError, "torch.Tensor"), (_ts().double(), TypeError, "float32"),
                          (_ts()[0], ValueError, r"\[S, T, n\]"), (_ts().transpose(1, 2), ValueError, r"\[3, 20, q\]")):
        with pytest.raises(exc, match=msg):
            ingest.regress_confounds(bad, _cf())
    nc = torch.empty(3, 20, 30).transpose(1, 2)
    with pytest.raises(ValueError, match="timeseries must be contiguous"):
        ingest.regress_confounds(nc, _cf())
    for bad, exc, msg in ((_ts().numpy().copy(), TypeError, "out must be a torch.Tensor"),
                          (torch.empty(3, 30, 20, dtype=torch.float64), TypeError, "out must be float32"),
                          (torch.empty(3, 30, 21), ValueError, r"out must be \(3, 30, 20\)"),
                          (torch.empty(3, 30, 20, device="meta"), ValueError, "out is on meta"),
                          (nc, ValueError, "out must be contiguous")):
        with pytest.raises(exc, match=msg):
            ingest.regress_confounds(_ts(), _cf(), out=bad)
    with pytest.raises(TypeError):                            # out is by keyword
        ingest.regress_confounds(_ts(), _cf(), torch.empty(3, 30, 20))


# ---- the binding and the C ABI: refusals return before any launch, so they need no device ------------------------
def test_the_binding_declares_the_symbols():
    for name, args in (("cgnn_ingest_confound_basis_bytes", 3), ("cgnn_ingest_confound_basis", 9),
                       ("cgnn_ingest_regress_workspace_bytes", 3), ("cgnn_ingest_regress", 12)):
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == args
        assert hasattr(_lib.load(), name), "exported by the built library"
    assert _lib.PROTOTYPES["cgnn_ingest_confound_basis_bytes"][0] is ctypes.c_int64
    assert _lib.PROTOTYPES["cgnn_ingest_regress_workspace_bytes"][0] is ctypes.c_int64
    assert _lib.ABI_VERSION == 2 and _lib.load().cgnn_abi_version() == 2


_A, _A2, _A8 = 0x1000, 0x1002, 0x1008             # 16-byte aligned; not 4-byte aligned; not 16-byte aligned


def test_the_byte_count_queries():
    lib = _lib.load()
    q = lib.cgnn_ingest_confound_basis_bytes
    assert q(6, 30, 1) == q(6, 30, 32) == 6 * 30 * 32 * 4 and q(6, 30, 33) == q(6, 30, 64) == 6 * 30 * 64 * 4
    assert q(0, 30, 24) == 0 and q(4096, 1200, 24) == 4096 * 1200 * 32 * 4
    for bad in ((6, 30, 0), (6, 30, 65), (6, 30, -1), (6, 1, 24), (-1, 30, 24), (6, 2 ** 30 + 1, 24), (2 ** 31, 30, 24)):
        assert q(*bad) < 0, bad
    w = lib.cgnn_ingest_regress_workspace_bytes
    assert w(6, 30, 20) == 6 * 20 * 8 and w(0, 30, 20) == 0 and w(4096, 1200, 360) == 4096 * 360 * 8
    for bad in ((6, 1, 20), (-1, 30, 20), (6, 30, 0), (2 ** 31 // 20 + 1, 30, 20), (6, 2 ** 30 + 1, 20)):
        assert w(*bad) < 0, bad


def _basis(lib, **change):
    args = dict(confounds=_A, S=6, T=30, q=24, basis=_A, basis_bytes=6 * 30 * 32 * 4, rank=_A, rank_bytes=24, stream=None)
    args.update(change)
    return lib.cgnn_ingest_confound_basis(*args.values())


def _regress(lib, **change):
    args = dict(ts=_A, S=6, T=30, n=20, basis=_A, basis_bytes=6 * 30 * 32 * 4, qpad=32, workspace=_A,
                workspace_bytes=6 * 20 * 8, out=_A, out_bytes=6 * 30 * 20 * 4, stream=None)
    args.update(change)
    return lib.cgnn_ingest_regress(*args.values())


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    bad = [dict(basis_bytes=6 * 30 * 32 * 4 - 1), dict(rank_bytes=23), dict(basis_bytes=-1), dict(rank_bytes=-1),
           dict(q=33), dict(confounds=None), dict(basis=None), dict(rank=None), dict(confounds=_A2), dict(rank=_A2),
           dict(basis=_A8), dict(q=0), dict(q=65), dict(q=-3), dict(T=1), dict(T=2 ** 30 + 1), dict(S=-1),
           dict(S=2 ** 31), dict(S=0, q=65), dict(S=0, T=1), dict(S=0, rank_bytes=-1)]
    wrong = [c for c in bad if _basis(lib, **c) != _INV]
    assert not wrong, wrong
    ok = [dict(S=0), dict(S=0, confounds=None, basis=None, rank=None, basis_bytes=0, rank_bytes=0)]
    wrong = [c for c in ok if _basis(lib, **c) != _OK]
    assert not wrong, wrong
    bad = [dict(basis_bytes=6 * 30 * 32 * 4 - 1), dict(workspace_bytes=6 * 20 * 8 - 1), dict(out_bytes=6 * 30 * 20 * 4 - 1),
           dict(basis_bytes=-1), dict(workspace_bytes=-1), dict(out_bytes=-1), dict(qpad=64), dict(qpad=48), dict(qpad=0),
           dict(qpad=96), dict(qpad=-32), dict(ts=None), dict(basis=None), dict(workspace=None), dict(out=None),
           dict(ts=_A2), dict(out=_A2), dict(basis=_A8), dict(workspace=_A8), dict(T=1), dict(T=2 ** 30 + 1), dict(S=-1),
           dict(n=0), dict(n=-2), dict(S=2 ** 31 // 20 + 1), dict(S=0, qpad=48), dict(S=0, T=1), dict(S=0, out_bytes=-1)]
    wrong = [c for c in bad if _regress(lib, **c) != _INV]
    assert not wrong, wrong
    ok = [dict(S=0), dict(S=0, ts=None, basis=None, workspace=None, out=None, basis_bytes=0, workspace_bytes=0,
                          out_bytes=0), dict(S=0, qpad=64)]
    wrong = [c for c in ok if _regress(lib, **c) != _OK]
    assert not wrong, wrong


# ---- what the device tests build their tolerance on ---------------------------------------------------------------------
def test_the_fp32_statement_is_at_the_quoted_ratio():
    """4 x this ratio is the device tolerance: measured on the host alone, never against the kernel."""
    worst = D.worst_host32_ratio()
    print(f"worst max_t |host_regress32 - host_regress| / (2^-24 max_t |xc|) = {worst:.4f}")
    assert round(worst, 2) == HOST32_RATIO
    assert 4 * HOST32_RATIO * D.EPS < 1e-5


def test_a_lost_confound_is_far_outside_the_tolerance():
    """Leaving confound 0 in (every ROI carries 3 x it) moves a column by far more than the tolerance."""
    for case in D.all_cases()[3:]:
        for x, c in _subjects(case):
            Q = D.host_basis(c)[0]
            xc = F.centred(x)
            lost = (Q[:, :1] @ (Q[:, :1].t() @ xc)).abs().max(0).values
            assert bool((lost >= 1e-3 * xc.abs().max(0).values).all())
