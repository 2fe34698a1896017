"""connectome_gnn_amd.ingest.filter_timeseries / filter_components without a GPU: the host statement
(tests/filter_data.py) against scipy's DCT and on the properties that define it, the index rule on examples worked by
hand, every refusal of the new call on CPU tensors, the two new functions of the C ABI, and the constant the device
tests build their tolerance on."""
import ctypes
import math

import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import filter_data as D

_OK, _INV = _lib.CGNN_OK, _lib.CGNN_EINVAL
HOST32_RATIO = 15.95                              # quoted by tests/test_gpu_filter.py, which takes 4 x this


def _scale(x):
    return D.centred(x).abs().max()


# ---- the statement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n,S,t_r,hp,lp", D.CASES + D.WIDE_CASES)
def test_statement_equals_scipy_dct(T, n, S, t_r, hp, lp):
    fft = pytest.importorskip("scipy.fft")
    k_lo, k_hi = D.components(T, t_r, hp, lp)
    mask = np.zeros((T, 1))
    mask[k_lo:k_hi + 1] = 1.0
    for x in D.frames(S, T, n):
        xc = D.centred(x).numpy()
        want = fft.idct(mask * fft.dct(xc, type=2, norm="ortho", axis=0), type=2, norm="ortho", axis=0)
        err = float((D.host_filter(x, t_r, hp, lp) - torch.from_numpy(want)).abs().max())
        assert err <= 1e-12 * float(_scale(x)), (T, n, err)


@pytest.mark.parametrize("T", [2, 9, 33, 600])
def test_the_basis_is_orthonormal(T):
    B = D.basis(T, range(1, T))
    assert float((B.t() @ B - torch.eye(T - 1, dtype=torch.float64)).abs().max()) <= 1e-13
    assert float(B.sum(0).abs().max()) <= 1e-13 * T          # and orthogonal to the constant: a mean stays removed


@pytest.mark.parametrize("T,n,S,t_r,hp,lp", D.CASES)
def test_keep_and_complement_agree_and_the_statement_is_idempotent(T, n, S, t_r, hp, lp):
    for x in D.frames(S, T, n):
        y, tol = D.host_filter(x, t_r, hp, lp), 1e-12 * float(_scale(x))
        assert float((y - D.host_complement(x, t_r, hp, lp)).abs().max()) <= tol
        assert float((D.host_filter(y, t_r, hp, lp) - y).abs().max()) <= tol


def test_the_cases_take_the_paths_they_are_there_for():
    forms = [(c, len(k)) for c, k in (D.form(T, *D.components(T, t_r, hp, lp)) for T, _, _, t_r, hp, lp in D.CASES)]
    assert forms == [(True, 0), (True, 1), (False, 12), (True, 24), (False, 28), (False, 17), (False, 99), (False, 256),
                     (True, 7)]
    assert D.components(50, 0.72, 0.05, 0.4) == (4, 28)      # keeps 25, drops 24: within one component
    wide = [(c, len(k)) for c, k in (D.form(T, *D.components(T, t_r, hp, lp)) for T, _, _, t_r, hp, lp in D.WIDE_CASES)]
    assert wide == [(False, 42), (False, 70), (False, 129), (True, 162), (False, 162), (False, 199)]
    assert D.MAX_COMPONENTS == ingest.FILTER_MAX_COMPONENTS == 256


# ---- filter_components ------------------------------------------------------------------------------------------------
def test_filter_components_on_examples_worked_by_hand():
    assert ingest.filter_components(1200, 0.72, 0.01, 0.1) == (18, 172)      # 17.28 -> drift order 17; 172.8 -> 172
    assert ingest.filter_components(1200, 0.72, 0.01) == (18, 1199)
    assert ingest.filter_components(1200, 0.72, None, 0.1) == (1, 172)
    assert ingest.filter_components(1200, 0.72) == (1, 1199)
    assert ingest.filter_components(300, 2.0, 0.008, 0.09) == (10, 108)      # 9.6 -> 9; 108
    assert ingest.filter_components(2, 1.0) == (1, 1)
    assert ingest.filter_components(100, 1.0, 0.0, 10.0) == (1, 99)          # a low_pass above Nyquist keeps all
    assert ingest.filter_components(100, 2.0, 0.0001, 0.0002) == (1, 0)      # a band without a component
    for T, _, _, t_r, hp, lp in D.CASES:
        assert ingest.filter_components(T, t_r, hp, lp) == D.components(T, t_r, hp, lp)
        if hp is not None:                                    # the dropped low set is the cosine drift set of that cutoff
            assert ingest.filter_components(T, t_r, hp, lp)[0] - 1 == math.floor(2 * T * t_r * hp)


def test_filter_components_refuses_bad_arguments():
    for args, exc, msg in (((1200.0, 0.72), TypeError, "T must be an int"), ((True, 0.72), TypeError, "T must be an int"),
                           ((1, 0.72), ValueError, "T >= 2"), ((10, "0.72"), TypeError, "t_r must be a float"),
                           ((10, None), TypeError, "t_r must be a float"), ((10, 0.0), ValueError, "t_r must be > 0"),
                           ((10, -1.0), ValueError, "t_r must be > 0"), ((10, math.inf), ValueError, "t_r must be finite"),
                           ((10, math.nan), ValueError, "t_r must be finite"),
                           ((10, 1.0, -0.1), ValueError, "high_pass must be >= 0"),
                           ((10, 1.0, math.nan), ValueError, "high_pass must be finite"),
                           ((10, 1.0, "a"), TypeError, "high_pass must be a float"),
                           ((10, 1.0, None, 0.0), ValueError, "low_pass must be > 0"),
                           ((10, 1.0, None, math.inf), ValueError, "low_pass must be finite"),
                           ((10, 1.0, None, [0.1]), TypeError, "low_pass must be a float"),
                           ((10, 1.0, 0.2, 0.2), ValueError, "below low_pass"),
                           ((10, 1.0, 0.3, 0.2), ValueError, "below low_pass")):
        with pytest.raises(exc, match=msg):
            ingest.filter_components(*args)


# ---- refusals of filter_timeseries: on CPU tensors, before the residency check ------------------------------------------
def _ts(T=30, n=20):
    return D.frames(3, T, n)


def test_a_valid_request_reaches_the_residency_check():
    for kw in (dict(t_r=1.0), dict(t_r=1.0, high_pass=0.05), dict(t_r=1.0, low_pass=0.2),
               dict(t_r=1.0, high_pass=0.05, low_pass=0.2), dict(t_r=2, high_pass=0, low_pass=1),
               dict(t_r=1.0, out=torch.empty(3, 30, 20))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ingest.filter_timeseries(_ts(), **kw)
    ts = _ts().clone()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.filter_timeseries(ts, t_r=1.0, out=ts)


def test_malformed_time_series_are_refused():
    for bad, exc, msg in ((_ts().numpy(), TypeError, "torch.Tensor"), (_ts().double(), TypeError, "float32"),
                          (_ts()[0], ValueError, r"\[S, T, n\]"), (_ts()[:, :1], ValueError, "T >= 2"),
                          (_ts()[:, :, :0], ValueError, "n >= 1"), (_ts().transpose(1, 2), ValueError, "contiguous")):
        with pytest.raises(exc, match=msg):
            ingest.filter_timeseries(bad, t_r=1.0, high_pass=0.05)
    with pytest.raises(TypeError):                            # t_r is required, and by keyword
        ingest.filter_timeseries(_ts())
    with pytest.raises(TypeError):
        ingest.filter_timeseries(_ts(), 1.0)


def test_a_malformed_band_is_refused():
    for kw, exc, msg in ((dict(t_r=0.0), ValueError, "t_r must be > 0"), (dict(t_r="1"), TypeError, "t_r must be a float"),
                         (dict(t_r=math.nan), ValueError, "finite"), (dict(t_r=1.0, high_pass=-1.0), ValueError, ">= 0"),
                         (dict(t_r=1.0, low_pass=0.0), ValueError, "low_pass must be > 0"),
                         (dict(t_r=1.0, high_pass=math.inf), ValueError, "finite"),
                         (dict(t_r=1.0, high_pass=0.2, low_pass=0.1), ValueError, "below low_pass"),
                         (dict(t_r=1.0, high_pass=torch.tensor(0.1)), TypeError, "high_pass must be a float")):
        with pytest.raises(exc, match=msg):
            ingest.filter_timeseries(_ts(), **kw)


def test_an_empty_band_is_refused():
    with pytest.raises(ValueError, match="holds no component of a 30-frame run"):
        ingest.filter_timeseries(_ts(), t_r=1.0, high_pass=0.001, low_pass=0.002)
    with pytest.raises(ValueError, match="holds no component of a 30-frame run"):
        ingest.filter_timeseries(_ts(), t_r=1.0, high_pass=0.6)          # above Nyquist: k_lo = 37 > T - 1


def test_more_components_than_the_limit_are_refused():
    ts = torch.zeros(1).expand(1, 1200, 3)                    # (never read: refused on its shape alone)
    with pytest.raises(ValueError, match="keeps 518 components and drops 681.*FILTER_MAX_COMPONENTS = 256"):
        ingest.filter_timeseries(ts, t_r=0.72, low_pass=0.3)
    with pytest.raises(ValueError, match="keeps 942 components and drops 257"):
        ingest.filter_timeseries(ts, t_r=0.72, high_pass=0.1492)
    with pytest.raises(ValueError, match="contiguous"):       # 256 dropped is accepted: on to the next check
        ingest.filter_timeseries(ts, t_r=0.72, high_pass=0.1487)


def test_a_malformed_out_is_refused():
    ts = _ts()
    for bad, exc, msg in ((ts.numpy().copy(), TypeError, "out must be a torch.Tensor"),
                          (torch.empty(3, 30, 20, dtype=torch.float64), TypeError, "out must be float32"),
                          (torch.empty(3, 30, 21), ValueError, r"out must be \(3, 30, 20\)"),
                          (torch.empty(3, 600), ValueError, r"out must be \(3, 30, 20\)"),
                          (torch.empty(3, 30, 20, device="meta"), ValueError, "out is on meta"),
                          (torch.empty(3, 20, 30).transpose(1, 2), ValueError, "out must be contiguous")):
        with pytest.raises(exc, match=msg):
            ingest.filter_timeseries(ts, t_r=1.0, high_pass=0.05, out=bad)


# ---- the binding and the C ABI: refusals return before any launch, so they need no device ------------------------
def test_the_binding_declares_both_symbols():
    for name, args in (("cgnn_ingest_filter_workspace_bytes", 4), ("cgnn_ingest_filter", 12)):
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == args
        assert hasattr(_lib.load(), name), "exported by the built library"
    assert _lib.PROTOTYPES["cgnn_ingest_filter_workspace_bytes"][0] is ctypes.c_int64
    assert _lib.ABI_VERSION == 2 and _lib.load().cgnn_abi_version() == 2


_A, _A2, _A8 = 0x1000, 0x1002, 0x1008             # 16-byte aligned; not 4-byte aligned; not 16-byte aligned
_TABLE = 30 * 32 * 4                              # the basis table of 30 frames and up to 32 components
_NEED = _TABLE + 6 * 20 * 8                       # and the means of 6 subjects of 20 ROIs


def _call(lib, comps=(2, 3, 5), **change):
    arr = (ctypes.c_int32 * len(comps))(*comps) if comps is not None else None
    args = dict(ts=_A, S=6, T=30, n=20, comps=arr, K=len(comps) if comps is not None else 3, complement=0, workspace=_A,
                workspace_bytes=_NEED, out=_A, out_bytes=6 * 30 * 20 * 4, stream=None)
    args.update(change)
    return lib.cgnn_ingest_filter(*args.values())


def test_the_workspace_query():
    q = _lib.load().cgnn_ingest_filter_workspace_bytes
    assert q(6, 30, 20, 3) == q(6, 30, 20, 32) == _NEED
    assert q(6, 30, 20, 33) == 30 * 64 * 4 + 6 * 20 * 8
    assert q(6, 30, 20, 256) == 30 * 256 * 4 + 6 * 20 * 8
    assert q(6, 30, 20, 0) == 6 * 20 * 8 and q(0, 30, 20, 3) == _TABLE
    for bad in ((6, 30, 20, 257), (6, 30, 20, -1), (6, 1, 20, 3), (-1, 30, 20, 3), (6, 30, 0, 3),
                (2 ** 31 // 20 + 1, 30, 20, 3), (6, 2 ** 30 + 1, 20, 3)):
        assert q(*bad) < 0, bad
    # nothing cohort-sized: the flagship shape asks for the table and the means
    assert q(4096, 1200, 360, 155) == 1200 * 160 * 4 + 4096 * 360 * 8


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    bad = [dict(workspace_bytes=_NEED - 1), dict(out_bytes=6 * 30 * 20 * 4 - 1), dict(workspace_bytes=-1),
           dict(out_bytes=-1), dict(ts=None), dict(out=None), dict(workspace=None), dict(ts=_A2), dict(out=_A2),
           dict(workspace=_A8), dict(K=257), dict(K=-1), dict(comps=None), dict(comps=(0, 3, 5)), dict(comps=(2, 3, 30)),
           dict(comps=(2, 5, 3)), dict(comps=(2, 3, 3)), dict(comps=(-4, 3, 5)), dict(T=1), dict(T=5), dict(S=-1),
           dict(n=0), dict(n=-2), dict(S=2 ** 31 // 20 + 1), dict(comps=(), K=0, complement=0), dict(T=2 ** 30 + 1),
           dict(S=0, K=257), dict(S=0, T=1), dict(S=0, comps=(5, 3, 2)), dict(S=0, out_bytes=-1)]
    wrong = [c for c in bad if _call(lib, **c) != _INV]
    assert not wrong, wrong
    ok = [dict(S=0), dict(S=0, ts=None, out=None, workspace=None, workspace_bytes=0, out_bytes=0),
          dict(S=0, comps=(), K=0, complement=1)]
    wrong = [c for c in ok if _call(lib, **c) != _OK]
    assert not wrong, wrong


# ---- what the device tests build their tolerance on ---------------------------------------------------------------------
def test_the_fp32_statement_is_at_the_quoted_ratio():
    """4 x this ratio is the device tolerance: measured on the host alone, never against the kernel."""
    worst = D.worst_host32_ratio()
    print(f"worst max_t |host_filter32 - host_filter| / (2^-24 max_t |xc|) = {worst:.4f}")
    assert round(worst, 2) == HOST32_RATIO
    wide = D.worst_host32_ratio(tuple(D.WIDE_CASES))
    print(f"the same over WIDE_CASES = {wide:.4f}")
    assert wide <= HOST32_RATIO, "the cases beyond the list stay inside the ratio the tolerance is built on"
    assert 4 * HOST32_RATIO * D.EPS < 1e-4, "the cap a lost component must stay outside of"


def test_a_lost_component_is_far_outside_the_tolerance():
    """Dropping any one planted component that the band keeps moves its column by far more than the cap 1e-4 max |xc|,
    of which the tolerance 4 x 15.95 x 2^-24 = 3.8e-6 stays clear."""
    checked = 0
    for T, n, S, t_r, hp, lp in D.CASES:
        k_lo, k_hi = D.components(T, t_r, hp, lp)
        ks, _ = D.planted(S, T, n)
        for s in (0,):
            x = D.frames(S, T, n)[s]
            xc = D.centred(x)
            scale = xc.abs().max(0).values
            for i in range(0, n, max(1, n // 6)):
                for k in {int(k) for k in ks[s, i]} & set(range(k_lo, k_hi + 1)):
                    b = D.basis(T, [k])[:, 0]
                    lost = float((b * float(b @ xc[:, i])).abs().max())
                    assert lost >= 0.02 * float(scale[i]) > 1e-4 * float(scale[i]), (T, i, k, lost)
                    checked += 1
    assert checked >= 40


def test_the_drift_example_is_what_the_device_test_needs():
    kw = {k: D.DRIFT[k] for k in ("t_r", "high_pass", "low_pass")}
    assert ingest.filter_components(D.DRIFT["T"], **kw) == (10, 108)          # component 1 is outside the band
    for x in D.drift_pair():
        assert D.corr01(x) > 0.95
        assert abs(D.corr01(D.host_filter(x, **kw))) < 0.2
