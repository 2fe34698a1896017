"""The host side of ``connectome_gnn_amd.ingest.series_features``, without a GPU: the statement of
tests/activity_data.py against ``numpy.fft.rfft``, the band index rule, Parseval, the exact cases, every refusal, and the
constants the device tolerance is built on, which are measured here on the host alone and never against the kernel.

Measured: ``c_f`` = the largest ``|host_features32 - host_features| / scale_f`` over all cases, subjects and columns is
0.97 for ``alff``, 1.30 for ``falff``, 2.98 for ``band_std`` and 5.10 for ``band_fraction`` (``scale`` = 2^-24 max_t |xc|
for the two amplitudes, 2^-24 for the two ratios).  The device is granted 4 x that.
"""
import ctypes

import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import activity_data as A
from tests.abi_header import check_header

# what is under test: the statement of tests/activity_data.py is checked below as the reference of these two, with the
# band taken from series_band and the names and their order from ingest.SERIES_FEATURES
series_features, series_band = ingest.series_features, ingest.series_band
NAMES = ingest.SERIES_FEATURES

# c_f, rounded to two places: tests/test_gpu_activity.py takes its tolerance 4 c_f scale_f from here
HOST32_RATIO = {"alff": 0.97, "falff": 1.30, "band_std": 2.98, "band_fraction": 5.10}


def test_the_names_and_limits_are_the_headers():
    assert ingest.SERIES_FEATURES == A.NAMES
    assert ingest.SERIES_MAX_FRAMES == 4096
    T = ingest.SERIES_MAX_FRAMES
    assert T * 2 * (T // 2) * 4 <= 64 * 2 ** 20, "falff's table stays at or below 64 MB"
    check_header("cgnn_activity.h", _lib.ACTIVITY_PROTOTYPES,
                 ["cgnn_ingest_activity_workspace_bytes", "cgnn_ingest_activity"],
                 [("int32_t n, int32_t bins", "int64_t n, int32_t bins"), ("int32_t k_lo, ", "")])


@pytest.mark.parametrize("T,n,t_r,lo,hi", A.CASES)
def test_the_statement_is_the_rfft_formulation(T, n, t_r, lo, hi):
    x, host = A.frames(T, n), A.host_case(T, n, t_r, lo, hi)
    assert tuple(host.shape) == (A.S, n, len(NAMES)) and host.dtype == torch.float64 and A.NAMES == NAMES
    assert A.band_of(T, t_r, lo, hi) == series_band(T, t_r, (lo, hi))
    for s in range(A.S):
        want = A.rfft_features(x[s], t_r, (lo, hi))
        bound = 1e-12 * want.abs()
        if A.KINDS[s] == "constcol":              # rfft of an exact zero column is exactly zero too
            assert bool((want[A.const_col(n)] == 0).all())
        assert bool((A.ratios(host[s], want, bound) <= 1.0).all()), (s, float(A.ratios(host[s], want, bound).max()))


def test_the_band_index_rule_at_its_edges():
    band = ingest.series_band
    assert band(100, 1.0, (0.1, 0.2)) == (10, 20), "a frequency exactly on a bin is inside, at both ends"
    assert band(100, 1.0, (0.1001, 0.1999)) == (11, 19)
    assert band(100, 1.0, (0.0, 0.05)) == (1, 5), "bin 0, the mean, is never in the band"
    assert band(100, 1.0, (0.3, 7.0)) == (30, 50), "a hi above Nyquist stops at K"
    assert band(101, 1.0, (0.3, 7.0)) == (31, 50), "K = T // 2 for odd T"
    assert band(2, 1.0, (0.0, 0.5)) == (1, 1)
    assert band(1200, 0.72, (0.01, 0.08)) == (9, 69)
    for T, n, t_r, lo, hi in A.CASES:
        assert band(T, t_r, (lo, hi)) == A.band_of(T, t_r, lo, hi)
        k_lo, k_hi = band(T, t_r, (lo, hi))
        assert 1 <= k_lo <= k_hi <= T // 2
    k_lo, k_hi = band(*A.CASES[6][0:1], A.CASES[6][2], A.CASES[6][3:5])
    assert (k_lo, k_hi) == (90, 149) and k_lo <= A.CHUNK < A.CHUNK + 1 <= k_hi, "CASES[6] straddles the chunk boundary of the whole-spectrum launch"
    k_lo, k_hi = band(9, 1.0, (0.12, 0.2))
    assert k_lo > k_hi, "no bin between 1.08 and 1.8"
    with pytest.raises(ValueError, match="holds no bin"):
        ingest.series_features(torch.zeros(1, 9, 2), t_r=1.0, band=(0.12, 0.2))
    with pytest.raises(ValueError, match="holds no bin"):
        ingest.series_features(torch.zeros(1, 9, 2), t_r=1.0, band=(0.6, 0.7), features=("alff",))


@pytest.mark.parametrize("T,n,t_r,lo,hi", A.CASES)
def test_parseval(T, n, t_r, lo, hi):
    """band_fraction^2 q is the band's power sum_band w_k |X_k|^2 / T, and over the whole spectrum that is q itself."""
    x, host = A.frames(T, n), A.host_case(T, n, t_r, lo, hi)
    k_lo, k_hi = series_band(T, t_r, (lo, hi))
    for s in range(A.S):
        p2, _, q, _ = A.powers(x[s])
        w = np.full(T // 2, 2.0)
        if T % 2 == 0:
            w[-1] = 1.0
        power = (w[:, None] * p2)[k_lo - 1:k_hi].sum(0) / T
        got = host[s, :, NAMES.index("band_fraction")].numpy() ** 2 * q
        assert np.all(np.abs(got - power) <= 1e-12 * power), s
        whole = (w[:, None] * p2).sum(0) / T
        assert np.all(np.abs(whole - q) <= 1e-12 * q), s


@pytest.mark.parametrize("T,n,t_r,lo,hi", A.CASES)
def test_a_constant_column_is_exactly_zero(T, n, t_r, lo, hi):
    for host in (A.host_case(T, n, t_r, lo, hi), A.host32_case(T, n, t_r, lo, hi)):
        col = host[4, A.const_col(n)]
        assert bool((col == 0).all()) and not bool(torch.signbit(col).any()), "all six features are +0.0"


def test_a_nan_makes_exactly_its_column_nan():
    T, n, t_r, lo, hi = A.CASES[2]
    x = A.frames(T, n)[0]
    clean = A.host_features(x, t_r, (lo, hi))
    bad = x.clone()
    bad[T // 2, 7] = float("nan")
    got = A.host_features(bad, t_r, (lo, hi))
    assert bool(torch.isnan(got[7]).all())
    got[7] = clean[7]
    assert torch.equal(got, clean)


def test_python_refuses_before_any_device_is_touched():
    f = ingest.series_features
    x = torch.zeros(2, 40, 3)                     # a CPU tensor throughout: no check below reaches a device
    for features in (("std", "alf"), ("strength",), ("std", "std"), ("alff", "std", "alff"), ()):
        with pytest.raises(ValueError, match="SERIES_FEATURES"):
            f(x, t_r=1.0, features=features)
    for t_r in (float("nan"), float("inf"), 0.0, -0.72, None):
        with pytest.raises(ValueError, match="t_r"):
            f(x, t_r=t_r)
    for band in ((0.1, 0.1), (0.2, 0.1), (-0.01, 0.1), (0.0, float("inf")), (float("nan"), 0.1)):
        with pytest.raises(ValueError, match=r"band|lo < hi"):
            f(x, t_r=1.0, band=band)
    with pytest.raises(ValueError, match="holds no bin"):
        f(x, t_r=1.0, band=(0.51, 0.9))
    with pytest.raises(ValueError, match="SERIES_MAX_FRAMES"):
        f(torch.zeros(1, ingest.SERIES_MAX_FRAMES + 1, 1), t_r=1.0, features=("band_std",))
    with pytest.raises(ValueError, match=r"\[S, T, n\]"):
        f(torch.zeros(40, 3), t_r=1.0)
    # the resident-data checks are the ones every time-series call shares, with their exceptions
    with pytest.raises(TypeError, match="float32"):
        f(x.double(), t_r=1.0)
    with pytest.raises(RuntimeError, match="ROCm"):
        f(x, t_r=1.0)
    with pytest.raises(RuntimeError, match="ROCm"):
        f(x, features=("std", "autocorr1"))       # no t_r needed without a spectral name
    with pytest.raises(RuntimeError, match="ROCm"):
        f(torch.zeros(1, ingest.SERIES_MAX_FRAMES + 1, 1), features=("std",))      # nor a bound on T


# ---- the entry point's own refusals, which return before any launch ----------------------------------------------------
_A16, _A2 = 1 << 20, (1 << 20) + 2                # made-up addresses: no call below may reach a launch
_OK, _INV = _lib.CGNN_OK, _lib.CGNN_EINVAL


def _need(S, T, n, bins):
    return _lib.load().cgnn_ingest_activity_workspace_bytes(S, T, n, bins)


def _abi(lib, *, S=5, T=300, n=12, ids=(0, 1, 2, 3, 4, 5), F=None, k_lo=90, k_hi=150, ts=_A16, workspace=_A16,
         workspace_bytes=None, out=_A16, out_bytes=None):
    F = len(ids) if F is None and ids is not None else F
    arr = None if ids is None else (ctypes.c_int32 * max(1, len(ids)))(*ids)
    wb = _need(S, T, n, T // 2) if workspace_bytes is None else workspace_bytes
    ob = 4 * S * n * F if out_bytes is None else out_bytes
    return lib.cgnn_ingest_activity(ts, S, T, n, arr, F, k_lo, k_hi, workspace, wb, out, ob, None)


def test_the_workspace_is_the_table_and_seven_doubles_a_column():
    assert _need(5, 300, 360, 150) == 300 * 512 * 4 + 7 * 5 * 360 * 8, "300 table columns: two chunks of 256"
    assert _need(5, 300, 360, 21) == 300 * 64 * 4 + 7 * 5 * 360 * 8, "42 columns in one chunk of 64"
    assert _need(5, 300, 360, 0) == 7 * 5 * 360 * 8
    assert _need(4096, 1200, 360, 600) == 1200 * 1280 * 4 + 7 * 4096 * 360 * 8, "nothing cohort-sized"
    assert _need(1, 4096, 1, 2048) <= 64 * 2 ** 20 + 56
    assert _need(1, 4097, 1, 0) > 0 and _need(1, 4097, 1, 1) == _INV
    for bad in ((-1, 300, 12, 0), (5, 1, 12, 0), (5, 300, 0, 0), (5, 300, 12, -1), (5, 300, 12, 151),
                (2 ** 31 // 12 + 1, 300, 12, 0), (5, 2 ** 30 + 1, 12, 0)):
        assert _need(*bad) == _INV, bad


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    need, ob = _need(5, 300, 12, 150), 4 * 5 * 12 * 6
    bad = [dict(workspace_bytes=need - 1), dict(out_bytes=ob - 1), dict(workspace_bytes=-1), dict(out_bytes=-1),
           dict(ts=None), dict(out=None), dict(workspace=None), dict(ts=_A2), dict(out=_A2), dict(workspace=_A16 + 8),
           dict(k_lo=151, k_hi=150), dict(k_lo=0), dict(k_hi=151), dict(ids=(0, 1, 6)), dict(ids=(0, -1)),
           dict(ids=(2, 2)), dict(ids=None, F=1), dict(ids=(), F=0), dict(ids=(0, 1, 2, 3, 4, 5), F=7), dict(T=1),
           dict(S=-1), dict(n=0), dict(S=2 ** 31 // 12 + 1), dict(T=2 ** 30 + 1, ids=(0,)),
           dict(T=4097, ids=(2,), k_lo=1, k_hi=5), dict(ids=(0, 1), k_lo=3, k_hi=2),
           dict(S=0, ids=(7,)), dict(S=0, T=1), dict(S=0, k_lo=5, k_hi=4), dict(S=0, out_bytes=-1)]
    wrong = [c for c in bad if _abi(lib, **c) != _INV]
    assert not wrong, wrong
    ok = [dict(S=0), dict(S=0, ts=None, out=None, workspace=None, workspace_bytes=0, out_bytes=0),
          dict(S=0, ids=(1,), k_lo=0, k_hi=0)]
    wrong = [c for c in ok if _abi(lib, **c) != _OK]
    assert not wrong, wrong


# ---- what the device tests build their tolerance on ---------------------------------------------------------------------
def test_the_fp32_statement_is_at_the_quoted_ratios():
    """4 x these ratios is the device tolerance: measured on the host alone, never against the kernel."""
    worst = {name: 0.0 for name in A.SPECTRAL}
    for case in A.CASES:
        x, host, host32 = A.frames(*case[:2]), A.host_case(*case), A.host32_case(*case)
        for name in A.SPECTRAL:
            j = A.NAMES.index(name)
            worst[name] = max(worst[name], float(A.ratios(host32[:, :, j], host[:, :, j], A.scale_of(name, x)).max()))
    for name in A.SPECTRAL:
        print(f"c_{name} = max |host_features32 - host_features| / scale = {worst[name]:.4f}")
    assert {name: round(v, 2) for name, v in worst.items()} == HOST32_RATIO
    j = [A.NAMES.index(name) for name in ("std", "autocorr1")]
    for case in A.CASES:
        assert torch.equal(A.host32_case(*case)[:, :, j], A.host_case(*case)[:, :, j]), "the moments stay fp64"


@pytest.mark.parametrize("T,n,t_r,lo,hi", A.CASES)
def test_the_tolerance_cannot_hide_a_wrong_band(T, n, t_r, lo, hi):
    """A band that loses a bin or counts one twice (the middle bin of the band, (k_lo + k_hi) // 2, the same for every
    column), and a Nyquist bin of weight 2 where the band holds it, move every feature they touch by more than the device
    tolerance 4 c_f scale_f in every non-constant column of every subject.  Where a column of seeded frames was too faint
    at that one bin the case was replaced (``activity_data.SEEDS``, and T = 298 for T = 300); the margin is as stated."""
    x, host = A.frames(T, n), A.host_case(T, n, t_r, lo, hi)
    k_lo, k_hi = series_band(T, t_r, (lo, hi))
    K, mid = T // 2, (k_lo + k_hi) // 2
    drop, twice = np.ones((K, 1)), np.ones((K, 1))
    drop[mid - 1], twice[mid - 1] = 0.0, 2.0
    wrongs = [("drop", dict(mult=drop), A.SPECTRAL), ("twice", dict(mult=twice), A.SPECTRAL)]
    if T % 2 == 0 and k_hi == K:
        wrongs.append(("nyquist", dict(nyquist_weight=2.0), ("band_std", "band_fraction")))
    checked, least = 0, float("inf")
    for s in range(A.S):
        p2, _, q, lag = A.powers(x[s])
        live = torch.ones(n, dtype=torch.bool)
        if A.KINDS[s] == "constcol":
            live[A.const_col(n)] = False
        for what, how, touched in wrongs:
            wrong = torch.from_numpy(A.finish(p2, q, lag, T, k_lo, k_hi, NAMES, **how))
            for name in touched:
                j = NAMES.index(name)
                tol = 4 * HOST32_RATIO[name] * A.scale_of(name, x[s])
                moved = (wrong[:, j] - host[s, :, j]).abs()
                least = min(least, float((moved / tol)[live].min()))
                assert bool((moved[live] > tol[live]).all()), (s, what, name, float((moved / tol)[live].min()))
                checked += 1
    print(f"T={T} n={n}: the least |wrong - host| / (4 c_f scale_f) over {checked} checks = {least:.2f} (must exceed 1)")
    assert checked == A.S * (8 + 2 * (T % 2 == 0 and k_hi == K))
    assert (T, n) not in ((64, 64), (2, 3), (298, 12)) or checked == A.S * 10, "these cases hold the Nyquist bin"
