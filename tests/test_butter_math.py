"""The Butterworth path of ``connectome_gnn_amd.ingest.filter_timeseries`` without a GPU: the design
``ingest.butterworth_sos`` against ``scipy.signal.butter``, a numpy model of the kernel's walk (tests/butter_data.py)
against ``scipy.signal.sosfiltfilt``, every refusal that is decided before the residency check, and the refusals of the C
ABI, which are decided on the host before any launch.

Measured here with scipy 1.15.3: the designs of ``butter_data.CASES`` and of orders 1 .. 8 in the three types are within
1.6e-13 of the largest response at 512 frequencies and their poles within 7.5e-15 (bound 1e-12 for both); the model is
within 2^-43.4 max_t |x| (order 6; 2^-45.8 at order 5) of ``sosfiltfilt`` over the cases (bound 2^-40), and its chunked and unchunked forms agree in bits.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytest.importorskip("scipy.signal")
import scipy.signal  # noqa: E402

from connectome_gnn_amd import _lib, ingest  # noqa: E402
from tests import butter_data as B  # noqa: E402
from tests.abi_header import check_header  # noqa: E402
from tests import confound_data as D  # noqa: E402
from tests import filter_data as F  # noqa: E402

# every design of CASES, and orders 1 .. 8 as band-, high- and low-pass at the production band
DESIGNS = sorted({c[2:] for c in B.CASES} | {(0.72, hp, lp, order) for order in range(1, 9)
                                             for hp, lp in ((0.01, 0.1), (0.01, None), (None, 0.1))},
                 key=lambda d: tuple(-1.0 if v is None else v for v in d))


def _poles(sos):
    sos = np.asarray(sos)
    return np.sort_complex(np.concatenate([np.roots(r[3:] if r[5] != 0 else r[3:5]) for r in sos]))


# ---- the design -------------------------------------------------------------------------------------------------------------
def test_the_design_has_scipys_transfer_function():
    worst_h = worst_p = 0.0
    for t_r, hp, lp, order in DESIGNS:
        sos = ingest.butterworth_sos(t_r, hp, lp, order)
        ref = B.butter(t_r, hp, lp, order)
        assert sos.shape == ref.shape == ((order if hp is not None and lp is not None else (order + 1) // 2), 6)
        assert sos.dtype == np.float64 and bool((sos[:, 3] == 1.0).all())
        h, href = scipy.signal.sosfreqz(sos, 512)[1], scipy.signal.sosfreqz(ref, 512)[1]
        eh = float(np.abs(h - href).max() / np.abs(href).max())
        ep = float(np.abs(_poles(sos) - _poles(ref)).max())
        worst_h, worst_p = max(worst_h, eh), max(worst_p, ep)
        assert eh <= 1e-12 and ep <= 1e-12, (t_r, hp, lp, order, eh, ep)
        assert B.edge_of(sos) == B.edge_of(ref) == ingest._butterworth_edge(sos), (t_r, hp, lp, order)
    print(f"{len(DESIGNS)} designs: max |H - H_scipy| / max |H_scipy| = {worst_h:.3e}, max |pole - pole_scipy| = "
          f"{worst_p:.3e} (bound 1e-12 for both)")


def test_the_designs_gain_at_frequency_zero_and_its_poles():
    for t_r, hp, lp, order in DESIGNS:
        sos = ingest.butterworth_sos(t_r, hp, lp, order)
        assert isinstance(sos, np.ndarray) and sos.dtype == np.float64 and sos.ndim == 2
        assert bool((np.abs(_poles(sos)) < 1.0).all()), "every pole lies inside the unit circle"
        if hp is None:                                                # a low-pass: unit gain at frequency 0
            dc = math.prod((r[0] + r[1] + r[2]) / (1.0 + r[4] + r[5]) for r in sos)
            assert abs(dc - 1.0) <= 1e-12, (t_r, lp, order, dc)
        else:                                                         # zeros at 1: exactly no gain there
            assert all(r[0] + r[1] + r[2] == 0.0 for r in sos), (t_r, hp, lp, order)


def test_the_default_edges_are_the_documented_ones():
    assert ingest._butterworth_edge(ingest.butterworth_sos(0.72, 0.01, 0.1)) == 33
    assert ingest._butterworth_edge(ingest.butterworth_sos(0.72, 0.01, None)) == 18
    assert ingest._butterworth_edge(ingest.butterworth_sos(0.72, None, 0.1)) == 18
    assert ingest._butterworth_edge(ingest.butterworth_sos(0.72, 0.01, 0.1, 1)) == 9
    assert ingest._butterworth_edge(ingest.butterworth_sos(0.72, 0.01, 0.1, 8)) == 51
    assert ingest.FILTERS == ("cosine", "butterworth") and ingest.BUTTERWORTH_MAX_ORDER == 8


# ---- the kernel's walk --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n,t_r,hp,lp,order", B.CASES)
def test_the_model_of_the_kernel_is_sosfiltfilt(T, n, t_r, hp, lp, order):
    n = min(n, 12)                                                    # (a lane is a column: a few columns show all)
    x = B.frames(T, n)
    want = B.host(x, t_r, hp, lp, order)
    sos = ingest.butterworth_sos(t_r, hp, lp, order)
    worst = 0.0
    for s, kind in enumerate(B.KINDS):
        got = B.model(x[s], sos, hp is None)
        err = (got - want[s]).abs().max(0).values / B.scale(x[s])
        worst = max(worst, float(err.max()))
        assert bool((err <= B.BOUND).all()), (kind, float(err.max()))
        assert torch.equal(got, B.model(x[s], sos, hp is None, chunked=False)), (kind, "chunked == unchunked, in bits")
    c = B.const_col(n)
    flat = B.model(x[4], sos, hp is None)[:, c].float()
    level = torch.tensor(B.CONST_VALUE if hp is None else 0.0, dtype=torch.float32)
    assert bool((flat == level).all()), "a constant column is exactly 0.0, or exactly its value under a low-pass"
    print(f"T={T} n={n} order={order}: max |model - sosfiltfilt| / max_t |x| = 2^{math.log2(max(worst, 1e-300)):.1f} "
          f"(bound 2^-40)")


def test_the_segments_cover_the_frames_and_start_at_the_first_real_frame():
    for T, edge in ((34, 33), (19, 18), (63, 33), (64, 33), (160, 51), (1201, 33), (10, 9)):
        segs = B.segments(T, edge)
        assert segs[0][0] == 0 and sum(c for _, c in segs) == T + edge
        assert all(a + c == b for (a, c), (b, _) in zip(segs, segs[1:]))
        assert all(f + c <= T for f, c in segs if c == B.CHUNK), "a chunk holds real frames only"
        assert len(segs) <= T // B.CHUNK + (B.CHUNK - 1 + edge) // B.SHORT + B.SHORT - 1, "the slab's bound"


# ---- the entry point: what is decided before the residency check ---------------------------------------------------------
def _ts(T=60, n=20):
    return F.frames(3, T, n)


def _mask(S=3, T=60):
    return torch.ones(S, T, dtype=torch.bool)


BAND = dict(t_r=0.72, high_pass=0.01, low_pass=0.1)


def test_the_filter_and_the_order_are_checked():
    with pytest.raises(ValueError, match=r"unknown filter 'bessel'.*FILTERS = \('cosine', 'butterworth'\)"):
        ingest.filter_timeseries(_ts(), filter="bessel", **BAND)
    with pytest.raises(ValueError, match=r"order=3 belongs to filter=\"butterworth\""):
        ingest.filter_timeseries(_ts(), filter="cosine", order=3, **BAND)
    with pytest.raises(ValueError, match=r"order=3 belongs to filter=\"butterworth\""):
        ingest.filter_timeseries(_ts(), order=3, **BAND)
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match=rf"BUTTERWORTH_MAX_ORDER\] = \[1, 8\], got {bad}"):
            ingest.filter_timeseries(_ts(), filter="butterworth", order=bad, **BAND)
        with pytest.raises(ValueError, match="BUTTERWORTH_MAX_ORDER"):
            ingest.butterworth_sos(0.72, 0.01, 0.1, bad)
    for bad in (5.0, True, "5"):
        with pytest.raises(TypeError, match="order must be an int"):
            ingest.filter_timeseries(_ts(), filter="butterworth", order=bad, **BAND)
    with pytest.raises(TypeError):
        ingest.filter_timeseries(_ts(), 0.72, 0.01, 0.1, None, None, None, False, "butterworth")   # by keyword


def test_the_bounds_are_refused_not_clipped():
    nyq = 1.0 / (2 * 0.72)
    with pytest.raises(ValueError, match="needs high_pass=, low_pass= or both"):
        ingest.filter_timeseries(_ts(), t_r=0.72, filter="butterworth")
    for kw in (dict(low_pass=0.7), dict(low_pass=nyq), dict(high_pass=0.7), dict(high_pass=0.0), dict(low_pass=-0.1),
               dict(high_pass=0.01, low_pass=0.7)):
        with pytest.raises(ValueError, match=rf"below the Nyquist frequency {nyq!r} Hz".replace(".", r"\.")):
            ingest.filter_timeseries(_ts(), t_r=0.72, filter="butterworth", **kw)
    for hp, lp in ((0.1, 0.01), (0.05, 0.05)):
        with pytest.raises(ValueError, match="high_pass must lie below low_pass"):
            ingest.filter_timeseries(_ts(), t_r=0.72, high_pass=hp, low_pass=lp, filter="butterworth")
    with pytest.raises(ValueError, match="low_pass must be finite"):
        ingest.filter_timeseries(_ts(), t_r=0.72, low_pass=float("nan"), filter="butterworth")
    with pytest.raises(ValueError, match="t_r must be > 0"):
        ingest.filter_timeseries(_ts(), t_r=0.0, low_pass=0.1, filter="butterworth")


def test_a_run_no_longer_than_the_pad_is_refused_as_scipy_refuses_it():
    with pytest.raises(ValueError, match=r"5 sections.*edge = 33.*T > 33 frames, got T = 33"):
        ingest.filter_timeseries(_ts(33), filter="butterworth", **BAND)
    with pytest.raises(ValueError, match=r"3 sections.*edge = 18.*got T = 18"):
        ingest.filter_timeseries(_ts(18), t_r=0.72, high_pass=0.01, filter="butterworth")
    with pytest.raises(ValueError, match=r"3 sections.*edge = 18.*got T = 10"):
        ingest.filter_timeseries(_ts(10), t_r=0.72, low_pass=0.1, filter="butterworth")
    with pytest.raises(ValueError):
        scipy.signal.sosfiltfilt(B.butter(0.72, 0.01, 0.1, 5), np.zeros(33))
    scipy.signal.sosfiltfilt(B.butter(0.72, 0.01, 0.1, 5), np.zeros(34))


def test_a_mask_needs_the_frames_interpolated():
    with pytest.raises(ValueError, match="recursive and cannot skip the censored frames.*pass interpolate=True"):
        ingest.filter_timeseries(_ts(), filter="butterworth", sample_mask=_mask(), **BAND)
    with pytest.raises(ValueError, match="interpolate=True replaces the censored frames: give sample_mask="):
        ingest.filter_timeseries(_ts(), filter="butterworth", interpolate=True, **BAND)


def test_the_shapes_are_checked_as_on_the_cosine_path():
    ts = _ts()
    with pytest.raises(ValueError, match=r"out must be \(3, 60, 20\)"):
        ingest.filter_timeseries(ts, filter="butterworth", out=torch.empty(3, 60, 19), **BAND)
    with pytest.raises(ValueError, match=r"confounds must be \[S, T, q\] = \[3, 60, q\]"):
        ingest.filter_timeseries(ts, filter="butterworth", confounds=D.confounds(3, 59, 6), **BAND)
    with pytest.raises(ValueError, match=r"sample_mask must be \[S, T\] = \[3, 60\]"):
        ingest.filter_timeseries(ts, filter="butterworth", sample_mask=_mask(3, 59), interpolate=True, **BAND)
    with pytest.raises(TypeError, match="timeseries must be float32"):
        ingest.filter_timeseries(ts.double(), filter="butterworth", **BAND)


def test_valid_requests_reach_the_residency_check():
    ts, m, c = _ts(), _mask(), D.confounds(3, 60, 6)
    calls = (lambda: ingest.filter_timeseries(ts, filter="butterworth", **BAND),
             lambda: ingest.filter_timeseries(ts, filter="butterworth", order=8, out=ts, **BAND),
             lambda: ingest.filter_timeseries(ts, t_r=0.72, low_pass=0.1, filter="butterworth", order=1),
             lambda: ingest.filter_timeseries(c, t_r=0.72, high_pass=0.01, filter="butterworth"),
             lambda: ingest.filter_timeseries(ts, filter="butterworth", confounds=c, **BAND),
             lambda: ingest.filter_timeseries(ts, filter="butterworth", sample_mask=m, interpolate=True, **BAND),
             lambda: ingest.filter_timeseries(ts, filter="butterworth", sample_mask=m, interpolate=True, confounds=c,
                                              **BAND),
             lambda: ingest.filter_timeseries(ts, filter="cosine", order=5, **BAND))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- the C ABI: every refusal is decided on the host ---------------------------------------------------------------------------
def _flat(sos):
    return (ctypes.c_double * (6 * len(sos)))(*(v for r in sos for v in r))


def test_the_workspace_query_refuses_every_bad_size():
    q = _lib.load().cgnn_ingest_butterworth_workspace_bytes
    for bad in ((6, 1, 20, 5), (6, 2 ** 30 + 1, 20, 5), (-1, 60, 20, 5), (6, 60, 0, 5), (6, 60, -3, 5),
                (2 ** 31 // 20 + 1, 60, 20, 5), (2 ** 31, 60, 1, 5), (6, 60, 20, 0), (6, 60, 20, 9), (6, 60, 20, -1)):
        assert q(*bad) < 0, bad
    assert _lib.ABI_VERSION == 2, "the change is additive"


def test_the_prototypes_match_their_header_type_by_type():
    """The two entry points are declared in include/cgnn_butterworth.h, which cgnn.h includes, and bound by
    ``_lib.BUTTERWORTH_PROTOTYPES``: the return type and every argument type of both, the library's exports, and the
    comparison itself against a doctored header."""
    hdr = check_header("cgnn_butterworth.h", _lib.BUTTERWORTH_PROTOTYPES,
                       ["cgnn_ingest_butterworth_workspace_bytes", "cgnn_ingest_butterworth"],
                       [("const double* sos, int32_t L", "const double* sos, int64_t L")])
    assert "#define CGNN_BUTTER_MAX_SECTIONS 8" in hdr and ingest.BUTTERWORTH_MAX_ORDER == 8


def test_the_entry_point_refuses_before_any_launch():
    """No device is present here: a call that went as far as a launch could not return CGNN_EINVAL for these."""
    lib = _lib.load()
    S, T, n = 3, 60, 20
    sos = ingest.butterworth_sos(**BAND)
    ts, work, out = 4096, 8192, 16384                                 # addresses that nothing dereferences
    good = [ts, S, T, n, _flat(sos), 5, 0, work, 2 ** 40, out, 4 * S * T * n, None]

    def refused(at, v):
        return lib.cgnn_ingest_butterworth(*(good[:at] + [v] + good[at + 1:])) == _lib.CGNN_EINVAL

    def with_sos(rows, T=T):
        args = list(good)
        args[2], args[4], args[5] = T, _flat(rows), len(rows)
        return lib.cgnn_ingest_butterworth(*args)

    assert refused(5, 0) and refused(5, 9) and refused(5, -1), "L outside 1 .. CGNN_BUTTER_MAX_SECTIONS"
    assert with_sos(list(sos) + list(sos)) == _lib.CGNN_EINVAL, "ten sections"
    for j, v, why in ((3, 2.0, "a0 != 1"), (0, float("nan"), "a NaN"), (4, float("inf"), "an Inf"), (5, -float("inf"), "")):
        rows = [list(r) for r in sos]
        rows[2][j] = v
        assert with_sos(rows) == _lib.CGNN_EINVAL, why
    rows = [list(r) for r in sos]
    rows[1][4], rows[1][5] = -2.0, 1.0                                # 1 + a1 + a2 == 0
    assert with_sos(rows) == _lib.CGNN_EINVAL
    assert with_sos(sos, T=33) == _lib.CGNN_EINVAL, "T <= edge"
    low = ingest.butterworth_sos(0.72, None, 0.1)
    assert with_sos(low, T=18) == _lib.CGNN_EINVAL, "T <= edge of three sections, one of them of first order"
    for at, v, why in ((2, 1, "T = 1"), (2, 2 ** 30 + 1, "T > 2^30"), (1, -1, "S < 0"), (3, 0, "n = 0"),
                       (1, 2 ** 31 // n + 1, "S n >= 2^31"), (4, None, "sos NULL"), (6, 2, "add_level"),
                       (8, -1, "negative workspace bytes"), (10, -1, "negative out bytes"), (0, None, "ts NULL"),
                       (7, None, "work NULL"), (9, None, "out NULL"), (0, ts + 2, "ts misaligned"),
                       (7, work + 8, "work misaligned"), (9, out + 2, "out misaligned"), (8, 8, "short work"),
                       (10, 4 * S * T * n - 1, "short out")):
        assert refused(at, v), why
    assert lib.cgnn_ingest_butterworth(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK, "S == 0: nothing to do"
