"""Interpolation of censored frames (``connectome_gnn_amd.ingest.interpolate_censored`` and
``filter_timeseries(..., interpolate=True)``) without a GPU: the host statement (tests/interp_data.py)
against ``scipy.interpolate.CubicSpline`` and on the properties that define it, the refusals of the two entry points that
are decided before the residency check, and the byte-count query of the C ABI.

Measured here: over ``interp_data.CASES`` the statement is at most 3.4e-13 of ``max_K |x|`` from scipy 1.15.3 (the gap of
600 frames in 1201, across which the cubic swings to six times the data; at most 7.3e-14 up to T = 300), inside the ``2^-40 = 9.1e-13``
it is granted; cubics, parabolas and lines come back within 8.0e-15 of their scale.
"""
import math

import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import confound_data as D
from tests import filter_data as F
from tests import interp_data as I


# ---- the masks and the frames ------------------------------------------------------------------------------------------
def test_the_new_masks_are_what_their_names_say():
    for T in (9, 67, 1201):
        m = I.masks(T)
        kept = {k: m[s] for s, k in enumerate(I.KINDS)}
        assert int(kept["three"].sum()) == 3 and int(kept["four"].sum()) == 4
        gap = (~kept["longgap"]).nonzero().flatten().tolist()
        assert gap == list(range(T // 4, T // 4 + T // 2))
        idx = kept["pairs"].nonzero().flatten()
        steps = (idx[1:] - idx[:-1]).tolist()
        assert set(steps[0::2]) == {1} and set(steps[1::2]) <= {2, 3, 4}, "two by two, gaps of 1 - 3 between"
        assert m.dtype == torch.bool and m.is_contiguous() and tuple(m.shape) == (14, T)
    assert I.KINDS[:10] == I.C.KINDS and torch.equal(I.masks(67)[:10], I.C.masks(10, 67))


def test_the_small_case_meets_every_special_count():
    counts = I.masks(9).sum(1).tolist()
    assert {0, 1, 2, 3, 4} <= set(counts), counts


def test_the_frames_carry_a_large_offset():
    x = I.frames(130, 84)
    assert x.dtype == torch.float32 and tuple(x.shape) == (I.S, 130, 84)
    assert float(x.mean((0, 1)).abs().max()) > 150 and 2.5 < float(x.std(1).mean()) < 3.5


# ---- the statement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n", I.CASES)
def test_the_statement_is_scipys_cubic_spline_inside_the_kept_range(T, n):
    interpolate = pytest.importorskip("scipy.interpolate")
    x, m, host = I.frames(T, n), I.masks(T), I.host_case(T, n)
    worst = 0.0
    for s, kind in enumerate(I.KINDS):
        idx = m[s].nonzero().flatten()
        if len(idx) < 2:
            continue
        lo, hi = int(idx[0]), int(idx[-1])
        spline = interpolate.CubicSpline(idx.double().numpy(), x[s][idx].double().numpy())
        want = torch.from_numpy(spline(torch.arange(lo, hi + 1).double().numpy()))
        err = (host[s][lo:hi + 1] - want).abs().max(0).values / I.scale(x[s], m[s])
        worst = max(worst, float(err.max()))
        assert bool((err <= I.BOUND).all()), (kind, float(err.max()))
    print(f"T={T} n={n}: max |host - CubicSpline| / max_K |x| = {worst:.3e} (bound 2^-40 = {I.BOUND:.3e})")


@pytest.mark.parametrize("T", [T for T, _ in I.CASES])
def test_a_not_a_knot_spline_reproduces_any_cubic(T):
    """... any parabola through three points and any line through two: needs no scipy."""
    t = torch.arange(T, dtype=torch.float64)
    cols = torch.stack([torch.ones(T, dtype=torch.float64), t, t * t / T, 50.0 * (t / T) ** 3 - t], 1)
    m = I.masks(T)
    worst = 0.0
    for s, kind in enumerate(I.KINDS):
        idx = m[s].nonzero().flatten()
        if len(idx) < 2:
            continue
        upto = 4 if len(idx) >= 4 else len(idx)                         # 1, t | t^2 | t^3
        lo, hi = int(idx[0]), int(idx[-1])
        got = I.host_interpolate(cols[:, :upto], m[s])
        err = (got - cols[:, :upto])[lo:hi + 1].abs().max(0).values / cols[:, :upto].abs().max(0).values
        worst = max(worst, float(err.max()))
        assert bool((err <= I.BOUND).all()), (kind, err.tolist())
    print(f"T={T}: polynomials come back within {worst:.3e} of their scale (bound {I.BOUND:.3e})")


@pytest.mark.parametrize("T,n", I.CASES[:4])
def test_ends_kept_frames_and_the_counts_zero_and_one(T, n):
    x, m, host = I.frames(T, n), I.masks(T), I.host_case(T, n)
    for s, kind in enumerate(I.KINDS):
        idx = m[s].nonzero().flatten()
        if len(idx) == 0:
            assert bool((host[s] == 0.0).all()), kind
            continue
        lo, hi = int(idx[0]), int(idx[-1])
        assert torch.equal(host[s][m[s]], x[s][m[s]].double()), (kind, "kept frames are the input")
        assert bool((host[s][:lo] == x[s][lo].double()).all()) and bool((host[s][hi:] == x[s][hi].double()).all()), kind
        if len(idx) == 1:
            assert bool((host[s] == x[s][lo].double()).all()), kind
    assert not bool(m[I.KINDS.index("none")].any()) and int(m[I.KINDS.index("one")].sum()) == 1


def test_two_kept_frames_give_the_line_and_a_constant_column_the_constant():
    T, n = 67, 97
    x, m = I.frames(T, n), I.masks(T)
    s = I.KINDS.index("two")
    a, b = m[s].nonzero().flatten().tolist()
    got = I.host_interpolate(x[s], m[s])
    t = torch.arange(a, b + 1, dtype=torch.float64)[:, None]
    line = x[s][a].double() + (t - a) / (b - a) * (x[s][b].double() - x[s][a].double())
    assert float((got[a:b + 1] - line).abs().max()) <= 1e-12
    flat = x.clone()
    flat[:, :, 3] = 101.3
    for s in range(I.S):
        if bool(m[s].any()):
            assert bool((I.host_interpolate(flat[s], m[s])[:, 3].float() == 101.3).all()), I.KINDS[s]


def test_censored_values_play_no_part_in_the_statement():
    T, n = 67, 97
    x, m, host = I.frames(T, n), I.masks(T), I.host_case(T, n)
    for s in range(I.S):
        bad = x[s].clone()
        bad[~m[s]] = float("nan")
        bad[~m[s], ::2] = 1e30
        assert torch.equal(I.host_interpolate(bad, m[s]), host[s]), I.KINDS[s]


def test_a_nan_in_a_kept_frame_stays_in_its_column():
    T, n = 33, 65
    x, m, host = I.frames(T, n), I.masks(T), I.host_case(T, n)
    s = I.KINDS.index("phase")
    bad = x[s].clone()
    bad[int(m[s].nonzero()[5]), 7] = float("nan")
    got = I.host_interpolate(bad, m[s])
    others = [i for i in range(n) if i != 7]
    assert torch.equal(got[:, others], host[s][:, others]) and not bool(torch.isfinite(got[:, 7]).all())


# ---- the entry points: what is decided before the residency check ---------------------------------------------------------
def _ts(T=30, n=20):
    return F.frames(3, T, n)


def _mask(S=3, T=30):
    return torch.ones(S, T, dtype=torch.bool)


def test_interpolate_needs_a_mask():
    with pytest.raises(ValueError, match="interpolate=True replaces the censored frames: give sample_mask="):
        ingest.filter_timeseries(_ts(), t_r=1.0, low_pass=0.05, interpolate=True)
    with pytest.raises(TypeError, match="interpolate must be a bool"):
        ingest.filter_timeseries(_ts(), t_r=1.0, sample_mask=_mask(), interpolate=1)
    with pytest.raises(TypeError):
        ingest.filter_timeseries(_ts(), 1.0, None, 0.05, None, None, _mask(), True)      # by keyword, as all of them


def test_the_default_still_refuses_a_low_pass_under_a_mask_in_the_same_words():
    ts, m = F.frames(3, 300, 20), _mask(3, 300)
    for kw in (dict(), dict(interpolate=False)):
        with pytest.raises(ValueError, match=r"drops 269 components, and with 0 confound columns.*CONFOUND_MAX = 64.*"
                                             "interpolated, which is not built"):
            ingest.filter_timeseries(ts, t_r=1.0, low_pass=0.05, sample_mask=m, **kw)


def test_valid_requests_reach_the_residency_check():
    ts, m, c = F.frames(3, 300, 20), _mask(3, 300), D.confounds(3, 300, 6)
    calls = (lambda: ingest.interpolate_censored(ts, m),
             lambda: ingest.interpolate_censored(ts, m, out=torch.empty_like(ts)),
             lambda: ingest.interpolate_censored(c, m),
             lambda: ingest.filter_timeseries(ts, t_r=1.0, low_pass=0.05, sample_mask=m, interpolate=True),
             lambda: ingest.filter_timeseries(ts, t_r=0.72, high_pass=0.01, low_pass=0.1, confounds=c, sample_mask=m,
                                              interpolate=True),
             lambda: ingest.filter_timeseries(ts, t_r=1.0, sample_mask=m, interpolate=True))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_the_interpolating_path_runs_the_unmasked_paths_checks():
    ts, m = F.frames(3, 300, 20), _mask(3, 300)
    with pytest.raises(ValueError, match="holds no component"):
        ingest.filter_timeseries(ts, t_r=1.0, high_pass=0.2, low_pass=0.2001, sample_mask=m, interpolate=True)
    long = torch.zeros(1, 1200, 2)
    with pytest.raises(ValueError, match="keeps 600 components and drops 599.*FILTER_MAX_COMPONENTS = 256"):
        ingest.filter_timeseries(long, t_r=1.0, low_pass=0.25, sample_mask=_mask(1, 1200), interpolate=True)
    with pytest.raises(ValueError, match=r"out must be \(3, 300, 20\)"):
        ingest.filter_timeseries(ts, t_r=1.0, low_pass=0.05, sample_mask=m, interpolate=True, out=torch.empty(3, 300, 19))
    with pytest.raises(ValueError, match=r"confounds must be \[S, T, q\] = \[3, 300, q\]"):
        ingest.filter_timeseries(ts, t_r=1.0, low_pass=0.05, sample_mask=m, interpolate=True,
                                 confounds=D.confounds(3, 299, 6))
    with pytest.raises(ValueError, match=r"sample_mask must be \[S, T\] = \[3, 300\]"):
        ingest.filter_timeseries(ts, t_r=1.0, low_pass=0.05, sample_mask=_mask(3, 299), interpolate=True)


def test_a_malformed_request_to_interpolate_censored_is_refused():
    ts = _ts()
    for bad, exc, msg in ((None, TypeError, "sample_mask must be a torch.Tensor"),
                          (_mask().numpy(), TypeError, "sample_mask must be a torch.Tensor"),
                          (_mask().to(torch.uint8), TypeError, "sample_mask must be bool"),
                          (_mask(3, 29), ValueError, r"sample_mask must be \[S, T\] = \[3, 30\]"),
                          (_mask(30, 3).t(), ValueError, "sample_mask must be contiguous"),
                          (_mask().to("meta"), ValueError, "sample_mask is on meta")):
        with pytest.raises(exc, match=msg):
            ingest.interpolate_censored(ts, bad)
    with pytest.raises(TypeError, match="timeseries must be float32"):
        ingest.interpolate_censored(ts.double(), _mask())
    with pytest.raises(ValueError, match=r"timeseries must be \[S, T, n\]"):
        ingest.interpolate_censored(ts[0], _mask())
    with pytest.raises(ValueError, match="out must be contiguous"):
        ingest.interpolate_censored(ts, _mask(), out=torch.empty(3, 20, 30).transpose(1, 2))
    with pytest.raises(TypeError, match="out must be float32"):
        ingest.interpolate_censored(ts, _mask(), out=torch.empty(3, 30, 20, dtype=torch.float64))
    with pytest.raises(TypeError):
        ingest.interpolate_censored(ts, _mask(), torch.empty_like(ts))                   # out is by keyword


# ---- the C ABI: the byte-count query needs no device --------------------------------------------------------------------
def test_the_workspace_query_refuses_every_bad_size():
    q = _lib.load().cgnn_ingest_interpolate_workspace_bytes
    for bad in ((6, 1, 20), (6, 2 ** 30 + 1, 20), (-1, 30, 20), (6, 30, 0), (6, 30, -3), (2 ** 31 // 20 + 1, 30, 20),
                (2 ** 31, 30, 1), (2 ** 21, 2 ** 30, 1)):
        assert q(*bad) < 0, bad
    assert _lib.PROTOTYPES["cgnn_ingest_interpolate_workspace_bytes"][1] == [_lib.I64, _lib.I32, _lib.I32]
    assert len(_lib.PROTOTYPES["cgnn_ingest_interpolate"][1]) == 11
    assert _lib.ABI_VERSION == 2, "the change is additive"


def test_the_production_band_is_out_of_the_regressions_reach():
    """What the feature is for: 0.01 - 0.1 Hz on 1200 frames at t_r = 0.72 drops over a thousand components."""
    k_lo, k_hi = ingest.filter_components(1200, 0.72, 0.01, 0.1)
    assert (k_lo, k_hi) == (18, 172) and 1199 - (k_hi - k_lo + 1) == 1044 > ingest.CONFOUND_MAX
    assert k_hi - k_lo + 1 <= ingest.FILTER_MAX_COMPONENTS and math.floor(2 * 1200 * 0.72 * 0.1) == 172
