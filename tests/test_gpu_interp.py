"""Interpolation of censored frames on the device (``connectome_gnn_amd.ingest.interpolate_censored`` and
``filter_timeseries(..., sample_mask=, interpolate=True)``; csrc/interpolate.hip) against the fp64 host
statement (tests/interp_data.py).

Every case has fourteen subjects, one per mask kind of ``interp_data.KINDS``.

Parity, per case and column, for every censored frame: ``|dev - host| <= 2^-24 |host| + 2^-40 max_K |x|``.  The bound is
derived, not measured: one rounding of an fp64 value to fp32, plus what two fp64 formulations of the same spline are
granted (tests/test_interp_math.py holds the host statement to that against scipy).  A solve or an evaluation in fp32
cannot meet it on frames whose columns sit at offsets of order 100.  Each case prints the device's own worst ratio
(measured on an MI355X: 0.8957, 0.9888, 0.9952, 0.9950, 0.9995 and 0.9978 of the bound in the order of ``interp_data.CASES``
-- the rounding itself reaches 1 where a mantissa is near 1; the composed call within 7.13 of ``2^-24 max |xc|`` of its host
statement on the kept frames of the last test, tolerance 63.8).

Everything else is exact: kept frames, ends, the counts 0 and 1, an all-True mask and a constant column are compared in
bits, and so are garbage in censored frames, a NaN in a kept one, in place, a second run and other grids.  The composed
call is compared in bits with the sequence of public calls it stands for, each of which has a parity suite of its own.
"""
import functools
import math

import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import censor_data as C
from tests import confound_data as D
from tests import filter_data as F
from tests import interp_data as I

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = I.S
C_FILTER = 4 * 15.95                              # tests/test_gpu_filter.py's tolerance, in 2^-24 max |xc|
# (T, n, t_r, high_pass, low_pass) of the composed call
BANDS = [(300, 360, 0.72, 0.01, 0.1), (1201, 70, 0.72, 0.01, 0.1), (130, 84, 2.0, 0.008, 0.08)]


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(T, n):
    """(host frames, host masks, the device's out-of-place result read back)"""
    x, m = I.frames(T, n), I.masks(T)
    xd, md = x.to(DEV), m.to(DEV)
    got = ingest.interpolate_censored(xd, md)
    assert got.dtype == torch.float32 and got.device.type == "cuda" and tuple(got.shape) == (S, T, n)
    assert got.data_ptr() != xd.data_ptr()
    assert torch.equal(_bits(xd.cpu()), _bits(x)) and torch.equal(md.cpu(), m), "the inputs are left alone"
    return x, m, got.cpu()


@pytest.mark.parametrize("T,n", I.CASES)
def test_parity_with_the_fp64_statement(T, n):
    x, m, got = _case(T, n)
    host = I.host_case(T, n)
    worst = 0.0
    for s, kind in enumerate(I.KINDS):
        r = I.column_ratios(got[s], host[s], x[s], m[s])
        worst = max(worst, float(r.max()))
        assert bool((r <= 1.0).all()), (kind, float(r.max()), int(r.argmax()))
    print(f"T={T} n={n}: max over subjects, columns and censored frames of |dev - host| / (2^-24 |host| + 2^-40 max_K |x|)"
          f" = {worst:.4f} (bound 1)")


@pytest.mark.parametrize("T,n", I.CASES)
def test_what_is_exact(T, n):
    x, m, got = _case(T, n)
    for s, kind in enumerate(I.KINDS):
        assert torch.equal(_bits(got[s][m[s]]), _bits(x[s][m[s]])), (kind, "kept frames are bit copies")
        idx = m[s].nonzero().flatten()
        if len(idx) == 0:
            assert torch.equal(_bits(got[s]), torch.zeros(T, n, dtype=torch.int32)), (kind, "exact (positive) zeros")
            continue
        lo, hi = int(idx[0]), int(idx[-1])
        assert torch.equal(_bits(got[s][:lo]), _bits(x[s][lo].expand(lo, n))), (kind, "the head holds x[t_0]")
        assert torch.equal(_bits(got[s][hi:]), _bits(x[s][hi].expand(T - hi, n))), (kind, "the tail holds x[t_{m-1}]")
        if len(idx) == 1:
            assert torch.equal(_bits(got[s]), _bits(x[s][lo].expand(T, n))), kind
    assert torch.equal(_bits(got[0]), _bits(x[0])) and bool(m[0].all()), "an all-True mask gives a bit copy"


@pytest.mark.parametrize("T,n", [I.CASES[1], I.CASES[3]])
def test_a_column_constant_over_the_kept_frames_is_that_constant(T, n):
    x, m, clean = _case(T, n)
    flat = x.clone()
    flat[:, :, n // 2] = 101.3
    flat[:, :, 0] = -0.1
    flat[:, :, n // 2][~m] = 55.0                                     # it varies in censored frames, which nobody reads
    got = ingest.interpolate_censored(flat.to(DEV), m.to(DEV)).cpu()
    some = m.any(1)
    assert bool((got[some][:, :, n // 2] == 101.3).all()) and bool((got[some][:, :, 0] == -0.1).all())
    assert bool((got[~some] == 0.0).all())
    others = [i for i in range(1, n) if i != n // 2]
    assert torch.equal(_bits(got[:, :, others]), _bits(clean[:, :, others])), "columns never mix"
    t_r, hp, lp = 2.0, 0.01, 0.1
    y = ingest.filter_timeseries(flat.to(DEV), t_r=t_r, high_pass=hp, low_pass=lp, sample_mask=m.to(DEV),
                                 interpolate=True).cpu()
    assert bool((y[:, :, n // 2] == 0.0).all()) and bool((y[:, :, 0] == 0.0).all()), "exactly 0 after the band-pass"


@pytest.mark.parametrize("T,n", [I.CASES[0], I.CASES[2], I.CASES[5]])
def test_censored_values_change_no_bit(T, n):
    x, m, want = _case(T, n)
    bad = x.clone()
    bad[~m] = float("nan")
    bad[:, :, 1::3][~m] = float("inf")
    bad[:, :, 2::3][~m] = 1e30
    got = ingest.interpolate_censored(bad.to(DEV), m.to(DEV)).cpu()
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("T,n", [I.CASES[1], I.CASES[4]])
def test_a_nan_in_a_kept_frame_stays_in_its_column_of_its_subject(T, n):
    x, m, clean = _case(T, n)
    for s in (I.KINDS.index("phase"), I.KINDS.index("three"), I.KINDS.index("longgap")):
        idx = m[s].nonzero().flatten()
        bad = x.clone()
        bad[s, int(idx[len(idx) // 2]), n - 2] = float("nan")
        got = ingest.interpolate_censored(bad.to(DEV), m.to(DEV)).cpu()
        assert not bool(torch.isfinite(got[s, :, n - 2]).all()), I.KINDS[s]
        got[s, :, n - 2] = clean[s, :, n - 2]
        assert torch.equal(_bits(got), _bits(clean)), I.KINDS[s]


@pytest.mark.parametrize("T,n", I.CASES)
def test_in_place_a_second_run_and_every_grid_give_the_same_bits(T, n):
    x, m, want = _case(T, n)
    md = m.to(DEV)
    dev = x.to(DEV)
    assert ingest.interpolate_censored(dev, md, out=dev) is dev
    assert torch.equal(_bits(dev.cpu()), _bits(want)), "out=timeseries gives the out-of-place bits"
    src = x.to(DEV)
    other = torch.full_like(src, -7.0)
    assert ingest.interpolate_censored(src, md, out=other) is other
    assert torch.equal(_bits(other.cpu()), _bits(want)) and torch.equal(_bits(src.cpu()), _bits(x)), "two runs"
    lib = _lib.load()
    for g in (3, 1):                              # 36 and 12 waves for 28 - 84 items: with 12 every wave walks several
        try:
            assert lib.cgnn_set_fused_grid(g) == _lib.CGNN_OK
            few = ingest.interpolate_censored(src, md)
        finally:
            lib.cgnn_set_fused_grid(0)
        assert torch.equal(_bits(few.cpu()), _bits(want)), g


def test_abi_runs_what_python_runs_and_refuses_before_any_launch():
    lib = _lib.load()
    T, n = I.CASES[2]
    x, m, want = _case(T, n)
    dev, keep = x.to(DEV), m.to(DEV)
    sp = _lib.stream_ptr()
    need = lib.cgnn_ingest_interpolate_workspace_bytes(S, T, n)
    assert need > 44 * S * T + 4 * S
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((S, T, n), -7.0, dtype=torch.float32, device=DEV)
    good = [_lib.ptr(dev), S, T, n, _lib.ptr(keep), S * T, _lib.ptr(work), need, _lib.ptr(out), _lib.nbytes(out), sp]
    bad = {"short keep": (5, S * T - 1), "short work": (7, need - 1), "short out": (9, _lib.nbytes(out) - 1),
           "negative keep bytes": (5, -1), "ts NULL": (0, None), "keep NULL": (4, None), "work NULL": (6, None),
           "out NULL": (8, None), "ts misaligned": (0, _lib.ptr(dev) + 2), "work misaligned": (6, _lib.ptr(work) + 8),
           "out misaligned": (8, _lib.ptr(out) + 2), "T = 1": (2, 1), "T > 2^30": (2, 2 ** 30 + 1), "S < 0": (1, -1),
           "n = 0": (3, 0), "S n >= 2^31": (1, 2 ** 31 // n + 1)}
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_interpolate(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    assert lib.cgnn_ingest_interpolate(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK              # S == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "nothing was written"
    assert lib.cgnn_ingest_interpolate(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(out.cpu()), _bits(want))
    good[8], good[9] = _lib.ptr(dev), _lib.nbytes(dev)                                            # out == ts
    assert lib.cgnn_ingest_interpolate(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(dev.cpu()), _bits(want))
    empty = x[:0].to(DEV)
    assert tuple(ingest.interpolate_censored(empty, m[:0].to(DEV)).shape) == (0, T, n)


# ---- the composed call ---------------------------------------------------------------------------------------------------
def _sequence(xd, md, cd, band):
    """the public calls ``filter_timeseries(..., sample_mask=, interpolate=True)`` stands for (module docstring of ingest)"""
    o = ingest.interpolate_censored(xd, md)
    assert ingest.filter_timeseries(o, out=o, **band) is o
    if cd is None:
        return ingest.filter_timeseries(o, t_r=band["t_r"], sample_mask=md, out=o)
    ci = ingest.interpolate_censored(cd, md)
    cf = ingest.filter_timeseries(ci, out=ci, **band)
    return ingest.regress_confounds(o, cf, sample_mask=md, out=o)


@pytest.mark.parametrize("q", [None, 24])
@pytest.mark.parametrize("T,n,t_r,hp,lp", BANDS)
def test_the_composed_call_is_its_sequence_of_public_calls(T, n, t_r, hp, lp, q):
    x, m = I.frames(T, n), I.masks(T)
    band = dict(t_r=t_r, high_pass=hp, low_pass=lp)
    xd, md = x.to(DEV), m.to(DEV)
    c = None if q is None else D.confounds(S, T, q)
    cd = None if c is None else c.to(DEV)
    want = _sequence(xd, md, cd, band).cpu()
    got = ingest.filter_timeseries(xd, sample_mask=md, interpolate=True, confounds=cd, **band)
    assert got.data_ptr() != xd.data_ptr() and torch.equal(_bits(xd.cpu()), _bits(x)), "the input is left alone"
    assert cd is None or torch.equal(_bits(cd.cpu()), _bits(c))
    assert torch.equal(_bits(got.cpu()), _bits(want))
    assert bool((got.cpu()[~m] == 0.0).all()), "censored frames are exactly 0"
    assert bool(torch.isfinite(got).all())
    assert ingest.filter_timeseries(xd, sample_mask=md, interpolate=True, confounds=cd, out=xd, **band) is xd
    assert torch.equal(_bits(xd.cpu()), _bits(want)), "in place too"


# ---- the point of the feature --------------------------------------------------------------------------------------------
def test_scrubbing_and_a_band_pass_are_one_call():
    """Two ROIs share an in-band cosine (period 50 frames = 36 s: 0.028 Hz); a fifth of the frames carry spikes of 1e4
    and are censored.  The regression path refuses the band (260 components to drop); the interpolating path returns, on
    the kept frames, what the host statement of the same composition returns."""
    num, T, n, t_r, hp, lp = 2, 300, 8, 0.72, 0.01, 0.1
    band = dict(t_r=t_r, high_pass=hp, low_pass=lp)
    g = torch.Generator().manual_seed(12000)
    t = torch.arange(T, dtype=torch.float64)
    wave = 2.0 * torch.cos(2.0 * math.pi * t / 50.0)
    x = 0.5 * torch.randn(num, T, n, generator=g, dtype=torch.float64)
    x[:, :, :2] += wave[None, :, None]
    keep = torch.ones(num, T, dtype=torch.bool)
    for s in range(num):
        at = torch.randperm(T, generator=g)[:T // 5]
        keep[s, at] = False
        x[s, at] += 1e4 * torch.where(torch.rand(T // 5, 1, generator=g) < 0.5, -1.0, 1.0).double()
    x = x.float().contiguous()
    xd, kd = x.to(DEV), keep.to(DEV)
    with pytest.raises(ValueError, match="drops 260 components.*interpolated, which is not built"):
        ingest.filter_timeseries(xd, sample_mask=kd, **band)
    got = ingest.filter_timeseries(xd, sample_mask=kd, interpolate=True, **band).cpu()
    clean = F.host_filter(wave[:, None].expand(T, 2).float(), **band)             # the cosine alone through the band
    for s in range(num):
        filled = I.host_interpolate(x[s], keep[s]).float()                        # rounded to fp32 once, as stored
        want = C.host_centred(F.host_filter(filled, **band), keep[s])
        scale = F.centred(filled).abs().max(0).values
        r = (got[s].double() - want)[keep[s]].abs().max(0).values / (F.EPS * scale)
        off = (want[:, :2] - C.host_centred(clean, keep[s]))[keep[s]].abs().max()
        print(f"subject {s}: max over columns of max_K |dev - host| / (2^-24 max |xc|) = {float(r.max()):.4f} (tolerance "
              f"{C_FILTER:.2f}); the host statement is within {float(off):.3f} of the clean cosine of amplitude 2 on the "
              f"kept frames, r_01 there {F.corr01(want[keep[s]]):.3f} (raw series: {F.corr01(x[s]):.3f})")
        assert bool((r <= C_FILTER).all()), (s, float(r.max()))
        assert bool((got[s][~keep[s]] == 0.0).all())
