"""The Butterworth band-pass on the device (``connectome_gnn_amd.ingest.filter_timeseries(..., filter="butterworth")``;
csrc/butterworth.hip) against the fp64 host statement, ``scipy.signal.sosfiltfilt`` of
``scipy.signal.butter`` (tests/butter_data.py).

Every case has five subjects, one per kind of ``butter_data.KINDS``: noise at offsets 0 and 100, a random walk at offset
10^4, a ramp, and a subject with one constant column.

Parity, per case, subject and column, for every frame: ``|dev - host| <= 2^-24 |host| + 2^-40 max_t |x|``.  The bound is
derived, not measured: one rounding of an fp64 value to fp32, plus what two fp64 formulations of the same filter are
granted (tests/test_butter_math.py holds a numpy model of the kernel's walk to that against scipy: at most 2^-43.4).  A
state, a forward output or the level held in fp32 cannot meet it on the walk at offset 10^4.  Each case prints the device's
own worst ratio (measured on an MI355X: 0.9950, 0.8673, 0.9892, 0.9988, 0.9968, 0.9932, 0.9955, 0.9974, 0.9918, 0.9848 and
0.9920 of the bound in the order of ``butter_data.CASES`` -- the rounding itself reaches 1 where a mantissa is near 1).

Everything else is exact and compared in bits: a constant column, in place, a second run, other grids, a NaN, and the
composed calls against the sequences of public calls they stand for.
"""
import ctypes
import functools

import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import butter_data as B
from tests import confound_data as D
from tests import interp_data as I

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = B.S


def _bits(t):
    return t.contiguous().view(torch.int32)


def _band(t_r, hp, lp, order):
    return dict(t_r=t_r, high_pass=hp, low_pass=lp, filter="butterworth", order=order)


@functools.lru_cache(maxsize=None)
def _case(T, n, t_r, hp, lp, order):
    """(host frames, the device's out-of-place result read back)"""
    x = B.frames(T, n)
    xd = x.to(DEV)
    got = ingest.filter_timeseries(xd, **_band(t_r, hp, lp, order))
    assert got.dtype == torch.float32 and got.device.type == "cuda" and tuple(got.shape) == (S, T, n)
    assert got.data_ptr() != xd.data_ptr()
    assert torch.equal(_bits(xd.cpu()), _bits(x)), "the input is left alone"
    return x, got.cpu()


@pytest.mark.parametrize("T,n,t_r,hp,lp,order", B.CASES)
def test_parity_with_sosfiltfilt(T, n, t_r, hp, lp, order):
    x, got = _case(T, n, t_r, hp, lp, order)
    host = B.host_case(T, n, t_r, hp, lp, order)
    worst = 0.0
    for s, kind in enumerate(B.KINDS):
        r = B.column_ratios(got[s], host[s], x[s])
        worst = max(worst, float(r.max()))
        print(f"T={T} n={n} order={order} {kind}: worst ratio {float(r.max()):.4f}")
    print(f"T={T} n={n} hp={hp} lp={lp} order={order}: max over subjects, columns and frames of |dev - host| / "
          f"(2^-24 |host| + 2^-40 max_t |x|) = {worst:.4f} (bound 1)")
    for s, kind in enumerate(B.KINDS):
        r = B.column_ratios(got[s], host[s], x[s])
        assert bool((r <= 1.0).all()), (kind, float(r.max()), int(r.argmax()))


@pytest.mark.parametrize("T,n,t_r,hp,lp,order", B.CASES)
def test_a_constant_column_is_exact(T, n, t_r, hp, lp, order):
    x, got = _case(T, n, t_r, hp, lp, order)
    c = B.const_col(n)
    level = B.CONST_VALUE if hp is None else 0.0                      # a low-pass keeps the level, the others remove it
    want = torch.full((T,), level, dtype=torch.float32)
    assert torch.equal(_bits(got[4, :, c]), _bits(want)), "exactly (positive) 0.0, or exactly the column's value"


@pytest.mark.parametrize("T,n,t_r,hp,lp,order", B.CASES)
def test_in_place_a_second_run_and_every_grid_give_the_same_bits(T, n, t_r, hp, lp, order):
    x, want = _case(T, n, t_r, hp, lp, order)
    band = _band(t_r, hp, lp, order)
    dev = x.to(DEV)
    assert ingest.filter_timeseries(dev, out=dev, **band) is dev
    assert torch.equal(_bits(dev.cpu()), _bits(want)), "out=timeseries gives the out-of-place bits"
    src = x.to(DEV)
    other = torch.full_like(src, -7.0)
    assert ingest.filter_timeseries(src, out=other, **band) is other
    assert torch.equal(_bits(other.cpu()), _bits(want)) and torch.equal(_bits(src.cpu()), _bits(x)), "two runs"
    lib = _lib.load()
    for g in (3, 1):                              # with S = 5 and n = 360: 30 items on 24 and 8 waves
        try:
            assert lib.cgnn_set_fused_grid(g) == _lib.CGNN_OK
            few = ingest.filter_timeseries(src, **band)
            few_in_place = src.clone()
            ingest.filter_timeseries(few_in_place, out=few_in_place, **band)
        finally:
            lib.cgnn_set_fused_grid(0)
        assert torch.equal(_bits(few.cpu()), _bits(want)), g
        assert torch.equal(_bits(few_in_place.cpu()), _bits(want)), g


@pytest.mark.parametrize("T,n,t_r,hp,lp,order", [B.CASES[0], B.CASES[3], B.CASES[5], B.CASES[8]])
def test_a_nan_makes_exactly_its_column_nan(T, n, t_r, hp, lp, order):
    x, clean = _case(T, n, t_r, hp, lp, order)
    band = _band(t_r, hp, lp, order)
    for s, t, c in ((4, T // 2, n - 1), (0, 0, 0), (2, T - 1, n // 2)):
        bad = x.clone()
        bad[s, t, c] = float("nan")
        got = ingest.filter_timeseries(bad.to(DEV), **band).cpu()
        assert bool(torch.isnan(got[s, :, c]).all()), (s, t, c, "a recursive filter run both ways reaches every frame")
        got[s, :, c] = clean[s, :, c]
        assert torch.equal(_bits(got), _bits(clean)), (s, t, c, "no other bit changes")


def test_abi_runs_what_python_runs_and_refuses_before_any_launch():
    lib = _lib.load()
    T, n, t_r, hp, lp, order = B.CASES[2]
    x, want = _case(T, n, t_r, hp, lp, order)
    dev = x.to(DEV)
    sp = _lib.stream_ptr()
    sos = ingest.butterworth_sos(t_r, hp, lp, order)
    L = len(sos)
    flat = (ctypes.c_double * (6 * L))(*(float(v) for r in sos for v in r))
    need = lib.cgnn_ingest_butterworth_workspace_bytes(S, T, n, L)
    assert need >= len(B.segments(T, B.edge_of(sos))) * 2 * L * 64 * 8
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((S, T, n), -7.0, dtype=torch.float32, device=DEV)
    good = [_lib.ptr(dev), S, T, n, flat, L, 0, _lib.ptr(work), need, _lib.ptr(out), _lib.nbytes(out), sp]
    bad = {"short work": (8, need - 1), "short out": (10, _lib.nbytes(out) - 1), "negative out bytes": (10, -1),
           "ts NULL": (0, None), "sos NULL": (4, None), "work NULL": (7, None), "out NULL": (9, None),
           "ts misaligned": (0, _lib.ptr(dev) + 2), "work misaligned": (7, _lib.ptr(work) + 8),
           "out misaligned": (9, _lib.ptr(out) + 2), "T <= edge": (2, 33), "T > 2^30": (2, 2 ** 30 + 1), "S < 0": (1, -1),
           "n = 0": (3, 0), "L = 0": (5, 0), "L = 9": (5, 9), "add_level = 2": (6, 2)}
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_butterworth(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    assert lib.cgnn_ingest_butterworth(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK              # S == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "nothing was written"
    assert lib.cgnn_ingest_butterworth(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(out.cpu()), _bits(want))
    good[9], good[10] = _lib.ptr(dev), _lib.nbytes(dev)                                           # out == ts
    assert lib.cgnn_ingest_butterworth(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(dev.cpu()), _bits(want))
    empty = x[:0].to(DEV)
    assert tuple(ingest.filter_timeseries(empty, **_band(t_r, hp, lp, order)).shape) == (0, T, n)


# ---- composition, in bits ---------------------------------------------------------------------------------------------------
BANDS = [(300, 360, 0.72, 0.01, 0.1), (130, 84, 2.0, 0.008, 0.08)]


@pytest.mark.parametrize("T,n,t_r,hp,lp", BANDS)
def test_confounds_are_filtered_alike_and_regressed(T, n, t_r, hp, lp):
    x, c = B.frames(T, n), D.confounds(S, T, 24)
    band = _band(t_r, hp, lp, 5)
    xd, cd = x.to(DEV), c.to(DEV)
    want = ingest.regress_confounds(ingest.filter_timeseries(xd, **band), ingest.filter_timeseries(cd, **band)).cpu()
    got = ingest.filter_timeseries(xd, confounds=cd, **band)
    assert got.data_ptr() != xd.data_ptr()
    assert torch.equal(_bits(xd.cpu()), _bits(x)) and torch.equal(_bits(cd.cpu()), _bits(c)), "the inputs are left alone"
    assert torch.equal(_bits(got.cpu()), _bits(want))
    assert ingest.filter_timeseries(xd, confounds=cd, out=xd, **band) is xd
    assert torch.equal(_bits(xd.cpu()), _bits(want)), "in place too"


def _sequence(xd, md, cd, band):
    """the public calls ``filter_timeseries(filter="butterworth", sample_mask=, interpolate=True)`` stands for"""
    o = ingest.interpolate_censored(xd, md)
    assert ingest.filter_timeseries(o, out=o, **band) is o
    if cd is None:
        return ingest.filter_timeseries(o, t_r=band["t_r"], sample_mask=md, out=o)
    ci = ingest.interpolate_censored(cd, md)
    cf = ingest.filter_timeseries(ci, out=ci, **band)
    return ingest.regress_confounds(o, cf, sample_mask=md, out=o)


@pytest.mark.parametrize("q", [None, 24])
@pytest.mark.parametrize("T,n,t_r,hp,lp", BANDS)
def test_the_composed_call_under_a_mask_is_its_sequence_of_public_calls(T, n, t_r, hp, lp, q):
    x, m = I.frames(T, n), I.masks(T)
    band = _band(t_r, hp, lp, 5)
    xd, md = x.to(DEV), m.to(DEV)
    c = None if q is None else D.confounds(I.S, T, q)
    cd = None if c is None else c.to(DEV)
    want = _sequence(xd, md, cd, band).cpu()
    got = ingest.filter_timeseries(xd, sample_mask=md, interpolate=True, confounds=cd, **band)
    assert got.data_ptr() != xd.data_ptr() and torch.equal(_bits(xd.cpu()), _bits(x)), "the input is left alone"
    assert cd is None or torch.equal(_bits(cd.cpu()), _bits(c))
    assert torch.equal(_bits(got.cpu()), _bits(want))
    assert bool((got.cpu()[~m] == 0.0).all()), "censored frames are exactly 0"
    assert ingest.filter_timeseries(xd, sample_mask=md, interpolate=True, confounds=cd, out=xd, **band) is xd
    assert torch.equal(_bits(xd.cpu()), _bits(want)), "in place too"
    with pytest.raises(ValueError, match="pass interpolate=True"):
        ingest.filter_timeseries(xd, sample_mask=md, **band)


def test_the_cosine_filter_gives_the_bits_it_gave():
    T, n, t_r, hp, lp = BANDS[0]
    xd = B.frames(T, n).to(DEV)
    want = ingest.filter_timeseries(xd, t_r=t_r, high_pass=hp, low_pass=lp)
    got = ingest.filter_timeseries(xd, t_r=t_r, high_pass=hp, low_pass=lp, filter="cosine", order=5)
    assert torch.equal(_bits(got.cpu()), _bits(want.cpu()))
