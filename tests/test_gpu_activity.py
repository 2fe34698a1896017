"""The series features on the device (``connectome_gnn_amd.ingest.series_features``; csrc/activity.hip)
against the fp64 host statement of tests/activity_data.py.

Every case has five subjects, one per kind of ``activity_data.KINDS``: noise at offsets 0 and 100, a random walk at offset
10^4, a ramp, and a subject with one constant column.

Parity, per case, subject and column.  ``std`` and ``autocorr1``: ``|dev - host| <= 2^-24 |host| + 2^-40 s`` with
``s = max_t |xc|`` and ``s = 1``: one rounding of an fp64 value to fp32, plus what two fp64 summation orders are granted.
The four spectral features: ``|dev - host| <= 4 c_f scale_f``, where ``c_f`` is what the fp32 operands cost the host's own
model (tests/test_activity_math.py measures it there, never against the kernel) and the factor 4 covers the device's own
``cospi`` / ``sinpi`` and fused multiply-adds, as in tests/test_gpu_filter.py.  Each case prints the device's own worst
ratio per feature, in units of its bound (the largest seen on an MI355X over the eight cases: ``std`` 0.9783,
``autocorr1`` 0.9853 -- the rounding itself reaches 1 where a mantissa is near 1 -- ``alff`` 0.2498, ``falff`` 0.3153,
``band_std`` 0.2744, ``band_fraction`` 0.2189).

Everything else is exact and compared in bits: the constant column, a second run, other grids, subsets and orders of the
names, the input, and a NaN.
"""
import ctypes
import functools

import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib, encoder_choice, ingest
from connectome_gnn_amd.resident import ResidentDataLoader
from tests import activity_data as A
from tests import ingest_data as I
from tests.test_activity_math import HOST32_RATIO

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = A.S
NAMES = A.NAMES


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(T, n, t_r, lo, hi):
    """(host frames, the device's six features read back)"""
    x = A.frames(T, n)
    xd = x.to(DEV)
    got = ingest.series_features(xd, t_r=t_r, band=(lo, hi))
    assert got.dtype == torch.float32 and got.device.type == "cuda" and tuple(got.shape) == (S, n, 6)
    assert torch.equal(_bits(xd.cpu()), _bits(x)), "the input is left alone"
    return x, got.cpu()


def _bound(name, host, x):
    """[S, n] float64: what column `name` of the device may differ from the statement by."""
    j = NAMES.index(name)
    if name == "std":
        return 2.0 ** -24 * host[:, :, j].abs() + 2.0 ** -40 * A.amplitude(x)
    if name == "autocorr1":
        return 2.0 ** -24 * host[:, :, j].abs() + 2.0 ** -40
    return 4 * HOST32_RATIO[name] * A.scale_of(name, x)


@pytest.mark.parametrize("T,n,t_r,lo,hi", A.CASES)
def test_parity_with_the_statement(T, n, t_r, lo, hi):
    x, got = _case(T, n, t_r, lo, hi)
    host = A.host_case(T, n, t_r, lo, hi)
    worst = {}
    for j, name in enumerate(NAMES):
        r = A.ratios(got[:, :, j], host[:, :, j], _bound(name, host, x))
        worst[name] = r
        print(f"T={T} n={n} band=({lo}, {hi}) {name}: worst |dev - host| / bound = {float(r.max()):.4f} (bound 1)")
    for name, r in worst.items():
        assert bool((r <= 1.0).all()), (name, float(r.max()), int(r.argmax()))


@pytest.mark.parametrize("T,n,t_r,lo,hi", A.CASES)
def test_a_constant_column_is_exactly_zero(T, n, t_r, lo, hi):
    _, got = _case(T, n, t_r, lo, hi)
    assert torch.equal(_bits(got[4, A.const_col(n)]), torch.zeros(6, dtype=torch.int32)), "+0.0 in all six features"


@pytest.mark.parametrize("T,n,t_r,lo,hi", A.CASES)
def test_a_second_run_and_every_grid_give_the_same_bits(T, n, t_r, lo, hi):
    x, want = _case(T, n, t_r, lo, hi)
    xd = x.to(DEV)
    assert torch.equal(_bits(ingest.series_features(xd, t_r=t_r, band=(lo, hi)).cpu()), _bits(want)), "two runs"
    lib = _lib.load()
    for g in (1, 3):                              # with S = 5 and n = 360: 30 items on 1 and on 3 workgroups per unit
        try:
            assert lib.cgnn_set_fused_grid(g) == _lib.CGNN_OK
            few = ingest.series_features(xd, t_r=t_r, band=(lo, hi))
        finally:
            lib.cgnn_set_fused_grid(0)
        assert torch.equal(_bits(few.cpu()), _bits(want)), g
    assert torch.equal(_bits(xd.cpu()), _bits(x)), "the input is left alone"


SUBSETS = [("std", "autocorr1"), ("autocorr1",), ("std", "autocorr1", "alff", "band_std", "band_fraction"), ("falff",),
           ("band_fraction", "std"), ("falff", "alff"), ("band_std",), tuple(reversed(A.NAMES))]


@pytest.mark.parametrize("T,n,t_r,lo,hi", A.CASES)
def test_any_subset_in_any_order_is_the_columns_of_the_full_call(T, n, t_r, lo, hi):
    x, full = _case(T, n, t_r, lo, hi)
    xd = x.to(DEV)
    for names in SUBSETS:
        got = ingest.series_features(xd, t_r=t_r, band=(lo, hi), features=names)
        assert tuple(got.shape) == (S, n, len(names))
        want = full[:, :, [NAMES.index(name) for name in names]]
        assert torch.equal(_bits(got.cpu()), _bits(want)), names
    got = ingest.series_features(xd, features=["autocorr1", "std"])       # no t_r without a spectral name
    assert torch.equal(_bits(got.cpu()), _bits(full[:, :, [1, 0]]))


@pytest.mark.parametrize("T,n,t_r,lo,hi", [A.CASES[1], A.CASES[2], A.CASES[5], A.CASES[7]])
def test_a_nan_makes_exactly_its_column_nan(T, n, t_r, lo, hi):
    x, clean = _case(T, n, t_r, lo, hi)
    for s, t, c in ((4, T // 2, n - 1), (0, 0, 0), (2, T - 1, n // 2)):
        bad = x.clone()
        bad[s, t, c] = float("nan")
        got = ingest.series_features(bad.to(DEV), t_r=t_r, band=(lo, hi)).cpu()
        assert bool(torch.isnan(got[s, c]).all()), (s, t, c)
        got[s, c] = clean[s, c]
        assert torch.equal(_bits(got), _bits(clean)), (s, t, c, "no other bit changes")


def test_abi_runs_what_python_runs_and_refuses_before_any_launch():
    lib = _lib.load()
    T, n, t_r, lo, hi = A.CASES[6]
    x, want = _case(T, n, t_r, lo, hi)
    dev = x.to(DEV)
    sp = _lib.stream_ptr()
    k_lo, k_hi = ingest.series_band(T, t_r, (lo, hi))
    ids = (ctypes.c_int32 * 6)(0, 1, 2, 3, 4, 5)
    unknown = (ctypes.c_int32 * 6)(0, 1, 2, 3, 4, 6)
    need = lib.cgnn_ingest_activity_workspace_bytes(S, T, n, T // 2)
    assert need >= T * 2 * (T // 2) * 4 + 3 * S * n * 8
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((S, n, 6), -7.0, dtype=torch.float32, device=DEV)
    good = [_lib.ptr(dev), S, T, n, ids, 6, k_lo, k_hi, _lib.ptr(work), need, _lib.ptr(out), _lib.nbytes(out), sp]
    bad = {"short work": (9, need - 1), "short out": (11, _lib.nbytes(out) - 1), "ts NULL": (0, None),
           "k_lo > k_hi": (6, k_hi + 1), "unknown id": (4, unknown), "work NULL": (8, None), "out NULL": (10, None),
           "ids NULL": (4, None), "ts misaligned": (0, _lib.ptr(dev) + 2), "work misaligned": (8, _lib.ptr(work) + 8),
           "T < 2": (2, 1), "S < 0": (1, -1), "n = 0": (3, 0), "F = 0": (5, 0), "F = 7": (5, 7), "k_hi > K": (7, T // 2 + 1)}
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_activity(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()), (name, "nothing was written")
    assert lib.cgnn_ingest_activity(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK                 # S == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "nothing was written"
    assert lib.cgnn_ingest_activity(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(out.cpu()), _bits(want))
    empty = x[:0].to(DEV)
    assert tuple(ingest.series_features(empty, t_r=t_r, band=(lo, hi)).shape) == (0, n, 6)


def test_the_features_train_on_the_fused_path():
    Sn, T, n = 8, 130, 84
    g = torch.Generator().manual_seed(7)
    mix = 0.6 * torch.randn(4, n, generator=g)
    ts = ((torch.randn(Sn, T, 4, generator=g) @ mix + torch.randn(Sn, T, n, generator=g)) * 3.0 + 100.0).to(DEV)
    feats = ingest.series_features(ts, t_r=0.72, band=(0.01, 0.1))
    assert feats.shape == (Sn, n, 6) and bool(torch.isfinite(feats).all())
    ds = ingest.from_timeseries(ts, I.labels(Sn).to(DEV), keep=0.1, node_features=feats)
    assert ds.x is feats, "the dataset's x is that tensor"
    torch.manual_seed(3)
    m = C.GCNConnectome(6, 64, dropout=0.0)
    tr = C.Trainer(m, torch.optim.Adam(m.parameters(), lr=1e-3), device=DEV)
    ld = ResidentDataLoader(ds, 8, shuffle=True, structure_cache=True)
    loss = tr.train_epoch(ld)                     # one batch: one step
    assert loss == loss and abs(loss) != float("inf"), loss
    assert tr.model.impl_used == "fused" and tr.model._fused_kind == "tile"
    batch = next(iter(ld))
    choice = encoder_choice.choose(tr.model, batch, batch.structure())
    assert choice.kind == "tile" and choice.reason is None, choice
