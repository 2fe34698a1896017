"""connectome_gnn_amd.ingest.filter_timeseries (csrc/filter.hip) on the device, against the fp64 host statement
(tests/filter_data.py).

Tolerance, for every column: ``max_t |y_dev - host_filter| <= c 2^-24 max_t |xc|``.  ``c`` is measured on the host, never
against the kernel: the statement evaluated on the operands the device holds (``filter_data.host_filter32``: fp32 ``xc``,
fp32 basis, the host's fp32 matmul, the form the call chooses) is at most 15.95 of ``2^-24 max |xc|`` away from the fp64
one over the issue's parity cases (the 256 components kept of 600 x 12; asserted in tests/test_filter_math.py, with the
further cases of ``WIDE_CASES`` inside it), and a
factor 4 covers the device's summation order and its own ``cospi``, as in tests/test_gpu_shrinkage.py: ``c = 63.8``, that
is ``3.8e-6 max |xc|``, while a lost or doubled component moves a column by more than ``2e-2 max |xc|`` (asserted
there too).  Each parity case prints the device's own ratio.
"""
import ctypes
import functools
import math

import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import filter_data as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
C_TOL = 4 * 15.95                                 # 4 x the largest host32 ratio (module docstring)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _band(t_r, hp, lp):
    return dict(t_r=t_r, high_pass=hp, low_pass=lp)


@functools.lru_cache(maxsize=None)
def _case(T, n, S, t_r, hp, lp):
    """(host frames, device result read back)"""
    x = D.frames(S, T, n)
    got = ingest.filter_timeseries(x.to(DEV), **_band(t_r, hp, lp))
    assert got.dtype == torch.float32 and got.device.type == "cuda" and tuple(got.shape) == (S, T, n)
    return x, got.cpu()


def _check(got, x, band, what):
    """every column of one subject within the tolerance; returns the largest ratio"""
    r = D.column_ratios(got, x, band["t_r"], band["high_pass"], band["low_pass"])
    worst = float(r.max())
    print(f"{what}: max over columns of max_t |y - host| / (2^-24 max_t |xc|) = {worst:.4f} (tolerance {C_TOL:.2f})")
    assert bool((r <= C_TOL).all()), (what, worst, int(r.argmax()))
    return worst


@pytest.mark.parametrize("T,n,S,t_r,hp,lp", D.CASES + D.WIDE_CASES)
def test_parity_with_the_fp64_statement(T, n, S, t_r, hp, lp):
    x, got = _case(T, n, S, t_r, hp, lp)
    complement, comps = D.form(T, *D.components(T, t_r, hp, lp))
    for s in range(S):
        _check(got[s], x[s], _band(t_r, hp, lp), f"T={T} n={n} {'complement' if complement else 'keep'} "
                                                  f"{len(comps)} subject {s}")
    again = ingest.filter_timeseries(x.to(DEV), **_band(t_r, hp, lp))
    assert torch.equal(_bits(again.cpu()), _bits(got)), "two calls, the same bits"


@pytest.mark.parametrize("T,n,S,t_r,hp,lp", D.CASES + D.WIDE_CASES)
def test_in_place_gives_the_bits_of_out_of_place(T, n, S, t_r, hp, lp):
    x, want = _case(T, n, S, t_r, hp, lp)
    dev = x.to(DEV)
    ret = ingest.filter_timeseries(dev, out=dev, **_band(t_r, hp, lp))
    assert ret is dev
    assert torch.equal(_bits(dev.cpu()), _bits(want))
    other = torch.full_like(dev, -7.0)
    src = x.to(DEV)
    assert ingest.filter_timeseries(src, out=other, **_band(t_r, hp, lp)) is other
    assert torch.equal(_bits(other.cpu()), _bits(want)) and torch.equal(src.cpu(), x), "the input is left as it is"


@pytest.mark.parametrize("T,n,t_r,hp,lp", [(33, 65, 2.0, 0.01, 0.1), (300, 360, 2.0, 0.008, 0.09),
                                           (326, 72, 1.0, None, 0.25077)])
def test_every_grid_gives_the_same_bits(T, n, t_r, hp, lp):
    S = 7                                                             # every workgroup walks several items
    x = D.frames(S, T, n)
    dev = x.to(DEV)
    full = ingest.filter_timeseries(dev, **_band(t_r, hp, lp))
    lib = _lib.load()
    for g in (3, 16):
        try:
            assert lib.cgnn_set_fused_grid(g) == _lib.CGNN_OK
            few = ingest.filter_timeseries(dev, **_band(t_r, hp, lp))
        finally:
            lib.cgnn_set_fused_grid(0)
        assert torch.equal(_bits(few), _bits(full)), g
    got = full.cpu()
    for s in (0, 6):
        _check(got[s], x[s], _band(t_r, hp, lp), f"T={T} n={n} of 7 subjects: subject {s}")


@pytest.mark.parametrize("T,n,S,t_r,hp,lp", [D.CASES[1], D.CASES[2], D.CASES[5], D.CASES[8]])
def test_a_constant_column_gives_exact_zeros(T, n, S, t_r, hp, lp):
    x, clean = _case(T, n, S, t_r, hp, lp)
    flat = x.clone()
    flat[:, :, n // 2] = 101.3
    flat[S - 1, :, 0] = -0.1
    got = ingest.filter_timeseries(flat.to(DEV), **_band(t_r, hp, lp)).cpu()
    assert bool((got[:, :, n // 2] == 0.0).all()) and bool((got[S - 1, :, 0] == 0.0).all())
    others = [i for i in range(1, n) if i != n // 2]
    assert torch.equal(_bits(got[:, :, others]), _bits(clean[:, :, others])), "columns never mix"


@pytest.mark.parametrize("T,n,S", [(2, 3, 2), (33, 65, 2), (300, 360, 2)])
def test_without_bounds_the_output_is_the_centred_input(T, n, S):
    x = D.frames(S, T, n)
    got = ingest.filter_timeseries(x.to(DEV), t_r=1.0).cpu()
    want = (x.double() - x.double().mean(1, keepdim=True))            # the host's fp64 mean
    ulp = torch.maximum(want.float().abs(), torch.tensor(2.0 ** -126)).log2().floor().exp2() * 2.0 ** -23
    assert bool(((got.double() - want.float().double()).abs() <= ulp.double()).all()), "to one ulp of xc"


def test_a_nan_stays_in_its_column_of_its_subject():
    for case in (D.CASES[2], D.CASES[3], D.CASES[0]):                 # keep, complement, pure centring
        T, n, S, t_r, hp, lp = case
        x, clean = _case(*case)
        bad = x.clone()
        bad[1, T // 2, n - 2] = float("nan")
        got = ingest.filter_timeseries(bad.to(DEV), **_band(t_r, hp, lp)).cpu()
        assert not bool(torch.isfinite(got[1, :, n - 2]).any()), case
        got[1, :, n - 2] = clean[1, :, n - 2]
        assert torch.equal(_bits(got), _bits(clean)), case


def _cosine(T, k, amplitude=1.0):
    t = torch.arange(T, dtype=torch.float64)
    return amplitude * torch.cos(math.pi * (2 * t + 1) * k / (2 * T))


def test_a_kept_cosine_is_returned_and_a_dropped_one_is_removed():
    T, n, t_r, hp, lp = 130, 84, 0.72, 0.01, 0.15                     # components 2 .. 28
    assert D.components(T, t_r, hp, lp) == (2, 28)
    x = torch.zeros(2, T, n, dtype=torch.float64)
    x[0] = 3.0 + _cosine(T, 20, 1.5)[:, None]                        # kept: comes back, without its offset
    x[1] = 3.0 + _cosine(T, 1, 1.5)[:, None]                         # component 1 is below k_lo (2 would be kept)
    x = x.float().contiguous()
    got = ingest.filter_timeseries(x.to(DEV), **_band(t_r, hp, lp)).cpu()
    _check(got[0], x[0], _band(t_r, hp, lp), "component 20 alone")
    # (against the cosine itself: also the rounding of 3 + 1.5 cos to fp32, half an ulp of 4.5 = 4 x 2^-24)
    assert float((got[0].double() - _cosine(T, 20, 1.5)[:, None]).abs().max()) <= C_TOL * D.EPS * 1.5 + 8 * D.EPS
    assert float(got[1].abs().max()) <= C_TOL * D.EPS * 1.5, "at most the tolerance of its amplitude is left"
    # and component 2 dropped by a band that starts above it
    hp = 0.017                                                        # floor(2 * 130 * 0.72 * 0.017) = 3: k_lo = 4
    assert D.components(T, t_r, hp, lp) == (4, 28)
    y = (3.0 + _cosine(T, 2, 1.5)[:, None]).expand(T, n).float().contiguous()[None]
    got = ingest.filter_timeseries(y.to(DEV), **_band(t_r, hp, lp)).cpu()
    assert float(got.abs().max()) <= C_TOL * D.EPS * 1.5


def test_abi_runs_what_python_runs_and_refuses_before_any_launch():
    lib = _lib.load()
    T, n, S, t_r, hp, lp = D.CASES[2]
    x, want = _case(*D.CASES[2])
    dev = x.to(DEV)
    sp = _lib.stream_ptr()
    complement, comps = D.form(T, *D.components(T, t_r, hp, lp))
    K = len(comps)
    arr = (ctypes.c_int32 * K)(*comps)
    need = lib.cgnn_ingest_filter_workspace_bytes(S, T, n, K)
    assert need == T * 32 * 4 + S * n * 8
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((S, T, n), -7.0, dtype=torch.float32, device=DEV)
    good = [_lib.ptr(dev), S, T, n, arr, K, int(complement), _lib.ptr(work), need, _lib.ptr(out), _lib.nbytes(out), sp]

    def arr_of(*ks):
        return (ctypes.c_int32 * len(ks))(*ks)

    bad = {"short work": (8, need - 1), "short out": (10, _lib.nbytes(out) - 1), "ts NULL": (0, None),
           "work NULL": (7, None), "out NULL": (9, None), "work misaligned": (7, _lib.ptr(work) + 8),
           "out misaligned": (9, _lib.ptr(out) + 2), "K = 257": (5, 257), "K = -1": (5, -1), "T = 1": (2, 1),
           "comps NULL": (4, None), "a component 0": (4, arr_of(0, *comps[1:])),
           "a component T": (4, arr_of(*comps[:-1], T)), "not ascending": (4, arr_of(*reversed(comps))),
           "a component twice": (4, arr_of(comps[0], *comps[:-1])), "S < 0": (1, -1), "n = 0": (3, 0)}
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_filter(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    assert lib.cgnn_ingest_filter(*(good[:5] + [0, 0] + good[7:])) == _lib.CGNN_EINVAL, "nothing kept"
    assert lib.cgnn_ingest_filter(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK                   # S == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "nothing was written"
    assert lib.cgnn_ingest_filter(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(out.cpu()), _bits(want))
    good[9], good[10] = _lib.ptr(dev), _lib.nbytes(dev)                                           # out == ts
    assert lib.cgnn_ingest_filter(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(dev.cpu()), _bits(want))
    empty = x[:0].to(DEV)
    assert tuple(ingest.filter_timeseries(empty, **_band(t_r, hp, lp)).shape) == (0, T, n)


def test_no_cohort_sized_temporaries():
    S, T, n = 64, 300, 360
    dev = D.frames(2, T, n).repeat(S // 2, 1, 1).contiguous().to(DEV)
    band = _band(2.0, 0.008, 0.09)
    ingest.filter_timeseries(dev, **band)                             # (the kernels are loaded)
    need = _lib.load().cgnn_ingest_filter_workspace_bytes(S, T, n, 99)
    assert need == T * 128 * 4 + S * n * 8
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ingest.filter_timeseries(dev, out=dev, **band)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < need + 2 ** 20 < 4 * S * T * n // 8, (peak, need)


def test_a_shared_drift_no_longer_makes_an_edge():
    """The point of the feature: two ROIs that share a slow drift and nothing else."""
    band = {k: D.DRIFT[k] for k in ("t_r", "high_pass", "low_pass")}
    x = D.drift_pair()
    S, n = x.shape[0], x.shape[2]
    dev = x.to(DEV)
    raw = ingest.correlation_matrices(dev).cpu()
    clean = ingest.filter_timeseries(dev, **band)
    r = ingest.correlation_matrices(clean).cpu()
    for s in range(S):
        print(f"subject {s}: r_01 {float(raw[s, 0, 1]):.4f} before, {float(r[s, 0, 1]):.4f} after "
              f"(host: {D.corr01(x[s]):.4f}, {D.corr01(D.host_filter(x[s], **band)):.4f})")
        assert float(raw[s, 0, 1]) > 0.9 and abs(float(r[s, 0, 1])) < 0.3
    y = torch.arange(S, dtype=torch.long) % 2
    ds = ingest.from_timeseries(clean, y, keep=0.25)
    before = ingest.from_timeseries(dev, y, keep=0.25)
    assert ds.x.shape == (S, n, 1) and int(ds.edge_ptr[-1]) > 0

    def has_edge(d, s):
        lo, hi = int(d.edge_ptr[s]), int(d.edge_ptr[s + 1])
        e = d.edge_local[:, lo:hi].cpu()
        return bool(((e[0] == 0) & (e[1] == 1)).any()) or bool(((e[0] == 1) & (e[1] == 0)).any())

    for s in range(S):
        assert has_edge(before, s) and not has_edge(ds, s), s
