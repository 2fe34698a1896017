"""connectome_gnn_amd.ingest.correlation_matrices / from_timeseries on the device (csrc/timeseries.hip) against the
fp64 host statement (tests/timeseries_data.py): parity at ``atol = (T + 32 + 4 kappa) 2^-23`` (twice the first-order
bound of T fp32 accumulations of products whose magnitudes sum to at most 1, the dropped terms of a split product
and the centring and scaling roundings, which grow with kappa = max |mean| / std, computed here in fp64), the exact
properties, windows, the grid stride, 64-bit offsets, memory, the C ABI's refusals, and the result served through
ResidentDataLoader + Trainer."""
import functools

import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib, ingest
from connectome_gnn_amd.resident import ResidentDataLoader
from connectome_gnn_amd.synthetic import RaggedPackedDataset
from tests import timeseries_data as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 3
SHAPES = [(2, 1), (2, 5), (3, 2), (7, 20), (31, 63), (32, 64), (33, 65), (70, 84), (33, 130), (40, 360),
          # the 96 x 96 tile walk: one full tile on the vector path; two tiles, one live column in the second, and
          # three tiles, both on the element path
          (5, 96), (33, 97), (9, 193)]


@functools.lru_cache(maxsize=None)
def _case(T, n, offset=0.0):
    """(host time series with the planted columns, fp64 statement, tolerance, device output, |.| device output)"""
    ts = D.planted(S, T, n, offset=offset)
    dev = ts.to(DEV)
    return ts, D.host_corr(ts), D.atol(T, D.kappa(ts)), ingest.correlation_matrices(dev), \
        ingest.correlation_matrices(dev, absolute=True)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_parity(got, want, tol, what):
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), what
    err = float((got.cpu().double() - want).abs().max())
    print(f"{what}: max error {err:.3e}, atol {tol:.3e}")
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("T,n", SHAPES)
def test_parity_with_the_fp64_statement(T, n):
    _, want, tol, got, _ = _case(T, n)
    assert got.device.type == "cuda" and got.is_contiguous()
    _check_parity(got, want, tol, f"T={T} n={n}")


def test_parity_at_an_offset_of_1000_standard_deviations():
    """kappa ~ 1000: the bound is ~ 5e-4; a raw-moment formula is off by kappa^2 2^-24 ~ 0.06 here."""
    ts, want, tol, got, _ = _case(70, 84, 1000.0)
    assert D.kappa(ts) > 900.0 and 4e-4 < tol < 6e-4
    _check_parity(got, want, tol, "T=70 n=84 offset=1000")


def _exact(T, n, offset):
    ts, _, _, got, got_abs = _case(T, n, offset)
    g = got.cpu()
    assert torch.equal(_bits(g), _bits(g.transpose(1, 2))), "bit-symmetric"
    assert float(g.min()) >= -1.0 and float(g.max()) <= 1.0 and not bool(torch.isnan(g).any())
    flat = torch.zeros(S, n, dtype=torch.bool)
    if n >= 5:
        flat[-1, 1] = flat[-1, n - 2] = True
    assert torch.equal(g.diagonal(dim1=1, dim2=2), (~flat).float()), "diagonal: exactly 1, 0 for a constant column"
    if n >= 5:
        for c in (1, n - 2):
            assert torch.equal(g[-1, c], torch.zeros(n)) and torch.equal(g[-1, :, c], torch.zeros(n)), c
    assert torch.equal(_bits(got_abs), _bits(got.abs())), "absolute=True is |.| of the default"
    again = ingest.correlation_matrices(ts.to(DEV))
    assert torch.equal(_bits(again), _bits(got)), "two calls, the same bits"


@pytest.mark.parametrize("T,n,offset", [s + (0.0,) for s in SHAPES] + [(70, 84, 1000.0)])
def test_exact_properties(T, n, offset):
    _exact(T, n, offset)


@pytest.mark.parametrize("n", [20, 84])
def test_windows_are_units_in_subject_major_order(n):
    T = 50
    ts = D.recipe(S, T, n)
    dev = ts.to(DEV)
    y = torch.tensor([1, 0, 1])
    for L, st in ((50, 50), (20, 20), (20, 7), (2, 1)):
        W = D.num_windows(T, L, st)
        got = ingest.correlation_matrices(dev, window=L, stride=st)
        assert tuple(got.shape) == (S * W, n, n)
        if st == L:
            assert torch.equal(_bits(ingest.correlation_matrices(dev, window=L)), _bits(got)), "stride defaults to L"
        for w in range(W):
            part = ingest.correlation_matrices(dev[:, w * st:w * st + L].contiguous())
            assert torch.equal(_bits(got[w::W]), _bits(part)), (L, st, w)
        _check_parity(got, D.host_corr(ts, window=L, stride=st), D.atol(L, D.kappa(ts, L, st)), f"n={n} L={L} st={st}")
        ds = ingest.from_timeseries(dev, y, keep=0.2, window=L, stride=st)
        assert torch.equal(ds.labels.cpu(), y.repeat_interleave(W)) and ds.x.shape == (S * W, n, 1)
        assert ds.edge_ptr.shape == (S * W + 1,)


def test_many_units_walk_the_grid_stride():
    Sg, T, n = 40, 40, 84
    ts = D.recipe(Sg, T, n, seed=3)
    dev = ts.to(DEV)
    lib = _lib.load()
    try:
        assert lib.cgnn_set_fused_grid(3) == _lib.CGNN_OK
        few = ingest.correlation_matrices(dev)
        few_w = ingest.correlation_matrices(dev, window=16, stride=8)
    finally:
        lib.cgnn_set_fused_grid(0)
    full = ingest.correlation_matrices(dev)
    assert torch.equal(_bits(few), _bits(full))
    assert torch.equal(_bits(few_w), _bits(ingest.correlation_matrices(dev, window=16, stride=8)))
    want, tol = D.host_corr(ts), D.atol(T, D.kappa(ts))
    _check_parity(few, want, tol, "3 workgroups per grid")
    _check_parity(full, want, tol, "default grid")


def test_offsets_beyond_2_31_elements():
    """1700 x 3600 x 360 = 2.2 G input elements (8.8 GB), generated on the device in slices; subjects 0, S // 2 and
    S - 1 against the host statement."""
    Sb, T, n = 1700, 3600, 360
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        pytest.skip(f"needs 16 GB of free device memory, {free / 2 ** 30:.1f} GB are free")
    assert Sb * T * n > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(5)
    ts = torch.empty(Sb, T, n, device=DEV)
    mix = torch.randn(4, n, device=DEV, generator=g)
    scale = 0.5 + 3.0 * torch.rand(n, device=DEV, generator=g)
    for lo in range(0, Sb, 50):                          # in slices: no second cohort-sized temporary
        hi = min(lo + 50, Sb)
        lat = torch.randn(hi - lo, T, 4, device=DEV, generator=g)
        ts[lo:hi] = (lat @ mix + torch.randn(hi - lo, T, n, device=DEV, generator=g)) * scale + 0.5
    got = ingest.correlation_matrices(ts)
    assert tuple(got.shape) == (Sb, n, n)
    for s in (0, Sb // 2, Sb - 1):
        x = ts[s:s + 1].cpu()
        _check_parity(got[s:s + 1], D.host_corr(x), D.atol(T, D.kappa(x)), f"subject {s}")
        assert torch.equal(_bits(got[s]), _bits(got[s].t()))
    del ts, got


def test_no_cohort_sized_temporaries():
    """Above the resident input only the output [U, n, n] and the statistics [U, n, 2] are allocated; the unfolded
    copy [U, 50, 84] that the torch formulation needs (17 MB here) does not fit under the bound."""
    Sm, T, n, L, st = 64, 200, 84, 50, 10
    dev = D.recipe(Sm, T, n, seed=2).to(DEV)
    U = Sm * D.num_windows(T, L, st)
    ingest.correlation_matrices(dev, window=L, stride=st)              # (the library is loaded, the kernels too)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ingest.correlation_matrices(dev, window=L, stride=st)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert tuple(out.shape) == (U, n, n)
    assert 4 * U * n * n <= peak <= 4 * U * n * n + 8 * U * n + 2 ** 20, (peak, 4 * U * n * n, 8 * U * n)
    assert 4 * U * L * n > 8 * U * n + 2 ** 20


def _refusals(fn, good, written, required, scalars, sentinels):
    """Every bad form of `good` returns CGNN_EINVAL and leaves the sentinel-filled outputs alone.
    written: (pointer position, byte-count position) of each written buffer; required: positions of the pointers
    that may not be NULL; scalars: {name: (position, value)}."""
    bad = {}
    for p, nb in written:
        bad[f"buffer at {p} one byte short"] = good[:nb] + [good[nb] - 1] + good[nb + 1:]
    for p in required:
        bad[f"pointer at {p} NULL"] = good[:p] + [None] + good[p + 1:]
    for name, (p, v) in scalars.items():
        bad[name] = good[:p] + [v] + good[p + 1:]
    for name, args in bad.items():
        assert fn(*args) == _lib.CGNN_EINVAL, name
    torch.cuda.synchronize()
    for t, v in sentinels:
        assert bool((t == v).all())


def test_corr_abi_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    T, n, L, st = 7, 20, 3, 2
    ts = D.recipe(S, T, n)
    dev = ts.to(DEV)
    sp = _lib.stream_ptr()
    limits = {"S < 0": (1, -1), "T = 1": (2, 1), "T = 0": (2, 0), "T < 0": (2, -4), "n = 0": (3, 0), "n < 0": (3, -1),
              "U * n >= 2^31": (1, 2 ** 31 // n + 1), "n * n >= 2^31": (3, 46341), "window = 1": (4, 1),
              "window < 0": (4, -2), "window > T": (4, T + 1)}

    def f32(*shape):
        return torch.full(shape, -7.0, dtype=torch.float32, device=DEV)

    for window, stride, more in ((0, 0, {}), (L, st, {"stride = 0": (5, 0), "stride < 0": (5, -1)})):
        W = D.num_windows(T, window or None, stride or None)
        stats, out = f32(S * W, n, 2), f32(S * W, n, n)
        good = [_lib.ptr(dev), S, T, n, window, stride, 0, _lib.ptr(stats), _lib.nbytes(stats), _lib.ptr(out),
                _lib.nbytes(out), sp]
        _refusals(lib.cgnn_ingest_corr, good, [(7, 8), (9, 10)], [0, 7, 9], dict(limits, **more),
                  [(stats, -7.0), (out, -7.0)])
        assert lib.cgnn_ingest_corr(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK          # S == 0
        assert lib.cgnn_ingest_corr(None, 0, T, n, window, stride, 0, None, 0, None, 0, sp) == _lib.CGNN_OK
        torch.cuda.synchronize()
        assert bool((stats == -7.0).all()) and bool((out == -7.0).all())
        assert lib.cgnn_ingest_corr(*good) == _lib.CGNN_OK
        want = D.host_corr(ts, window=window or None, stride=stride or None)
        _check_parity(out, want, D.atol(window or T, D.kappa(ts, window or None, stride or None)), f"window={window}")
        assert torch.equal(_bits(out), _bits(ingest.correlation_matrices(dev, window=window or None,
                                                                        stride=stride or None)))
    assert tuple(ingest.correlation_matrices(dev[:0]).shape) == (0, n, n)


def _same_dataset(got, want):
    """Two device datasets, every field, dtypes and shapes included."""
    assert type(got) is RaggedPackedDataset and type(want) is RaggedPackedDataset
    for name in ("x", "edge_local", "edge_weight", "labels", "edge_ptr_dev"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.device.type == "cuda" and a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, a.shape, b.shape)
        assert torch.equal(a, b), name
    assert got.edge_ptr.device.type == "cpu" and got.edge_ptr.dtype == torch.long
    assert torch.equal(got.edge_ptr, want.edge_ptr) and torch.equal(got.edge_ptr_dev.cpu(), got.edge_ptr)


def _fit(ds):
    torch.manual_seed(3)
    m = C.GCNConnectome(1, 64, dropout=0.0)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
    tr = C.Trainer(m, opt, device=DEV, graph=True)
    ld = ResidentDataLoader(ds, 16, shuffle=True, structure_cache=True)
    vl = ResidentDataLoader(ds, 16, shuffle=False, structure_cache=True)
    hist = tr.fit(ld, vl, num_epochs=2, patience=10, verbose=False)
    return tr, hist, [p.detach().clone() for p in tr.model.parameters()]


@pytest.mark.parametrize("window,stride", [(None, None), (30, 15)])
def test_timeseries_through_loader_and_trainer(window, stride):
    """72 subjects x 60 frames x 84 ROIs, two classes that differ in the coupling of the first 28 ROIs, keep = 0.1,
    the default strength feature: from_timeseries is from_matrices of correlation_matrices, and Trainer.fit over
    ResidentDataLoader(structure_cache=True) gives the same bits on both, on the fused path."""
    Sg, T, n = 72, 60, 84
    ts, y = D.two_classes(Sg, T, n)
    W = D.num_windows(T, window, stride)
    dev = ts.to(DEV)
    ds = ingest.from_timeseries(dev, y, keep=0.1, window=window, stride=stride)
    mats = ingest.correlation_matrices(dev, window=window, stride=stride)
    ref = ingest.from_matrices(mats, y.repeat_interleave(W), keep=0.1)
    _same_dataset(ds, ref)
    assert ds.x.shape == (Sg * W, n, 1) and int(ds.edge_ptr[-1]) > 0
    tr_a, hist_a, par_a = _fit(ds)
    tr_b, hist_b, par_b = _fit(ref)
    assert tr_a.model.impl_used == "fused" and tr_b.model.impl_used == "fused"
    assert hist_a == hist_b and len(hist_a["train_loss"]) == 2
    assert all(torch.isfinite(torch.tensor(v)).all() for v in hist_a.values())
    for a, b in zip(par_a, par_b):
        assert torch.equal(a, b)
