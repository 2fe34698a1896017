"""connectome_gnn_amd.ingest.kendall_counts / kendall_matrices (csrc/kendall.hip) and ``kendall=True`` of the
connectivity calls on the device, against the host statement (tests/kendall_data.py).

The counts are exact integers: ``torch.equal`` on int32.  Tau is ``fp32(G_ij / sqrt(G_ii G_jj))`` formed in fp64: the
device's fp64 square root and quotient are each within an ulp of fp64, which can move the fp32 rounding across at most one
boundary, so the bound is one fp32 ulp of ``fp32(statement)``; the number of entries that differ at all is printed (0 on
an MI355X: both operations are correctly rounded there).  Symmetry, the unit diagonal, the zero and the NaN rows are
compared bit for bit.
"""
import numpy as np
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import censor_data as CD
from tests import kendall_data as KD
from tests import rank_data as RD

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 3
# the edges of a chunk of 16 frames, of the frame block and the 64-deep instruction (both 64: 63, 64, 65, and 129 = two
# blocks and a frame), of a 96-wide tile (95, 96, 97; 193: three tiles and a tile pair that is not adjacent); long units
# with few columns
SHAPES = [(2, 1), (3, 7), (15, 16), (16, 17), (17, 15), (63, 5), (64, 33), (65, 96), (127, 97), (128, 95), (129, 193),
          (257, 20), (1200, 20), (4096, 3)]
WINDOWS = [(200, 50, 10), (67, 33, 17)]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _counts_are(got, want, what=""):
    assert got.dtype == torch.int32 and got.device.type == "cuda", what
    assert torch.equal(got.cpu(), torch.from_numpy(want).to(torch.int32)), what


def _tau_is(got, g, what="", absolute=False):
    """got (fp32, device) against the statement's normalisation of the counts g (int64 array): within one fp32 ulp;
    returns the number of entries that differ at all."""
    assert got.dtype == torch.float32 and got.device.type == "cuda", what
    u = KD.ulps(got.cpu().numpy(), KD.tau_of(g, absolute))
    assert u.max(initial=0) <= 1, (what, int(u.max()))
    return int((u != 0).sum())


def _unfold(m, L, st):
    return m.unfold(1, L, st).reshape(-1, L).contiguous()


@pytest.mark.parametrize("T,n", SHAPES)
def test_the_counts_are_the_statements_and_tau_is_within_an_ulp(T, n):
    x = RD.series(S, T, n).to(DEV)
    want = KD.series_counts(S, T, n)
    got = ingest.kendall_counts(x)
    assert tuple(got.shape) == (S, n, n)
    _counts_are(got, want, (T, n))
    assert torch.equal(got, got.transpose(1, 2)), "bit-symmetric"
    tau = ingest.kendall_matrices(x)
    differ = _tau_is(tau, want, (T, n))
    print(f"kendall tau (T, n) = ({T}, {n}): {differ} of {tau.numel()} entries differ from fp32(statement)")
    assert torch.equal(_bits(tau), _bits(tau.transpose(1, 2))), "bit-symmetric"
    ok = ~torch.isnan(tau)
    assert bool((tau[ok].abs() <= 1.0).all())
    assert torch.equal(_bits(ingest.kendall_matrices(x, absolute=True))[ok], _bits(tau.abs())[ok])


def test_the_special_columns_are_exactly_as_stated():
    T, n = 129, 33
    x = RD.series(S, T, n)
    g = ingest.kendall_counts(x.to(DEV)).cpu()
    tau = ingest.kendall_matrices(x.to(DEV)).cpu()
    col = RD.SPECIAL
    c, d = col["constant"], col["descending"]
    assert not bool(g[c % S, c].any()) and not bool(g[c % S, :, c].any())
    assert torch.equal(_bits(tau[c % S, c]), torch.zeros(n, dtype=torch.int32)), "an exact zero row, diagonal included"
    assert torch.equal(_bits(tau[c % S, :, c]), torch.zeros(n, dtype=torch.int32))
    assert int(g[d % S, d, d]) == T * (T - 1) // 2, "no ties"
    diag = torch.diagonal(g, dim1=1, dim2=2)
    assert torch.equal(torch.diagonal(tau, dim1=1, dim2=2)[diag > 0], torch.ones(int((diag > 0).sum())))
    # the NaN column: -1 and zeros / NaN in its row and column of its unit only; every other bit is that of the run
    # without the NaN
    s, k = RD.nan_at(S, n)
    clean = RD.series(S, T, n, 0, False).to(DEV)
    g0, tau0 = ingest.kendall_counts(clean).cpu(), ingest.kendall_matrices(clean).cpu()
    assert int(g[s, k, k]) == -1 and int(g[s, k].abs().sum()) == 1 and int(g[s, :, k].abs().sum()) == 1
    assert bool(torch.isnan(tau[s, k]).all()) and bool(torch.isnan(tau[s, :, k]).all())
    assert int(torch.isnan(tau).sum()) == 2 * n - 1 and not bool(torch.isnan(tau0).any())
    for got, base in ((g, g0), (tau, tau0)):
        got, base = got.clone(), base.clone()
        got[s, k], got[s, :, k] = base[s, k], base[s, :, k]
        assert torch.equal(_bits(got), _bits(base)), "no other column and no other unit"


@pytest.mark.parametrize("T", [67, 300])
def test_masks_select_the_frames_and_censored_values_are_never_looked_at(T):
    n, num = 9, len(CD.KINDS)
    x, m = RD.series(num, T, n), RD.masks(num, T)
    xd, md = x.to(DEV), m.to(DEV)
    want = KD.host_counts(x, m)
    got = ingest.kendall_counts(xd, sample_mask=md)
    _counts_are(got, want, T)
    tau = ingest.kendall_matrices(xd, sample_mask=md)
    _tau_is(tau, want, T)
    for name in ("none", "one"):
        s = CD.KINDS.index(name)
        assert not bool(got[s].any()) and not bool(_bits(tau[s]).any()), name
    for poison in (float("nan"), float("inf"), 1e30):
        p = x.clone()
        p[~m] = poison
        assert torch.equal(ingest.kendall_counts(p.to(DEV), sample_mask=md), got), poison
        assert torch.equal(_bits(ingest.kendall_matrices(p.to(DEV), sample_mask=md)), _bits(tau)), poison
    every = torch.ones(num, T, dtype=torch.bool, device=DEV)
    assert torch.equal(ingest.kendall_counts(xd, sample_mask=every), ingest.kendall_counts(xd))
    assert torch.equal(_bits(ingest.kendall_matrices(xd, sample_mask=every)), _bits(ingest.kendall_matrices(xd)))


@pytest.mark.parametrize("T,window,stride", WINDOWS)
def test_windows_are_the_call_on_the_unfolded_units(T, window, stride):
    n, num = 9, len(CD.KINDS)
    x, m = RD.series(num, T, n).to(DEV), RD.masks(num, T).to(DEV)
    units = x.unfold(1, window, stride).permute(0, 1, 3, 2).reshape(-1, window, n).contiguous()
    for keep, folded in ((None, None), (m, _unfold(m, window, stride))):
        got = ingest.kendall_counts(x, window=window, stride=stride, sample_mask=keep)
        assert tuple(got.shape) == (units.shape[0], n, n)
        assert torch.equal(got, ingest.kendall_counts(units, sample_mask=folded))
        tau = ingest.kendall_matrices(x, window=window, stride=stride, sample_mask=keep)
        assert torch.equal(_bits(tau), _bits(ingest.kendall_matrices(units, sample_mask=folded)))
    _counts_are(ingest.kendall_counts(x, window=window, stride=stride, sample_mask=m),
                KD.host_counts(x.cpu(), m.cpu(), window, stride), (T, window, stride))


def test_the_compositions_are_bit_for_bit():
    T, n, num = 120, 12, 8
    x = RD.plain(num, T, n).to(DEV)
    y = torch.arange(num) % 2
    m = RD.masks(num, T).to(DEV)
    for kw in (dict(), dict(window=60, stride=30), dict(sample_mask=m), dict(absolute=True)):
        tau = ingest.kendall_matrices(x, **kw)
        assert torch.equal(_bits(ingest.correlation_matrices(x, kendall=True, **kw)), _bits(tau)), kw
    tau = ingest.kendall_matrices(x)
    for shrinkage in (0.1, torch.full((num,), 0.1, device=DEV)):
        for absolute in (False, True):
            got = ingest.correlation_matrices(x, kendall=True, kind="partial", shrinkage=shrinkage, absolute=absolute)
            want = ingest.partial_correlation(tau, shrinkage=shrinkage, absolute=absolute)
            assert torch.equal(_bits(got), _bits(want)), (shrinkage, absolute)
    assert not torch.equal(_bits(tau), _bits(ingest.correlation_matrices(x, rank=True)))
    assert torch.equal(_bits(ingest.correlation_matrices(x, kendall=False)), _bits(ingest.correlation_matrices(x)))
    ds = ingest.from_timeseries(x, y, kendall=True, keep=0.2, measures=True)
    ref = ingest.from_matrices(tau, y, keep=0.2, measures=True)
    assert int(ds.edge_ptr[-1]) > 0
    for name in ("x", "edge_local", "edge_weight", "labels", "edge_ptr_dev"):
        assert torch.equal(getattr(ds, name), getattr(ref, name)), name
    knn = ingest.from_timeseries(x, y, kendall=True, knn=3)
    ref = ingest.from_matrices(tau, y, knn=3)
    for name in ("x", "edge_local", "edge_weight", "labels", "edge_ptr_dev"):
        assert torch.equal(getattr(knn, name), getattr(ref, name)), name


def test_every_run_every_grid_and_every_choice_of_outputs_give_the_same_bits():
    U, T, n = 12, 129, 84
    x = RD.plain(U, T, n).to(DEV)
    g, tau = ingest.kendall_counts(x), ingest.kendall_matrices(x)
    _counts_are(g, KD.host_counts(x.cpu()))
    assert torch.equal(ingest.kendall_counts(x), g) and torch.equal(_bits(ingest.kendall_matrices(x)), _bits(tau))
    ranked = ingest.rank_timeseries(x)

    def both():
        c = torch.empty(U, n, n, dtype=torch.int32, device=DEV)
        t = torch.empty(U, n, n, dtype=torch.float32, device=DEV)
        ingest._call(x.device, "cgnn_ingest_kendall", ranked, U, T, n, 0, *_lib.buf(c), *_lib.buf(t))
        return c, t

    c, t = both()
    assert torch.equal(c, g) and torch.equal(_bits(t), _bits(tau)), "in place is the path with separate counts"
    lib = _lib.load()
    try:
        assert lib.cgnn_set_fused_grid(3) == _lib.CGNN_OK
        few = ingest.kendall_counts(x), ingest.kendall_matrices(x), *both()
    finally:
        lib.cgnn_set_fused_grid(0)
    assert torch.equal(few[0], g) and torch.equal(few[2], g), "6 workgroups"
    assert torch.equal(_bits(few[1]), _bits(tau)) and torch.equal(_bits(few[3]), _bits(tau)), "6 workgroups"
