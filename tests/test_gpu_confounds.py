"""connectome_gnn_amd.ingest.confound_basis / regress_confounds / filter_timeseries(confounds=) (csrc/confounds.hip,
csrc/filter.hip) on the device, against the fp64 host statement (tests/confound_data.py).

Basis: the kept pattern and the rank are the host's; a kept column is within ``2^-23 max_t |Q_host[:, j]|`` of the host's
(one rounding to fp32, which the device's fp64 summation order may flip); dropped and pad columns are exactly 0.

Output, for every column: ``max_t |out_dev - host_regress| <= c 2^-24 max_t |xc|``.  ``c`` is measured on the host, never
against the kernel: the statement evaluated on the operands the device holds (``confound_data.host_regress32``: fp32
``xc``, fp32 ``Q``, the host's fp32 matmul) is at most 11.09 of ``2^-24 max |xc|`` away from the fp64 one over the cases
(asserted in tests/test_confound_math.py), and a factor 4 covers the device's summation order and its own basis, as in
tests/test_gpu_filter.py: ``c = 44.4``, that is ``2.6e-6 max |xc|``, while a confound left in moves a column by more
than ``1e-3 max |xc|`` (asserted there too).  Each parity case prints the device's own ratio (measured on an MI355X: at
most 11.09 for the output, at most 0.45 of the basis bound, 16.2 of 108.2 for the composition).
"""
import functools

import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import confound_data as D
from tests import filter_data as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
C_TOL = 4 * 11.09                                 # 4 x the largest host32 ratio (module docstring)
C_FILTER = 4 * 15.95                              # tests/test_gpu_filter.py's, for the composition


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(T, n, S, q, near):
    """(host frames, host confounds, device basis, rank and result read back)"""
    x, c = D.frames(S, T, n, q, 0, near), D.confounds(S, T, q, 0, near)
    basis, rank = ingest.confound_basis(c.to(DEV))
    qpad = (q + 31) // 32 * 32
    assert basis.dtype == torch.float32 and tuple(basis.shape) == (S, T, qpad) and basis.device.type == "cuda"
    assert rank.dtype == torch.int32 and tuple(rank.shape) == (S,)
    got = ingest.regress_confounds(x.to(DEV), c.to(DEV))
    assert got.dtype == torch.float32 and got.device.type == "cuda" and tuple(got.shape) == (S, T, n)
    return x, c, basis.cpu(), rank.cpu(), got.cpu()


def _check(got, x, c, what, tol=C_TOL):
    """every column of one subject within the tolerance; returns the largest ratio"""
    r = D.column_ratios(got, x, c)
    worst = float(r.max())
    print(f"{what}: max over columns of max_t |out - host| / (2^-24 max_t |xc|) = {worst:.4f} (tolerance {tol:.2f})")
    assert bool((r <= tol).all()), (what, worst, int(r.argmax()))
    return worst


@pytest.mark.parametrize("T,n,S,q,near", D.all_cases())
def test_the_basis_is_the_hosts(T, n, S, q, near):
    x, c, basis, rank, _ = _case(T, n, S, q, near)
    for s in range(S):
        Q, kept, _ = D.host_basis(c[s])
        assert int(rank[s]) == sum(kept)
        dev = basis[s].double()
        dropped = [j for j in range(basis.shape[2]) if j >= q or not kept[j]]
        assert bool((basis[s][:, dropped] == 0.0).all()), "dropped and pad columns are exactly 0"
        K = [j for j in range(q) if kept[j]]
        assert bool((dev[:, K].abs().max(0).values > 0.0).all()), "the kept pattern"
        err = (dev[:, K] - Q[:, K]).abs().max(0).values
        bound = 2.0 ** -23 * Q[:, K].abs().max(0).values
        print(f"T={T} q={q} subject {s}: rank {int(rank[s])}, max_j |Q_dev - Q_host| / (2^-23 max |Q_host_j|) = "
              f"{float((err / bound).max()):.4f}")
        assert bool((err <= bound).all()), (s, int((err / bound).argmax()))
        gram = dev[:, K].t() @ dev[:, K] - torch.eye(len(K), dtype=torch.float64)
        assert float(gram.abs().max()) <= 2.0 ** -22
    again, rank2 = ingest.confound_basis(c.to(DEV))
    assert torch.equal(_bits(again.cpu()), _bits(basis)) and torch.equal(rank2.cpu(), rank), "two calls, the same bits"


@pytest.mark.parametrize("T,n,S,q,near", D.all_cases())
def test_parity_with_the_fp64_statement(T, n, S, q, near):
    x, c, _, _, got = _case(T, n, S, q, near)
    for s in range(S):
        _check(got[s], x[s], c[s], f"T={T} n={n} q={q}{' near-copy' if near else ''} subject {s}")
    again = ingest.regress_confounds(x.to(DEV), c.to(DEV))
    assert torch.equal(_bits(again.cpu()), _bits(got)), "two calls, the same bits"


@pytest.mark.parametrize("T,n,S,q,near", D.all_cases())
def test_in_place_gives_the_bits_of_out_of_place(T, n, S, q, near):
    x, c, _, _, want = _case(T, n, S, q, near)
    dev, cd = x.to(DEV), c.to(DEV)
    assert ingest.regress_confounds(dev, cd, out=dev) is dev
    assert torch.equal(_bits(dev.cpu()), _bits(want))
    other = torch.full_like(dev, -7.0)
    src = x.to(DEV)
    assert ingest.regress_confounds(src, cd, out=other) is other
    assert torch.equal(_bits(other.cpu()), _bits(want))
    assert torch.equal(src.cpu(), x) and torch.equal(cd.cpu(), c), "the inputs are left as they are"


@pytest.mark.parametrize("T,n,q", [(33, 65, 24), (300, 360, 64)])
def test_every_grid_gives_the_same_bits(T, n, q):
    S = 7                                                             # every workgroup walks several subjects and items
    x, c = D.frames(S, T, n, q), D.confounds(S, T, q)
    dev, cd = x.to(DEV), c.to(DEV)
    basis, rank = ingest.confound_basis(cd)
    full = ingest.regress_confounds(dev, cd)
    lib = _lib.load()
    for g in (3, 16):
        try:
            assert lib.cgnn_set_fused_grid(g) == _lib.CGNN_OK
            b, r = ingest.confound_basis(cd)
            few = ingest.regress_confounds(dev, cd)
        finally:
            lib.cgnn_set_fused_grid(0)
        assert torch.equal(_bits(b), _bits(basis)) and torch.equal(r, rank), g
        assert torch.equal(_bits(few), _bits(full)), g
    got = full.cpu()
    for s in (0, 6):
        assert int(rank[s]) == D.host_rank(c[s])
        _check(got[s], x[s], c[s], f"T={T} n={n} q={q} of 7 subjects: subject {s}")


@pytest.mark.parametrize("T,n,S,q,near", [D.all_cases()[1], D.all_cases()[3], D.all_cases()[5]])
def test_a_constant_roi_gives_exact_zeros(T, n, S, q, near):
    x, c, _, _, clean = _case(T, n, S, q, near)
    flat = x.clone()
    flat[:, :, n // 2] = 101.3
    flat[S - 1, :, 0] = -0.1
    got = ingest.regress_confounds(flat.to(DEV), c.to(DEV)).cpu()
    assert bool((got[:, :, n // 2] == 0.0).all()) and bool((got[S - 1, :, 0] == 0.0).all())
    others = [i for i in range(1, n) if i != n // 2]
    assert torch.equal(_bits(got[:, :, others]), _bits(clean[:, :, others])), "columns never mix"


def test_a_nan_in_an_roi_stays_in_its_column_of_its_subject():
    for case in (D.all_cases()[3], D.all_cases()[4]):
        T, n, S, q, near = case
        x, c, _, _, clean = _case(*case)
        bad = x.clone()
        bad[1, T // 2, n - 2] = float("nan")
        got = ingest.regress_confounds(bad.to(DEV), c.to(DEV)).cpu()
        assert not bool(torch.isfinite(got[1, :, n - 2]).any()), case
        got[1, :, n - 2] = clean[1, :, n - 2]
        assert torch.equal(_bits(got), _bits(clean)), case


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_a_non_finite_confound_makes_its_subject_nan(value):
    T, n, S, q, near = D.all_cases()[3]
    x, c, basis, rank, clean = _case(T, n, S, q, near)
    bad = c.clone()
    bad[1, T - 1, q - 3] = value
    b, r = ingest.confound_basis(bad.to(DEV))
    assert r.cpu().tolist() == [int(rank[0]), -1]
    assert bool(torch.isnan(b[1]).all()) and torch.equal(_bits(b[0].cpu()), _bits(basis[0]))
    got = ingest.regress_confounds(x.to(DEV), bad.to(DEV)).cpu()
    assert bool(torch.isnan(got[1]).all()), "never 'nothing regressed'"
    assert torch.equal(_bits(got[0]), _bits(clean[0])), "the other subject keeps its bits"


def _band(t_r, hp, lp):
    return dict(t_r=t_r, high_pass=hp, low_pass=lp)


@pytest.mark.parametrize("T,n,S,q,t_r,hp,lp", D.BANDS)
def test_filter_with_confounds_is_the_composition(T, n, S, q, t_r, hp, lp):
    x, c = D.frames(S, T, n, q), D.confounds(S, T, q)
    dev, cd = x.to(DEV), c.to(DEV)
    band = _band(t_r, hp, lp)
    plain = ingest.filter_timeseries(dev, **band)
    two = ingest.regress_confounds(plain, ingest.filter_timeseries(cd, **band))
    got = ingest.filter_timeseries(dev, confounds=cd, **band)
    assert torch.equal(_bits(got), _bits(two)), "the two-call composition, bit for bit"
    assert torch.equal(dev.cpu(), x) and torch.equal(cd.cpu(), c), "the inputs are left as they are"
    work = x.to(DEV)
    assert ingest.filter_timeseries(work, confounds=cd, out=work, **band) is work
    assert torch.equal(_bits(work), _bits(got)), "in place"
    assert torch.equal(_bits(ingest.filter_timeseries(dev, confounds=None, **band)), _bits(plain))
    got = got.cpu()
    for s in range(S):
        want = D.host_filter_regress(x[s], c[s], t_r, hp, lp)
        scale = F.centred(x[s]).abs().max(0).values
        r = (got[s].double() - want).abs().max(0).values / (D.EPS * scale)
        print(f"T={T} n={n} q={q} subject {s}: filter + regress, worst ratio {float(r.max()):.4f} "
              f"(tolerance {C_FILTER + C_TOL:.2f})")
        assert bool((r <= C_FILTER + C_TOL).all()), (s, float(r.max()))


def test_abi_runs_what_python_runs_and_refuses_before_any_launch():
    lib = _lib.load()
    T, n, S, q, near = D.all_cases()[3]
    x, c, basis_want, rank_want, want = _case(T, n, S, q, near)
    dev, cd = x.to(DEV), c.to(DEV)
    sp = _lib.stream_ptr()
    nb = lib.cgnn_ingest_confound_basis_bytes(S, T, q)
    assert nb == S * T * 32 * 4
    basis = torch.full((S, T, 32), -7.0, dtype=torch.float32, device=DEV)
    rank = torch.full((S,), -7, dtype=torch.int32, device=DEV)
    good = [_lib.ptr(cd), S, T, q, _lib.ptr(basis), nb, _lib.ptr(rank), 4 * S, sp]
    bad = {"short basis": (5, nb - 1), "short rank": (7, 4 * S - 1), "confounds NULL": (0, None), "basis NULL": (4, None),
           "rank NULL": (6, None), "basis misaligned": (4, _lib.ptr(basis) + 8), "rank misaligned": (6, _lib.ptr(rank) + 2),
           "q = 0": (3, 0), "q = 65": (3, 65), "q = 33 in a basis of 32": (3, 33), "T = 1": (2, 1), "S < 0": (1, -1)}
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_confound_basis(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    assert lib.cgnn_ingest_confound_basis(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK           # S == 0
    torch.cuda.synchronize()
    assert bool((basis == -7.0).all()) and bool((rank == -7).all()), "nothing was written"
    assert lib.cgnn_ingest_confound_basis(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(basis.cpu()), _bits(basis_want)) and torch.equal(rank.cpu(), rank_want)

    need = lib.cgnn_ingest_regress_workspace_bytes(S, T, n)
    assert need == S * n * 8
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((S, T, n), -7.0, dtype=torch.float32, device=DEV)
    good = [_lib.ptr(dev), S, T, n, _lib.ptr(basis), nb, 32, _lib.ptr(work), need, _lib.ptr(out), _lib.nbytes(out), sp]
    bad = {"short basis": (5, nb - 1), "short work": (8, need - 1), "short out": (10, _lib.nbytes(out) - 1),
           "ts NULL": (0, None), "basis NULL": (4, None), "work NULL": (7, None), "out NULL": (9, None),
           "basis misaligned": (4, _lib.ptr(basis) + 8), "work misaligned": (7, _lib.ptr(work) + 8),
           "out misaligned": (9, _lib.ptr(out) + 2), "qpad = 48": (6, 48), "qpad = 64 on a basis of 32": (6, 64),
           "qpad = 0": (6, 0), "T = 1": (2, 1), "S < 0": (1, -1), "n = 0": (3, 0)}
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_regress(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    assert lib.cgnn_ingest_regress(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK                  # S == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "nothing was written"
    assert lib.cgnn_ingest_regress(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(out.cpu()), _bits(want))
    good[9], good[10] = _lib.ptr(dev), _lib.nbytes(dev)                                           # out == ts
    assert lib.cgnn_ingest_regress(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(dev.cpu()), _bits(want))
    empty, none = x[:0].to(DEV), c[:0].to(DEV)
    assert tuple(ingest.regress_confounds(empty, none).shape) == (0, T, n)
    b, r = ingest.confound_basis(none)
    assert tuple(b.shape) == (0, T, 32) and tuple(r.shape) == (0,)


def test_no_cohort_sized_temporaries_beyond_the_basis():
    S, T, n, q = 64, 300, 360, 24
    dev = D.frames(2, T, n, q).repeat(S // 2, 1, 1).contiguous().to(DEV)
    cd = D.confounds(2, T, q).repeat(S // 2, 1, 1).contiguous().to(DEV)
    ingest.regress_confounds(dev, cd)                                 # (the kernels are loaded)
    lib = _lib.load()
    need = lib.cgnn_ingest_confound_basis_bytes(S, T, q) + lib.cgnn_ingest_regress_workspace_bytes(S, T, n)
    assert need == S * T * 32 * 4 + S * n * 8
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ingest.regress_confounds(dev, cd, out=dev)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < need + 2 ** 20 and need < 4 * S * T * n // 8, (peak, need)


def test_a_shared_motion_artefact_no_longer_makes_an_edge():
    """The point of the feature: two ROIs that share a spiky confound and nothing else."""
    x, c = D.spike_pair()
    S, n = x.shape[0], x.shape[2]
    dev, cd = x.to(DEV), c.to(DEV)
    raw = ingest.correlation_matrices(dev).cpu()
    clean = ingest.regress_confounds(dev, cd)
    r = ingest.correlation_matrices(clean).cpu()
    for s in range(S):
        print(f"subject {s}: r_01 {float(raw[s, 0, 1]):.4f} before, {float(r[s, 0, 1]):.4f} after "
              f"(host: {F.corr01(x[s]):.4f}, {F.corr01(D.host_regress(x[s], c[s])):.4f})")
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
