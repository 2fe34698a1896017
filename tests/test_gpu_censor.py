"""Frame censoring on the device (``sample_mask=`` of connectome_gnn_amd.ingest; csrc/filter.hip, confounds.hip,
timeseries.hip, shrinkage.hip) against the fp64 host statement by compaction (tests/censor_data.py).

Every case has ten subjects, one per mask kind of ``censor_data.KINDS``.

Basis: the kept pattern and the rank are the host's; a kept column is within ``2^-23 max_t |Q_host[:, j]|`` of the host's;
``|Q^T Q - I| <= 2^-22``; rows at censored frames, dropped and pad columns are exactly 0.

Outputs, for every column: ``max_t |out_dev - host| <= c 2^-24 max_K |xc|`` with ``c = 4 x 23.42``: the statement on the
operands the device holds (``censor_data.host_regress32``) is at most 23.42 of ``2^-24 max_K |xc|`` from the fp64 one over
the cases (asserted in tests/test_censor_math.py, never measured against the kernel), and the factor 4 is the margin of
the project's other parity tests.  Censored frames are exactly 0.

Correlations: every unit within ``timeseries_data.atol(L_u, kappa_u)`` of ``host_unit`` of its kept rows, bit-symmetric,
an exact diagonal, and exactly zero where fewer than two frames are kept.  Ledoit-Wolf: within ``4 x 0.5711 x 2^-24 cond``,
0.5711 being the host32 ratio of these units (tests/test_censor_math.py).

Each parity case prints the device's own worst ratio (measured on an MI355X: at most 0.49 of the basis bound and 0.33 of
the Gram bound, 23.43 for the outputs, 0.033 of the correlations' tolerance, 0.5711 for the estimate).
"""
import ctypes
import functools

import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import censor_data as C
from tests import confound_data as D
from tests import filter_data as F
from tests import timeseries_data as TS

pytestmark = pytest.mark.gpu
DEV = "cuda"
C_TOL = 4 * 23.42                                 # 4 x the largest host32 ratio (module docstring)
C_LW = 4 * 0.5711
S = C.S


def _bits(t):
    return t.contiguous().view(torch.int32)


def _band(t_r, hp):
    return dict(t_r=1.0 if t_r is None else t_r, high_pass=hp)


def _device_design(cd, T, t_r, hp):
    """cgnn_ingest_design of the device confounds cd [S, T, q]: the device tensor [S, T, K + q] (cd itself if K == 0)."""
    comps = C.dropped_components(T, t_r, hp)
    K, q = len(comps), cd.shape[2]
    if K == 0:
        return cd
    lib = _lib.load()
    design = torch.full((cd.shape[0], T, K + q), -7.0, dtype=torch.float32, device=DEV)
    assert lib.cgnn_ingest_design_bytes(cd.shape[0], T, K, q) == _lib.nbytes(design)
    _lib.check(lib.cgnn_ingest_design(_lib.ptr(cd), cd.shape[0], T, q, (ctypes.c_int32 * K)(*comps), K, _lib.ptr(design),
                                      _lib.nbytes(design), _lib.stream_ptr()), "cgnn_ingest_design")
    return design


@functools.lru_cache(maxsize=None)
def _regression(case):
    """(host subjects, device design read back, basis, rank, output) of a regression case"""
    T, n, q, t_r, hp = case
    x, c, m = D.frames(S, T, n, q), D.confounds(S, T, q), C.masks(S, T)
    xd, cd, md = x.to(DEV), c.to(DEV), m.to(DEV)
    design = _device_design(cd, T, t_r, hp)
    basis, rank = ingest.confound_basis(design, sample_mask=md)
    w = design.shape[2]
    assert basis.dtype == torch.float32 and tuple(basis.shape) == (S, T, (w + 31) // 32 * 32)
    assert rank.dtype == torch.int32 and tuple(rank.shape) == (S,)
    got = ingest.filter_timeseries(xd, confounds=cd, sample_mask=md, **_band(t_r, hp))
    assert got.dtype == torch.float32 and tuple(got.shape) == (S, T, n) and got.device.type == "cuda"
    assert torch.equal(xd.cpu(), x) and torch.equal(cd.cpu(), c) and torch.equal(md.cpu(), m), "the inputs are left alone"
    return C.regression_subjects(case), design.cpu(), basis.cpu(), rank.cpu(), got.cpu()


@pytest.mark.parametrize("case", C.REGRESSION_CASES)
def test_the_design_is_table_values_then_confounds(case):
    T, n, q, t_r, hp = case
    subjects, design, _, _, _ = _regression(case)
    K = len(C.dropped_components(T, t_r, hp))
    for s, (x, d, keep, kind) in enumerate(subjects):
        assert torch.equal(_bits(design[s][:, K:]), _bits(d[:, K:])), "the confound columns are copies"
        # one rounding of an fp64 value to fp32: the host's cosine and the device's cospi may round apart
        assert float((design[s][:, :K].double() - d[:, :K].double()).abs().max() if K else 0.0) <= 2.0 ** -24
        assert torch.equal(_bits(design[s][:, :K]), _bits(design[0][:, :K])), "the same grid for every subject"


@pytest.mark.parametrize("case", C.REGRESSION_CASES)
def test_the_basis_is_the_hosts_on_the_kept_frames(case):
    subjects, _, basis, rank, _ = _regression(case)
    for s, (x, d, keep, kind) in enumerate(subjects):
        Q, kept, _ = C.host_basis(d, keep)
        q = d.shape[1]
        assert int(rank[s]) == sum(kept), (kind, int(rank[s]), sum(kept))
        assert bool((basis[s][~keep] == 0.0).all()), (kind, "rows at censored frames are exactly 0")
        dropped = [j for j in range(basis.shape[2]) if j >= q or not kept[j]]
        assert bool((basis[s][:, dropped] == 0.0).all()), (kind, "dropped and pad columns are exactly 0")
        K = [j for j in range(q) if kept[j]]
        if not K:
            continue
        dev = basis[s].double()
        assert bool((dev[:, K].abs().max(0).values > 0.0).all()), (kind, "the kept pattern")
        err = (dev[:, K] - Q[:, K]).abs().max(0).values
        bound = 2.0 ** -23 * Q[:, K].abs().max(0).values
        gram = dev[:, K].t() @ dev[:, K] - torch.eye(len(K), dtype=torch.float64)
        print(f"{case} {kind}: rank {int(rank[s])} of Tk = {int(keep.sum())}, max_j |Q_dev - Q_host| / (2^-23 max "
              f"|Q_host_j|) = {float((err / bound).max()):.4f}, |Q^T Q - I| / 2^-22 = {float(gram.abs().max()) * 2 ** 22:.4f}")
        assert bool((err <= bound).all()), (kind, int((err / bound).argmax()))
        assert float(gram.abs().max()) <= 2.0 ** -22, kind


@pytest.mark.parametrize("case", C.REGRESSION_CASES)
def test_parity_with_the_fp64_statement(case):
    T, n, q, t_r, hp = case
    subjects, _, _, _, got = _regression(case)
    for s, (x, d, keep, kind) in enumerate(subjects):
        assert bool((got[s][~keep] == 0.0).all()), (kind, "censored frames are exactly 0")
        r = C.column_ratios(got[s], x, d, keep)
        print(f"{case} {kind}: max over columns of max_t |out - host| / (2^-24 max_K |xc|) = {float(r.max()):.4f} "
              f"(tolerance {C_TOL:.2f})")
        assert bool((r <= C_TOL).all()), (kind, float(r.max()), int(r.argmax()))
    xd, cd, md = D.frames(S, T, n, q).to(DEV), D.confounds(S, T, q).to(DEV), C.masks(S, T).to(DEV)
    again = ingest.filter_timeseries(xd, confounds=cd, sample_mask=md, **_band(t_r, hp))
    assert torch.equal(_bits(again.cpu()), _bits(got)), "two calls, the same bits"
    assert ingest.filter_timeseries(xd, confounds=cd, sample_mask=md, out=xd, **_band(t_r, hp)) is xd
    assert torch.equal(_bits(xd.cpu()), _bits(got)), "out=timeseries gives the out-of-place bits"


@pytest.mark.parametrize("case", [C.REGRESSION_CASES[1], C.REGRESSION_CASES[3]])
def test_masked_centring_and_a_band_without_confounds(case):
    T, n, q, t_r, hp = case
    x, m = D.frames(S, T, n, q), C.masks(S, T)
    xd, md = x.to(DEV), m.to(DEV)
    centred = ingest.filter_timeseries(xd, t_r=t_r, sample_mask=md).cpu()
    band = ingest.filter_timeseries(xd, t_r=t_r, high_pass=hp, sample_mask=md).cpu()
    for s in range(S):
        r0 = C.column_ratios(centred[s], x[s], None, m[s])               # one rounding of the fp64 difference
        assert bool((r0 <= 1.0).all()) and bool((centred[s][~m[s]] == 0.0).all()), (C.KINDS[s], float(r0.max()))
        d = C.host_design(None, T, t_r, hp)
        r = C.column_ratios(band[s], x[s], d, m[s])
        assert bool((r <= C_TOL).all()) and bool((band[s][~m[s]] == 0.0).all()), (C.KINDS[s], float(r.max()))
    work = x.to(DEV)
    assert ingest.filter_timeseries(work, t_r=t_r, sample_mask=md, out=work) is work
    assert torch.equal(_bits(work.cpu()), _bits(centred))


# ---- connectivity ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _connectivity(case):
    T, n, window, stride = case
    ts, m = TS.planted(S, T, n), C.masks(S, T)
    dev, md = ts.to(DEV), m.to(DEV)
    kw = dict(window=window, stride=stride, sample_mask=md)
    r = ingest.correlation_matrices(dev, **kw)
    a = ingest.ledoit_wolf_shrinkage(dev, **kw)
    U = S * TS.num_windows(T, window, stride)
    assert r.dtype == torch.float32 and tuple(r.shape) == (U, n, n) and a.dtype == torch.float64 and tuple(a.shape) == (U,)
    assert torch.equal(dev.cpu(), ts), "the inputs are left alone"
    return C.connectivity_units(case), r.cpu(), a.cpu()


@pytest.mark.parametrize("case", C.CONNECTIVITY_CASES)
def test_correlations_of_the_kept_frames(case):
    units, got, _ = _connectivity(case)
    worst = 0.0
    for u, x in enumerate(units):
        want = C.host_unit(x)
        g = got[u]
        assert torch.equal(_bits(g), _bits(g.t())), (u, "bit-symmetric")
        assert torch.equal(g.diagonal().double(), want.diagonal()), (u, "an exact diagonal")
        if x.shape[0] < 2:
            assert not bool(g.any()), (u, "an empty unit is all zero")
            continue
        tol = TS.atol(x.shape[0], C.unit_kappa(x))
        err = float((g.double() - want).abs().max())
        worst = max(worst, err / tol)
        assert err <= tol, (u, x.shape[0], err, tol)
    print(f"{case}: worst |r - host| / atol(L_u, kappa_u) over {len(units)} units = {worst:.4f}")
    T, n, window, stride = case
    md = C.masks(S, T).to(DEV)
    again = ingest.correlation_matrices(TS.planted(S, T, n).to(DEV), window=window, stride=stride, sample_mask=md,
                                        absolute=True)
    assert torch.equal(_bits(again.cpu()), _bits(got.abs())), "absolute is |r|, and two calls give the same bits"


@pytest.mark.parametrize("case", C.CONNECTIVITY_CASES)
def test_ledoit_wolf_of_the_kept_frames(case):
    units, _, got = _connectivity(case)
    worst = 0.0
    for u, x in enumerate(units):
        want, k = C.host_lw(x), C.cond(x)
        a = float(got[u])
        if x.shape[0] <= 2 or k == 0.0:
            assert a == 0.0, (u, x.shape[0], a)
            continue
        err = abs(a - want)
        worst = max(worst, err / (C.EPS * k))
        assert err <= C_LW * C.EPS * k, (u, x.shape[0], a, want, k)
    print(f"{case}: worst |alpha - host| / (2^-24 cond) = {worst:.4f} (tolerance {C_LW:.4f})")


# ---- properties -------------------------------------------------------------------------------------------------------------
def _everything(xd, cd, md, T, t_r, hp, window, stride):
    """Every output a mask reaches, on device tensors: basis, rank, regression, band, correlations of both kinds, the
    estimate."""
    basis, rank = ingest.confound_basis(cd, sample_mask=md)
    out = [basis, rank, ingest.regress_confounds(xd, cd, sample_mask=md),
           ingest.filter_timeseries(xd, confounds=cd, sample_mask=md, **_band(t_r, hp)),
           ingest.filter_timeseries(xd, t_r=1.0, sample_mask=md)]
    kw = dict(window=window, stride=stride, sample_mask=md)
    out += [ingest.correlation_matrices(xd, **kw), ingest.ledoit_wolf_shrinkage(xd, **kw),
            ingest.correlation_matrices(xd, kind="partial", shrinkage="ledoit_wolf", **kw),
            ingest.correlation_matrices(xd, kind="partial", shrinkage=0.25, absolute=True, **kw)]
    return out


def _same(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        u, v = u.cpu(), v.cpu()
        same = torch.equal(u, v) if u.dtype == torch.int32 else torch.equal(u.view(torch.uint8), v.view(torch.uint8))
        assert same, (what, i)


PROPERTY_CASES = [(33, 65, 24, 2.0, 0.01, 8, 4), (130, 84, 32, 0.72, 0.01, 50, 25)]       # (T, n, q, t_r, hp, window, stride)


@pytest.mark.parametrize("T,n,q,t_r,hp,window,stride", PROPERTY_CASES)
def test_an_all_true_mask_gives_the_bits_of_the_unmasked_calls(T, n, q, t_r, hp, window, stride):
    xd, cd = D.frames(S, T, n, q).to(DEV), D.confounds(S, T, q).to(DEV)
    every = torch.ones(S, T, dtype=torch.bool, device=DEV)
    basis, rank = ingest.confound_basis(cd)
    got = _everything(xd, cd, every, T, t_r, hp, window, stride)
    kw = dict(window=window, stride=stride)
    want = [basis, rank, ingest.regress_confounds(xd, cd), None, ingest.filter_timeseries(xd, t_r=1.0),
            ingest.correlation_matrices(xd, **kw), ingest.ledoit_wolf_shrinkage(xd, **kw),
            ingest.correlation_matrices(xd, kind="partial", shrinkage="ledoit_wolf", **kw),
            ingest.correlation_matrices(xd, kind="partial", shrinkage=0.25, absolute=True, **kw)]
    keep = [i for i, w in enumerate(want) if w is not None]
    _same([got[i] for i in keep], [want[i] for i in keep], "an all-True mask")


@pytest.mark.parametrize("T,n,q,t_r,hp,window,stride", PROPERTY_CASES)
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), 1e30])
def test_censored_values_change_no_bit(T, n, q, t_r, hp, window, stride, poison):
    """Selection, never multiplication."""
    x, c, m = D.frames(S, T, n, q), D.confounds(S, T, q), C.masks(S, T)
    md = m.to(DEV)
    clean = _everything(x.to(DEV), c.to(DEV), md, T, t_r, hp, window, stride)
    bad_x, bad_c = x.clone(), c.clone()
    bad_x[~m] = poison
    bad_c[~m] = -poison
    dirty = _everything(bad_x.to(DEV), bad_c.to(DEV), md, T, t_r, hp, window, stride)
    _same(dirty, clean, f"{poison} in the censored frames")


@pytest.mark.parametrize("T,n,q,t_r,hp,window,stride", PROPERTY_CASES)
def test_every_grid_gives_the_same_bits(T, n, q, t_r, hp, window, stride):
    xd, cd, md = D.frames(S, T, n, q).to(DEV), D.confounds(S, T, q).to(DEV), C.masks(S, T).to(DEV)
    full = _everything(xd, cd, md, T, t_r, hp, window, stride)
    lib = _lib.load()
    for g in (3, 16):
        try:
            assert lib.cgnn_set_fused_grid(g) == _lib.CGNN_OK
            few = _everything(xd, cd, md, T, t_r, hp, window, stride)
        finally:
            lib.cgnn_set_fused_grid(0)
        _same(few, full, f"grid {g}")


def test_an_roi_constant_over_its_kept_frames_is_exactly_zero():
    T, n, q, t_r, hp = C.REGRESSION_CASES[3]
    x, c, m = D.frames(S, T, n, q).clone(), D.confounds(S, T, q), C.masks(S, T)
    col = n // 2
    x[:, :, col] = 101.3
    x[:, :, col][~m] = torch.randn(int((~m).sum()))                     # it varies where nobody looks
    xd, cd, md = x.to(DEV), c.to(DEV), m.to(DEV)
    clean = _regression(C.REGRESSION_CASES[3])[4]
    got = ingest.filter_timeseries(xd, confounds=cd, sample_mask=md, **_band(t_r, hp)).cpu()
    assert bool((got[:, :, col] == 0.0).all())
    others = [i for i in range(n) if i != col]
    assert torch.equal(_bits(got[:, :, others]), _bits(clean[:, :, others])), "columns never mix"
    r = ingest.correlation_matrices(xd, sample_mask=md).cpu()
    assert bool((r[:, col, :] == 0.0).all()) and bool((r[:, :, col] == 0.0).all()), "diagonal included"


def test_a_nan_in_a_kept_frame_stays_in_its_column_of_its_subject():
    T, n, q, t_r, hp = C.REGRESSION_CASES[3]
    x, c, m = D.frames(S, T, n, q).clone(), D.confounds(S, T, q), C.masks(S, T)
    s, col = 2, n - 2                                                   # the random mask
    t = int(m[s].nonzero()[5])
    x[s, t, col] = float("nan")
    clean = _regression(C.REGRESSION_CASES[3])[4]
    got = ingest.filter_timeseries(x.to(DEV), confounds=c.to(DEV), sample_mask=m.to(DEV), **_band(t_r, hp)).cpu()
    assert bool(torch.isnan(got[s, m[s], col]).all()) and bool((got[s, ~m[s], col] == 0.0).all())
    got[s, :, col] = clean[s, :, col]
    assert torch.equal(_bits(got), _bits(clean))


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_a_non_finite_confound_counts_only_in_a_kept_frame(value):
    T, n, q, t_r, hp = C.REGRESSION_CASES[1]
    _, _, _, _, clean = _regression(C.REGRESSION_CASES[1])
    x, c, m = D.frames(S, T, n, q), D.confounds(S, T, q), C.masks(S, T)
    cd, md = c.to(DEV), m.to(DEV)
    basis, rank = ingest.confound_basis(cd, sample_mask=md)
    s = 3                                                               # the phase mask: frame 1 censored, frame 2 kept
    bad = c.clone()
    bad[s, 1, q - 3] = value
    b, r = ingest.confound_basis(bad.to(DEV), sample_mask=md)
    assert torch.equal(_bits(b), _bits(basis)) and torch.equal(r, rank), "in a censored frame it changes nothing"
    bad = c.clone()
    bad[s, 2, q - 3] = value
    b, r = ingest.confound_basis(bad.to(DEV), sample_mask=md)
    want = rank.clone()
    want[s] = -1
    assert torch.equal(r, want)
    assert bool(torch.isnan(b[s][md[s]]).all()) and bool((b[s][~md[s]] == 0.0).all())
    others = [i for i in range(S) if i != s]
    assert torch.equal(_bits(b[others]), _bits(basis[others]))
    got = ingest.filter_timeseries(x.to(DEV), confounds=bad.to(DEV), sample_mask=md, **_band(t_r, hp)).cpu()
    assert bool(torch.isnan(got[s][m[s]]).all()) and bool((got[s][~m[s]] == 0.0).all()), "never 'nothing regressed'"
    assert torch.equal(_bits(got[others]), _bits(clean[others])), "the other subjects keep their bits"


# ---- the composition, through the ABI ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [C.REGRESSION_CASES[2], C.REGRESSION_CASES[4]])
def test_filter_under_a_mask_is_design_basis_regress_through_the_abi(case):
    T, n, q, t_r, hp = case
    lib = _lib.load()
    want = _regression(case)[4]
    xd, cd, md = D.frames(S, T, n, q).to(DEV), D.confounds(S, T, q).to(DEV), C.masks(S, T).to(DEV)
    sp = _lib.stream_ptr()
    design = _device_design(cd, T, t_r, hp)
    w = design.shape[2]
    qpad = (w + 31) // 32 * 32
    basis = torch.full((S, T, qpad), -7.0, dtype=torch.float32, device=DEV)
    rank = torch.full((S,), -7, dtype=torch.int32, device=DEV)
    good = [_lib.ptr(design), S, T, w, _lib.ptr(md), S * T, _lib.ptr(basis), _lib.nbytes(basis), _lib.ptr(rank), 4 * S, sp]
    for name, (p, v) in {"keep NULL": (4, None), "short keep": (5, S * T - 1), "short basis": (7, _lib.nbytes(basis) - 1),
                         "basis misaligned": (6, _lib.ptr(basis) + 8), "T = 1": (2, 1)}.items():
        assert lib.cgnn_ingest_confound_basis_masked(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    torch.cuda.synchronize()
    assert bool((basis == -7.0).all()) and bool((rank == -7).all()), "nothing was written"
    assert lib.cgnn_ingest_confound_basis_masked(*good) == _lib.CGNN_OK
    need = lib.cgnn_ingest_regress_workspace_bytes(S, T, n)
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((S, T, n), -7.0, dtype=torch.float32, device=DEV)
    good = [_lib.ptr(xd), S, T, n, _lib.ptr(md), S * T, _lib.ptr(basis), _lib.nbytes(basis), qpad, _lib.ptr(work), need,
            _lib.ptr(out), _lib.nbytes(out), sp]
    for name, (p, v) in {"keep NULL": (4, None), "short keep": (5, S * T - 1), "short out": (12, _lib.nbytes(out) - 1),
                         "qpad = 0 with a basis": (8, 0), "qpad = 48": (8, 48), "basis NULL": (6, None)}.items():
        assert lib.cgnn_ingest_regress_masked(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "nothing was written"
    assert lib.cgnn_ingest_regress_masked(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(out.cpu()), _bits(want)), "bit for bit"
    empty = ingest.filter_timeseries(xd[:0], confounds=cd[:0], sample_mask=md[:0], **_band(t_r, hp))
    assert tuple(empty.shape) == (0, T, n)


def test_the_in_place_call_allocates_design_basis_and_means_only():
    S_, T, n, q, t_r, hp = 60, 300, 360, 24, 2.0, 0.008
    reps = S_ // S
    xd = D.frames(S, T, n, q).repeat(reps, 1, 1).contiguous().to(DEV)
    cd = D.confounds(S, T, q).repeat(reps, 1, 1).contiguous().to(DEV)
    md = C.masks(S, T).repeat(reps, 1).contiguous().to(DEV)
    ingest.filter_timeseries(xd, confounds=cd, sample_mask=md, out=xd, **_band(t_r, hp))      # (the kernels are loaded)
    lib = _lib.load()
    K = len(C.dropped_components(T, t_r, hp))
    need = lib.cgnn_ingest_design_bytes(S_, T, K, q) + lib.cgnn_ingest_confound_basis_bytes(S_, T, K + q) + \
        lib.cgnn_ingest_regress_workspace_bytes(S_, T, n)
    assert need == S_ * T * 33 * 4 + S_ * T * 64 * 4 + S_ * n * 8
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ingest.filter_timeseries(xd, confounds=cd, sample_mask=md, out=xd, **_band(t_r, hp))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < need + 2 ** 20 and need < 4 * S_ * T * n // 3, (peak, need)


# ---- the point of the feature -----------------------------------------------------------------------------------------------
def test_censoring_removes_an_artefact_that_no_confound_carries():
    """Two ROIs share 20 spiky frames and nothing else; the mask is ``confound 0 == 0``."""
    x, c = D.spike_pair()
    num, n = x.shape[0], x.shape[2]
    dev = x.to(DEV)
    md = (c[:, :, 0] == 0).contiguous().to(DEV)
    raw = ingest.correlation_matrices(dev).cpu()
    r = ingest.correlation_matrices(dev, sample_mask=md).cpu()
    for s in range(num):
        print(f"subject {s}: r_01 {float(raw[s, 0, 1]):.4f} without the mask, {float(r[s, 0, 1]):.4f} with it "
              f"(host: {F.corr01(x[s]):.4f}, {F.corr01(x[s][md[s].cpu()]):.4f})")
        assert float(raw[s, 0, 1]) > 0.9 and abs(float(r[s, 0, 1])) < 0.2
    y = torch.arange(num, dtype=torch.long) % 2
    before = ingest.from_timeseries(dev, y, keep=0.25)
    ds = ingest.from_timeseries(dev, y, keep=0.25, sample_mask=md)
    assert ds.x.shape == (num, n, 1) and int(ds.edge_ptr[-1]) > 0

    def has_edge(d, s):
        lo, hi = int(d.edge_ptr[s]), int(d.edge_ptr[s + 1])
        e = d.edge_local[:, lo:hi].cpu()
        return bool(((e[0] == 0) & (e[1] == 1)).any()) or bool(((e[0] == 1) & (e[1] == 0)).any())

    for s in range(num):
        assert has_edge(before, s) and not has_edge(ds, s), s
    want = ingest.from_matrices(ingest.correlation_matrices(dev, sample_mask=md), y, keep=0.25)
    assert torch.equal(ds.edge_local, want.edge_local) and torch.equal(_bits(ds.edge_weight), _bits(want.edge_weight))
    none = torch.zeros_like(md)
    empty = ingest.from_timeseries(dev, y, keep=0.25, sample_mask=none)
    assert int(empty.edge_ptr[-1]) == 0, "no kept frame: graphs without edges"


# ---- the masked and the unmasked entry point of a pair check alike ------------------------------------------------------------
def test_pairs_refuse_alike():
    """Each pair shares one host body: a bad argument is CGNN_EINVAL from both entry points, before any launch, and
    the good arguments are CGNN_OK from both (an all-True mask on the masked side)."""
    lib = _lib.load()
    S_, T, n, q, qpad = 2, 8, 5, 3, 32
    gen = torch.Generator().manual_seed(5)
    ts = torch.randn(S_, T, n, generator=gen).to(DEV)
    conf = torch.randn(S_, T, q, generator=gen).to(DEV)
    keep = torch.ones(S_, T, dtype=torch.bool, device=DEV)

    def fresh(*shape, dtype=torch.float32):
        return torch.full(shape, -7, dtype=dtype, device=DEV)

    stats, mats, alpha = fresh(S_, n, 2), fresh(S_, n, n), fresh(S_, dtype=torch.float64)
    basis, rank, out = fresh(S_, T, qpad), fresh(S_, dtype=torch.int32), fresh(S_, T, n)
    work = torch.empty(lib.cgnn_ingest_regress_workspace_bytes(S_, T, n), dtype=torch.uint8, device=DEV)
    shape = dict(S=S_, T=T, n=n, window=0, stride=0, keep=_lib.ptr(keep), keep_bytes=S_ * T, sp=_lib.stream_ptr())

    def buf(name, t):
        return {name: _lib.ptr(t), name + "_bytes": _lib.nbytes(t)}

    # name: (the masked entry's arguments in order, those the unmasked one does not take, input, output, what the call
    # writes, the good arguments)
    pairs = {
        "cgnn_ingest_corr": ("ts S T n window stride absolute keep keep_bytes stats stats_bytes out out_bytes sp",
                             "keep keep_bytes", "ts", "out", (stats, mats),
                             dict(shape, ts=_lib.ptr(ts), absolute=0, **buf("stats", stats), **buf("out", mats))),
        "cgnn_ingest_shrinkage": ("ts S T n window stride keep keep_bytes stats stats_bytes matrices matrices_bytes "
                                  "alpha alpha_bytes sp", "keep keep_bytes stats_bytes matrices_bytes", "ts", "alpha",
                                  (alpha,),
                                  dict(shape, ts=_lib.ptr(ts), **buf("stats", stats), **buf("matrices", mats),
                                       **buf("alpha", alpha))),
        "cgnn_ingest_confound_basis": ("ts S T n keep keep_bytes basis basis_bytes rank rank_bytes sp",
                                       "keep keep_bytes", "ts", "basis", (basis, rank),
                                       dict(shape, ts=_lib.ptr(conf), n=q, **buf("basis", basis), **buf("rank", rank))),
        "cgnn_ingest_regress": ("ts S T n keep keep_bytes basis basis_bytes qpad work work_bytes out out_bytes sp",
                                "keep keep_bytes", "ts", "out", (out,),
                                dict(shape, ts=_lib.ptr(ts), qpad=qpad, **buf("basis", basis), **buf("work", work),
                                     **buf("out", out))),
    }
    for name, (order, masked_only, src, dst, outs, good) in pairs.items():
        def both(change):
            args = dict(good, **change)
            masked = [args[k] for k in order.split()]
            plain = [args[k] for k in order.split() if k not in masked_only.split()]
            return getattr(lib, name)(*plain), getattr(lib, name + "_masked")(*masked)

        bad = {"T = 1": dict(T=1), "a null input": {src: None}, "a null output": {dst: None},
               "a negative byte count": {dst + "_bytes": -1}, "an input offset by one byte": {src: good[src] + 1},
               "an output one float short": {dst + "_bytes": good[dst + "_bytes"] - 4}}
        if "window" in order.split():
            bad.update({"window > T": dict(window=T + 1, stride=1), "stride = 0": dict(window=4, stride=0)})
        if name == "cgnn_ingest_regress":
            bad["qpad = 48"] = dict(qpad=48)
        for what, change in bad.items():
            assert both(change) == (_lib.CGNN_EINVAL, _lib.CGNN_EINVAL), (name, what)
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in outs), (name, "a refused call wrote")
        assert both({}) == (_lib.CGNN_OK, _lib.CGNN_OK), name
