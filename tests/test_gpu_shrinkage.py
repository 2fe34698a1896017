"""connectome_gnn_amd.ingest.ledoit_wolf_shrinkage (csrc/shrinkage.hip), the per-unit shrinkage of
``partial_correlation`` (csrc/partial.hip) and ``shrinkage="ledoit_wolf"`` on the device, against the fp64 host
statement (tests/shrinkage_data.py).

Tolerance of the estimate: ``|a_dev - a_host| <= c 2^-24 cond`` with ``cond = (B + F) / (L O)``, the factor by which the
quotient magnifies a relative error of its two sums (0 where the answer is exactly 0).  ``c`` is measured on the host,
never against the kernel: the statement evaluated on fp32 ``z`` and ``R`` (``shrinkage_data.host_lw32``) is at most
0.4508 of ``2^-24 cond`` away from the fp64 one over the parity cases below (the planted unit 2 of 300 x 84; asserted in
tests/test_shrinkage_math.py), and a factor 4 covers the device's ``R``, which differs from the host's fp32 product in
summation order: ``c = 1.8032``.  Each parity case prints the device's own ratio.
"""
import functools

import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib, ingest
from connectome_gnn_amd.resident import ResidentDataLoader
from tests import partial_data as P
from tests import shrinkage_data as D
from tests import timeseries_data as TS

pytestmark = pytest.mark.gpu
DEV = "cuda"
C_TOL = 4 * 0.4508                                # 4 x the largest host32 ratio (module docstring)
C_PARTIAL = 1.16                                  # tests/test_gpu_partial.py's bound on the inverse


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@functools.lru_cache(maxsize=None)
def _case(kind, L, n, S):
    """(host frames, device estimate read back)"""
    x = D.frames(kind, S, L, n)
    got = ingest.ledoit_wolf_shrinkage(x.to(DEV))
    assert got.dtype == torch.float64 and got.device.type == "cuda" and tuple(got.shape) == (S,)
    return x, got.cpu()


def _check_unit(got, x, what, want_of=None):
    """|got - host_lw(x)| <= c 2^-24 cond(x); where cond is 0 the answer is exact."""
    want, k = D.host_lw(x if want_of is None else want_of), D.cond(x if want_of is None else want_of)
    err, tol = abs(got - want), C_TOL * D.EPS * k
    print(f"{what}: a {want:.6f}, cond {k:.3f}, error {err:.3e}, ratio err / (2^-24 cond) "
          f"{err / (D.EPS * k) if k else 0.0:.4f}, tol {tol:.3e}")
    assert err <= tol, (what, got, want, err, tol)


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("L,n,S", D.CASES)
def test_parity_with_the_fp64_statement(L, n, S, kind):
    x, got = _case(kind, L, n, S)
    for s in range(S):
        _check_unit(float(got[s]), x[s], f"{kind} L={L} n={n} unit {s}")
    again = ingest.ledoit_wolf_shrinkage(x.to(DEV))
    assert torch.equal(_bits(again.cpu()), _bits(got)), "two calls, the same bits"


def test_the_clip_gives_exactly_one():
    assert D.ratio(D.clipped()[0]) > 1.0
    got = ingest.ledoit_wolf_shrinkage(D.clipped().to(DEV)).cpu()
    assert got.tolist() == [1.0]


@pytest.mark.parametrize("kind", D.KINDS)
def test_one_roi_and_two_frames_give_exactly_zero(kind):
    assert _case(kind, 7, 1, 2)[1].tolist() == [0.0, 0.0]
    assert _case(kind, 2, 5, 3)[1].tolist() == [0.0, 0.0, 0.0]
    x = torch.full((2, 9, 4), 2.5)
    x[:, :, 2] = D.frames(kind, 2, 9, 1)[:, :, 0]                    # one ROI that is not constant
    assert ingest.ledoit_wolf_shrinkage(x.to(DEV)).cpu().tolist() == [0.0, 0.0]


@pytest.mark.parametrize("L,n,S", [(40, 65, 2), (66, 97, 3), (300, 84, 3)])
def test_a_constant_column_changes_nothing_beyond_p(L, n, S):
    x, got = _case("planted", L, n, S)
    others = [i for i in range(n) if i != n // 2]
    less = x[:, :, others].contiguous()
    got_less = ingest.ledoit_wolf_shrinkage(less.to(DEV)).cpu()
    for s in range(S):
        _check_unit(float(got[s]), x[s], f"L={L} n={n} unit {s} against the statement without the column", less[s])
        _check_unit(float(got_less[s]), less[s], f"L={L} n={n - 1} unit {s}: the column deleted")


def test_a_nan_frame_gives_a_nan_for_its_own_unit_only():
    x, want = _case("planted", 66, 97, 3)
    bad = x.clone()
    bad[1, 40] = float("nan")
    got = ingest.ledoit_wolf_shrinkage(bad.to(DEV)).cpu()
    assert bool(torch.isnan(got[1])) and torch.equal(_bits(got[[0, 2]]), _bits(want[[0, 2]]))
    # in windows: only the windows that hold the frame
    T, L, st = 50, 20, 10                                             # windows [0, 20) [10, 30) [20, 40) [30, 50)
    ts = D.planted(2, T, 20).clone()
    clean = ingest.ledoit_wolf_shrinkage(ts.to(DEV), window=L, stride=st).cpu()
    ts[1, 25, 3] = float("nan")
    got = ingest.ledoit_wolf_shrinkage(ts.to(DEV), window=L, stride=st).cpu()
    assert torch.isnan(got).tolist() == [False] * 4 + [False, True, True, False]
    keep = ~torch.isnan(got)
    assert torch.equal(_bits(got[keep]), _bits(clean[keep]))


def test_many_units_walk_the_grid_stride():
    ts = D.planted(40, 300, 84, seed=3)
    dev = ts.to(DEV)
    lib = _lib.load()
    try:
        assert lib.cgnn_set_fused_grid(3) == _lib.CGNN_OK
        few = ingest.ledoit_wolf_shrinkage(dev)
    finally:
        lib.cgnn_set_fused_grid(0)
    full = ingest.ledoit_wolf_shrinkage(dev)
    assert torch.equal(_bits(few), _bits(full))
    got = full.cpu()
    for s in range(0, 40, 13):
        _check_unit(float(got[s]), ts[s], f"40 units: unit {s}")


@pytest.mark.parametrize("n", [20, 84])
def test_windows_are_the_per_window_calls(n):
    T, L, st = 50, 20, 7
    ts = D.planted(3, T, n)
    dev = ts.to(DEV)
    W = TS.num_windows(T, L, st)
    got = ingest.ledoit_wolf_shrinkage(dev, window=L, stride=st)
    assert tuple(got.shape) == (3 * W,) and not bool(torch.isnan(got).any())
    for w in range(W):
        part = ingest.ledoit_wolf_shrinkage(dev[:, w * st:w * st + L].contiguous())
        assert torch.equal(_bits(got[w::W]), _bits(part)), w
    _check_unit(float(got[W + 2]), ts[1, 2 * st:2 * st + L], "subject 1, window 2")


# ---- k_partial with a shrinkage per unit -------------------------------------------------------------------------
@pytest.mark.parametrize("T,n", [(40, 5), (66, 33), (300, 84)])
def test_a_constant_tensor_has_the_bits_of_the_scalar_call(T, n):
    R = P.cohort(3, T, n).to(DEV)
    for a in (0.1, 0.0, 1.0):
        want = ingest.partial_correlation(R, shrinkage=a)
        for dtype in (torch.float64, torch.float32):                  # (0.1 in float32 is another number)
            each = torch.full([3], a, dtype=dtype, device=DEV)
            got = ingest.partial_correlation(R, shrinkage=each)
            if dtype == torch.float64 or a != 0.1:
                assert torch.equal(_bits(got), _bits(want)), (a, dtype)
            else:
                assert torch.equal(_bits(got), _bits(ingest.partial_correlation(R, shrinkage=float(each[0])))), a
        absolute = ingest.partial_correlation(R, shrinkage=torch.full([3], a, dtype=torch.float64, device=DEV),
                                              absolute=True)
        assert torch.equal(_bits(absolute), _bits(want.abs())), a


@pytest.mark.parametrize("T,n", [(40, 5), (66, 33), (300, 84)])
def test_each_unit_has_the_bits_of_the_scalar_call_at_its_own_value(T, n):
    R = P.cohort(3, T, n).to(DEV)
    values = [0.05, 0.3, 0.7]
    got = ingest.partial_correlation(R, shrinkage=torch.tensor(values, dtype=torch.float64, device=DEV))
    for u, a in enumerate(values):
        assert torch.equal(_bits(got[u]), _bits(ingest.partial_correlation(R, shrinkage=a)[u])), u


@pytest.mark.parametrize("T,n", [(40, 5), (66, 33), (300, 84)])
def test_a_unit_with_a_value_outside_the_unit_interval_is_all_nan_and_alone(T, n):
    R = P.cohort(3, T, n).to(DEV)
    want = ingest.partial_correlation(R, shrinkage=0.1)
    for bad in (1.5, -0.1, float("nan"), float("inf")):
        got = ingest.partial_correlation(R, shrinkage=torch.tensor([0.1, bad, 0.1], dtype=torch.float64, device=DEV))
        assert bool(torch.isnan(got[1]).all()), bad
        assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[2]), _bits(want[2])), bad
    # in place too: the refused unit's correlations are overwritten by NaN, not left
    ts = TS.recipe(3, T, n).to(DEV)
    got = ingest.correlation_matrices(ts, kind="partial",
                                      shrinkage=torch.tensor([0.1, 1.5, 0.1], dtype=torch.float64, device=DEV))
    assert bool(torch.isnan(got[1]).all()) and not bool(torch.isnan(got[[0, 2]]).any())


# ---- end to end --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,n,S", [(9, 33, 3), (66, 97, 3), (300, 84, 3), (120, 360, 2)])
def test_the_estimator_by_name_equals_the_two_step_call(L, n, S):
    ts = D.planted(S, L, n)
    dev = ts.to(DEV)
    alpha = ingest.ledoit_wolf_shrinkage(dev)
    for absolute in (False, True):
        one = ingest.correlation_matrices(dev, kind="partial", shrinkage="ledoit_wolf", absolute=absolute)
        two = ingest.partial_correlation(ingest.correlation_matrices(dev), shrinkage=alpha, absolute=absolute)
        assert torch.equal(_bits(one), _bits(two)), absolute
    # the inverse's error apart from the estimate's and the correlation's: the host statement of the device's own
    # correlations at the device's own alpha
    R = ingest.correlation_matrices(dev).cpu()
    got = one.cpu()
    for s, a in enumerate(alpha.cpu().tolist()):
        assert 0.0 < a < 1.0
        kappa = P.kappa_of(R[s:s + 1], a)
        assert kappa <= P.KAPPA_CAP
        err = float((got[s].double() - P.host_partial(R[s], a, absolute=True)).abs().max())
        tol = P.tol(kappa, C_PARTIAL)
        print(f"L={L} n={n} unit {s}: alpha {a:.4f}, kappa {kappa:.1f}, max error {err:.3e}, tol {tol:.3e}")
        assert err <= tol, (s, err, tol)
    mid = n // 2                                                      # the planted constant column is excluded
    assert torch.equal(got[:, mid], torch.zeros(S, n)) and torch.equal(got[:, :, mid], torch.zeros(S, n))


def test_short_windows_are_accepted_with_the_estimator():
    T, L, n = 60, 20, 33
    dev = D.planted(3, T, n).to(DEV)
    with pytest.raises(ValueError, match="give shrinkage > 0"):
        ingest.correlation_matrices(dev, window=L, kind="partial")
    got = ingest.correlation_matrices(dev, window=L, kind="partial", shrinkage="ledoit_wolf")
    assert tuple(got.shape) == (9, n, n) and not bool(torch.isnan(got).any())
    alpha = ingest.ledoit_wolf_shrinkage(dev, window=L)
    assert bool(((alpha > 0) & (alpha < 1)).all())
    assert torch.equal(_bits(got), _bits(ingest.partial_correlation(ingest.correlation_matrices(dev, window=L),
                                                                    shrinkage=alpha)))


def test_no_cohort_sized_temporaries():
    """Above the resident frames only the output, the statistics, the estimate and the partial workspace (one slab per
    workgroup) are allocated."""
    U, T, n = 64, 120, 360
    dev = D.planted(2, T, n).repeat(U // 2, 1, 1).contiguous().to(DEV)
    ingest.correlation_matrices(dev, kind="partial", shrinkage="ledoit_wolf")      # (the kernels are loaded)
    need = _lib.load().cgnn_ingest_partial_workspace_bytes(U, n)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ingest.correlation_matrices(dev, kind="partial", shrinkage="ledoit_wolf")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert tuple(out.shape) == (U, n, n)
    small = 8 * U * n + 8 * U
    assert 4 * U * n * n <= peak < 4 * U * n * n + small + need + 2 ** 20, (peak, 4 * U * n * n, small, need)
    assert torch.equal(_bits(out[:2]), _bits(out[2:4]))


def test_abi_runs_what_python_runs_and_refuses_before_any_launch():
    lib = _lib.load()
    S, T, n = 3, 66, 33
    dev = D.planted(S, T, n).to(DEV)
    sp = _lib.stream_ptr()
    stats = torch.empty(S, n, 2, dtype=torch.float32, device=DEV)
    R = torch.empty(S, n, n, dtype=torch.float32, device=DEV)
    assert lib.cgnn_ingest_corr(_lib.ptr(dev), S, T, n, 0, 0, 0, _lib.ptr(stats), _lib.nbytes(stats), _lib.ptr(R),
                                _lib.nbytes(R), sp) == _lib.CGNN_OK
    alpha = torch.full((S,), -7.0, dtype=torch.float64, device=DEV)
    good = [_lib.ptr(dev), S, T, n, 0, 0, _lib.ptr(stats), _lib.ptr(R), _lib.ptr(alpha), _lib.nbytes(alpha), sp]
    bad = {"short alpha": (9, 8 * S - 1), "alpha NULL": (8, None), "stats NULL": (6, None), "matrices NULL": (7, None),
           "ts NULL": (0, None), "alpha misaligned": (8, _lib.ptr(alpha) + 4), "n = 1025": (3, 1025), "T = 1": (2, 1),
           "window > T": (4, T + 1), "S < 0": (1, -1)}
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_shrinkage(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    assert lib.cgnn_ingest_shrinkage(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK                # S == 0
    torch.cuda.synchronize()
    assert bool((alpha == -7.0).all()), "nothing was written"
    assert lib.cgnn_ingest_shrinkage(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(alpha), _bits(ingest.ledoit_wolf_shrinkage(dev)))
    # cgnn_ingest_partial_each on the existing workspace query
    need = lib.cgnn_ingest_partial_workspace_bytes(S, n)
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((S, n, n), -7.0, dtype=torch.float32, device=DEV)
    good = [_lib.ptr(R), S, n, _lib.ptr(alpha), 0, _lib.ptr(work), need, _lib.ptr(out), _lib.nbytes(out), sp]
    bad = {"short work": (6, need - 1), "short out": (8, _lib.nbytes(out) - 1), "shrinkage NULL": (3, None),
           "shrinkage misaligned": (3, _lib.ptr(alpha) + 4), "n = 1025": (2, 1025), "U < 0": (1, -1)}
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_partial_each(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    assert lib.cgnn_ingest_partial_each(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK             # U == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "nothing was written"
    assert lib.cgnn_ingest_partial_each(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(out), _bits(ingest.correlation_matrices(dev, kind="partial", shrinkage="ledoit_wolf")))
    empty = dev[:0]
    assert tuple(ingest.ledoit_wolf_shrinkage(empty).shape) == (0,)
    assert tuple(ingest.correlation_matrices(empty, kind="partial", shrinkage="ledoit_wolf").shape) == (0, n, n)


def test_estimated_shrinkage_through_loader_and_trainer():
    ts, y = TS.two_classes(32, 200, 20)
    dev = ts.to(DEV)
    ds = ingest.from_timeseries(dev, y, kind="partial", shrinkage="ledoit_wolf", keep=0.2, measures=True)
    fixed = ingest.from_timeseries(dev, y, kind="partial", shrinkage=0.1, keep=0.2, measures=True)
    assert ds.x.shape == (32, 20, 5) and int(ds.edge_ptr[-1]) > 0
    mats = ingest.correlation_matrices(dev, kind="partial", shrinkage=ingest.ledoit_wolf_shrinkage(dev))
    ref = ingest.from_matrices(mats, y, keep=0.2, measures=True)
    for name in ("x", "edge_local", "edge_weight", "labels", "edge_ptr_dev"):
        assert torch.equal(getattr(ds, name), getattr(ref, name)), name
    assert not torch.equal(ds.edge_weight, fixed.edge_weight), "each unit's own shrinkage, not 0.1"
    torch.manual_seed(3)
    m = C.GCNConnectome(5, 64, dropout=0.0)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2, weight_decay=1e-4, capturable=True)
    tr = C.Trainer(m, opt, device=DEV, graph=True)
    ld = ResidentDataLoader(ds, 16, shuffle=True, structure_cache=True)
    vl = ResidentDataLoader(ds, 16, shuffle=False, structure_cache=True)
    hist = tr.fit(ld, vl, num_epochs=2, patience=10, verbose=False)
    loss = hist["train_loss"]
    assert len(loss) == 2 and all(torch.isfinite(torch.tensor(v)).all() for v in hist.values())
    assert loss[1] < loss[0], loss
