"""connectome_gnn_amd.ingest.partial_correlation / correlation_matrices(kind="partial") on the device
(csrc/partial.hip) against the fp64 host statement (tests/partial_data.py) of the same fp32 bits.

Tolerance: ``tol = c kappa 2^-24 + 4 2^-24`` with ``kappa`` the fp64 2-norm condition number of the shrunk matrix,
asserted ``<= 4096`` for every parity case.  ``c`` is measured against the host's fp32 LAPACK (``partial_data.host32``:
cholesky, triangular inverse, ``M^T M``), never against the kernel: the largest ``err_host32 / (kappa 2^-24)`` over the
parity cohorts below is 0.2901 (at n = 2, shrinkage 0.1; at most 0.17 for n >= 31 and 0.03 at n = 360), and a factor 4
covers the kernel's k-ascending fp32 accumulation against LAPACK's blocked sums: ``c = 1.161``.  Each parity case
prints the device's own ratio.

The block of the factorisation is 32 for every n up to 1024: there is no size at which the block rule changes.  The
shapes straddle the multiples of 32 (the block), of 96 (the tile of the final product) and of 4 (the vector stores).
"""
import functools

import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib, ingest
from connectome_gnn_amd.resident import ResidentDataLoader
from tests import partial_data as D
from tests import timeseries_data as TS

pytestmark = pytest.mark.gpu
DEV = "cuda"
C_TOL = 4 * 0.2901                                # 4 x the largest host32 ratio (module docstring)
WHITE = (1100, 1024, 1)
SHAPES = [(40, 1, 3), (40, 2, 3), (40, 5, 3), (64, 31, 3), (64, 32, 3), (66, 33, 3), (130, 64, 3), (130, 65, 3),
          (200, 96, 3), (200, 97, 3), (300, 84, 3), (300, 130, 3), (400, 193, 3), (1200, 360, 2), WHITE]
PARITY = [s + (a,) for s in SHAPES for a in (0.0, 0.1)] + [(60, 84, 3, 0.1), (400, 360, 3, 0.1)]


def _frames(T, n, S):
    return D.white_frames(T, n) if (T, n, S) == WHITE else TS.recipe(S, T, n)


def _matrices(T, n, S):
    return D.white(T, n) if (T, n, S) == WHITE else D.cohort(S, T, n)


@functools.lru_cache(maxsize=None)
def _case(T, n, S, a):
    """(host matrices, fp64 statement, kappa, device output, |.| device output)"""
    R = _matrices(T, n, S)
    dev = R.to(DEV)
    return R, D.host_partial(R, a), D.kappa_of(R, a), ingest.partial_correlation(dev, shrinkage=a), \
        ingest.partial_correlation(dev, shrinkage=a, absolute=True)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_parity(got, want, kappa, what):
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), what
    assert kappa <= D.KAPPA_CAP, (what, kappa)
    err = float((got.cpu().double() - want).abs().max())
    tol = D.tol(kappa, C_TOL)
    print(f"{what}: kappa {kappa:.1f}, max error {err:.3e}, ratio err / (kappa 2^-24) {err / (kappa * D.EPS):.4f}, "
          f"tol {tol:.3e}")
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("T,n,S,a", PARITY)
def test_parity_with_the_fp64_statement(T, n, S, a):
    _, want, kappa, got, _ = _case(T, n, S, a)
    assert got.device.type == "cuda" and got.is_contiguous()
    _check_parity(got, want, kappa, f"T={T} n={n} shrinkage={a}")


@pytest.mark.parametrize("T,n,S,a", PARITY)
def test_exact_properties(T, n, S, a):
    R, _, _, got, got_abs = _case(T, n, S, a)
    g = got.cpu()
    assert torch.equal(_bits(g), _bits(g.transpose(1, 2))), "bit-symmetric"
    assert torch.equal(g.diagonal(dim1=1, dim2=2), torch.ones(S, n)), "diagonal: exactly 1"
    assert float(g.min()) >= -1.0 and float(g.max()) <= 1.0 and not bool(torch.isnan(g).any())
    assert torch.equal(_bits(got_abs), _bits(got.abs())), "absolute=True is |.| of the default"
    again = ingest.partial_correlation(R.to(DEV), shrinkage=a)
    assert torch.equal(_bits(again), _bits(got)), "two calls, the same bits"


@pytest.mark.parametrize("T,n,S", SHAPES + [(60, 84, 3)])
def test_in_place_over_the_correlations_equals_the_two_step_call(T, n, S):
    dev = _frames(T, n, S).to(DEV)
    r = ingest.correlation_matrices(dev)
    for absolute in (False, True):
        two = ingest.partial_correlation(r, shrinkage=0.1, absolute=absolute)
        one = ingest.correlation_matrices(dev, kind="partial", shrinkage=0.1, absolute=absolute)
        assert torch.equal(_bits(one), _bits(two)), absolute
    assert torch.equal(_bits(r), _bits(ingest.correlation_matrices(dev, kind="correlation", shrinkage=0.0)))


@pytest.mark.parametrize("n", [1, 5, 33, 97, 360])
def test_identity_gives_exact_zeros(n):
    eye = torch.eye(n).expand(2, n, n).contiguous()
    for a in (0.0, 0.1, 1.0):
        assert torch.equal(ingest.partial_correlation(eye.to(DEV), shrinkage=a).cpu(), eye), a


def test_full_shrinkage_gives_exact_zeros():
    R = D.cohort(3, 300, 84)
    assert torch.equal(ingest.partial_correlation(R.to(DEV), shrinkage=1.0).cpu(), torch.eye(84).expand(3, 84, 84))


def test_block_diagonal_gives_exact_zeros_across_the_blocks():
    R = D.block_diagonal((40, 57))
    got = ingest.partial_correlation(R.to(DEV)).cpu()[0]
    assert torch.equal(got[:40, 40:], torch.zeros(40, 57)) and torch.equal(got[40:, :40], torch.zeros(57, 40))
    _check_parity(got[None], D.host_partial(R), D.kappa_of(R), "blocks of 40 + 57")


@pytest.mark.parametrize("T,n,a", [(40, 5, 0.0), (66, 33, 0.0), (300, 84, 0.0), (200, 97, 0.1), (400, 193, 0.0)])
def test_constant_columns_are_excluded(T, n, a):
    R = D.planted(3, T, n)
    assert float(R[-1, 1, 1]) == 0.0 and float(R[-1, n - 2, n - 2]) == 0.0
    got = ingest.partial_correlation(R.to(DEV), shrinkage=a).cpu()
    assert not bool(torch.isnan(got).any())
    for c in (1, n - 2):
        assert torch.equal(got[-1, c], torch.zeros(n)) and torch.equal(got[-1, :, c], torch.zeros(n)), c
    others = [i for i in range(n) if i not in (1, n - 2)]
    assert torch.equal(got[-1].diagonal()[others], torch.ones(n - 2))
    assert torch.equal(got[:-1].diagonal(dim1=1, dim2=2), torch.ones(2, n))
    reduced = R[-1][others][:, others].contiguous()[None]
    _check_parity(got[-1][others][:, others][None], D.host_partial(reduced, a), D.kappa_of(reduced, a),
                  f"T={T} n={n}: the other ROIs against the reduced matrix")
    _check_parity(got, D.host_partial(R, a), D.kappa_of(R, a), f"T={T} n={n}: planted")
    assert torch.equal(_bits(got), _bits(got.transpose(1, 2)))


@pytest.mark.parametrize("n,T", [(33, 66), (84, 300), (130, 300)])
def test_an_indefinite_unit_is_all_nan_and_its_neighbours_are_untouched(n, T):
    R = D.cohort(3, T, n).clone()
    want = ingest.partial_correlation(R.to(DEV))
    R[1, 2, n - 3] = R[1, n - 3, 2] = 1.5
    got = ingest.partial_correlation(R.to(DEV))
    assert bool(torch.isnan(got[1]).all())
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[2]), _bits(want[2]))
    assert bool(torch.isnan(D.host_partial(R)[1]).all())
    ds = ingest.from_matrices(got, torch.zeros(3, dtype=torch.long), keep=0.2)
    ptr = ds.edge_ptr
    assert int(ptr[2] - ptr[1]) == 0 and int(ptr[1] - ptr[0]) > 0 and int(ptr[3] - ptr[2]) > 0   # NaN: never an edge


def test_many_units_walk_the_grid_stride():
    Sg, T, n = 40, 300, 84
    R = D.cohort(Sg, T, n, seed=3)
    dev = R.to(DEV)
    lib = _lib.load()
    try:
        assert lib.cgnn_set_fused_grid(3) == _lib.CGNN_OK
        few = ingest.partial_correlation(dev, shrinkage=0.1)
    finally:
        lib.cgnn_set_fused_grid(0)
    full = ingest.partial_correlation(dev, shrinkage=0.1)
    assert torch.equal(_bits(few), _bits(full))
    _check_parity(full, D.host_partial(R, 0.1), D.kappa_of(R, 0.1), "40 units")


@pytest.mark.parametrize("n", [20, 84])
def test_windows_are_the_per_window_calls(n):
    T, L, st = 50, 20, 7
    dev = TS.recipe(3, T, n).to(DEV)
    W = TS.num_windows(T, L, st)
    got = ingest.correlation_matrices(dev, window=L, stride=st, kind="partial", shrinkage=0.2)
    assert tuple(got.shape) == (3 * W, n, n) and not bool(torch.isnan(got).any())
    for w in range(W):
        part = ingest.correlation_matrices(dev[:, w * st:w * st + L].contiguous(), kind="partial", shrinkage=0.2)
        assert torch.equal(_bits(got[w::W]), _bits(part)), w


def test_abi_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    U, n = 3, 84
    dev = D.cohort(U, 300, n).to(DEV)
    sp = _lib.stream_ptr()
    need = lib.cgnn_ingest_partial_workspace_bytes(U, n)
    assert need >= U * 96 * 96 * 4
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((U, n, n), -7.0, dtype=torch.float32, device=DEV)
    good = [_lib.ptr(dev), U, n, 0.1, 0, _lib.ptr(work), need, _lib.ptr(out), _lib.nbytes(out), sp]
    bad = {"short work": (6, need - 1), "short out": (8, _lib.nbytes(out) - 1), "n = 1025": (2, 1025),
           "n = 0": (2, 0), "U < 0": (1, -1), "U * n >= 2^31": (1, 2 ** 31 // n + 1), "shrinkage < 0": (3, -0.5),
           "shrinkage > 1": (3, 1.5), "shrinkage NaN": (3, float("nan")), "matrices NULL": (0, None),
           "work NULL": (5, None), "out NULL": (7, None), "work misaligned": (5, _lib.ptr(work) + 4),
           "out misaligned": (7, _lib.ptr(out) + 2), "work bytes < 0": (6, -1), "out bytes < 0": (8, -1)}
    for name, (p, v) in bad.items():
        assert lib.cgnn_ingest_partial(*(good[:p] + [v] + good[p + 1:])) == _lib.CGNN_EINVAL, name
    for args in ((U, 1025), (U, 0), (-1, n), (2 ** 31 // n + 1, n)):
        assert lib.cgnn_ingest_partial_workspace_bytes(*args) < 0, args
    assert lib.cgnn_ingest_partial_workspace_bytes(0, n) == 0
    assert lib.cgnn_ingest_partial(*(good[:1] + [0] + good[2:])) == _lib.CGNN_OK                  # U == 0
    assert lib.cgnn_ingest_partial(None, 0, n, 0.1, 0, None, 0, None, 0, sp) == _lib.CGNN_OK
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "nothing was written"
    assert lib.cgnn_ingest_partial(*good) == _lib.CGNN_OK
    assert torch.equal(_bits(out), _bits(ingest.partial_correlation(dev, shrinkage=0.1)))
    assert tuple(ingest.partial_correlation(dev[:0]).shape) == (0, n, n)


def test_no_cohort_sized_temporaries():
    """Above the resident input only the output and the workspace (one slab per workgroup) are allocated; the
    in-place form allocates the workspace alone."""
    U, n = 64, 360
    dev = D.cohort(2, 1200, n).repeat(U // 2, 1, 1).contiguous().to(DEV)
    ingest.partial_correlation(dev, shrinkage=0.1)                     # (the library is loaded, the kernel too)
    need = _lib.load().cgnn_ingest_partial_workspace_bytes(U, n)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ingest.partial_correlation(dev, shrinkage=0.1)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert tuple(out.shape) == (U, n, n)
    assert 4 * U * n * n <= peak < 4 * U * n * n + need + 2 ** 20, (peak, 4 * U * n * n, need)
    assert torch.equal(_bits(out[:2]), _bits(out[2:4]))


def test_partial_correlation_through_loader_and_trainer():
    ts, y = TS.two_classes(32, 200, 20)
    dev = ts.to(DEV)
    ds = ingest.from_timeseries(dev, y, kind="partial", shrinkage=0.1, keep=0.2, measures=True)
    plain = ingest.from_timeseries(dev, y, keep=0.2, measures=True)
    assert ds.x.shape == (32, 20, 5) and int(ds.edge_ptr[-1]) > 0
    mats = ingest.correlation_matrices(dev, kind="partial", shrinkage=0.1)
    ref = ingest.from_matrices(mats, y, keep=0.2, measures=True)
    for name in ("x", "edge_local", "edge_weight", "labels", "edge_ptr_dev"):
        assert torch.equal(getattr(ds, name), getattr(ref, name)), name
    assert ds.edge_local.shape != plain.edge_local.shape or not torch.equal(ds.edge_local, plain.edge_local), \
        "direct edges, not the correlation's"
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
