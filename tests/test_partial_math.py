"""connectome_gnn_amd.ingest's partial-correlation entry points without a GPU: the host statement
(tests/partial_data.py) against its definition by regression residuals and on the matrices whose answer is known, the
excluded-ROI and all-NaN rules, every refusal of ``partial_correlation`` / ``correlation_matrices`` /
``from_timeseries``, and the binding."""
import ctypes

import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import partial_data as D
from tests import timeseries_data as TS


# ---- the statement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n", [(30, 2), (40, 3), (40, 5), (64, 8), (64, 12)])
def test_statement_equals_the_correlation_of_regression_residuals(T, n):
    ts = TS.recipe(2, T, n)
    for s in range(2):
        R = TS.host_corr(ts[s:s + 1])[0]                  # fp64: the identity is exact, not a rounding study
        got = D.host_unit(R)
        want = D.residual_partial(ts[s])
        assert float((got - want).abs().max()) <= 1e-10
        assert torch.equal(got, got.t()) and torch.equal(got.diagonal(), torch.ones(n, dtype=torch.float64))
        assert torch.equal(D.host_unit(R, absolute=True), got.abs())


def test_statement_reads_the_upper_triangle_only():
    R = D.cohort(1, 40, 5)[0].clone()
    want = D.host_unit(R)
    R[3, 1] = 0.75                                        # below the diagonal: not read
    assert torch.equal(D.host_unit(R), want)
    R[1, 3] = 0.75
    assert not torch.equal(D.host_unit(R), want)


@pytest.mark.parametrize("n", [1, 2, 12])
def test_identity_gives_zeros(n):
    eye = torch.eye(n)
    for a in (0.0, 0.3, 1.0):
        assert torch.equal(D.host_unit(eye, a), eye.double())


def test_block_diagonal_gives_zeros_across_blocks():
    R = D.block_diagonal((5, 7), T=40)[0]
    got = D.host_unit(R)
    assert torch.equal(got[:5, 5:], torch.zeros(5, 7, dtype=torch.float64))
    assert torch.equal(got[5:, :5], torch.zeros(7, 5, dtype=torch.float64))
    assert float((got[:5, :5] - D.host_unit(R[:5, :5])).abs().max()) <= 1e-12
    assert float((got[5:, 5:] - D.host_unit(R[5:, 5:])).abs().max()) <= 1e-12
    assert float(got[:5, :5].abs().sum()) > 5.0           # (the blocks themselves are not trivial)


def test_full_shrinkage_gives_zeros():
    R = D.cohort(3, 40, 12)
    got = D.host_partial(R, 1.0)
    assert torch.equal(got, torch.eye(12, dtype=torch.float64).expand(3, 12, 12))
    mid = D.host_partial(R, 0.5)
    off = ~torch.eye(12, dtype=torch.bool)
    assert float(mid[:, off].abs().max()) < float(D.host_partial(R, 0.0)[:, off].abs().max())


def test_excluded_rois_give_zero_rows_and_columns_and_leave_the_others_alone():
    n = 12
    R = D.planted(3, 40, n)
    assert float(R[-1, 1, 1]) == 0.0 and float(R[-1, n - 2, n - 2]) == 0.0
    for a in (0.0, 0.2):
        got = D.host_partial(R, a)
        assert not bool(torch.isnan(got).any())
        for c in (1, n - 2):
            assert torch.equal(got[-1, c], torch.zeros(n, dtype=torch.float64))
            assert torch.equal(got[-1, :, c], torch.zeros(n, dtype=torch.float64))
        others = [i for i in range(n) if i not in (1, n - 2)]
        reduced = D.host_unit(R[-1][others][:, others], a)
        assert float((got[-1][others][:, others] - reduced).abs().max()) <= 1e-12
        assert torch.equal(got[-1].diagonal()[others], torch.ones(n - 2, dtype=torch.float64))
        assert D.kappa_of(R[-1:], a) == pytest.approx(D.kappa2(D.covariance(R[-1][others][:, others], a)[0]))


def test_an_indefinite_or_nan_unit_is_all_nan_and_alone():
    R = D.cohort(3, 40, 12).clone()
    want = D.host_partial(R)
    R[1, 2, 7] = R[1, 7, 2] = 1.5
    got = D.host_partial(R)
    assert bool(torch.isnan(got[1]).all())
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    R[1, 2, 7] = R[1, 7, 2] = float("nan")
    assert bool(torch.isnan(D.host_partial(R)[1]).all())
    # fewer frames than ROIs: singular by construction, positive definite again with shrinkage
    few = D.cohort(1, 8, 12)
    assert D.kappa_of(few, 0.0) > 1e12 and D.kappa_of(few, 0.1) < 100.0
    assert not bool(torch.isnan(D.host_partial(few, 0.1)).any())


def test_host32_is_the_statement_to_fp32_accuracy():
    for T, n, a in ((40, 5, 0.0), (66, 33, 0.0), (60, 84, 0.1)):
        R = D.cohort(3, T, n)
        k = D.kappa_of(R, a)
        assert k <= D.KAPPA_CAP
        err = float((D.host32(R, a).double() - D.host_partial(R, a)).abs().max())
        assert err <= D.tol(k, 0.3), (T, n, a, err, k)      # the measured ratio: the device tests allow 4 x it


# ---- refusals: on CPU tensors, before the residency check ------------------------------------------------------
def _ts(T=30, n=20):
    return TS.recipe(3, T, n)


def _y():
    return torch.zeros(3, dtype=torch.long)


def _both(exc, msg, ts, **kw):
    with pytest.raises(exc, match=msg):
        ingest.correlation_matrices(ts, **kw)
    with pytest.raises(exc, match=msg):
        ingest.from_timeseries(ts, _y(), keep=0.1, **kw)


def test_unknown_kind_is_refused():
    for kind in ("covariance", "Partial", None, 1):
        _both(ValueError, "unknown kind", _ts(), kind=kind)


def test_shrinkage_outside_the_unit_interval_is_refused():
    for a in (-0.01, 1.01, float("nan"), float("inf")):
        _both(ValueError, r"shrinkage must lie in \[0, 1\]", _ts(), kind="partial", shrinkage=a)
        with pytest.raises(ValueError, match=r"shrinkage must lie in \[0, 1\]"):
            ingest.partial_correlation(D.cohort(3, 40, 5), shrinkage=a)
    for a in ("0.1", None, True):
        _both(TypeError, "shrinkage must be a float", _ts(), kind="partial", shrinkage=a)


def test_shrinkage_with_plain_correlation_is_refused():
    _both(ValueError, 'shrinkage applies to kind="partial"', _ts(), shrinkage=0.1)
    _both(ValueError, 'shrinkage applies to kind="partial"', _ts(), kind="correlation", shrinkage=1.0)


def test_too_few_frames_without_shrinkage_are_refused():
    _both(ValueError, "give shrinkage > 0", _ts(21, 20), kind="partial")                 # n + 1 frames
    _both(ValueError, "give shrinkage > 0", _ts(30, 20), kind="partial", window=21, stride=3)   # per UNIT
    for kw in ({"shrinkage": 0.1}, {"shrinkage": 1.0}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):                       # accepted: on to residency
            ingest.correlation_matrices(_ts(21, 20), kind="partial", **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.correlation_matrices(_ts(22, 20), kind="partial")                         # n + 2 frames
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.from_timeseries(_ts(30, 20), _y(), keep=0.1, kind="partial", window=22, stride=4)


def test_more_than_1024_nodes_are_refused():
    assert ingest.PARTIAL_MAX_NODES == 1024
    big = torch.zeros(1).expand(1, 2, 1025)               # no storage behind it
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.correlation_matrices(big, kind="partial", shrinkage=0.5)
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.from_timeseries(big, torch.zeros(1, dtype=torch.long), keep=0.1, kind="partial", shrinkage=0.5)
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.partial_correlation(torch.zeros(1).expand(1, 1025, 1025))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.partial_correlation(torch.zeros(1, 1024, 1024))


def test_malformed_matrices_are_refused():
    R = D.cohort(3, 40, 5)
    for bad, exc, msg in ((R.numpy(), TypeError, "torch.Tensor"), (R.double(), TypeError, "float32"),
                          (R[0], ValueError, r"\[S, n, n\]"), (R[:, :4], ValueError, r"\[S, n, n\]"),
                          (R.transpose(1, 2), ValueError, "contiguous")):
        with pytest.raises(exc, match=msg):
            ingest.partial_correlation(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.partial_correlation(R, shrinkage=0.1, absolute=True)


def test_plain_correlation_takes_the_new_arguments_at_their_defaults():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.correlation_matrices(_ts(), kind="correlation", shrinkage=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.from_timeseries(_ts(), _y(), keep=0.1, kind="correlation", shrinkage=0)


# ---- the binding -----------------------------------------------------------------------------------------------
def test_the_binding_declares_both_symbols():
    for name, args in (("cgnn_ingest_partial_workspace_bytes", 2), ("cgnn_ingest_partial", 10)):
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == args
    assert _lib.PROTOTYPES["cgnn_ingest_partial"][1][3] is ctypes.c_double          # shrinkage
    assert ingest.KINDS == ("correlation", "partial")


def test_the_byte_count_refuses_bad_sizes_without_a_device():
    loaded = _lib.load()
    for args in ((-1, 20), (3, 0), (3, -1), (3, 1025), (2 ** 31, 4)):
        assert loaded.cgnn_ingest_partial_workspace_bytes(*args) < 0, args
    assert loaded.cgnn_ingest_partial_workspace_bytes(0, 20) == 0
    assert loaded.cgnn_ingest_partial(None, 0, 20, 0.0, 0, None, 0, None, 0, None) == _lib.CGNN_OK
    assert loaded.cgnn_ingest_partial(None, 3, 1025, 0.0, 0, None, 0, None, 0, None) == _lib.CGNN_EINVAL
    assert loaded.cgnn_ingest_partial(None, 0, 20, 1.5, 0, None, 0, None, 0, None) == _lib.CGNN_EINVAL
