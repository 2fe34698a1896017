"""connectome_gnn_amd.ingest's shrinkage estimate and per-unit shrinkage without a GPU: the host statement
(tests/shrinkage_data.py) against scikit-learn and on the cases whose answer is known, every refusal of
``ledoit_wolf_shrinkage`` / ``partial_correlation`` / ``correlation_matrices`` / ``from_timeseries`` that the new
arguments add, and the two new functions of the C ABI."""
import pytest
import torch

from connectome_gnn_amd import _lib, ingest
from tests import partial_data as P
from tests import shrinkage_data as D
from tests import timeseries_data as TS

_OK, _INV = _lib.CGNN_OK, _lib.CGNN_EINVAL


# ---- the statement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("L,n,S", D.CASES)
def test_statement_equals_scikit_learn(L, n, S, kind):
    cov = pytest.importorskip("sklearn.covariance")
    for x in D.frames(kind, S, L, n):
        _, rs, z = D._standardised(x)
        kept = rs != 0                                    # constant columns are dropped before the call
        want = cov.ledoit_wolf_shrinkage((z[:, kept] * L ** 0.5).numpy(), assume_centered=True)
        assert abs(D.host_lw(x) - want) <= 1e-12, (L, n, kind)
        assert 0.0 <= D.host_lw(x) <= 1.0
    if kind == "planted" and n >= 3:
        assert int((D._standardised(D.frames(kind, S, L, n)[0])[1] == 0).sum()) == 1, "one constant column"


def test_one_roi_gives_zero():
    for x in D.white(2, 7, 1):
        assert D.host_lw(x) == 0.0 and D.host_lw32(x) == 0.0 and D.cond(x) == 0.0


def test_one_roi_that_is_not_constant_gives_zero():
    x = torch.full((9, 4), 2.5)
    x[:, 2] = D.white(1, 9, 1)[0, :, 0]
    assert D.host_lw(x) == 0.0 and D.host_lw32(x) == 0.0
    assert D.host_lw(torch.full((9, 4), 2.5)) == 0.0      # and none at all


def test_two_frames_give_zero():
    for kind in D.KINDS:
        for x in D.frames(kind, 3, 2, 5):
            assert D.host_lw(x) == 0.0 and D.host_lw32(x) == 0.0
            assert abs(D.ratio(x)) <= 1e-14               # B - F is zero up to rounding, of either sign


def test_the_clip_gives_exactly_one():
    x = D.clipped()[0]
    assert tuple(x.shape) == (1000, 12)
    assert D.ratio(x) > 1.0 and abs(D.ratio(x) - 1.34) < 0.01      # (or the case no longer meets the clip)
    assert D.host_lw(x) == 1.0 and D.host_lw32(x) == 1.0


def test_a_nan_frame_gives_a_nan():
    x = D.planted(1, 9, 33)[0].clone()
    x[4] = float("nan")
    assert D.host_lw(x) != D.host_lw(x) and D.host_lw32(x) != D.host_lw32(x)


def test_a_constant_column_changes_p_only():
    x = D.planted(1, 66, 97)[0]
    others = [i for i in range(97) if i != 97 // 2]
    assert D.host_lw(x) == pytest.approx(D.host_lw(x[:, others].contiguous()), abs=1e-14)


def test_the_fp32_statement_is_within_the_measured_ratio():
    """What the device tests build their tolerance on: 4 x this ratio, measured on the host alone."""
    worst = D.worst_host32_ratio()
    print(f"worst |host_lw32 - host_lw| / (2^-24 cond) = {worst:.4f}")
    assert 0.0 < worst <= 0.4508


def test_windows_are_units():
    ts = D.planted(2, 50, 20)
    got = D.host_cohort(ts, 20, 7)
    assert tuple(got.shape) == (2 * TS.num_windows(50, 20, 7),)
    assert float(got[5 + 3]) == D.host_lw(ts[1, 21:41])


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


def test_the_names():
    assert ingest.SHRINKAGES == ("ledoit_wolf",)
    assert callable(ingest.ledoit_wolf_shrinkage)


def test_a_malformed_shrinkage_tensor_is_refused():
    R = P.cohort(3, 40, 5)
    good = torch.full((3,), 0.1, dtype=torch.float64)
    for bad, exc, msg in ((good[:2], ValueError, r"\[U\] = \[3\]"), (good[None], ValueError, r"\[U\] = \[3\]"),
                          (torch.tensor(0.1, dtype=torch.float64), ValueError, r"\[U\] = \[3\]"),
                          (good.half(), TypeError, "float64"), (torch.zeros(3, dtype=torch.long), TypeError, "float64"),
                          (good.to("meta"), ValueError, "is on meta")):
        with pytest.raises(exc, match=msg):
            ingest.partial_correlation(R, shrinkage=bad)
        _both(exc, msg, _ts(), kind="partial", shrinkage=bad)
    # one value per UNIT: three subjects in windows are more than three units
    _both(ValueError, r"\[U\] = \[9\]", _ts(), kind="partial", shrinkage=good, window=10)
    for ok in (good, good.float(), torch.full((3,), 7.0, dtype=torch.float64)):     # values are the kernel's to read
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ingest.partial_correlation(R, shrinkage=ok)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ingest.correlation_matrices(_ts(), kind="partial", shrinkage=ok)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ingest.from_timeseries(_ts(), _y(), keep=0.1, kind="partial", shrinkage=ok)


def test_an_estimator_needs_the_frames():
    with pytest.raises(ValueError, match="ledoit_wolf_shrinkage"):
        ingest.partial_correlation(P.cohort(3, 40, 5), shrinkage="ledoit_wolf")


def test_an_estimator_with_plain_correlation_is_refused():
    _both(ValueError, 'shrinkage applies to kind="partial"', _ts(), shrinkage="ledoit_wolf")
    _both(ValueError, 'shrinkage applies to kind="partial"', _ts(), kind="correlation", shrinkage="ledoit_wolf")
    _both(ValueError, 'shrinkage applies to kind="partial"', _ts(), shrinkage=torch.zeros(3, dtype=torch.float64))


def test_an_unknown_estimator_is_refused():
    for a in ("oas", "Ledoit_Wolf", "", "0.1", b"ledoit_wolf", ("ledoit_wolf",), [0.1, 0.1, 0.1]):
        _both(TypeError, "^shrinkage must be a float", _ts(), kind="partial", shrinkage=a)
        with pytest.raises(TypeError, match="^shrinkage must be a float"):
            ingest.partial_correlation(P.cohort(3, 40, 5), shrinkage=a)


def test_few_frames_are_accepted_with_an_estimate_or_a_tensor():
    for a in ("ledoit_wolf", torch.full((3,), 0.3, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):                       # accepted: on to residency
            ingest.correlation_matrices(_ts(21, 20), kind="partial", shrinkage=a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.from_timeseries(_ts(30, 20), _y(), keep=0.1, kind="partial", window=10, shrinkage="ledoit_wolf")
    _both(ValueError, "give shrinkage > 0", _ts(21, 20), kind="partial", shrinkage=0.0)   # the float 0.0 alone


def test_the_estimate_refuses_what_the_correlation_refuses():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.ledoit_wolf_shrinkage(_ts())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.ledoit_wolf_shrinkage(_ts(), window=10, stride=3)
    with pytest.raises(ValueError, match="contiguous"):
        ingest.ledoit_wolf_shrinkage(_ts().transpose(1, 2))
    for bad, exc, msg in ((_ts().numpy(), TypeError, "torch.Tensor"), (_ts().double(), TypeError, "float32"),
                          (_ts()[0], ValueError, r"\[S, T, n\]"), (_ts()[:, :1], ValueError, "T >= 2")):
        with pytest.raises(exc, match=msg):
            ingest.ledoit_wolf_shrinkage(bad)
    with pytest.raises(ValueError, match=r"window must lie in \[2, T\]"):
        ingest.ledoit_wolf_shrinkage(_ts(), window=31)
    with pytest.raises(ValueError, match="give window= with it"):
        ingest.ledoit_wolf_shrinkage(_ts(), stride=3)
    with pytest.raises(TypeError, match="window must be an int"):
        ingest.ledoit_wolf_shrinkage(_ts(), window=10.0)
    with pytest.raises(ValueError, match="n <= 1024"):
        ingest.ledoit_wolf_shrinkage(torch.zeros(1).expand(1, 2, 1025))


# ---- the binding and the C ABI: refusals return before any launch, so they need no device ------------------------
def test_the_binding_declares_both_symbols():
    for name, args in (("cgnn_ingest_shrinkage", 11), ("cgnn_ingest_partial_each", 10)):
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == args
    assert _lib.PROTOTYPES["cgnn_ingest_partial_each"][1][3] is _lib.DevPtr              # shrinkage: a device pointer
    assert _lib.ABI_VERSION == 2 and _lib.load().cgnn_abi_version() == 2


_A, _A2, _A4 = 0x1000, 0x1002, 0x1004            # 16-byte aligned; not 4-byte aligned; not 8-byte aligned
_LW = "cgnn_ingest_shrinkage"
_EACH = "cgnn_ingest_partial_each"
_DEFAULTS = {
    # 6 subjects of 30 frames and 20 ROIs: 6 units, or 18 in windows of 10
    _LW: dict(ts=_A, S=6, T=30, n=20, window=0, stride=0, stats=_A, matrices=_A, alpha=_A, alpha_bytes=48, stream=None),
    # 3 units of 20 ROIs: a slab [32][32] per workgroup
    _EACH: dict(matrices=_A, U=3, n=20, shrinkage=_A, absolute=0, workspace=_A, workspace_bytes=3 * 32 * 32 * 4, out=_A,
                out_bytes=3 * 20 * 20 * 4, stream=None),
}
_CALLS = [
    (_LW, dict(alpha_bytes=47), _INV),
    (_LW, dict(alpha_bytes=-1), _INV),
    (_LW, dict(window=10, stride=10), _INV),                         # 18 units now: 144 bytes
    (_LW, dict(window=10, stride=10, alpha_bytes=143), _INV),
    (_LW, dict(ts=None), _INV),
    (_LW, dict(stats=None), _INV),
    (_LW, dict(matrices=None), _INV),
    (_LW, dict(alpha=None), _INV),
    (_LW, dict(ts=_A2), _INV),
    (_LW, dict(stats=_A2), _INV),
    (_LW, dict(matrices=_A2), _INV),
    (_LW, dict(alpha=_A4), _INV),
    (_LW, dict(S=-1), _INV),
    (_LW, dict(n=0), _INV),
    (_LW, dict(n=-3), _INV),
    (_LW, dict(n=1025), _INV),
    (_LW, dict(T=1), _INV),
    (_LW, dict(window=1, stride=1), _INV),
    (_LW, dict(window=31, stride=1), _INV),
    (_LW, dict(window=-2, stride=1), _INV),
    (_LW, dict(window=10, stride=0), _INV),
    (_LW, dict(window=10, stride=-1), _INV),
    (_LW, dict(S=2 ** 31 // 20 + 1), _INV),
    (_LW, dict(S=2 ** 31 // 20 // 2, window=2, stride=1), _INV),     # S * n < 2^31, U * n is not
    (_LW, dict(S=0), _OK),
    (_LW, dict(S=0, ts=None, stats=None, matrices=None, alpha=None, alpha_bytes=0), _OK),
    (_LW, dict(S=0, n=1025), _INV),                                  # the ranges come before S == 0
    (_LW, dict(S=0, T=1), _INV),
    (_LW, dict(S=0, alpha_bytes=-1), _INV),
    (_EACH, dict(workspace_bytes=3 * 32 * 32 * 4 - 1), _INV),
    (_EACH, dict(out_bytes=3 * 20 * 20 * 4 - 1), _INV),
    (_EACH, dict(workspace_bytes=-1), _INV),
    (_EACH, dict(out_bytes=-1), _INV),
    (_EACH, dict(matrices=None), _INV),
    (_EACH, dict(shrinkage=None), _INV),
    (_EACH, dict(workspace=None), _INV),
    (_EACH, dict(out=None), _INV),
    (_EACH, dict(matrices=_A2), _INV),
    (_EACH, dict(shrinkage=_A4), _INV),
    (_EACH, dict(workspace=_A4), _INV),
    (_EACH, dict(out=_A2), _INV),
    (_EACH, dict(U=-1), _INV),
    (_EACH, dict(n=0), _INV),
    (_EACH, dict(n=1025), _INV),
    (_EACH, dict(U=2 ** 31 // 20 + 1), _INV),
    (_EACH, dict(U=0), _OK),
    (_EACH, dict(U=0, matrices=None, shrinkage=None, workspace=None, workspace_bytes=0, out=None, out_bytes=0), _OK),
    (_EACH, dict(U=0, n=1025), _INV),
]


def test_the_new_entry_points_refuse_bad_arguments_with_the_documented_code():
    lib = _lib.load()
    assert lib.cgnn_set_fused_grid(4) == _OK              # (the slab count of the defaults does not depend on a device)
    try:
        assert lib.cgnn_ingest_partial_workspace_bytes(3, 20) == 3 * 32 * 32 * 4
        got = []
        for name, change, want in _CALLS:
            args = dict(_DEFAULTS[name], **change)
            got.append((name, change, want, getattr(lib, name)(*args.values())))
    finally:
        assert lib.cgnn_set_fused_grid(0) == _OK
    wrong = [(n, c, w, g) for n, c, w, g in got if g != w]
    assert not wrong, wrong
