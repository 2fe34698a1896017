"""The host statement of the mid-ranks (tests/rank_data.py): against ``scipy.stats.rankdata`` and ``spearmanr``, its
exactness in fp32; the constants and the tables that must not move; the argument checks of ``ingest.rank_timeseries`` and
``rank=``; the header and the binding of cgnn_ingest_rank and the refusals of the C entry points, none of which reaches
a launch.  No device is touched."""
import numpy as np
import pytest
import scipy.stats
import torch

from connectome_gnn_amd import _lib, ingest
from tests import censor_data as CD
from tests import rank_data as RD
from tests.abi_header import check_header

S = 3
SHAPES = [(2, 1), (3, 7), (65, 5), (129, 33), (300, 9)]


# ---- the statement ----
@pytest.mark.parametrize("T,n", SHAPES)
def test_the_statement_is_scipys_rankdata(T, n):
    num = len(CD.KINDS)
    x, m = RD.series(num, T, n).numpy(), RD.masks(num, T).numpy()
    plain = RD.host_ranks(x)
    masked = RD.host_ranks(x, m)
    for s in range(num):
        want = scipy.stats.rankdata(x[s], method="average", axis=0, nan_policy="propagate")
        assert np.array_equal(plain[s], want, equal_nan=True), (T, n, s)
        want = np.zeros((T, n))
        if m[s].any():
            want[m[s]] = scipy.stats.rankdata(x[s][m[s]], method="average", axis=0, nan_policy="propagate")
        assert np.array_equal(masked[s], want, equal_nan=True), (T, n, s, CD.KINDS[s])
        assert not masked[s][~m[s]].any()
    at = RD.nan_at(num, n)
    if at is not None:
        assert np.isnan(plain[at[0], :, at[1]]).all() and np.isnan(plain).sum() == T, "its column of its subject"


def test_the_recipe_holds_what_it_says():
    T, n = 129, 33
    x = RD.series(S, T, n)
    r = RD.series_ranks(S, T, n)
    col = RD.SPECIAL
    assert sorted(col.values()) == list(range(5))
    assert (r[col["constant"] % S, :, col["constant"]] == (T + 1) / 2).all()
    z = x[col["zeros"] % S, :, col["zeros"]]
    assert bool(torch.signbit(z[z == 0]).any()) and not bool(torch.signbit(z[z == 0]).all()), "both zeros"
    assert len(set(r[col["zeros"] % S, :, col["zeros"]][(z == 0).numpy()])) == 1, "-0.0 == +0.0"
    i = x[col["infs"] % S, :, col["infs"]]
    assert bool((i == float("inf")).any()) and bool((i == float("-inf")).any())
    assert np.isfinite(r[col["infs"] % S, :, col["infs"]]).all(), "+-inf are ordinary values"
    sub = x[col["subnormal"] % S, :, col["subnormal"]]
    assert len(set(sub.tolist())) == T and float(sub.abs().max()) < 2.0 ** -126 and bool((sub == 0).any())
    assert (r[col["subnormal"] % S, :, col["subnormal"]] == np.arange(1, T + 1)).all(), "subnormals are values"
    assert (r[col["descending"] % S, :, col["descending"]] == np.arange(T, 0, -1)).all()
    ties = sum(len(np.unique(RD.plain(S, T, n)[s, :, c])) < T for s in range(S) for c in range(n))
    assert ties == S * n, "quarter steps: every column has ties"
    assert bool(torch.isnan(x).sum() == 1) and not bool(torch.isnan(RD.series(S, T, n, 0, False)).any())
    assert set(CD.KINDS) >= {"one", "two", "none"} and RD.masks(10, 67) is CD.masks(10, 67)


@pytest.mark.parametrize("T,n", [(65, 5), (300, 9)])
def test_corrcoef_of_the_ranks_is_scipys_spearman(T, n):
    x = RD.plain(S, T, n).numpy()
    for s in range(S):
        want = scipy.stats.spearmanr(x[s].astype(np.float64)).statistic
        assert np.abs(RD.spearman(x[s]) - want).max() <= 1e-12
    m = RD.masks(10, T).numpy()[2]                      # the random mask
    want = scipy.stats.spearmanr(x[0][m].astype(np.float64)).statistic
    assert np.abs(RD.spearman(x[0], m) - want).max() <= 1e-12


def test_every_rank_is_a_multiple_of_a_half_and_exact_in_fp32():
    for T, n in SHAPES:
        r = RD.series_ranks(S, T, n)
        r = r[~np.isnan(r)]
        assert (2 * r == np.round(2 * r)).all() and r.min() >= 1 and r.max() <= T
        assert (r.astype(np.float32).astype(np.float64) == r).all()
    # every value a unit of up to RANK_MAX_FRAMES frames can hold
    every = np.arange(2, 2 * RD.MAX_FRAMES + 1) / 2.0
    assert (every.astype(np.float32).astype(np.float64) == every).all()
    g = np.random.default_rng(5)
    v = np.round(4 * g.standard_normal(RD.MAX_FRAMES)).astype(np.float32) / 4
    r = RD.column_ranks(v)
    assert np.array_equal(r, scipy.stats.rankdata(v, method="average")) and r.max() <= RD.MAX_FRAMES
    assert (r.astype(np.float32).astype(np.float64) == r).all() and r.sum() == RD.MAX_FRAMES * (RD.MAX_FRAMES + 1) / 2


def test_the_constants_and_what_must_not_move():
    assert ingest.RANK_MAX_FRAMES == RD.MAX_FRAMES == 4096
    assert ingest.KINDS == ("correlation", "partial"), "ranking is an argument, not a kind"
    assert len(_lib.PROTOTYPES) == 127
    assert list(_lib.RANK_PROTOTYPES) == ["cgnn_ingest_rank", "cgnn_ingest_rank_masked"]
    import connectome_gnn_amd
    assert not {"rank_timeseries", "RANK_MAX_FRAMES"} & set(connectome_gnn_amd.__all__)
    with pytest.raises(ValueError, match="unknown kind"):
        ingest.correlation_matrices(RD.plain(S, 9, 5), kind="spearman")


# ---- the Python arguments ----
def test_rank_timeseries_and_rank_check_their_arguments():
    x = RD.plain(S, 30, 5)
    y = torch.arange(S) % 2
    for bad in ("yes", 1, 0, None, 1.0):
        with pytest.raises(TypeError, match="rank must be a bool"):
            ingest.correlation_matrices(x, rank=bad)
        with pytest.raises(TypeError, match="rank must be a bool"):
            ingest.from_timeseries(x, y, keep=0.5, rank=bad)
        with pytest.raises(TypeError, match="rank must be a bool"):
            ingest.ledoit_wolf_shrinkage(x, rank=bad)
    long = torch.zeros(1, 4097, 2)
    with pytest.raises(ValueError, match="at most RANK_MAX_FRAMES = 4096 frames"):
        ingest.rank_timeseries(long)
    with pytest.raises(ValueError, match="at most RANK_MAX_FRAMES = 4096 frames"):
        ingest.correlation_matrices(long, rank=True)
    with pytest.raises(ValueError, match="at most RANK_MAX_FRAMES = 4096 frames"):
        ingest.from_timeseries(long, torch.zeros(1, dtype=torch.long), keep=0.5, rank=True)
    with pytest.raises(ValueError, match="at most RANK_MAX_FRAMES = 4096 frames"):
        ingest.ledoit_wolf_shrinkage(long, rank=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # the window is what is ranked
        ingest.rank_timeseries(long, window=4096)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # and without rank=True nothing is
        ingest.correlation_matrices(long)
    # out
    with pytest.raises(TypeError, match="out must be a torch.Tensor or None"):
        ingest.rank_timeseries(x, out=x.numpy())
    with pytest.raises(TypeError, match="out must be float32"):
        ingest.rank_timeseries(x, out=x.double())
    with pytest.raises(ValueError, match=r"out must be \(3, 30, 5\)"):
        ingest.rank_timeseries(x, out=torch.empty(S, 30, 4))
    with pytest.raises(ValueError, match=r"out must be \(9, 10, 5\) as the ranked units are"):
        ingest.rank_timeseries(x, window=10, out=x)
    with pytest.raises(ValueError, match=r"out must be \(9, 10, 5\)"):
        ingest.rank_timeseries(x, window=10, out=torch.empty(S, 3, 10, 5))
    with pytest.raises(ValueError, match="out must be contiguous"):
        ingest.rank_timeseries(x, out=torch.empty(S, 5, 30).transpose(1, 2))
    # the series, the window and the mask are checked as everywhere
    with pytest.raises(TypeError, match="float32"):
        ingest.rank_timeseries(x.double())
    with pytest.raises(ValueError, match=r"window must lie in \[2, T\]"):
        ingest.rank_timeseries(x, window=31)
    with pytest.raises(ValueError, match="give window= with it"):
        ingest.rank_timeseries(x, stride=3)
    with pytest.raises(TypeError, match="sample_mask must be bool"):
        ingest.rank_timeseries(x, sample_mask=torch.ones(S, 30))
    with pytest.raises(ValueError, match=r"sample_mask must be \[S, T\]"):
        ingest.rank_timeseries(x, sample_mask=torch.ones(S, 29, dtype=torch.bool))
    # a valid request gets as far as the device check: there is no CPU path
    m = RD.masks(S, 30)
    for call in (lambda: ingest.rank_timeseries(x), lambda: ingest.rank_timeseries(x, out=x),
                 lambda: ingest.rank_timeseries(x, window=10, stride=3, sample_mask=m),
                 lambda: ingest.rank_timeseries(x, window=10, out=torch.empty(9, 10, 5)),
                 lambda: ingest.correlation_matrices(x, rank=True),
                 lambda: ingest.correlation_matrices(x, rank=True, kind="partial", shrinkage="ledoit_wolf", window=12),
                 lambda: ingest.correlation_matrices(x, rank=False),
                 lambda: ingest.ledoit_wolf_shrinkage(x, rank=True, sample_mask=m),
                 lambda: ingest.from_timeseries(x, y, keep=0.5, rank=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- the C ABI ----
def test_the_prototypes_match_their_header_type_by_type():
    hdr = check_header("cgnn_rank.h", _lib.RANK_PROTOTYPES, ["cgnn_ingest_rank", "cgnn_ingest_rank_masked"],
                       [("int32_t stride, ", ""), ("const uint8_t* keep", "int32_t keep")])
    lib = _lib.load()
    assert f"#define CGNN_RANK_MAX_FRAMES {ingest.RANK_MAX_FRAMES}\n" in hdr
    assert _lib.ABI_VERSION == 2 and lib.cgnn_abi_version() == 2, "the change is additive"


_A, _A2 = 0x1000, 0x1002                    # 4-byte aligned / not: never dereferenced
_INV, _OK = _lib.CGNN_EINVAL, _lib.CGNN_OK
_CALL, _MASKED = "cgnn_ingest_rank", "cgnn_ingest_rank_masked"
_BIG_S = 2 ** 31 // 20 + 1                  # S * n >= 2^31 at n = 20
# defaults that pass every check but the output's byte count: S = 6 runs of 50 frames and 20 ROIs, out one byte short
_DEFAULTS = {
    _CALL: dict(ts=_A, S=6, T=50, n=20, window=0, stride=0, out=_A, out_bytes=6 * 50 * 20 * 4 - 1, stream=None),
    _MASKED: dict(ts=_A, S=6, T=50, n=20, window=0, stride=0, keep=_A, keep_bytes=300, out=_A,
                  out_bytes=6 * 50 * 20 * 4 - 1, stream=None),
}
_EMPTY = dict(ts=None, S=0, out=None, out_bytes=0)
_BOTH = [
    # ---- everything is in order but the output, which is one byte short
    (dict(), _INV),
    (dict(out_bytes=0), _INV),
    (dict(out_bytes=-1), _INV),
    (dict(window=20, stride=10, out_bytes=6 * 4 * 20 * 20 * 4 - 1), _INV),      # 4 windows a subject
    (dict(T=4096, out_bytes=6 * 4096 * 20 * 4 - 1), _INV),
    # ---- the request, with an output that is long enough: the refusal is its own
    (dict(out_bytes=2 ** 40, T=4097), _INV),                                      # L > CGNN_RANK_MAX_FRAMES
    (dict(out_bytes=2 ** 40, T=2 ** 20), _INV),
    (dict(out_bytes=2 ** 40, T=8192, window=4097, stride=1), _INV),
    (dict(out_bytes=2 ** 40, T=1), _INV),
    (dict(out_bytes=2 ** 40, window=1, stride=1), _INV),
    (dict(out_bytes=2 ** 40, window=51, stride=1), _INV),
    (dict(out_bytes=2 ** 40, window=20, stride=0), _INV),
    (dict(out_bytes=2 ** 40, window=-4, stride=1), _INV),
    (dict(out_bytes=2 ** 40, S=-1), _INV),
    (dict(out_bytes=2 ** 40, n=0), _INV),
    (dict(out_bytes=2 ** 40, n=-3), _INV),
    (dict(out_bytes=2 ** 40, S=_BIG_S), _INV),
    (dict(S=2 ** 22, window=2, stride=1), _INV),                                  # U * n >= 2^31 (and a short output)
    (dict(out_bytes=2 ** 40, n=2 ** 16), _INV),                                   # n * n >= 2^31
    # ---- the buffers
    (dict(out_bytes=2 ** 40, ts=None), _INV),
    (dict(out_bytes=2 ** 40, out=None), _INV),
    (dict(out_bytes=2 ** 40, ts=_A2), _INV),
    (dict(out_bytes=2 ** 40, out=_A2), _INV),
    # ---- S == 0: CGNN_OK before any buffer is looked at; the request comes before it
    (dict(S=0), _OK),
    (dict(_EMPTY), _OK),
    (dict(_EMPTY, T=4096), _OK),
    (dict(_EMPTY, window=20, stride=3), _OK),
    (dict(_EMPTY, T=4097), _INV),
    (dict(_EMPTY, T=1), _INV),
    (dict(_EMPTY, window=51, stride=1), _INV),
    (dict(_EMPTY, n=0), _INV),
    (dict(_EMPTY, out_bytes=-1), _INV),
]
_KEEP = [
    (dict(out_bytes=2 ** 40, keep=None), _INV),
    (dict(out_bytes=2 ** 40, keep_bytes=299), _INV),
    (dict(out_bytes=2 ** 40, keep_bytes=-1), _INV),
    (dict(out_bytes=2 ** 40, window=20, stride=10, keep_bytes=6 * 4 * 10), _INV),    # keep is [S, T] under a window too
    (dict(_EMPTY, keep=None, keep_bytes=0), _OK),
    (dict(_EMPTY, keep_bytes=-1), _INV),
]


def test_the_entry_points_check_their_arguments_before_any_launch():
    """No device is present here: a call that went as far as a launch could not return these codes.  (Every refused call
    keeps an output that is too short or has another argument out of order, so none can reach the launch on a machine
    that has a device either.)"""
    lib = _lib.load()
    got = []
    calls = [(name, c, w) for name in (_CALL, _MASKED) for c, w in _BOTH] + [(_MASKED, c, w) for c, w in _KEEP]
    for name, change, want in calls:
        args = dict(_DEFAULTS[name])
        unknown = set(change) - set(args)
        assert not unknown, (name, unknown)
        args.update(change)
        got.append((name, change, want, getattr(lib, name)(*args.values())))
    wrong = [(n, c, w, g) for n, c, w, g in got if g != w]
    assert not wrong, wrong
