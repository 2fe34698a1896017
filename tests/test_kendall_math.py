"""The host statement of Kendall's tau (tests/kendall_data.py): against ``scipy.stats.kendalltau``, its diagonal against
the tie runs, its invariances; the constants and the tables that must not move; the argument checks of
``ingest.kendall_counts``, ``ingest.kendall_matrices`` and ``kendall=``; the header and the binding of cgnn_ingest_kendall
and the refusals of the C entry point, none of which reaches a launch.  No device is touched."""
import numpy as np
import pytest
import scipy.stats
import torch

from connectome_gnn_amd import _lib, ingest
from tests import kendall_data as KD
from tests import rank_data as RD
from tests.abi_header import check_header

S = 3


# ---- the statement ----
def _against_scipy(x, kept=None):
    """The largest |statement - scipy| over the pairs of columns of one unit, and whether the fp32 casts are equal."""
    x = np.asarray(x, dtype=np.float32)
    tau = KD.tau_of(KD.unit_counts(x, kept))
    xk = x if kept is None else x[kept]
    worst, same = 0.0, True
    for i in range(x.shape[1]):
        for j in range(i + 1, x.shape[1]):
            want = scipy.stats.kendalltau(xk[:, i].astype(np.float64), xk[:, j].astype(np.float64)).statistic
            assert not np.isnan(want), "no column of these series is constant"
            worst = max(worst, abs(tau[i, j] - want))
            same &= np.float32(tau[i, j]) == np.float32(want)
    return worst, same


@pytest.mark.parametrize("T,n", [(65, 5), (300, 9)])
def test_the_statement_is_scipys_kendalltau(T, n):
    """tau-b, ties and all: <= 1e-15 from scipy and equal as fp32, plain, quantised and under the random mask."""
    mask = RD.masks(10, T).numpy()[2]
    assert 0 < mask.sum() < T
    for name, x in (("plain", RD.plain(S, T, n).numpy()), ("quantised", KD.quantised(S, T, n).numpy())):
        for s in range(S):
            for kept in (None, mask):
                worst, same = _against_scipy(x[s], kept)
                assert worst <= 1e-15 and same, (name, s, kept is not None, worst)


def test_the_diagonal_counts_the_untied_pairs():
    for T, n in ((65, 5), (129, 33)):
        x = RD.series(S, T, n).numpy()
        g = KD.series_counts(S, T, n)
        m = RD.masks(S, T).numpy()
        gm = KD.host_counts(x, m)
        at = RD.nan_at(S, n)
        for s in range(S):
            for i in range(n):
                if at == (s, i):
                    assert g[s, i, i] == -1 and not g[s, i, :i].any() and not g[s, :i, i].any()
                    assert not g[s, i, i + 1:].any() and not g[s, i + 1:, i].any()
                    continue
                assert g[s, i, i] == T * (T - 1) // 2 - KD.tie_pairs(x[s, :, i]) >= 0
                if not np.isnan(x[s, m[s], i]).any():
                    Lu = int(m[s].sum())
                    assert gm[s, i, i] == Lu * (Lu - 1) // 2 - KD.tie_pairs(x[s, m[s], i]) >= 0
            assert (g[s] == g[s].T).all()
        c = RD.SPECIAL["constant"]
        assert g[c % S, c, c] == 0 and not g[c % S, c].any(), "a constant column: every pair is tied"
        tau = KD.tau_of(g)
        assert not tau[c % S, c].any() and not tau[c % S, :, c].any(), "an exact zero row and column, diagonal included"
        d = RD.SPECIAL["descending"]
        assert g[d % S, d, d] == T * (T - 1) // 2 and tau[d % S, d, d] == 1.0
        if at is not None:
            assert np.isnan(tau[at[0], at[1]]).all() and np.isnan(tau[at[0], :, at[1]]).all()
            assert np.isnan(tau).sum() == 2 * n - 1, "its row and column of its unit, nothing else"
        ok = ~np.isnan(tau)
        assert (np.abs(tau[ok]) <= 1.0).all()


def test_the_counts_see_only_the_order_of_the_kept_frames():
    T, n = 65, 5
    x = RD.plain(S, T, n).numpy()
    g = KD.host_counts(x)
    perm = np.random.default_rng(3).permutation(T)
    assert (KD.host_counts(x[:, perm]) == g).all(), "a permutation of the frames"
    assert (KD.host_counts(x ** 3) == g).all(), "a strictly increasing map"
    m = RD.masks(10, T).numpy()[2]
    poisoned = x.copy()
    poisoned[:, ~m] = np.nan
    assert (KD.host_counts(poisoned, np.broadcast_to(m, (S, T))) == KD.host_counts(x[:, m])).all()
    for few in ([], [7]):                         # fewer than two kept frames: no pair
        k = np.zeros(T, dtype=bool)
        k[few] = True
        assert not KD.unit_counts(x[0], k).any()


def test_tau_of_the_spike_pair_beside_its_pearson_correlation():
    """The README's example: ROIs 0 and 1 share 20 spiky frames of 300 and nothing else.  Pearson r = 0.976; tau-b,
    which counts pairs of frames and not their sizes, stays below 0.2 as Spearman's rho (0.154) does."""
    x = RD.spike_pair()[0].numpy()
    r = np.corrcoef(x[:, 0].astype(np.float64), x[:, 1].astype(np.float64))[0, 1]
    tau = KD.tau_of(KD.unit_counts(x))[0, 1]
    want = scipy.stats.kendalltau(x[:, 0].astype(np.float64), x[:, 1].astype(np.float64)).statistic
    assert abs(r - 0.976) < 1e-3 and abs(tau - want) <= 1e-15 and 0.0 < tau < 0.2, (r, tau)


def test_the_constants_and_what_must_not_move():
    assert ingest.KENDALL_MAX_FRAMES == KD.MAX_FRAMES == ingest.RANK_MAX_FRAMES == 4096
    assert ingest.KINDS == ("correlation", "partial"), "tau is an argument, not a kind"
    assert ingest.SHRINKAGES == ("ledoit_wolf",)
    assert len(_lib.PROTOTYPES) == 127
    assert list(_lib.KENDALL_PROTOTYPES) == ["cgnn_ingest_kendall"]
    assert list(_lib.RANK_PROTOTYPES) == ["cgnn_ingest_rank", "cgnn_ingest_rank_masked"]
    import connectome_gnn_amd
    assert not {"kendall_counts", "kendall_matrices", "KENDALL_MAX_FRAMES"} & set(connectome_gnn_amd.__all__)
    with pytest.raises(ValueError, match="unknown kind"):
        ingest.correlation_matrices(RD.plain(S, 9, 5), kind="kendall")


# ---- the Python arguments ----
def test_the_kendall_calls_and_kendall_check_their_arguments():
    x = RD.plain(S, 30, 5)
    y = torch.arange(S) % 2
    for bad in ("yes", 1, 0, None, 1.0):
        with pytest.raises(TypeError, match="kendall must be a bool"):
            ingest.correlation_matrices(x, kendall=bad)
        with pytest.raises(TypeError, match="kendall must be a bool"):
            ingest.from_timeseries(x, y, keep=0.5, kendall=bad)
    with pytest.raises(ValueError, match="function of the ranks alone"):
        ingest.correlation_matrices(x, kendall=True, rank=True)
    with pytest.raises(ValueError, match="function of the ranks alone"):
        ingest.from_timeseries(x, y, keep=0.5, kendall=True, rank=True)
    with pytest.raises(ValueError, match="frames of a Pearson correlation matrix"):
        ingest.correlation_matrices(x, kendall=True, kind="partial", shrinkage="ledoit_wolf")
    with pytest.raises(ValueError, match="frames of a Pearson correlation matrix"):
        ingest.from_timeseries(x, y, keep=0.5, kendall=True, kind="partial", shrinkage="ledoit_wolf")
    with pytest.raises(ValueError, match='shrinkage applies to kind="partial"'):
        ingest.correlation_matrices(x, kendall=True, shrinkage=0.1)
    long = torch.zeros(1, 4097, 2)
    for call in (lambda: ingest.kendall_counts(long), lambda: ingest.kendall_matrices(long),
                 lambda: ingest.correlation_matrices(long, kendall=True),
                 lambda: ingest.from_timeseries(long, torch.zeros(1, dtype=torch.long), keep=0.5, kendall=True)):
        with pytest.raises(ValueError, match="at most KENDALL_MAX_FRAMES = 4096 frames.*rank shorter windows"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # the window is what is counted
        ingest.kendall_counts(long, window=4096)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # and without kendall=True nothing is
        ingest.correlation_matrices(long, kendall=False)
    # the series, the window and the mask are checked as everywhere
    for fn in (ingest.kendall_counts, ingest.kendall_matrices):
        with pytest.raises(TypeError, match="float32"):
            fn(x.double())
        with pytest.raises(TypeError, match="timeseries must be a torch.Tensor"):
            fn(x.numpy())
        with pytest.raises(ValueError, match=r"window must lie in \[2, T\]"):
            fn(x, window=31)
        with pytest.raises(ValueError, match="give window= with it"):
            fn(x, stride=3)
        with pytest.raises(TypeError, match="sample_mask must be bool"):
            fn(x, sample_mask=torch.ones(S, 30))
        with pytest.raises(ValueError, match=r"sample_mask must be \[S, T\]"):
            fn(x, sample_mask=torch.ones(S, 29, dtype=torch.bool))
        with pytest.raises(ValueError, match="timeseries must be contiguous"):
            fn(torch.zeros(S, 5, 30).transpose(1, 2))
    # a valid request gets as far as the device check: there is no CPU path
    m = RD.masks(S, 30)
    for call in (lambda: ingest.kendall_counts(x), lambda: ingest.kendall_matrices(x, absolute=True),
                 lambda: ingest.kendall_counts(x, window=10, stride=3, sample_mask=m),
                 lambda: ingest.kendall_matrices(x, window=10, sample_mask=m),
                 lambda: ingest.correlation_matrices(x, kendall=True),
                 lambda: ingest.correlation_matrices(x, kendall=True, kind="partial", shrinkage=0.1, window=12),
                 lambda: ingest.correlation_matrices(x, kendall=True, kind="partial", shrinkage=torch.full((S,), 0.1)),
                 lambda: ingest.from_timeseries(x, y, keep=0.5, kendall=True),
                 lambda: ingest.from_timeseries(x, y, knn=2, kendall=True, sample_mask=m)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- the C ABI ----
def test_the_prototype_matches_its_header_type_by_type():
    hdr = check_header("cgnn_kendall.h", _lib.KENDALL_PROTOTYPES, ["cgnn_ingest_kendall"],
                       [("int32_t absolute, ", ""), ("int32_t* counts", "int32_t counts"), ("int64_t U", "int32_t U")])
    lib = _lib.load()
    assert f"#define CGNN_KENDALL_MAX_FRAMES {ingest.KENDALL_MAX_FRAMES}\n" in hdr
    assert _lib.ABI_VERSION == 2 and lib.cgnn_abi_version() == 2, "the change is additive"
    assert list(_lib.HEADERS)[-1] == "cgnn_kendall.h"


_A, _A2 = 0x1000, 0x1002                    # 4-byte aligned / not: never dereferenced
_INV, _OK = _lib.CGNN_EINVAL, _lib.CGNN_OK
_BIG_U = 2 ** 31 // 20 + 1                  # U * n >= 2^31 at n = 20
_FULL = 6 * 20 * 20 * 4
# defaults that pass every check but the byte counts of both outputs: 6 units of 50 frames and 20 ROIs, one byte short
_DEFAULTS = dict(ranks=_A, U=6, L=50, n=20, absolute=0, counts=_A, counts_bytes=_FULL - 1, out=_A, out_bytes=_FULL - 1,
                 stream=None)
_LONG = dict(counts_bytes=2 ** 40, out_bytes=2 ** 40)
_EMPTY = dict(ranks=None, U=0, counts=None, counts_bytes=0, out=None, out_bytes=0)
_CASES = [
    # ---- everything is in order but an output, which is one byte short
    (dict(), _INV),
    (dict(counts_bytes=_FULL), _INV),                                             # out is short
    (dict(out_bytes=_FULL), _INV),                                                # counts are
    (dict(counts=None, counts_bytes=0), _INV),                                    # out alone, short
    (dict(out=None, out_bytes=0), _INV),                                          # counts alone, short
    (dict(counts_bytes=0, out_bytes=_FULL), _INV),
    (dict(counts_bytes=-1, out_bytes=_FULL), _INV),
    (dict(counts_bytes=_FULL, out_bytes=-1), _INV),
    (dict(counts=None, counts_bytes=-1, out_bytes=_FULL), _INV),                  # a negative count is refused as such
    (dict(L=4096), _INV),
    # ---- the request, with outputs that are long enough: the refusal is its own
    (dict(_LONG, L=4097), _INV),                                                  # L > CGNN_KENDALL_MAX_FRAMES
    (dict(_LONG, L=2 ** 20), _INV),
    (dict(_LONG, L=1), _INV),
    (dict(_LONG, L=0), _INV),
    (dict(_LONG, L=-5), _INV),
    (dict(_LONG, U=-1), _INV),
    (dict(_LONG, n=0), _INV),
    (dict(_LONG, n=-3), _INV),
    (dict(_LONG, U=_BIG_U), _INV),                                                # U * n >= 2^31
    (dict(_LONG, n=2 ** 16), _INV),                                               # n * n >= 2^31
    # ---- the buffers
    (dict(_LONG, ranks=None), _INV),
    (dict(_LONG, counts=None, out=None), _INV),                                   # at least one output
    (dict(counts=None, counts_bytes=0, out=None, out_bytes=0), _INV),
    (dict(_LONG, ranks=_A2), _INV),
    (dict(_LONG, counts=_A2), _INV),
    (dict(_LONG, out=_A2), _INV),
    # ---- U == 0: CGNN_OK before any buffer is looked at; the request comes before it
    (dict(U=0), _OK),
    (dict(_EMPTY), _OK),
    (dict(_EMPTY, L=4096), _OK),
    (dict(_EMPTY, L=4097), _INV),
    (dict(_EMPTY, L=1), _INV),
    (dict(_EMPTY, n=0), _INV),
    (dict(_EMPTY, out_bytes=-1), _INV),
    (dict(_EMPTY, counts_bytes=-1), _INV),
]


def test_the_entry_point_checks_its_arguments_before_any_launch():
    """No device is present here: a call that went as far as a launch could not return these codes.  (Every refused call
    keeps an output that is too short or has another argument out of order, so none can reach the launch on a machine
    that has a device either.)"""
    lib = _lib.load()
    got = []
    for change, want in _CASES:
        args = dict(_DEFAULTS)
        unknown = set(change) - set(args)
        assert not unknown, unknown
        args.update(change)
        got.append((change, want, lib.cgnn_ingest_kendall(*args.values())))
    wrong = [(c, w, g) for c, w, g in got if g != w]
    assert not wrong, wrong
