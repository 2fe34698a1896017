"""connectome_gnn_amd.ingest's time-series entry points without a GPU: the host statement (tests/timeseries_data.py)
against numpy.corrcoef and against itself on slices, its conventions, what the tolerance of the device tests is
made of, and every refusal of ``correlation_matrices`` / ``from_timeseries``."""
import numpy as np
import pytest
import torch

from connectome_gnn_amd import ingest
from tests import timeseries_data as D

SHAPES = [(3, 2), (7, 20), (33, 65), (70, 84), (40, 360)]


@pytest.mark.parametrize("T,n", SHAPES)
def test_statement_equals_numpy_corrcoef(T, n):
    ts = D.recipe(3, T, n)
    got = D.host_corr(ts)
    assert got.shape == (3, n, n) and got.dtype == torch.float64
    for s in range(3):
        want = np.corrcoef(ts[s].double().numpy(), rowvar=False)
        assert float(np.abs(got[s].numpy() - want).max()) <= 1e-12
        assert torch.equal(got[s].diagonal(), torch.ones(n, dtype=torch.float64))
    assert torch.equal(D.host_corr(ts, absolute=True), got.abs())


@pytest.mark.parametrize("L,st", [(50, None), (20, None), (20, 7), (2, 1)])
def test_windowed_statement_is_the_statement_on_slices_in_unit_order(L, st):
    S, T, n = 3, 50, 20
    ts = D.recipe(S, T, n)
    step = L if st is None else st
    W = D.num_windows(T, L, st)
    assert W == {(50, None): 1, (20, None): 2, (20, 7): 5, (2, 1): 49}[(L, st)]
    got = D.host_corr(ts, window=L, stride=st)
    assert got.shape == (S * W, n, n)
    for s in range(S):
        for w in range(W):
            want = D.host_corr(ts[s:s + 1, w * step:w * step + L].contiguous())[0]
            assert torch.equal(got[s * W + w], want), (s, w)          # unit u = s * W + w
    assert ingest._check_timeseries(ts, L, st) == (S, T, n, L, step, W)


def test_zero_variance_convention():
    S, T, n = 3, 31, 63
    ts = D.planted(S, T, n)
    r = D.host_corr(ts)
    assert not bool(torch.isnan(r).any())
    for c in (1, n - 2):
        assert torch.equal(r[-1, c], torch.zeros(n, dtype=torch.float64))
        assert torch.equal(r[-1, :, c], torch.zeros(n, dtype=torch.float64))
    others = [i for i in range(n) if i not in (1, n - 2)]
    assert torch.equal(r[-1].diagonal()[others], torch.ones(n - 2, dtype=torch.float64))
    assert torch.equal(r[:-1], D.host_corr(D.recipe(S, T, n))[:-1])     # the other subjects are the recipe's


def _emulate_fp32(ts, raw_moments):
    """What an fp32 product gives: the definition (fp64 statistics, fp32 centring, scaling and product), or the
    raw-moment formula E[xy] - E[x]E[y] in fp32."""
    out = []
    for x in ts:
        L = x.shape[0]
        if raw_moments:
            sxy, sx = x.t() @ x, x.sum(0)
            cov = sxy - sx[:, None] * sx[None, :] / L
            sd = torch.sqrt(cov.diagonal())
            out.append(cov / (sd[:, None] * sd[None, :]))
        else:
            m = x.double().mean(0)
            q = ((x.double() - m) ** 2).sum(0)
            z = (x - m.float()) * (1.0 / torch.sqrt(q)).float()
            out.append(z.t() @ z)
    return torch.stack(out).double()


def test_tolerance_holds_for_the_definition_and_not_for_raw_moments():
    off = ~torch.eye(84, dtype=torch.bool)
    for offset in (0.0, 1000.0):
        ts = D.recipe(3, 70, 84, offset=offset)
        k = D.kappa(ts)
        assert (k > 900.0) == (offset == 1000.0)
        tol = D.atol(70, k)
        want = D.host_corr(ts)
        err = float((_emulate_fp32(ts, False) - want)[:, off].abs().max())
        assert err <= tol, (offset, err, tol)
    assert 4e-4 < tol < 6e-4
    err = float((_emulate_fp32(ts, True) - want)[:, off].nan_to_num(nan=2.0).abs().max())
    assert err > 10 * tol, (err, tol)


# ---- refusals -------------------------------------------------------------------------------------------------
def _ts():
    return D.recipe(3, 7, 20)


def _huge(shape):
    return torch.zeros(1).expand(*shape)      # no storage behind it


BAD = [
    ("not a tensor", lambda: (_ts().numpy(), {}), TypeError, "torch.Tensor"),
    ("dtype", lambda: (_ts().double(), {}), TypeError, "float32"),
    ("rank 2", lambda: (_ts()[0], {}), ValueError, r"\[S, T, n\]"),
    ("rank 4", lambda: (_ts()[None], {}), ValueError, r"\[S, T, n\]"),
    ("n = 0", lambda: (torch.zeros(3, 7, 0), {}), ValueError, r"\[S, T, n\]"),
    ("T = 1", lambda: (_ts()[:, :1].contiguous(), {}), ValueError, "T >= 2"),
    ("T = 0", lambda: (torch.zeros(3, 0, 20), {}), ValueError, "T >= 2"),
    ("window = 1", lambda: (_ts(), {"window": 1}), ValueError, "window must lie in"),
    ("window = 0", lambda: (_ts(), {"window": 0}), ValueError, "window must lie in"),
    ("window < 0", lambda: (_ts(), {"window": -3}), ValueError, "window must lie in"),
    ("window > T", lambda: (_ts(), {"window": 8}), ValueError, "window must lie in"),
    ("window a float", lambda: (_ts(), {"window": 3.0}), TypeError, "window must be an int"),
    ("window a bool", lambda: (_ts(), {"window": True}), TypeError, "window must be an int"),
    ("stride = 0", lambda: (_ts(), {"window": 3, "stride": 0}), ValueError, "stride must be >= 1"),
    ("stride < 0", lambda: (_ts(), {"window": 3, "stride": -1}), ValueError, "stride must be >= 1"),
    ("stride a float", lambda: (_ts(), {"window": 3, "stride": 1.5}), TypeError, "stride must be an int"),
    ("stride without window", lambda: (_ts(), {"stride": 2}), ValueError, "give window="),
    ("U * n >= 2^31", lambda: (_huge((2 ** 29, 2, 4)), {}), ValueError, r"units \* n"),
    ("U * n >= 2^31 by windows", lambda: (_huge((2 ** 20, 2 ** 10, 4)), {"window": 2, "stride": 1}), ValueError,
     r"units \* n"),
    ("n * n >= 2^31", lambda: (_huge((1, 2, 46341)), {}), ValueError, r"n \* n"),
    ("not contiguous", lambda: (_ts().transpose(1, 2), {}), ValueError, "contiguous"),
    ("a strided slice", lambda: (_ts()[:, ::2], {}), ValueError, "contiguous"),
]


@pytest.mark.parametrize("name,make,exc,msg", BAD, ids=[b[0] for b in BAD])
def test_malformed_timeseries_are_refused(name, make, exc, msg):
    ts, kw = make()
    S = ts.shape[0] if isinstance(ts, torch.Tensor) and ts.dim() == 3 and ts.shape[0] < 100 else 1
    with pytest.raises(exc, match=msg):
        ingest.correlation_matrices(ts, **kw)
    with pytest.raises(exc, match=msg):
        ingest.from_timeseries(ts, torch.zeros(S, dtype=torch.long), keep=0.1, **kw)


def test_cpu_timeseries_are_refused():
    ts, y = _ts(), torch.zeros(3, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.correlation_matrices(ts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.correlation_matrices(ts, window=3, stride=2, absolute=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.from_timeseries(ts, y, keep=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.from_timeseries(ts, y, min_weight=torch.zeros(9), window=3, stride=2,
                               node_features=torch.zeros(9, 20, 4))


def test_threshold_arguments_are_refused():
    ts, y = _ts(), torch.zeros(3, dtype=torch.long)
    for kw in ({}, {"keep": 0.1, "num_edges": 3}, {"keep": 0.1, "min_weight": 0.2},
               {"num_edges": 3, "min_weight": 0.2}, {"keep": 0.1, "num_edges": 3, "min_weight": 0.2}):
        with pytest.raises(ValueError, match="exactly one"):
            ingest.from_timeseries(ts, y, **kw)
    for keep in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"keep must lie in \[0, 1\]"):
            ingest.from_timeseries(ts, y, keep=keep)
    with pytest.raises(ValueError, match="num_edges must be >= 0"):
        ingest.from_timeseries(ts, y, num_edges=-1)
    with pytest.raises(TypeError, match="num_edges must be an int"):
        ingest.from_timeseries(ts, y, num_edges=2.5)
    for bad in (torch.zeros(2), torch.zeros(3, 1), torch.zeros(3, dtype=torch.long)):
        with pytest.raises(ValueError, match="min_weight tensor"):
            ingest.from_timeseries(ts, y, min_weight=bad)
    with pytest.raises(ValueError, match="min_weight tensor"):          # one threshold per UNIT
        ingest.from_timeseries(ts, y, min_weight=torch.zeros(3), window=3, stride=2)


def test_labels_and_features_are_refused():
    ts, y = _ts(), torch.arange(3, dtype=torch.long) % 2
    for bad in (y.int(), y.float(), y[:2], y.view(3, 1), y.tolist(), y.repeat_interleave(3)):
        with pytest.raises(ValueError, match=r"labels must be an int64 tensor \[S\]"):
            ingest.from_timeseries(ts, bad, keep=0.1, window=3, stride=2)       # labels are per SUBJECT
    for bad in (torch.zeros(9, 20, 4).double(), torch.zeros(3, 20, 4), torch.zeros(9, 19, 4), torch.zeros(9, 20)):
        with pytest.raises(ValueError, match=r"node_features must be a float32 tensor \[U, n, F\]"):
            ingest.from_timeseries(ts, y, keep=0.1, window=3, stride=2, node_features=bad)   # ... per UNIT
