"""The closed forms of the edge-weight gradient that csrc/edge_grad.hip implements, against the oracle's own
autograd (reference models.py:94-114 GCN, :146-149 GraphSAGE) in fp64, on the CPU.  Per edge e = (s -> d),
with X' the aggregate's input and dY the gradient at its output:

    g_e = <dY[d], X'[s]>
    GCN : ddis_i = sum_{src=i} g w dis[dst] + sum_{dst=i} g w dis[src] + 2 dis_i <dY[i], X'[i]>
          dw_e   = g_e dis_s dis_d - 1/2 dis_s^3 ddis_s
    SAGE: dw_e   = (g_e - <dY[d], agg[d]>) / (wsum_d + 1e-8)
"""
import pytest
import torch

from oracle import reference_path as O


def _graph(n, e, seed, dup=True):
    """Random COO with duplicate edges, isolated nodes and nodes without in-edges."""
    g = torch.Generator().manual_seed(seed)
    live = max(2, n - 3)                                   # the last nodes get no edges at all
    src = torch.randint(0, live, (e,), generator=g)
    dst = torch.randint(0, live // 2 + 1, (e,), generator=g)   # upper half: no in-edges
    if dup and e >= 4:
        src[-2:], dst[-2:] = src[:2], dst[:2]              # duplicates of the first two edges
    w = torch.rand(e, generator=g, dtype=torch.float64) + 0.1
    return torch.stack([src, dst]), w


def gcn_dw(xp, ei, w, dy):
    n = xp.shape[0]
    s, d = ei
    deg = torch.zeros(n, dtype=xp.dtype).index_add_(0, s, w) + 1.0
    dis = (deg + 1e-8).pow(-0.5)
    g = (dy[d] * xp[s]).sum(1)
    gself = (dy * xp).sum(1)
    ddis = (torch.zeros(n, dtype=xp.dtype).index_add_(0, s, g * w * dis[d])
            + torch.zeros(n, dtype=xp.dtype).index_add_(0, d, g * w * dis[s]) + 2.0 * dis * gself)
    return g * dis[s] * dis[d] - 0.5 * dis[s] ** 3 * ddis[s]


def sage_dw(x, ei, w, dy_agg, agg):
    n = x.shape[0]
    s, d = ei
    den = torch.zeros(n, dtype=x.dtype).index_add_(0, d, w) + 1e-8
    g = (dy_agg[d] * x[s]).sum(1)
    return (g - (dy_agg * agg).sum(1)[d]) / den[d]


def _fp64(fn):
    torch.set_default_dtype(torch.float64)
    try:
        return fn()
    finally:
        torch.set_default_dtype(torch.float32)


@pytest.mark.parametrize("n,e,fin,fout,seed", [(12, 40, 5, 8, 0), (30, 200, 16, 4, 1), (9, 3, 1, 3, 2),
                                               (50, 400, 7, 32, 3)])
def test_gcn_closed_form_matches_oracle_autograd(n, e, fin, fout, seed):
    ei, w0 = _graph(n, e, seed)
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(n, fin, generator=g, dtype=torch.float64)
    wt = torch.randn(fout, fin, generator=g, dtype=torch.float64)
    b = torch.randn(fout, generator=g, dtype=torch.float64)
    r = torch.randn(n, fout, generator=g, dtype=torch.float64)

    def run():
        w = w0.clone().requires_grad_(True)
        (O.gcn_layer(x, ei, w, wt, b) * r).sum().backward()
        return w.grad
    want = _fp64(run)
    got = gcn_dw(x @ wt.t(), ei, w0, r)           # X' = X W^T, dY = r
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # the aggregate-first form of layer 0 (A_hat X) W^T: the same edge gradient with X' = X, dY = r W
    got0 = gcn_dw(x, ei, w0, r @ wt)
    assert float((got0 - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("n,e,fin,fout,seed", [(12, 40, 5, 8, 0), (30, 200, 16, 4, 1), (9, 3, 1, 3, 2),
                                               (50, 400, 7, 32, 3)])
def test_sage_closed_form_matches_oracle_autograd(n, e, fin, fout, seed):
    ei, w0 = _graph(n, e, seed)
    g = torch.Generator().manual_seed(200 + seed)
    x = torch.randn(n, fin, generator=g, dtype=torch.float64)
    wt = torch.randn(fout, 2 * fin, generator=g, dtype=torch.float64)
    b = torch.randn(fout, generator=g, dtype=torch.float64)
    r = torch.randn(n, fout, generator=g, dtype=torch.float64)

    def run():
        w = w0.clone().requires_grad_(True)
        (O.sage_layer(x, ei, w, wt, b) * r).sum().backward()
        return w.grad
    want = _fp64(run)
    # the weighted mean and the gradient arriving at it (the Linear + ReLU after it: plain autograd)
    s, d = ei
    den = torch.zeros(n, dtype=torch.float64).index_add_(0, d, w0) + 1e-8
    agg = torch.zeros(n, fin, dtype=torch.float64).index_add_(0, d, x[s] * w0[:, None]) / den[:, None]
    a = agg.clone().requires_grad_(True)
    (torch.relu(torch.cat([x, a], 1) @ wt.t() + b) * r).sum().backward()
    got = sage_dw(x, ei, w0, a.grad, agg)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_layer_gradients_add_up_over_layers():
    """Two layers sharing one edge_weight: the total is the sum of the per-layer closed forms."""
    n, fin, h = 20, 4, 6
    ei, w0 = _graph(n, 90, 7)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n, fin, generator=g, dtype=torch.float64)
    w1, w2 = torch.randn(h, fin, generator=g, dtype=torch.float64), torch.randn(h, h, generator=g, dtype=torch.float64)
    b1, b2 = torch.randn(h, generator=g, dtype=torch.float64), torch.randn(h, generator=g, dtype=torch.float64)
    r = torch.randn(n, h, generator=g, dtype=torch.float64)

    def run():
        w = w0.clone().requires_grad_(True)
        (O.gcn_layer(O.gcn_layer(x, ei, w, w1, b1), ei, w, w2, b2) * r).sum().backward()
        return w.grad
    want = _fp64(run)
    y1 = _fp64(lambda: O.gcn_layer(x, ei, w0, w1, b1))
    # dY at layer 1's output through layer 2 with the weights held fixed: A_hat^T r W2 (dense fp64 form)
    a = torch.zeros(n, n, dtype=torch.float64)
    a.index_put_((ei[0], ei[1]), w0, accumulate=True)
    a += torch.eye(n, dtype=torch.float64)
    dis = (a.sum(1) + 1e-8).pow(-0.5)
    ahat = dis[:, None] * a * dis[None, :]
    dy1 = ahat @ (r @ w2)
    got = gcn_dw(y1 @ w2.t(), ei, w0, r) + gcn_dw(x @ w1.t(), ei, w0, dy1)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
