"""The closed form of the node-feature gradient that csrc/fused_gcn_l0.hip implements (k_l0_bwd<WANT_G>, k_l0_dx),
against the oracle's own autograd (reference models.py:84-114 GCNLayer, BatchNorm1d in training mode) in fp64, on
the CPU.  With Y0 = (A_hat X0) W0^T + b, Z0 = BatchNorm(Y0) and dZ0 the gradient at Z0:

    dY0 = BatchNorm'(dZ0) = gamma invstd (dZ0 - mean(dZ0) - xhat mean(dZ0 xhat))
    G0  = dY0 W0             [N, F0]
    dX0 = A_hat^T G0         [N, F0]

and the same dX0 when the forward is evaluated in the centred form P0' = [A_hat (X0 - 1 c^T) | r - rbar],
W' = [W0 | W0 c] with arbitrary constants c, rbar: the function does not depend on them, so dX0 takes the
true W0 (the first F0 columns of W') and ignores the ones column.
"""
import pytest
import torch

from oracle import reference_path as O

EPS = 1e-5


def _graph(n, e, seed):
    """Random COO with duplicate edges, isolated nodes and nodes without in-edges."""
    g = torch.Generator().manual_seed(seed)
    live = max(2, n - 3)                                   # the last nodes get no edges at all
    src = torch.randint(0, live, (e,), generator=g)
    dst = torch.randint(0, live // 2 + 1, (e,), generator=g)   # upper half: no in-edges
    if e >= 4:
        src[-2:], dst[-2:] = src[:2], dst[:2]              # duplicates of the first two edges
    w = torch.rand(e, generator=g, dtype=torch.float64) + 0.1
    return torch.stack([src, dst]), w


def _ahat(n, ei, w):
    """The normalised operator, densely: A_hat[d, s] = dis[d] (A + I)[s, d] dis[s], source-side degree."""
    a = torch.zeros(n, n, dtype=torch.float64)
    a.index_put_((ei[0], ei[1]), w, accumulate=True)        # a[src, dst]
    a += torch.eye(n, dtype=torch.float64)
    dis = (a.sum(1) + 1e-8).pow(-0.5)
    return (dis[:, None] * a * dis[None, :]).t()


def _bn_backward(y, dz, gamma):
    """dY of training-mode BatchNorm (biased batch variance) from the gradient at its output."""
    mean, var = y.mean(0), y.var(0, unbiased=False)
    invstd = (var + EPS).rsqrt()
    xhat = (y - mean) * invstd
    return gamma * invstd * (dz - dz.mean(0) - xhat * (dz * xhat).mean(0))


def _fp64(fn):
    torch.set_default_dtype(torch.float64)
    try:
        return fn()
    finally:
        torch.set_default_dtype(torch.float32)


def _case(n, e, fin, fout, seed):
    ei, w = _graph(n, e, seed)
    g = torch.Generator().manual_seed(300 + seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = rnd(n, fin) * 3.0 + 20.0                            # features far from zero, as the centred form expects
    wt, b, gamma, beta, r = rnd(fout, fin), rnd(fout), rnd(fout), rnd(fout), rnd(n, fout)
    return ei, w, x, wt, b, gamma, beta, r


CASES = [(12, 40, 5, 8, 0), (30, 200, 8, 4, 1), (9, 3, 1, 3, 2), (50, 400, 7, 32, 3)]


@pytest.mark.parametrize("n,e,fin,fout,seed", CASES)
def test_closed_form_matches_oracle_autograd(n, e, fin, fout, seed):
    ei, w, x0, wt, b, gamma, beta, r = _case(n, e, fin, fout, seed)

    def run():
        x = x0.clone().requires_grad_(True)
        y = O.gcn_layer(x, ei, w, wt, b)
        z = torch.nn.functional.batch_norm(y, None, None, gamma, beta, True, 0.1, EPS)
        (torch.relu(z) * r).sum().backward()
        return x.grad, y.detach(), z.detach()
    want, y, z = _fp64(run)
    ah = _ahat(n, ei, w)
    assert float((ah @ x0 @ wt.t() + b - y).abs().max()) <= 1e-12 * float(y.abs().max())
    dz = r * (z > 0)
    got = ah.t() @ (_bn_backward(y, dz, gamma) @ wt)
    assert float((got - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("n,e,fin,fout,seed", [c for c in CASES if c[2] <= 7])
def test_centred_forward_leaves_the_gradient_unchanged(n, e, fin, fout, seed):
    ei, w, x0, wt, b, gamma, beta, r = _case(n, e, fin, fout, seed)
    ah = _ahat(n, ei, w)
    g = torch.Generator().manual_seed(400 + seed)
    c = torch.randn(fin, generator=g, dtype=torch.float64) * 5.0 + 18.0     # arbitrary constants
    rbar = float(torch.randn(1, generator=g, dtype=torch.float64)) + 1.0

    def grad_of(forward):
        x = x0.clone().requires_grad_(True)
        y = forward(x)
        z = torch.nn.functional.batch_norm(y, None, None, gamma, beta, True, 0.1, EPS)
        (torch.relu(z) * r).sum().backward()
        return x.grad, y.detach(), z.detach()

    def centred(x):
        ones = torch.ones(n, 1, dtype=torch.float64)
        p = torch.cat([ah @ (x - c), ah @ ones - rbar], 1)                  # P0'
        w_eff = torch.cat([wt, (wt @ c)[:, None]], 1)                       # W'
        return p @ w_eff.t() + (b + rbar * (wt @ c))                        # + mean_offset
    want, y, z = _fp64(lambda: grad_of(lambda x: O.gcn_layer(x, ei, w, wt, b)))
    via_centred, yc, _ = _fp64(lambda: grad_of(centred))
    assert float((yc - y).abs().max()) <= 1e-11 * float(y.abs().max())
    assert float((via_centred - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max()))
    # what the kernels compute in that form: dY0 from the rows rebuilt WITHOUT the constant term (BatchNorm is
    # invariant under a per-channel shift), narrowed with the first F0 columns of W' only
    y_c = yc - (b + rbar * (wt @ c))
    w_eff = torch.cat([wt, (wt @ c)[:, None]], 1)
    dy = _bn_backward(y_c, r * (z > 0), gamma)
    got = ah.t() @ (dy @ w_eff[:, :fin])
    assert float((got - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max()))
