"""GPU parity of the drop-in models against the goldens recorded from the reference
(G2-G7) and against the oracle on fresh seeded inputs.  Tolerance 1e-5 (north_star)."""
import numpy as np
import pytest
import torch

from oracle import reference_path as O
from tests import golden_util as G
from tests import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = P.TOL
GTOL = P.GTOL     # gradients: same bars as the oracle-vs-golden test; see tests/parity.py


def _cbatch(bd):
    from connectome_gnn_amd import ConnectomeBatch
    return ConnectomeBatch(bd["node_features"], bd["edge_index"], bd["edge_weight"], bd["batch"],
                           bd.get("labels"), bd["ptr"])


def _model(kind, in_ch, hidden, **kw):
    import connectome_gnn_amd as C
    return (C.GCNConnectome if kind == "gcn" else C.GraphSAGEConnectome)(in_ch, hidden, **kw)


@pytest.mark.parametrize("name", ["gcn", "sage"])
@pytest.mark.parametrize("tag", ["sum", "cot"])
def test_g2_layers(name, tag):
    from connectome_gnn_amd.models import GCNLayer, SAGELayer
    d = G.load("g2_layers_6node.npz")
    layer = (GCNLayer if name == "gcn" else SAGELayer)(4, 7)
    layer.load_state_dict(G.group(d, f"{name}_param"))
    layer = layer.to(DEV)
    x = torch.from_numpy(d["x"]).to(DEV).requires_grad_(True)
    ei, ew = torch.from_numpy(d["edge_index"]).to(DEV), torch.from_numpy(d["edge_weight"]).to(DEV)
    out = layer(x, ei, ew)
    c = torch.ones_like(out) if tag == "sum" else torch.from_numpy(d["cotangent"]).to(DEV)
    (out * c).sum().backward()
    g = G.group(d, f"{name}_{tag}")
    torch.testing.assert_close(out.cpu(), g["out"], **TOL)
    torch.testing.assert_close(x.grad.cpu(), g["dx"], **TOL)
    torch.testing.assert_close(layer.linear.weight.grad.cpu(), g["d_linear.weight"], **TOL)
    bias = layer.bias if name == "gcn" else layer.linear.bias
    torch.testing.assert_close(bias.grad.cpu(), g["d_bias" if name == "gcn" else "d_linear.bias"], **TOL)


FILES = [("g3_models_8x20_h32.npz", 32, 32), ("g4_models_4x84_h64.npz", 64, 64),
         ("g5_models_2x360.npz", 64, 128), ("g6_mixed_20_35_84.npz", 32, 32)]


@pytest.mark.parametrize("fname,h_gcn,h_sage", FILES)
@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_models_vs_golden(fname, h_gcn, h_sage, kind):
    d = G.load(fname)
    b = _cbatch(G.group(d, "batch")).to(DEV)
    hidden = h_gcn if kind == "gcn" else h_sage
    torch.manual_seed(42)
    m = _model(kind, 5, hidden)
    init = G.group(d, f"{kind}_init")
    for k, v in m.state_dict().items():
        assert torch.equal(v, init[k]), k          # a7/a9: same init stream as the reference
    m = m.to(DEV).eval()
    with torch.no_grad():
        torch.testing.assert_close(m(b).cpu(), G.group(d, f"{kind}_eval")["logits"], **TOL)
        torch.testing.assert_close(m.encode(b).cpu(), G.group(d, f"{kind}_eval")["encode"], **TOL)
    torch.manual_seed(42)
    m = _model(kind, 5, hidden, dropout=0.0).to(DEV).train()
    logits = m(b)
    loss = torch.nn.functional.cross_entropy(logits, b.labels)
    loss.backward()
    tr = G.group(d, f"{kind}_train")
    torch.testing.assert_close(logits.cpu(), tr["logits"], **TOL)
    torch.testing.assert_close(loss.cpu(), tr["loss"], **TOL)
    grads = dict(m.named_parameters())
    for k, g in G.group(d, f"{kind}_grad").items():
        torch.testing.assert_close(grads[k].grad.cpu(), g, **GTOL, msg=lambda s: f"{k}: {s}")
    sd = m.state_dict()
    for k, v in G.group(d, f"{kind}_after").items():
        torch.testing.assert_close(sd[k].cpu(), v, **TOL)


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_g7_trainer_trajectory(kind):
    import connectome_gnn_amd as C
    d = G.load("g7_trainer_40x20.npz")
    gs = [C.ConnectomeGraph(*g) for g in G.split_graphs(G.group(d, "all"), d["edge_counts"])]
    torch.manual_seed(42)
    m = _model(kind, 5, 32, dropout=0.0)
    tr = C.Trainer(m, torch.optim.Adam(m.parameters(), lr=1e-3), device=DEV)
    hist = tr.fit(C.ConnectomeDataLoader(gs[:30], batch_size=10, shuffle=False),
                  C.ConnectomeDataLoader(gs[30:], batch_size=10, shuffle=False),
                  num_epochs=3, patience=8, verbose=False)
    gh = G.group(d, f"{kind}_hist")
    np.testing.assert_allclose(hist["train_loss"], gh["train_loss"].numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(hist["val_loss"], gh["val_loss"].numpy(), rtol=1e-4, atol=1e-5)
    ev = tr.evaluate(C.ConnectomeDataLoader(gs[30:], batch_size=10, shuffle=False))
    assert ev["total"] == 10 and 0.0 <= ev["accuracy"] <= 1.0
    sd = m.state_dict()
    for k, v in G.group(d, f"{kind}_final").items():
        if kind == "gcn" and (k.startswith("convs.") and k.endswith(".bias") or "running_mean" in k):
            continue    # zero-true-gradient bias ahead of BN: chaotic in the reference itself
        torch.testing.assert_close(sd[k].cpu(), v, rtol=1e-4, atol=2e-5, msg=lambda s: f"{k}: {s}")


@pytest.mark.parametrize("kind,n,k,hidden,nb", [("gcn", 84, 8, 64, 32), ("sage", 84, 8, 64, 16),
                                               ("gcn", 360, 14, 64, 8), ("sage", 360, 14, 128, 4),
                                               ("gcn", 50, 6, 256, 3), ("sage", 50, 6, 256, 3),
                                               ("sage", 100, 10, 128, 48), ("gcn", 100, 10, 128, 48),
                                               # >= 4096 rows at hidden 256: every weight-stationary GEMM form
                                               # (two halves, packed layer-0 panel, per-panel weight gradient)
                                               ("sage", 100, 10, 256, 48), ("gcn", 100, 10, 256, 48),
                                               # (16 graphs, not 12: at 12 x 360 rows ONE ReLU pre-activation of
                                               # GraphSAGE's last layer, channel 133, sits within rounding of 0 and
                                               # the split-bf16 GEMM lands on the other side of it than every fp32
                                               # CPU order -- 2 % of that channel's bias gradient, same value on the
                                               # fused and the layered path; tools/_bin probe)
                                               ("sage", 360, 14, 256, 16), ("gcn", 360, 14, 256, 16)])
def test_models_vs_oracle_fresh(kind, n, k, hidden, nb):
    """Seeded fresh inputs (our generator), train mode dropout 0: logits, loss, all grads.

    A gradient passes if it is within GTOL of the fp32 oracle, or -- where the fp32 CPU arithmetic
    of the reference is itself the noisy side (a ReLU pre-activation within rounding of 0 moves a
    weight gradient by ~1e-5) -- if it is at least as close to the oracle evaluated in fp64 as the
    fp32 oracle is."""
    import connectome_gnn_amd as C
    b = C.collate_graphs(C.generate_dataset(nb, n, k, seed=123))
    torch.manual_seed(7)
    m = _model(kind, 5, hidden, dropout=0.0)
    lo, loss_o, g32, _ = P.oracle_run(kind, m.state_dict(), b)
    _, _, g64, _ = P.oracle_run(kind, m.state_dict(), b, dtype=torch.float64)
    m = m.to(DEV).train()
    bd = b.to(DEV)
    lg = m(bd)
    loss_g = torch.nn.functional.cross_entropy(lg, bd.labels)
    loss_g.backward()
    torch.testing.assert_close(lg.cpu(), lo, **TOL)
    torch.testing.assert_close(loss_g.cpu(), loss_o, **TOL)
    floor = P.NoiseFloor(kind, m.state_dict(), b)
    for k_, p in m.named_parameters():
        P.assert_grad(k_, p.grad, g32[k_], g64[k_], f"fresh-{kind}-{n}-h{hidden}", floor)


def test_resident_assemble_matches_collate():
    import connectome_gnn_amd as C
    from connectome_gnn_amd.resident import assemble_batch
    from connectome_gnn_amd.synthetic import generate_packed
    ds = generate_packed(12, 20, 4, seed=5)
    ids = torch.tensor([7, 0, 3, 11])
    want = C.collate_graphs([ds.graph(int(i)) for i in ids])
    got = assemble_batch(ds.to(DEV), ids)
    for f in ("node_features", "edge_index", "edge_weight", "batch", "labels", "ptr"):
        assert torch.equal(getattr(got, f).cpu(), getattr(want, f)), f


def test_dropout_train_mode_statistics():
    """Dropout masks cannot match the CPU oracle (different RNG); check the contract instead:
    eval is deterministic, train-mode outputs are finite and vary run to run."""
    import connectome_gnn_amd as C
    b = C.collate_graphs(C.generate_dataset(16, 84, 8, seed=3)).to(DEV)
    torch.manual_seed(0)
    m = C.GCNConnectome(5, 64).to(DEV)
    m.train()
    a, c = m(b), m(b)
    assert torch.isfinite(a).all() and not torch.equal(a, c)
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(b), m(b))


# ----------------------------------------------------------------------------- fused GCN path
def _oracle_grads(kind, model, b, training=True):
    st = O.require_grad({k_: v.clone() for k_, v in model.state_dict().items()})
    ob = O.OBatch(b.node_features, b.edge_index, b.edge_weight, b.batch, b.labels, b.ptr)
    lo = O.FORWARD[kind](st, ob, 0.0, training)
    loss = torch.nn.functional.cross_entropy(lo, ob.labels)
    loss.backward()
    return lo, loss, st


@pytest.mark.parametrize("sizes,k,f0,layers", [
    ([84] * 8, 8, 5, 3), ([360] * 3, 14, 5, 3), ([20] * 70, 4, 5, 3), ([20, 35, 84, 7, 360, 1, 2], 4, 5, 3),
    ([100] * 5, 10, 1, 1), ([64] * 9, 6, 16, 2), ([384, 383, 17], 12, 7, 4)])
def test_fused_gcn_vs_oracle(sizes, k, f0, layers):
    import connectome_gnn_amd as C
    gs = []
    for i, n in enumerate(sizes):
        g = C.generate_connectome(max(n, 1), min(k, max(2 * ((n - 1) // 2), 0)), seed=100 + i) if n > 2 \
            else C.ConnectomeGraph(torch.randn(n, 5), torch.zeros(2, 0, dtype=torch.long),
                                   torch.zeros(0), torch.tensor(i % 2))
        x = torch.randn(n, f0, generator=torch.Generator().manual_seed(i))
        gs.append(C.ConnectomeGraph(x, g.edge_index, g.edge_weight, torch.tensor(i % 2)))
    b = C.collate_graphs(gs)
    torch.manual_seed(5)
    m = C.GCNConnectome(f0, 64, 2, layers, dropout=0.0, impl="fused")
    with torch.no_grad():                       # non-trivial BN affine + bias so every term counts
        for bn in m.batch_norms:
            bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.3, 0.3)
        for cv in m.convs:
            cv.bias.uniform_(-0.2, 0.2)
    lo, loss_o, st = _oracle_grads("gcn", m, b)
    m = m.to(DEV).train()
    bd = b.to(DEV)
    lg = m(bd)
    assert m.impl_used == "fused"
    loss_g = torch.nn.functional.cross_entropy(lg, bd.labels)
    loss_g.backward()
    torch.testing.assert_close(lg.cpu(), lo, **TOL)
    torch.testing.assert_close(loss_g.cpu(), loss_o, **TOL)
    for k_, p in m.named_parameters():
        want = st[k_].grad
        torch.testing.assert_close(p.grad.cpu(), want, rtol=1e-4,
                                   atol=2e-6 + 1e-5 * float(want.abs().max()),
                                   msg=lambda s: f"{k_}: {s}")
    sd = m.state_dict()
    for k_, v in st.items():
        if "running" in k_ or "num_batches" in k_:
            torch.testing.assert_close(sd[k_].cpu(), v.detach(), **TOL)
    # eval mode uses the running statistics
    m.eval()
    with torch.no_grad():
        le = m(bd)
        lo_e = O.gcn_forward({k_: v.detach() for k_, v in st.items()}, O.OBatch(
            b.node_features, b.edge_index, b.edge_weight, b.batch, b.labels, b.ptr), 0.0, False)
    # (oracle state was updated by its own training forward, same as the model's)
    torch.testing.assert_close(le.cpu(), lo_e, **TOL)


def test_fused_matches_layered_and_is_deterministic():
    import connectome_gnn_amd as C
    b = C.collate_graphs(C.generate_dataset(24, 84, 8, seed=9)).to(DEV)
    outs = {}
    for impl in ("fused", "layered"):
        torch.manual_seed(3)
        m = C.GCNConnectome(5, 64, dropout=0.0, impl=impl).to(DEV).train()
        lg = m(b)
        torch.nn.functional.cross_entropy(lg, b.labels).backward()
        outs[impl] = (lg.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()})
        if impl == "fused":
            m.zero_grad()
            lg2 = m(b)
            torch.nn.functional.cross_entropy(lg2, b.labels).backward()
            assert torch.equal(lg2, lg)                      # no atomics: bit-identical reruns
            for k, p in m.named_parameters():
                assert torch.equal(p.grad, outs[impl][1][k]), k
    torch.testing.assert_close(outs["fused"][0], outs["layered"][0], **TOL)
    for k, g in outs["layered"][1].items():
        torch.testing.assert_close(outs["fused"][1][k], g, rtol=1e-4, atol=2e-6 + 1e-5 * float(g.abs().max()))


def test_fused_dropout_contract():
    """Dropout (p=0.3) in the fused path: keep rate, 1/(1-p) scaling (mean preserved), masks
    regenerate per call, and backward uses the SAME mask as forward (finite-difference check
    through a frozen mask is impossible, so check d/dbeta of a linear probe instead)."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd import fused
    b = C.collate_graphs(C.generate_dataset(64, 84, 8, seed=4)).to(DEV)
    torch.manual_seed(0)
    m = C.GCNConnectome(5, 64, 2, 3, dropout=0.3, impl="fused").to(DEV).train()
    e1, e2 = m.encode(b), m.encode(b)
    assert torch.isfinite(e1).all() and not torch.equal(e1, e2)
    m0 = C.GCNConnectome(5, 64, 2, 3, dropout=0.0, impl="fused").to(DEV).train()
    m0.load_state_dict(m.state_dict())
    # E[dropout(x)] = x: pooled means over many nodes agree within sampling noise only for the
    # LAST layer's dropout; earlier masks change the activations themselves, so compare loosely.
    ref = m0.encode(b)
    acc = torch.zeros_like(ref)
    for _ in range(20):
        acc += m.encode(b).detach()
    rel = (acc / 20 - ref).norm() / ref.norm()
    assert rel < 0.25, float(rel)
    # mask bytes: keep rate ~ 0.7
    out = fused.encode(m, b, b.structure())
    ctx = out.grad_fn.c if hasattr(out.grad_fn, "c") else None
    if ctx is not None:
        for mk in ctx.masks:
            bits = torch.stack([(mk >> i) & 1 for i in range(4)]).float().mean()
            assert abs(float(bits) - 0.7) < 0.01, float(bits)
    out.sum().backward()
    for p in m.parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all()


def test_fused_headline_shape_properties():
    """Full BASELINE size (4096 x 360-ROI, hidden 64): finite, deterministic, and permuting
    the graphs of the batch permutes the embeddings (block-diagonal independence) while BN
    statistics -- sums over all nodes -- do not move beyond fp32 rounding."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd.resident import assemble_batch
    from connectome_gnn_amd.synthetic import generate_packed
    ds = generate_packed(512, 360, 14, seed=1).to(DEV)
    ids = torch.arange(512).repeat(8)                      # 4096 graphs resident (8 x 512 distinct)
    perm = torch.randperm(4096, generator=torch.Generator().manual_seed(0))
    torch.manual_seed(1)
    m = C.GCNConnectome(5, 64, dropout=0.0).to(DEV).train()
    b1 = assemble_batch(ds, ids)
    e1 = m.encode(b1)
    rm1 = m.batch_norms[2].running_mean.clone()
    assert m.impl_used == "fused" and torch.isfinite(e1).all()
    torch.manual_seed(1)
    m2 = C.GCNConnectome(5, 64, dropout=0.0).to(DEV).train()
    e2 = m2.encode(assemble_batch(ds, ids[perm]))
    torch.testing.assert_close(e2, e1[perm.to(DEV)], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(m2.batch_norms[2].running_mean, rm1, rtol=1e-4, atol=1e-6)
    e1.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


def test_edge_cases_empty_graphs_and_fallbacks():
    """Zero-node / zero-edge graphs inside a batch, a graph larger than the LDS tile (the wide encoder
    over the CSR gather aggregate), and hidden 32 (op-by-op path) all agree with the oracle."""
    import connectome_gnn_amd as C
    g_ok = C.generate_connectome(30, 4, seed=1)
    empty = C.ConnectomeGraph(torch.zeros(0, 5), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0),
                              torch.tensor(1))
    lonely = C.ConnectomeGraph(torch.randn(3, 5), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0),
                               torch.tensor(0))
    big = C.generate_connectome(400, 6, seed=2)
    for graphs, hidden, want_impl in (([g_ok, empty, lonely, g_ok], 64, "fused"), ([g_ok, big], 64, "fused"),
                                      ([g_ok, big], 32, "layered")):
        b = C.collate_graphs(graphs)
        torch.manual_seed(2)
        m = C.GCNConnectome(5, hidden, dropout=0.0)
        st = O.require_grad({k: v.clone() for k, v in m.state_dict().items()})
        ob = O.OBatch(b.node_features, b.edge_index, b.edge_weight, b.batch, b.labels, b.ptr)
        lo = O.gcn_forward(st, ob, 0.0, True)
        lo.sum().backward()
        m = m.to(DEV).train()
        lg = m(b.to(DEV))
        assert m.impl_used == want_impl
        assert want_impl == "layered" or m._fused_kind == ("wide" if any(g is big for g in graphs) else "tile")
        lg.sum().backward()
        torch.testing.assert_close(lg.cpu(), lo, **TOL)
        for k, p in m.named_parameters():
            w = st[k].grad
            torch.testing.assert_close(p.grad.cpu(), w, rtol=1e-4, atol=2e-6 + 1e-5 * float(w.abs().max()),
                                       msg=lambda s: f"{k}: {s}")
    with pytest.raises(RuntimeError, match="not applicable"):
        C.GCNConnectome(5, 32, impl="fused").to(DEV)(C.collate_graphs([g_ok]).to(DEV))


def test_sage_edge_cases_empty_graphs_and_fallbacks():
    """GraphSAGE: zero-node / zero-edge graphs inside a batch on the one-node encoder, a graph
    larger than the LDS tile (same encoder over the CSR gather aggregate) and hidden 32 on the
    op-by-op path -- all against the oracle."""
    import connectome_gnn_amd as C
    g_ok = C.generate_connectome(30, 4, seed=1)
    empty = C.ConnectomeGraph(torch.zeros(0, 5), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0),
                              torch.tensor(1))
    lonely = C.ConnectomeGraph(torch.randn(3, 5), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0),
                               torch.tensor(0))
    big = C.generate_connectome(400, 6, seed=2)
    for graphs, hidden, want_impl in (([g_ok, empty, lonely, g_ok], 64, "fused"),
                                      ([g_ok, big], 64, "fused"), ([g_ok, lonely], 32, "layered")):
        b = C.collate_graphs(graphs)
        torch.manual_seed(2)
        m = C.GraphSAGEConnectome(5, hidden, dropout=0.0)
        st = O.require_grad({k: v.clone() for k, v in m.state_dict().items()})
        ob = O.OBatch(b.node_features, b.edge_index, b.edge_weight, b.batch, b.labels, b.ptr)
        lo = O.sage_forward(st, ob, 0.0, True)
        lo.sum().backward()
        m = m.to(DEV).train()
        lg = m(b.to(DEV))
        assert m.impl_used == want_impl
        lg.sum().backward()
        torch.testing.assert_close(lg.cpu(), lo, **TOL)
        for k, p in m.named_parameters():
            w = st[k].grad
            torch.testing.assert_close(p.grad.cpu(), w, rtol=1e-4, atol=2e-6 + 1e-5 * float(w.abs().max()),
                                       msg=lambda s_: f"{k}: {s_}")
    with pytest.raises(RuntimeError, match="not applicable"):
        C.GraphSAGEConnectome(5, 32, impl="fused").to(DEV)(C.collate_graphs([g_ok]).to(DEV))


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_graphed_step_matches_eager_and_redraws_dropout(kind):
    """HIP-graph replay of the whole step == eager steps (dropout 0), and with dropout > 0 every
    replay draws a fresh mask (the by-value seed is frozen in the graph; the device key is not).
    Both encoders (fused GCN, one-node GraphSAGE), the head kernel and the loss are inside the graph."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd.graphed import GraphedTrainStep
    b = C.collate_graphs(C.generate_dataset(32, 84, 8, seed=6)).to(DEV)
    b.structure()
    cls = C.GCNConnectome if kind == "gcn" else C.GraphSAGEConnectome

    def run(graph: bool, steps=4):
        torch.manual_seed(11)
        m = cls(5, 64, dropout=0.0).to(DEV).train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-2, capturable=True)
        m.prepare_batch(b, reuse=True)      # (what the captured step does: both runs on the same node order)

        def eager():
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(m(b), b.labels)
            loss.backward(); opt.step()
            return float(loss)

        if graph:
            # one eager warm-up step (it also creates the optimizer state OUTSIDE the graph,
            # as torch requires), then replays
            st = GraphedTrainStep(m, opt, b, warmup=1)
            return [float(st()) for _ in range(steps)], m
        eager()
        return [eager() for _ in range(steps)], m

    le, me = run(False)
    lg, mg = run(True)
    np.testing.assert_allclose(lg, le, rtol=1e-5, atol=1e-6)
    for (k, p), (_, q) in zip(me.named_parameters(), mg.named_parameters()):
        if not (k.startswith("convs.") and k.endswith(".bias")):     # zero-true-gradient bias: noise
            torch.testing.assert_close(p, q, rtol=1e-4, atol=1e-5, msg=lambda s: f"{k}: {s}")
    # dropout: replays must differ from each other
    torch.manual_seed(1)
    m = cls(5, 64, dropout=0.5).to(DEV).train()
    opt = torch.optim.SGD(m.parameters(), lr=0.0)               # frozen weights: only masks change
    st = GraphedTrainStep(m, opt, b, warmup=1)
    vals = {round(float(st()), 7) for _ in range(5)}
    assert len(vals) >= 4, vals


def test_graphed_fp16_storage_step_redraws_dropout():
    """GCNConnectome(storage='fp16') under HIP-graph replay: the keep masks of every layer (read
    from the graph pool's mask buffers through record_dropout) and the loss differ between
    replays -- the by-value seeds are frozen in the graph, the device key words are refreshed by
    the captured cgnn_rng_advance."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd.graphed import GraphedTrainStep
    b = C.collate_graphs(C.generate_dataset(4, 200, 20, seed=3)).to(DEV)
    b.structure()
    torch.manual_seed(1)
    m = C.GCNConnectome(5, 64, dropout=0.5, storage="fp16").to(DEV).train()
    m.record_dropout = True
    opt = torch.optim.SGD(m.parameters(), lr=0.0)               # frozen weights: only masks change
    st = GraphedTrainStep(m, opt, b, warmup=1)
    assert m.impl_used == "fused" and m._fused_kind == "half"
    seen, losses = [], set()
    for _ in range(4):
        losses.add(round(float(st()), 7))
        seen.append([t.clone() for t in m.last_dropout["layers"]])
    assert len(losses) >= 3, losses
    for li in range(3):
        for a in range(4):
            for c in range(a + 1, 4):
                assert not torch.equal(seen[a][li], seen[c][li]), f"layer {li}: replays {a},{c} share a mask"


def test_sage_one_node_encoder_matches_layered_and_is_deterministic():
    """GraphSAGE: the one-node encoder (sage_path.py) against the op-by-op layered path on the same
    weights (dropout 0), and its dropout contract: same torch seed -> identical step, masks used
    consistently forward/backward (finite grads, BatchNorm statistics updated once)."""
    import connectome_gnn_amd as C
    b = C.collate_graphs(C.generate_dataset(6, 84, 8, seed=5) + C.generate_dataset(3, 200, 10, seed=6)).to(DEV)
    outs = {}
    for impl in ("fused", "layered"):
        torch.manual_seed(11)
        m = C.GraphSAGEConnectome(5, 128, dropout=0.0, impl=impl).to(DEV).train()
        lg = m(b)
        torch.nn.functional.cross_entropy(lg, b.labels).backward()
        assert m.impl_used == impl
        outs[impl] = (lg.detach(), {k: p.grad.clone() for k, p in m.named_parameters()},
                      {k: v.clone() for k, v in m.state_dict().items() if "running" in k})
    torch.testing.assert_close(outs["fused"][0], outs["layered"][0], **TOL)
    for k, g in outs["layered"][1].items():
        torch.testing.assert_close(outs["fused"][1][k], g, rtol=1e-4, atol=1e-5 * float(g.abs().max()) + 1e-7,
                                   msg=lambda s_: f"{k}: {s_}")
    for k, v in outs["layered"][2].items():
        torch.testing.assert_close(outs["fused"][2][k], v, **TOL)
    runs = []
    for _ in range(2):
        torch.manual_seed(3)
        m = C.GraphSAGEConnectome(5, 64, dropout=0.4, impl="fused").to(DEV).train()
        lg = m(b)
        torch.nn.functional.cross_entropy(lg, b.labels).backward()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters())
        assert int(m.batch_norms[0].num_batches_tracked) == 1
        runs.append((lg.detach(), [p.grad.clone() for p in m.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, c) for a, c in zip(runs[0][1], runs[1][1]))
    m.eval()
    with torch.no_grad():
        e = m.encode(b)
    assert m.impl_used == "fused" and e.shape == (9, 64) and torch.isfinite(e).all()


def test_gcn_wide_encoder_matches_layered():
    """GCN hidden 128: the one-node wide encoder (gcn_wide_path.py) against the op-by-op path on the
    same weights (dropout 0); hidden 64 with 20 input features (> the per-tile kernels' 16) takes
    the wide encoder too."""
    import connectome_gnn_amd as C
    b = C.collate_graphs(C.generate_dataset(6, 84, 8, seed=5) + C.generate_dataset(3, 200, 10, seed=6)).to(DEV)
    outs = {}
    for impl in ("fused", "layered"):
        torch.manual_seed(11)
        m = C.GCNConnectome(5, 128, dropout=0.0, impl=impl).to(DEV).train()
        lg = m(b)
        torch.nn.functional.cross_entropy(lg, b.labels).backward()
        assert m.impl_used == impl and (impl == "layered" or m._fused_kind == "wide")
        outs[impl] = (lg.detach(), {k: p.grad.clone() for k, p in m.named_parameters()},
                      {k: v.clone() for k, v in m.state_dict().items() if "running" in k})
    torch.testing.assert_close(outs["fused"][0], outs["layered"][0], **TOL)
    for k, g in outs["layered"][1].items():
        torch.testing.assert_close(outs["fused"][1][k], g, rtol=1e-4, atol=1e-5 * float(g.abs().max()) + 1e-7,
                                   msg=lambda s_: f"{k}: {s_}")
    for k, v in outs["layered"][2].items():
        torch.testing.assert_close(outs["fused"][2][k], v, **TOL)
    wide_in = C.ConnectomeBatch(torch.randn(b.num_nodes, 20, device=DEV), b.edge_index, b.edge_weight,
                                b.batch, b.labels, b.ptr)
    m = C.GCNConnectome(20, 64, dropout=0.2).to(DEV).train()
    m(wide_in).sum().backward()
    assert m.impl_used == "fused" and m._fused_kind == "wide"
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())


def test_sage_config3_full_size_properties():
    """BASELINE config 3 at full size (512 x 360-ROI GraphSAGE, hidden 128) on the one-node
    encoder: finite, and permuting the graphs of the batch permutes the embeddings (block-diagonal
    independence) while the batch-wide BatchNorm statistics stay put; backward is finite and
    deterministic run to run."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd.resident import assemble_batch
    from connectome_gnn_amd.synthetic import generate_packed
    ds = generate_packed(512, 360, 14, seed=2).to(DEV)
    ids = torch.arange(512)
    perm = torch.randperm(512, generator=torch.Generator().manual_seed(0))
    outs = []
    for order in (ids, ids[perm], ids):
        torch.manual_seed(1)
        m = C.GraphSAGEConnectome(5, 128, dropout=0.0).to(DEV).train()
        e = m.encode(assemble_batch(ds, order))
        assert m.impl_used == "fused" and torch.isfinite(e).all()
        e.square().sum().backward()
        outs.append((e.detach(), m.batch_norms[2].running_mean.clone(),
                     [p.grad.clone() for p in m.parameters() if p.grad is not None]))
    torch.testing.assert_close(outs[1][0], outs[0][0][perm.to(DEV)], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(outs[1][1], outs[0][1], rtol=1e-4, atol=1e-6)
    assert torch.equal(outs[2][0], outs[0][0])
    assert all(torch.equal(a, c) for a, c in zip(outs[2][2], outs[0][2]))
    assert all(torch.isfinite(g).all() for g in outs[0][2])


def test_resident_loader_prefetch_is_equivalent():
    """ResidentDataLoader(prefetch=True) builds the next batch (and its structure) on a side stream:
    same batches in the same order, and the same training trajectory, as without prefetch."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd.resident import ResidentDataLoader
    from connectome_gnn_amd.synthetic import generate_packed
    ds = generate_packed(96, 84, 8, seed=9).to(DEV)
    runs = []
    for pf in (False, True):
        torch.manual_seed(4)
        m = C.GCNConnectome(5, 64, dropout=0.0)
        tr = C.Trainer(m, torch.optim.Adam(m.parameters(), lr=1e-2), device=DEV)
        ld = ResidentDataLoader(ds, batch_size=20, shuffle=True, prefetch=pf, prepare=tr.model.prepare_batch)
        torch.manual_seed(5)
        first = [(b.labels.clone(), b.edge_index[:, :7].clone(), b.num_graphs) for b in ld]
        torch.manual_seed(5)
        losses = [tr.train_epoch(ld) for _ in range(3)]
        runs.append((first, losses, [p.detach().clone() for p in m.parameters()]))
    assert len(runs[0][0]) == len(runs[1][0]) == 5
    for (la, ea, na), (lb, eb, nb) in zip(runs[0][0], runs[1][0]):
        assert na == nb and torch.equal(la, lb) and torch.equal(ea, eb)
    assert runs[0][1] == runs[1][1]
    assert all(torch.equal(a, c) for a, c in zip(runs[0][2], runs[1][2]))


@pytest.mark.parametrize("trial", range(10))
def test_models_random_batches_vs_oracle(trial):
    """Random ragged batches (graphs of 1..384 nodes, mixed degrees, both models, hidden 64/128)
    against the oracle: logits within 1e-5 of the scale; every gradient within 1e-5 of its
    tensor's scale of the fp32 oracle, or at least as close to the oracle evaluated in fp64 as the
    fp32 oracle itself (degenerate graphs make BatchNorm ill-conditioned in any fp32 arithmetic)."""
    import random
    import connectome_gnn_amd as C
    rnd = random.Random(1000 + trial)
    kind = rnd.choice(["gcn", "sage"])
    hidden = rnd.choice([64, 128])
    graphs = []
    for g in range(rnd.randint(2, 10)):
        n = rnd.choice([1, 2, 3, 17, 40, 84, 100, 200, 360, 384])
        if n <= 3:
            ei = torch.tensor([[0], [n - 1]], dtype=torch.long) if n > 1 else torch.zeros(2, 0, dtype=torch.long)
            gen = torch.Generator().manual_seed(trial * 100 + g)
            graphs.append(C.ConnectomeGraph(torch.randn(n, 5, generator=gen), ei,
                                            torch.rand(ei.shape[1], generator=gen) + 0.1, torch.tensor(g % 2)))
        else:
            k = min(rnd.choice([2, 4, 6, 8, 14]), max(2, (n - 1) // 2 * 2))
            graphs.append(C.generate_connectome(n, k, seed=trial * 100 + g))
    b = C.collate_graphs(graphs)
    torch.manual_seed(trial)
    m = _model(kind, 5, hidden, dropout=0.0)

    lo, _, g32, _ = P.oracle_run(kind, m.state_dict(), b)
    lo64, _, g64, _ = P.oracle_run(kind, m.state_dict(), b, dtype=torch.float64)
    floor = P.NoiseFloor(kind, m.state_dict(), b)
    m = m.to(DEV).train()
    bd = b.to(DEV)
    lg = m(bd)
    torch.nn.functional.cross_entropy(lg, bd.labels).backward()
    assert m.impl_used == "fused"
    scale = float(lo.abs().max()) + 1e-6
    err_l = float((lg.detach().cpu() - lo).abs().max())
    assert err_l <= 1e-5 * scale + 1e-6 or \
        float((lg.detach().cpu().double() - lo64).abs().max()) <= float((lo.double() - lo64).abs().max()) + 1e-9
    for k_, p in m.named_parameters():
        P.assert_grad(k_, p.grad, g32[k_], g64[k_], f"random-{trial}-{kind}-h{hidden}", floor)


# ------------------------------------------------------ the benchmarked mode: dropout ON, pinned
@pytest.mark.parametrize("kind,n,k,hidden,nb,impl,want", [
    ("gcn", 84, 8, 64, 24, "auto", "fused"),         # cfg1/2 shape: per-tile fused kernels
    ("gcn", 360, 14, 64, 6, "auto", "fused"),        # cfg4 (headline) shape
    ("sage", 84, 8, 64, 16, "auto", "fused"),        # one-node GraphSAGE encoder
    ("sage", 360, 14, 128, 4, "auto", "fused"),      # cfg3 shape
    ("gcn", 100, 10, 128, 12, "auto", "fused"),      # wide one-node GCN encoder
    ("gcn", 84, 8, 64, 8, "layered", "layered"),     # op-by-op path
    ("sage", 84, 8, 64, 8, "layered", "layered"),
    ("gcn", 84, 8, 64, 24, "twin", "fused"),         # per-tile kernels on the degree-ordered twin
    ("gcn", 360, 14, 64, 6, "twin", "fused"),        # (what bench.py's resident batches run: prepare_batch(reuse=True))
    ("sage", 360, 14, 128, 4, "twin", "fused"),      # GraphSAGE and the wide GCN encoder on the twin
    ("gcn", 100, 10, 128, 12, "twin", "fused"),
])
def test_dropout_on_matches_oracle_with_replayed_masks(kind, n, k, hidden, nb, impl, want):
    """train() with dropout 0.3 -- the mode bench.py times.  The HIP path's own keep decisions
    (layer keep bits + head factor, ``model.record_dropout``) are replayed through the oracle
    (reference models.py:199,210,261 with the Bernoulli draw replaced), so logits, loss, every
    gradient and the BatchNorm running statistics are compared at the dropout-off tolerances:
    this covers the mask-scaled ReLU'/dropout' backward and the readout rebuild."""
    import connectome_gnn_amd as C
    b = C.collate_graphs(C.generate_dataset(nb, n, k, seed=321))
    torch.manual_seed(11)
    twin = impl == "twin"
    m = _model(kind, 5, hidden, dropout=0.3, impl="auto" if twin else impl)
    sd0 = {k_: v.clone() for k_, v in m.state_dict().items()}
    m = m.to(DEV).train()
    m.record_dropout = True
    bd = b.to(DEV)
    if twin:
        m.prepare_batch(bd, reuse=True)
        tw = bd.structure().__dict__.get("_degree_twin")
        assert tw is not None and not torch.equal(tw.perm, torch.arange(b.num_nodes, device=DEV))
        assert torch.equal(torch.sort(tw.perm).values, torch.arange(b.num_nodes, device=DEV))
    lg = m(bd)
    loss_g = torch.nn.functional.cross_entropy(lg, bd.labels)
    loss_g.backward()
    assert m.impl_used == want
    masks = P.recorded_masks(m, b.num_nodes, b.num_graphs)
    assert len(masks["layers"]) == 3
    for keep in masks["layers"]:
        assert 0.65 < float(keep.mean()) < 0.75          # p = 0.3 was really applied
    assert 0.15 < float(masks["head"].mean()) < 0.6      # relu'(z) & keep: ~0.7 of the live units
    lo, loss_o, g32, st32 = P.oracle_run(kind, sd0, b, 0.3, True, masks)
    _, _, g64, _ = P.oracle_run(kind, sd0, b, 0.3, True, masks, dtype=torch.float64)
    torch.testing.assert_close(lg.detach().cpu(), lo, **TOL)
    torch.testing.assert_close(loss_g.detach().cpu(), loss_o, **TOL)
    floor = P.NoiseFloor(kind, sd0, b, 0.3, masks)
    for k_, p in m.named_parameters():
        P.assert_grad(k_, p.grad, g32[k_], g64[k_], f"dropout-{kind}-{n}-h{hidden}-{impl}", floor)
    sd = m.state_dict()
    for k_ in sd:
        if "running" in k_ or "num_batches" in k_:
            torch.testing.assert_close(sd[k_].cpu(), st32[k_], **TOL, msg=lambda s: f"{k_}: {s}")


def test_dropout_masks_are_reproducible_under_manual_seed():
    """torch.manual_seed makes the dropout draw reproducible (seeds come from a dedicated generator
    keyed by torch.initial_seed(), _lib.next_seed), and the global CPU RNG that the loaders'
    shuffles use is NOT consumed by a forward pass."""
    import connectome_gnn_amd as C
    b = C.collate_graphs(C.generate_dataset(6, 84, 8, seed=3)).to(DEV)
    outs = []
    for _ in range(2):
        torch.manual_seed(5)
        m = C.GCNConnectome(5, 64).to(DEV).train()
        before = torch.get_rng_state()
        outs.append(m(b).detach().clone())
        assert torch.equal(torch.get_rng_state(), before)
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------- config 5's model shape against the oracle
@pytest.mark.parametrize("dropout,ngraphs", [(0.0, 3), (0.3, 3), (0.3, 5)])
def test_cfg5_shape_gcn_1000roi_h256_vs_oracle(dropout, ngraphs):
    """BASELINE config 5's model: 1000-ROI graphs at 10 % density (k = 100), hidden 256, 3 layers;
    graphs > 384 nodes take the large-graph path.  fp32 against the fp32 oracle (the fp16-storage
    path is validated against this same oracle at fp16 resolution in test_gpu_kernels).  Five graphs =
    5000 rows: layer 0 then runs through the packed 32-wide panel of the weight-stationary GEMMs."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd.resident import assemble_batch
    from connectome_gnn_amd.synthetic import generate_packed
    ds = generate_packed(ngraphs, 1000, 100, seed=9)
    b = assemble_batch(ds, torch.arange(ngraphs))
    assert b.num_nodes == 1000 * ngraphs and b.edge_index.shape[1] == 100_000 * ngraphs
    torch.manual_seed(3)
    m = _model("gcn", 5, 256, dropout=dropout)
    sd0 = {k_: v.clone() for k_, v in m.state_dict().items()}
    m = m.to(DEV).train()
    m.record_dropout = True
    bd = b.to(DEV)
    lg = m(bd)
    loss_g = torch.nn.functional.cross_entropy(lg, bd.labels)
    loss_g.backward()
    masks = P.recorded_masks(m, b.num_nodes, b.num_graphs) if dropout > 0 else None
    lo, loss_o, g32, st32 = P.oracle_run("gcn", sd0, b, dropout, True, masks)
    _, _, g64, _ = P.oracle_run("gcn", sd0, b, dropout, True, masks, dtype=torch.float64)
    torch.testing.assert_close(lg.detach().cpu(), lo, **TOL)
    torch.testing.assert_close(loss_g.detach().cpu(), loss_o, **TOL)
    floor = P.NoiseFloor("gcn", sd0, b, dropout, masks)
    for k_, p in m.named_parameters():
        P.assert_grad(k_, p.grad, g32[k_], g64[k_], f"cfg5-p{dropout}", floor)
    sd = m.state_dict()
    for k_ in sd:
        if "running" in k_:
            torch.testing.assert_close(sd[k_].cpu(), st32[k_], **TOL)


@pytest.mark.parametrize("kind", ["gcn", "sage"])
@pytest.mark.parametrize("in_ch,hidden,n,nb", [(1, 64, 84, 8), (8, 64, 84, 60), (9, 64, 84, 60), (16, 64, 360, 12),
                                               (17, 64, 360, 12), (32, 128, 100, 48), (40, 64, 100, 48),
                                               (64, 128, 100, 48), (3, 256, 360, 16), (20, 256, 100, 48),
                                               (128, 128, 50, 10), (7, 192, 100, 48), (12, 32, 84, 60)])
def test_shape_sweep_vs_oracle(kind, in_ch, hidden, n, nb):
    """Input widths 1 .. 128 x hidden 32 .. 256 x row counts below and above the 4096 from which the
    weight-stationary GEMMs and the packed layer-0 panels apply: whatever path the dispatcher picks
    (per-tile, wide, GraphSAGE encoder, op by op), logits and every gradient against the oracle."""
    import connectome_gnn_amd as C
    gs = C.generate_dataset(nb, n, k=8, seed=31 + in_ch)
    g = torch.Generator().manual_seed(in_ch * 1000 + hidden)
    gs = [C.ConnectomeGraph(torch.randn(x.num_nodes, in_ch, generator=g), x.edge_index, x.edge_weight, x.label) for x in gs]
    b = C.collate_graphs(gs)
    torch.manual_seed(11)
    m = _model(kind, in_ch, hidden, dropout=0.0)
    sd0 = {k_: v.clone() for k_, v in m.state_dict().items()}
    lo, loss_o, g32, _ = P.oracle_run(kind, sd0, b)
    _, _, g64, _ = P.oracle_run(kind, sd0, b, dtype=torch.float64)
    m = m.to(DEV).train()
    bd = b.to(DEV)
    lg = m(bd)
    loss_g = torch.nn.functional.cross_entropy(lg, bd.labels)
    loss_g.backward()
    torch.testing.assert_close(lg.cpu(), lo, **TOL)
    P.assert_grads({k_: p.grad for k_, p in m.named_parameters()}, kind, sd0, b,
                   f"sweep-{kind}-f{in_ch}-h{hidden}-{n}x{nb}", g32=g32, g64=g64)
    # ... and the eval-mode forward on the running statistics that step left behind (each side its own)
    _, _, _, st32 = P.oracle_run(kind, sd0, b)
    sd = m.state_dict()
    for k_ in sd:
        if "running" in k_:
            torch.testing.assert_close(sd[k_].cpu(), st32[k_], **TOL)
    le_o, _, _, _ = P.oracle_run(kind, st32, b, 0.0, training=False)
    m.eval()
    with torch.no_grad():
        le = m(bd)
    torch.testing.assert_close(le.cpu(), le_o, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("kind,hidden,n,k,nb", [("gcn", 64, 360, 14, 6), ("sage", 128, 84, 8, 20), ("gcn", 256, 1000, 100, 3),
                                                ("gcn", 32, 84, 8, 9)])
def test_training_step_loss_through_the_one_launch_classifier_vs_oracle(kind, hidden, n, k, nb):
    """The Trainer's way of taking a step -- ops.model_loss (model.forward_loss: classifier + cross-entropy +
    their backward in one launch, cgnn_head_loss_f32) and the unit upstream gradient -- with dropout 0.3 on every
    path it meets (per-tile GCN, GraphSAGE encoder, large graphs, hidden 32 = the three-launch form): loss and
    every gradient against the oracle with the kernels' own keep decisions replayed."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd import ops
    from connectome_gnn_amd.resident import assemble_batch
    from connectome_gnn_amd.synthetic import generate_packed
    b = assemble_batch(generate_packed(nb, n, k, seed=21), torch.arange(nb))
    torch.manual_seed(8)
    m = _model(kind, 5, hidden, dropout=0.3)
    sd0 = {k_: v.clone() for k_, v in m.state_dict().items()}
    m = m.to(DEV).train()
    m.record_dropout = True
    bd = b.to(DEV)
    loss = ops.model_loss(m, ops.CrossEntropyLoss(), bd)
    ops.backward_unit(loss)
    masks = P.recorded_masks(m, b.num_nodes, b.num_graphs)
    _, loss_o, g32, _ = P.oracle_run(kind, sd0, b, 0.3, True, masks)
    _, _, g64, _ = P.oracle_run(kind, sd0, b, 0.3, True, masks, dtype=torch.float64)
    torch.testing.assert_close(loss.detach().cpu(), loss_o, **TOL)
    P.assert_grads({k_: p.grad for k_, p in m.named_parameters()}, kind, sd0, b, f"step-{kind}-h{hidden}-{n}",
                   dropout=0.3, masks=masks, g32=g32, g64=g64)


def test_a_relu_tie_is_found_and_resolved():
    """GraphSAGE hidden 256 on 12 x 360-ROI graphs: ONE of 1.1 M last-layer pre-activations is +5.4e-8 in
    float64 (channel median 0.5) and the split-bf16 GEMM rounds it to 0 -- 2 % of that channel's bias
    gradient.  Rules (1)-(3) fail; rule (4) lists the tie and passes with it -- and only
    it -- decided the other way."""
    import connectome_gnn_amd as C
    b = C.collate_graphs(C.generate_dataset(12, 360, 14, seed=123))
    torch.manual_seed(7)
    m = _model("sage", 5, 256, dropout=0.0)
    sd0 = {k_: v.clone() for k_, v in m.state_dict().items()}
    ties = P.relu_ties("sage", sd0, b)
    assert ("layer2", 931, 133) in ties and len(ties) <= P.RELU_TIE_LIST
    _, _, g32, _ = P.oracle_run("sage", sd0, b)
    _, _, g64, _ = P.oracle_run("sage", sd0, b, dtype=torch.float64)
    m = m.to(DEV).train()
    lg = m(b.to(DEV))
    torch.nn.functional.cross_entropy(lg, b.labels.to(DEV)).backward()
    grads = {k_: p.grad for k_, p in m.named_parameters()}
    before = len(P.ARBITER["relu_ties"])
    P.assert_grads(grads, "sage", sd0, b, "tie-demo", g32=g32, g64=g64)
    # on the boxes this was written on rules (1)-(3) fail and exactly this tie resolves it; a host whose fp32
    # matmul happens to round the tie the way the GPU does (rule (3) includes the single-threaded evaluation)
    # would pass without rule (4): both are fine
    used = P.ARBITER["relu_ties"][before:]
    assert len(used) <= 1 and all("[('layer2', 931, 133)] decided" in u for u in used)


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_ragged_large_graphs_on_the_band_aggregate_vs_oracle(kind):
    """Graphs of 1000, 333 and 610 nodes at band-like density plus an edgeless and an empty one in one
    batch (pitch 1024, ragged row blocks, a graph that would fit an LDS tile riding along): the one-node
    encoders over dense fragments + gather remainder against the oracle, dropout masks replayed."""
    import connectome_gnn_amd as C
    graphs = [C.generate_connectome(1000, 80, seed=5), C.generate_connectome(333, 60, seed=6),
              C.ConnectomeGraph(torch.randn(7, 5), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0), torch.tensor(0)),
              C.generate_connectome(610, 90, seed=7),
              C.ConnectomeGraph(torch.zeros(0, 5), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0), torch.tensor(1))]
    b = C.collate_graphs(graphs)
    torch.manual_seed(6)
    m = _model(kind, 5, 128, dropout=0.3)
    sd0 = {k_: v.clone() for k_, v in m.state_dict().items()}
    m = m.to(DEV).train()
    m.record_dropout = True
    bd = b.to(DEV)
    lg = m(bd)
    assert m.impl_used == "fused"
    s = bd.structure()
    bf, bb = s.band_ops(kind, s.gcn_norm() if kind == "gcn" else s.sage_norm())
    assert bf is not None and bb is not None and 0.5 < bf[1].covered < 1.0
    loss_g = torch.nn.functional.cross_entropy(lg, bd.labels)
    loss_g.backward()
    masks = P.recorded_masks(m, b.num_nodes, b.num_graphs)
    lo, loss_o, g32, st32 = P.oracle_run(kind, sd0, b, 0.3, True, masks)
    _, _, g64, _ = P.oracle_run(kind, sd0, b, 0.3, True, masks, dtype=torch.float64)
    torch.testing.assert_close(lg.detach().cpu(), lo, **TOL)
    floor = P.NoiseFloor(kind, sd0, b, 0.3, masks)
    for k_, p in m.named_parameters():
        P.assert_grad(k_, p.grad, g32[k_], g64[k_], f"ragged-band-{kind}", floor)


def test_structures_are_released_by_reference_count():
    """A batch's structure -- CSR, blocked-ELL, the dense fragments of large graphs, the degree-ordered twin --
    holds hundreds of MB at the benchmark sizes: it must die with the batch, not wait for the cycle collector
    (a cycle through such a cache once cost ~100 ms collector stalls per epoch)."""
    import gc
    import weakref
    import connectome_gnn_amd as C
    gc.collect()
    gc.disable()
    try:
        for graphs, hidden in (([C.generate_connectome(600, 80, seed=1), C.generate_connectome(450, 70, seed=2)], 128),
                               (C.generate_dataset(6, 100, 8, seed=3), 64)):
            b = C.collate_graphs(graphs).to(DEV)
            m = C.GCNConnectome(5, hidden, dropout=0.0).to(DEV).train()
            m.prepare_batch(b, reuse=True)
            m(b).sum().backward()
            s = b.structure()
            refs = [weakref.ref(s)]
            twin = s.__dict__.get("_degree_twin")
            if twin is not None:
                refs.append(weakref.ref(twin))
            del s, twin, b, m
            assert all(r() is None for r in refs), "a structure survived its batch without the cycle collector"
    finally:
        gc.enable()


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_graphs_beyond_the_band_builder_take_the_gather_aggregate(kind):
    """A 1100-node graph (more than the 1024 the dense-fragment builder takes) next to a small one and an
    empty one: the one-node encoders run over the plain CSR gather aggregate, against the oracle."""
    import connectome_gnn_amd as C
    graphs = [C.generate_connectome(1100, 40, seed=3), C.generate_connectome(50, 6, seed=4),
              C.ConnectomeGraph(torch.zeros(0, 5), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0), torch.tensor(1))]
    b = C.collate_graphs(graphs)
    torch.manual_seed(5)
    m = _model(kind, 5, 64, dropout=0.0)
    sd0 = {k_: v.clone() for k_, v in m.state_dict().items()}
    m = m.to(DEV).train()
    bd = b.to(DEV)
    lg = m(bd)
    assert m.impl_used == "fused"
    s = bd.structure()
    assert s.band_ops(kind, s.gcn_norm() if kind == "gcn" else s.sage_norm()) == (None, None)
    loss_g = torch.nn.functional.cross_entropy(lg, bd.labels)
    loss_g.backward()
    lo, loss_o, g32, st32 = P.oracle_run(kind, sd0, b, 0.0, True, None)
    _, _, g64, _ = P.oracle_run(kind, sd0, b, 0.0, True, None, dtype=torch.float64)
    torch.testing.assert_close(lg.detach().cpu(), lo, **TOL)
    floor = P.NoiseFloor(kind, sd0, b, 0.0, None)
    for k_, p in m.named_parameters():
        P.assert_grad(k_, p.grad, g32[k_], g64[k_], f"big1100-{kind}", floor)


@pytest.mark.parametrize("dropout,hidden,ngraphs", [(0.0, 128, 3), (0.3, 128, 3), (0.3, 256, 5)])
def test_sage_1000roi_h128_band_aggregate_vs_oracle(dropout, hidden, ngraphs):
    """GraphSAGE on 1000-ROI graphs at 10 % density (BASELINE config 5's graphs), hidden 128: the one-node
    encoder over the large-graph aggregate -- dense fragments of A_w / den as split-bf16 matrix products
    (band_aggregate.hip, with the row division and, in the backward, the dX1 addend), the other edges
    through the gather kernel -- against the fp32 oracle, dropout masks replayed."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd.resident import assemble_batch
    from connectome_gnn_amd.synthetic import generate_packed
    ds = generate_packed(ngraphs, 1000, 100, seed=11)
    b = assemble_batch(ds, torch.arange(ngraphs))
    torch.manual_seed(4)
    m = _model("sage", 5, hidden, dropout=dropout)
    sd0 = {k_: v.clone() for k_, v in m.state_dict().items()}
    m = m.to(DEV).train()
    m.record_dropout = True
    bd = b.to(DEV)
    lg = m(bd)
    assert m.impl_used == "fused"
    s = bd.structure()
    bf, bb = s.band_ops("sage", s.sage_norm())
    assert bf is not None and bb is not None and bf[1].covered > 0.5
    loss_g = torch.nn.functional.cross_entropy(lg, bd.labels)
    loss_g.backward()
    masks = P.recorded_masks(m, b.num_nodes, b.num_graphs) if dropout > 0 else None
    lo, loss_o, g32, st32 = P.oracle_run("sage", sd0, b, dropout, True, masks)
    _, _, g64, _ = P.oracle_run("sage", sd0, b, dropout, True, masks, dtype=torch.float64)
    torch.testing.assert_close(lg.detach().cpu(), lo, **TOL)
    torch.testing.assert_close(loss_g.detach().cpu(), loss_o, **TOL)
    floor = P.NoiseFloor("sage", sd0, b, dropout, masks)
    for k_, p in m.named_parameters():
        P.assert_grad(k_, p.grad, g32[k_], g64[k_], f"sage1000-p{dropout}", floor)
    sd = m.state_dict()
    for k_ in sd:
        if "running" in k_:
            torch.testing.assert_close(sd[k_].cpu(), st32[k_], **TOL)


# ------------------------------------------------------------------- argument validation (ADVICE)
@pytest.mark.parametrize("kind,hidden", [("gcn", 64), ("gcn", 128), ("sage", 64)])
def test_fused_paths_reject_wrong_dtype_and_width(kind, hidden):
    """The reference raises on float64 features, half models and a feature width that differs from
    in_channels (F.linear shape/dtype errors); the fused encoders hand raw pointers to the kernels,
    so they must check first instead of reading out of bounds."""
    import connectome_gnn_amd as C
    gs = C.generate_dataset(4, 40, 6, seed=1)
    b = C.collate_graphs(gs).to(DEV)
    m = _model(kind, 5, hidden).to(DEV).train()
    b64 = C.ConnectomeBatch(b.node_features.double(), b.edge_index, b.edge_weight, b.batch, b.labels, b.ptr)
    with pytest.raises(TypeError):
        m(b64)
    wide = C.ConnectomeBatch(torch.randn(b.num_nodes, 8, device=DEV), b.edge_index, b.edge_weight, b.batch,
                             b.labels, b.ptr)
    with pytest.raises(ValueError):
        m(wide)
    with pytest.raises(TypeError):
        _model(kind, 5, hidden).to(DEV).half()(b)
    m(b)                                                    # and the good batch still runs


@pytest.mark.parametrize("in_ch,hidden,sizes,k", [(5, 64, [84] * 16, 8), (2, 128, [360] * 6, 14), (8, 256, [1000] * 6, 100),
                                                  (5, 256, [700, 333, 1024, 64, 5, 900, 1000], 60), (3, 128, [1024] * 5, 40),
                                                  (16, 64, [500] * 9, 30), (5, 256, [360] * 16, 14)])
def test_fp16_storage_shape_sweep_vs_fp32_oracle(in_ch, hidden, sizes, k):
    """GCNConnectome(storage="fp16") over graph sizes 5 .. 1024 (uniform and ragged), hidden 64 / 128 / 256,
    1 .. 16 input features, row counts on both sides of the 4096 from which the half GEMMs go
    weight-stationary: against the fp32 oracle at fp16 resolution (the bars of the config-5 test).
    (ONE input feature is left out on purpose: layer 0 is then rank one, every channel of its BatchNorm output
    is the same signal up to sign, and half-rounded activations put up to 10 % on the classifier's weight
    gradient -- the fp32-storage path has 1e-6 there; tools/_bin/fp16_probe.py.  Two features: 2.5 %.)"""
    import connectome_gnn_amd as C
    gs = [C.generate_connectome(n, min(k, max(n // 2 * 2 - 2, 2)), seed=77 + i) for i, n in enumerate(sizes)]
    g = torch.Generator().manual_seed(in_ch + hidden)
    gs = [C.ConnectomeGraph(torch.randn(x.num_nodes, in_ch, generator=g), x.edge_index, x.edge_weight, x.label) for x in gs]
    b = C.collate_graphs(gs)
    torch.manual_seed(3)
    m = C.GCNConnectome(in_ch, hidden, dropout=0.0, storage="fp16")
    sd0 = {k_: v.clone() for k_, v in m.state_dict().items()}
    m = m.to(DEV).train()
    bd = b.to(DEV)
    lg = m(bd)
    assert m.impl_used == "fused" and m._fused_kind == "half"
    loss_g = torch.nn.functional.cross_entropy(lg, bd.labels)
    loss_g.backward()
    lo, loss_o, g32, st32 = P.oracle_run("gcn", sd0, b, 0.0, True, None)
    scale = float(lo.abs().max()) + 1e-3
    assert float((lg.detach().cpu() - lo).abs().max()) <= 1e-2 * scale
    assert abs(float(loss_g) - float(loss_o)) <= 1e-2 * abs(float(loss_o))
    for k_, p in m.named_parameters():
        w = g32[k_]
        if k_.startswith("convs.") and k_.endswith(".bias"):
            continue        # zero true gradient ahead of BatchNorm: rounding noise over rounding noise
        err = float((p.grad.cpu() - w).abs().max())
        assert err <= 3e-2 * float(w.abs().max()) + 1e-5, f"{k_}: {err:.3e} vs scale {float(w.abs().max()):.3e}"


# ------------------------------------------------- config 5 in fp16 storage against the fp32 oracle
@pytest.mark.parametrize("dropout", [0.0, 0.3])
def test_cfg5_fp16_storage_gcn_vs_fp32_oracle(dropout):
    """BASELINE config 5 as specified: 1000-ROI graphs at 10 % density, hidden 256, fp16 STORAGE with
    fp32 accumulation (GCNConnectome(storage="fp16"), gcn_half_path.py).  The reference has no fp16
    path (.half() raises), so the yardstick is the fp32 oracle at fp16 resolution: logits
    and loss within 1e-2 of their scale, every gradient within 3e-2 of its tensor's scale (three
    layers of half-rounded activations, 1000-node sums); with dropout the GPU's keep masks are
    replayed through the oracle."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd.resident import assemble_batch
    from connectome_gnn_amd.synthetic import generate_packed
    ds = generate_packed(4, 1000, 100, seed=9)
    b = assemble_batch(ds, torch.arange(4))
    torch.manual_seed(3)
    m = C.GCNConnectome(5, 256, dropout=dropout, storage="fp16")
    sd0 = {k_: v.clone() for k_, v in m.state_dict().items()}
    m = m.to(DEV).train()
    m.record_dropout = True
    bd = b.to(DEV)
    lg = m(bd)
    assert lg.dtype == torch.float32 and m.impl_used == "fused" and m._fused_kind == "half"
    loss_g = torch.nn.functional.cross_entropy(lg, bd.labels)
    loss_g.backward()
    masks = P.recorded_masks(m, b.num_nodes, b.num_graphs) if dropout > 0 else None
    lo, loss_o, g32, st32 = P.oracle_run("gcn", sd0, b, dropout, True, masks)
    scale = float(lo.abs().max()) + 1e-3
    assert float((lg.detach().cpu() - lo).abs().max()) <= 1e-2 * scale
    assert abs(float(loss_g) - float(loss_o)) <= 1e-2 * abs(float(loss_o))
    for k_, p in m.named_parameters():
        assert p.grad.dtype == torch.float32
        w = g32[k_]
        err = float((p.grad.cpu() - w).abs().max())
        assert err <= 3e-2 * float(w.abs().max()) + 1e-5, f"{k_}: {err:.3e} vs scale {float(w.abs().max()):.3e}"
    sd = m.state_dict()
    for k_ in sd:
        if "running" in k_:
            torch.testing.assert_close(sd[k_].cpu(), st32[k_], rtol=5e-3, atol=5e-4)
    m.eval()
    with torch.no_grad():
        e1, e2 = m.encode(bd), m.encode(bd)
    assert torch.equal(e1, e2) and torch.isfinite(e1).all()
    with pytest.raises(ValueError):
        C.GraphSAGEConnectome(5, 64, storage="fp16")


@pytest.mark.parametrize("offset,scale", [(0.0, 1.0), (3.0, 1.0), (-2.0, 0.25), (10.0, 1.0), (100.0, 1.0),
                                          (300.0, 1.0), (1000.0, 10.0), (-50.0, 0.1)])
def test_fused_gcn_layer0_moment_statistics_with_offset_features(offset, scale):
    """Layer 0's BatchNorm sums come from the second moments of P0 = A_hat X0 (fused_gcn_l0.hip),
    CENTRED on a per-workgroup shift (round 3): node features whose mean is many standard
    deviations (un-normalised strength / degree columns, mean / sigma up to 500 here) must still give
    the oracle's logits, loss, gradients and running statistics.  Up to a few sigma that is the usual
    fp32 tolerance.  Beyond, the fp32 reference ITSELF drifts from the exact answer (its X0 W0^T
    carries 2^-24 * mean of rounding against a spread of sigma): there logits / loss / running
    statistics must be within the usual tolerance of the fp32 oracle OR at least as close to the
    float64 oracle as the fp32 oracle is; gradients go through the suite's rules (tests/parity.py), and
    where the mean is >= 100 sigma the weight gradients must be markedly closer to float64 than the
    fp32 reference's."""
    import connectome_gnn_amd as C
    graphs = C.generate_dataset(12, 360, 14, seed=5)
    b = C.collate_graphs(graphs)
    b.node_features = b.node_features * scale + offset
    far = abs(offset) > 5.0 * scale
    torch.manual_seed(11)
    m = _model("gcn", 5, 64, dropout=0.0)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    lo, loss_o, g32, stats_o = P.oracle_run("gcn", sd0, b)
    lo64, loss64, g64, stats64 = P.oracle_run("gcn", sd0, b, dtype=torch.float64)
    m = m.to(DEV).train()
    bd = b.to(DEV)
    lg = m(bd)
    assert m.impl_used == "fused"
    loss_g = torch.nn.functional.cross_entropy(lg, bd.labels)
    loss_g.backward()

    def close(got, want32, want64, what, tol=TOL):
        got = got.detach().cpu()
        try:
            torch.testing.assert_close(got, want32, **tol)
            return
        except AssertionError:
            if not far:
                raise
        e_gpu = float((got.double() - want64).abs().max())
        e_cpu = float((want32.double() - want64).abs().max())
        assert e_gpu <= e_cpu + 1e-12, f"{what}: HIP {e_gpu:.3e} from float64, the fp32 oracle {e_cpu:.3e}"

    close(lg, lo, lo64, "logits")
    close(loss_g, loss_o, loss64, "loss")
    floor = P.NoiseFloor("gcn", sd0, b)
    worst = 0.0
    for k_, p in m.named_parameters():
        P.assert_grad(k_, p.grad, g32[k_], g64[k_], f"offset{offset}", floor)
        if k_.endswith("linear.weight"):
            e_gpu = float((p.grad.detach().cpu().double() - g64[k_]).abs().max())
            e_cpu = float((g32[k_].double() - g64[k_]).abs().max())
            worst = max(worst, e_gpu / max(e_cpu, 1e-30))
    if offset >= 100.0:
        # far from zero the centred layer 0 is not merely "as good as fp32": the weight gradients
        # must be several times CLOSER to float64 than the fp32 reference's own (measured 0.01-0.3).
        # ((-50, 0.1) is left to the rules above: there every fp32 evaluation -- the reference, the
        # layered and the fused HIP path -- shares one deviation from float64, tools/offset_probe.py.)
        assert worst <= 0.5, f"weight gradients are only {worst:.2f}x the fp32 oracle's distance from float64"
    sd = m.state_dict()
    for k_, v in stats_o.items():
        close(sd[k_], v, stats64[k_], k_, dict(rtol=2e-5, atol=1e-6))


def test_backward_unit_equals_backward():
    """ops.backward_unit (cached unit root gradient, no multiply in cross_entropy's backward) gives
    bit-identical gradients to loss.backward()."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd import ops
    b = C.collate_graphs(C.generate_dataset(16, 84, 8, seed=9)).to(DEV)
    grads = []
    for unit in (False, True):
        torch.manual_seed(3)
        m = _model("gcn", 5, 64, dropout=0.3).to(DEV).train()
        torch.manual_seed(4)
        loss = ops.cross_entropy(m(b), b.labels)
        assert loss.dim() == 0
        (ops.backward_unit if unit else torch.Tensor.backward)(loss)
        grads.append([p.grad.clone() for p in m.parameters()])
    for a, c in zip(*grads):
        assert torch.equal(a, c)
    # a non-unit root gradient still scales
    torch.manual_seed(3)
    m = _model("gcn", 5, 64, dropout=0.3).to(DEV).train()
    torch.manual_seed(4)
    (2.0 * ops.cross_entropy(m(b), b.labels)).backward()
    for a, p in zip(grads[0], m.parameters()):
        torch.testing.assert_close(p.grad, 2.0 * a, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_relabel_by_degree_is_an_invariance(kind):
    """PackedDataset.relabel_by_degree renumbers every subject's nodes; logits, loss and gradients
    of both models are those of the original numbering up to the order of the sums."""
    from connectome_gnn_amd.resident import assemble_batch
    from connectome_gnn_amd.synthetic import generate_packed
    ds = generate_packed(6, 360, 14, seed=8).to(DEV)
    ds2 = ds.relabel_by_degree()
    ids = torch.arange(6, device=DEV)
    outs = []
    for d in (ds, ds2):
        torch.manual_seed(5)
        m = _model(kind, 5, 64, dropout=0.0).to(DEV).train()
        b = assemble_batch(d, ids)
        lg = m(b)
        loss = torch.nn.functional.cross_entropy(lg, b.labels)
        loss.backward()
        outs.append((lg.detach(), loss.detach(), [p.grad.clone() for p in m.parameters()]))
    # the same multiset of degrees per subject, now non-increasing along the node index
    def degrees(d):
        z = torch.zeros(6, 360, dtype=torch.long, device=DEV)
        return z.scatter_add_(1, d.edge_local[:, 1], torch.ones_like(d.edge_local[:, 1])) \
                .scatter_add_(1, d.edge_local[:, 0], torch.ones_like(d.edge_local[:, 0]))
    d1, d2 = degrees(ds), degrees(ds2)
    assert bool((d2[:, 1:] <= d2[:, :-1]).all()) and torch.equal(d1.sort(1).values, d2.sort(1).values)
    torch.testing.assert_close(outs[0][0], outs[1][0], rtol=2e-5, atol=2e-6)
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=2e-5, atol=2e-6)
    for a, c in zip(outs[0][2], outs[1][2]):
        torch.testing.assert_close(a, c, rtol=1e-3, atol=1e-5 * float(a.abs().max()) + 2e-6)


def test_degree_ordered_twin_is_the_same_model_on_ragged_batches():
    """prepare_batch(reuse=True): the per-tile GCN encoder runs on the batch's degree-ordered twin
    (every graph's nodes renumbered by decreasing degree inside the structure; node features gathered
    through the permutation).  Same logits, loss and gradients as on the batch's own order up to the
    order of the sums; less blocked-ELL padding; the public batch untouched."""
    import connectome_gnn_amd as C
    gs = C.generate_dataset(5, 84, 8, seed=9) + C.generate_dataset(3, 200, 12, seed=10) + C.generate_dataset(2, 33, 4, seed=11)
    b = C.collate_graphs(gs).to(DEV)
    ei0 = b.edge_index.clone()
    outs = []
    for reuse in (False, True):
        torch.manual_seed(2)
        m = C.GCNConnectome(5, 64, dropout=0.0).to(DEV).train()
        if reuse:
            m.prepare_batch(b, reuse=True)
        lg = m(b)
        assert m.impl_used == "fused"
        torch.nn.functional.cross_entropy(lg, b.labels).backward()
        outs.append((lg.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    s = b.structure()
    tw = s.__dict__["_degree_twin"]
    assert torch.equal(b.edge_index, ei0)
    grid = 256
    pad = lambda st: int(st.fused_meta(384, grid).blk_off_dst[-1])
    assert pad(tw) < pad(s)                                           # fewer padded blocked-ELL entries
    # nodes stay inside their graphs
    assert torch.equal(s.node_graph.to(torch.long)[tw.perm], s.node_graph.to(torch.long))
    torch.testing.assert_close(outs[1][0], outs[0][0], rtol=1e-5, atol=2e-6)
    for k, g0 in outs[0][1].items():
        if k.startswith("convs.") and k.endswith(".bias"):
            continue
        g1 = outs[1][1][k]
        assert float((g1 - g0).abs().max()) <= 2e-5 * float(g0.abs().max()) + 2e-6, k


def test_encoder_choice_is_per_call_not_per_model():
    """One GCN (hidden 64, 4 input features, 2 layers, eval) prepared for two kept batches -- A on the per-tile
    kernels, B (a 400-node graph) on the wide encoder -- and run on A, B, A: each call runs and records its own
    encoder, and A's logits are bit-equal both times and to those of a model that only ever saw A."""
    import connectome_gnn_amd as C

    def cut(graphs):                                   # the generator makes 5 features: keep 4
        return [C.ConnectomeGraph(g.node_features[:, :4].contiguous(), g.edge_index, g.edge_weight, g.label)
                for g in graphs]
    ga = cut(C.generate_dataset(3, 20, 4, seed=3))
    gb = cut([C.generate_connectome(400, 6, seed=2), C.generate_connectome(20, 4, seed=4)])
    a, b = C.collate_graphs(ga).to(DEV), C.collate_graphs(gb).to(DEV)
    torch.manual_seed(6)
    m = C.GCNConnectome(4, 64, num_layers=2).to(DEV).eval()
    m.prepare_batch(a, reuse=True)
    m.prepare_batch(b, reuse=True)
    outs, kinds = [], []
    with torch.no_grad():
        for batch in (a, b, a):
            outs.append(m(batch).clone())
            kinds.append((m.impl_used, m._fused_kind))
    assert kinds == [("fused", "tile"), ("fused", "wide"), ("fused", "tile")]
    assert torch.equal(outs[0], outs[2])
    only_a = C.GCNConnectome(4, 64, num_layers=2).to(DEV).eval()
    only_a.load_state_dict(m.state_dict())
    a2 = C.collate_graphs(ga).to(DEV)
    only_a.prepare_batch(a2, reuse=True)
    with torch.no_grad():
        assert torch.equal(only_a(a2), outs[0])
    assert only_a._fused_kind == "tile" and torch.isfinite(outs[1]).all()


@pytest.mark.parametrize("mode", ["keep", "drop"])
def test_capture_with_a_live_earlier_autograd_graph_raises_instead_of_crashing(mode):
    """building a captured step while a non-detached `loss` of an earlier eager step is alive used to
    end in a segmentation fault inside capture_end (stale AccumulateGrad nodes bound to the default stream).
    GraphedTrainStep now detects the condition before capturing and raises; once the tensors are dropped the
    same call captures and replays.  Run in a child process (tools/capture_probe.py): undetected, the condition
    kills the interpreter."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "capture_probe.py"), mode], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "captured + replayed ok" in r.stdout
    if mode == "keep":
        assert "detected:" in r.stdout


def test_kernel_timer_keys_the_benchmark_reads_are_recorded(monkeypatch):
    """bench.py's roofline line reads per-kernel times from a KernelTimer under fixed keys; a key that no launch
    records any more prints 0 there without failing anything.  One eager forward + backward on the smallest batch
    that reaches each path (the rows of tools/encoder_bits.py), and every key must have recorded a launch."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd import _lib
    gen = C.generate_dataset
    cases = [("cgnn_gcn_fused_bwd", 64, lambda: gen(4, 84, 8, seed=1)),                                   # "tile"
             ("cgnn_aggregate_tiled_f32[F=128]", 128, lambda: gen(4, 84, 8, seed=2)),                     # "wide h128"
             ("cgnn_band_aggregate_f32+cgnn_aggregate_acc_f32[F=64]", 64,
              lambda: gen(2, 400, 6, seed=3) + gen(1, 30, 4, seed=4)),                                    # "wide 400 band"
             # more than 1024 nodes in a graph: no band operator, the plain CSR gather aggregate ("wide 1100")
             ("cgnn_aggregate_f32[F=64]", 64, lambda: gen(1, 1100, 6, seed=9) + gen(1, 30, 4, seed=4))]
    timer = _lib.KernelTimer([key for key, _, _ in cases])
    monkeypatch.setattr(_lib, "TIMER", timer)
    for key, hidden, make in cases:
        torch.manual_seed(11)
        m = C.GCNConnectome(5, hidden, dropout=0.3).to(DEV).train()
        b = C.collate_graphs(make()).to(DEV)
        torch.nn.functional.cross_entropy(m(b), b.labels).backward()
    torch.cuda.synchronize()
    counts = {key: len(timer.events[key]) for key, _, _ in cases}
    print(counts)
    assert all(n >= 1 for n in counts.values()), counts
    assert all(ms >= 0.0 for key in counts for ms in timer.ms(key))
