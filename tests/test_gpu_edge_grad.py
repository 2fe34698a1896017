"""Differentiable edge weights: dL/d(batch.edge_weight) on the layered path (csrc/edge_grad.hip, ops.edge_weight_grad)
against the oracle's own autograd through a requires_grad edge weight (reference models.py:94-114, :146-149),
in fp32 and fp64 (tests/parity.py assert_grad), plus the kernels against torch on random CSR batches."""
import pytest
import torch

from oracle import reference_path as O
from tests import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = P.TOL


def _model(kind, in_ch, hidden, **kw):
    import connectome_gnn_amd as C
    return (C.GCNConnectome if kind == "gcn" else C.GraphSAGEConnectome)(in_ch, hidden, **kw)


def oracle_run_ew(kind, state_dict, b, edge_weight, dropout=0.0, training=True, masks=None, x_grad=False,
                  dtype=torch.float32):
    """oracle_run (tests/parity.py) with the edge weights (and optionally the node features) requiring grad.
    Returns (logits, {param: grad}, edge_weight grad, node_features grad or None)."""
    torch.set_default_dtype(dtype)
    try:
        cast = lambda v: v.detach().cpu().clone().to(dtype) if v.is_floating_point() else v.detach().cpu().clone()
        st = O.require_grad({k: cast(v) for k, v in state_dict.items()})
        ew = cast(edge_weight).requires_grad_(True)
        x = cast(b.node_features).requires_grad_(x_grad)
        ob = O.OBatch(x, b.edge_index.cpu(), ew, b.batch.cpu(), b.labels.cpu(), b.ptr.cpu())
        mk = None
        if masks is not None:
            mk = {"layers": [cast(m) for m in masks["layers"]], "head": cast(masks["head"])}
        logits = O.FORWARD[kind](st, ob, dropout, training, mk)
        torch.nn.functional.cross_entropy(logits, ob.labels).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    grads = {k: v.grad for k, v in st.items() if v.grad is not None}
    return logits.detach(), grads, ew.grad, (x.grad if x_grad else None)


def _fp64(fn):
    torch.set_default_dtype(torch.float64)
    try:
        return fn()
    finally:
        torch.set_default_dtype(torch.float32)


# ------------------------------------------------------------------------------------------ kernels
def _odd_batch(big=False):
    """Graphs with isolated nodes, duplicate edges, nodes without in-edges, an edgeless and an empty graph
    (and one of more than 384 nodes)."""
    import connectome_gnn_amd as C
    g = torch.Generator().manual_seed(3)
    dup = C.generate_connectome(40, 6, seed=1)
    dup = C.ConnectomeGraph(dup.node_features, torch.cat([dup.edge_index, dup.edge_index[:, :7]], 1),
                            torch.cat([dup.edge_weight, dup.edge_weight[:7] * 0.5]), dup.label)
    src = torch.randint(0, 20, (60,), generator=g)
    dst = torch.randint(0, 10, (60,), generator=g)                 # nodes 10..29: no in-edges, 20..29 isolated
    lop = C.ConnectomeGraph(torch.randn(30, 5), torch.stack([src, dst]), torch.rand(60, generator=g) + 0.1,
                            torch.tensor(1))
    graphs = [dup, lop, C.ConnectomeGraph(torch.randn(7, 5), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0),
                                          torch.tensor(0)),
              C.ConnectomeGraph(torch.zeros(0, 5), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0), torch.tensor(1)),
              C.generate_connectome(84, 10, seed=2)]
    if big:
        graphs.append(C.generate_connectome(500, 30, seed=4))
    return C.collate_graphs(graphs)


def _csr(s):
    return [t.cpu().long() for t in (s.rowptr_dst, s.col_dst, s.eid_dst)]


@pytest.mark.parametrize("F", [1, 5, 7, 32, 64, 100, 128, 256])
def test_sddmm_kernel_vs_torch(F):
    from connectome_gnn_amd import ops
    b = _odd_batch(big=F in (7, 64, 256)).to(DEV)
    s = b.structure()
    n, e = s.num_nodes, s.num_edges
    rp, col, eid = _csr(s)
    rows = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    g = torch.Generator().manual_seed(F)
    dy, x, xs = (torch.randn(n, F, generator=g) for _ in range(3))
    rowdiv = torch.rand(n, generator=g) + 0.5
    d64, x64, s64 = dy.double(), x.double(), xs.double()
    ref = (d64[rows] * x64[col]).sum(1)
    self_ref = (d64 * s64).sum(1)
    tol = dict(rtol=1e-5, atol=2e-5 * max(F, 16) ** 0.5)
    dyd, xd, xsd = dy.to(DEV), x.to(DEV), xs.to(DEV)
    # slot order, no per-row term
    got = ops.sddmm_raw(s.rowptr_dst, s.col_dst, None, dyd, xd)
    torch.testing.assert_close(got.cpu().double(), ref, **tol)
    # COO order through eid, the GCN self-loop term
    gself = torch.full((n,), float("nan"), device=DEV)
    got = ops.sddmm_raw(s.rowptr_dst, s.col_dst, s.eid_dst, dyd, xd, xself=xsd, gself=gself)
    want = torch.empty(e, dtype=torch.float64)
    want[eid] = ref
    torch.testing.assert_close(got.cpu().double(), want, **tol)
    torch.testing.assert_close(gself.cpu().double(), self_ref, **tol)
    # GraphSAGE's whole dw: (g - <dY[d], Y[d]>) / rowdiv[d], COO order
    got = ops.sddmm_raw(s.rowptr_dst, s.col_dst, s.eid_dst, dyd, xd, xself=xsd, rowdiv=rowdiv.to(DEV))
    want[eid] = (ref - self_ref[rows]) / rowdiv.double()[rows]
    torch.testing.assert_close(got.cpu().double(), want, rtol=1e-5, atol=4 * tol["atol"])
    # strided operands (column slices of wider buffers) take the same results
    wide = torch.randn(n, F + 3, device=DEV)
    wide[:, 1:F + 1] = xd
    got = ops.sddmm_raw(s.rowptr_dst, s.col_dst, None, dyd, wide[:, 1:F + 1])
    torch.testing.assert_close(got.cpu().double(), ref, **tol)


def test_gcn_norm_bwd_kernel_vs_torch():
    from connectome_gnn_amd import ops
    b = _odd_batch(big=True).to(DEV)
    s = b.structure()
    norm = s.gcn_norm()
    n, e = s.num_nodes, s.num_edges
    g = torch.Generator().manual_seed(5)
    gc, gself = torch.randn(e, generator=g), torch.randn(n, generator=g)
    dw = ops.gcn_norm_bwd_raw(s, s._edge_weight, norm.dis, gc.to(DEV), gself.to(DEV))
    src, dst = b.edge_index.cpu()
    w, dis, g64 = b.edge_weight.cpu().double(), norm.dis.cpu().double(), gc.double()
    ddis = (torch.zeros(n, dtype=torch.float64).index_add_(0, src, g64 * w * dis[dst])
            + torch.zeros(n, dtype=torch.float64).index_add_(0, dst, g64 * w * dis[src]) + 2 * dis * gself.double())
    want = g64 * dis[src] * dis[dst] - 0.5 * dis[src] ** 3 * ddis[src]
    torch.testing.assert_close(dw.cpu().double(), want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))


def test_short_scratch_and_bad_arguments_are_refused():
    from connectome_gnn_amd import _lib
    lib = _lib.load()
    b = _odd_batch().to(DEV)
    s = b.structure()
    norm = s.gcn_norm()
    n, e = s.num_nodes, s.num_edges
    gc, gself, dw = torch.zeros(e, device=DEV), torch.zeros(n, device=DEV), torch.zeros(e, device=DEV)
    need = int(lib.cgnn_gcn_norm_bwd_workspace_bytes(n))
    assert need >= 4 * n
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(nbytes, wsp=_lib.ptr(ws)):
        return lib.cgnn_gcn_norm_bwd(_lib.ptr(s.rowptr_dst), _lib.ptr(s.col_dst), _lib.ptr(s.eid_dst),
                                     _lib.ptr(s.rowptr_src), _lib.ptr(s.col_src), _lib.ptr(s.eid_src),
                                     _lib.ptr(s._edge_weight), _lib.ptr(norm.dis), _lib.ptr(gc), _lib.ptr(gself), n, e,
                                     _lib.ptr(dw), wsp, nbytes, _lib.stream_ptr())
    assert call(need - 4) == _lib.CGNN_EINVAL
    assert call(need, None) == _lib.CGNN_EINVAL
    assert call(need) == _lib.CGNN_OK
    x = torch.zeros(n, 64, device=DEV)
    sd = lambda xs, rd, gs, f=64: lib.cgnn_sddmm_f32(
        _lib.ptr(s.rowptr_dst), _lib.ptr(s.col_dst), None, _lib.ptr(x), 64, _lib.ptr(x), 64, xs, 64, rd, _lib.ptr(dw),
        gs, n, f, _lib.stream_ptr())
    assert sd(None, _lib.ptr(gself), None) == _lib.CGNN_EINVAL        # rowdiv without Xself
    assert sd(None, None, _lib.ptr(gself)) == _lib.CGNN_EINVAL        # gself without Xself
    assert sd(None, None, None, 0) == _lib.CGNN_EINVAL                # F = 0
    assert sd(None, None, None, 65) == _lib.CGNN_EINVAL               # row stride < F
    assert sd(_lib.ptr(x), None, _lib.ptr(gself)) == _lib.CGNN_OK
    torch.cuda.synchronize()
    # an empty CSR: nothing launched, nothing read
    assert lib.cgnn_sddmm_f32(None, None, None, None, 8, None, 8, None, 0, None, None, None, 0, 8,
                              _lib.stream_ptr()) == _lib.CGNN_OK


# ------------------------------------------------------------------------------------------ layers
def _layer_case(kind, n, k, fin, fout, seed, structure_check=None):
    import connectome_gnn_amd as C
    from connectome_gnn_amd.models import GCNLayer, SAGELayer, _AdHocBatch
    from connectome_gnn_amd.structure import BatchStructure
    gr = C.generate_connectome(n, k, seed=seed)
    ei, w0 = gr.edge_index, gr.edge_weight
    torch.manual_seed(seed)
    layer = (GCNLayer if kind == "gcn" else SAGELayer)(fin, fout)
    with torch.no_grad():
        if kind == "gcn":
            layer.bias.normal_()
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(n, fin, generator=g)
    r = torch.randn(n, fout, generator=g)
    layer = layer.to(DEV)
    ew = w0.to(DEV).requires_grad_(True)
    xd = x.to(DEV)
    s = BatchStructure.build(_AdHocBatch(xd, ei.to(DEV), ew))
    if structure_check is not None:
        structure_check(s, layer)
    y = layer(xd, ei.to(DEV), ew, structure=s)
    (y * r.to(DEV)).sum().backward()
    wt = layer.linear.weight.detach().cpu()
    bias = (layer.bias if kind == "gcn" else layer.linear.bias).detach().cpu()
    fn = O.gcn_layer if kind == "gcn" else O.sage_layer

    def oracle(dtype):
        def run():
            w = w0.clone().to(dtype).requires_grad_(True)
            (fn(x.to(dtype), ei, w, wt.to(dtype), bias.to(dtype)) * r.to(dtype)).sum().backward()
            return w.grad
        return _fp64(run) if dtype == torch.float64 else run()
    P.assert_grad("edge_weight", ew.grad, oracle(torch.float32), oracle(torch.float64), f"layer-{kind}-{n}-{fin}-{fout}")


@pytest.mark.parametrize("kind,n,k,fin,fout,form", [
    ("gcn", 84, 10, 5, 64, "aggregate-first"),     # layer 0: (A_hat X) W^T at in_channels
    ("gcn", 84, 10, 1, 16, "aggregate-first"),
    ("gcn", 90, 12, 64, 32, "gather"),             # CSR gather (width not a multiple of 64)
    ("gcn", 500, 20, 100, 100, "gather"),          # a graph over 384 nodes at an odd width
    ("gcn", 84, 10, 64, 64, "tiled"),
    ("gcn", 200, 14, 128, 128, "tiled"),
    ("gcn", 360, 16, 256, 256, "tiled"),
    ("gcn", 1000, 80, 64, 64, "band"),
    ("sage", 84, 10, 5, 64, "gather"),
    ("sage", 500, 20, 7, 32, "gather"),
    ("sage", 84, 10, 64, 64, "tiled"),
    ("sage", 200, 14, 128, 64, "tiled"),
    ("sage", 360, 16, 256, 64, "tiled"),
    ("sage", 1000, 80, 128, 64, "band"),
])
def test_layer_edge_grad_vs_oracle(kind, n, k, fin, fout, form):
    def check(s, layer):
        width = fout if kind == "gcn" else fin
        if form == "tiled":
            assert s.tiled_ok(width)
        elif form == "band":
            norm = s.gcn_norm() if kind == "gcn" else s.sage_norm()
            assert s.band_ops(kind, norm)[0] is not None
        elif form == "gather":
            assert not s.tiled_ok(width)
    _layer_case(kind, n, k, fin, fout, 7, check)


def test_adhoc_layer_call_without_structure():
    """The reference's GCNLayer(x, edge_index, edge_weight) call form (_AdHocBatch route)."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd.models import GCNLayer
    gr = C.generate_connectome(60, 8, seed=9)
    torch.manual_seed(0)
    layer = GCNLayer(5, 64).to(DEV)
    ew = gr.edge_weight.to(DEV).requires_grad_(True)
    layer(gr.node_features.to(DEV), gr.edge_index.to(DEV), ew).sum().backward()
    assert ew.grad is not None and ew.grad.shape == ew.shape and bool(ew.grad.abs().sum() > 0)


# ------------------------------------------------------------------------------------------ models
MODEL_CASES = [
    ("gcn", 84, 10, 64, 8), ("gcn", 120, 12, 128, 6), ("sage", 84, 10, 64, 8), ("sage", 100, 10, 128, 6),
]


@pytest.mark.parametrize("kind,n,k,hidden,nb", MODEL_CASES)
@pytest.mark.parametrize("mode", ["train0", "train_dropout", "eval"])
@pytest.mark.parametrize("x_grad", [False, True])
def test_model_edge_grad_vs_oracle(kind, n, k, hidden, nb, mode, x_grad):
    import connectome_gnn_amd as C
    b = C.collate_graphs(C.generate_dataset(nb, n, k, seed=77))
    p = 0.3 if mode == "train_dropout" else 0.0
    torch.manual_seed(4)
    m = _model(kind, 5, hidden, dropout=p, num_layers=3)
    sd0 = {k_: v.clone() for k_, v in m.state_dict().items()}
    m = m.to(DEV)
    m.train(mode != "eval")
    m.record_dropout = mode == "train_dropout"
    bd = b.to(DEV)
    ew = bd.edge_weight.clone().requires_grad_(True)
    bd.edge_weight = ew
    if x_grad:
        bd.node_features = bd.node_features.clone().requires_grad_(True)
    lg = m(bd)
    assert m.impl_used == "layered"
    torch.nn.functional.cross_entropy(lg, bd.labels).backward()
    assert ew.grad is not None
    masks = P.recorded_masks(m, b.num_nodes, b.num_graphs) if mode == "train_dropout" else None
    training = mode != "eval"
    lo, g32, e32, x32 = oracle_run_ew(kind, sd0, b, b.edge_weight, p, training, masks, x_grad)
    _, g64, e64, x64 = oracle_run_ew(kind, sd0, b, b.edge_weight, p, training, masks, x_grad, torch.float64)
    torch.testing.assert_close(lg.detach().cpu(), lo, **TOL)
    where = f"edge-{kind}-{n}-h{hidden}-{mode}"
    P.assert_grad("edge_weight", ew.grad, e32, e64, where)
    if x_grad:
        P.assert_grad("node_features", bd.node_features.grad, x32, x64, where)
    floor = P.NoiseFloor(kind, sd0, b, p, masks) if training else None
    for k_, prm in m.named_parameters():
        P.assert_grad(k_, prm.grad, g32[k_], g64[k_], where, floor)


def _flipped(flips):
    """O.RELU_HOOK taking the ReLU decisions listed in ``flips`` the other way (parity.oracle_run_flipped)."""
    by_site = {}
    for site, r, c in flips:
        by_site.setdefault(site, []).append((r, c))

    def hook(site, pre):
        if site not in by_site:
            return None
        mask = pre.detach() > 0
        for r, c in by_site[site]:
            mask[r, c] = ~mask[r, c]
        return mask
    return hook


def test_band_model_edge_grad_vs_oracle():
    """1000-ROI graphs (batches the band operator covers): the edge gradient of a 3-layer model against the
    oracle.  An edge gradient is local: a ReLU pre-activation within rounding of zero (parity.relu_ties) that
    an fp32 evaluation decides the other way moves the gradients of the edges around that node by O(1) of
    their size, so -- rule (4) of tests/parity.py -- the oracle is also evaluated with its ties decided the
    other way, subset by subset, and the HIP gradient must match one of those evaluations."""
    import itertools
    import connectome_gnn_amd as C
    b = C.collate_graphs([C.generate_connectome(1000, 80, seed=5), C.generate_connectome(1000, 80, seed=6)])
    torch.manual_seed(6)
    m = _model("gcn", 5, 64, dropout=0.0, num_layers=3)
    sd0 = {k_: v.clone() for k_, v in m.state_dict().items()}
    m = m.to(DEV).train()
    bd = b.to(DEV)
    ew = bd.edge_weight.clone().requires_grad_(True)
    bd.edge_weight = ew
    lg = m(bd)
    assert m.impl_used == "layered"
    s = bd.structure()
    assert s.band_ops("gcn", s.gcn_norm())[0] is not None
    torch.nn.functional.cross_entropy(lg, bd.labels).backward()
    ties = P.relu_ties("gcn", sd0, b)
    assert len(ties) <= 6
    errs = []
    for k in range(len(ties) + 1):
        for flips in itertools.combinations(ties, k):
            O.RELU_HOOK = _flipped(flips) if flips else None
            try:
                lo, _, e32, _ = oracle_run_ew("gcn", sd0, b, b.edge_weight)
                _, _, e64, _ = oracle_run_ew("gcn", sd0, b, b.edge_weight, dtype=torch.float64)
            finally:
                O.RELU_HOOK = None
            torch.testing.assert_close(lg.detach().cpu(), lo, **TOL)
            err = float((ew.grad.cpu().double() - e64).abs().max())
            errs.append(err)
            if err <= float((e32.double() - e64).abs().max()) + 1e-5 * float(e64.abs().max()):
                P.assert_grad("edge_weight", ew.grad, e32, e64, f"edge-band-gcn-ties{len(flips)}")
                return
    raise AssertionError(f"edge_weight: no ReLU-tie resolution of {ties} matches; errors {errs}")


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_mask_learning_loop_vs_oracle(kind):
    """A device mask Parameter through edge_weight = base * sigmoid(mask), three Adam steps: at every step the
    logits and mask.grad match the oracle evaluated at the same mask, and the oracle's own loop ends at the same
    mask."""
    import connectome_gnn_amd as C
    b = C.collate_graphs(C.generate_dataset(6, 84, 10, seed=12))
    torch.manual_seed(2)
    m = _model(kind, 5, 64, dropout=0.0)
    sd0 = {k_: v.clone() for k_, v in m.state_dict().items()}
    m = m.to(DEV).train()
    bd = b.to(DEV)
    base = bd.edge_weight.clone()
    e = base.numel()
    mask = torch.nn.Parameter(torch.zeros(e, device=DEV))
    opt = torch.optim.Adam([mask], lr=0.05)
    omask = torch.nn.Parameter(torch.zeros(e))
    oopt = torch.optim.Adam([omask], lr=0.05)
    obase = b.edge_weight.clone()
    for step in range(3):
        opt.zero_grad()
        bd.edge_weight = base * torch.sigmoid(mask)
        lg = m(bd)
        assert m.impl_used == "layered"
        torch.nn.functional.cross_entropy(lg, bd.labels).backward()
        assert mask.grad is not None

        def oracle(dtype, mvals):
            torch.set_default_dtype(dtype)
            try:
                mk = mvals.detach().cpu().to(dtype).requires_grad_(True)
                st = O.require_grad({k_: (v.to(dtype) if v.is_floating_point() else v) for k_, v in sd0.items()})
                ob = O.OBatch(b.node_features.to(dtype), b.edge_index, obase.to(dtype) * torch.sigmoid(mk), b.batch,
                              b.labels, b.ptr)
                lo = O.FORWARD[kind](st, ob, 0.0, True)
                torch.nn.functional.cross_entropy(lo, ob.labels).backward()
            finally:
                torch.set_default_dtype(torch.float32)
            return lo.detach(), mk.grad
        lo, g32 = oracle(torch.float32, mask)
        _, g64 = oracle(torch.float64, mask)
        torch.testing.assert_close(lg.detach().cpu(), lo, **TOL)
        P.assert_grad("mask", mask.grad, g32, g64, f"mask-loop-{kind}-step{step}")
        opt.step()
        # the oracle's own loop
        oopt.zero_grad()
        _, og = oracle(torch.float32, omask)
        omask.grad = og
        oopt.step()
    torch.testing.assert_close(mask.detach().cpu(), omask.detach(), rtol=0, atol=1e-4)


# ------------------------------------------------------------------------------------------ determinism, routing
@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_edge_grad_is_deterministic(kind):
    import connectome_gnn_amd as C
    b = C.collate_graphs([C.generate_connectome(84, 10, seed=i) for i in range(6)]
                         + [C.generate_connectome(500, 30, seed=9)]).to(DEV)
    torch.manual_seed(3)
    m = _model(kind, 5, 64, dropout=0.0).to(DEV).train()
    grads = []
    for _ in range(2):
        ew = b.edge_weight.detach().clone().requires_grad_(True)
        b.edge_weight = ew
        torch.nn.functional.cross_entropy(m(b), b.labels).backward()
        grads.append(ew.grad.clone())
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_routing_with_and_without_edge_grads(kind):
    import connectome_gnn_amd as C
    b = C.collate_graphs(C.generate_dataset(4, 84, 10, seed=1)).to(DEV)
    torch.manual_seed(0)
    m = _model(kind, 5, 64, dropout=0.0).to(DEV).train()
    m(b)
    assert m.impl_used == "fused"                     # no edge grads: unchanged
    b.edge_weight = b.edge_weight.clone().requires_grad_(True)
    with torch.no_grad():
        m(b)
    assert m.impl_used == "fused"                     # no autograd recording: unchanged
    m(b)
    assert m.impl_used == "layered"
    mf = _model(kind, 5, 64, dropout=0.0, impl="fused").to(DEV)
    with pytest.raises(RuntimeError, match="edge_weight requires grad"):
        mf(b)
    with torch.no_grad():
        mf(b)
    assert mf.impl_used == "fused"
    if kind == "gcn":
        mh = _model(kind, 5, 64, dropout=0.0, storage="fp16").to(DEV)
        with pytest.raises(RuntimeError, match="edge_weight requires grad"):
            mh(b)
