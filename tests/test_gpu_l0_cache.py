"""Kept batches: layer 0's batch constants (dis, P0 = A_hat X0 and the per-workgroup second moments of its
rows) are aggregated once (cgnn_gcn_l0_agg) and every step only turns the moments into its BatchNorm sums
(cgnn_gcn_l0_stats).  The split must not change a bit: every case below runs the same training twice on
the same kept batch -- once with the cache, once with ``fused._NO_L0_CACHE`` (cgnn_gcn_dis + cgnn_gcn_l0_fwd
on every step, the path of a batch that is not kept) -- and compares with ``torch.equal``.

Shapes: 10 x 360-ROI (one graph per tile); 30 x 360-ROI on 3 workgroups (two tiles per k_l0_fwd workgroup,
24 moment sets on 3 k_l0_stats workgroups = 8 sets each, all its groups busy); 64 x 84-ROI (four graphs per
tile); graphs of 5 .. 360 nodes; one 5-node graph (255 of the 256 moment sets are zero).  F0 = 8 is the raw
form (no spare column for the centring), F0 = 1 the narrowest centred one."""
import copy
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _graphs(name):
    import connectome_gnn_amd as C
    if name in ("10x360", "30x360-grid3"):
        return tuple(C.generate_dataset(10 if name == "10x360" else 30, 360, 14, seed=3))
    if name == "64x84":
        return tuple(C.generate_dataset(64, 84, 8, seed=4))
    if name == "ragged":
        sizes = [5, 17, 84, 200, 360, 33, 120, 6, 359, 48, 361 - 84, 16]
        return tuple(C.generate_connectome(n, 4 if n < 20 else 8, seed=100 + i) for i, n in enumerate(sizes))
    assert name == "single5"
    return (C.generate_connectome(5, 4, seed=9),)


BATCHES = ["10x360", "30x360-grid3", "64x84", "ragged", "single5"]


def _batch(name, f0, offset=0.0):
    """The named batch on the device with F0 feature columns (the generator's five, repeated and rescaled
    per column, cut to F0) plus `offset`."""
    import connectome_gnn_amd as C
    b = C.collate_graphs(list(_graphs(name)))
    x = b.node_features
    x = torch.cat([x, 0.5 * x + 0.25], dim=1)[:, :f0].contiguous()
    b.node_features = x + offset
    return b.to(DEV)


@pytest.fixture
def grid_for(request):
    """cgnn_set_fused_grid(3) for the '-grid3' batch, restored afterwards (as test_gpu_multiunit does)."""
    from connectome_gnn_amd import _lib
    lib = _lib.load()
    full = int(lib.cgnn_fused_grid())

    def use(name):
        if name.endswith("-grid3"):
            assert lib.cgnn_set_fused_grid(3) == 0
    try:
        yield use
    finally:
        torch.cuda.synchronize()
        assert lib.cgnn_set_fused_grid(0) == 0
        assert int(lib.cgnn_fused_grid()) == full


def _snapshot(m, loss):
    out = {"loss": loss.detach().clone()}
    for k, p in m.named_parameters():
        out["grad:" + k] = p.grad.detach().clone()
        out["param:" + k] = p.detach().clone()
    for k, v in m.named_buffers():                       # running_mean / running_var / num_batches_tracked
        out["buffer:" + k] = v.detach().clone()
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs (max abs diff " \
                                        f"{(a[k].double() - b[k].double()).abs().max().item():.3e})"


def _train(monkeypatch, model, batch, no_cache, steps=3, edit_after=None):
    """`steps` eager training steps with the project's Adam on the kept batch; a snapshot after every step.
    edit_after: after that step (1-based) the batch's features are doubled in place."""
    from connectome_gnn_amd import fused
    from connectome_gnn_amd.optim import Adam
    monkeypatch.setattr(fused, "_NO_L0_CACHE", no_cache)
    torch.manual_seed(17)                                # the dropout draws
    m = copy.deepcopy(model).to(DEV).train()
    m.prepare_batch(batch, reuse=True)
    opt = Adam(m.parameters(), lr=1e-2)
    snaps = []
    for i in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(m(batch), batch.labels)
        loss.backward()
        assert m.impl_used == "fused" and m._fused_kind == "tile"
        opt.step()
        snaps.append(_snapshot(m, loss))
        if edit_after == i + 1:
            batch.node_features.mul_(2)
    torch.cuda.synchronize()
    return snaps, m


def _kept_structure(batch):
    s = batch.structure()
    return s.__dict__.get("_degree_twin") or s


def _pair(monkeypatch, name, f0, no_tails, offset=0.0, edit_after=None, steps=3):
    import connectome_gnn_amd as C
    from connectome_gnn_amd import fused
    monkeypatch.setattr(fused, "_NO_TAILS", no_tails)
    torch.manual_seed(5)
    model = C.GCNConnectome(f0, 64, 2, 3, 0.3)
    ba, bb = _batch(name, f0, offset), _batch(name, f0, offset)
    off, _ = _train(monkeypatch, model, ba, True, steps, edit_after)
    assert "_l0_batch" not in _kept_structure(ba).__dict__ and "_dis" not in _kept_structure(ba).__dict__
    on, _ = _train(monkeypatch, model, bb, False, steps, edit_after)
    st = _kept_structure(bb)
    assert st.__dict__.get("_kept") and "_l0_batch" in st.__dict__ and "_dis" in st.__dict__
    for i, (a, b) in enumerate(zip(off, on)):
        _assert_same(a, b, f"{name} F0={f0} no_tails={no_tails} step {i + 1}")
    return st


@pytest.mark.parametrize("no_tails", [False, True], ids=["tails", "slab"])
@pytest.mark.parametrize("f0", [1, 5, 7, 8])
@pytest.mark.parametrize("name", BATCHES)
def test_cache_on_equals_cache_off(monkeypatch, grid_for, name, f0, no_tails):
    grid_for(name)
    st = _pair(monkeypatch, name, f0, no_tails)
    if name == "30x360-grid3":
        # 10800 nodes -> 43 wanted, capped at 8 x 3: 24 moment sets, 8 per k_l0_stats workgroup; 30 tiles on 24
        # k_l0_fwd workgroups
        assert st.__dict__["_l0_batch"][4].shape == (24, 81)


@pytest.mark.parametrize("no_tails", [False, True], ids=["tails", "slab"])
def test_cache_with_features_far_from_zero(monkeypatch, no_tails):
    """Features offset by 100: the centred form (P0' and the W0 c column) carries the result."""
    _pair(monkeypatch, "10x360", 5, no_tails, offset=100.0)


def test_eval_forward_equal(monkeypatch):
    """Eval mode: no statistics; k_l0_stats only writes w_eff / mean_offset (centred) or is not launched (raw)."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd import fused
    for f0 in (5, 8):
        torch.manual_seed(5)
        model = C.GCNConnectome(f0, 64, 2, 3, 0.3)
        outs = []
        for no_cache in (True, False):
            monkeypatch.setattr(fused, "_NO_L0_CACHE", no_cache)
            b = _batch("64x84", f0)
            m = copy.deepcopy(model).to(DEV).eval()
            m.prepare_batch(b, reuse=True)
            with torch.no_grad():
                outs.append(m(b).clone())
            assert m.impl_used == "fused"
        assert torch.equal(outs[0], outs[1]), f0


@pytest.mark.parametrize("no_tails", [False, True], ids=["tails", "slab"])
def test_in_place_feature_edit_reaggregates(monkeypatch, no_tails):
    """batch.node_features.mul_(2) after step 1: the next eager steps aggregate the new features."""
    _pair(monkeypatch, "64x84", 5, no_tails, edit_after=1)


def test_captured_steps_equal(monkeypatch):
    """GraphedTrainStep on a kept batch, with and without the cache: three replays each, all results equal."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd import _lib, fused
    from connectome_gnn_amd.graphed import GraphedTrainStep
    from connectome_gnn_amd.optim import Adam
    torch.manual_seed(5)
    model = C.GCNConnectome(5, 64, 2, 3, 0.3)
    runs = []
    for no_cache in (True, False):
        monkeypatch.setattr(fused, "_NO_L0_CACHE", no_cache)
        monkeypatch.setattr(_lib, "_capture_gen", None)   # the seeds frozen into the graph: the same draw
        torch.manual_seed(17)
        b = _batch("64x84", 5)
        m = copy.deepcopy(model).to(DEV).train()
        opt = Adam(m.parameters(), lr=1e-2)
        step = GraphedTrainStep(m, opt, b, warmup=1)
        assert ("_l0_batch" in _kept_structure(b).__dict__) == (not no_cache)
        snaps = []
        for _ in range(3):
            loss = step()
            snaps.append(_snapshot(m, loss))
        torch.cuda.synchronize()
        runs.append(snaps)
        del step
    for i, (a, b_) in enumerate(zip(*runs)):
        _assert_same(a, b_, f"replay {i + 1}")


def test_short_buffers_and_wrong_set_count_are_refused():
    """ABI 2: CGNN_EINVAL before any launch, outputs untouched."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd import _lib, fused
    lib = _lib.load()
    b = _batch("10x360", 5)
    s = b.structure()
    grid = int(lib.cgnn_fused_grid())
    meta = s.fused_meta(fused.MAX_ROWS, grid)
    tiles = s.tiles_struct(meta, s.gcn_dis(meta))
    tp = ctypes.byref(tiles)
    sp = _lib.stream_ptr(torch.device(DEV))
    nn_, sets = s.num_nodes, int(lib.cgnn_l0_grid(s.num_nodes))
    f32 = dict(dtype=torch.float32, device=DEV)
    p0 = torch.full((nn_, 8), 7.0, **f32)
    moments = torch.full((sets, 81), 7.0, dtype=torch.float64, device=DEV)
    one = torch.full((1,), 7, dtype=torch.uint8, device=DEV)
    assert lib.cgnn_gcn_l0_agg(tp, _lib.ptr(b.node_features), 5, None, _lib.ptr(p0), _lib.ptr(one), 1, sp) == -1
    assert lib.cgnn_gcn_l0_agg(tp, _lib.ptr(b.node_features), 5, None, _lib.ptr(p0), None, 0, sp) == -1
    torch.cuda.synchronize()
    assert bool((p0 == 7.0).all()) and int(one[0]) == 7
    assert lib.cgnn_gcn_l0_agg(tp, _lib.ptr(b.node_features), 5, None, _lib.ptr(p0), _lib.ptr(moments),
                               _lib.nbytes(moments), sp) == 0
    w, bias = torch.randn(64, 5, **f32), torch.randn(64, **f32)
    slab = torch.full((sets, 128), 7.0, dtype=torch.float64, device=DEV)
    args = (5, _lib.ptr(w), _lib.ptr(bias), None, None, None)
    assert lib.cgnn_gcn_l0_stats(_lib.ptr(moments), sets, *args, _lib.ptr(one), 1, None, sp) == -1
    assert sets == grid                                   # 3600 nodes: one set per CU, the bottom of cgnn_l0_grid's range
    for bad_sets in (8 * grid + 1, grid - 1, 0):          # no value cgnn_l0_grid returns
        assert lib.cgnn_gcn_l0_stats(_lib.ptr(moments), bad_sets, *args, _lib.ptr(slab), _lib.nbytes(slab), None, sp) == -1
    # with a tail the call knows the batch's row count: a set count of another batch size is refused
    m = C.GCNConnectome(5, 64, 2, 3, 0.3).to(DEV)
    bn_mod = m.batch_norms[0]
    bn_out = torch.full((256,), 7.0, **f32)
    rm0, nbt0 = bn_mod.running_mean.clone(), bn_mod.num_batches_tracked.clone()
    tail = fused._tail_fwd(bn_mod, bn_out.device, float(300 * 8 * grid), bn_mod.weight, bn_mod.bias, bn_out, None, 0)
    assert int(lib.cgnn_l0_grid(300 * 8 * grid)) != sets
    assert lib.cgnn_gcn_l0_stats(_lib.ptr(moments), sets, *args, None, 0, ctypes.byref(tail), sp) == -1
    torch.cuda.synchronize()
    assert int(one[0]) == 7 and bool((slab == 7.0).all()) and bool((bn_out == 7.0).all())
    assert torch.equal(bn_mod.running_mean, rm0) and torch.equal(bn_mod.num_batches_tracked, nbt0)
    assert not bool(fused._bn_acc(bn_mod, bn_out.device, 0).any())
    # and the accepted call writes every row of the slab
    assert lib.cgnn_gcn_l0_stats(_lib.ptr(moments), sets, *args, _lib.ptr(slab), _lib.nbytes(slab), None, sp) == 0
    torch.cuda.synchronize()
    assert not bool((slab == 7.0).any())
