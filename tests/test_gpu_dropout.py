"""Every dropout draw of the package against the host model of tests/dropout_data.py, BIT FOR BIT: the keep
masks are a pure integer function of (seed, device word, row, chunk, p), so the kernels either draw the model's
bits or they are wrong.  csrc/drop_ew.h states the contract ("a fused consumer draws exactly the bits the
stand-alone apply pass would"; the three advancers "advance the words alike, so graph replay draws the masks an
eager run would"); tests/test_dropout_math.py establishes on the CPU that the model's bits are good noise.

The seeds are known because ``_lib.next_seed`` is wrapped (it still calls through, and logs) or replaced; the
masks come from ``model.record_dropout`` / ``record=``; the classifier's input from a wrapper around ``ops.head``
and ``ops.head_loss``.  Shapes are tiny: graphs of [84, 84, 20, 1, 384, 383, 3] nodes (two equal graphs, a
single node, a full tile, one row short of it), 5 features."""
import numpy as np
import pytest
import torch

from tests import dropout_data as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = 0.3
SIZES = [84, 84, 20, 1, 384, 383, 3]
SEEDS = {"all62": 2 ** 62 - 1, "low0": 0x2545F491_00000000, "high0": 0x00000000_9E3779B1}


# ------------------------------------------------------------------------------------------------ helpers
class Tap:
    """Wraps _lib.next_seed (calls through, or hands out ``forced`` in turn, and logs what it returned) and the two
    classifier entry points of ops (logs the pooled input).  The call sites reach all three through their modules."""

    def __init__(self, monkeypatch, forced=None):
        from connectome_gnn_amd import _lib, ops
        self.seeds, self.pooled = [], []
        real_seed, real_head, real_head_loss = _lib.next_seed, ops.head, ops.head_loss
        forced = list(forced) if forced is not None else None

        def next_seed(device=None):
            s = real_seed(device) if forced is None else forced[len(self.seeds) % len(forced)]
            self.seeds.append(int(s))
            return s

        def head(classifier, pooled, *a, **k):
            self.pooled.append(pooled.detach().clone())
            return real_head(classifier, pooled, *a, **k)

        def head_loss(classifier, pooled, *a, **k):
            self.pooled.append(pooled.detach().clone())
            return real_head_loss(classifier, pooled, *a, **k)

        monkeypatch.setattr(_lib, "next_seed", next_seed)
        monkeypatch.setattr(ops, "head", head)
        monkeypatch.setattr(ops, "head_loss", head_loss)


def _batch(sizes, k=3, f=5, seed=0):
    """Block-diagonal batch of random undirected graphs (both directions stored, no self-loops); a graph of 0
    nodes or 1 node has no edges."""
    import connectome_gnn_amd as C
    g = torch.Generator().manual_seed(seed)
    graphs = []
    for i, n in enumerate(sizes):
        if n > 1:
            s = torch.randint(0, n, (n * k,), generator=g)
            d = (s + torch.randint(1, n, (n * k,), generator=g)) % n
        else:
            s = d = torch.zeros(0, dtype=torch.long)
        w = torch.rand(s.numel(), generator=g) + 0.05
        graphs.append(C.ConnectomeGraph(torch.randn(n, f, generator=g), torch.stack([torch.cat([s, d]), torch.cat([d, s])]),
                                        torch.cat([w, w]), torch.tensor(i % 2)))
    return C.collate_graphs(graphs)


def _words(values):
    """uint32 values -> the int32 device vector the kernels read them from."""
    return torch.from_numpy(np.array(values, dtype=np.uint32).view(np.int32).copy()).to(DEV)


def _state(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


def _twin_inverse(batch):
    """inv with recorded[i] = twin_rows[inv[i]] (structure.unpermute_record), or None without a twin."""
    tw = getattr(batch.structure(), "__dict__", {}).get("_degree_twin")
    if tw is None:
        return None
    perm = tw.perm.cpu().numpy()
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    return inv


def _check_layers(layers, seeds, p, rows, width, words, inv, what):
    assert len(layers) == len(seeds) == len(words), (what, len(layers), len(seeds), len(words))
    for li, (mask, seed, word) in enumerate(zip(layers, seeds, words)):
        want = D.layer_keep(seed, p, rows, width, word)
        if inv is not None:
            want = want[inv]                       # the model's rows are the twin's; the record is un-permuted
        hit = D.first_mismatch(D.unpack(mask.cpu().numpy(), rows, width), want)
        assert hit is None, f"{what}: mask {li} (seed {seed:#x}, word {word:#x}) first differs at (row, column) {hit}"


def _head_decisions(fac, pooled, clf, seed, p, word):
    """(got, want, live): fac > 0 on the device, keep & (z > 0) of the model with the pre-activation in float64, and
    the elements that are not within 1e-5 of their row's largest |z| of a ReLU tie."""
    l1 = clf[0]
    z = (pooled.detach().double().cpu() @ l1.weight.detach().double().cpu().t() + l1.bias.detach().double().cpu()).numpy()
    live = np.abs(z) >= 1e-5 * np.abs(z).max(axis=1, keepdims=True)
    keep = D.head_keep(seed, p, z.shape[0], z.shape[1], word)
    return fac.detach().cpu().numpy() > 0, keep & (z > 0), live


def _check_head(fac, pooled, clf, seed, p, word, what):
    got, want, live = _head_decisions(fac, pooled, clf, seed, p, word)
    assert (~live).mean() <= 0.01, (what, float((~live).mean()))
    hit = D.first_mismatch(got & live, want & live)
    assert hit is None, f"{what}: head (seed {seed:#x}, word {word:#x}) first differs at (row, unit) {hit}"
    vals = np.unique(fac.detach().cpu().numpy())
    scale = np.float32(1.0 / (1.0 - float(np.float32(p))))
    assert set(vals.tolist()) <= {0.0, float(scale)}, (what, vals[:5])


def _model(kind, hidden, layers, dropout=P, **kw):
    import connectome_gnn_amd as C
    cls = C.GCNConnectome if kind == "gcn" else C.GraphSAGEConnectome
    m = cls(5, hidden, 2, layers, dropout, **kw).to(DEV).train()
    m.record_dropout = True
    return m


def _forward_and_check(m, bd, tap, path, what, p=P, words=None, inv=None):
    """One training forward; every layer mask and the head against the model with the logged seeds.  words: the
    values of the device words the draws read (None: eager without a state, every word 0)."""
    L, hidden = len(m.convs), m.batch_norms[0].num_features
    n0, h0 = len(tap.seeds), len(tap.pooled)
    m(bd)
    torch.cuda.synchronize()
    seeds = tap.seeds[n0:]
    assert len(seeds) == L + 1 and len(tap.pooled) == h0 + 1, (what, len(seeds))
    site = D.site_words(path, L)
    value = (lambda i: 0) if words is None else (lambda i: int(words[i]))
    rec = m.last_dropout
    _check_layers(rec["layers"], seeds[:L], p, bd.num_nodes, hidden, [value(i) for i in site["layers"]], inv, what)
    _check_head(rec["head_factor"], tap.pooled[-1], m.classifier, seeds[L], p, value(site["head"]), what)
    return seeds, [t.clone() for t in rec["layers"]]


# ------------------------------------------------------------------------------- every path, eager
WITH_EMPTY = SIZES[:3] + [0] + SIZES[3:]      # an empty graph, on the paths whose other tests run one
PATHS = [
    # name            kind   hidden L  model kwargs                    sizes             grid  path     impl_used / kind
    ("tile-L3",       "gcn",  64,   3, {},                              WITH_EMPTY,       0,    "tile",  ("fused", "tile")),
    ("tile-L3-grid3", "gcn",  64,   3, {},                              WITH_EMPTY,       3,    "tile",  ("fused", "tile")),
    ("tile-L1",       "gcn",  64,   1, {},                              WITH_EMPTY,       0,    "tile",  ("fused", "tile")),
    ("tile-L4",       "gcn",  64,   4, {},                              WITH_EMPTY,       0,    "tile",  ("fused", "tile")),
    ("layered-h32",   "gcn",  32,   3, {"impl": "layered"},             SIZES,            0,    "stage", ("layered", None)),
    ("wide-h128",     "gcn",  128,  3, {},                              SIZES + [400],    0,    "stage", ("fused", "wide")),
    ("sage-h64",      "sage", 64,   3, {},                              WITH_EMPTY,       0,    "stage", ("fused", None)),
    ("sage-h128",     "sage", 128,  3, {},                              WITH_EMPTY,       0,    "stage", ("fused", None)),
    ("fp16-h64",      "gcn",  64,   3, {"storage": "fp16"},             SIZES,            0,    "stage", ("fused", "half")),
]


@pytest.mark.parametrize("name,kind,hidden,layers,kw,sizes,grid,path,used", PATHS, ids=[c[0] for c in PATHS])
def test_every_path_draws_the_models_bits(monkeypatch, name, kind, hidden, layers, kw, sizes, grid, path, used):
    from connectome_gnn_amd import _lib
    lib = _lib.load()
    bd = _batch(sizes).to(DEV)
    torch.manual_seed(3)
    m = _model(kind, hidden, layers, **kw)
    tap = Tap(monkeypatch)
    assert lib.cgnn_set_fused_grid(grid) == 0
    try:
        _forward_and_check(m, bd, tap, path, name)
    finally:
        assert lib.cgnn_set_fused_grid(0) == 0
    assert m.impl_used == used[0] and (used[1] is None or m._fused_kind == used[1])


def test_degree_ordered_twin_draws_in_its_own_row_order(monkeypatch):
    """prepare_batch(reuse=True): the encoder runs on the batch's degree-ordered twin, so row r of the stream is
    the twin's node r; the record is returned in the batch's node order (structure.unpermute_record)."""
    bd = _batch(SIZES).to(DEV)
    torch.manual_seed(3)
    m = _model("gcn", 64, 3)
    m.prepare_batch(bd, reuse=True)
    inv = _twin_inverse(bd)
    assert inv is not None and not np.array_equal(inv, np.arange(inv.size))
    _forward_and_check(m, bd, Tap(monkeypatch), "tile", "twin", inv=inv)
    assert m.impl_used == "fused" and m._fused_kind == "tile"


def test_fused_and_layered_draw_identical_masks_from_the_same_seeds(monkeypatch):
    """drop_ew.h: "a fused consumer draws exactly the bits the stand-alone apply pass would" -- the per-tile
    kernels (phase A of the next layer, the readout) and the layered path's cgnn_bn_act_fwd_apply, h64, same seeds."""
    bd = _batch(SIZES).to(DEV)
    seeds = D.next_seeds(77, 0, 4)
    got = {}
    for impl in ("fused", "layered"):
        torch.manual_seed(3)
        m = _model("gcn", 64, 3, impl=impl)
        with monkeypatch.context() as mp:
            logged, got[impl] = _forward_and_check(m, bd, Tap(mp, forced=seeds), "tile" if impl == "fused" else "stage", impl)
        assert logged == seeds and m.impl_used == impl
    for li, (a, b) in enumerate(zip(got["fused"], got["layered"])):
        assert torch.equal(a, b), f"layer {li}: the fused and the layered path drew different bits"


def test_seeds_follow_the_device_generator(monkeypatch):
    """The real seed formula (the wrapper only listens): after torch.manual_seed(s) the seeds are
    mix64(mix64(s) + offset) >> 2 with the device generator's offset advancing by 4 per draw -- predicted from the
    generator's state BEFORE the forward, and the masks of a 3-layer fused forward are the model's with them."""
    bd = _batch(SIZES).to(DEV)
    for s in (5, 1234567):
        torch.manual_seed(s)
        m = _model("gcn", 64, 3)
        gen = torch.cuda.default_generators[torch.cuda.current_device()]
        off = int(gen.get_offset())
        assert int(gen.initial_seed()) == s
        predicted = D.next_seeds(s, off, 4)
        with monkeypatch.context() as mp:
            logged, _ = _forward_and_check(m, bd, Tap(mp), "tile", f"manual_seed({s})")
        assert logged == predicted, (s, off)
        assert int(gen.get_offset()) == off + 16


# ------------------------------------------------------------------------------------ direct calls
def _bn_reference_grad(y, mod, relu, keep, p, cot, out_dev):
    """dL/dy of sum(cot * drop(act(BatchNorm(y)))) in float64 with the MODEL's keep mask (ReLU decisions within
    1e-5 of the largest |z| of a tie are taken as the device took them)."""
    y64 = y.detach().double().cpu().requires_grad_(True)
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    z = (y64 - mean) / torch.sqrt(var + mod.eps) * mod.weight.detach().double().cpu() + mod.bias.detach().double().cpu()
    if relu:
        zd = z.detach()
        pos = torch.where(zd.abs() < 1e-5 * zd.abs().max(), out_dev.cpu() != 0, zd > 0)
        z = z * pos
    scale = float(np.float32(1.0 / (1.0 - float(np.float32(p)))))
    ((z * torch.from_numpy(keep) * scale) * cot.double().cpu()).sum().backward()
    return y64.grad


@pytest.mark.parametrize("p", [0.3, 0.5, 2.0 ** -17], ids=["p0.3", "p0.5", "p2^-17"])
@pytest.mark.parametrize("seed", list(SEEDS.values()), ids=list(SEEDS))
def test_direct_calls_with_chosen_seeds(monkeypatch, seed, p):
    """ops.bn_act_drop, ops.head and the BatchNorm-prologue aggregate with seeds that lose nothing only if all 64 bits
    travel from Python to make_drop (2^62 - 1; low half zero; high half zero), with and without a device word; the
    backward of the first two uses the forward's bits (float64 formula with the MODEL's mask, at the tolerances
    test_bn_act_drop_matches_torch and test_fused_head_matches_torch use for p = 0)."""
    from connectome_gnn_amd import _lib, ops
    tap = Tap(monkeypatch, forced=[seed])
    word_value = 0x9ABCDEF1
    word = _words([word_value])
    g = torch.Generator().manual_seed(11)
    for (rows, width), relu, use_word in (((257, 64), True, False), ((33, 256), False, True)):
        y = (torch.randn(rows, width, generator=g) * 1.7 + 0.3).to(DEV).requires_grad_(True)
        cot = torch.randn(rows, width, generator=g).to(DEV)
        mod = torch.nn.BatchNorm1d(width).to(DEV).train()
        with torch.no_grad():
            mod.weight.copy_(torch.linspace(0.5, 1.5, width))
            mod.bias.copy_(torch.linspace(-0.2, 0.3, width))
        rec = {}
        out = ops.bn_act_drop(y, mod, relu, p, True, word.data_ptr() if use_word else None, rec)
        (out * cot).sum().backward()
        what = f"bn_act_drop {rows}x{width}"
        _check_layers(rec["layers"], [seed], p, rows, width, [word_value if use_word else 0], None, what)
        keep = D.layer_keep(seed, p, rows, width, word_value if use_word else 0)
        want = _bn_reference_grad(y, mod, relu, keep, p, cot, out.detach())
        torch.testing.assert_close(y.grad.double().cpu(), want, rtol=1e-4, atol=2e-6 + 1e-5 * float(want.abs().max()),
                                   msg=lambda s_: f"{what}: the backward did not use the model's mask: {s_}")
    for (h, bsz), use_word in (((64, 37), False), ((256, 5), True), ((32, 1), True)):
        torch.manual_seed(h + bsz)
        clf = torch.nn.Sequential(torch.nn.Linear(h, h // 2), torch.nn.ReLU(), torch.nn.Dropout(p),
                                  torch.nn.Linear(h // 2, 2)).to(DEV)
        assert ops.head_supported(clf)
        x = torch.randn(bsz, h, generator=g).to(DEV).requires_grad_(True)
        cot = torch.randn(bsz, 2, generator=g).to(DEV)
        rec = {}
        wv = word_value if use_word else 0
        out = ops.head(clf, x, True, word.data_ptr() if use_word else None, rec)
        (out * cot).sum().backward()
        what = f"head h{h} B{bsz}"
        _check_head(rec["head_factor"], x, clf, seed, p, wv, what)
        got, want, live = _head_decisions(rec["head_factor"], x, clf, seed, p, wv)
        fac = np.where(live, want, got) * float(np.float32(1.0 / (1.0 - float(np.float32(p)))))
        x64 = x.detach().double().cpu().requires_grad_(True)
        l1, l2 = clf[0], clf[3]
        z = x64 @ l1.weight.detach().double().cpu().t() + l1.bias.detach().double().cpu()
        ref = (z * torch.from_numpy(fac)) @ l2.weight.detach().double().cpu().t() + l2.bias.detach().double().cpu()
        (ref * cot.double().cpu()).sum().backward()
        torch.testing.assert_close(x.grad.double().cpu(), x64.grad, rtol=1e-5, atol=1e-6,
                                   msg=lambda s_: f"{what}: the backward did not use the model's mask: {s_}")
        if ops.head_loss_supported(clf):
            rec2 = {}
            ops.head_loss(clf, x.detach(), torch.zeros(bsz, dtype=torch.long, device=DEV), True,
                          word.data_ptr() if use_word else None, rec2)
            assert torch.equal(rec2["head_factor"], rec["head_factor"]), f"{what}: head_loss drew other bits than head"
    # the BatchNorm prologue of the tiled aggregate (GraphSAGE's form), five graphs of 84 nodes, 64 features
    bd = _batch([84] * 5).to(DEV)
    s = bd.structure()
    lib = _lib.load()
    ell = s.fused_meta(384, int(lib.cgnn_fused_grid()), 0.0)
    norm = s.sage_norm(backward_coef=False)
    n, f = bd.num_nodes, 64
    z = torch.randn(n, f, generator=g).to(DEV)
    coef = torch.randn(4 * f, generator=g).to(DEV)
    for use_word in (False, True):
        mask = torch.zeros(n * f // 4, dtype=torch.uint8, device=DEV)
        x = torch.full_like(z, float("nan"))
        ops.aggregate_tiled_bn_raw(s, ell, ops.AGG_POST_DIV, z, None, norm.den, None, coef, False, p, seed,
                                   word.data_ptr() if use_word else None, mask, x)
        _check_layers([mask], [seed], p, n, f, [word_value if use_word else 0], None, "aggregate_tiled_bn")
        keep = torch.from_numpy(D.layer_keep(seed, p, n, f, word_value if use_word else 0)).to(DEV)
        assert torch.isfinite(x).all() and not bool((x != 0)[~keep].any())      # a dropped element is written as 0


# ------------------------------------------------------------------------------------- graph replay
GRAPHED = [("tile-h64", 64, {}, "tile", True), ("layered-h32", 32, {"impl": "layered"}, "stage", False),
           ("fp16-h64", 64, {"storage": "fp16"}, "stage", False)]


def _graphed(monkeypatch, hidden, layers, kw, sizes, head_loss):
    import connectome_gnn_amd as C
    from connectome_gnn_amd import ops
    from connectome_gnn_amd.graphed import GraphedTrainStep
    bd = _batch(sizes).to(DEV)
    bd.structure()
    torch.manual_seed(1)
    m = _model("gcn", hidden, layers, dropout=0.5, **kw)
    opt = torch.optim.SGD(m.parameters(), lr=0.0)                 # frozen weights: only the masks change
    tap = Tap(monkeypatch)
    step = GraphedTrainStep(m, opt, bd, loss_fn=ops.CrossEntropyLoss() if head_loss else None, warmup=1)
    assert isinstance(m, C.GCNConnectome) and len(tap.seeds) == 2 * (layers + 1)
    return bd, m, tap, step


def _replays_follow_the_model(bd, m, tap, step, path, what, replays=3):
    """After each replay: the state has moved by refresh on its first L + 1 words only, and every recorded mask is
    the model's with the seed frozen into the graph and the word the site table names."""
    L, hidden = len(m.convs), m.batch_norms[0].num_features
    seeds = tap.seeds[-(L + 1):]                                   # the capture's draws (the warm-up's came first)
    site = D.site_words(path, L)
    inv = _twin_inverse(bd)
    torch.cuda.synchronize()
    prev = _state(m.rng_device_state)
    for r in range(replays):
        step()
        torch.cuda.synchronize()
        cur = _state(m.rng_device_state)
        want = D.refresh_state(prev, site["advanced"])
        assert np.array_equal(cur, want), (what, r, np.flatnonzero(cur != want))
        rec = m.last_dropout
        _check_layers(rec["layers"], seeds[:L], 0.5, bd.num_nodes, hidden, [int(cur[i]) for i in site["layers"]], inv,
                      f"{what}, replay {r}")
        _check_head(rec["head_factor"], tap.pooled[-1], m.classifier, seeds[L], 0.5, int(cur[site["head"]]),
                    f"{what}, replay {r}")
        prev = cur


@pytest.mark.parametrize("name,hidden,kw,path,head_loss", GRAPHED, ids=[c[0] for c in GRAPHED])
def test_graph_replay_draws_the_models_bits_with_the_refreshed_words(monkeypatch, name, hidden, kw, path, head_loss):
    bd, m, tap, step = _graphed(monkeypatch, hidden, 3, kw, [84, 20, 1, 100, 3], head_loss)
    assert m.rng_device_state.numel() == 16
    _replays_follow_the_model(bd, m, tap, step, path, name)


def test_sixteen_layer_captured_step_owns_its_words(monkeypatch):
    """16 layers: the step advances 17 words and the classifier reads word 16 -- one past the 16-word state that
    GraphedTrainStep used to allocate whatever the model.  The state is sized from the model now; words 0..16
    follow refresh, and every mask (layer 15's, the readout's and the head's among them) is the model's."""
    bd, m, tap, step = _graphed(monkeypatch, 64, 16, {}, [20] * 4, True)
    assert m.impl_used == "fused" and m._fused_kind == "tile"
    assert m.rng_device_state.numel() == 17 and m.rng_device_state.dtype == torch.int32
    _replays_follow_the_model(bd, m, tap, step, "tile", "16 layers", replays=2)


def test_captured_step_refuses_dropout_words_it_cannot_own():
    from connectome_gnn_amd.graphed import GraphedTrainStep
    bd = _batch([20] * 4).to(DEV)
    m = _model("gcn", 64, 16, dropout=0.5)
    m.rng_device_state = torch.zeros(16, dtype=torch.int32, device=DEV)
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    with pytest.raises(ValueError, match="at least 17 words"):
        GraphedTrainStep(m, opt, bd, warmup=1)
    deep = _model("gcn", 64, 64, dropout=0.5)
    with pytest.raises(ValueError, match="at most 64"):
        GraphedTrainStep(deep, torch.optim.SGD(deep.parameters(), lr=0.0), bd, warmup=1)
    assert int(m.batch_norms[0].num_batches_tracked) == 0          # refused before any step was taken


# ------------------------------------------------------------------------------- the three advancers
START = [(0x9E3779B9 * (i + 3) ^ 0x5BD1E995 * i) & 0xFFFFFFFF for i in range(16)] + [0xFFFFFFFF, 0, 1, 0x80000000] * 12


@pytest.mark.parametrize("n", [1, 4, 16, 64])
def test_rng_advance_and_the_one_launch_finaliser_follow_refresh(n):
    from connectome_gnn_amd import _lib
    lib = _lib.load()
    sp = _lib.stream_ptr(torch.device(DEV))
    state = _words(START)
    _lib.check(lib.cgnn_rng_advance(_lib.ptr(state), n, sp), "cgnn_rng_advance")
    assert np.array_equal(_state(state), D.refresh_state(START, n))
    # cgnn_bn_stats_finalize_rng: a valid 4-row slab of [sum(64) | sumsq(64)] over 10 rows per workgroup
    g = torch.Generator().manual_seed(n)
    rows = torch.randn(4, 10, 64, generator=g, dtype=torch.float64)
    slab = torch.cat([rows.sum(1), (rows * rows).sum(1)], dim=1).to(DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    gamma, beta, rm, rv = torch.ones(64, **f32), torch.zeros(64, **f32), torch.zeros(64, **f32), torch.ones(64, **f32)
    tracked, bn_out = torch.zeros(1, dtype=torch.int64, device=DEV), torch.empty(256, **f32)
    state = _words(START)
    _lib.check(lib.cgnn_bn_stats_finalize_rng(_lib.ptr(slab), 4, 40.0, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(rm),
                                              _lib.ptr(rv), 0.1, 1e-5, _lib.ptr(tracked), _lib.ptr(bn_out),
                                              _lib.ptr(state), n, None, sp), "cgnn_bn_stats_finalize_rng")
    assert np.array_equal(_state(state), D.refresh_state(START, n))
    assert int(tracked) == 1 and bool(torch.isfinite(bn_out).all())
    mean = rows.reshape(40, 64).mean(0)
    torch.testing.assert_close(bn_out[128:192].double().cpu(), mean, rtol=1e-6, atol=1e-6)   # (it still finalised)


def test_rng_advance_refuses_no_words_and_more_than_a_state_holds():
    from connectome_gnn_amd import _lib
    lib = _lib.load()
    sp = _lib.stream_ptr(torch.device(DEV))
    state = _words(START)
    for n in (0, 65, -1):
        assert lib.cgnn_rng_advance(_lib.ptr(state), n, sp) == _lib.CGNN_EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(_state(state), np.array(START, dtype=np.uint32))


@pytest.mark.parametrize("layers", [1, 3, 15])
def test_eager_forward_with_a_state_advances_it_in_the_producers_tail(monkeypatch, layers):
    """The per-tile GCN refreshes the words inside layer 0's BatchNorm finalisation: the producer's tail for the
    narrow layer 0 (3 and 15 layers: n = 4, 16), the one-launch finaliser otherwise (1 layer: n = 2; a tail never
    advances a single word, since a model has at least one layer and the classifier).  The words beyond
    num_layers + 1 stay put, and the masks of the same forward are drawn with the refreshed words."""
    bd = _batch([84, 20, 1, 100, 3]).to(DEV)
    torch.manual_seed(4)
    m = _model("gcn", 64, layers)
    m.rng_device_state = _words(START[:32])
    _forward_and_check(m, bd, Tap(monkeypatch), "tile", f"eager with a state, {layers} layers",
                       words=D.refresh_state(START[:32], layers + 1))
    assert np.array_equal(_state(m.rng_device_state), D.refresh_state(START[:32], layers + 1))
    assert m.impl_used == "fused" and m._fused_kind == "tile"
