"""Host tests (no device) of the encoder choice: encoder_choice.choose as a decision table, its purity, and
Trainer._subject_cache_serves.  The expected values are what the commit before this module existed answered
on the same inputs (its _try_fused / _fused_kind / _subject_cache_serves, driven by a throw-away script over
CASES and CACHE_CASES below)."""
import types

import pytest
import torch
import torch.nn as nn

import connectome_gnn_amd as C
from connectome_gnn_amd import encoder_choice
from connectome_gnn_amd.structure import EDGE_GRAD_REASON, BatchStructure


class NoCsr:
    """Stand-in for a structure assembled from a per-subject cache: the declared interface and no CSR."""
    has_csr = False
    cache = object()
    _edge_weight = _degree_twin = _kept = None

    def __init__(self):
        self._path_agreement = {}

    def tiled_ok(self, width):
        return width % 64 == 0 and self.block_diagonal and self.num_nodes > 0 and self.max_nodes_per_graph <= 384


class _Bn(nn.BatchNorm1d):
    """A BatchNorm1d subclass: passes fused.eligible's BatchNorm check, fails bn_stage.bn_modules_ok's type test."""


def build(kind="gcn", fin=4, hid=64, layers=2, impl="auto", storage="fp32", sizes=(20, 20, 20), csr=True,
          block_diagonal=True, x_grad=False, ew_grad=False, bn=None):
    """(model, batch, structure) on the CPU, the structure filled by hand."""
    torch.manual_seed(0)
    cls = C.GCNConnectome if kind == "gcn" else C.GraphSAGEConnectome
    m = cls(fin, hid, 2, layers, 0.3, impl=impl, storage=storage)
    if bn == "no_stats":
        m.batch_norms = nn.ModuleList(nn.BatchNorm1d(hid, track_running_stats=False) for _ in range(layers))
    elif bn == "subclass":
        m.batch_norms = nn.ModuleList(_Bn(hid) for _ in range(layers))
    elif bn == "sync":
        m.batch_norms = nn.ModuleList(nn.SyncBatchNorm(hid) for _ in range(layers))
    s = BatchStructure() if csr else NoCsr()
    s.num_nodes, s.num_graphs, s.max_nodes_per_graph = sum(sizes), len(sizes), max(sizes)
    s.block_diagonal = block_diagonal
    s._edge_weight = torch.ones(8, requires_grad=ew_grad)
    x = torch.zeros(sum(sizes), fin, requires_grad=x_grad)
    b = types.SimpleNamespace(node_features=x, num_nodes=sum(sizes), num_graphs=len(sizes), labels=None)
    return m, b, s


BIG = (385, 20)
RAISE = "raise"
X_GRAD_TILE = ("node_features require grad: the fused path returns the input gradient from its narrow layer 0 "
               "only (in_channels <= 8 and num_layers >= 2)")
OFF_TILES = "graphs do not fit an LDS tile and hidden_dim is not 64, 128 or 256"
# name: (build kwargs, expected kind, expected record in model._fused_kind, expected reason)
#   kind RAISE: choose() raises RuntimeError with `reason` as its whole message
CASES = {
    "gcn-h64":             (dict(), "tile", "tile", None),
    "gcn-h64-f16":         (dict(fin=16), "tile", "tile", None),
    "gcn-h64-384":         (dict(sizes=(384, 20)), "tile", "tile", None),
    "gcn-h64-f17":         (dict(fin=17), "wide", "wide", None),
    "gcn-h128":            (dict(hid=128), "wide", "wide", None),
    "gcn-h64-385-csr":     (dict(sizes=BIG), "wide", "wide", None),
    "gcn-h64-385-nocsr":   (dict(sizes=BIG, csr=False), None, "tile", "a graph has more than 384 nodes"),
    "gcn-h64-nocsr":       (dict(csr=False), "tile", "tile", None),
    "gcn-h32":             (dict(hid=32), None, "tile", "hidden_dim != 64"),
    "gcn-h32-fused":       (dict(hid=32, impl="fused"), RAISE, None,
                            "impl='fused' requested but not applicable: hidden_dim != 64"),
    "gcn-h64-f64":         (dict(fin=64), None, "tile", "in_channels > 16"),
    "gcn-layered":         (dict(impl="layered"), None, None, None),
    "gcn-fp16":            (dict(storage="fp16", sizes=(400, 400)), "half", "half", None),
    "gcn-fp16-layered":    (dict(storage="fp16", impl="layered"), "half", "half", None),
    "gcn-fp16-1025":       (dict(storage="fp16", sizes=(1025,)), RAISE, None,
                            "storage='fp16' requested but not applicable: a graph has more than 1024 nodes"),
    "gcn-cross-csr":       (dict(block_diagonal=False), "wide", "wide", None),
    "gcn-cross-nocsr":     (dict(block_diagonal=False, csr=False), None, "tile", "edges cross graph boundaries"),
    "gcn-xgrad-narrow":    (dict(x_grad=True, fin=8), "tile", "tile", None),
    "gcn-xgrad-f12":       (dict(x_grad=True, fin=12), None, "tile", X_GRAD_TILE),
    "gcn-xgrad-1layer":    (dict(x_grad=True, layers=1), None, "tile", X_GRAD_TILE),
    "gcn-xgrad-h128":      (dict(x_grad=True, hid=128), None, "tile", "hidden_dim != 64"),
    "gcn-ewgrad":          (dict(ew_grad=True), None, "tile", EDGE_GRAD_REASON),
    "gcn-ewgrad-fused":    (dict(ew_grad=True, impl="fused"), RAISE, None,
                            "impl='fused' requested but not applicable: " + EDGE_GRAD_REASON),
    "gcn-bn-nostats":      (dict(bn="no_stats"), None, "tile", "BatchNorm without affine/running stats/momentum"),
    "gcn-bn-subclass":     (dict(bn="subclass"), "tile", "tile", None),
    "gcn-bn-subclass-h128": (dict(bn="subclass", hid=128), None, "tile", "hidden_dim != 64"),
    "gcn-syncbn":          (dict(bn="sync"), "tile", "tile", None),
    "sage-h64":            (dict(kind="sage"), "sage", None, None),
    "sage-h128":           (dict(kind="sage", hid=128), "sage", None, None),
    "sage-h256":           (dict(kind="sage", hid=256), "sage", None, None),
    "sage-h192":           (dict(kind="sage", hid=192), None, None, "hidden_dim is not 64, 128, 256, ..."),
    "sage-h512":           (dict(kind="sage", hid=512), "sage", None, None),
    "sage-h100":           (dict(kind="sage", hid=100), None, None, "hidden_dim is not 64, 128, 256, ..."),
    "sage-h128-385":       (dict(kind="sage", hid=128, sizes=BIG), "sage", None, None),
    "sage-h512-385":       (dict(kind="sage", hid=512, sizes=BIG), None, None, OFF_TILES),
    "sage-h512-385-fused": (dict(kind="sage", hid=512, sizes=BIG, impl="fused"), RAISE, None,
                            "impl='fused' requested but not applicable: " + OFF_TILES),
    "sage-h512-385-nocsr": (dict(kind="sage", hid=512, sizes=BIG, csr=False), None, None,
                            "graphs do not fit an LDS tile and the structure has no CSR form"),
    "sage-h64-nocsr":      (dict(kind="sage", csr=False), "sage", None, None),
    "sage-layered":        (dict(kind="sage", impl="layered"), None, None, None),
    "sage-xgrad":          (dict(kind="sage", x_grad=True), None, None, "node_features require grad"),
    "sage-ewgrad":         (dict(kind="sage", ew_grad=True), None, None, EDGE_GRAD_REASON),
    "sage-bn-subclass":    (dict(kind="sage", bn="subclass"), None, None,
                            "BatchNorm is not a plain affine BatchNorm1d / SyncBatchNorm with running stats"),
}


def _snapshot(obj, skip=()):
    """vars(obj): scalars by value, everything else by identity (containers one level down as well)."""
    out = {}
    for k, v in vars(obj).items():
        if k in skip:
            continue
        if isinstance(v, (bool, int, float, str, type(None))):
            out[k] = v
        elif isinstance(v, dict):
            out[k] = (id(v), {kk: id(vv) for kk, vv in v.items()})
        else:
            out[k] = id(v)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_decision_table_and_purity(name):
    kw, kind, record, reason = CASES[name]
    m, b, s = build(**kw)
    before = _snapshot(m), [(n, id(p)) for n, p in m.named_parameters()], _snapshot(s, skip=("_path_agreement",))
    if kind == RAISE:
        with pytest.raises(RuntimeError) as err:
            encoder_choice.choose(m, b, s)
        assert str(err.value) == reason
    else:
        got = encoder_choice.choose(m, b, s)
        assert got == (kind, reason, record)
        assert encoder_choice.agreed(m, b, s, got) is got          # no process group: the local answer stands
    after = _snapshot(m), [(n, id(p)) for n, p in m.named_parameters()], _snapshot(s, skip=("_path_agreement",))
    assert before == after
    assert not hasattr(m, "_fused_kind") and m.impl_used is None    # the records are encode's alone


def test_choice_does_not_depend_on_the_batch_seen_before():
    m, a, sa = build()
    _, b, sb = build(sizes=BIG)
    first = encoder_choice.choose(m, a, sa)
    assert first.kind == "tile" and encoder_choice.choose(m, b, sb).kind == "wide"
    assert encoder_choice.choose(m, a, sa) == first


def test_torch_grad_mode_is_part_of_the_edge_gradient_row():
    m, b, s = build(ew_grad=True)
    with torch.no_grad():
        assert encoder_choice.choose(m, b, s).kind == "tile"


@pytest.mark.parametrize("local, other, want", [
    ("tile", 2, ("tile", None, "tile")),
    ("tile", 1, ("wide", None, "wide")),                   # another rank runs the wide encoder: so does this one
    ("tile", 0, (None, "another rank's shard is not covered", "tile")),
    ("wide", 2, ("wide", None, "wide")),
    ("wide", 0, (None, "another rank's shard is not covered", "wide")),
    (None, 2, (None, "hidden_dim != 64", "tile")),
    ("sage", 2, ("sage", None, None)),
    ("sage", 0, (None, "another rank's shard is not covered", None)),
])
def test_cross_rank_agreement_is_a_step_on_the_answer(monkeypatch, local, other, want):
    """SyncBatchNorm in training on two ranks: one all-reduce(MIN) of the wire code (0 layered, 1 wide, 2 tile or
    GraphSAGE) per (model, structure), cached on the structure; the step returns the agreed choice."""
    from connectome_gnn_amd import dist as cdist
    kw = {"tile": dict(), "wide": dict(hid=128), None: dict(hid=32), "sage": dict(kind="sage")}[local]
    m, b, s = build(bn="sync", **kw)
    m.train()
    sent = []
    monkeypatch.setattr(encoder_choice.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(encoder_choice.dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(cdist, "agree_min", lambda code, dev: sent.append(code) or min(code, other))
    choice = encoder_choice.choose(m, b, s)
    assert choice.kind == local
    before = _snapshot(m)
    assert encoder_choice.agreed(m, b, s, choice) == want
    assert encoder_choice.agreed(m, b, s, choice) == want
    assert sent == [{"tile": 2, "sage": 2, "wide": 1, None: 0}[local]] and len(s._path_agreement) == 1
    assert _snapshot(m) == before
    m.eval()
    assert encoder_choice.agreed(m, b, s, choice) is choice         # running statistics: nothing to agree on


# name: (model kwargs for build(), nodes per graph of the dataset, expected answer)
CACHE_CASES = {
    "gcn-h64":          (dict(), 84, True),
    "gcn-h64-f16":      (dict(fin=16), 84, True),
    "gcn-h64-f17":      (dict(fin=17), 84, False),
    "gcn-h128":         (dict(hid=128), 84, False),
    "gcn-h32":          (dict(hid=32), 84, False),
    "gcn-h64-fused":    (dict(impl="fused"), 84, True),
    "gcn-h64-layered":  (dict(impl="layered"), 84, False),
    "gcn-h64-fp16":     (dict(storage="fp16"), 84, False),
    "gcn-h64-syncbn":   (dict(bn="sync"), 84, False),
    "gcn-h64-bn-sub":   (dict(bn="subclass"), 84, False),
    "gcn-h64-nostats":  (dict(bn="no_stats"), 84, False),
    "gcn-h64-n384":     (dict(), 384, True),
    "gcn-h64-n385":     (dict(), 385, False),
    "gcn-h64-n0":       (dict(), 0, False),
    "sage-h64":         (dict(kind="sage"), 84, True),
    "sage-h128":        (dict(kind="sage", hid=128), 84, True),
    "sage-h256":        (dict(kind="sage", hid=256), 84, True),
    "sage-h192":        (dict(kind="sage", hid=192), 84, False),
    "sage-h512":        (dict(kind="sage", hid=512), 84, False),
    "sage-h100":        (dict(kind="sage", hid=100), 84, False),
    "sage-h64-layered": (dict(kind="sage", impl="layered"), 84, False),
    "sage-h64-syncbn":  (dict(kind="sage", bn="sync"), 84, False),
    "sage-h64-n385":    (dict(kind="sage"), 385, False),
}


@pytest.mark.parametrize("name", list(CACHE_CASES))
def test_subject_cache_serves(name):
    kw, n, want = CACHE_CASES[name]
    tr = C.Trainer.__new__(C.Trainer)
    tr.model = build(**kw)[0]
    ds = types.SimpleNamespace(x=torch.zeros(2, n, 4))
    assert tr._subject_cache_serves(ds, 2) is want
