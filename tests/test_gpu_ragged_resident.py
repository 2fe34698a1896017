"""Same-atlas datasets with per-subject edge counts served from the device: the ragged on-device collate
(cgnn_collate_edges, csrc/collate.hip) against ``collate_graphs``, its C-ABI refusals, and the loader, subject
cache and Trainer paths over a ``RaggedPackedDataset``."""
import functools

import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib
from connectome_gnn_amd.graph import shard_slice
from connectome_gnn_amd.resident import ResidentDataLoader, assemble_batch
from connectome_gnn_amd.synthetic import RaggedPackedDataset, pack_graphs
from tests import ragged_data as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("node_features", "edge_index", "edge_weight", "batch", "labels", "ptr")


@functools.lru_cache(maxsize=None)
def _device_set(S, n, k):
    graphs = R.ragged_graphs(S, n, k)
    ds = pack_graphs(list(graphs))
    assert type(ds) is RaggedPackedDataset
    return graphs, ds.to(DEV)


def _check_collate(ds, graphs, ids, on_device=False):
    """assemble_batch(ds, ids) == collate_graphs of the same subjects, all six public fields and the host eptr."""
    ids_t = torch.tensor(ids, dtype=torch.long)
    got = assemble_batch(ds, ids_t.to(DEV) if on_device else ids_t)
    want = C.collate_graphs([graphs[i] for i in ids])
    ref = want.to(DEV)
    for name in FIELDS:
        a, b = getattr(got, name), getattr(ref, name)
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, a.shape, b.shape)
        assert a.device.type == "cuda" and torch.equal(a, b), name
    assert got._eptr.device.type == "cpu" and got._eptr.dtype == torch.long
    assert torch.equal(got._eptr, R.host_eptr(graphs, ids)) and torch.equal(got._eptr, want._eptr)
    assert got._eptr_dev.dtype == torch.int32 and torch.equal(got._eptr_dev.cpu().long(), got._eptr)
    return got


def _id_cases(S):
    g = torch.Generator().manual_seed(11)
    shuffled = torch.randperm(S, generator=g).tolist()
    repeats = torch.randint(0, S, (2 * S + 1,), generator=g).tolist() + [S - 1, S - 1, R.EMPTY, R.EMPTY, 0]
    return {"shuffled": shuffled, "repeats": repeats, "one": [S // 2], "one_whole": [S - 1], "empty_only": [R.EMPTY],
            "empty_twice_then_one": [R.EMPTY, R.EMPTY, 0], "full": list(range(S))}


@pytest.mark.parametrize("S,n,k", R.SHAPES)
def test_ragged_collate_is_bit_identical_to_collate_graphs(S, n, k):
    graphs, ds = _device_set(S, n, k)
    for name, ids in _id_cases(S).items():
        b = _check_collate(ds, graphs, ids)
        assert b.num_graphs == len(ids) and b.num_nodes == len(ids) * n, name
    # ids that exist on the device only (one read-back of the ids, same result)
    _check_collate(ds, graphs, _id_cases(S)["shuffled"], on_device=True)
    # the batch builds its structure per graph in LDS from the offsets the kernel left on the device
    b = _check_collate(ds, graphs, _id_cases(S)["repeats"])
    s = b.structure()
    twin = C.collate_graphs([graphs[i] for i in _id_cases(S)["repeats"]]).to(DEV).structure()
    assert s.block_diagonal and torch.equal(s.rowptr_dst, twin.rowptr_dst) and torch.equal(s.eid_dst, twin.eid_dst)
    assert torch.equal(s.rowptr_src, twin.rowptr_src) and torch.equal(s.eid_src, twin.eid_src)
    with pytest.raises(IndexError):
        assemble_batch(ds, torch.tensor([0, S]))


def _hand_graph(num_edges, salt, n=20):
    """A labelled graph on n nodes with exactly `num_edges` directed edges (duplicates allowed) and weights
    that identify (graph, edge)."""
    j = torch.arange(num_edges, dtype=torch.long)
    ei = torch.stack([(j * 3 + salt) % n, (j * 7 + 3 * salt + 1) % n])
    w = (j.to(torch.float32) + 1.0) / 4096.0 + float(salt)
    x = torch.arange(n * 5, dtype=torch.float32).view(n, 5) + salt
    return C.ConnectomeGraph(x, ei, w, torch.tensor(salt % 2, dtype=torch.long), f"hand-{salt}")


@functools.lru_cache(maxsize=None)
def _hand_set():
    """Run lengths 0, 1 and c-1, c, c+1 for both widths the kernel works in -- the edges a thread moves with
    16-byte accesses and the edges of a chunk -- in two orders, so that the runs meet every alignment."""
    widths = (_lib.COLLATE_VEC, _lib.COLLATE_CHUNK)
    assert widths == (4, 1024)
    lens = [0, 1] + [c + d for c in widths for d in (-1, 0, 1)]
    lens = lens + [2] + lens[::-1] + [0, 0, 7]
    graphs = tuple(_hand_graph(m, i) for i, m in enumerate(lens))
    return graphs, pack_graphs(list(graphs)).to(DEV)


def test_ragged_collate_run_lengths_around_every_width():
    graphs, ds = _hand_set()
    S = len(graphs)
    _check_collate(ds, graphs, list(range(S)))
    _check_collate(ds, graphs, list(range(S))[::-1])
    g = torch.Generator().manual_seed(5)
    _check_collate(ds, graphs, torch.randint(0, S, (3 * S,), generator=g).tolist())
    for i in range(S):                       # every run alone: source offset arbitrary, destination offset 0
        _check_collate(ds, graphs, [i])
        _check_collate(ds, graphs, [1, i])   # ... and behind a one-edge run: destination offset 1


def test_ragged_collate_one_subject_ten_times_the_rest():
    lens = [30, 37, 12001, 25, 31, 0, 28]
    assert max(lens) >= 10 * sorted(lens)[-2]
    graphs = tuple(_hand_graph(m, i) for i, m in enumerate(lens))
    ds = pack_graphs(list(graphs)).to(DEV)
    _check_collate(ds, graphs, list(range(len(lens))))
    _check_collate(ds, graphs, [2, 0, 2, 5, 2, 1])


@pytest.mark.parametrize("b", [_lib.COLLATE_LDS_GRAPHS, _lib.COLLATE_LDS_GRAPHS + 1])
def test_ragged_collate_batch_sizes_around_the_lds_search_limit(b):
    """Up to COLLATE_LDS_GRAPHS graphs the batch's edge offsets are searched in LDS, beyond in global memory."""
    graphs, ds = _device_set(*R.SHAPES[0])
    g = torch.Generator().manual_seed(b)
    _check_collate(ds, graphs, torch.randint(0, len(graphs), (b,), generator=g).tolist())


def test_ragged_collate_on_a_small_grid():
    """The copy walks its chunks with a grid stride: with the persistent grid shrunk to 3 (x 4 workgroups) the
    360-node set and a 4097-graph batch put several chunks on every workgroup."""
    lib = _lib.load()
    big, big_ds = _device_set(*R.SHAPES[2])
    small, small_ds = _device_set(*R.SHAPES[0])
    g = torch.Generator().manual_seed(2)
    many = torch.randint(0, len(small), (_lib.COLLATE_LDS_GRAPHS + 1,), generator=g).tolist()
    assert lib.cgnn_set_fused_grid(3) == 0
    try:
        for ids in _id_cases(len(big)).values():
            _check_collate(big_ds, big, ids)
        _check_collate(small_ds, small, many)
        _check_collate(small_ds, small, many[:1000])
    finally:
        assert lib.cgnn_set_fused_grid(0) == 0


def test_collate_edges_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    graphs, ds = _device_set(*R.SHAPES[1])
    S, n = len(graphs), 84
    ids_h = [3, 0, R.EMPTY, 7, 3]
    ids = torch.tensor(ids_h, device=DEV)
    b = len(ids_h)
    ne = sum(graphs[i].num_edges for i in ids_h)
    ei = torch.full((2, ne), -7, dtype=torch.long, device=DEV)
    ew = torch.full((ne,), -7.0, dtype=torch.float32, device=DEV)
    ep = torch.full((b + 1,), -7, dtype=torch.int32, device=DEV)
    sp = _lib.stream_ptr()
    good = [_lib.ptr(ds.edge_local), _lib.ptr(ds.edge_weight), _lib.ptr(ds.edge_ptr_dev), S, int(ds.edge_weight.numel()),
            _lib.ptr(ids), b, n, ne, _lib.ptr(ei), _lib.nbytes(ei), _lib.ptr(ew), _lib.nbytes(ew), _lib.ptr(ep),
            _lib.nbytes(ep), sp]
    bad = {}
    for name, pos in (("edge_index", 10), ("edge_weight", 12), ("eptr", 14)):          # each written buffer one byte short
        bad[f"{name} one byte short"] = good[:pos] + [good[pos] - 1] + good[pos + 1:]
    for name, pos in (("edge_local", 0), ("edge_weight_ds", 1), ("edge_ptr", 2), ("ids", 5), ("edge_index", 9),
                      ("edge_weight", 11), ("eptr", 13)):                               # each required pointer NULL
        bad[f"{name} NULL"] = good[:pos] + [None] + good[pos + 1:]
    bad["n = 0"] = good[:7] + [0] + good[8:]
    bad["n < 0"] = good[:7] + [-1] + good[8:]
    bad["b < 0"] = good[:6] + [-1] + good[7:]
    bad["num_edges < 0"] = good[:8] + [-1] + good[9:]
    bad["num_edges >= 2^31"] = good[:8] + [2 ** 31] + good[9:]
    for name, args in bad.items():
        assert lib.cgnn_collate_edges(*args) == _lib.CGNN_EINVAL, name
    torch.cuda.synchronize()
    assert bool((ei == -7).all()) and bool((ew == -7.0).all()) and bool((ep == -7).all())
    # nothing to do: CGNN_OK without a launch, whatever the pointers
    assert lib.cgnn_collate_edges(*(good[:6] + [0] + good[7:])) == _lib.CGNN_OK
    assert lib.cgnn_collate_edges(*([None] * 3 + [S, 0, None, b, n, 0] + [None, 0] * 3 + [sp])) == _lib.CGNN_OK
    torch.cuda.synchronize()
    assert bool((ei == -7).all()) and bool((ew == -7.0).all()) and bool((ep == -7).all())
    # the full-size call
    assert lib.cgnn_collate_edges(*good) == _lib.CGNN_OK
    ref = C.collate_graphs([graphs[i] for i in ids_h])
    assert torch.equal(ei.cpu(), ref.edge_index) and torch.equal(ew.cpu(), ref.edge_weight)
    assert torch.equal(ep.cpu().long(), ref._eptr)


def _train_steps(make_model, batches, pick):
    torch.manual_seed(0)
    m = make_model().to(DEV).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    logits = []
    for rb in batches:
        b = pick(rb)
        opt.zero_grad()
        lg = m(b)
        assert m.impl_used == "fused"
        torch.nn.functional.cross_entropy(lg, b.labels).backward()
        opt.step()
        logits.append(lg.detach().clone())
    return logits, [p.detach().clone() for p in m.parameters()]


@pytest.mark.parametrize("kind,shape", [("gcn", R.SHAPES[2]), ("sage", R.SHAPES[1])])
def test_subject_structure_cache_equals_per_batch_build_ragged(kind, shape):
    """The recipe of test_subject_structure_cache_equals_per_batch_build on ragged data: batch 3, hidden 64,
    dropout 0.3, three optimiser steps; logits and final parameters bit-identical between ResidentBatch (per-subject
    cache) and assemble_batch + the per-batch builders."""
    from connectome_gnn_amd.structure_cache import ResidentBatch
    graphs, ds = _device_set(*shape)
    torch.manual_seed(3)
    ld = ResidentDataLoader(ds, batch_size=3, shuffle=True, structure_cache=True)
    batches = (list(ld) + list(ld))[:3]
    assert len(batches) == 3 and all(isinstance(b, ResidentBatch) and b.num_graphs == 3 for b in batches)
    cls = C.GCNConnectome if kind == "gcn" else C.GraphSAGEConnectome
    cached = _train_steps(lambda: cls(5, 64, dropout=0.3), batches, lambda rb: rb)
    built = _train_steps(lambda: cls(5, 64, dropout=0.3), batches, lambda rb: assemble_batch(ds, rb._ids))
    for a, c in zip(cached[0], built[0]):
        assert torch.isfinite(a).all() and torch.equal(a, c)
    for a, c in zip(cached[1], built[1]):
        assert torch.equal(a, c)
    # the lazily assembled COO is the ragged collate's
    for rb in batches:
        ref = assemble_batch(ds, rb._ids)
        assert rb._coo is None
        assert torch.equal(rb.edge_index, ref.edge_index) and torch.equal(rb.edge_weight, ref.edge_weight)
        assert torch.equal(rb.batch, ref.batch)
        want = C.collate_graphs([graphs[i] for i in rb._ids.tolist()])
        assert torch.equal(rb.edge_index.cpu(), want.edge_index) and torch.equal(rb.node_features.cpu(), want.node_features)
        assert torch.equal(rb.labels.cpu(), want.labels)


@functools.lru_cache(maxsize=None)
def _script_graphs():
    graphs = R.thresholded(C.generate_dataset(72, 84, 8, seed=5))
    assert len({g.num_edges for g in graphs}) > 8 and any(g.num_edges % 2 for g in graphs)
    return graphs


@pytest.mark.parametrize("kind,hidden", [("gcn", 64), ("sage", 64), ("gcn", 32), ("gcn", 128)])
def test_the_unchanged_reference_script_is_served_from_the_device_on_ragged_data(kind, hidden):
    """The recipe of test_the_unchanged_reference_script_is_served_from_the_device on 72 thresholded 84-node
    graphs: the default Trainer packs both loaders into HBM (RaggedPackedDataset), follows the host loader's
    trajectory and RNG consumption, replays captured steps for the two hidden-64 encoders and serves the others
    eagerly through the ragged collate."""
    graphs = _script_graphs()
    hist, rng_after, evals, trainers = {}, {}, {}, {}
    for mode in ("host", "default"):
        torch.manual_seed(3)
        cls = C.GCNConnectome if kind == "gcn" else C.GraphSAGEConnectome
        m = cls(5, hidden, dropout=0.0)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4)
        tr = C.Trainer(m, opt, device=DEV, **({"resident": False, "graph": False} if mode == "host" else {}))
        ld = C.ConnectomeDataLoader(graphs[:56], batch_size=16, shuffle=True)        # 3 x 16 + 8: two batch sizes
        vl = C.ConnectomeDataLoader(graphs[56:], batch_size=16, shuffle=False)
        hist[mode] = tr.fit(ld, vl, num_epochs=4, patience=10, verbose=False)
        evals[mode] = tr.evaluate(vl)
        rng_after[mode] = torch.get_rng_state()
        trainers[mode] = tr
    for key in ("train_loss", "val_loss", "val_acc"):
        print(kind, hidden, key, hist["default"][key], hist["host"][key])
        torch.testing.assert_close(torch.tensor(hist["default"][key]), torch.tensor(hist["host"][key]),
                                   rtol=2e-4, atol=2e-6, msg=lambda s: f"{key}: {s}")
    assert evals["default"]["total"] == evals["host"]["total"] == 16
    assert evals["default"]["correct"] == evals["host"]["correct"]
    assert abs(evals["default"]["loss"] - evals["host"]["loss"]) <= 2e-4 * abs(evals["host"]["loss"]) + 2e-6
    assert torch.equal(rng_after["default"], rng_after["host"])      # the same randperm calls, nothing else drawn
    tr = trainers["default"]
    assert len(tr._resident) == 2 and all(v[2] is not None for v in tr._resident.values())
    assert all(type(v[2].dataset) is RaggedPackedDataset for v in tr._resident.values())
    served = hidden == 64
    assert tr.graph is served
    if served:
        assert sorted(k[2] for k in tr._graphs if k[0] == "resident") == [8, 16]     # one captured step per batch size
        assert all(g["capturable"] for g in tr.optimizer.param_groups)
    else:
        assert not tr._graphs                                        # eager, batches from the ragged collate
        assert all(v[2].structure_cache is None for v in tr._resident.values())
    assert not trainers["host"]._graphs and not trainers["host"]._resident


def test_ragged_loader_prefetch_and_cached_batches():
    graphs, ds = _device_set(*R.SHAPES[1])
    # prefetch on the side stream: the same batches as without it
    for cache in (False, True):
        got = {}
        for prefetch in (False, True):
            torch.manual_seed(3)
            ld = ResidentDataLoader(ds, batch_size=5, shuffle=True, prefetch=prefetch, structure_cache=cache)
            got[prefetch] = [(b._ids.clone() if cache else b.labels.clone(), b.node_features.clone(),
                              b.edge_index.clone(), b.edge_weight.clone()) for b in ld]
        torch.cuda.synchronize()
        assert len(got[False]) == len(got[True]) == 3
        for plain, pre in zip(got[False], got[True]):
            for a, c in zip(plain, pre):
                assert torch.equal(a, c)
    # ... and they are collate_graphs' (the permutation is the global generator's)
    torch.manual_seed(3)
    order = torch.randperm(len(graphs)).tolist()
    want = C.collate_graphs([graphs[i] for i in order[:5]])
    assert torch.equal(got[False][0][2].cpu(), want.edge_index) and torch.equal(got[False][0][1].cpu(), want.node_features)
    # rank / world size: this rank's contiguous shard of every global batch
    torch.manual_seed(3)
    shard = list(ResidentDataLoader(ds, batch_size=5, shuffle=True, rank=1, world_size=2))
    want = C.collate_graphs([graphs[i] for i in shard_slice(order[:5], 1, 2)])
    assert torch.equal(shard[0].edge_index.cpu(), want.edge_index) and torch.equal(shard[0].labels.cpu(), want.labels)
    # cached batches, order re-drawn per epoch: the same objects come round again
    torch.manual_seed(4)
    ld = ResidentDataLoader(ds, batch_size=5, shuffle="batches", cache_batches=True)
    first, second = list(ld), list(ld)
    assert len(first) == 3 and {id(b) for b in first} == {id(b) for b in second}
    assert sorted(b.num_graphs for b in first) == [2, 5, 5]
    ids = ld._fixed_order.tolist()
    for j, b in enumerate(ld._cache):
        want = C.collate_graphs([graphs[i] for i in ids[5 * j:5 * j + 5]])
        assert torch.equal(b.edge_index.cpu(), want.edge_index) and torch.equal(b._eptr, want._eptr)
