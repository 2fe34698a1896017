"""CPU tests: drop-in data API (mirrors the reference's tests/test_graph.py and
tests/test_synthetic.py assertions), the C-ABI symbol table, and the no-fallback rule."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib
from connectome_gnn_amd.graph import shard_slice
from connectome_gnn_amd.synthetic import NUM_REGIONS, generate_packed, small_world_stats
from tests import abi_header
from tests import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _simple_graph(n=10, e=20, f=4, label=0, seed=0):
    g = torch.Generator().manual_seed(seed)
    s, d = torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)
    w = torch.rand(e, generator=g)
    return C.ConnectomeGraph(torch.randn(n, f, generator=g), torch.stack([torch.cat([s, d]), torch.cat([d, s])]),
                             torch.cat([w, w]), torch.tensor(label))


# ------------------------------------------------------------------------------- C ABI
def test_public_names_match_reference():
    assert C.__all__ == ["ConnectomeGraph", "ConnectomeBatch", "ConnectomeDataLoader",
                         "collate_graphs", "generate_connectome", "generate_dataset",
                         "REGION_NAMES", "GCNConnectome", "GraphSAGEConnectome", "Trainer"]


def test_library_exports_every_declared_symbol():
    """Every function declared in include/cgnn.h is exported by libcgnn_hip.so and bound in
    _lib.PROTOTYPES (no compute calls: this box has no GPU)."""
    hdr = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cgnn_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 30
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in cgnn.h but not exported"
    assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
    loaded = _lib.load()
    assert loaded.cgnn_abi_version() == _lib.ABI_VERSION
    assert loaded.cgnn_build_target() == b"gfx950"
    assert loaded.cgnn_csr_workspace_bytes(1000, 5000) > 0
    assert loaded.cgnn_csr_workspace_bytes(-1, 0) < 0          # CGNN_EINVAL, no crash


def _abi_mismatches(header: str) -> set:
    """Names whose declaration in ``header`` and whose row of _lib.PROTOTYPES differ in the return type or in any
    argument type (or that only one of the two has)."""
    declared = abi_header.declared(header)
    bad = set(declared) ^ set(_lib.PROTOTYPES)
    for name in set(declared) & set(_lib.PROTOTYPES):
        res, args = _lib.PROTOTYPES[name]
        if declared[name] != (res, list(args)):
            bad.add(name)
    return bad


def test_prototypes_match_the_header_type_by_type():
    """Return type and every argument type of all 127 rows of _lib.PROTOTYPES against include/cgnn.h -- and the
    comparison itself against a doctored header (one widened integer, one dropped parameter), so that a parser
    that matches nothing cannot pass."""
    hdr = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    assert len(_lib.PROTOTYPES) == 127
    assert _abi_mismatches(hdr) == set()
    one = "int cgnn_rng_advance(uint32_t* state, int32_t n, void* stream);"
    two = "int cgnn_bn_reduce(const double* slab, int32_t rows, int32_t width, double* sums, void* stream);"
    assert one in hdr and two in hdr
    doctored = hdr.replace(one, one.replace("int32_t n", "int64_t n")).replace(two, two.replace("int32_t width, ", ""))
    assert _abi_mismatches(doctored) == {"cgnn_rng_advance", "cgnn_bn_reduce"}


def test_the_registry_is_cgnn_h_and_the_headers_it_includes():
    """_lib.HEADERS, which load() binds from: cgnn.h first, then every include/cgnn_*.h that cgnn.h includes, in its
    order, and nothing else -- a family whose header is included but has no entry would load without argtypes.  Every
    such header is a file, and no header under include/ is left out of cgnn.h."""
    included = re.findall(r'^#include "(cgnn_\w+\.h)"', abi_header.read("cgnn.h"), flags=re.M)
    assert len(included) >= 11 and len(set(included)) == len(included)
    assert list(_lib.HEADERS) == ["cgnn.h"] + included
    assert _lib.HEADERS["cgnn.h"] is _lib.PROTOTYPES
    assert sorted(os.listdir(abi_header.INCLUDE)) == sorted(_lib.HEADERS)
    with pytest.raises(_lib.CgnnError, match="cgnn_ingest_knn is in the tables of both cgnn_knn.h and cgnn_twice.h"):
        _lib.check_disjoint({**_lib.HEADERS, "cgnn_twice.h": {"cgnn_ingest_knn": (ctypes.c_int, [])}})


def test_devptr_through_a_foreign_call():
    """DevPtr as an argtype of libc's memcmp: tensors, their addresses as ints and None (NULL) are taken, in any
    mix, with the same answer; a float or a str is refused with the argument's position."""
    memcmp = ctypes.CDLL(None).memcmp
    memcmp.restype, memcmp.argtypes = ctypes.c_int, [_lib.DevPtr, _lib.DevPtr, ctypes.c_size_t]
    a = torch.arange(1000, dtype=torch.int64)
    same, other = a.clone(), a.clone()
    other[999] += 1
    n = _lib.nbytes(a)
    for b, equal in ((same, True), (other, False)):
        answers = {memcmp(a, b, n) == 0, memcmp(a.data_ptr(), b, n) == 0, memcmp(a, b.data_ptr(), n) == 0,
                   memcmp(_lib.ptr(a), _lib.ptr(b), n) == 0}
        assert answers == {equal}
    assert memcmp(None, None, 0) == 0
    for bad in (1.5, "a"):
        with pytest.raises(ctypes.ArgumentError, match="argument 2"):
            memcmp(a, bad, n)


class _StubLib:
    """Stands in for the loaded library: every cgnn_* attribute is a callable that records its arguments and
    returns ``rc``."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def __getattr__(self, name):
        if not name.startswith("cgnn_"):
            raise AttributeError(name)
        return lambda *args: (self.calls.append((name, args)), self.rc)[1]


def test_call_appends_the_stream_checks_the_code_and_leaves_torch_cuda_alone(monkeypatch):
    """_lib.call against a stub library.  This machine has no GPU: with stream= given, a call that touched torch.cuda
    (device guard, stream lookup, events) would raise -- with no timer installed, and with one that does not name
    the key."""
    t = torch.zeros(4)
    for timer in (None, _lib.KernelTimer(["cgnn_other", "cgnn_x[F=8]"])):
        stub = _StubLib()
        monkeypatch.setattr(_lib, "_lib", stub)
        monkeypatch.setattr(_lib, "TIMER", timer)
        assert _lib.call("cgnn_x", t, 3, *_lib.buf(t), stream=0x1234) == _lib.CGNN_OK
        assert _lib.call("cgnn_x", None, stream=0x5678, key="cgnn_x[F=64]") == _lib.CGNN_OK
        assert stub.calls == [("cgnn_x", (t, 3, t, 16, 0x1234)), ("cgnn_x", (None, 0x5678))]
        stub.rc = _lib.CGNN_EUNSUPPORTED
        assert _lib.call("cgnn_x", stream=1, accept=(_lib.CGNN_EUNSUPPORTED,)) == _lib.CGNN_EUNSUPPORTED
        with pytest.raises(_lib.CgnnError, match=r"cgnn_x failed: CGNN_EUNSUPPORTED"):
            _lib.call("cgnn_x", stream=1)
        stub.rc = _lib.CGNN_EINVAL
        with pytest.raises(_lib.CgnnError, match=r"cgnn_y failed: CGNN_EINVAL"):
            _lib.call("cgnn_y", stream=1, accept=(_lib.CGNN_EUNSUPPORTED,))
        assert [c[1][-1] for c in stub.calls[2:]] == [1, 1, 1]
    assert _lib.buf(None) == (None, 0)


def test_tiles_struct_layout_matches_header():
    t = _lib.CgnnTiles()
    assert ctypes.sizeof(t) == 8 + 4 + 4 + 7 * 8
    assert [f[0] for f in t._fields_] == ["num_nodes", "num_tiles", "max_tile_rows", "tile_ptr",
                                          "tile_blk", "blk_off_dst", "ent_dst", "blk_off_src",
                                          "ent_src", "dis"]


def test_no_cpu_fallback_and_no_oracle_import_in_product():
    """The product path must raise on CPU tensors and must never import oracle/."""
    b = C.collate_graphs(C.generate_dataset(2, 20, 4))
    for cls in (C.GCNConnectome, C.GraphSAGEConnectome):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls(5, 16)(b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        b.structure()
    pkg = os.path.join(ROOT, "connectome_gnn_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "import oracle" not in src and "from oracle" not in src, fn


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libcgnn_hip.so")
    with pytest.raises(_lib.CgnnError, match="no CPU/eager fallback"):
        _lib.load()


# ------------------------------------------------------------------- containers / collate
def test_graph_properties_and_helpers():
    g = _simple_graph()
    assert (g.num_nodes, g.num_edges, g.num_features) == (10, 40, 4)
    a = g.adjacency_matrix()
    assert a.shape == (10, 10) and torch.allclose(a, a.t())
    assert (g.degree() >= 0).all()
    assert g.to("cpu").subject_id == g.subject_id


def test_collate_shapes_offsets_ptr():
    g1, g2 = _simple_graph(10, 20, label=0), _simple_graph(7, 9, label=1, seed=1)
    b = C.collate_graphs([g1, g2])
    assert b.num_graphs == 2 and b.num_nodes == 17
    assert b.edge_index.shape == (2, 58) and b.edge_index.dtype == torch.int64
    assert b.batch.tolist() == [0] * 10 + [1] * 7
    assert b.ptr.tolist() == [0, 10, 17]
    assert int(b.edge_index[:, 40:].min()) >= 10          # second graph offset by N1
    assert b.labels.tolist() == [0, 1]
    unl = C.collate_graphs([C.ConnectomeGraph(g1.node_features, g1.edge_index, g1.edge_weight)])
    assert unl.labels is None


def test_collate_bit_exact_vs_golden_g1():
    d = G.load("g1_collate_8x20.npz")
    bd = G.group(d, "batch")
    gs = [C.ConnectomeGraph(*g) for g in G.split_graphs(bd, d["edge_counts"])]
    b = C.collate_graphs(gs)
    for f in ("node_features", "edge_index", "edge_weight", "batch", "labels", "ptr"):
        assert torch.equal(getattr(b, f), bd[f]), f


def test_loader_len_partial_batch_and_shuffle_rng():
    ds = [_simple_graph(seed=i) for i in range(10)]
    ld = C.ConnectomeDataLoader(ds, batch_size=4, shuffle=False)
    assert len(ld) == math.ceil(10 / 4)
    sizes = [b.num_graphs for b in ld]
    assert sizes == [4, 4, 2]
    torch.manual_seed(3)
    want = torch.randperm(10).tolist()
    torch.manual_seed(3)
    first = next(iter(C.ConnectomeDataLoader(ds, batch_size=10, shuffle=True)))
    assert torch.equal(first.node_features[:10], ds[want[0]].node_features)


def test_shard_slice_partitions():
    for n in (0, 1, 7, 8, 4096):
        for w in (1, 2, 3, 8):
            parts = [shard_slice(list(range(n)), r, w) for r in range(w)]
            assert sum(parts, []) == list(range(n))
            assert max(map(len, parts)) - min(map(len, parts)) <= 1


def test_sharded_loader_covers_global_batch():
    ds = [_simple_graph(seed=i) for i in range(9)]
    full = [b for b in C.ConnectomeDataLoader(ds, batch_size=4, shuffle=False)]
    parts = [[b for b in C.ConnectomeDataLoader(ds, batch_size=4, shuffle=False, rank=r, world_size=2)]
             for r in range(2)]
    assert len(full) == 3 and len(parts[0]) == len(parts[1]) == 2   # 1-graph tail < world: dropped
    for i in range(2):
        cat = torch.cat([parts[0][i].node_features, parts[1][i].node_features])
        assert torch.equal(cat, full[i].node_features)


# ------------------------------------------------------------------------------ synthetic
def test_generator_contract():
    assert len(C.REGION_NAMES) == NUM_REGIONS == 83        # the reference's list has 83 entries
    g = C.generate_connectome(num_regions=84, seed=0)
    assert g.num_nodes == 84 and g.num_features == 5 and g.num_edges == 84 * 8
    assert (g.edge_weight > 0).all() and int(g.label) in (0, 1)
    assert int(g.edge_index.max()) < 84 and int(g.edge_index.min()) >= 0
    g2 = C.generate_connectome(num_regions=84, seed=0)
    assert torch.equal(g.edge_index, g2.edge_index) and torch.allclose(g.node_features, g2.node_features)
    assert not torch.equal(g.edge_index, C.generate_connectome(num_regions=84, seed=1).edge_index)
    s, d = g.edge_index
    assert torch.equal(s[0::2], d[1::2]) and torch.equal(d[0::2], s[1::2])       # both directions
    key = s * 84 + d
    assert key.unique().numel() == key.numel() and (s != d).all()               # simple graph
    ds = C.generate_dataset(100, num_regions=20, seed=42)
    pos = sum(int(x.label) for x in ds)
    assert len(ds) == 100 and 5 < pos < 95
    st = small_world_stats(ds[:5])
    assert set(st) == {"mean_clustering", "mean_avg_path_length", "num_graphs"} and 0 < st["mean_clustering"] < 1


def test_generator_matches_reference_distribution_g8():
    """G8 (one graph from the reference generator): same edge count, weight law and feature
    scales -- the streams differ by construction, the distributions must not."""
    d = G.load("g8_generate_seed42.npz")
    n = d["node_features"].shape[0]
    ours = C.generate_dataset(40, num_regions=n, k=8, seed=1)
    assert ours[0].num_edges == d["edge_index"].shape[1]
    w_ref = d["edge_weight"]
    w = torch.cat([g.edge_weight for g in ours]).numpy()
    assert abs(w.mean() - 2 / 7) < 0.01 and abs(float(w_ref.mean()) - 2 / 7) < 0.05      # Beta(2,5)
    x = torch.cat([g.node_features for g in ours]).numpy()
    assert np.allclose(x[:, 2].std(), 1.0, atol=0.05) and np.allclose(x[:, 4].std(), 1.0, atol=0.05)
    deg = np.bincount(ours[0].edge_index[1].numpy(), minlength=n)
    assert deg.sum() == n * 8 and deg.min() >= 2


def test_packed_dataset_equals_list_dataset():
    ds = generate_packed(6, 20, 4, seed=5)
    ls = C.generate_dataset(6, 20, 4, seed=5)
    for i in range(6):
        g = ds.graph(i)
        assert torch.equal(g.edge_index, ls[i].edge_index) and torch.equal(g.node_features, ls[i].node_features)
        assert torch.equal(g.edge_weight, ls[i].edge_weight) and int(g.label) == int(ls[i].label)


def test_resident_assemble_matches_collate_cpu():
    from connectome_gnn_amd.resident import ResidentDataLoader, assemble_batch
    ds = generate_packed(12, 20, 4, seed=5)
    ids = torch.tensor([7, 0, 3, 11])
    want = C.collate_graphs([ds.graph(int(i)) for i in ids])
    got = assemble_batch(ds, ids)
    for f in ("node_features", "edge_index", "edge_weight", "batch", "labels", "ptr"):
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    ld = ResidentDataLoader(ds, batch_size=5, shuffle=False)
    assert len(ld) == 3 and [b.num_graphs for b in ld] == [5, 5, 2]


# ------------------------------------------------------------------------- tiling (fused path)
def test_tile_partition_rules():
    from connectome_gnn_amd.structure import BatchStructure
    for sizes in ([360] * 10, [84] * 512, [20] * 1000, [20, 35, 84, 7, 360, 1, 2], [384, 383, 17]):
        s = BatchStructure()
        s._ptr_host = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        s.max_nodes_per_graph = max(sizes)
        s.num_nodes = int(sum(sizes))
        s.rowptr_dst = torch.zeros(1)
        tptr, rows = s.tile_ptr(384, 256)
        cuts = tptr.tolist()
        assert cuts[0] == 0 and cuts[-1] == s.num_nodes and rows <= 384
        assert all(b > a for a, b in zip(cuts, cuts[1:]))
        assert set(cuts) <= set(s._ptr_host.tolist())          # tiles are unions of whole graphs
        assert max(b - a for a, b in zip(cuts, cuts[1:])) == rows


def test_state_dict_keys_and_param_counts():
    """identical state_dict keys/shapes and parameter counts."""
    counts = {("gcn", 64): 11234, ("sage", 64): 19746, ("gcn", 128): 42946, ("sage", 128): 76354,
              ("gcn", 256): 167810, ("sage", 256): 300162}
    for (kind, h), want in counts.items():
        m = (C.GCNConnectome if kind == "gcn" else C.GraphSAGEConnectome)(5, h)
        assert sum(p.numel() for p in m.parameters()) == want
    d = G.load("g3_models_8x20_h32.npz")
    for kind, cls in (("gcn", C.GCNConnectome), ("sage", C.GraphSAGEConnectome)):
        torch.manual_seed(42)
        sd = cls(5, 32).state_dict()
        init = G.group(d, f"{kind}_init")
        assert list(sd.keys()) == list(init.keys())
        assert all(torch.equal(sd[k], init[k]) for k in init)      # same init stream (a7/a9)
        m = cls(5, 32)
        m.load_state_dict(init)                                     # reference checkpoint loads


def test_packed_dataset_from_graphs_round_trip():
    """PackedDataset.from_graphs: the reference-style list of graphs packed for the resident loader."""
    import pytest
    import torch
    import connectome_gnn_amd as C
    from connectome_gnn_amd.synthetic import PackedDataset
    gs = C.generate_dataset(5, 20, 4, seed=3)
    ds = PackedDataset.from_graphs(gs)
    assert ds.num_subjects == 5
    for i, g in enumerate(gs):
        h = ds.graph(i)
        assert torch.equal(h.node_features, g.node_features) and torch.equal(h.edge_index, g.edge_index)
        assert torch.equal(h.edge_weight, g.edge_weight) and int(h.label) == int(g.label)
    with pytest.raises(ValueError):
        PackedDataset.from_graphs(gs + C.generate_dataset(1, 21, 4, seed=1))


def test_bench_pmc_keys_resolve_in_committed_profiles():
    """bench.py's `roofline.traffic` comes from the PMC summaries under profiles/: every workload
    that has a committed summary must resolve to a kernel in it (r2: a template parameter added
    to k_gcn_bwd silently nulled the field), and a stale prefix raises instead of returning null."""
    import importlib.util
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("cgnn_bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    resolved = 0
    for wl, (files, bsz, prefixes) in bench.PMC_FILES.items():
        present = [f for f in files if os.path.exists(os.path.join(root, "profiles", f))]
        if not present:
            continue
        per_launch, per_step, src = bench.pmc_traffic(wl, bsz)
        assert per_launch and per_launch > 0 and per_step and per_step > per_launch, (wl, per_launch, per_step)
        assert present[0] in src
        doc = json.load(open(os.path.join(root, "profiles", present[0])))
        assert any(k.startswith(pf) for k in doc["kernels"] for pf in prefixes)
        assert bench.pmc_traffic(wl, bsz + 1) == (None, None, None)          # another batch: no claim
        resolved += 1
    assert resolved >= 4                                # headline, cfg2, cfg3, cfg5-fp16
    bench.PMC_FILES["_stale"] = (bench.PMC_FILES["cfg4-headline-gcn-4096x360-h64"][0], 4096, ("k_no_such_kernel<",))
    with pytest.raises(RuntimeError, match="stale"):
        bench.pmc_traffic("_stale", 4096)


def test_bench_extra_configs_name_known_workloads():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("cgnn_bench2", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    labels = [c[0] for c in bench.EXTRA_CONFIGS]
    for want in ("cfg2-gcn-512x84-h64", "cfg3-sage-512x360-h128", "cfg5-gcn-64x1000-h256-fp16",
                 "shard512-gcn-512x360-h64"):
        assert want in labels
    assert all(key in bench.WORKLOADS and launch in ("eager", "graph", "graph-dp", "auto", "trainer", "plain", "demo") for _, key, launch, _ in bench.EXTRA_CONFIGS)


def test_bench_dump_outputs_writes_float_arrays(tmp_path):
    """bench.py --dump-outputs: the loss plus every parameter, gradient and buffer the step left in the model,
    one DIR/<name>.npy each, float32 (float64 for the integer step counter), values unchanged."""
    import bench
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(5, 8), torch.nn.BatchNorm1d(8)).train()
    loss = m(torch.randn(16, 5)).square().mean()
    loss.backward()
    n = bench.dump_outputs(str(tmp_path / "out"), m, loss)
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "out"))
    assert n == len(names) == 12 and "loss" in names and "grad.0.weight" in names
    assert "buffer.1.running_var" in names and "buffer.1.num_batches_tracked" in names
    for f in names:
        a = np.load(tmp_path / "out" / f"{f}.npy")
        assert a.dtype == (np.float64 if f.endswith("num_batches_tracked") else np.float32), f
    np.testing.assert_array_equal(np.load(tmp_path / "out" / "grad.0.weight.npy"), m[0].weight.grad.numpy())
    assert float(np.load(tmp_path / "out" / "loss.npy")[0]) == float(loss.detach())


def test_bench_rank_bookkeeping_for_eight_gpus():
    """The 8-GPU run nobody can rehearse on hardware: bench.py's rank bookkeeping driven for
    --gpus 8 with no GPU work -- shard sizes, launch=auto -> HIP-graph replay at 512 graphs per rank, the config
    keys that name RCCL, the unequal-shard weights, and the projected figure kept out of `value`."""
    import bench
    sizes = []
    for r in range(8):
        p = bench.plan_run("strong", "auto", 4096, r, 8)
        assert p["shard_sizes"] == [512] * 8 and p["graphs_this_rank"] == 512 and p["global_batch"] == 4096
        assert p["equal_shards"] and p["local_graphs"] is None
        assert p["launch"] == "graph"                      # 512 graphs per rank are host-bound when launched eagerly
        sizes.append(p["graphs_this_rank"])
    assert sum(sizes) == 4096
    # 1, 2, 4 GPUs of the driver's scaling sweep: eager at >= 2048 graphs per rank, replay below
    assert [bench.plan_run("strong", "auto", 4096, 0, w)["launch"] for w in (1, 2, 4, 8)] == ["eager", "eager", "graph", "graph"]
    # a global batch that does not divide: contiguous runs differing by one graph, weights = local counts
    p = [bench.plan_run("strong", "auto", 4100, r, 8) for r in range(8)]
    assert [q["graphs_this_rank"] for q in p] == [513] * 4 + [512] * 4 and not p[0]["equal_shards"]
    assert [q["local_graphs"] for q in p] == [513] * 4 + [512] * 4
    w = bench.plan_run("weak", "auto", 4096, 3, 8)
    assert w["global_batch"] == 8 * 4096 and w["graphs_this_rank"] == 4096 and w["launch"] == "eager"
    with pytest.raises(SystemExit):
        bench.plan_run("strong", "auto", 4, 0, 8)
    cfg = bench.parallel_config(8, "nccl", "strong", False, True, "split", None)
    assert cfg["backend"] == "rccl" and cfg["rccl_ranks"] == 8 and cfg["bn"] == "per-rank"
    assert cfg["launch"] == "hip-graph replay (split all-reduce)" and cfg["parallelism"] == "graph-sharded dp8"
    cfg = bench.parallel_config(8, "gloo", "strong", True, False, "split", "graph capture failed on another rank; eager launches")
    assert cfg["rccl_ranks"] == 0 and cfg["launch"] == "eager" and cfg["bn"] == "sync" and "another rank" in cfg["launch_note"]
    pr = bench.projection_8gpu(1.86, 0.327)
    assert "value" not in pr and pr["what"].startswith("projection") and pr["n_gpus"] == 8
    assert 4.5 < pr["speedup_vs_1gpu"][1] < pr["speedup_vs_1gpu"][0] < 6.0


def test_bn_tail_struct_layout_matches_header():
    """struct cgnn_bn_tail (include/cgnn.h; the library static_asserts 120 bytes) and its ctypes mirror."""
    from connectome_gnn_amd import _lib
    t = _lib.CgnnBnTail()
    assert ctypes.sizeof(t) == 120 and _lib.BN_ACC_BYTES == 16448
    assert _lib.CgnnBnTail.count.offset == 8 and _lib.CgnnBnTail.gamma.offset == 24
    assert _lib.CgnnBnTail.momentum.offset == 56 and _lib.CgnnBnTail.rng_n.offset == 88 and _lib.CgnnBnTail.bwc.offset == 112
    hdr = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    assert "#define CGNN_BN_ACC_BYTES 16448" in hdr


def test_trainer_host_side_decisions_for_the_packed_path():
    """CPU-checkable pieces of Trainer's packed path (train.py): the optimizer switch, the prepare-callback
    signature probe, the claim / disarm protocol of direct gradient destinations."""
    import connectome_gnn_amd as C
    from connectome_gnn_amd import ops
    from connectome_gnn_amd.structure import call_prepare
    m = torch.nn.Linear(4, 2)
    tr = C.Trainer.__new__(C.Trainer)
    tr.optimizer = torch.optim.Adam(m.parameters(), lr=1e-3)
    assert tr._make_capturable() and all(g["capturable"] for g in tr.optimizer.param_groups)
    assert not any(g.get("fused") for g in tr.optimizer.param_groups)          # CPU parameters: no fused kernel
    tr.optimizer = torch.optim.SGD(m.parameters(), lr=1e-3)
    assert not tr._make_capturable()                                           # not an optimizer we know to switch
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    m(torch.randn(3, 4)).sum().backward()
    opt.step()
    tr.optimizer = opt
    assert not tr._make_capturable()                                           # state exists on the host already
    calls = []
    call_prepare(lambda b, reuse=False: calls.append(("kw", reuse)), 1)
    call_prepare(lambda b: calls.append(("plain",)), 1)

    def raises_inside(b, reuse=False):
        raise TypeError("from inside")
    with pytest.raises(TypeError, match="from inside"):
        call_prepare(raises_inside, 1)                                          # not swallowed, not retried
    assert calls == [("kw", True), ("plain",)]
    p = torch.nn.Parameter(torch.zeros(3))
    assert ops.grad_destination(p) is None                                      # never armed
    p._cgnn_direct = True
    p.grad = torch.zeros(3)
    assert ops.grad_destination(p) is None and p._cgnn_direct is False         # host tensors are never written to; disarmed


# ---- refusal codes of the tile entry points (csrc/fused_gcn.hip, fused_readout.hip, aggregate_tiled*.hip) ----
# One row = one call with one bad argument (a few with two, where the ORDER of the checks decides the code) and
# the status the library returns for it.  Every row returns before any launch and before any HIP runtime call:
# the pointers are made-up values that are only ever compared and masked, and the workgroup count behind the
# slab sizes is pinned with cgnn_set_fused_grid.
_A, _M = 0x1000, 0x1004          # 16-byte aligned / misaligned device-pointer values
_GRID = 4                        # pinned workgroup count: [grid][128] f64 slab = 4096 bytes
_INV, _UNS, _OK = _lib.CGNN_EINVAL, _lib.CGNN_EUNSUPPORTED, _lib.CGNN_OK
_TILE_FIELDS = ("tile_ptr", "tile_blk", "blk_off_dst", "ent_dst", "blk_off_src", "ent_src", "dis")


def _tiles(**kw):
    if kw.pop("null", False):
        return None
    t = _lib.CgnnTiles()
    t.num_nodes, t.num_tiles, t.max_tile_rows = 10, 1, 16
    for f in _TILE_FIELDS:
        setattr(t, f, _A)
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _l0(**kw):
    s = _lib.CgnnL0Src()
    s.P0, s.W0, s.b0, s.F0 = _A, _A, _A, 5
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _tail(mode):
    t = _lib.CgnnBnTail()
    t.acc, t.count, t.mode = _A, 10.0, mode
    for f in ("gamma", "beta", "running_mean", "running_var", "bn_out", "dgamma", "dbeta", "bwc"):
        setattr(t, f, _A)
    return t


# defaults that pass every check (such a call would launch; every row below breaks at least one of them)
_REFUSAL_DEFAULTS = {
    "cgnn_gcn_fused_fwd_first": dict(t={}, X0=_A, F0=5, W0=_A, bias=_A, Y=_A, stat_slab=_A, stat_slab_bytes=4096,
                                     stream=None),
    "cgnn_gcn_fused_fwd": dict(t={}, Yprev=_A, l0=None, bn_prev=_A, p_drop=0.0, seed=0, seed_dev=None, mask_out=None,
                               W=_A, bias=_A, Y=_A, stat_slab=_A, stat_slab_bytes=4096, tail=None, stream=None),
    "cgnn_gcn_fused_bwd": dict(t={}, dZ=_A, Y=_A, bn=_A, bwc=_A, Yprev=_A, l0=None, bn_prev=_A, p_drop=0.0,
                               mask_prev=None, W=_A, dZprev=_A, s_slab_prev=_A, s_slab_prev_bytes=4096, dW_slab=_A,
                               dW_slab_bytes=65536, db_slab=_A, db_slab_bytes=2048, dP=None, node_graph=None,
                               gptr=None, mask_cur=None, tail=None, stream=None),
    "cgnn_gcn_fused_bwd_first": dict(t={}, dZ=_A, Y=_A, bn=_A, bwc=_A, X0=_A, F0=5, dW_slab=_A, dW_slab_bytes=16384,
                                     db_slab=_A, db_slab_bytes=2048, p_drop=0.0, dP=None, node_graph=None, gptr=None,
                                     mask_cur=None, stream=None),
    "cgnn_gcn_fused_pool_bwd_sums": dict(dP=_A, F1=_A, F2=_A, gptr=_A, num_graphs=3, s_slab=_A, s_slab_bytes=4096,
                                         stream=None),
    "cgnn_gcn_fused_pool_bwd": dict(dP=_A, Y=_A, bn=_A, p_drop=0.0, mask=None, gptr=_A, num_graphs=3, dZ=_A,
                                    s_slab=_A, s_slab_bytes=4096, stream=None),
    "cgnn_aggregate_tiled_f32": dict(t={}, flags=0, X=_A, ldx=64, F=64, pre=None, post=None, bias=None, Yadd=None,
                                     ldadd=0, Y=_A, ldy=64, stream=None),
    "cgnn_aggregate_tiled_bn_f32": dict(t={}, flags=0, Z=_A, ldz=64, F=64, pre=None, post=None, bias=None, Y=_A,
                                        ldy=64, coef=_A, relu=1, p_drop=0.0, seed=0, seed_dev=None, mask_out=None,
                                        Xout=_A, ldxo=64, stream=None),
    "cgnn_aggregate_tiled_f16": dict(t={}, flags=0, X=_A, ldx=64, F=64, pre=None, post=None, bias=None, Y=_A, ldy=64,
                                     stream=None),
}

_FWD1, _FWD, _BWD, _BWD1 = ("cgnn_gcn_fused_fwd_first", "cgnn_gcn_fused_fwd", "cgnn_gcn_fused_bwd",
                            "cgnn_gcn_fused_bwd_first")
_PSUM, _PBWD = "cgnn_gcn_fused_pool_bwd_sums", "cgnn_gcn_fused_pool_bwd"
_AGG, _AGGBN, _AGGH = "cgnn_aggregate_tiled_f32", "cgnn_aggregate_tiled_bn_f32", "cgnn_aggregate_tiled_f16"
_POOLIN = dict(dP=_A, node_graph=_A, gptr=_A, dZ=None)

_REFUSALS = [
    # ---- first-layer forward
    (_FWD1, dict(t=dict(null=True)), _INV),
    (_FWD1, dict(t=dict(num_tiles=-1)), _INV),
    (_FWD1, dict(t=dict(num_nodes=-1)), _INV),
    (_FWD1, dict(t=dict(max_tile_rows=385)), _UNS),
    (_FWD1, dict(t=dict(max_tile_rows=385), F0=0), _UNS),            # the row limit decides, whatever else is wrong
    (_FWD1, dict(t=dict(max_tile_rows=385, dis=None)), _UNS),
    (_FWD1, dict(t=dict(dis=None)), _INV),
    (_FWD1, dict(t=dict(ent_src=None)), _INV),
    (_FWD1, dict(F0=0), _INV),
    (_FWD1, dict(F0=17), _INV),
    (_FWD1, dict(X0=None), _INV),
    (_FWD1, dict(Y=None), _INV),
    (_FWD1, dict(stat_slab_bytes=4095), _INV),
    # ---- projection-first forward
    (_FWD, dict(t=dict(null=True)), _INV),
    (_FWD, dict(t=dict(max_tile_rows=385)), _UNS),
    (_FWD, dict(t=dict(max_tile_rows=385), W=None), _UNS),
    (_FWD, dict(t=dict(tile_blk=None)), _INV),
    (_FWD, dict(Yprev=None), _INV),                                  # neither Yprev nor a factored layer 0
    (_FWD, dict(Yprev=None, l0=dict(F0=9)), _INV),
    (_FWD, dict(Yprev=None, l0=dict(W0=None)), _INV),
    (_FWD, dict(bn_prev=None), _INV),
    (_FWD, dict(p_drop=1.0), _INV),
    (_FWD, dict(p_drop=-0.5), _INV),
    (_FWD, dict(tail=1), _INV),                                      # a backward tail on the forward
    (_FWD, dict(stat_slab_bytes=4095), _INV),
    # ---- backward
    (_BWD, dict(t=dict(null=True)), _INV),
    (_BWD, dict(t=dict(max_tile_rows=385)), _UNS),
    (_BWD, dict(t=dict(max_tile_rows=385), p_drop=1.0), _UNS),
    (_BWD, dict(t=dict(blk_off_src=None)), _INV),
    (_BWD, dict(W=None), _INV),
    (_BWD, dict(Yprev=None), _INV),
    (_BWD, dict(s_slab_prev=None), _INV),                            # no slab and no tail to take the sums
    (_BWD, dict(p_drop=1.0), _INV),
    (_BWD, dict(p_drop=0.5), _INV),                                  # dropout without mask_prev
    (_BWD, dict(p_drop=0.5, mask_prev=0x1001), _INV),                # mask_prev is read as 4-byte words
    (_BWD, dict(dZ=None), _INV),
    (_BWD, dict(_POOLIN, gptr=None), _INV),
    (_BWD, dict(_POOLIN, p_drop=0.5, mask_prev=_A), _INV),           # readout form with dropout needs mask_cur
    (_BWD, dict(tail=0), _INV),                                      # a forward tail on the backward
    (_BWD, dict(s_slab_prev_bytes=4095), _INV),
    (_BWD, dict(dW_slab_bytes=65535), _INV),
    (_BWD, dict(db_slab_bytes=2047), _INV),
    # ---- first-layer backward
    (_BWD1, dict(t=dict(null=True)), _INV),
    (_BWD1, dict(t=dict(max_tile_rows=385)), _UNS),
    (_BWD1, dict(t=dict(max_tile_rows=385), F0=17), _UNS),
    (_BWD1, dict(t=dict(tile_ptr=None)), _INV),
    (_BWD1, dict(F0=0), _INV),
    (_BWD1, dict(F0=17), _INV),
    (_BWD1, dict(X0=None), _INV),
    (_BWD1, dict(p_drop=1.0), _INV),
    (_BWD1, dict(dZ=None), _INV),
    (_BWD1, dict(_POOLIN, node_graph=None), _INV),
    (_BWD1, dict(_POOLIN, p_drop=0.5), _INV),
    (_BWD1, dict(dW_slab_bytes=16383), _INV),
    (_BWD1, dict(db_slab_bytes=2047), _INV),
    # ---- readout backward
    (_PSUM, dict(num_graphs=-1), _INV),
    (_PSUM, dict(F2=None), _INV),
    (_PSUM, dict(s_slab=None), _INV),
    (_PSUM, dict(s_slab_bytes=4095), _INV),
    (_PBWD, dict(num_graphs=-1), _INV),
    (_PBWD, dict(p_drop=1.0), _INV),
    (_PBWD, dict(p_drop=0.5), _INV),                                 # dropout without its mask
    (_PBWD, dict(Y=None), _INV),
    (_PBWD, dict(s_slab=None), _INV),
    (_PBWD, dict(s_slab_bytes=4095), _INV),
    # ---- tiled aggregation, fp32: bad values first, then unsupported shapes, then an empty batch, then pointers
    (_AGG, dict(t=dict(null=True)), _INV),
    (_AGG, dict(t=dict(num_nodes=-1)), _INV),
    (_AGG, dict(t=dict(num_tiles=-1)), _INV),
    (_AGG, dict(F=0), _INV),
    (_AGG, dict(F=0, t=dict(max_tile_rows=385)), _INV),
    (_AGG, dict(ldx=63), _INV),
    (_AGG, dict(ldy=63), _INV),
    (_AGG, dict(Yadd=_A, ldadd=63), _INV),
    (_AGG, dict(Yadd=_A, ldadd=60, F=96, ldx=96, ldy=96), _INV),
    (_AGG, dict(F=96, ldx=96, ldy=96), _UNS),
    (_AGG, dict(F=96, ldx=96, ldy=96, X=None), _UNS),
    (_AGG, dict(ldx=66), _UNS),
    (_AGG, dict(ldy=66), _UNS),
    (_AGG, dict(Yadd=_A, ldadd=66), _UNS),
    (_AGG, dict(t=dict(max_tile_rows=385)), _UNS),
    (_AGG, dict(X=_M), _UNS),
    (_AGG, dict(Y=_M), _UNS),
    (_AGG, dict(bias=_M), _UNS),
    (_AGG, dict(Yadd=_M, ldadd=64), _UNS),
    (_AGG, dict(X=_M, t=dict(num_tiles=0)), _UNS),
    (_AGG, dict(X=None, t=dict(num_tiles=0)), _OK),                  # nothing to do comes before the NULL checks
    (_AGG, dict(X=None, t=dict(num_nodes=0)), _OK),
    (_AGG, dict(X=None), _INV),
    (_AGG, dict(Y=None), _INV),
    (_AGG, dict(t=dict(tile_ptr=None)), _INV),
    (_AGG, dict(t=dict(tile_blk=None)), _INV),
    (_AGG, dict(t=dict(ent_dst=None)), _INV),
    (_AGG, dict(t=dict(blk_off_dst=None)), _INV),
    (_AGG, dict(flags=1, t=dict(ent_src=None)), _INV),
    (_AGG, dict(flags=1, t=dict(blk_off_src=None)), _INV),
    # ---- tiled aggregation with the BatchNorm prologue
    (_AGGBN, dict(t=dict(null=True)), _INV),
    (_AGGBN, dict(F=0), _INV),
    (_AGGBN, dict(ldz=63), _INV),
    (_AGGBN, dict(ldxo=63), _INV),
    (_AGGBN, dict(p_drop=1.0), _INV),
    (_AGGBN, dict(p_drop=1.0, F=96, ldz=96, ldy=96, ldxo=96), _INV),
    (_AGGBN, dict(coef=None), _INV),
    (_AGGBN, dict(coef=None, t=dict(max_tile_rows=385)), _INV),
    (_AGGBN, dict(Xout=None), _INV),
    (_AGGBN, dict(F=96, ldz=96, ldy=96, ldxo=96), _UNS),
    (_AGGBN, dict(ldz=66), _UNS),
    (_AGGBN, dict(ldxo=66), _UNS),
    (_AGGBN, dict(t=dict(max_tile_rows=385)), _UNS),
    (_AGGBN, dict(Z=_M), _UNS),
    (_AGGBN, dict(coef=_M), _UNS),
    (_AGGBN, dict(Xout=_M), _UNS),
    (_AGGBN, dict(Z=None, t=dict(num_tiles=0)), _OK),
    (_AGGBN, dict(Z=None), _INV),
    (_AGGBN, dict(Y=None), _INV),
    (_AGGBN, dict(flags=1, t=dict(ent_src=None)), _INV),
    # ---- tiled aggregation, fp16 storage: 8-element row strides, 1024-row tiles
    (_AGGH, dict(t=dict(null=True)), _INV),
    (_AGGH, dict(t=dict(num_tiles=-1)), _INV),
    (_AGGH, dict(F=-64), _INV),
    (_AGGH, dict(ldy=63), _INV),
    (_AGGH, dict(F=96, ldx=96, ldy=96), _UNS),
    (_AGGH, dict(ldx=68), _UNS),
    (_AGGH, dict(ldy=68), _UNS),
    (_AGGH, dict(t=dict(max_tile_rows=1025)), _UNS),
    (_AGGH, dict(t=dict(max_tile_rows=1024), X=None), _INV),         # 1024 rows pass the limit; the NULL is what is wrong
    (_AGGH, dict(X=_M), _UNS),
    (_AGGH, dict(bias=_M), _UNS),
    (_AGGH, dict(Y=None, t=dict(num_nodes=0)), _OK),
    (_AGGH, dict(Y=None), _INV),
    (_AGGH, dict(t=dict(tile_ptr=None)), _INV),
    (_AGGH, dict(flags=1, t=dict(blk_off_src=None)), _INV),
]


def test_tile_entry_points_refuse_bad_arguments_with_the_documented_code():
    lib = _lib.load()
    assert lib.cgnn_set_fused_grid(_GRID) == _OK
    keep = []                                    # structures passed by pointer stay alive over the call
    got = []
    try:
        for name, bad, want in _REFUSALS:
            args = dict(_REFUSAL_DEFAULTS[name])
            unknown = set(bad) - set(args)
            assert not unknown, (name, unknown)
            args.update(bad)
            t = _tiles(**args["t"]) if "t" in args else None
            if "t" in args:
                args["t"] = ctypes.byref(t) if t is not None else None
            if isinstance(args.get("l0"), dict):
                args["l0"] = ctypes.byref(_l0(**args["l0"]))
            if isinstance(args.get("tail"), int):
                args["tail"] = ctypes.byref(_tail(args["tail"]))
            keep.append((t, args))
            got.append((name, bad, want, getattr(lib, name)(*args.values())))
    finally:
        assert lib.cgnn_set_fused_grid(0) == _OK
    wrong = [(n, b, w, g) for n, b, w, g in got if g != w]
    assert not wrong, wrong


# ---- argument checks of the node-measure families (csrc/measure_request.h; measures.hip, paths.hip, wpaths.hip) ----
# The same kind of table for cgnn_ingest_{measures,paths,wpaths} and their _workspace_bytes: one row = one call and
# what it returns.  No row launches or reaches the HIP runtime: it is a refusal, a call with S == 0 (CGNN_OK before any
# pointer is looked at) or a byte-count query.  S = 6 (wpaths: 3) subjects of n = 20 nodes, every measure of the family.
_i32 = ctypes.c_int32
_MEAS, _PATHS, _WPATHS = "cgnn_ingest_measures", "cgnn_ingest_paths", "cgnn_ingest_wpaths"
_MEAS_WS, _PATHS_WS, _WPATHS_WS = (f + "_workspace_bytes" for f in (_MEAS, _PATHS, _WPATHS))
_ID5, _ID4, _ID3 = (_i32 * 5)(0, 1, 2, 3, 4), (_i32 * 4)(0, 1, 2, 3), (_i32 * 3)(0, 1, 2)
_COL4, _COL3 = (_i32 * 4)(5, 1, 2, 4), (_i32 * 3)(5, 1, 3)
_A2 = 0x1002                     # a pointer that is not 4-byte aligned
_EMPTY = dict(matrices=None, S=0, thr=None, workspace=None, workspace_bytes=0, x=None, x_bytes=0)
_BIG_S = 2 ** 31 // 20 + 1       # S * n >= 2^31 at n = 20

# defaults that pass every check (the three calls would launch; every row below breaks a check or has S == 0)
_MEASURE_DEFAULTS = {
    _MEAS_WS: dict(S=6, n=20, measures=_ID5, num=5),
    _PATHS_WS: dict(S=6, n=20, measures=_ID4, num=4),
    _WPATHS_WS: dict(S=3, n=20, measures=_ID3, num=3),
    _MEAS: dict(matrices=_A, S=6, n=20, thr=_A, measures=_ID5, num=5, workspace=_A, workspace_bytes=5888, x=_A,
                x_bytes=2400, stream=None),
    _PATHS: dict(matrices=_A, S=6, n=20, thr=_A, measures=_ID4, num=4, cols=_COL4, ldx=7, workspace=_A,
                 workspace_bytes=16, x=_A, x_bytes=3360, stream=None),
    _WPATHS: dict(matrices=_A, S=3, n=20, thr=_A, measures=_ID3, num=3, cols=_COL3, ldx=6, workspace=_A,
                  workspace_bytes=12288, x=_A, x_bytes=1440, dist=_A, dist_bytes=4800, stream=None),
}

_MEASURE_CALLS = [
    # ---- byte counts: [k | s | (smax, wmax) | T(b) partials | T(u) partials]; none; a slab per workgroup at grid 4
    (_MEAS_WS, dict(), 5888),
    (_MEAS_WS, dict(measures=(_i32 * 2)(1, 0), num=2), 1280),        # no partial sums without clustering
    (_MEAS_WS, dict(measures=(_i32 * 1)(3), num=1), 3584),
    (_MEAS_WS, dict(S=0), 0),
    (_MEAS_WS, dict(S=1, n=46340), 179537664),                       # the largest n with n * n < 2^31
    (_MEAS_WS, dict(S=1, n=46341), _INV),
    (_MEAS_WS, dict(S=-1), _INV),
    (_MEAS_WS, dict(n=0), _INV),
    (_MEAS_WS, dict(measures=None), _INV),
    (_MEAS_WS, dict(measures=None, num=0), _INV),
    (_MEAS_WS, dict(num=0), _INV),
    (_MEAS_WS, dict(num=6), _INV),
    (_MEAS_WS, dict(measures=(_i32 * 2)(3, 3), num=2), _INV),
    (_MEAS_WS, dict(S=_BIG_S), _INV),
    (_MEAS_WS, dict(n=46341), _INV),
    (_PATHS_WS, dict(), 0),
    (_PATHS_WS, dict(n=1024), 0),
    (_PATHS_WS, dict(n=1025), _INV),
    (_PATHS_WS, dict(S=-1), _INV),
    (_PATHS_WS, dict(n=0), _INV),
    (_PATHS_WS, dict(measures=None), _INV),
    (_PATHS_WS, dict(measures=None, num=0), _INV),
    (_PATHS_WS, dict(num=0), _INV),
    (_PATHS_WS, dict(num=5), _INV),
    (_PATHS_WS, dict(measures=(_i32 * 2)(3, 3), num=2), _INV),
    (_PATHS_WS, dict(measures=(_i32 * 1)(4), num=1), _INV),
    (_PATHS_WS, dict(S=_BIG_S), _INV),
    (_WPATHS_WS, dict(), 12288),
    (_WPATHS_WS, dict(measures=None, num=0), 12288),                 # distances alone: no measure is a request
    (_WPATHS_WS, dict(S=100, n=84), 16 * 96 * 96 * 4),               # 4 workgroups a CU at 32 KB of LDS
    (_WPATHS_WS, dict(S=100, n=360), 4 * 384 * 384 * 4),             # 1 at 104 KB
    (_WPATHS_WS, dict(S=100, n=512), 4 * 512 * 512 * 4),             # blocks of 32 up to here: 136 KB
    (_WPATHS_WS, dict(S=100, n=513), 8 * 528 * 528 * 4),             # of 16 beyond: 2 at 68 KB
    (_WPATHS_WS, dict(n=1024), 3 * 1024 * 1024 * 4),
    (_WPATHS_WS, dict(n=1025), _INV),
    (_WPATHS_WS, dict(S=-1), _INV),
    (_WPATHS_WS, dict(n=0), _INV),
    (_WPATHS_WS, dict(measures=None), _INV),
    (_WPATHS_WS, dict(num=4), _INV),
    (_WPATHS_WS, dict(num=-1), _INV),
    (_WPATHS_WS, dict(measures=(_i32 * 2)(2, 2), num=2), _INV),
    (_WPATHS_WS, dict(measures=(_i32 * 1)(3), num=1), _INV),
    (_WPATHS_WS, dict(S=_BIG_S), _INV),
    # ---- cgnn_ingest_measures
    (_MEAS, dict(workspace_bytes=5887), _INV),
    (_MEAS, dict(x_bytes=2399), _INV),
    (_MEAS, dict(x_bytes=-1), _INV),
    (_MEAS, dict(workspace_bytes=-1), _INV),
    (_MEAS, dict(matrices=None), _INV),
    (_MEAS, dict(thr=None), _INV),
    (_MEAS, dict(measures=None), _INV),
    (_MEAS, dict(workspace=None), _INV),
    (_MEAS, dict(x=None), _INV),
    (_MEAS, dict(S=-1), _INV),
    (_MEAS, dict(n=0), _INV),
    (_MEAS, dict(n=-3), _INV),
    (_MEAS, dict(S=_BIG_S), _INV),
    (_MEAS, dict(n=46341), _INV),
    (_MEAS, dict(num=0), _INV),
    (_MEAS, dict(num=-1), _INV),
    (_MEAS, dict(num=6), _INV),
    (_MEAS, dict(measures=(_i32 * 5)(0, 1, 2, 3, 5)), _INV),
    (_MEAS, dict(measures=(_i32 * 5)(0, -1, 2, 3, 4)), _INV),
    (_MEAS, dict(measures=(_i32 * 5)(0, 1, 2, 3, 3)), _INV),
    (_MEAS, dict(workspace=_M), _INV),
    (_MEAS, dict(matrices=_A2), _INV),
    (_MEAS, dict(thr=_A2), _INV),
    (_MEAS, dict(x=_A2), _INV),
    (_MEAS, dict(measures=None, num=0, x=None, x_bytes=0), _INV),    # no measure: only wpaths takes that
    (_MEAS, dict(S=0), _OK),
    (_MEAS, dict(_EMPTY), _OK),
    (_MEAS, dict(_EMPTY, n=46340), _OK),
    (_MEAS, dict(_EMPTY, n=46341), _INV),
    (_MEAS, dict(_EMPTY, workspace=_M, workspace_bytes=-1, x_bytes=-1), _OK),   # buffers come after S == 0 here
    (_MEAS, dict(_EMPTY, num=0), _INV),                              # the request comes before it
    (_MEAS, dict(_EMPTY, measures=None, num=0), _INV),
    (_MEAS, dict(_EMPTY, measures=None), _INV),
    # ---- cgnn_ingest_paths
    (_PATHS, dict(x_bytes=3359), _INV),
    (_PATHS, dict(x_bytes=-1), _INV),
    (_PATHS, dict(matrices=None), _INV),
    (_PATHS, dict(thr=None), _INV),
    (_PATHS, dict(measures=None), _INV),
    (_PATHS, dict(cols=None), _INV),
    (_PATHS, dict(x=None), _INV),
    (_PATHS, dict(S=-1), _INV),
    (_PATHS, dict(n=0), _INV),
    (_PATHS, dict(n=-3), _INV),
    (_PATHS, dict(n=1025), _INV),
    (_PATHS, dict(S=_BIG_S), _INV),
    (_PATHS, dict(num=0), _INV),
    (_PATHS, dict(num=-1), _INV),
    (_PATHS, dict(num=5), _INV),
    (_PATHS, dict(measures=(_i32 * 4)(0, 1, 2, 4)), _INV),
    (_PATHS, dict(measures=(_i32 * 4)(0, -1, 2, 3)), _INV),
    (_PATHS, dict(measures=(_i32 * 4)(0, 1, 3, 3)), _INV),
    (_PATHS, dict(cols=(_i32 * 4)(5, 1, 2, 7)), _INV),               # a column == ldx
    (_PATHS, dict(cols=(_i32 * 4)(5, -1, 2, 4)), _INV),
    (_PATHS, dict(cols=(_i32 * 4)(5, 1, 2, 5)), _INV),
    (_PATHS, dict(ldx=5), _INV),
    (_PATHS, dict(ldx=0), _INV),
    (_PATHS, dict(workspace_bytes=-1), _INV),
    (_PATHS, dict(workspace=_M), _INV),
    (_PATHS, dict(matrices=_A2), _INV),
    (_PATHS, dict(x=_A2), _INV),
    (_PATHS, dict(thr=_A2), _INV),
    (_PATHS, dict(ldx=2 ** 31 - 1), _INV),                           # S * n * ldx * 4 would wrap 64 bits
    (_PATHS, dict(ldx=2 ** 30), _INV),
    (_PATHS, dict(measures=None, num=0, cols=None, x=None, x_bytes=0), _INV),   # no measure: only wpaths takes that
    (_PATHS, dict(S=0), _OK),
    (_PATHS, dict(_EMPTY), _OK),
    (_PATHS, dict(_EMPTY, n=1024), _OK),
    (_PATHS, dict(_EMPTY, n=1025), _INV),
    (_PATHS, dict(_EMPTY, ldx=2 ** 31 - 1), _OK),
    (_PATHS, dict(_EMPTY, workspace_bytes=-1), _INV),                # these two come before S == 0
    (_PATHS, dict(_EMPTY, workspace=_M), _INV),
    (_PATHS, dict(_EMPTY, x_bytes=-1), _OK),                         # x's byte count after it
    (_PATHS, dict(_EMPTY, num=0), _INV),
    (_PATHS, dict(_EMPTY, measures=None, num=0, cols=None), _INV),
    (_PATHS, dict(_EMPTY, cols=None), _INV),
    # ---- cgnn_ingest_wpaths
    (_WPATHS, dict(x_bytes=1439), _INV),
    (_WPATHS, dict(dist_bytes=4799), _INV),
    (_WPATHS, dict(workspace_bytes=12287), _INV),
    (_WPATHS, dict(workspace=None), _INV),
    (_WPATHS, dict(matrices=None), _INV),
    (_WPATHS, dict(thr=None), _INV),
    (_WPATHS, dict(measures=None), _INV),
    (_WPATHS, dict(cols=None), _INV),
    (_WPATHS, dict(x=None), _INV),
    (_WPATHS, dict(S=-1), _INV),
    (_WPATHS, dict(n=0), _INV),
    (_WPATHS, dict(n=-3), _INV),
    (_WPATHS, dict(n=1025), _INV),
    (_WPATHS, dict(S=_BIG_S), _INV),
    (_WPATHS, dict(num=-1), _INV),
    (_WPATHS, dict(num=4), _INV),
    (_WPATHS, dict(measures=(_i32 * 3)(0, 1, 3)), _INV),
    (_WPATHS, dict(measures=(_i32 * 3)(0, -1, 2)), _INV),
    (_WPATHS, dict(measures=(_i32 * 3)(0, 2, 2)), _INV),
    (_WPATHS, dict(cols=(_i32 * 3)(5, 1, 6)), _INV),                 # a column == ldx
    (_WPATHS, dict(cols=(_i32 * 3)(5, -1, 3)), _INV),
    (_WPATHS, dict(cols=(_i32 * 3)(5, 1, 5)), _INV),
    (_WPATHS, dict(ldx=5), _INV),
    (_WPATHS, dict(ldx=0), _INV),
    (_WPATHS, dict(workspace_bytes=-1), _INV),
    (_WPATHS, dict(x_bytes=-1), _INV),
    (_WPATHS, dict(dist_bytes=-1), _INV),
    (_WPATHS, dict(workspace=_M), _INV),
    (_WPATHS, dict(matrices=_A2), _INV),
    (_WPATHS, dict(x=_A2), _INV),
    (_WPATHS, dict(dist=_A2), _INV),
    (_WPATHS, dict(thr=_A2), _INV),
    (_WPATHS, dict(ldx=2 ** 31 - 1), _INV),
    (_WPATHS, dict(ldx=2 ** 30), _INV),
    (_WPATHS, dict(measures=None, num=0, cols=None, ldx=0, x=None, x_bytes=0, dist=None, dist_bytes=0), _INV),  # neither
    (_WPATHS, dict(measures=None, num=0, cols=None, ldx=0, x=None, x_bytes=0, workspace_bytes=12287), _INV),
    (_WPATHS, dict(S=0), _OK),
    (_WPATHS, dict(_EMPTY, dist=None, dist_bytes=0), _OK),
    (_WPATHS, dict(_EMPTY, dist=None, dist_bytes=0, n=1024), _OK),
    (_WPATHS, dict(_EMPTY, dist=None, dist_bytes=0, n=1025), _INV),
    (_WPATHS, dict(_EMPTY, dist=None, dist_bytes=0, ldx=2 ** 31 - 1), _OK),
    (_WPATHS, dict(_EMPTY, dist=None, dist_bytes=0, workspace_bytes=-1), _INV),     # these four come before S == 0
    (_WPATHS, dict(_EMPTY, dist=None, dist_bytes=0, workspace=_M), _INV),
    (_WPATHS, dict(_EMPTY, dist=None, dist_bytes=0, x_bytes=-1), _INV),
    (_WPATHS, dict(_EMPTY, dist=None, dist_bytes=-1), _INV),
    (_WPATHS, dict(_EMPTY, measures=None, num=0, cols=None, ldx=0, dist_bytes=0), _OK),   # distances alone, x NULL
    (_WPATHS, dict(_EMPTY, cols=None, dist=None, dist_bytes=0), _INV),
]


def test_measure_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.load()
    assert lib.cgnn_set_fused_grid(_GRID) == _OK
    got = []
    try:
        for name, change, want in _MEASURE_CALLS:
            args = dict(_MEASURE_DEFAULTS[name])
            unknown = set(change) - set(args)
            assert not unknown, (name, unknown)
            args.update(change)
            got.append((name, change, want, getattr(lib, name)(*args.values())))
    finally:
        assert lib.cgnn_set_fused_grid(0) == _OK
    wrong = [(n, c, w, g) for n, c, w, g in got if g != w]
    assert not wrong, wrong
