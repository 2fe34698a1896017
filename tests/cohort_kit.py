"""What the GPU tests of the column families share (test_gpu_paths, _wpaths, _modules, _pagerank, _core, _rw): a family
turns a cohort of matrices ``[S, n, n]`` into columns ``[S, n, F]`` through one C entry point with the ``ids, cols, ldx``
request of ``ingest._run_family``.  Here are the helpers that were the same code up to the family's names, and the bodies
of the properties every such family has, each as a function of ``call``, the family's public function as a closure.

Not here, on purpose: the parity of a family with its fp64 statement (``_check_cohort``), its staging paths, its sizes
and refusals, its NaN and +inf rules.  Those are what a family is; they stay in its test file, and so does every
assertion that one family makes and another does not, even under the same test name."""
import contextlib
import ctypes

import torch

import connectome_gnn_amd as C
from connectome_gnn_amd import _lib, encoder_choice, ingest
from connectome_gnn_amd.resident import ResidentDataLoader
from tests import ingest_data as I
from tests import modules_data as D

DEV = "cuda"
NAN_BITS = 0x7FC00000


def bits(t):
    """The int32 view of a float32 (or int32) tensor: what bit equality compares."""
    return t.contiguous().view(torch.int32)


def thresholds(dev, mats, kw):
    """(device thresholds, the host's) of ``keep=`` or ``min_weight=0.0``: the same numbers."""
    host = D.host_thresholds(mats, kw)
    thr = ingest.select_thresholds(dev, **kw) if "keep" in kw else torch.zeros(len(mats), device=DEV)
    assert thr.cpu().tolist() == host
    return thr, host


def raw(name, dev, thr, ids, cols, ldx, head=(), mid=(), tail=(), work=None, accept=()):
    """One call of the C entry point ``name`` on ``dev`` ``[S, n, n]``: measure ``ids[m]`` into column ``cols[m]`` of a
    NaN-filled ``x`` ``[S, n, ldx]`` (``None`` where no id is asked for).  ``head``, ``mid`` and ``tail`` are what else
    the signature takes, where ``ingest._run_family`` puts them: between ``thr`` and the request, between ``cols, ldx``
    and the workspace, behind ``x``; ``work`` is the workspace.  Returns ``(x, the return code)``; a code that is
    neither CGNN_OK nor in ``accept`` raises."""
    S, n = int(dev.shape[0]), int(dev.shape[1])
    x = torch.full((S, n, ldx), float("nan"), device=DEV) if ids else None
    num = len(ids)
    rc = _lib.call(name, dev, S, n, thr, *head, (ctypes.c_int32 * num)(*ids), num, (ctypes.c_int32 * num)(*cols), ldx,
                   *mid, *_lib.buf(work), *_lib.buf(x), *tail, accept=accept)
    return x, rc


@contextlib.contextmanager
def grid_of_three():
    """The launch grid (``cgnn_set_fused_grid``, process-wide) at 3 inside the block, and as it was after it.  The hook
    can be read only through its effect, ``cgnn_fused_grid()``: 0 takes the override away, and where that does not give
    the grid that was read on entry, an override was in force then and is put back."""
    lib = _lib.load()
    saved = int(lib.cgnn_fused_grid())
    try:
        assert lib.cgnn_set_fused_grid(3) == _lib.CGNN_OK
        yield
    finally:
        lib.cgnn_set_fused_grid(0)
        if int(lib.cgnn_fused_grid()) != saved:
            lib.cgnn_set_fused_grid(saved)


# ---- the properties ----
def check_grid_of_three(run):
    """``run()``, a tuple of device tensors, at a grid of three, at the default grid and once more: the same bits.
    Returns ``(few, full)``, the first two."""
    with grid_of_three():
        few = run()
    full, again = run(), run()
    for a, b, c in zip(few, full, again):
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(b), bits(c))
    return few, full


def check_knn(call, dev):
    """``knn=8`` in both symmetric modes is ``call`` on ``knn_sparsify``'s matrices at ``min_weight=0.0``, by bits."""
    for mode in ("union", "mutual"):
        sparse = ingest.knn_sparsify(dev, 8, mode=mode)
        assert torch.equal(bits(call(dev, knn=8, knn_mode=mode)), bits(call(sparse, min_weight=0.0))), mode


def check_backbone(call, dev, **kw):
    """``backbone="mst"``, alone and united with ``keep=0.1``, is ``call`` on ``mst_backbone``'s matrices at
    ``min_weight=0.0``, by bits; ``kw`` goes to both sides of the united case, whose result is returned."""
    assert torch.equal(bits(call(dev, backbone="mst")), bits(call(ingest.mst_backbone(dev), min_weight=0.0)))
    got = call(dev, backbone="mst", keep=0.1, **kw)
    united = ingest.mst_backbone(dev, keep=0.1)
    assert torch.equal(bits(got), bits(call(united, min_weight=0.0, **kw)))
    return got


def check_group(call, dev, **kw):
    """``group="mean"`` at ``keep=0.1`` is ``call`` on ``group_sparsify``'s matrices at ``min_weight=0.0``, by bits."""
    masked = ingest.group_sparsify(dev, "mean", keep=0.1)
    assert torch.equal(bits(call(dev, group="mean", keep=0.1, **kw)), bits(call(masked, min_weight=0.0, **kw)))


def check_no_subjects(call, dev, cols, dtype=torch.float32):
    """``call`` on the empty cohort ``dev`` ``[0, n, n]``: an empty ``[0, n, cols]`` of ``dtype`` on the device."""
    x = call(dev)
    assert tuple(x.shape) == (0, int(dev.shape[1]), cols) and x.dtype == dtype and x.device.type == "cuda"


def check_trains_on_the_fused_path(call, cols):
    """The ``cols`` columns of ``call`` on 12 random symmetric subjects of 84 nodes, passed as ``node_features=``: one
    epoch of a GCN runs on the fused tile path, chosen for no other reason.  Returns ``(matrices, columns)`` for what
    the family knows about its values."""
    S, n = 12, 84
    r = torch.rand(S, n, n, generator=torch.Generator().manual_seed(4))
    mats = torch.maximum(r, r.transpose(1, 2)).contiguous().to(DEV)
    feats = call(mats)
    assert feats.shape == (S, n, cols) and bool(torch.isfinite(feats).all())
    ds = ingest.from_matrices(mats, I.labels(S).to(DEV), keep=0.1, node_features=feats)
    assert ds.x.shape == (S, n, cols)
    torch.manual_seed(3)
    m = C.GCNConnectome(cols, 64, dropout=0.0)
    tr = C.Trainer(m, torch.optim.Adam(m.parameters(), lr=1e-3), device=DEV)
    ld = ResidentDataLoader(ds, 6, shuffle=True, structure_cache=True)
    loss = tr.train_epoch(ld)
    assert loss == loss and abs(loss) != float("inf"), loss
    assert tr.model.impl_used == "fused" and tr.model._fused_kind == "tile"
    batch = next(iter(ld))
    choice = encoder_choice.choose(tr.model, batch, batch.structure())
    assert choice.kind == "tile" and choice.reason is None, choice
    return mats, feats
