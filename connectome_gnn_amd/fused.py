"""Fused per-tile GCN encoder (hidden = 64): host orchestration of csrc/fused_gcn.hip.

One ``torch.autograd.Function`` covers GCNConnectome.encode end to end (reference
models.py:203-211): per layer one persistent HIP kernel that keeps each tile's [rows x 64]
feature block in LDS, plus two tiny kernels for the batch-wide BatchNorm reduction.  What
touches HBM per layer is the previous layer's pre-BatchNorm output (read), the CSR (read)
and this layer's pre-BatchNorm output (write); BatchNorm-apply, ReLU, dropout, the
projection and the BatchNorm statistics never make a round trip.

Saved for backward: the pre-BatchNorm outputs Y_l, the 4x64 BatchNorm coefficient blocks and
one dropout keep-byte per (node, 4-column chunk); activations are rebuilt in LDS.
"""
from __future__ import annotations

import os
from typing import List, Optional

import torch
import torch.distributed as dist

from . import _lib, bn_stage, ops

HID = 64
MAX_ROWS = 384
MAX_F0 = 16


def widths_ineligible(model) -> Optional[str]:
    """The part of eligible() that the layer widths decide (Trainer asks it before building a subject cache)."""
    hid, fin = model.convs[0].linear.weight.shape
    if hid != HID:
        return f"hidden_dim != {HID}"
    if fin > MAX_F0:
        return f"in_channels > {MAX_F0}"
    return None


def eligible(model, batch, structure) -> Optional[str]:
    """None if the fused path covers this (model, batch); else the reason it does not."""
    why = widths_ineligible(model)
    if why is not None:
        return why
    if not structure.block_diagonal:
        return "edges cross graph boundaries"
    if structure.max_nodes_per_graph > MAX_ROWS:
        return f"a graph has more than {MAX_ROWS} nodes"
    why = bn_stage.ineligible(batch, structure, input_grad_ok=True)
    if why is not None:
        return why
    if batch.node_features.requires_grad and not _narrow0(len(model.convs), model.convs[0].linear.weight.shape[1]):
        # dX0 = A_hat^T (dY0 W0) exists for the factored layer 0 only (cgnn_gcn_l0_bwd_dx, cgnn_gcn_l0_dx)
        return ("node_features require grad: the fused path returns the input gradient from its narrow layer 0 "
                "only (in_channels <= 8 and num_layers >= 2)")
    # looser than bn_stage.bn_modules_ok (no type test); merging them would move a GCN with a BatchNorm1d subclass
    # off the per-tile kernels
    for bn in model.batch_norms:
        if not (bn.affine and bn.track_running_stats) or bn.momentum is None:
            return "BatchNorm without affine/running stats/momentum"
    return None


def _tiles_struct(s, meta, dis: torch.Tensor):
    return s.tiles_struct(meta, dis)


def _narrow0(num_layers: int, in_channels: int) -> bool:
    """Layer 0 runs in the narrow (factored) form of csrc/fused_gcn_l0.hip."""
    return num_layers >= 2 and in_channels <= 8


_ZEROS = {}


def _zeros(dev) -> torch.Tensor:
    """64 fp32 zeros on `dev` (the bias of a layer handed on without its constant term)."""
    z = _ZEROS.get(dev)
    if z is None:
        z = _ZEROS[dev] = torch.zeros(HID, dtype=torch.float32, device=dev)
    return z


def _l0_center(s, x0: torch.Tensor, tiles, stream) -> torch.Tensor:
    """The centring constants of the factored layer 0 (cgnn_gcn_l0_center): column means of X0 and
    the mean row sum of the normalised operator over the batch's first tile.  It is a conditioning hint, not part of the arithmetic (any value
    gives the same result up to rounding), so it is computed once per (batch, feature tensor)
    and cached on the structure -- one tiny launch at a batch's first use -- or once per DATASET for
    batches assembled from a per-subject structure cache."""
    cache = s.cache
    if cache is not None and torch.cuda.is_current_stream_capturing():
        # a captured step that assembles another batch of a per-subject structure cache on every replay:
        # ONE set of constants per dataset -- those of the batch the step's eager warm-up ran on, stored
        # below -- instead of a launch per replay (6.4 us of a 0.2 ms step at 512 x 84-ROI).  Any value is
        # correct; eager steps keep their per-batch constants (and with them bit-identity to the
        # per-batch build of the same subjects).
        const = cache._l0_center
        if const is not None and const[0] == int(x0.shape[1]):
            return const[1]
    key = (x0.data_ptr(), x0._version, tuple(x0.shape))
    hit = s._l0_center
    if hit is None or hit[0] != key:
        center = torch.empty(8, dtype=torch.float32, device=x0.device)
        _lib.call("cgnn_gcn_l0_center", tiles, x0, x0.shape[1], center, stream=stream)
        hit = (key, center)
        s._l0_center = hit
        if cache is not None and not torch.cuda.is_current_stream_capturing() and cache._l0_center is None:
            cache._l0_center = (int(x0.shape[1]), center)
    return hit[1]


# diagnostic A/B switch (never set in the product): recompute dis, P0 and its moments on every step of a kept
# batch (cgnn_gcn_dis + cgnn_gcn_l0_fwd), as on a batch that is not kept
_NO_L0_CACHE = bool(os.environ.get("CGNN_DIAG_NO_L0_CACHE"))


def _kept(s) -> bool:
    """`s` belongs to a batch that is trained on repeatedly (prepare_batch(reuse=True) -> keep_batch): what
    layer 0 derives from the batch alone -- dis, P0 and the moments of its rows -- is kept with it."""
    return not _NO_L0_CACHE and bool(s._kept)


def _l0_batch_constants(s, x0: torch.Tensor, center, tiles, sets: int, stream):
    """(P0, moments) of the factored layer 0 on a kept structure, or None = run the full kernel.  Cached as
    `_l0_center` / `permuted_features` are: per (feature tensor, its version, shape), per centre tensor (None
    for the raw form) and per cgnn_l0_grid (the cgnn_set_fused_grid test hook changes it).  A miss aggregates
    again (cgnn_gcn_l0_agg) -- except while a stream is capturing, where nothing may be allocated into the
    graph's pool and kept: the step then runs cgnn_gcn_l0_fwd."""
    key = (x0.data_ptr(), x0._version, tuple(x0.shape), None if center is None else center.data_ptr(), sets)
    hit = s._l0_batch
    if hit is not None and hit[0] == key:
        return hit[3], hit[4]
    if torch.cuda.is_current_stream_capturing():
        return None
    p0 = torch.empty(s.num_nodes, 8, dtype=torch.float32, device=x0.device)
    moments = torch.empty(sets, 81, dtype=torch.float64, device=x0.device)
    _lib.call("cgnn_gcn_l0_agg", tiles, x0, x0.shape[1], center, p0, *_lib.buf(moments), stream=stream)
    # (x0 and the centre are held so that their addresses stay theirs while the entry lives)
    s._l0_batch = (key, x0, center, p0, moments)
    return p0, moments


def keep_batch(model, s, x0: torch.Tensor) -> None:
    """prepare_batch(reuse=True): mark the structure the encoder will run on as kept and, when the narrow
    layer 0 applies, fill its batch constants now -- eagerly, outside any capture."""
    if not s.has_csr or s.num_nodes == 0:     # (a cached structure lives for one shuffle)
        return
    s._kept = True
    if _NO_L0_CACHE or x0.requires_grad or not x0.is_cuda:
        return
    lib = _lib.load()
    fmeta = s.fused_meta(MAX_ROWS, lib.cgnn_fused_grid())
    with _lib.device_guard(x0.device):
        dis = s.gcn_dis(fmeta)
        if not _narrow0(len(model.convs), x0.shape[1]):
            return
        x0 = x0.detach().contiguous()
        tiles = _tiles_struct(s, fmeta, dis)
        sp = _lib.stream_ptr(x0.device)
        center = _l0_center(s, x0, tiles, sp) if (x0.shape[1] < 8 and bn_stage.sync_group_of(model) is None) else None
        _l0_batch_constants(s, x0, center, tiles, lib.cgnn_l0_grid(s.num_nodes), sp)


class _Ctx:
    """Everything of one forward pass that backward needs and autograd must not track."""
    __slots__ = ("s", "meta", "dis", "tiles", "grid", "ys", "bns", "masks", "p", "x0", "f0", "p0", "count_dev", "fsum", "l0src", "l0keep",
                 "count", "sync_group", "num_layers", "training", "grad_dst", "bn_modules")


def _sync_sums(buf: torch.Tensor, group) -> None:
    """Full-batch BatchNorm across ranks (SURVEY 8e option i): one all-reduce of the fp64 block
    [sum | sumsq | rows]; everything, the row count included, stays on the device."""
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)


# diagnostic A/B switch (never set in the product): the slab + finalisation-launch protocol of rounds 1-3
_NO_TAILS = bool(os.environ.get("CGNN_DIAG_NO_BN_TAILS"))


def _bn_acc(bn_mod, dev, which: int) -> torch.Tensor:
    """The module's accumulator for BatchNorm sums finalised in a producer kernel's tail (csrc/bn_tail.h):
    zero when created, left zero by every launch that uses it.  which: 0 = forward statistics, 1 = backward."""
    acc = bn_mod.__dict__.get("_cgnn_acc")
    if acc is None or acc.device != dev:
        acc = torch.zeros(2, _lib.BN_ACC_BYTES // 8, dtype=torch.int64, device=dev)
        bn_mod.__dict__["_cgnn_acc"] = acc
    return acc[which]


def _tail_fwd(bn_mod, dev, count, gamma, beta, bn_out, rng, rng_n) -> "_lib.CgnnBnTail":
    t = _lib.CgnnBnTail()
    t.acc, t.count, t.mode = _bn_acc(bn_mod, dev, 0).data_ptr(), float(count), 0
    t.gamma, t.beta = gamma.data_ptr(), beta.data_ptr()
    t.running_mean, t.running_var = bn_mod.running_mean.data_ptr(), bn_mod.running_var.data_ptr()
    t.momentum, t.eps = float(bn_mod.momentum), float(bn_mod.eps)
    t.num_batches_tracked = bn_mod.num_batches_tracked.data_ptr()
    t.bn_out = bn_out.data_ptr()
    t.rng_state, t.rng_n = (rng.data_ptr(), rng_n) if rng is not None else (None, 0)
    return t


def _tail_bwd(bn_mod, dev, count, zero_coef, dgamma, dbeta, bwc) -> "_lib.CgnnBnTail":
    t = _lib.CgnnBnTail()
    t.acc, t.count, t.mode, t.zero_coef = _bn_acc(bn_mod, dev, 1).data_ptr(), float(count), 1, int(zero_coef)
    t.dgamma, t.dbeta, t.bwc = dgamma.data_ptr(), dbeta.data_ptr(), bwc.data_ptr()
    return t


class FusedGCNEncode(torch.autograd.Function):
    """P[B,64] = mean-pool(GCN stack(x0)); args = x0, then (W, b, gamma, beta) per layer.  Differentiable
    in the parameters and, with the narrow layer 0, in x0."""

    @staticmethod
    def forward(ctx, x0, meta, *params):
        lib = _lib.load()
        s = meta["structure"]
        bns_mod = meta["batch_norms"]
        training: bool = meta["training"]
        p: float = meta["dropout"] if training else 0.0
        sync_group = meta.get("sync_group")
        L = len(params) // 4
        dev = x0.device
        x0 = x0.contiguous()
        nn_, B = s.num_nodes, s.num_graphs
        grid = lib.cgnn_fused_grid()
        fmeta = s.fused_meta(MAX_ROWS, grid)      # static per batch (cached on the structure)
        # the normalisation itself: every forward -- on a kept batch a batch constant, like the CSR
        dis = s.gcn_dis(fmeta, fresh=_NO_L0_CACHE)
        tiles = _tiles_struct(s, fmeta, dis)
        f32 = dict(dtype=torch.float32, device=dev)
        stat_slab = torch.empty(grid, 128, dtype=torch.float64, device=dev) if training else None
        # [sum(64) | sumsq(64) | rows]: the 129th word carries this rank's row count through the
        # sync-BN all-reduce
        sums = torch.empty(129, dtype=torch.float64, device=dev) if training else None
        ys: List[torch.Tensor] = []
        bns: List[torch.Tensor] = []
        masks: List[Optional[torch.Tensor]] = []
        local_count = count = float(nn_)
        count_dev = None                           # device copy of the global row count (sync-BN)
        narrow0 = _narrow0(L, x0.shape[1])         # layer-0 narrow form (fused_gcn_l0.hip)
        if ctx.needs_input_grad[0] and not narrow0:
            raise RuntimeError("FusedGCNEncode: the input gradient exists for the narrow layer 0 only "
                               "(in_channels <= 8, num_layers >= 2)")
        p0 = l0src = l0keep = None
        sp = _lib.stream_ptr(dev)           # one lookup per pass (torch.cuda.current_stream is ~10 us)
        rng = meta.get("rng_state")       # device uint32 words: set when the step is graph-captured

        def rng_ptr(i: int):
            return None if rng is None or p <= 0 else rng.data_ptr() + 4 * i

        # graph replay: the device dropout words are refreshed once per step -- inside layer 0's
        # BatchNorm finalisation when that is the single-launch form, else by a launch of its own
        rng_in_finalize = rng is not None and p > 0 and training and sync_group is None
        with _lib.device_guard(dev):
            if rng is not None and p > 0 and not rng_in_finalize:
                _lib.call("cgnn_rng_advance", rng, L + 1, stream=sp)
            # per-rank BatchNorm in training: the layer's statistics are finalised by the LAST WORKGROUP of the
            # kernel that produces them (csrc/bn_tail.h) -- no slab, no finalisation launch; with a sync group the
            # sums have to cross the ranks between the two, so the slab protocol stays
            tails = training and sync_group is None and not _NO_TAILS
            for l in range(L):
                w, b, gamma, beta = (t.contiguous() for t in params[4 * l:4 * l + 4])
                y = torch.empty(nn_, HID, **f32) if not (l == 0 and narrow0) else None
                slab, slab_rows = stat_slab, grid
                bn_mod = bns_mod[l]
                bn = torch.empty(4 * HID, **f32)
                tail = None
                if tails and (l > 0 or narrow0):
                    adv = rng_in_finalize and l == 0
                    tail = _tail_fwd(bn_mod, dev, count, gamma, beta, bn, rng if adv else None, L + 1 if adv else 0)
                if l == 0 and narrow0:
                    # layer 0, narrow form: Y0 = (A_hat X0) W0^T + b is NEVER written: only the
                    # narrow aggregate P0 = A_hat X0 (32 B per node) is kept and every consumer
                    # rebuilds the rows of Y0 it needs from it (cgnn_l0src)
                    # ... in CENTRED form when column 7 is spare (F0 <= 7) and the statistics are this
                    # rank's own: P0' = [A_hat (X0 - 1 c^T) | r - rbar], W' = [W0 | W0 c], handed on
                    # without its constant term (mean_offset) -- the same function, evaluated at the
                    # scale of the features' spread rather than of their mean (cgnn_gcn_l0_fwd).
                    # (Under sync-BN the ranks' constants would differ: raw form there.)
                    y = None
                    f0 = int(x0.shape[1])
                    center = _l0_center(s, x0, tiles, sp) if (f0 < 8 and sync_group is None) else None
                    slab_rows = lib.cgnn_l0_grid(nn_)
                    # kept batch: P0 and the per-workgroup moments of its rows are batch constants (aggregated
                    # once, cgnn_gcn_l0_agg); the step only turns the moments into this step's sums
                    # (cgnn_gcn_l0_stats).  Never for a differentiable x0 (a fresh gather per pass).
                    const = None
                    if _kept(s) and not ctx.needs_input_grad[0] and not x0.requires_grad:
                        const = _l0_batch_constants(s, x0, center, tiles, slab_rows, sp)
                    p0 = const[0] if const is not None else torch.empty(nn_, 8, **f32)
                    if center is not None:
                        w_eff, mean_off = torch.empty(HID, f0 + 1, **f32), torch.empty(HID, **f32)
                        l0src = _lib.CgnnL0Src(_lib.ptr(p0), _lib.ptr(w_eff), _lib.ptr(_zeros(dev)), f0 + 1)
                        l0keep = (w_eff, _zeros(dev), center, mean_off)     # the struct holds raw pointers
                    else:
                        w_eff = mean_off = None
                        l0src = _lib.CgnnL0Src(_lib.ptr(p0), _lib.ptr(w), _lib.ptr(b), f0)
                        l0keep = (w, b, None, None)
                    slab = torch.empty(slab_rows, 128, dtype=torch.float64, device=dev) if (training and tail is None) else None
                    if const is not None:
                        _lib.call("cgnn_gcn_l0_stats", const[1], slab_rows, f0, w, b, center, w_eff, mean_off,
                                  *_lib.buf(slab), tail, stream=sp)
                    else:
                        _lib.call("cgnn_gcn_l0_fwd", tiles, x0, f0, w, b, p0, None, *_lib.buf(slab), center, w_eff,
                                  mean_off, tail, stream=sp)
                elif l == 0:
                    _lib.call("cgnn_gcn_fused_fwd_first", tiles, x0, x0.shape[1], w, b, y, *_lib.buf(stat_slab),
                              stream=sp)
                else:
                    mask = torch.empty(nn_ * 16, dtype=torch.uint8, device=dev) if p > 0 else None
                    seed = _lib.next_seed(dev) if p > 0 else 0
                    _lib.call("cgnn_gcn_fused_fwd", tiles, ys[-1], l0src if ys[-1] is None else None, bns[-1], p, seed,
                              rng_ptr(l), mask, w, b, y, None if tail is not None else stat_slab,
                              _lib.nbytes(stat_slab), tail, stream=sp)
                    masks.append(mask)
                cnt = count
                if tail is not None:
                    pass                                   # finalised inside the producing launch
                elif training and sync_group is None:
                    # one launch: reduce partials, finalise, update running stats and the counter
                    adv = rng_in_finalize and l == 0
                    _lib.call("cgnn_bn_stats_finalize_rng", slab, slab_rows, cnt, gamma, beta, bn_mod.running_mean,
                              bn_mod.running_var, float(bn_mod.momentum), float(bn_mod.eps), bn_mod.num_batches_tracked,
                              bn, rng if adv else None, L + 1 if adv else 0,
                              l0keep[3] if (l == 0 and l0keep is not None) else None, stream=sp)
                else:
                    cnt_dev = None
                    if training:
                        _lib.call("cgnn_bn_reduce", slab, slab_rows, 128, sums, stream=sp)
                        sums[128] = local_count
                        _sync_sums(sums, sync_group)
                        cnt_dev = sums.data_ptr() + 128 * 8
                        if count_dev is None:
                            count_dev = sums[128:129].clone()     # global rows, for backward
                        bn_mod.num_batches_tracked.add_(1)
                    _lib.call("cgnn_bn_finalize", sums, cnt, cnt_dev, gamma, beta, bn_mod.running_mean,
                              bn_mod.running_var, float(bn_mod.momentum), float(bn_mod.eps), int(training), bn,
                              l0keep[3] if (l == 0 and l0keep is not None) else None, stream=sp)
                ys.append(y)
                bns.append(bn)
            mask = torch.empty(nn_ * 16, dtype=torch.uint8, device=dev) if p > 0 else None
            seed = _lib.next_seed(dev) if p > 0 else 0
            pooled = torch.empty(B, HID, **f32)
            # per-graph factor sums: the readout backward needs no second pass over Y
            want_grad = ctx.needs_input_grad[0] or any(ctx.needs_input_grad[2:])
            fsum = torch.empty(2, B, HID, **f32) if want_grad else None
            _lib.call("cgnn_gcn_fused_pool_fwd", ys[-1], bns[-1], p, seed, rng_ptr(L), mask, s.gptr, B, pooled, fsum,
                      None if fsum is None else fsum.data_ptr() + 4 * B * HID, stream=sp)
            masks.append(mask)
        c = _Ctx()
        c.s, c.meta, c.dis, c.tiles, c.grid = s, fmeta, dis, tiles, grid
        c.ys, c.bns, c.masks, c.p, c.x0, c.f0, c.p0 = ys, bns, masks, p, x0, x0.shape[1], p0
        c.count, c.sync_group, c.num_layers, c.training = count, sync_group, L, training
        c.count_dev = count_dev
        c.fsum = fsum
        c.l0src, c.l0keep = l0src, l0keep
        c.grad_dst = meta.get("grad_dst") or [None] * (4 * L)
        c.bn_modules = bns_mod
        if meta.get("record") is not None:
            meta["record"]["layers"] = list(masks)
        ctx.c = c
        ctx.save_for_backward(*params)
        return pooled

    @staticmethod
    def backward(ctx, d_pooled):
        lib = _lib.load()
        c: _Ctx = ctx.c
        params = ctx.saved_tensors
        L, grid, s = c.num_layers, c.grid, c.s
        dev = d_pooled.device
        nn_, B = s.num_nodes, s.num_graphs
        f32 = dict(dtype=torch.float32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        sp = _lib.stream_ptr(dev)           # one lookup per pass (torch.cuda.current_stream is ~10 us)
        d_pooled = d_pooled.contiguous()
        s_slab = torch.empty(grid, 128, **f64)
        sums = torch.empty(128, **f64)
        # every layer gets its own slabs: all slab -> dW/db reductions run as ONE launch at the end
        # of the backward (they do not feed the chain)
        jobs = []
        dz = torch.empty(nn_, HID, **f32)
        dz_prev = torch.empty(nn_, HID, **f32) if L > 1 else None
        grads: List[Optional[torch.Tensor]] = [None] * (4 * L)
        dst = c.grad_dst

        def out(i: int, *shape) -> torch.Tensor:
            """where parameter i's gradient is written: its armed .grad view (ops.grad_destination; the
            gradient is then NOT returned to autograd) or a fresh tensor"""
            return dst[i] if dst[i] is not None else torch.empty(*shape, **f32)

        def bn_backward(l: int) -> torch.Tensor:
            """sums of layer l (in s_slab) -> dgamma/dbeta of layer l and its c1|c2 block."""
            direct = c.sync_group is None       # (under sync-BN the parameter gradients are the LOCAL sums)
            dgamma = out(4 * l + 2, HID) if direct else torch.empty(HID, **f32)
            dbeta = out(4 * l + 3, HID) if direct else torch.empty(HID, **f32)
            bwc = torch.empty(2 * HID, **f32)
            if c.sync_group is None:
                _lib.call("cgnn_bn_bwd_stats_finalize", s_slab, grid, c.count, int(not c.training), dgamma, dbeta, bwc,
                          stream=sp)
            else:
                _lib.call("cgnn_bn_reduce", s_slab, grid, 128, sums, stream=sp)
                # parameter gradients are the LOCAL sums (the gradient all-reduce averages them,
                # exactly like torch's SyncBatchNorm); c1|c2 need the sums over all ranks
                local_dbeta, local_dgamma = sums[:HID].float(), sums[HID:].float()
                dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=c.sync_group)
                _lib.call("cgnn_bn_bwd_finalize", sums, c.count, c.count_dev, int(not c.training), dgamma, dbeta, bwc,
                          stream=sp)
                dgamma, dbeta = local_dgamma, local_dbeta
            grads[4 * l + 2], grads[4 * l + 3] = dgamma, dbeta
            return bwc

        # the last layer rebuilds its incoming gradient from dP (POOLIN); the readout backward
        # only supplies the BatchNorm-backward sums (dZ = NULL)
        pool_args = (d_pooled, s.node_graph, s.gptr, c.masks[-1])
        none_args = (None, None, None, None)
        with _lib.device_guard(dev):
            if c.fsum is not None and c.sync_group is None:
                # per-rank BatchNorm: the sums over all graphs and the coefficients in one launch
                dgamma, dbeta, bwc = out(4 * (L - 1) + 2, HID), out(4 * (L - 1) + 3, HID), torch.empty(2 * HID, **f32)
                _lib.call("cgnn_gcn_fused_pool_bwd_finalize", d_pooled, c.fsum, c.fsum.data_ptr() + 4 * B * HID, s.gptr,
                          B, c.count, int(not c.training), dgamma, dbeta, bwc, stream=sp)
                grads[4 * (L - 1) + 2], grads[4 * (L - 1) + 3] = dgamma, dbeta
            else:
                if c.fsum is not None:
                    _lib.call("cgnn_gcn_fused_pool_bwd_sums", d_pooled, c.fsum, c.fsum.data_ptr() + 4 * B * HID, s.gptr,
                              B, *_lib.buf(s_slab), stream=sp)
                else:
                    _lib.call("cgnn_gcn_fused_pool_bwd", d_pooled, c.ys[-1], c.bns[-1], c.p, c.masks[-1], s.gptr, B,
                              None, *_lib.buf(s_slab), stream=sp)
                bwc = bn_backward(L - 1)
            bns_mod = c.bn_modules
            for l in range(L - 1, 0, -1):
                w = params[4 * l].contiguous()
                extra = pool_args if l == L - 1 else none_args
                dw_slab = torch.empty(grid, HID * HID, **f32)
                db_slab = torch.empty(grid, HID, **f64)
                # per-rank BatchNorm: the coefficients of the layer BELOW (its dgamma / dbeta / c1|c2) come out
                # of this launch's tail (csrc/bn_tail.h) instead of a finalisation launch of their own
                tail = nxt = None
                if c.sync_group is None and not _NO_TAILS:
                    nxt = (out(4 * (l - 1) + 2, HID), out(4 * (l - 1) + 3, HID), torch.empty(2 * HID, **f32))
                    tail = _tail_bwd(bns_mod[l - 1], dev, c.count, not c.training, *nxt)
                _lib.call("cgnn_gcn_fused_bwd", c.tiles, dz, c.ys[l], c.bns[l], bwc, c.ys[l - 1],
                          c.l0src if c.ys[l - 1] is None else None, c.bns[l - 1], c.p, c.masks[l - 1], w, dz_prev,
                          None if tail is not None else s_slab, _lib.nbytes(s_slab), *_lib.buf(dw_slab),
                          *_lib.buf(db_slab), *extra, tail, stream=sp)
                dw, db = out(4 * l, HID, HID), out(4 * l + 1, HID)
                jobs.append((dw_slab, db_slab, grid, HID, HID, dw, db))
                grads[4 * l], grads[4 * l + 1] = dw, db
                if nxt is not None:
                    grads[4 * (l - 1) + 2], grads[4 * (l - 1) + 3], bwc = nxt
                else:
                    bwc = bn_backward(l - 1)
                dz, dz_prev = dz_prev, dz
            dw0, db0 = out(0, HID, c.f0), out(1, HID)
            dx0 = None
            if c.p0 is not None:
                # dW0 = dY0^T P0, db0 = sum dY0: streaming, no aggregation (fused_gcn_l0.hip)
                g0 = lib.cgnn_l0_grid(nn_)
                dw_slab0 = torch.empty(g0, HID * 8, **f32)
                db_slab0 = torch.empty(g0, HID, **f64)
                l0_args = (c.l0src, c.bns[0], bwc, c.p0, nn_, *_lib.buf(dw_slab0), *_lib.buf(db_slab0), c.l0keep[2])
                if ctx.needs_input_grad[0]:
                    # ... and the node-feature gradient dX0 = A_hat^T G0 with G0 = dY0 W0 [Nn, 8]: the 64 -> F0
                    # narrowing rides in the same streaming pass, then one narrow transposed aggregate
                    gbuf = torch.empty(nn_, 8, **f32)
                    dx0 = torch.empty(nn_, c.f0, **f32)
                    _lib.call("cgnn_gcn_l0_bwd_dx", dz, *l0_args, *_lib.buf(gbuf), stream=sp)
                    _lib.call("cgnn_gcn_l0_dx", c.tiles, gbuf, c.f0, *_lib.buf(dx0), stream=sp)
                else:
                    _lib.call("cgnn_gcn_l0_bwd", dz, None, *l0_args, stream=sp)
                jobs.append((dw_slab0, db_slab0, g0, 8, c.f0, dw0, db0))
            else:
                extra = pool_args if L == 1 else none_args
                dw_slab = torch.empty(grid, HID * 16, **f32)
                db_slab = torch.empty(grid, HID, **f64)
                _lib.call("cgnn_gcn_fused_bwd_first", c.tiles, dz, c.ys[0], c.bns[0], bwc, c.x0, c.f0,
                          *_lib.buf(dw_slab), *_lib.buf(db_slab), c.p, *extra, stream=sp)
                jobs.append((dw_slab, db_slab, grid, 16, c.f0, dw0, db0))
            grads[0], grads[1] = dw0, db0
            for i0 in range(0, len(jobs), _lib.DW_MAX_JOBS):
                chunk = jobs[i0:i0 + _lib.DW_MAX_JOBS]
                jb = _lib.CgnnDwJobs()
                jb.n = len(chunk)
                for i, (sw, sb, rows, oc, tc, dw_o, db_o) in enumerate(chunk):
                    jb.dw_slab[i], jb.db_slab[i] = sw.data_ptr(), sb.data_ptr()
                    jb.rows[i], jb.out_cols[i], jb.take_cols[i] = rows, oc, tc
                    jb.dW[i], jb.db[i] = dw_o.data_ptr(), db_o.data_ptr()
                _lib.call("cgnn_dw_db_reduce_multi", jb, stream=sp)
        ctx.c = None
        return (dx0, None, *ops.undelivered(grads, dst))


def encode(model, batch, structure) -> torch.Tensor:
    return bn_stage.encode(FusedGCNEncode, model, batch, structure)
