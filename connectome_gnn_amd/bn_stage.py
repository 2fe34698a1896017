"""The BatchNorm(+ReLU)+dropout stage of the one-node encoders (gcn_wide_path.py, sage_path.py,
gcn_half_path.py), and the entry glue they share with fused.py.

  forward, layer l     statistics slab of Y: the producing GEMM's epilogue, else cgnn_bn_act_fwd_stats
                       [a | b | mean | invstd] = BatchNorm coefficients  cgnn_bn_act_finalize (+ all-reduce, sync-BN)
                       dropout keep mask, seed and device RNG word
                       X' = drop(act(a Y + b))                   cgnn_bn_act_fwd_apply; last layer fused with the
                                                                 readout (cgnn_bn_act_pool_fwd, factor sums Fsum)
  backward, layer l    c1|c2, dgamma, dbeta: from Fsum on the last layer, else cgnn_bn_act_bwd_stats + _bwd_finalize
                       dY = BatchNorm'(dX' * drop' * act')       cgnn_bn_act_bwd_apply (+ the column sums of db;
                                                                 every layer's db in one launch at the end)

GCN has its ReLU after the BatchNorm (relu = 1 to apply / pool / bwd_stats, no inner ReLU in bwd_apply);
GraphSAGE has it inside the conv, before (relu = 0, and bwd_apply applies ReLU' of Z).  fp16 storage
runs the ``_f16`` twins of the per-node kernels, which take the same arguments.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist

from . import _lib, ops
from .structure import EDGE_GRAD_REASON, edge_grad_requested, twin_view, unpermute_record

PAD_K = 32           # a narrow layer 0 packed to one 32-wide panel for the weight-stationary GEMMs
PAD_MIN_ROWS = 4096  # (= the row count from which the weight-stationary GEMMs apply)


def f32(dev, *shape):
    return torch.empty(*shape, dtype=torch.float32, device=dev)


def sync_group_of(model):
    """The process group of the model's SyncBatchNorm layers when full-batch statistics across
    ranks are in effect (training, world size > 1), else None."""
    group = None
    for bn in model.batch_norms:
        if isinstance(bn, torch.nn.SyncBatchNorm) and model.training and dist.is_initialized() \
                and dist.get_world_size(bn.process_group) > 1:
            group = bn.process_group if bn.process_group is not None else dist.group.WORLD
    return group


def bn_modules_ok(model) -> bool:
    """Plain affine BatchNorm1d / SyncBatchNorm with running statistics and a fixed momentum."""
    for bn in model.batch_norms:
        if type(bn) not in (torch.nn.BatchNorm1d, torch.nn.SyncBatchNorm) \
                or not (bn.affine and bn.track_running_stats) or bn.momentum is None:
            return False
    return True


def ineligible(batch, structure, model=None, input_grad_ok: bool = False) -> Optional[str]:
    """The reason shared by every one-node encoder's eligible() for not covering (model, batch), or None;
    with `model`, its BatchNorm modules are checked too (bn_modules_ok).  input_grad_ok: the encoder returns
    the gradient of the node features itself (fused.py) -- edge-weight gradients still come first."""
    if batch.node_features.requires_grad and not input_grad_ok:
        return "node_features require grad"
    if edge_grad_requested(structure):
        return EDGE_GRAD_REASON
    if model is not None and not bn_modules_ok(model):
        return "BatchNorm is not a plain affine BatchNorm1d / SyncBatchNorm with running stats"
    return None


def encode(fn, model, batch, structure, half: bool = False) -> torch.Tensor:
    """fn.apply(x0, cfg, *params) with (W, b, gamma, beta) per layer: on the batch's degree-ordered twin
    when one was prepared (structure.twin_view; only the node features enter in the batch's own order),
    with the parameters' armed .grad destinations and the SyncBatchNorm group -- none of the three for
    the fp16-storage path (half=True)."""
    params = []
    for conv, bn in zip(model.convs, model.batch_norms):     # (GCNLayer keeps its bias outside the Linear)
        params += [conv.linear.weight, conv.linear.bias if conv.linear.bias is not None else conv.bias,
                   bn.weight, bn.bias]
    cfg = {"structure": structure, "batch_norms": list(model.batch_norms), "training": model.training,
           "dropout": float(model.dropout), "rng_state": getattr(model, "rng_device_state", None),
           "record": model._dropout_record()}
    if half:
        return fn.apply(batch.node_features, cfg, *params)
    cfg["structure"], x0, twin = twin_view(structure, batch.node_features)
    cfg["sync_group"], cfg["grad_dst"] = sync_group_of(model), ops.claim_destinations(params, model.training)
    out = fn.apply(x0, cfg, *params)
    unpermute_record(twin, cfg["record"])
    return out


def linear_fwd_stats(x1, x2, w, b, grid, relu: bool = True):
    """act([x1 | x2] W^T + b) and the per-workgroup (sum | sum of squares) slab of the result, or
    (None, None) when the shape is outside the weight-stationary kernel."""
    m, k1 = x1.shape
    k2 = 0 if x2 is None else x2.shape[1]
    n = w.shape[0]
    y = torch.empty(m, n, dtype=torch.float32, device=x1.device)
    slab = torch.empty(grid, 2 * n, dtype=torch.float64, device=x1.device)
    rc = _lib.call("cgnn_linear_fwd_stats_f32", x1, x1.stride(0), k1, x2, 0 if x2 is None else x2.stride(0), k2,
                   w, b, int(relu), y, y.stride(0), m, n, *_lib.buf(slab), accept=(_lib.CGNN_EUNSUPPORTED,))
    return (None, None) if rc == _lib.CGNN_EUNSUPPORTED else (y, slab)


class BnStage:
    """The stage of one encoder pass.  The forward builds it layer by layer and keeps what the backward
    needs (Y, coefficient blocks, keep masks, factor sums); the backward reuses it and collects the
    gradients of the biases and BatchNorm parameters in ``grads`` (the path adds the weights')."""

    def __init__(self, cfg, num_layers: int, dev, relu_after_bn: bool, half: bool = False):
        self.lib, self.dev, self.L = _lib.load(), dev, num_layers
        self.s, self.bn_modules = cfg["structure"], cfg["batch_norms"]
        self.training = cfg["training"]
        self.p = cfg["dropout"] if self.training else 0.0
        self.rng = cfg.get("rng_state")          # device words a captured step refreshes per replay
        self.sync_group, self.count_block = cfg.get("sync_group"), None
        self.grad_dst = cfg.get("grad_dst") or [None] * (4 * num_layers)
        self.record = cfg.get("record")
        self.relu, self.sfx = int(relu_after_bn), "_f16" if half else ""
        self.n = self.s.num_nodes
        self.ys, self.coefs, self.masks, self.seeds, self.rws = [], [], [], [], []
        self.fsum = None
        self._begin()
        if self.rng is not None and self.p > 0:
            self._launch("cgnn_rng_advance", self.rng, num_layers + 1)

    def _begin(self):
        self.sp = _lib.stream_ptr(self.dev)      # one lookup per pass (torch.cuda.current_stream is ~10 us)
        self.rows = int(self.lib.cgnn_bn_act_slab_rows(self.n))

    def _launch(self, name, *args):
        _lib.call(name, *args, stream=self.sp)

    # ---- forward

    def forward(self, y, gamma, beta, slab=None) -> None:
        """The next layer's coefficient block and dropout words from its pre-BatchNorm output Y and, when
        the producer left one, the statistics slab of Y (running statistics in eval mode).  With a sync
        group the per-rank sums and row count are all-reduced first (one fp64 block of 2H+1 words; the
        count never returns to the host)."""
        li, n, hid, dev, bn = len(self.ys), self.n, y.shape[1], self.dev, self.bn_modules[len(self.ys)]
        srows = self.rows if slab is None else slab.shape[0]
        if self.training and slab is None:
            slab = torch.empty(self.rows, 2 * hid, dtype=torch.float64, device=dev)
            self._launch("cgnn_bn_act_fwd_stats" + self.sfx, y, n, hid, *_lib.buf(slab))
        coef = f32(dev, 4 * hid)
        count_dev = None
        if self.training and self.sync_group is not None:
            block = torch.empty(2 * hid + 1, dtype=torch.float64, device=dev)
            torch.sum(slab[:srows], dim=0, out=block[:2 * hid])
            block[2 * hid:] = float(n)
            dist.all_reduce(block, op=dist.ReduceOp.SUM, group=self.sync_group)
            slab, srows, count_dev = block, 1, block.data_ptr() + 8 * 2 * hid
            self.count_block = block
        self._launch("cgnn_bn_act_finalize", slab, srows, hid, float(max(n, 1)), count_dev, int(self.training),
                     gamma, beta, bn.running_mean, bn.running_var, float(bn.momentum), float(bn.eps),
                     bn.num_batches_tracked if self.training else None, coef)
        p = self.p
        self.ys.append(y)
        self.coefs.append(coef)
        self.masks.append(torch.empty(n * (hid // 4), dtype=torch.uint8, device=dev) if p > 0 else None)
        self.seeds.append(_lib.next_seed(dev) if p > 0 else 0)
        self.rws.append(None if (self.rng is None or p <= 0) else self.rng.data_ptr() + 4 * li)

    def apply(self, li: int) -> torch.Tensor:
        """X' of layer li (cgnn_bn_act_fwd_apply)."""
        y = self.ys[li]
        x = torch.empty_like(y)
        self._launch("cgnn_bn_act_fwd_apply" + self.sfx, y, self.coefs[li], self.relu, self.p, self.seeds[li],
                     self.rws[li], self.masks[li], x, self.n, y.shape[1])
        return x

    def pool(self, needs_grad: bool) -> torch.Tensor:
        """The last layer: BatchNorm + dropout + mean-pool in one pass, X' never written.  Leaves the
        factor sums for its backward statistics (under sync-BN the sums are exchanged through the slab
        of the ordinary statistics pass instead)."""
        y, s, hid = self.ys[-1], self.s, self.ys[-1].shape[1]
        pooled = f32(self.dev, s.num_graphs, hid)
        self.fsum = f32(self.dev, 2, s.num_graphs, hid) if (self.sync_group is None and needs_grad) else None
        self._launch("cgnn_bn_act_pool_fwd" + self.sfx, y, self.coefs[-1], self.relu, self.p, self.seeds[-1],
                     self.rws[-1], self.masks[-1], s.gptr, s.num_graphs, pooled, hid, self.fsum)
        if self.record is not None:
            self.record["layers"] = list(self.masks)
        return pooled

    # ---- backward

    def begin_backward(self, dP) -> None:
        self._begin()
        self.dP = dP
        self.grads = [None] * (4 * self.L)
        self.deferred = _lib.DeferredReduce()

    def bwd_coefs(self, li: int, dx) -> torch.Tensor:
        """c1|c2 of layer li (dgamma, dbeta to ``grads``) from the incoming gradient dX' (None on the last
        layer: rebuilt from dP inside the kernels).  The last layer takes the factor sums its pooled
        forward pass left: the readout's gradient is constant per graph, so no pass over Y is needed.
        With a sync group the sums are all-reduced for c1|c2 while dgamma/dbeta stay the rank-local sums
        (the gradient all-reduce averages them), exactly like torch's SyncBatchNorm."""
        y, coef, s, n, dev = self.ys[li], self.coefs[li], self.s, self.n, self.dev
        hid = y.shape[1]
        direct = self.sync_group is None or self.count_block is None   # (armed .grad views, ops.grad_destination)
        dgamma, dbeta = (d if (direct and d is not None) else f32(dev, hid)
                         for d in self.grad_dst[4 * li + 2:4 * li + 4])
        bwc = f32(dev, 2 * hid)
        if li == self.L - 1 and self.fsum is not None:
            self._launch("cgnn_bn_act_pool_bwd_finalize", self.dP, self.fsum, s.gptr, s.num_graphs, hid,
                         float(max(n, 1)), int(not self.training), dgamma, dbeta, bwc)
        else:
            slab = torch.empty(self.rows, 2 * hid, dtype=torch.float64, device=dev)
            self._launch("cgnn_bn_act_bwd_stats" + self.sfx, dx, y, self.masks[li], coef, self.relu, self.p, n, hid,
                         *_lib.buf(slab), *self._pool(li))
            if direct:
                self._launch("cgnn_bn_act_bwd_finalize", slab, self.rows, hid, float(max(n, 1)), None,
                             int(not self.training), dgamma, dbeta, bwc)
            else:
                sums = torch.sum(slab, dim=0)                          # fp64 [2H] = sum dZ | sum dZ*xhat
                local_dbeta, local_dgamma = sums[:hid].float(), sums[hid:].float()
                dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=self.sync_group)
                self._launch("cgnn_bn_act_bwd_finalize", sums, 1, hid, 0.0, self.count_block.data_ptr() + 8 * 2 * hid,
                             int(not self.training), dgamma, dbeta, bwc)
                dgamma, dbeta = local_dgamma, local_dbeta
        self.grads[4 * li + 2], self.grads[4 * li + 3] = dgamma, dbeta
        return bwc

    def bwd_apply(self, li: int, dx, bwc) -> torch.Tensor:
        """dY of layer li (cgnn_bn_act_bwd_apply), its column sums queued for db."""
        y, n = self.ys[li], self.n
        hid = y.shape[1]
        cs_rows = int(self.lib.cgnn_bn_act_apply_blocks(n, hid))
        cs_slab = torch.empty(cs_rows, hid, dtype=torch.float64, device=self.dev)
        dy = torch.empty_like(y)
        self._launch("cgnn_bn_act_bwd_apply" + self.sfx, dx, y, self.masks[li], self.coefs[li], bwc, self.relu, self.p,
                     1 - self.relu, *_lib.buf(cs_slab), dy, n, hid, *self._pool(li))
        self.add_db(li, cs_slab, cs_rows)
        return dy

    def backward(self, li: int, dx) -> torch.Tensor:
        """BatchNorm + dropout backward of layer li and its db, in two passes: dY."""
        return self.bwd_apply(li, dx, self.bwd_coefs(li, dx))

    def _pool(self, li: int):
        return (self.dP, self.s.node_graph, self.s.gptr) if li == self.L - 1 else (None, None, None)

    def add_db(self, li: int, cs_slab, rows: int) -> None:
        """db of layer li from a slab of its column sums: all layers' in one launch at the end (finish)."""
        d = self.grad_dst[4 * li + 1]
        self.grads[4 * li + 1] = d if d is not None else f32(self.dev, cs_slab.shape[1])
        self.deferred.add(cs_slab, rows, cs_slab.shape[1], self.grads[4 * li + 1])

    def dw(self, li: int, w) -> torch.Tensor:
        """Where layer li's weight gradient is written: its armed .grad view, else a new array like W."""
        d = self.grad_dst[4 * li]
        self.grads[4 * li] = d if d is not None else torch.empty_like(w)
        return self.grads[4 * li]

    def finish(self):
        """The deferred db reductions; then what the backward returns to autograd for the parameters."""
        self.deferred.flush(self.sp)
        return ops.undelivered(self.grads, self.grad_dst)
