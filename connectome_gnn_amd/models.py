"""GCN / GraphSAGE connectome classifiers on the MI355X message-passing kernels.

Drop-in for the reference's model API (connectome_gnn/models.py:159-266): same class names,
constructor signatures, attributes (``convs``, ``batch_norms``, ``classifier``, ``dropout``),
``encode``/``forward``, identical ``state_dict`` keys/shapes and -- because parameters are
created in the same order with the same initialisers -- identical initial weights under
``torch.manual_seed``.

What differs is how a layer is evaluated.  The reference issues ~13 ATen ops per GCN layer on
an int64 COO and materialises [E+N, F] message tensors (models.py:90-114).  Here a batch is
bucket-sorted once into CSR (structure.py) and a layer is
    projection   : fp32 MFMA GEMM                     (cgnn_linear_*)
    aggregation  : atomics-free segment reduction      (cgnn_aggregate_f32)
    readout      : contiguous segment mean             (cgnn_pool_mean_*)
all hand-written HIP for gfx950, reached through the C ABI in include/cgnn.h.  BatchNorm,
ReLU, dropout, the 2-layer classifier head and the loss stay PyTorch-ROCm host code in this
execution path (``impl="layered"``); the fused per-graph path replaces them as well.

There is no CPU path: CPU tensors raise (the oracle under oracle/ is test infrastructure).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, encoder_choice, fused, gcn_half_path, ops
from .graph import ConnectomeBatch
from .structure import BatchStructure, GcnNorm, SageNorm, _require_device


_TILE_ROWS = 384


def _grid() -> int:
    return int(_lib.load().cgnn_fused_grid())


class _AdHocBatch:
    """Lets a layer be called with raw (x, edge_index, edge_weight) like the reference's
    GCNLayer/SAGELayer (models.py:84-89,136-141): one graph, no batch vector."""

    def __init__(self, x, edge_index, edge_weight):
        n = x.shape[0]
        self.edge_index, self.edge_weight = edge_index, edge_weight
        self.batch = None
        self.ptr = torch.tensor([0, n], dtype=torch.long, device=x.device)
        self.num_nodes, self.num_graphs = n, 1


class GCNLayer(nn.Module):
    """Y = (D^-1/2 (A + I) D^-1/2)^T X W^T + b with source-side weighted degree
    (reference models.py:66-114).  Parameters: ``linear.weight [out,in]``, ``bias [out]``."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.linear = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))
        nn.init.xavier_uniform_(self.linear.weight)

    def forward(self, x, edge_index, edge_weight, *, structure: Optional[BatchStructure] = None,
                norm: Optional[GcnNorm] = None):
        _require_device(x, "x")
        if structure is None:
            structure = BatchStructure.build(_AdHocBatch(x, edge_index, edge_weight))
        if norm is None:
            norm = structure.gcn_norm()
        s = structure
        bf, bb = s.band_ops("gcn", norm) if s.has_csr else (None, None)
        fwd = (s.rowptr_dst, s.col_dst, norm.coef_dst, norm.selfc, None, bf)
        bwd = (s.rowptr_src, s.col_src, norm.coef_src, bb)
        # edge_weight.requires_grad: every aggregate also returns its dL/dw (ops.edge_weight_grad)
        eg = dict(edge_weight=edge_weight, edge_grad=("gcn", s, norm)) if ops.edge_grad_wanted(edge_weight) else {}
        w = self.linear.weight
        if w.shape[1] < w.shape[0]:
            # A_hat (X W^T) == (A_hat X) W^T: aggregate at the narrower width first
            return ops.linear(ops.aggregate(x, None, fwd, bwd, **eg), None, w, self.bias)
        t = ops.linear(x, None, w, None)
        if s.tiled_ok(t.shape[1]):
            # wide features: LDS-staged tiles, dis * (A_w + I)(dis * T) with the self-loop in the ELL
            meta = s.fused_meta(_TILE_ROWS, _grid(), 1.0)
            return ops.aggregate_tiled(t, self.bias, s, meta, pre=norm.dis, post=norm.dis, **eg)
        return ops.aggregate(t, self.bias, fwd, bwd, **eg)


class SAGELayer(nn.Module):
    """relu(Linear([x || weighted-mean of in-neighbours])) (reference models.py:121-152)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.linear = nn.Linear(in_channels * 2, out_channels)
        nn.init.xavier_uniform_(self.linear.weight)

    def forward(self, x, edge_index, edge_weight, *, structure: Optional[BatchStructure] = None,
                norm: Optional[SageNorm] = None):
        _require_device(x, "x")
        if structure is None:
            structure = BatchStructure.build(_AdHocBatch(x, edge_index, edge_weight))
        if norm is None:
            norm = structure.sage_norm()
        s = structure
        eg = dict(edge_weight=edge_weight, edge_grad=("sage", s, norm)) if ops.edge_grad_wanted(edge_weight) else {}
        if s.tiled_ok(x.shape[1]):
            # wide features: LDS-staged tiles, (A_w X) / (wsum + 1e-8), no self-loop
            meta = s.fused_meta(_TILE_ROWS, _grid(), 0.0)
            agg = ops.aggregate_tiled(x, None, s, meta, post=norm.den, post_div=True, **eg)
        else:
            bf, bb = s.band_ops("sage", norm) if s.has_csr else (None, None)
            agg = ops.aggregate(x, None, (s.rowptr_dst, s.col_dst, norm.w_dst, None, norm.den, bf),
                                (s.rowptr_src, s.col_src, norm.coef_src_bwd, bb), **eg)
        # the [x || agg] concat is never materialised: two K-panels of one GEMM, ReLU epilogue
        return ops.linear(x, agg, self.linear.weight, self.linear.bias, relu=True)


def _head(hidden_dim: int, num_classes: int, dropout: float) -> nn.Sequential:
    return nn.Sequential(nn.Linear(hidden_dim, hidden_dim // 2), nn.ReLU(), nn.Dropout(dropout),
                         nn.Linear(hidden_dim // 2, num_classes))


class _ConnectomeModel(nn.Module):
    _layer_cls = None
    _relu_after_bn = False
    _family = None                    # "gcn" | "sage": whose encoders (encoder_choice.py) and ELL

    def __init__(self, in_channels: int, hidden_dim: int = 64, num_classes: int = 2,
                 num_layers: int = 3, dropout: float = 0.3, *, impl: str = "auto", storage: str = "fp32"):
        super().__init__()
        if impl not in ("auto", "fused", "layered"):
            raise ValueError("impl must be 'auto', 'fused' or 'layered'")
        if storage not in ("fp32", "fp16"):
            raise ValueError("storage must be 'fp32' (the reference's arithmetic) or 'fp16'")
        self.dropout = dropout
        self.impl = impl              # execution path; not part of the reference API/state_dict
        # "fp16": activations cross HBM as IEEE half, fp32 accumulate (GCN, large dense graphs:
        # gcn_half_path.py); parameters, gradients and the state_dict stay fp32
        self.storage = storage
        if storage == "fp16" and not self._relu_after_bn:
            raise ValueError("storage='fp16' is implemented for GCNConnectome only")
        if storage == "fp16" and in_channels < 2:
            # measured: with ONE input feature layer 0 is rank one, every channel of its
            # BatchNorm output is the same signal up to sign, and half-rounded activations put up to 10 % on the
            # classifier's weight gradient (fp32 storage: 1e-6 on the same inputs)
            raise ValueError("storage='fp16' needs at least 2 input features (a rank-one layer 0 loses the "
                             "classifier gradient to half rounding); use storage='fp32'")
        self.impl_used = None
        self.rng_device_state = None  # uint32 device words for graph-captured dropout (graphed.py)
        # parity hook: when True, every training forward leaves the dropout keep decisions it drew
        # in ``last_dropout`` ({"layers": [uint8 keep bits per layer], "head_factor": [B,H/2]}), so a
        # test can replay the same masks through the CPU oracle (tests/test_gpu_models.py)
        self.record_dropout = False
        self.last_dropout = None
        widths = [in_channels] + [hidden_dim] * num_layers
        self.convs = nn.ModuleList(self._layer_cls(a, b) for a, b in zip(widths, widths[1:]))
        self.batch_norms = nn.ModuleList(nn.BatchNorm1d(hidden_dim) for _ in range(num_layers))
        self.classifier = _head(hidden_dim, num_classes, dropout)

    def _norm(self, structure):
        return structure.gcn_norm() if self._family == "gcn" else structure.sage_norm()

    def _rng_word(self, i: int) -> Optional[int]:
        """Address of a captured step's dropout word `i` (the layers', then the classifier's); None when eager."""
        rng = self.rng_device_state
        return None if rng is None else rng.data_ptr() + 4 * i

    def _dropout_record(self):
        """Fresh record dict for this forward when ``record_dropout`` is on, else None."""
        if not (self.record_dropout and self.training and self.dropout > 0):
            return None
        if self.last_dropout is None or "layers" in self.last_dropout:
            self.last_dropout = {}
        return self.last_dropout

    def _validate(self, batch: ConnectomeBatch) -> None:
        """The fused encoders hand raw device pointers to the kernels, so what the reference's
        F.linear would reject (models.py:111,151: fp16/fp64 tensors, a feature width that is not
        in_channels) is rejected here, before any path is chosen."""
        x = batch.node_features
        _require_device(x, "batch.node_features")
        if x.dtype != torch.float32:
            raise TypeError(f"batch.node_features must be float32 (the reference is fp32-only), got {x.dtype}")
        for name, prm in self.named_parameters():
            if prm.dtype != torch.float32:
                raise TypeError(f"parameter {name} must be float32, got {prm.dtype}")
            if not prm.is_cuda:
                _require_device(prm, f"parameter {name}")
        fin = self.convs[0].linear.weight.shape[1] // (1 if self._relu_after_bn else 2)
        if x.dim() != 2 or x.shape[1] != fin:
            raise ValueError(f"batch.node_features must be [num_nodes, {fin}] (in_channels), got "
                             f"{tuple(x.shape)}")

    def encode(self, batch: ConnectomeBatch) -> torch.Tensor:
        """Graph embeddings [B, hidden] (reference models.py:203-211 / 256-262)."""
        self._validate(batch)
        s = batch.structure()
        choice = encoder_choice.agreed(self, batch, s, encoder_choice.choose(self, batch, s))
        # the records of what ran: written here only, read back by nothing in the package
        self.impl_used = "layered" if choice.kind is None else "fused"
        if choice.record is not None:
            self._fused_kind = choice.record
        if choice.kind is not None:
            return encoder_choice.ENCODERS[choice.kind].encode(self, batch, s)
        norm = self._norm(s)                  # once per forward pass, shared by all layers
        x = batch.node_features
        rng = self.rng_device_state           # set by graphed.GraphedTrainStep
        if rng is not None and self.training and self.dropout > 0:
            _lib.call("cgnn_rng_advance", rng, len(self.convs) + 1)
        rec = self._dropout_record()
        for li, (conv, bn) in enumerate(zip(self.convs, self.batch_norms)):
            x = conv(x, batch.edge_index, batch.edge_weight, structure=s, norm=norm)
            if ops.bn_act_drop_supported(bn, x.shape[1]):
                # BatchNorm (+ReLU) + dropout in two streaming HIP passes each way
                x = ops.bn_act_drop(x, bn, self._relu_after_bn, self.dropout, self.training,
                                    self._rng_word(li), rec)
            else:                     # SyncBatchNorm / odd widths: torch ops
                x = F.relu(bn(x)) if self._relu_after_bn else bn(x)
                x = F.dropout(x, p=self.dropout, training=self.training)
        return ops.pool_mean(x, s.gptr, batch.num_graphs)

    def forward_loss(self, batch: ConnectomeBatch):
        """(logits, mean cross-entropy against batch.labels) with the classifier, the loss and their
        backward in ONE launch (ops.head_loss) -- the Trainer's step, reference train.py:48-50 -- or None
        when the head is not one of that kernel's shapes or the model is not training on a GPU batch."""
        if not (self.training and batch.node_features.is_cuda and batch.labels is not None
                and ops.head_loss_supported(self.classifier)):
            return None
        pooled = self.encode(batch)
        rec = self.last_dropout if self.record_dropout else None
        return ops.head_loss(self.classifier, pooled, batch.labels, True, self._rng_word(len(self.convs)), rec)

    def forward(self, batch: ConnectomeBatch) -> torch.Tensor:
        """Class logits [B, num_classes]."""
        pooled = self.encode(batch)
        if ops.head_supported(self.classifier):
            # Linear -> ReLU -> Dropout -> Linear on [B, hidden] in one HIP kernel each way
            rec = self.last_dropout if (self.record_dropout and self.training) else None
            return ops.head(self.classifier, pooled, self.training, self._rng_word(len(self.convs)), rec)
        if self.record_dropout and self.training and self.last_dropout is not None \
                and self.dropout > 0 and len(self.classifier) == 4:
            # parity hook for heads outside head.hip's widths (torch modules): same record format
            l1, act, drop, l2 = self.classifier
            h = act(l1(pooled))
            y = drop(h)
            self.last_dropout["head_factor"] = ((y != 0) & (h > 0)).float() / (1.0 - drop.p)
            return l2(y)
        return self.classifier(pooled)

    def prepare_batch(self, batch: ConnectomeBatch, reuse: bool = False) -> None:
        """Build every piece of static per-batch metadata this model will use (CSR, and the
        blocked-ELL of the fused path) now -- these builds read sizes back to the host, so they
        must not happen inside a HIP-graph capture or a timed region.  reuse=True says the batch
        will be trained on repeatedly (cached batches, captured steps): structure work that only
        pays when amortised is then done too -- the one-node encoders over LDS tiles run on the batch's
        degree-ordered twin (structure.degree_ordered_twin: 19 % -> 3 % of blocked-ELL padding on small-world
        connectomes) and the per-tile GCN path keeps its per-batch constants (fused.keep_batch)."""
        s = batch.structure()
        hid = self.convs[-1].linear.weight.shape[0]
        self_loop = 1.0 if self._family == "gcn" else 0.0      # GCN's ELL carries it, GraphSAGE's does not
        # (fp16 storage: no twin, nothing kept; whether it covers the batch is encode's to say)
        kind = None if self.storage == "fp16" else encoder_choice.choose(self, batch, s).kind
        if reuse:
            # (no twin under cross-rank BatchNorm, where the ranks agree on paths, or for cached structures)
            if kind is not None and s.has_csr and s.tiled_ok(hid) \
                    and not any(isinstance(bn, nn.SyncBatchNorm) for bn in self.batch_norms):
                s.degree_ordered_twin().fused_meta(_TILE_ROWS, _grid(), self_loop)
            twin = s._degree_twin
            if twin is not None:                            # the encoder runs on the twin's metadata
                xt = twin.permuted_features(batch.node_features)
                if kind == "tile":
                    fused.keep_batch(self, twin, xt)
                return
        if self.storage == "fp16":
            gcn_half_path.dense_operators(s)
            return
        if s.tiled_ok(hid):
            s.fused_meta(_TILE_ROWS, _grid(), self_loop)
        elif s.has_csr:
            # large graphs: the dense fragments of the operator as matrix-core operands (band_aggregate.hip)
            s.band_ops(self._family, self._norm(s))
        if reuse and kind == "tile":
            fused.keep_batch(self, s, batch.node_features)


class GCNConnectome(_ConnectomeModel):
    """conv -> BatchNorm1d -> ReLU -> dropout per layer, mean-pool, MLP head
    (reference models.py:159-216)."""
    _layer_cls = GCNLayer
    _relu_after_bn = True
    _family = "gcn"


class GraphSAGEConnectome(_ConnectomeModel):
    """conv (ReLU inside) -> BatchNorm1d -> dropout per layer -- no ReLU after BN
    (reference models.py:219-266)."""
    _layer_cls = SAGELayer
    _family = "sage"
