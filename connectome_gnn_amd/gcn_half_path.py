"""GCN encoder with fp16-STORAGE activations for large dense parcellations (BASELINE config 5:
1000-ROI graphs at 10 % density, hidden 256) -- one autograd node, host orchestration only.

The reference has no fp16 path (models.py:46,97,103,147 hard-code fp32; ``.half()`` raises), so
this is new: every [Nn, H] array that crosses HBM is IEEE half, every accumulation is fp32 (fp64 for
the BatchNorm statistics), parameters and their gradients stay fp32.  Selected with
``GCNConnectome(..., storage="fp16")``; validated against the fp32 oracle at fp16 resolution.

At ~100 neighbours per node the per-edge forms of the aggregation are bound by vector/LDS work
per edge, so the operator is applied DENSE, per graph, on the fp16 matrix cores:

  once per batch    Mf, Mb = dense D^-1/2 (A + I) D^-1/2 of every graph and its transpose, half,
                    MFMA-fragment-major                         cgnn_dense_adj_f16 (static, cached)
  layer 0           P0 = Mf X0 on a 64-column half panel (narrow: a quarter of a 256-wide pass),
                    Y0 = P0 W0^T + b0
  layer l > 0       T = X W^T                       cgnn_linear_fwd_f16 (weight-stationary, fp32 accumulate)
                    Y = Mf T + b                    cgnn_dense_aggregate_f16 (v_mfma_f32_32x32x16_f16)
  every layer       X' = dropout(relu(BatchNorm(Y)))            cgnn_bn_act_*_f16 (two passes, bn_stage.py)
  readout           fused into the last BatchNorm pass
  backward          dY = BatchNorm'(...) (two passes, db = column sums), dT = Mb dY,
                    dW = dT^T X (cgnn_linear_bwd_weight_f16: LDS transposing reads, fp32 partials
                    per run of rows), dX = dT W (cgnn_linear_bwd_input_f16);
                    layer 0: dW0 = dY0^T P0, no aggregation

Every product is a hand-written kernel of csrc/gemm_h16.hip (v_mfma_f32_32x32x16_f16, weights
converted fp32 -> half inside the kernels): nothing on this path goes to a GEMM library.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops
from .bn_stage import BnStage, bn_modules_ok, encode as _encode, ineligible
from .structure import BatchStructure

MAX_NODES = 1024          # dense pitch limit of cgnn_dense_adj_f16


def eligible(model, batch, structure: BatchStructure) -> Optional[str]:
    hid = model.convs[0].linear.weight.shape[0]
    if hid not in (64, 128, 256):
        return "hidden_dim is not 64, 128 or 256 (the half projections of gemm_h16.hip)"
    if not structure.block_diagonal:
        return "edges cross graph boundaries"
    if structure.max_nodes_per_graph > MAX_NODES:
        return f"a graph has more than {MAX_NODES} nodes"
    why = ineligible(batch, structure)
    if why is not None:
        return why
    if model.convs[0].linear.weight.shape[1] > P0_COLS:
        return f"more than {P0_COLS} input features"
    if not bn_modules_ok(model) or any(isinstance(bn, torch.nn.SyncBatchNorm) for bn in model.batch_norms):
        return "BatchNorm is not a plain affine BatchNorm1d with running stats"
    return None


def _agg(s, m, x, bias=None, stat_slab=None):
    if isinstance(m, ops.DensePack):
        return ops.dense_aggregate_c16_raw(s, m, x, bias, stat_slab)
    return ops.dense_aggregate_f16_raw(s, m, x, bias, stat_slab)


PACK_BELOW = 0.6       # use the per-fragment operator when it is at most this fraction of the dense bytes


def _operator(s: BatchStructure, coef, selfc, transposed: bool):
    """The dense operator of one ordering in the smaller of its two forms: per MFMA fragment
    (ops.DensePack: nearly full fragments dense, the others as entry lists) when that is clearly
    smaller -- the aggregate is bound by the operator's bytes, which come from HBM on each of
    the five launches of a step -- else the plain dense [B, P, P] half matrix."""
    pk = ops.dense_pack_f16(s, coef, selfc, transposed)
    pitch = pk.pitch
    if pk.nbytes() <= PACK_BELOW * (2.0 * s.num_graphs * pitch * pitch):
        return pk
    return ops.dense_adj_f16(s, coef, selfc, transposed)


def dense_operators(s: BatchStructure):
    """(Mf, Mb): normalised operator and its transpose, built once per batch structure."""
    if s._dense_f16 is None:
        norm = s.gcn_norm()
        s._dense_f16 = (_operator(s, norm.coef_dst, norm.selfc, False), _operator(s, norm.coef_src, norm.selfc, True))
    return s._dense_f16


P0_COLS = 64             # layer 0's input features ride in one 64-column half panel


class _Saved:
    __slots__ = ("s", "mb", "xs", "ws", "p0", "bn")


class GcnHalfEncode(torch.autograd.Function):
    """P[B,H] = mean-pool(GCN stack(x0)), activations stored as half."""

    @staticmethod
    def forward(ctx, x0, cfg, *params):
        lib = _lib.load()
        s: BatchStructure = cfg["structure"]
        L = len(params) // 4
        dev = x0.device
        mf, mb = dense_operators(s)
        sv = _Saved()
        sv.s, sv.mb = s, mb
        sv.xs, sv.ws = [], []
        x = None
        with _lib.device_guard(dev):
            sv.bn = bn = BnStage(cfg, L, dev, relu_after_bn=True, half=True)
            for li in range(L):
                w, b, gamma, beta = (t.contiguous() for t in params[4 * li:4 * li + 4])
                hid = w.shape[0]
                slab = None
                if li == 0:
                    # A_hat (X0 W0^T) == (A_hat X0) W0^T: aggregate the few input columns (one
                    # 64-column half panel through the dense operator), then project
                    sv.p0 = _agg(s, mf, ops.pad_cast_f16(x0, P0_COLS))    # [Nn, 64] half, cols >= F0 zero
                    y = None
                    if bn.training:                                        # statistics in the epilogue
                        y, slab = ops.linear_fwd_stats_f16_raw(sv.p0, w, b, int(lib.cgnn_fused_grid()))
                    if y is None:
                        y = ops.linear_fwd_f16_raw(sv.p0, w, b)           # K = 64 panel, W0 [H, F0]
                else:
                    t = ops.linear_fwd_f16_raw(x, w)                       # half in / out, fp32 accumulate
                    if bn.training:                                        # statistics in the epilogue
                        slab = torch.empty(int(lib.cgnn_fused_grid()), 2 * hid, dtype=torch.float64, device=dev)
                    y = _agg(s, mf, t, b, slab)
                bn.forward(y, gamma, beta, slab)
                sv.xs.append(x); sv.ws.append(w)
                if li < L - 1:
                    x = bn.apply(li)
            # readout fused into the last BatchNorm pass; its per-graph factor sums: the backward
            # statistics of this layer need no pass over Y
            pooled = bn.pool(any(ctx.needs_input_grad))
        ctx.sv = sv
        return pooled

    @staticmethod
    def backward(ctx, dP):
        sv: _Saved = ctx.sv
        s, bn = sv.s, sv.bn
        dev = dP.device
        dP = dP.contiguous()
        with _lib.device_guard(dev):
            bn.begin_backward(dP)
            dx = None                           # last layer: gradient rebuilt from dP inside the kernels
            for li in range(bn.L - 1, -1, -1):
                x, w = sv.xs[li], sv.ws[li]
                bwc = bn.bwd_coefs(li, dx)
                if li > 0 and isinstance(sv.mb, ops.DensePack):
                    # dT = A_hat^T dY with dY formed while the aggregate stages its slices: no apply
                    # pass, dY is never written (db from the per-graph column sums it leaves)
                    dt, cs_slab = ops.dense_aggregate_c16_bnbwd_raw(
                        s, sv.mb, dx, dP if li == bn.L - 1 else None, bn.ys[li], bn.masks[li], bn.coefs[li], bwc,
                        True, bn.p)
                    bn.add_db(li, cs_slab, s.num_graphs)
                    dy = None
                else:
                    dy = bn.bwd_apply(li, dx, bwc)
                    dt = None
                if li == 0:
                    # Y0 = (A_hat X0) W0^T + b0: dW0 = dY0^T P0, no aggregation in the backward
                    bn.grads[0] = ops.linear_bwd_weight_f16_raw(dy, sv.p0, w.shape[1])
                    break
                if dt is None:
                    dt = _agg(s, sv.mb, dy)         # dT = A_hat^T dY
                bn.grads[4 * li] = ops.linear_bwd_weight_f16_raw(dt, x)
                dx = ops.linear_bwd_input_f16_raw(dt, w)                   # dX = dT W
            grads = bn.finish()
        ctx.sv = None
        return (None, None, *grads)


def encode(model, batch, structure: BatchStructure) -> torch.Tensor:
    return _encode(GcnHalfEncode, model, batch, structure, half=True)
