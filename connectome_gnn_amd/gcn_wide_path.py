"""GCN encoder as one autograd node for hidden = 128, 256, ... (hidden 64 has the per-tile fused
kernels of fused.py): host orchestration, the GCN counterpart of sage_path.py.

GCNConnectome.encode (reference models.py:203-211) with hand-written backward, so that every pass
over a node array is one HIP kernel doing several things at once:

  forward, layer 0     P0 = A_hat X0 (narrow)                   cgnn_aggregate_f32
                       Y0 = P0 W0^T + b (+ BatchNorm statistics) cgnn_linear_fwd_stats_f32 (packed K=32)
  forward, layer l>0   T  = X W^T                                cgnn_linear_fwd_f32 (W in LDS)
                       Y  = dis * (A_w + I)(dis * T) + b         cgnn_aggregate_tiled_f32 (LDS tiles); graphs of
                                                                 more than 384 nodes: cgnn_aggregate_f32 (CSR
                                                                 gather) + cgnn_band_aggregate_f32 (dense
                                                                 fragments as split-bf16 MFMA products)
  every layer          X' = dropout(relu(BatchNorm(Y)))          cgnn_bn_act_* (bn_stage.py); last layer
                                                                 fused with the readout
  backward, layer l    dY = BatchNorm'(dX' * drop' * relu'), db = colsum(dY)   cgnn_bn_act_bwd_*
                       dT = dis * (A_w + I)^T (dis * dY)         cgnn_aggregate_tiled_f32 (transposed)
                       dW = dT^T X ; dX = dT W                   cgnn_linear_bwd_weight/input_f32
  backward, layer 0    dW0 = dY0^T P0                            cgnn_linear_bwd_weight_f32 (packed)

No arithmetic of the path happens in torch here; torch allocates buffers and orders the launches.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops
from .bn_stage import PAD_K, PAD_MIN_ROWS, BnStage, encode as _encode, f32, ineligible, linear_fwd_stats
from .structure import TILED_MAX_ROWS


def widths_ineligible(model) -> Optional[str]:
    """The part of eligible() that the layer widths decide."""
    hid, fin = model.convs[0].linear.weight.shape
    if hid % 64 or not bool(_lib.load().cgnn_bn_act_width_ok(hid)):
        return "hidden_dim is not 64, 128, 256, ..."
    if fin >= hid:
        return "input features are not narrower than hidden_dim"
    return None


def eligible(model, batch, structure) -> Optional[str]:
    """None if this path covers (model, batch); else the reason it does not."""
    why = widths_ineligible(model)
    if why is None and not structure.has_csr and not structure.tiled_ok(model.convs[0].linear.weight.shape[0]):
        why = "graphs do not fit an LDS tile and the structure has no CSR form"
    return why or ineligible(batch, structure, model)


class _Saved:
    __slots__ = ("s", "ell", "norm", "xs", "ws", "p0", "padded", "tiled", "band", "bn")


class GcnWideEncode(torch.autograd.Function):
    """P[B,H] = mean-pool(GCN stack(x0)); args = x0, cfg, then (W, b, gamma, beta) per layer."""

    @staticmethod
    def forward(ctx, x0, cfg, *params):
        lib = _lib.load()
        s = cfg["structure"]
        L = len(params) // 4
        dev = x0.device
        x = x0.contiguous()
        n_nodes = s.num_nodes
        grid = int(lib.cgnn_fused_grid())
        sv = _Saved()
        sv.s = s
        sv.norm = nrm = s.gcn_norm()
        sv.tiled = s.tiled_ok(params[0].shape[0])
        # graphs of <= 384 nodes: LDS tiles over the blocked-ELL (with the self-loop entry); larger ones:
        # the CSR gather kernel, its dense fragments on the matrix cores where the batch has them
        sv.ell = s.fused_meta(TILED_MAX_ROWS, grid, 1.0) if sv.tiled else None
        sv.band = (None, None) if sv.tiled else s.band_ops("gcn", nrm)
        sv.xs, sv.ws = [], []
        sv.p0, sv.padded = None, False
        with _lib.device_guard(dev):
            sv.bn = bn = BnStage(cfg, L, dev, relu_after_bn=True)
            for li in range(L):
                w, b, gamma, beta = (t.contiguous() for t in params[4 * li:4 * li + 4])
                hid, fin = w.shape[0], x.shape[1]
                slab, y = None, None
                if li == 0:
                    # narrow input: aggregate first (A_hat (X W^T) == (A_hat X) W^T, models.py:111-114)
                    pad = fin <= PAD_K and hid in (64, 128, 256) and n_nodes >= PAD_MIN_ROWS
                    width = PAD_K if pad else fin
                    p0 = torch.zeros(n_nodes, width, dtype=torch.float32, device=dev) if pad \
                        else f32(dev, n_nodes, fin)
                    ops.aggregate_raw(s.rowptr_dst, s.col_dst, nrm.coef_dst, nrm.selfc, None, None, x,
                                      out=p0[:, :fin])
                    wq = w
                    if pad:
                        wq = torch.zeros(hid, PAD_K, dtype=torch.float32, device=dev)
                        wq[:, :fin].copy_(w)
                    if bn.training:
                        y, slab = linear_fwd_stats(p0, None, wq, b, grid, relu=False)
                    if y is None:
                        y = ops.linear_fwd_raw(p0, None, wq, b, False)
                    sv.p0, sv.padded = p0, pad
                else:
                    t = ops.linear_fwd_raw(x, None, w, None, False)
                    if sv.tiled:
                        y = ops.aggregate_tiled_raw(s, sv.ell, 0, t, nrm.dis, nrm.dis, b)
                    else:
                        y = ops.aggregate_raw(s.rowptr_dst, s.col_dst, nrm.coef_dst, nrm.selfc, None, b, t,
                                              band=sv.band[0])
                bn.forward(y, gamma, beta, slab)
                sv.xs.append(x); sv.ws.append(w)
                if li < L - 1:
                    x = bn.apply(li)
            pooled = bn.pool(any(ctx.needs_input_grad))
        ctx.sv = sv
        return pooled

    @staticmethod
    def backward(ctx, dP):
        sv: _Saved = ctx.sv
        s, bn, nrm = sv.s, sv.bn, sv.norm
        dev = dP.device
        dP = dP.contiguous()
        with _lib.device_guard(dev):
            bn.begin_backward(dP)
            dx = None                      # last layer: gradient rebuilt from dP inside the kernels
            for li in range(bn.L - 1, -1, -1):
                x, w = sv.xs[li], sv.ws[li]
                hid, fin = w.shape[0], x.shape[1]
                dy = bn.backward(li, dx)
                if li == 0:
                    # Y0 = P0 W0^T + b  ->  dW0 = dY0^T P0 (no aggregation in the backward)
                    if sv.padded:
                        dwp = f32(dev, hid, PAD_K)
                        ops.linear_bwd_weight_raw(dy, sv.p0, dwp, 0)
                        bn.grads[0] = dwp[:, :fin].contiguous()
                    else:
                        ops.linear_bwd_weight_raw(dy, sv.p0, bn.dw(0, w), 0)
                    break
                if sv.tiled:
                    dt = ops.aggregate_tiled_raw(s, sv.ell, ops.AGG_TRANSPOSED, dy, nrm.dis, nrm.dis, None)
                else:
                    dt = ops.aggregate_raw(s.rowptr_src, s.col_src, nrm.coef_src, nrm.selfc, None, None, dy,
                                           band=sv.band[1])
                ops.linear_bwd_weight_raw(dt, x, bn.dw(li, w), 0)
                dx = ops.linear_bwd_input_raw(dt, w, 0, fin)
            grads = bn.finish()
        ctx.sv = None
        return (None, None, *grads)


def encode(model, batch, structure) -> torch.Tensor:
    return _encode(GcnWideEncode, model, batch, structure)
