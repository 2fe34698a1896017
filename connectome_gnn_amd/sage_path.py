"""GraphSAGE encoder as one autograd node (hidden % 64 == 0): host orchestration.

GraphSAGEConnectome.encode (reference models.py:256-262) through the generic ops is ~25 autograd
nodes per step; autograd then inserts a ReLU-mask multiply, a gradient add and a column sum per
layer as separate passes over [Nn, H] arrays.  Here the whole encoder is one
``torch.autograd.Function`` whose backward is written out by hand, so that every pass over a node
array is a HIP kernel that does several things at once:

  forward, layer l     A  = A_w X / (wsum + 1e-8)            cgnn_aggregate_tiled_f32 (LDS tiles)
                       Z  = relu([X | A] W^T + b)            cgnn_linear_fwd_f32 (MFMA, W in LDS)
                       X' = dropout(BatchNorm(Z))            cgnn_bn_act_* (bn_stage.py)
  backward, layer l    dPre = BatchNorm'(dX' * drop') * (Z > 0), db = colsum(dPre)
                                                             cgnn_bn_act_bwd_* (one apply pass)
                       dW = dPre^T [X | A]                   cgnn_linear_bwd_weight2_f32 (one pass)
                       [dX1 | dA] = dPre W                   cgnn_linear_bwd_input_f32 (one pass)
                       dX = dX1 + A_w^T (dA / (wsum+1e-8))   cgnn_aggregate_tiled_f32 (+Yadd)

No arithmetic of the path happens in torch here; torch allocates buffers and orders the launches.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops
from .bn_stage import PAD_K, PAD_MIN_ROWS, BnStage, encode as _encode, f32, ineligible, linear_fwd_stats
from .structure import TILED_MAX_ROWS


def widths_ineligible(model, tiled: bool = True) -> Optional[str]:
    """The part of eligible() that the layer widths decide.  tiled=False: off the tiled aggregate -- and what
    Trainer asks before building a subject cache, which it does for these widths only."""
    hid = model.convs[0].linear.weight.shape[0]
    if hid % 64 or not bool(_lib.load().cgnn_bn_act_width_ok(hid)):
        return "hidden_dim is not 64, 128, 256, ..."
    if not tiled and hid not in (64, 128, 256):
        # off the tiled aggregate the backward adds dX1 inside the gather kernel (ops.aggregate_raw(yadd=...)),
        # which covers widths 64 / 128 / 256 only: wider layers on large graphs take the layered path
        return "graphs do not fit an LDS tile and hidden_dim is not 64, 128 or 256"
    return None


def eligible(model, batch, structure) -> Optional[str]:
    """None if this path covers (model, batch); else the reason it does not."""
    tiled = structure.tiled_ok(model.convs[0].linear.weight.shape[0])
    if not tiled and not structure.has_csr:
        return widths_ineligible(model) or "graphs do not fit an LDS tile and the structure has no CSR form"
    return widths_ineligible(model, tiled) or ineligible(batch, structure, model)


class _Saved:
    __slots__ = ("s", "ell", "norm", "xs", "aggs", "ws", "xa0", "tiled", "band", "bn")


def _agg_narrow_tiled(s, ell, norm, x, out=None):
    """The same mean for a narrow x (layer 0's few input features) through the LDS-tiled aggregate on a
    zero-padded 64-column panel -- for structures that carry no CSR (the per-subject structure cache)."""
    f = x.shape[1]
    panel = torch.nn.functional.pad(x, (0, 64 * ((f + 63) // 64) - f))
    agg = ops.aggregate_tiled_raw(s, ell, ops.AGG_POST_DIV, panel, None, norm.den, None)[:, :f]
    if out is None:
        return agg.contiguous()
    out.copy_(agg)
    return out


def _agg_fwd(s, ell, norm, x, band=None):
    """weighted mean of in-neighbours, models.py:146-149"""
    if ell is not None and s.tiled_ok(x.shape[1]):
        return ops.aggregate_tiled_raw(s, ell, ops.AGG_POST_DIV, x, None, norm.den, None)
    if not s.has_csr:
        return _agg_narrow_tiled(s, ell, norm, x)
    return ops.aggregate_raw(s.rowptr_dst, s.col_dst, norm.w_dst, None, norm.den, None, x, band=band)


class SageEncode(torch.autograd.Function):
    """P[B,H] = mean-pool(SAGE stack(x0)); args = x0, cfg, then (W, b, gamma, beta) per layer."""

    @staticmethod
    def forward(ctx, x0, cfg, *params):
        lib = _lib.load()
        s = cfg["structure"]
        L = len(params) // 4
        dev = x0.device
        x = x0.contiguous()
        n_nodes = s.num_nodes
        sv = _Saved()
        sv.s = s
        grid = int(lib.cgnn_fused_grid())
        # graphs of <= 384 nodes: LDS tiles over the blocked-ELL; larger ones: the CSR gather kernel, its dense
        # fragments on the matrix cores where the batch has them (the transposed pass then needs w / den per edge)
        sv.tiled = s.tiled_ok(params[0].shape[0])
        sv.ell = s.fused_meta(TILED_MAX_ROWS, grid, 0.0) if sv.tiled else None
        sv.norm = s.sage_norm(backward_coef=not sv.tiled)
        sv.band = (None, None) if sv.tiled else s.band_ops("sage", sv.norm)
        sv.xs, sv.aggs, sv.ws = [], [], []
        sv.xa0 = None
        with _lib.device_guard(dev):
            sv.bn = bn = BnStage(cfg, L, dev, relu_after_bn=False)
            for li in range(L):
                w, b, gamma, beta = (t.contiguous() for t in params[4 * li:4 * li + 4])
                hid = w.shape[0]
                agg = None
                if li > 0:
                    # the previous layer's BatchNorm+dropout is applied here, by the consumer
                    pz = bn.ys[li - 1]
                    if sv.tiled and s.tiled_ok(pz.shape[1]):
                        # X' = drop(BatchNorm(Z)) formed while the aggregate stages its tiles (and
                        # written out for the projection): no apply pass
                        x = torch.empty_like(pz)
                        agg = ops.aggregate_tiled_bn_raw(s, sv.ell, ops.AGG_POST_DIV, pz, None, sv.norm.den, None,
                                                         bn.coefs[li - 1], False, bn.p, bn.seeds[li - 1],
                                                         bn.rws[li - 1], bn.masks[li - 1], x)
                    else:
                        x = bn.apply(li - 1)
                fin = x.shape[1]
                slab = None
                if li == 0 and 2 * fin <= PAD_K and hid in (64, 128, 256) and n_nodes >= PAD_MIN_ROWS:
                    # narrow input layer: pack [x0 | agg(x0) | 0] and the zero-padded weight into
                    # 32-wide panels so that the tall weight-stationary GEMMs apply (K = 10 would
                    # otherwise run the per-tile kernels at a few % of the matrix-core rate)
                    xa = torch.nn.functional.pad(x, (0, PAD_K - fin))        # one pass: [x0 | 0]
                    if not s.has_csr:
                        agg = _agg_narrow_tiled(s, sv.ell, sv.norm, x, out=xa[:, fin:2 * fin])
                    else:
                        agg = ops.aggregate_raw(s.rowptr_dst, s.col_dst, sv.norm.w_dst, None, sv.norm.den,
                                                None, x, out=xa[:, fin:2 * fin])
                    wp = torch.nn.functional.pad(w, (0, PAD_K - 2 * fin))
                    sv.xa0 = xa
                    gemm_in = (xa, None, wp)
                else:
                    if agg is None:
                        agg = _agg_fwd(s, sv.ell, sv.norm, x, sv.band[0])
                    gemm_in = (x, agg, w)
                z = None
                if bn.training:
                    # projection with the BatchNorm statistics of its output in the epilogue
                    z, slab = linear_fwd_stats(*gemm_in, b, grid)
                if z is None:
                    z = ops.linear_fwd_raw(*gemm_in, b, True)
                bn.forward(z, gamma, beta, slab)
                sv.xs.append(x); sv.aggs.append(agg); sv.ws.append(w)
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
            dx = None                      # last layer: gradient rebuilt from dP inside the kernels
            for li in range(bn.L - 1, -1, -1):
                x, agg, w = sv.xs[li], sv.aggs[li], sv.ws[li]
                hid, fin = w.shape[0], x.shape[1]
                # ---- BatchNorm + dropout backward, ReLU' of the layer and db in two passes
                dpre = bn.backward(li, dx)
                # ---- dW = dPre^T [X | A]
                if li == 0 and sv.xa0 is not None:
                    dwp = f32(dev, hid, PAD_K)
                    ops.linear_bwd_weight_raw(dpre, sv.xa0, dwp, 0)
                    bn.grads[0] = dwp[:, :2 * fin].contiguous()
                    break
                ops.linear_bwd_weight2_raw(dpre, x, agg, bn.dw(li, w))
                if li == 0:
                    break
                # ---- [dX1 | dA] = dPre W, then dX = dX1 + A_w^T (dA / den)
                dcat = ops.linear_bwd_input_raw(dpre, w, 0, 2 * fin)
                if sv.tiled:
                    dx = ops.aggregate_tiled_raw(s, sv.ell, ops.AGG_TRANSPOSED | ops.AGG_PRE_DIV,
                                                 dcat[:, fin:], sv.norm.den, None, None, yadd=dcat[:, :fin])
                else:
                    dx = ops.aggregate_raw(s.rowptr_src, s.col_src, sv.norm.coef_src_bwd, None, None, None,
                                           dcat[:, fin:], band=sv.band[1], yadd=dcat[:, :fin])
            grads = bn.finish()
        ctx.sv = None
        return (None, None, *grads)


def encode(model, batch, structure) -> torch.Tensor:
    return _encode(SageEncode, model, batch, structure)
