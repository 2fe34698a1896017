"""torch.autograd bridges over the C ABI (include/cgnn.h).

Each Function is a thin shim: it allocates outputs/scratch with torch's caching allocator,
passes raw device pointers + the current HIP stream to libcgnn_hip.so, and wires the
matching backward kernels.  No arithmetic of the message-passing path happens in torch here.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .structure import _require_device


def _prep(t: Optional[torch.Tensor], what: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    _require_device(t, what)
    if t.dtype != torch.float32:
        # the reference is fp32-only on this path (SURVEY: .half()/.double() raise)
        raise TypeError(f"{what} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _scratch(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------ raw launchers
class BandOp:
    """The dense 32 x 16 fragments of one aggregation operator as pre-split MFMA operands
    (cgnn_band_pack_f32) plus the CSR of the edges outside them: together the operator.  Static per
    batch, like the CSR it is built from."""
    __slots__ = ("bfrag", "bstep", "boff", "pitch", "rowptr", "col", "coef", "num_items", "covered")


BAND_MIN_NNZ = 64          # a fragment goes to the matrix cores when it holds more non-zeros than this
BAND_MIN_COVER = 0.5       # ... and the band form is used when such fragments hold at least this share of the edges


def band_operator_f32(structure, rowptr, col, coef) -> Optional[BandOp]:
    """BandOp of the CSR ordering (rowptr, col, coef) of ``structure`` -- or None when the graphs are
    small enough for the LDS-tiled aggregate, too large for the fragment builder, or not dense enough."""
    s = structure
    if not s.block_diagonal or s.max_nodes_per_graph <= 384 or s.max_nodes_per_graph > 1024 or s.num_edges == 0:
        return None
    dev = coef.device
    pitch = (s.max_nodes_per_graph + 63) // 64 * 64
    steps, nrb = pitch // 16, pitch // 32
    nrows = s.num_graphs * nrb
    counts = torch.empty(nrows * steps, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        _lib.call("cgnn_dense_pack_count", rowptr, col, coef, None, s.gptr, s.num_graphs, pitch, counts)
        cnt = counts.view(nrows, steps).to(torch.int64)
        is_d = cnt > BAND_MIN_NNZ
        covered = float((cnt * is_d).sum()) / max(float(cnt.sum()), 1.0)      # host sync: collate-time
        if covered < BAND_MIN_COVER:
            return None
        boff = torch.zeros(nrows + 1, dtype=torch.int64, device=dev)
        torch.cumsum(is_d.sum(1), 0, out=boff[1:])
        items = int(boff[-1])
        rank = torch.cumsum(is_d, 1) - is_d.to(torch.int64) + boff[:-1, None]
        fpos = torch.where(is_d, rank, torch.full_like(cnt, 0xFFFFFFFF))
        fpos32 = torch.where(fpos >= 2 ** 31, fpos - 2 ** 32, fpos).to(torch.int32).contiguous()
        op = BandOp()
        op.bfrag = torch.empty(max(items, 1) * 3 * 64 * 4, dtype=torch.int32, device=dev)     # 3 KB per fragment
        op.bstep = torch.zeros(max(items, 1), dtype=torch.int32, device=dev)
        _lib.call("cgnn_band_pack_f32", rowptr, col, coef, s.gptr, s.num_graphs, pitch, fpos32, op.bfrag, op.bstep)
        # the CSR of the edges outside the listed fragments (COO order inside a row is kept)
        nn_ = s.num_nodes
        deg = (rowptr[1:] - rowptr[:-1]).to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(nn_, device=dev), deg)
        g = s.node_graph.to(torch.int64)[rows]
        gbase = s.gptr.to(torch.int64)[g]
        frag = (g * nrb + (rows - gbase) // 32) * steps + (col.to(torch.int64) - gbase) // 16
        keep = ~is_d.reshape(-1)[frag]
        op.col, op.coef = col[keep].contiguous(), coef[keep].contiguous()
        rp = torch.zeros(nn_ + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(rows[keep], minlength=nn_), 0, out=rp[1:])
        op.rowptr = rp.to(torch.int32)
        torch.cuda.current_stream(dev).synchronize()        # fpos32 is a temporary of this call
    op.boff, op.pitch, op.num_items, op.covered = boff.to(torch.int32), pitch, items, covered
    return op


def band_aggregate_raw(structure, band: BandOp, selfc, rowdiv, bias, x, out=None, yadd=None) -> torch.Tensor:
    """The operator of ``band`` applied to x with the epilogue of aggregate_raw (+ yadd): the dense fragments'
    part written by cgnn_band_aggregate_f32, the remaining edges added by cgnn_aggregate_acc_f32."""
    n, f = x.shape
    y = torch.empty_like(x) if out is None else out
    # (one timed region: the two launches are one aggregation -- bench.py prices them together)
    with _lib.device_guard(x.device), _lib.timed("cgnn_band_aggregate_f32+cgnn_aggregate_acc_f32", f"F={f}"):
        sp = _lib.stream_ptr()
        _lib.call("cgnn_band_aggregate_f32", band.bfrag, band.bstep, band.boff, band.pitch, structure.gptr,
                  structure.num_graphs, x, x.stride(0), f, rowdiv, yadd, 0 if yadd is None else yadd.stride(0),
                  y, y.stride(0), stream=sp)
        _lib.call("cgnn_aggregate_acc_f32", band.rowptr, band.col, band.coef, selfc, rowdiv, bias, x, x.stride(0),
                  y, y.stride(0), n, f, stream=sp)
    return y


def aggregate_raw(rowptr, col, coef, selfc, rowdiv, bias, x, out=None, band=None, yadd=None) -> torch.Tensor:
    """out: optional [n, f] destination (may be a column slice of a wider row-major buffer).
    band = (structure, BandOp): the operator's dense fragments go to the matrix cores
    (band_aggregate.hip) and only the remaining edges through the gather kernel (widths 64, 128, 256).
    yadd: [n, f] added to the result (GraphSAGE's dX = dX1 + A^T(dA / den)); widths 64, 128, 256."""
    f = x.shape[1]
    wide = f in (64, 128, 256) and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and (
        out is None or (out.stride(0) % 4 == 0 and out.data_ptr() % 16 == 0))
    if band is not None and wide and (yadd is None or (yadd.stride(0) % 2 == 0 and yadd.data_ptr() % 8 == 0)):
        return band_aggregate_raw(band[0], band[1], selfc, rowdiv, bias, x, out, yadd)
    if yadd is not None:
        if not wide:
            raise ValueError("aggregate_raw(yadd=...) takes widths 64, 128, 256 (16-byte aligned rows)")
        y = torch.empty_like(x) if out is None else out
        y.copy_(yadd)                                  # the sum lands on top (cgnn_aggregate_acc_f32)
        _lib.call("cgnn_aggregate_acc_f32", rowptr, col, coef, selfc, rowdiv, bias, x, x.stride(0), y, y.stride(0),
                  x.shape[0], f, device=x.device, key=f"cgnn_aggregate_acc_f32[F={f}]")
        return y
    n, f = x.shape
    y = torch.empty_like(x) if out is None else out
    _lib.call("cgnn_aggregate_f32", rowptr, col, coef, selfc, rowdiv, bias, x, x.stride(0), y, y.stride(0), n, f,
              device=x.device, key=f"cgnn_aggregate_f32[F={f}]")
    return y


def colsum_raw(a: torch.Tensor) -> torch.Tensor:
    m, n = a.shape
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    slab = _scratch(_lib.load().cgnn_colsum_workspace_bytes(m, n), a.device)
    _lib.call("cgnn_colsum_f32", a, a.stride(0), out, m, n, *_lib.buf(slab), device=a.device)
    return out


def sddmm_raw(rowptr, col, eid, dy, x, xself=None, rowdiv=None, out=None, gself=None, num_slots=None) -> torch.Tensor:
    """out[eid[k] or k] = (<dy[r], x[col[k]]> - <dy[r], xself[r]>) / rowdiv[r] over the CSR (rowptr, col)
    (the subtraction and division only with rowdiv); gself[r] = <dy[r], xself[r]> (cgnn_sddmm_f32)."""
    n, f = dy.shape
    if out is None:
        out = torch.empty(int(col.numel()) if num_slots is None else num_slots, dtype=torch.float32,
                          device=dy.device)
    _lib.call("cgnn_sddmm_f32", rowptr, col, eid, dy, dy.stride(0), x, x.stride(0), xself,
              0 if xself is None else xself.stride(0), rowdiv, out, gself, n, f,
              device=dy.device, key=f"cgnn_sddmm_f32[F={f}]")
    return out


def gcn_norm_bwd_raw(structure, edge_weight, dis, g, gself) -> torch.Tensor:
    """dw [Ee] (COO order) of one GCN aggregate from g (COO order) and gself (cgnn_gcn_norm_bwd)."""
    s = structure
    dw = torch.empty(s.num_edges, dtype=torch.float32, device=g.device)
    ws = _scratch(_lib.load().cgnn_gcn_norm_bwd_workspace_bytes(s.num_nodes), g.device)
    _lib.call("cgnn_gcn_norm_bwd", s.rowptr_dst, s.col_dst, s.eid_dst, s.rowptr_src, s.col_src, s.eid_src,
              edge_weight, dis, g, gself, s.num_nodes, s.num_edges, dw, *_lib.buf(ws), device=g.device)
    return dw


def edge_grad_wanted(edge_weight) -> bool:
    """The loss gradient w.r.t. the batch's edge weights is asked for: the aggregates then take
    ``edge_weight`` as an autograd input (models.GCNLayer / SAGELayer)."""
    return edge_weight is not None and edge_weight.requires_grad and torch.is_grad_enabled()


def edge_weight_grad(kind: str, structure, norm, dy, xp, y=None) -> torch.Tensor:
    """dL/dw [Ee] (COO order) of one aggregate Y = A_hat X' (+ b) with dY = dy at its output:
    GCN (models.py:94-114) through the normalisation's backward, GraphSAGE (:146-149) whole in the SDDMM
    (y = the aggregate's output, the weighted mean)."""
    s = structure
    ew = s._edge_weight
    if s.num_edges == 0:
        return torch.zeros(0, dtype=torch.float32, device=dy.device)
    if kind == "gcn":
        g = torch.empty(s.num_edges, dtype=torch.float32, device=dy.device)
        gself = torch.empty(s.num_nodes, dtype=torch.float32, device=dy.device)
        sddmm_raw(s.rowptr_dst, s.col_dst, s.eid_dst, dy, xp, xself=xp, out=g, gself=gself)
        return gcn_norm_bwd_raw(s, ew, norm.dis, g, gself)
    return sddmm_raw(s.rowptr_dst, s.col_dst, s.eid_dst, dy, xp, xself=y, rowdiv=norm.den)


def _edge_grad_check(edge_weight, edge_grad):
    if edge_weight is None:
        return
    if edge_grad is None or edge_grad[0] not in ("gcn", "sage"):
        raise ValueError("edge_weight needs edge_grad=(kind 'gcn' | 'sage', structure, norm)")
    s = edge_grad[1]
    if not s.has_csr:
        raise RuntimeError("edge-weight gradients need the batch's own CSR structure (BatchStructure), got "
                           f"{type(s).__name__}")
    if edge_weight.numel() != s.num_edges:
        raise ValueError(f"edge_weight has {edge_weight.numel()} entries, the structure {s.num_edges} edges")


def _edge_grad_out(ctx, dy, xp, y):
    """dw shaped as the edge_weight input, or None when autograd does not ask for it."""
    if ctx.edge_grad is None or not ctx.needs_input_grad[ctx.ew_index]:
        return None
    kind, s, norm = ctx.edge_grad
    return edge_weight_grad(kind, s, norm, dy, xp, y).view(ctx.ew_shape)


def linear_fwd_raw(x1, x2, w, bias, relu: bool) -> torch.Tensor:
    m, k1 = x1.shape
    k2 = 0 if x2 is None else x2.shape[1]
    n = w.shape[0]
    if w.shape[1] != k1 + k2:
        raise ValueError(f"weight is {tuple(w.shape)}, inputs give K = {k1}+{k2}")
    y = torch.empty(m, n, dtype=torch.float32, device=x1.device)
    _lib.call("cgnn_linear_fwd_f32", x1, x1.stride(0), k1, x2, 0 if x2 is None else x2.stride(0), k2, w, bias,
              int(relu), y, y.stride(0), m, n, device=x1.device)
    return y


def linear_bwd_input_raw(dy, w, k0: int, k: int) -> torch.Tensor:
    m, n = dy.shape
    dx = torch.empty(m, k, dtype=torch.float32, device=dy.device)
    _lib.call("cgnn_linear_bwd_input_f32", dy, dy.stride(0), w, w.stride(0), k0, dx, dx.stride(0), m, n, k,
              device=dy.device)
    return dx


def linear_bwd_weight_raw(dy, x, dw, k0: int) -> None:
    m, n = dy.shape
    k = x.shape[1]
    slab = _scratch(_lib.load().cgnn_linear_bwd_weight_workspace_bytes(m, n, k), dy.device)
    _lib.call("cgnn_linear_bwd_weight_f32", dy, dy.stride(0), x, x.stride(0), dw, dw.stride(0), k0, m, n, k,
              *_lib.buf(slab), device=dy.device)


def linear_bwd_weight2_raw(dy, x1, x2, dw) -> None:
    """dW [N, K1 + K2] = dY^T [X1 | X2] (cgnn_linear_bwd_weight2_f32: one pass over dY when the joint shape
    fits the weight-stationary kernel, else panel by panel); panels may differ in width."""
    m, n = dy.shape
    k1, k2 = x1.shape[1], x2.shape[1]
    slab = _scratch(_lib.load().cgnn_linear_bwd_weight2_workspace_bytes(m, n, k1, k2), dy.device)
    _lib.call("cgnn_linear_bwd_weight2_f32", dy, dy.stride(0), x1, x1.stride(0), k1, x2, x2.stride(0), k2,
              dw, dw.stride(0), m, n, *_lib.buf(slab), device=dy.device)


# ------------------------------------------------------------------------- autograd Functions
class _Aggregate(torch.autograd.Function):
    """Y = A_coef X (+ selfc*X) (/rowdiv) (+bias); backward runs the transposed CSR."""

    @staticmethod
    def forward(ctx, x, bias, fwd, bwd, edge_weight=None, edge_grad=None):
        rowptr, col, coef, selfc, rowdiv = fwd[:5]
        x = _prep(x, "x")
        bias_c = _prep(bias, "bias")
        y = aggregate_raw(rowptr, col, coef, selfc, rowdiv, bias_c, x, band=fwd[5] if len(fwd) > 5 else None)
        ctx.bwd = bwd
        ctx.selfc = selfc
        ctx.has_bias = bias is not None
        ctx.edge_grad = None
        if edge_weight is not None and ctx.needs_input_grad[4]:
            # X' (and GraphSAGE's weighted mean, the output) kept for the SDDMM of the edge gradient
            ctx.edge_grad, ctx.ew_index, ctx.ew_shape = edge_grad, 4, edge_weight.shape
            ctx.save_for_backward(x, y if edge_grad[0] == "sage" else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _prep(dy, "grad")
        t_rowptr, t_col, t_coef = ctx.bwd[:3]
        dx = db = dw = None
        if ctx.needs_input_grad[0]:
            dx = aggregate_raw(t_rowptr, t_col, t_coef, ctx.selfc, None, None, dy,
                               band=ctx.bwd[3] if len(ctx.bwd) > 3 else None)
        if ctx.has_bias and ctx.needs_input_grad[1]:
            db = colsum_raw(dy)
        if ctx.edge_grad is not None:
            xp, y = ctx.saved_tensors
            dw = _edge_grad_out(ctx, dy, xp, y)
        return dx, db, None, None, dw, None


AGG_TRANSPOSED, AGG_PRE_DIV, AGG_POST_DIV = 1, 2, 4   # include/cgnn.h


def aggregate_tiled_raw(structure, meta, flags: int, x, pre, post, bias, yadd=None) -> torch.Tensor:
    """Y = post * A(pre * X) (+bias) (+yadd) through cgnn_aggregate_tiled_f32 (LDS-staged tiles).
    x / yadd may be column slices of wider row-major buffers (their row stride is passed on)."""
    n, f = x.shape
    y = torch.empty(n, f, dtype=torch.float32, device=x.device)
    _lib.call("cgnn_aggregate_tiled_f32", structure.tiles_struct(meta), int(flags), x, x.stride(0), f, pre, post,
              bias, yadd, 0 if yadd is None else yadd.stride(0), y, y.stride(0),
              device=x.device, key=f"cgnn_aggregate_tiled_f32[F={f}]")
    return y


def aggregate_tiled_bn_raw(structure, meta, flags: int, z, pre, post, bias, coef, relu: bool, p: float,
                           seed: int, seed_dev, mask, xout) -> torch.Tensor:
    """Y = post * A(pre * X) (+bias) with X = drop(act(a z + b)) formed while the tiles are staged and
    also written to ``xout`` (keep bytes to ``mask``): cgnn_aggregate_tiled_bn_f32."""
    n, f = z.shape
    y = torch.empty(n, f, dtype=torch.float32, device=z.device)
    # (timed under the plain tiled aggregate's key: bench.py prices both as the same aggregation)
    _lib.call("cgnn_aggregate_tiled_bn_f32", structure.tiles_struct(meta), int(flags), z, z.stride(0), f, pre, post,
              bias, y, y.stride(0), coef, int(relu), float(p), int(seed), seed_dev, mask, xout, xout.stride(0),
              device=z.device, key=f"cgnn_aggregate_tiled_f32[F={f}]")
    return y


def aggregate_tiled_f16_raw(structure, meta, flags: int, x, pre, post, bias) -> torch.Tensor:
    """fp16-storage / fp32-accumulate tiled aggregate (cgnn_aggregate_tiled_f16): x, result half."""
    _require_device(x, "x")
    if x.dtype != torch.float16:
        raise TypeError(f"x must be float16, got {x.dtype}")
    n, f = x.shape
    y = torch.empty(n, f, dtype=torch.float16, device=x.device)
    _lib.call("cgnn_aggregate_tiled_f16", structure.tiles_struct(meta), int(flags), x, x.stride(0), f, pre, post,
              bias, y, y.stride(0), device=x.device, key=f"cgnn_aggregate_tiled_f16[F={f}]")
    return y


def dense_adj_f16(structure, coef, selfc, transposed: bool = False) -> torch.Tensor:
    """[B, P, P] half dense operator of one CSR ordering (cgnn_dense_adj_f16); static per batch."""
    s = structure
    pitch = (s.max_nodes_per_graph + 63) // 64 * 64
    m = torch.empty(s.num_graphs, pitch, pitch, dtype=torch.float16, device=coef.device)
    rowptr, col = (s.rowptr_src, s.col_src) if transposed else (s.rowptr_dst, s.col_dst)
    _lib.call("cgnn_dense_adj_f16", rowptr, col, coef, selfc, s.gptr, s.num_graphs, pitch, m, device=coef.device)
    return m


def dense_aggregate_f16_raw(structure, m, x, bias=None, stat_slab=None) -> torch.Tensor:
    """Y_g = M_g X_g on the fp16 matrix cores (cgnn_dense_aggregate_f16); x, result half.
    stat_slab: optional fp64 [cgnn_fused_grid(), 2F] for the result's BatchNorm sums."""
    _require_device(x, "x")
    if x.dtype != torch.float16 or m.dtype != torch.float16:
        raise TypeError("x and m must be float16")
    n, f = x.shape
    y = torch.empty(n, f, dtype=torch.float16, device=x.device)
    _lib.call("cgnn_dense_aggregate_f16", m, m.shape[1], structure.gptr, structure.num_graphs, x, x.stride(0), f,
              bias, y, y.stride(0), *_lib.buf(stat_slab), device=x.device, key=f"cgnn_dense_aggregate_f16[F={f}]")
    return y


class DensePack:
    """A dense per-graph operator of one CSR ordering stored per MFMA fragment (cgnn_dense_pack_*):
    nearly full fragments dense, the others as lists of their non-zero entries, empty ones not at
    all.  Static per batch, like the CSR it is built from."""
    __slots__ = ("dfrag", "dstep", "doff", "sent", "sstep", "soff", "pitch", "nnz", "num_dense", "num_sparse")

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.dfrag, self.dstep, self.doff, self.sent,
                                                          self.sstep, self.soff))


def dense_pack_f16(structure, coef, selfc, transposed: bool = False) -> DensePack:
    s = structure
    dev = coef.device
    pitch = (s.max_nodes_per_graph + 63) // 64 * 64
    steps, nrows = pitch // 16, s.num_graphs * (pitch // 32)
    rowptr, col = (s.rowptr_src, s.col_src) if transposed else (s.rowptr_dst, s.col_dst)
    counts = torch.empty(nrows * steps, dtype=torch.int32, device=dev)
    args = (rowptr, col, coef, selfc, s.gptr, s.num_graphs, pitch)
    pk = DensePack()
    with _lib.device_guard(dev):
        _lib.call("cgnn_dense_pack_count", *args, counts)
        cnt = counts.view(nrows, steps).to(torch.int64)
        is_d, is_s = cnt > 64, (cnt > 0) & (cnt <= 64)
        nd, ns = is_d.sum(1), is_s.sum(1)
        ns4 = (ns + 3) // 4 * 4                              # the aggregate loads four chunks at a time
        doff = torch.zeros(nrows + 1, dtype=torch.int64, device=dev)
        soff = torch.zeros(nrows + 1, dtype=torch.int64, device=dev)
        torch.cumsum(nd, 0, out=doff[1:])
        torch.cumsum(ns4, 0, out=soff[1:])
        tot_d, tot_s = int(doff[-1]), int(soff[-1])          # host sync: collate-time, outside the step
        if max(tot_d, tot_s) >= 2 ** 30:
            raise ValueError("dense operator too large to pack")
        rank_d = torch.cumsum(is_d, 1) - is_d.to(torch.int64) + doff[:-1, None]
        rank_s = torch.cumsum(is_s, 1) - is_s.to(torch.int64) + soff[:-1, None]
        fpos = torch.full_like(cnt, 0xFFFFFFFF)
        fpos = torch.where(is_d, rank_d | 0x80000000, fpos)
        fpos = torch.where(is_s, rank_s, fpos)
        fpos = torch.where(fpos >= 2 ** 31, fpos - 2 ** 32, fpos).to(torch.int32)    # uint32 bit patterns
        pk.dfrag = torch.empty(max(tot_d, 1) * 512, dtype=torch.float16, device=dev)
        pk.dstep = torch.zeros(max(tot_d, 1), dtype=torch.int32, device=dev)
        pk.sent = torch.full((max(tot_s, 4) * 64,), 0xFFFF, dtype=torch.int32, device=dev)
        pk.sstep = torch.zeros(max(tot_s, 4), dtype=torch.int32, device=dev)
        pk.doff, pk.soff = doff.to(torch.int32), soff.to(torch.int32)
        _lib.call("cgnn_dense_pack_fill", *args, fpos.contiguous(), pk.dfrag, pk.dstep, pk.sent, pk.sstep)
        torch.cuda.current_stream(dev).synchronize()        # fpos is a temporary of this call
    pk.pitch, pk.nnz, pk.num_dense, pk.num_sparse = pitch, int(counts.sum()), tot_d, int(ns.sum())
    return pk


def dense_aggregate_c16_raw(structure, pack: DensePack, x, bias=None, stat_slab=None) -> torch.Tensor:
    """Y_g = M_g X_g from the per-fragment operator (cgnn_dense_aggregate_c16); x, result half."""
    _require_device(x, "x")
    if x.dtype != torch.float16:
        raise TypeError("x must be float16")
    n, f = x.shape
    y = torch.empty(n, f, dtype=torch.float16, device=x.device)
    _lib.call("cgnn_dense_aggregate_c16", pack.dfrag, pack.dstep, pack.doff, pack.sent, pack.sstep, pack.soff,
              pack.pitch, structure.gptr, structure.num_graphs, x, x.stride(0), f, bias, y, y.stride(0),
              *_lib.buf(stat_slab), device=x.device, key=f"cgnn_dense_aggregate_c16[F={f}]")
    return y


def dense_aggregate_c16_bnbwd_raw(structure, pack: DensePack, dx, dP, yl, mask, coef, bwc, relu: bool, p: float):
    """dT = M_g dY with dY = BatchNorm'(dX' * act' * drop') formed while the slices are staged
    (cgnn_dense_aggregate_c16_bnbwd): returns (dT half [M, F], cs_slab fp64 [B, F] = per-graph column
    sums of dY).  Exactly one of dx (half [M, F]) and dP (fp32 [B, F], readout gradient)."""
    n, f = yl.shape
    dt = torch.empty(n, f, dtype=torch.float16, device=yl.device)
    cs = torch.empty(structure.num_graphs, f, dtype=torch.float64, device=yl.device)
    _lib.call("cgnn_dense_aggregate_c16_bnbwd", pack.dfrag, pack.dstep, pack.doff, pack.sent, pack.sstep, pack.soff,
              pack.pitch, structure.gptr, structure.num_graphs, dx, 0 if dx is None else dx.stride(0), dP,
              yl, yl.stride(0), mask, coef, bwc, int(relu), float(p), f, dt, dt.stride(0), *_lib.buf(cs),
              device=yl.device, key=f"cgnn_dense_aggregate_c16_bnbwd[F={f}]")
    return dt, cs


# ---- fp16-storage projections (gemm_h16.hip): activations half, weights / weight gradients fp32
def _need_half(t: torch.Tensor, what: str) -> None:
    _require_device(t, what)
    if t.dtype != torch.float16 or t.stride(-1) != 1:
        raise TypeError(f"{what} must be a float16 matrix with contiguous rows")


def linear_fwd_f16_raw(x, w, bias=None) -> torch.Tensor:
    """Y = X W^T + bias: X half [M, K], W fp32 [N, Kw] with Kw <= K (columns k >= Kw of X are
    ignored: layer 0's few input features ride in a 64-column panel); Y half [M, N]."""
    _need_half(x, "x")
    m, k = x.shape
    n, kw = w.shape
    y = torch.empty(m, n, dtype=torch.float16, device=x.device)
    _lib.call("cgnn_linear_fwd_f16", x, x.stride(0), k, w, w.stride(0), kw, bias, y, y.stride(0), m, n,
              device=x.device, key=f"cgnn_linear_fwd_f16[K={k},N={n}]")
    return y


def linear_fwd_stats_f16_raw(x, w, bias, grid: int):
    """linear_fwd_f16_raw that also leaves the BatchNorm statistics of Y (sum | sum of squares per
    column, fp64 per-workgroup partials [grid, 2N]) -- or (None, None) outside the kernel's shapes."""
    _need_half(x, "x")
    m, k = x.shape
    n, kw = w.shape
    y = torch.empty(m, n, dtype=torch.float16, device=x.device)
    slab = torch.empty(grid, 2 * n, dtype=torch.float64, device=x.device)
    rc = _lib.call("cgnn_linear_fwd_stats_f16", x, x.stride(0), k, w, w.stride(0), kw, bias, y, y.stride(0), m, n,
                   *_lib.buf(slab), device=x.device, key=f"cgnn_linear_fwd_stats_f16[K={k},N={n}]",
                   accept=(_lib.CGNN_EUNSUPPORTED,))
    return (None, None) if rc == _lib.CGNN_EUNSUPPORTED else (y, slab)


def linear_bwd_input_f16_raw(dy, w) -> torch.Tensor:
    """dX = dY W: dY half [M, N], W fp32 [N, K]; dX half [M, K]."""
    _need_half(dy, "dy")
    m, n = dy.shape
    k = w.shape[1]
    dx = torch.empty(m, k, dtype=torch.float16, device=dy.device)
    _lib.call("cgnn_linear_bwd_input_f16", dy, dy.stride(0), w, w.stride(0), dx, dx.stride(0), m, n, k,
              device=dy.device, key=f"cgnn_linear_bwd_input_f16[K={k},N={n}]")
    return dx


def linear_bwd_weight_f16_raw(dy, x, kw: Optional[int] = None) -> torch.Tensor:
    """dW[N, kw] (fp32) = dY^T X[:, :kw]: dY half [M, N], X half [M, K]."""
    _need_half(dy, "dy")
    _need_half(x, "x")
    m, n = dy.shape
    k = x.shape[1]
    kw = k if kw is None else int(kw)
    nbytes = int(_lib.load().cgnn_linear_bwd_weight_f16_workspace_bytes(m, n, k))
    if nbytes < 0:
        raise _lib.CgnnError(f"cgnn_linear_bwd_weight_f16: shape N={n}, K={k} not covered")
    slab = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=dy.device)
    dw = torch.empty(n, kw, dtype=torch.float32, device=dy.device)
    _lib.call("cgnn_linear_bwd_weight_f16", dy, dy.stride(0), x, x.stride(0), dw, kw, kw, m, n, k, *_lib.buf(slab),
              device=dy.device, key=f"cgnn_linear_bwd_weight_f16[K={k},N={n}]")
    return dw


def pad_cast_f16(x, width: int) -> torch.Tensor:
    """[x | zeros] as a half [M, width] panel (x fp32 [M, F], F <= width)."""
    _require_device(x, "x")
    if x.dtype != torch.float32 or x.stride(1) != 1:
        raise TypeError("x must be a float32 matrix with contiguous rows")
    m, f = x.shape
    y = torch.empty(m, width, dtype=torch.float16, device=x.device)
    _lib.call("cgnn_pad_cast_f16", x, x.stride(0), f, y, width, m, device=x.device)
    return y


class _AggregateTiled(torch.autograd.Function):
    """Y = post * A(pre * X) + bias on the blocked-ELL tiles; backward = the transposed ELL with
    pre and post swapped."""

    @staticmethod
    def forward(ctx, x, bias, structure, meta, pre, post, pre_div, post_div, edge_weight=None, edge_grad=None):
        x = _prep(x, "x")
        bias_c = _prep(bias, "bias")
        flags = (AGG_PRE_DIV if pre_div else 0) | (AGG_POST_DIV if post_div else 0)
        y = aggregate_tiled_raw(structure, meta, flags, x, pre, post, bias_c)
        ctx.cfg = (structure, meta, pre, post, pre_div, post_div)
        ctx.has_bias = bias is not None
        ctx.edge_grad = None
        if edge_weight is not None and ctx.needs_input_grad[8]:
            ctx.edge_grad, ctx.ew_index, ctx.ew_shape = edge_grad, 8, edge_weight.shape
            ctx.save_for_backward(x, y if edge_grad[0] == "sage" else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        structure, meta, pre, post, pre_div, post_div = ctx.cfg
        dy = _prep(dy, "grad")
        dx = db = dw = None
        if ctx.needs_input_grad[0]:
            flags = AGG_TRANSPOSED | (AGG_PRE_DIV if post_div else 0) | (AGG_POST_DIV if pre_div else 0)
            dx = aggregate_tiled_raw(structure, meta, flags, dy, post, pre, None)
        if ctx.has_bias and ctx.needs_input_grad[1]:
            db = colsum_raw(dy)
        if ctx.edge_grad is not None:
            xp, y = ctx.saved_tensors
            dw = _edge_grad_out(ctx, dy, xp, y)
        return dx, db, None, None, None, None, None, None, dw, None


def aggregate_tiled(x, bias, structure, meta, pre=None, post=None, pre_div=False, post_div=False,
                    edge_weight=None, edge_grad=None):
    """edge_weight / edge_grad: as aggregate()."""
    if edge_weight is None:
        return _AggregateTiled.apply(x, bias, structure, meta, pre, post, pre_div, post_div)
    _edge_grad_check(edge_weight, edge_grad)
    return _AggregateTiled.apply(x, bias, structure, meta, pre, post, pre_div, post_div, edge_weight, edge_grad)


def aggregate(x, bias, fwd, bwd, edge_weight=None, edge_grad=None) -> torch.Tensor:
    """fwd = (rowptr, col, coef, selfc|None, rowdiv|None [, band]) on the dst-sorted CSR;
    bwd = (rowptr, col, coef [, band]) on the src-sorted CSR (coef already divided by rowdiv);
    band = (structure, BandOp) or None (aggregate_raw).
    edge_weight (optional): the batch's COO edge weights [Ee] the coefficients were computed from, taken as an
    autograd input: backward then returns dL/dw of this aggregate, edge_grad = ("gcn", structure, GcnNorm) or
    ("sage", structure, SageNorm) saying how (edge_weight_grad).  The forward launches are the same."""
    if edge_weight is None:
        return _Aggregate.apply(x, bias, fwd, bwd)
    _edge_grad_check(edge_weight, edge_grad)
    return _Aggregate.apply(x, bias, fwd, bwd, edge_weight, edge_grad)


class _Linear(torch.autograd.Function):
    """Y = act(X1 W[:, :K1]^T + X2 W[:, K1:]^T + b) on the matrix cores."""

    @staticmethod
    def forward(ctx, x1, x2, w, bias, relu):
        x1, x2, w, bias_c = _prep(x1, "x"), _prep(x2, "x2"), _prep(w, "weight"), _prep(bias, "bias")
        y = linear_fwd_raw(x1, x2, w, bias_c, relu)
        ctx.relu = relu
        ctx.has_x2 = x2 is not None
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x1, x2, w, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x1, x2, w, y = ctx.saved_tensors
        dy = _prep(dy, "grad")
        if ctx.relu:
            dy = dy * (y > 0)            # elementwise mask; the GEMMs below are the HIP kernels
        k1 = x1.shape[1]
        k2 = x2.shape[1] if x2 is not None else 0
        dx1 = dx2 = dw = db = None
        if ctx.needs_input_grad[0]:
            dx1 = linear_bwd_input_raw(dy, w, 0, k1)
        if x2 is not None and ctx.needs_input_grad[1]:
            dx2 = linear_bwd_input_raw(dy, w, k1, k2)
        if ctx.needs_input_grad[2]:
            dw = torch.empty_like(w)
            linear_bwd_weight_raw(dy, x1, dw, 0)
            if x2 is not None:
                linear_bwd_weight_raw(dy, x2, dw, k1)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            db = colsum_raw(dy)
        return dx1, dx2, dw, db, None


def linear(x1, x2, w, bias, relu: bool = False) -> torch.Tensor:
    return _Linear.apply(x1, x2, w, bias, relu)


class _PoolMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gptr, num_graphs):
        x = _prep(x, "x")
        f = x.shape[1]
        p = torch.empty(num_graphs, f, dtype=torch.float32, device=x.device)
        _lib.call("cgnn_pool_mean_fwd_f32", x, x.stride(0), gptr, p, num_graphs, f, device=x.device)
        ctx.gptr, ctx.shape = gptr, x.shape
        return p

    @staticmethod
    def backward(ctx, dp):
        dp = _prep(dp, "grad")
        n, f = ctx.shape
        dx = torch.empty(n, f, dtype=torch.float32, device=dp.device)
        _lib.call("cgnn_pool_mean_bwd_f32", dp, ctx.gptr, dx, dx.stride(0), dp.shape[0], f, device=dp.device)
        return dx, None, None


def pool_mean(x, gptr, num_graphs: int) -> torch.Tensor:
    return _PoolMean.apply(x, gptr, num_graphs)


class _BnActDrop(torch.autograd.Function):
    """X' = dropout(act(BatchNorm1d(Y))) in two streaming passes each way (elementwise.hip)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, bn_mod, relu, p, training, rng_word=None, record=None):
        lib = _lib.load()
        y = _prep(y, "y")
        m, n = y.shape
        dev = y.device
        f32 = dict(dtype=torch.float32, device=dev)
        p_eff = float(p) if training else 0.0
        coef = torch.empty(4 * n, **f32)
        x = torch.empty_like(y)
        mask = torch.empty(m * (n // 4), dtype=torch.uint8, device=dev) if p_eff > 0 else None
        seed = _lib.next_seed(dev) if p_eff > 0 else 0
        sp = _lib.stream_ptr(dev)           # one lookup per pass (torch.cuda.current_stream is ~10 us)
        with _lib.device_guard(dev):
            rows = int(lib.cgnn_bn_act_slab_rows(m))
            slab = torch.empty(rows, 2 * n, dtype=torch.float64, device=dev) if training else None
            if training:
                _lib.call("cgnn_bn_act_fwd_stats", y, m, n, *_lib.buf(slab), stream=sp)
            _lib.call("cgnn_bn_act_finalize", slab, rows, n, float(max(m, 1)), None, int(training),
                      gamma.contiguous(), beta.contiguous(), bn_mod.running_mean, bn_mod.running_var,
                      float(bn_mod.momentum), float(bn_mod.eps), bn_mod.num_batches_tracked if training else None,
                      coef, stream=sp)
            _lib.call("cgnn_bn_act_fwd_apply", y, coef, int(relu), p_eff, seed, rng_word if p_eff > 0 else None,
                      mask, x, m, n, stream=sp)
        if record is not None:
            record.setdefault("layers", []).append(mask)
        ctx.save_for_backward(y, coef, mask)
        ctx.cfg = (bool(relu), p_eff, bool(training))
        return x

    @staticmethod
    def backward(ctx, dx):
        lib = _lib.load()
        y, coef, mask = ctx.saved_tensors
        relu, p_eff, training = ctx.cfg
        dx = _prep(dx, "grad")
        m, n = y.shape
        dev = y.device
        f32 = dict(dtype=torch.float32, device=dev)
        sp = _lib.stream_ptr(dev)           # one lookup per pass (torch.cuda.current_stream is ~10 us)
        dgamma, dbeta, bwc = torch.empty(n, **f32), torch.empty(n, **f32), torch.empty(2 * n, **f32)
        dy = torch.empty_like(y)
        with _lib.device_guard(dev):
            rows = int(lib.cgnn_bn_act_slab_rows(m))
            slab = torch.empty(rows, 2 * n, dtype=torch.float64, device=dev)
            _lib.call("cgnn_bn_act_bwd_stats", dx, y, mask, coef, int(relu), p_eff, m, n, *_lib.buf(slab),
                      None, None, None, stream=sp)
            _lib.call("cgnn_bn_act_bwd_finalize", slab, rows, n, float(max(m, 1)), None, int(not training),
                      dgamma, dbeta, bwc, stream=sp)
            _lib.call("cgnn_bn_act_bwd_apply", dx, y, mask, coef, bwc, int(relu), p_eff, 0, None, 0, dy, m, n,
                      None, None, None, stream=sp)
        return dy, dgamma, dbeta, None, None, None, None, None, None


def bn_act_drop_supported(bn_mod, width: int) -> bool:
    """Plain nn.BatchNorm1d (affine, running stats, fixed momentum) of a power-of-two width."""
    return (type(bn_mod) is torch.nn.BatchNorm1d and bn_mod.affine and bn_mod.track_running_stats
            and bn_mod.momentum is not None and bool(_lib.load().cgnn_bn_act_width_ok(width)))


def bn_act_drop(y, bn_mod, relu: bool, p: float, training: bool, rng_word=None, record=None) -> torch.Tensor:
    """rng_word: device address of a uint32 that a captured cgnn_rng_advance refreshes (graph replay);
    record: dict that receives the keep-bit array of this launch (parity tests)."""
    return _BnActDrop.apply(y, bn_mod.weight, bn_mod.bias, bn_mod, relu, p, training, rng_word, record)


class _Head(torch.autograd.Function):
    """logits = Linear2(dropout(relu(Linear1(P)))) in one HIP kernel each way (csrc/head.hip)."""

    @staticmethod
    def forward(ctx, p, w1, b1, w2, b2, p_drop, training, rng_word, record=None):
        p, w1, b1, w2, b2 = (_prep(t, "head tensor") for t in (p, w1, b1, w2, b2))
        bsz, h = p.shape
        h2, c = w1.shape[0], w2.shape[0]
        dev = p.device
        f32 = dict(dtype=torch.float32, device=dev)
        p_eff = float(p_drop) if training else 0.0
        seed = _lib.next_seed(dev) if p_eff > 0 else 0
        h1, fac = torch.empty(bsz, h2, **f32), torch.empty(bsz, h2, **f32)
        logits = torch.empty(bsz, c, **f32)
        _lib.call("cgnn_head_fwd_f32", p, bsz, h, h2, c, w1, b1, w2, b2, p_eff, seed,
                  rng_word if p_eff > 0 else None, h1, fac, logits, device=dev)
        if record is not None:
            record["head_factor"] = fac          # relu'(z) * keep / (1 - p) per hidden unit
        ctx.save_for_backward(p, w1, w2, h1, fac)
        return logits

    @staticmethod
    def backward(ctx, dl):
        lib = _lib.load()
        p, w1, w2, h1, fac = ctx.saved_tensors
        dl = _prep(dl, "grad")
        bsz, h = p.shape
        h2, c = w1.shape[0], w2.shape[0]
        dev = p.device
        wd = h2 * h + h2 + c * h2 + c
        with _lib.device_guard(dev):
            rows = int(lib.cgnn_head_grid(bsz, h, h2, c))
            slab = torch.empty(rows, wd, dtype=torch.float32, device=dev)
            dp = torch.empty_like(p)
            flat = torch.empty(wd, dtype=torch.float32, device=dev)
            _lib.call("cgnn_head_bwd_f32", dl, p, h1, fac, bsz, h, h2, c, w1, w2, dp, *_lib.buf(slab))
            _lib.call("cgnn_slab_reduce_f32", slab, rows, 1, wd, wd, flat, wd)
        o1, o2, o3 = h2 * h, h2 * h + h2, h2 * h + h2 + c * h2
        return (dp, flat[:o1].view(h2, h), flat[o1:o2], flat[o2:o3].view(c, h2), flat[o3:],
                None, None, None, None)


class _HeadLoss(torch.autograd.Function):
    """(logits, loss) = the classifier and the batch-mean cross-entropy, with the whole backward of both
    done in the same launch (cgnn_head_loss_f32): the loss's upstream gradient in a training step is the
    unit, so dP and the parameter gradients are known when the forward ends.  backward() hands them out
    (scaled when the upstream gradient is not the unit); a gradient arriving through `logits` as well goes
    through cgnn_head_bwd_f32 on top."""

    @staticmethod
    def forward(ctx, p, w1, b1, w2, b2, labels, p_drop, training, rng_word, record=None, grad_dst=None):
        """grad_dst (optional): ONE contiguous fp32 run [W1 | b1 | W2 | b2] that receives the parameter
        gradients directly (the adjacent ``.grad`` views of a flat data-parallel buffer, grad_destination);
        backward then returns None for the four parameters."""
        lib = _lib.load()
        p, w1, b1, w2, b2 = (_prep(t, "head tensor") for t in (p, w1, b1, w2, b2))
        _require_device(labels, "labels")
        if labels.dtype != torch.int64:
            raise TypeError(f"labels must be int64, got {labels.dtype}")
        bsz, h = p.shape
        h2, c = w1.shape[0], w2.shape[0]
        dev = p.device
        f32 = dict(dtype=torch.float32, device=dev)
        p_eff = float(p_drop) if training else 0.0
        seed = _lib.next_seed(dev) if p_eff > 0 else 0
        wd = h2 * h + h2 + c * h2 + c
        h1, fac = torch.empty(bsz, h2, **f32), torch.empty(bsz, h2, **f32)
        logits, dp = torch.empty(bsz, c, **f32), torch.empty_like(p)
        flat = torch.empty(wd + 1, **f32)
        with _lib.device_guard(dev):
            rows = int(lib.cgnn_head_loss_grid(bsz, h, h2, c))
            slab = torch.empty(rows, wd + 1, **f32)
            sp = _lib.stream_ptr()
            _lib.call("cgnn_head_loss_f32", p, bsz, h, h2, c, w1, b1, w2, b2, labels.contiguous(), p_eff, seed,
                      rng_word if p_eff > 0 else None, h1, fac, logits, dp, *_lib.buf(slab), stream=sp)
            if grad_dst is not None:
                _lib.call("cgnn_slab_reduce_f32_split", slab, rows, wd + 1, wd, grad_dst, flat.data_ptr() + 4 * wd,
                          stream=sp)
            else:
                _lib.call("cgnn_slab_reduce_f32", slab, rows, 1, wd + 1, wd + 1, flat, wd + 1, stream=sp)
        if record is not None:
            record["head_factor"] = fac
        ctx.save_for_backward(p, w1, w2, h1, fac, dp, flat)
        ctx.grad_dst = grad_dst
        ctx.set_materialize_grads(False)
        return logits, flat[wd]

    @staticmethod
    def backward(ctx, dlogits, g):
        p, w1, w2, h1, fac, dp, flat = ctx.saved_tensors
        bsz, h = p.shape
        h2, c = w1.shape[0], w2.shape[0]
        o1, o2, o3 = h2 * h, h2 * h + h2, h2 * h + h2 + c * h2
        wd = o3 + c
        outs = None
        if g is not None and ctx.grad_dst is not None:
            # the parameter gradients already sit in the caller's buffer (written by the forward launch)
            if not _is_unit_grad(g):
                dp = dp * g
                ctx.grad_dst.mul_(g)
            outs = [dp, None, None, None, None]
        elif g is not None:
            if not _is_unit_grad(g):
                dp, flat = dp * g, flat * g
            outs = [dp, flat[:o1].view(h2, h), flat[o1:o2], flat[o2:o3].view(c, h2), flat[o3:wd]]
        if dlogits is not None:                   # a second consumer of the logits: the ordinary backward on top
            lib = _lib.load()
            dl = _prep(dlogits, "grad")
            with _lib.device_guard(p.device):
                rows = int(lib.cgnn_head_grid(bsz, h, h2, c))
                slab = torch.empty(rows, wd, dtype=torch.float32, device=p.device)
                dp2 = torch.empty_like(p)
                fl2 = torch.empty(wd, dtype=torch.float32, device=p.device)
                _lib.call("cgnn_head_bwd_f32", dl, p, h1, fac, bsz, h, h2, c, w1, w2, dp2, *_lib.buf(slab))
                _lib.call("cgnn_slab_reduce_f32", slab, rows, 1, wd, wd, fl2, wd)
            extra = [dp2, fl2[:o1].view(h2, h), fl2[o1:o2], fl2[o2:o3].view(c, h2), fl2[o3:]]
            outs = extra if outs is None else [b if a is None else a + b for a, b in zip(outs, extra)]
        if outs is None:
            outs = [None] * 5
        return (*outs, None, None, None, None, None, None)


def grad_destination(p) -> Optional[torch.Tensor]:
    """The tensor a hand-written backward may write ``p``'s gradient into INSTEAD of returning it to autograd
    (it then returns None for that input): ``p.grad`` when its owner has just zeroed it and armed it for exactly
    this (dist.GradSync.zero_grad: ``.grad`` is a view of the flat all-reduce buffer; writing there replaces
    AccumulateGrad's in-place add, one launch per parameter).  Claiming disarms: a second op that uses the same
    parameter gets None and goes through autograd."""
    if not getattr(p, "_cgnn_direct", False):
        return None
    g = p.grad
    p._cgnn_direct = False
    if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or not g.is_cuda:
        return None
    return g


def claim_destinations(params, training: bool):
    """grad_destination of every parameter of a one-node encoder (None entries = through autograd), or
    all-None outside a training forward."""
    if not (training and torch.is_grad_enabled()):
        return [None] * len(params)
    return [grad_destination(q) for q in params]


def undelivered(grads, dst):
    """What a hand-written backward returns to autograd: None where the gradient was written into its
    destination (grads[i] IS dst[i]), the gradient itself elsewhere."""
    return [None if (d is not None and g is d) else g for g, d in zip(grads, dst)]


def head_loss_supported(classifier) -> bool:
    """head_supported and one of the register-tiled shapes of cgnn_head_loss_f32 (two classes,
    hidden = 2 x the classifier's inner width in {32, 64, 128, 256}) -- the reference's default head."""
    if not head_supported(classifier):
        return False
    l1, l2 = classifier[0], classifier[3]
    return l2.out_features == 2 and l1.in_features == 2 * l1.out_features and l1.in_features in (32, 64, 128, 256)


def head_loss(classifier, pooled, labels, training: bool, rng_word=None, record=None):
    """(logits, mean cross-entropy) of head_loss_supported classifiers in one launch each way."""
    l1, _, drop, l2 = classifier
    ps = (l1.weight, l1.bias, l2.weight, l2.bias)
    dst = None
    if training and all(getattr(q, "_cgnn_direct", False) for q in ps):
        # the four gradients as ONE run of the flat buffer: only when their views are adjacent and in this order
        views = [q.grad for q in ps]
        if all(v is not None and v.is_contiguous() and v.dtype == torch.float32 for v in views) and all(
                views[i].data_ptr() + 4 * views[i].numel() == views[i + 1].data_ptr() for i in range(3)):
            for q in ps:
                grad_destination(q)                       # claimed (disarmed)
            dst = views[0]
    return _HeadLoss.apply(pooled, l1.weight, l1.bias, l2.weight, l2.bias, labels, drop.p, training, rng_word, record, dst)


def model_loss(model, loss_fn, batch) -> torch.Tensor:
    """loss_fn(model(batch), batch.labels) -- the training step's loss, reference train.py:48-49 -- through
    the model's fused classifier + loss launch when loss_fn is this package's CrossEntropyLoss (mean
    reduction, torch's defaults) and the model offers it for this batch."""
    fused = getattr(model, "forward_loss", None)
    if fused is not None and type(loss_fn) is CrossEntropyLoss:
        out = fused(batch)
        if out is not None:
            return out[1]
    return loss_fn(model(batch), batch.labels)


def head_supported(classifier) -> bool:
    """The reference's head layout: Sequential(Linear, ReLU, Dropout, Linear) at a covered width."""
    import torch.nn as nn
    if not (isinstance(classifier, nn.Sequential) and len(classifier) == 4):
        return False
    l1, act, drop, l2 = classifier
    if not (type(l1) is nn.Linear and type(act) is nn.ReLU and type(drop) is nn.Dropout
            and type(l2) is nn.Linear and l1.bias is not None and l2.bias is not None
            and l2.in_features == l1.out_features):
        return False
    return bool(_lib.load().cgnn_head_supported(l1.in_features, l1.out_features, l2.out_features))


def head(classifier, pooled, training: bool, rng_word=None, record=None) -> torch.Tensor:
    l1, _, drop, l2 = classifier
    return _Head.apply(pooled, l1.weight, l1.bias, l2.weight, l2.bias, drop.p, training, rng_word, record)


def unpack_keep_bits(mask: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """Keep-bit bytes of the dropout kernels -> float {0,1} [rows, cols].  Layout (every mask
    kernel of the library): byte ``row * cols/4 + chunk``, bit i <-> column ``4*chunk + i``."""
    m = mask.view(rows, cols // 4, 1).to(torch.int32)
    bits = (m >> torch.arange(4, device=mask.device, dtype=torch.int32).view(1, 1, 4)) & 1
    return bits.reshape(rows, cols).to(torch.float32)


class _CrossEntropy(torch.autograd.Function):
    """Mean cross-entropy and its gradient in one launch (csrc/head.hip, cgnn_cross_entropy_f32)."""

    @staticmethod
    def forward(ctx, logits, labels):
        logits = _prep(logits, "logits")
        _require_device(labels, "labels")
        if labels.dtype != torch.int64:
            raise TypeError(f"labels must be int64, got {labels.dtype}")
        bsz, c = logits.shape
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        dl = torch.empty_like(logits)
        _lib.call("cgnn_cross_entropy_f32", logits, labels.contiguous(), bsz, c, loss, dl, device=logits.device)
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        if _is_unit_grad(g):                  # backward_unit(): d loss / d loss = 1, nothing to scale
            return dl, None
        return dl * g, None


_UNIT = {}


def unit_grad(device) -> torch.Tensor:
    """The constant 0-dim 1.0 of a device: the root gradient of a scalar loss (never written to)."""
    key = (device.type, device.index)
    if key not in _UNIT:
        _UNIT[key] = torch.ones((), dtype=torch.float32, device=device)
    return _UNIT[key]


def _is_unit_grad(g: torch.Tensor) -> bool:
    u = _UNIT.get((g.device.type, g.device.index))
    return u is not None and g.data_ptr() == u.data_ptr()


def backward_unit(loss: torch.Tensor) -> None:
    """``loss.backward()`` for a scalar loss, with the root gradient taken from a cached constant
    instead of a fresh ``ones_like`` (one fill launch) -- and recognised by ``cross_entropy``'s
    backward, which then returns its stored gradient without the multiply by 1 (one more launch).
    Same gradients, two launches fewer per step."""
    if loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda:
        torch.autograd.backward(loss, grad_tensors=unit_grad(loss.device))
    else:
        loss.backward()


def cross_entropy(logits, labels) -> torch.Tensor:
    return _CrossEntropy.apply(logits, labels)


class CrossEntropyLoss(torch.nn.Module):
    """torch.nn.CrossEntropyLoss() (default arguments: mean reduction, no weights, no smoothing)
    for [B, C] logits on the GPU, as one HIP launch; what the reference's Trainer uses
    (train.py:39).  ``ignore_index = -100`` rows behave as in torch (no loss, zero gradient, not
    counted).  One deviation: a label outside [0, C) other than -100 makes torch raise; here the
    loss becomes NaN instead (raising would need a device-to-host sync on every step)."""

    def forward(self, logits, labels):
        return cross_entropy(logits, labels)
