/* cgnn.h -- C ABI of libcgnn_hip.so: the MI355X (gfx950) kernels behind the
 * batched message-passing path of connectome-gnn-suite.
 *
 * The reference has no FFI seam on this path (it is pure PyTorch); each entry
 * point below names the reference lines whose arithmetic it replaces.  The reference-side
 * binding (ctypes) is shown in INTEGRATION.md and implemented in connectome_gnn_amd/_lib.py.
 *
 * Conventions
 *   - extern "C"; every function returns int: CGNN_OK or a negative CGNN_E* code.  Nothing
 *     throws, aborts, allocates, frees or synchronises.
 *   - Pointers are DEVICE pointers unless the name ends in _host.  Sizes are element counts.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All work is
 *     enqueued on it; outputs are valid once the stream reaches that point.
 *   - Re-entrant and thread-safe for distinct buffers/streams; no global mutable state.
 *   - Floating point is fp32 storage / fp32 accumulate unless a name says otherwise
 *     (BatchNorm statistics are accumulated in fp64).  Indices inside the library are int32;
 *     the int64 COO of the reference (graph.py:104-105) is read only by cgnn_csr_build.
 *
 * Layout vocabulary (graph.py:101-140): a ConnectomeBatch packs B graphs block-diagonally:
 *   Nn nodes, Ee directed edges, node n of graph g has global id ptr[g] + n;
 *   edge_index is [2, Ee] int64 row-major (row 0 = src, row 1 = dst).
 */
#ifndef CGNN_H
#define CGNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_OK            0
#define CGNN_EINVAL       (-1)  /* bad argument (null pointer, negative size, unsupported width) */
#define CGNN_ELAUNCH      (-2)  /* hipGetLastError() != hipSuccess after a launch */
#define CGNN_EUNSUPPORTED (-3)  /* shape outside what this build of the kernels covers */

#define CGNN_ABI_VERSION 2   /* 2: every scratch / partial-sum buffer the library WRITES is passed with its
                              * byte count (`<name>_bytes` right after the pointer); a buffer shorter than what
                              * the path about to run writes makes the call return CGNN_EINVAL before any launch
                              * (a NULL optional buffer ignores its count) */

/* Library/ABI version and the gfx target the kernels were compiled for ("gfx950"). */
int cgnn_abi_version(void);
const char* cgnn_build_target(void);

/* ---------------------------------------------------------------------------------------
 * Structure: destination- and source-sorted CSR of the batch COO.
 * Replaces the implicit index handling of scatter_add_/index in models.py:40-54,103-113,
 * 146-149 (forward = rows by dst; autograd's backward of x[src] = rows by src).
 * Slots inside a row keep COO order (stable), so per-row sums run in the reference's order
 * and duplicate edges survive.
 * ------------------------------------------------------------------------------------- */

/* Bytes of scratch cgnn_csr_build needs for (num_nodes, num_edges). */
int64_t cgnn_csr_workspace_bytes(int64_t num_nodes, int64_t num_edges);

/* edge_index : int64 [2, Ee]         (graph.py:152 offsets already applied)
 * node_graph : int64 [Nn] or NULL    (ConnectomeBatch.batch; enables the cross-graph check)
 * rowptr_dst : int32 [Nn+1] out      in-edge row pointer       rowptr_src: same for out-edges
 * eid_dst    : int32 [Ee]   out      COO edge id of each slot  eid_src
 * col_dst    : int32 [Ee]   out      src node of each slot     col_src  : dst node of each slot
 * flags      : int32 [4]    out      [0] edges with an endpoint outside [0,Nn) (dropped),
 *                                    [1] edges whose endpoints lie in different graphs,
 *                                    [2] max in-degree, [3] max out-degree
 * workspace  : cgnn_csr_workspace_bytes() bytes, 16-byte aligned */
int cgnn_csr_build(const int64_t* edge_index, const int64_t* node_graph,
                   int64_t num_nodes, int64_t num_edges,
                   int32_t* rowptr_dst, int32_t* eid_dst, int32_t* col_dst,
                   int32_t* rowptr_src, int32_t* eid_src, int32_t* col_src,
                   int32_t* flags, void* workspace, int64_t workspace_bytes, void* stream);

/* Same outputs as cgnn_csr_build for batches whose COO is grouped by graph: the edges of graph g
 * are exactly the run [eptr[g], eptr[g+1]) and both endpoints lie in [gptr[g], gptr[g+1]) -- what
 * collate_graphs (graph.py:143-167) produces.  One workgroup builds a whole graph in LDS (single
 * pass over the COO, no global atomics): ~10x faster than the generic build at 4096 x 360-ROI.
 * gptr/eptr int32 [B+1]; max_nodes <= 1024, max_edges < 65535 and LDS = 16*(max_nodes+1) +
 * 8*max_edges <= 128 KB, else CGNN_EUNSUPPORTED.  flags as cgnn_csr_build; if flags[0] or flags[1] is non-zero the input
 * was not grouped/block-diagonal and the outputs are incomplete: rebuild with cgnn_csr_build. */
int cgnn_csr_build_grouped(const int64_t* edge_index, const int32_t* gptr, const int32_t* eptr,
                           int32_t num_graphs, int64_t num_nodes, int64_t num_edges,
                           int32_t max_nodes, int32_t max_edges,
                           int32_t* rowptr_dst, int32_t* eid_dst, int32_t* col_dst,
                           int32_t* rowptr_src, int32_t* eid_src, int32_t* col_src,
                           int32_t* flags, void* stream);

/* GCN symmetric normalisation, models.py:94-108: self-loop weight 1 appended last,
 * deg[i] = sum_{e: src=i} w_e + 1 (SOURCE side), dis = (deg + 1e-8)^-1/2,
 * c_e = dis[src]*w_e*dis[dst].  Layer independent -> once per batch.
 * dis [Nn], selfc [Nn] = dis^2, coef_dst [Ee] (dst-CSR slot order), coef_src [Ee]. */
int cgnn_gcn_norm(const int64_t* edge_index, const float* edge_weight,
                  int64_t num_nodes, int64_t num_edges,
                  const int32_t* rowptr_dst, const int32_t* eid_dst,
                  const int32_t* rowptr_src, const int32_t* eid_src,
                  float* dis, float* selfc, float* coef_dst, float* coef_src, void* stream);

/* GraphSAGE weighted-mean normalisation, models.py:146-149:
 * den[d] = sum_{e: dst=d} w_e + 1e-8; w_dst [Ee] = w permuted to dst-CSR slots;
 * coef_src_bwd [Ee] = w_e / den[dst_e] in src-CSR slots (backward of the mean; may be NULL when
 * the caller's backward divides by den itself, as cgnn_aggregate_tiled_f32 does). */
int cgnn_sage_norm(const int64_t* edge_index, const float* edge_weight,
                   int64_t num_nodes, int64_t num_edges,
                   const int32_t* rowptr_dst, const int32_t* eid_dst,
                   const int32_t* rowptr_src, const int32_t* eid_src,
                   float* den, float* w_dst, float* coef_src_bwd, void* stream);

/* ---------------------------------------------------------------------------------------
 * Edge-weighted segment reduction (the "scatter"), models.py:50-54,112-114,146-149.
 *   Y[r, :] = ( sum_{s in row r} coef[s] * X[col[s], :] ) / rowdiv[r]
 *             + selfc[r] * X[r, :] + bias[:]
 * rowdiv, selfc, bias may be NULL (treated as 1, 0, 0).  No atomics: one wave owns a row,
 * slots are summed in order.  The transposed pass (autograd of x[src]) is the same call on
 * the src-sorted CSR.  ldx/ldy are row strides in elements (>= F).
 * ------------------------------------------------------------------------------------- */
int cgnn_aggregate_f32(const int32_t* rowptr, const int32_t* col, const float* coef,
                       const float* selfc, const float* rowdiv, const float* bias,
                       const float* X, int64_t ldx, float* Y, int64_t ldy,
                       int64_t num_rows, int32_t F, void* stream);
/* Y[r, :] += the same sum (F = 64, 128 or 256; else CGNN_EUNSUPPORTED): the edges outside the dense
 * fragments that cgnn_band_aggregate_f32 has just written to Y (below). */
int cgnn_aggregate_acc_f32(const int32_t* rowptr, const int32_t* col, const float* coef,
                           const float* selfc, const float* rowdiv, const float* bias,
                           const float* X, int64_t ldx, float* Y, int64_t ldy,
                           int64_t num_rows, int32_t F, void* stream);

/* ---------------------------------------------------------------------------------------
 * Edge-weight gradients (csrc/edge_grad.hip): the reference's autograd of edge_weight through
 * models.py:94-114 (GCN) and :146-149 (SAGE).  Every aggregate is Y = A_hat X' (+ b); with dY the
 * gradient at its output, per edge e = (s -> d): g_e = <dY[d,:], X'[s,:]>.  No atomics: two
 * identical calls give bit-identical outputs.
 * ------------------------------------------------------------------------------------- */

/* SDDMM over the dst-sorted CSR (rowptr, col): for slot k of row r,
 *     g[eid ? eid[k] : k] = ( <dY[r,:], X[col[k],:]> - t_r ) / rowdiv[r]
 * with t_r = <dY[r,:], Xself[r,:]> and the division only when rowdiv is not NULL (else t_r = 0 and
 * no division): rowdiv = den of cgnn_sage_norm and Xself = the aggregate's output give GraphSAGE's
 * whole dw_e (models.py:146-149) in COO order through eid = eid_dst.  gself [num_rows] (nullable)
 * receives t_r: the GCN self-loop's <dY[i], X'[i]> (models.py:98-100).  Xself is required when
 * rowdiv or gself is given.  Any F >= 1; F = 64 / 128 / 256 with 16-byte aligned rows take the
 * vector path.  Row strides lddy / ldx / ldxs in elements (>= F).  col and g may be NULL only when the
 * CSR has no slots (rowptr all zero). */
int cgnn_sddmm_f32(const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                   const float* dY, int64_t lddy, const float* X, int64_t ldx,
                   const float* Xself, int64_t ldxs, const float* rowdiv, float* g, float* gself,
                   int64_t num_rows, int32_t F, void* stream);

/* Bytes of scratch cgnn_gcn_norm_bwd needs for num_nodes (the per-node ddis). */
int64_t cgnn_gcn_norm_bwd_workspace_bytes(int64_t num_nodes);

/* Backward of cgnn_gcn_norm (models.py:94-108) for one aggregate: from g [Ee] (COO order, cgnn_sddmm_f32
 * with eid = eid_dst), gself [Nn], the COO edge weights w and dis of the forward,
 *     ddis_i = sum_{e: src=i} g_e w_e dis[dst_e] + sum_{e: dst=i} g_e w_e dis[src_e] + 2 dis_i gself_i
 *     dw_e   = g_e dis[src_e] dis[dst_e] - 1/2 dis[src_e]^3 ddis[src_e]          (COO order)
 * ddis goes to `workspace` (cgnn_gcn_norm_bwd_workspace_bytes(Nn) bytes; shorter -> CGNN_EINVAL). */
int cgnn_gcn_norm_bwd(const int32_t* rowptr_dst, const int32_t* col_dst, const int32_t* eid_dst,
                      const int32_t* rowptr_src, const int32_t* col_src, const int32_t* eid_src,
                      const float* edge_weight, const float* dis, const float* g, const float* gself,
                      int64_t num_nodes, int64_t num_edges, float* dw, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Feature projection on the matrix cores (v_mfma_f32_32x32x2_f32: exact fp32),
 * models.py:111 (GCN, no bias) and :151-152 (SAGE: Linear([X || agg]) + bias, ReLU).
 *   fwd        : Y[M,N]  = act( X1[M,K1] W[:, 0:K1]^T + X2[M,K2] W[:, K1:K1+K2]^T + bias )
 *   bwd_input  : dX[M,K] = dY[M,N] W[:, k0:k0+K]        (ldw = K1+K2)
 *   bwd_weight : dW[N, k0:k0+K] = dY^T X                 (partials in `slab`, then reduced
 *                                                          in fp64, deterministic)
 * W is the nn.Linear weight [N, K1+K2] row-major.  X2/K2 = NULL/0 for one panel.
 * relu != 0 applies max(.,0) in the epilogue.
 * ------------------------------------------------------------------------------------- */
int cgnn_linear_fwd_f32(const float* X1, int64_t ldx1, int32_t K1,
                        const float* X2, int64_t ldx2, int32_t K2,
                        const float* W, const float* bias, int32_t relu,
                        float* Y, int64_t ldy, int64_t M, int32_t N, void* stream);

/* cgnn_linear_fwd_f32 that also leaves the BatchNorm statistics of its output behind:
 * stat_slab fp64 [cgnn_fused_grid()][2N] = per-workgroup (sum Y | sum Y^2), the layout
 * cgnn_bn_act_finalize reads -- saves the separate pass of cgnn_bn_act_fwd_stats over Y.
 * Only the tall weight-stationary shapes (M >= 4096, N in {64,128}, K % 32 == 0, K*N <= 32768,
 * 16-byte aligned rows) are covered; others return CGNN_EUNSUPPORTED and launch nothing. */
int cgnn_linear_fwd_stats_f32(const float* X1, int64_t ldx1, int32_t K1,
                              const float* X2, int64_t ldx2, int32_t K2,
                              const float* W, const float* bias, int32_t relu,
                              float* Y, int64_t ldy, int64_t M, int32_t N,
                              double* stat_slab, int64_t stat_slab_bytes, void* stream);

int cgnn_linear_bwd_input_f32(const float* dY, int64_t lddy, const float* W, int32_t ldw,
                              int32_t k0, float* dX, int64_t lddx,
                              int64_t M, int32_t N, int32_t K, void* stream);

/* Bytes of `slab` scratch for cgnn_linear_bwd_weight_f32(M, N, K) / for cgnn_linear_bwd_weight2_f32 with
 * panels K1, K2 (the larger of the joint one-pass form and the per-panel forms it may fall back to). */
int64_t cgnn_linear_bwd_weight_workspace_bytes(int64_t M, int32_t N, int32_t K);
int64_t cgnn_linear_bwd_weight2_workspace_bytes(int64_t M, int32_t N, int32_t K1, int32_t K2);

int cgnn_linear_bwd_weight_f32(const float* dY, int64_t lddy, const float* X, int64_t ldx,
                               float* dW, int32_t ldw, int32_t k0,
                               int64_t M, int32_t N, int32_t K, void* slab, int64_t slab_bytes, void* stream);

/* Both K-panels of dW = dY^T [X1 | X2] in one pass over dY (SAGELayer's Linear(2*in, out)).
 * slab: cgnn_linear_bwd_weight2_workspace_bytes(M, N, K1, K2) bytes. */
int cgnn_linear_bwd_weight2_f32(const float* dY, int64_t lddy, const float* X1, int64_t ldx1,
                                int32_t K1, const float* X2, int64_t ldx2, int32_t K2, float* dW,
                                int32_t ldw, int64_t M, int32_t N, void* slab, int64_t slab_bytes, void* stream);

/* fp16-STORAGE forms of the projection for large dense parcellations (BASELINE config 5; the
 * reference, models.py:111 and its autograd backward, has no fp16 path -- results are the fp32
 * oracle's to fp16 resolution).  Activations X / Y / dY / dX are IEEE half, the weight and its
 * gradient stay fp32 (converted to half once per workgroup while it is laid out as MFMA operands
 * in LDS), accumulation is fp32 on v_mfma_f32_32x32x16_f16.
 *   fwd       : Y[M,N] = X[M,K] W^T + bias   W fp32 [N, Kw] row-major with row stride ldw; columns
 *               k >= Kw of X meet zeros (layer 0's 5 input features ride in a 64-column panel)
 *   bwd_input : dX[M,K] = dY[M,N] W           W fp32 [N, K], row stride ldw
 *   bwd_weight: dW[n*ldw + k] = sum_m dY[m,n] X[m,k] for k < Kw   (fp32 partials per run of rows in
 *               `slab`, cgnn_linear_bwd_weight_f16_workspace_bytes(M,N,K) bytes, folded in fixed
 *               order with fp64 accumulation)
 * Shapes: N, K in {64,128,256} for fwd / bwd_input (K any multiple of 32 <= 256 on the reduction
 * side), N and K in {64,128,256} for bwd_weight; rows 16-byte aligned (ld % 8 == 0).
 * Anything else returns CGNN_EUNSUPPORTED and launches nothing. */
int cgnn_linear_fwd_f16(const void* X, int64_t ldx, int32_t K, const float* W, int32_t ldw, int32_t Kw,
                        const float* bias, void* Y, int64_t ldy, int64_t M, int32_t N, void* stream);
int cgnn_linear_bwd_input_f16(const void* dY, int64_t lddy, const float* W, int32_t ldw, void* dX,
                              int64_t lddx, int64_t M, int32_t N, int32_t K, void* stream);
/* cgnn_linear_fwd_f16 with the BatchNorm statistics of its output left behind by the epilogue
 * (per-workgroup fp64 partials, stat_slab [cgnn_fused_grid()][2 * N]: sum | sum of squares of the
 * half-rounded output columns, N = 128 or 256; combined by cgnn_bn_act_finalize with rows =
 * cgnn_fused_grid()): the projection in front of a BatchNorm (models.py:111,208) needs no statistics pass. */
int cgnn_linear_fwd_stats_f16(const void* X, int64_t ldx, int32_t K, const float* W, int32_t ldw, int32_t Kw,
                              const float* bias, void* Y, int64_t ldy, int64_t M, int32_t N, double* stat_slab, int64_t stat_slab_bytes,
                              void* stream);
int64_t cgnn_linear_bwd_weight_f16_workspace_bytes(int64_t M, int32_t N, int32_t K);
int cgnn_linear_bwd_weight_f16(const void* dY, int64_t lddy, const void* X, int64_t ldx, float* dW,
                               int32_t ldw, int32_t Kw, int64_t M, int32_t N, int32_t K, void* slab, int64_t slab_bytes,
                               void* stream);
/* Y[M, Fp] (half) = [X[M, F] (fp32) | zeros]: the input features of a batch as a half panel. */
int cgnn_pad_cast_f16(const float* X, int64_t ldx, int32_t F, void* Y, int32_t Fp, int64_t M, void* stream);

/* Column sums (bias gradients, models.py:81,114): out[j] = sum_r A[r, j]; fp64 combine.
 * slab: cgnn_colsum_workspace_bytes(M, N) bytes. */
int64_t cgnn_colsum_workspace_bytes(int64_t M, int32_t N);
int cgnn_colsum_f32(const float* A, int64_t lda, float* out, int64_t M, int32_t N,
                    void* slab, int64_t slab_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Per-graph mean-pool readout, models.py:40-47,57-59: P[g,:] = sum_{n in g} X[n,:] / (n_g+1e-8)
 * using the contiguous node ranges gptr (int32 [B+1], = ConnectomeBatch.ptr).
 * ------------------------------------------------------------------------------------- */
int cgnn_pool_mean_fwd_f32(const float* X, int64_t ldx, const int32_t* gptr, float* P,
                           int32_t num_graphs, int32_t F, void* stream);
int cgnn_pool_mean_bwd_f32(const float* dP, const int32_t* gptr, float* dX, int64_t lddx,
                           int32_t num_graphs, int32_t F, void* stream);


/* =======================================================================================
 * FUSED PER-TILE GCN PATH (hidden = 64, fp32): the MI355X-first form of models.py:84-114 +
 * 203-216 and of its autograd backward.
 *
 * A *tile* is a run of consecutive whole graphs with at most CGNN_FUSED_MAX_ROWS nodes; its
 * [rows x 64] fp32 feature tile (<= 96 KB) lives in the CU's 160 KB LDS for the whole layer.
 * One persistent workgroup (8 waves) per CU walks the tiles.  Per layer, HBM sees exactly:
 * read the previous layer's pre-BatchNorm output, read the CSR once, write this layer's
 * pre-BatchNorm output.  BatchNorm-apply + ReLU + dropout are applied while the tile is being
 * staged, the projection runs on the matrix cores out of LDS, BatchNorm statistics are
 * accumulated (fp64) in the epilogue.  The batch-wide BatchNorm reduction is the only global
 * barrier, hence one launch per layer.
 *
 *   forward  l=0 : T = X0 W0^T (MFMA) -> LDS ; Y0 = A_hat T + b                (fwd_first)
 *   forward  l>0 : X = drop(relu(a*Yprev+b)) -> LDS ; Y = (A_hat X) W^T + b    (fwd)
 *   backward l   : dY = BN'(dZ) -> LDS ; dT = A_hat^T dY ; dW += dT^T X ;
 *                  dZprev = (dT W) * drop' * relu'                              (bwd, bwd_first)
 *
 * `bn` blocks are float[4*64]: a = gamma*invstd | b = beta - mean*a | mean | invstd.
 * `bwc` blocks are float[2*64]: c1 = sum(dZ)/N | c2 = sum(dZ*xhat)/N.
 * Dropout keep-bits are produced by a counter-based hash of (seed, element) when a layer's
 * output is first consumed and stored as one byte per (node, 4-column chunk) in `mask`
 * ([Nn*16] bytes); mask == NULL or p == 0 means no dropout.
 * Per-workgroup partial sums go to `*_slab` arrays with cgnn_fused_grid() rows and are
 * combined by cgnn_slab_reduce_* / cgnn_bn_reduce in a fixed order (deterministic, no atomics).
 * ===================================================================================== */
#define CGNN_FUSED_HIDDEN   64
#define CGNN_FUSED_MAX_ROWS 384
#define CGNN_FUSED_MAX_F0   16

/* Blocked-ELL metadata of one edge ordering (rows = destinations for forward, rows = sources
 * for the transposed passes).  Rows are grouped in 16-row blocks aligned to the start of each
 * tile; block b stores width_b = max degree in the block + 1 steps of 16 entries each
 * (entry (s, i) at blk_off[b] + 16*s + i), every entry 8 bytes:
 *     uint32 lds_offset = 256 * (neighbour's row inside the tile)   float weight
 * A row's real edges come first in COO order, then its self-loop (weight 1), then zero-weight
 * padding, so the kernels' inner loop is branch-free and sums in the reference's order.
 * Built once per batch (the weights are the raw edge weights; the symmetric normalisation is
 * applied as  dis[d] * sum_e w_e * (dis[s_e] * x[s_e])  with `dis` recomputed every step). */

/* Pass 1: widths + exclusive scan.  tile_ptr/tile_blk int32 [T+1] (tile_blk = prefix of
 * ceil(rows/16), NB = num_blocks = tile_blk[T]), rowptr int32 [Nn+1] of the ordering.
 * blk_off int32 [NB+1] out (in entries); scratch: int32 [NB/2048 + 8]. */
int cgnn_bell_plan(const int32_t* tile_ptr, const int32_t* tile_blk, int32_t num_tiles,
                   int32_t num_blocks, const int32_t* rowptr, int32_t* blk_off, int32_t* scratch, int64_t scratch_bytes,
                   void* stream);
/* Pass 2: fill entries (8 bytes each, blk_off[NB] of them).  self_weight: weight of the appended
 * self-loop entry -- 1 for GCN (models.py:97-100), 0 for GraphSAGE (no self-loop, models.py:146). */
int cgnn_bell_fill(const int32_t* tile_ptr, const int32_t* tile_blk, int32_t num_tiles,
                   const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                   const float* edge_weight, float self_weight, const int32_t* blk_off,
                   void* entries, void* stream);

/* out[i] = src[idx[i]] (edge weights permuted to CSR slot order, once per batch). */
int cgnn_gather_f32(const float* src, const int32_t* idx, int64_t n, float* out, void* stream);

/* Several row gathers by one id list in ONE launch: dst[j][i] = src[j][ids[i]] for rows of
 * row_bytes[j] bytes (a multiple of 4; pointers 4-byte aligned).  The on-device form of the
 * reference's collate for device-resident regular datasets (graph.py:143-167 stacks node features and
 * labels per graph) extended to the per-subject structure arrays: node features, labels, blocked-ELL
 * block offsets and `dis` of a batch leave in one kernel.
 * ids_offset (nullable, device): the id list starts at ids + *ids_offset -- a captured step reads the
 * batch's position in the epoch's permutation from a device cursor, so replays need no host copy. */
#define CGNN_GATHER_MAX_JOBS 8
typedef struct cgnn_gather_jobs {
  int32_t n;
  const void* src[CGNN_GATHER_MAX_JOBS];
  void* dst[CGNN_GATHER_MAX_JOBS];
  int64_t row_bytes[CGNN_GATHER_MAX_JOBS];
} cgnn_gather_jobs;
int cgnn_gather_rows(const cgnn_gather_jobs* jobs, const int64_t* ids, int32_t num_ids,
                     const int64_t* ids_offset, void* stream);
/* End-of-step bookkeeping of an epoch replayed from one captured step (reference train.py:52-54 keeps
 * the running loss on the host): *tally += *loss * weight (tally nullable), *cursor += step. */
int cgnn_epoch_advance(int64_t* cursor, int64_t step, const float* loss, float weight, float* tally,
                       void* stream);

/* The COO of a batch from a device-resident dataset whose subjects keep different numbers of edges -- the
 * on-device form of collate_graphs (graph.py:143-167), bit-identical to it.  The dataset holds subject i's
 * edges as the run [edge_ptr[i], edge_ptr[i+1]) of edge_local (int64 [2, ds_edges], node ids local to the
 * graph) and edge_weight_ds (float [ds_edges]); every subject has n nodes.  For the b subject ids:
 *     eptr[g+1] - eptr[g]           = edge_ptr[ids[g]+1] - edge_ptr[ids[g]],  eptr[0] = 0   (int32 [b+1])
 *     edge_index[r][eptr[g] + j]    = edge_local[r][edge_ptr[ids[g]] + j] + g * n           (r = 0, 1)
 *     edge_weight[eptr[g] + j]      = edge_weight_ds[edge_ptr[ids[g]] + j]
 * eptr is COMPUTED HERE, on the device (one workgroup scans the counts ahead of the copy, same stream): it is
 * an output -- the form cgnn_csr_build_grouped takes -- not an input.  num_edges is the batch's edge count as
 * the caller's host copy of edge_ptr gives it: it sizes the launch, is the row stride of edge_index
 * ([2, num_edges]) and bounds every write (sums beyond it are cut off; a subject id outside [0, num_subjects)
 * or a run outside [0, ds_edges] counts as empty).  The three outputs come with their byte counts; a short or
 * NULL buffer, b < 0, n <= 0, b * n or num_edges >= 2^31 return CGNN_EINVAL before any launch.  b == 0 or
 * num_edges == 0: CGNN_OK, nothing launched, nothing written (eptr of such a batch is all zeros).
 * edge_index and edge_weight 16-byte aligned.  The copy walks chunks of CGNN_COLLATE_CHUNK edges of the
 * batch's flat edge range with a grid stride over 4 * cgnn_fused_grid() workgroups, a thread moving
 * CGNN_COLLATE_VEC edges with 16-byte accesses; eptr is searched in LDS for b <= CGNN_COLLATE_LDS_GRAPHS. */
#define CGNN_COLLATE_VEC 4
#define CGNN_COLLATE_CHUNK 1024
#define CGNN_COLLATE_LDS_GRAPHS 4096
int cgnn_collate_edges(const int64_t* edge_local, const float* edge_weight_ds, const int64_t* edge_ptr,
                       int64_t num_subjects, int64_t ds_edges, const int64_t* ids, int32_t b, int32_t n,
                       int64_t num_edges, int64_t* edge_index, int64_t edge_index_bytes,
                       float* edge_weight, int64_t edge_weight_bytes, int32_t* eptr, int64_t eptr_bytes,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * A device-resident cohort of dense connectivity matrices -> the flat edge arrays above (DESIGN.md 4.3b;
 * the step the reference README's "Extending to real HCP data" leaves to a host loop).
 * matrices: float [S, n, n], contiguous, any sign, not necessarily symmetric.  For subject s with matrix A:
 *   candidates  the n(n-1) off-diagonal entries; a NaN candidate ranks as -inf
 *   threshold   t_s = the candidate of descending rank k, 0-based (the (k+1)-th largest); -inf when
 *               k >= n(n-1) or when the rank falls on a NaN -- or t_s is given (absolute thresholding)
 *   edges       i -> j  iff  i != j, A[i,j] > t_s and A[i,j] > 0, compared as floats, both strict (a NaN
 *               fails both): at most k edges, fewer when ties straddle the threshold
 *   order       row-major (i ascending, then j ascending)
 * Three calls, each enqueued on `stream`; every written buffer comes with its byte count; a NULL or short
 * buffer, S < 0, n <= 0, k < 0, S * n >= 2^31 or n * n >= 2^31 return CGNN_EINVAL before any launch;
 * S == 0 returns CGNN_OK with nothing launched.  Element offsets into `matrices` are 64-bit.
 *
 * cgnn_ingest_select: thr[s] = t_s (float [S]).  An exact radix select per subject on an order-preserving
 *   uint32 image of the floats (three passes of 11/11/10 bits, histogram in LDS): no sort, no workspace.  One
 *   workgroup owns a subject; 3 * cgnn_fused_grid() workgroups walk the subjects with a grid stride.
 * cgnn_ingest_count: row_count[s * n + i] (int32 [S * n]) = edges leaving node i of subject s.  select != 0:
 *   thr is an OUTPUT, selected as above for k by the same workgroup just before it counts (one pass over HBM
 *   per subject); select == 0: thr is an INPUT (k must still be >= 0 and is not used).
 *   strength (nullable, float [S * n] = the default node feature [S, n, 1]): strength_i / (max_i strength_i +
 *   1e-8) with strength_i = the sum of the kept A[i, j] over j (ConnectomeGraph.degree()); zeros for a subject
 *   without edges.
 * cgnn_ingest_fill: row_off (int64 [S * n + 1]) = the exclusive running sum of row_count over all rows of all
 *   subjects, num_edges = row_off[S * n] as the caller read it back: edge_local[0][p] = i, edge_local[1][p] = j
 *   (int64 [2, num_edges]), edge_weight[p] = A[i,j] for the kept entries of row (s, i) at p = row_off[s*n + i]
 *   onwards in column order, placed by ballot + lane prefix (a wave per row; no atomics: the same bits on
 *   every run).  Positions outside [0, num_edges) are not written.  num_edges == 0: CGNN_OK, nothing launched;
 *   num_edges > S n (n-1): CGNN_EINVAL.  The edge pointer of a RaggedPackedDataset is row_off[0 :: n].
 * ------------------------------------------------------------------------------------- */
int cgnn_ingest_select(const float* matrices, int64_t S, int32_t n, int64_t k, float* thr, int64_t thr_bytes,
                       void* stream);
int cgnn_ingest_count(const float* matrices, int64_t S, int32_t n, int32_t select, int64_t k, float* thr,
                      int64_t thr_bytes, int32_t* row_count, int64_t row_count_bytes, float* strength,
                      int64_t strength_bytes, void* stream);
int cgnn_ingest_fill(const float* matrices, int64_t S, int32_t n, const float* thr, const int64_t* row_off,
                     int64_t num_edges, int64_t* edge_local, int64_t edge_local_bytes, float* edge_weight,
                     int64_t edge_weight_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * A device-resident cohort of ROI time series -> Pearson correlation matrices, the input of the three calls
 * above.  ts: float [S, T, n], contiguous, one row per frame.
 *   units    without a window (window == 0) one unit per subject over all T frames; with window = L in [2, T]
 *            and stride >= 1, W = (T - L) / stride + 1 units per subject, unit u = s * W + w covering frames
 *            [w * stride, w * stride + L).  U = S * W.
 *   per unit m_i = the mean of column i and q_i = sum_t (x[t,i] - m_i)^2, both accumulated in fp64 as centred
 *            sums (blocks of 8 frames centred in registers and merged pairwise: one read, no E[x^2] - E[x]^2);
 *            r[i,j] = sum_t z[t,i] z[t,j], z[t,i] = (x[t,i] - m_i) / sqrt(q_i), operands centred and scaled in
 *            fp32, products on the fp32 matrix pipe, fp32 accumulation over t ascending.  No atomics: the same
 *            bits on every run and for every grid.
 *   output   out: float [U, n, n].  r[i,j] and r[j,i] are the same bits (one is the mirror store of the other);
 *            off-diagonals are clamped to [-1, 1]; r[i,i] is exactly 1.  A column with q_i == 0 has 1/sqrt(q_i)
 *            taken as 0: its row and column, diagonal included, are exactly 0.  absolute != 0 stores |r|.
 *            Non-finite inputs are not checked and propagate.
 *   stats    workspace, float [U, n, 2] = (m_i, 1/sqrt(q_i)) per unit and column, written by the first of the
 *            two launches and read by the second (a persistent grid of 2 * cgnn_fused_grid() workgroups over
 *            the (unit, 96 x 96 tile pair bi <= bj) items).
 * A NULL or short buffer, S < 0, n <= 0, T < 2, window outside {0} u [2, T], stride < 1 with a window,
 * U * n >= 2^31 or n * n >= 2^31 return CGNN_EINVAL before any launch; S == 0 returns CGNN_OK with nothing
 * launched and nothing written.  Element offsets into ts and out are 64-bit.
 * ------------------------------------------------------------------------------------- */
int cgnn_ingest_corr(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride,
                     int32_t absolute, float* stats, int64_t stats_bytes, float* out, int64_t out_bytes,
                     void* stream);

/* ---------------------------------------------------------------------------------------
 * Graph-theoretic node features of the thresholded cohort.  matrices: float [S, n, n] as above;
 * thr: float [S], the thresholds cgnn_ingest_select / cgnn_ingest_count left or the caller's.  Per subject with
 * matrix A and threshold t:
 *   e_ij    iff i != j, A_ij > t and A_ij > 0 (the edge test above; a NaN is never an edge)
 *   a_ij = A_ij, b_ij = 1 where e_ij, else 0;  k_i = sum_j b_ij;  s_i = sum_j a_ij;  wmax = max a_ij;
 *   u_ij = cbrt(a_ij / wmax) where e_ij, else 0 (evaluated in fp32 as cbrt(a_ij) * (1 / cbrt(wmax)));
 *   for a value map v:  T_i(v) = sum_{j,k} v_ki v_kj v_ij
 *   CGNN_MEASURE_STRENGTH             s_i / (max_i s_i + 1e-8): the bits of cgnn_ingest_count's strength
 *   CGNN_MEASURE_DEGREE               k_i / (n - 1); 0 for n == 1
 *   CGNN_MEASURE_MEAN_WEIGHT          s_i / (k_i + 1e-8)
 *   CGNN_MEASURE_CLUSTERING           T_i(b) / (k_i (k_i - 1)) if k_i >= 2, else 0
 *   CGNN_MEASURE_WEIGHTED_CLUSTERING  T_i(u) / (k_i (k_i - 1)) if k_i >= 2, else 0 (Onnela's geometric-mean form
 *                                     on weights scaled by the subject's maximum)
 * For a symmetric kept set T_i(v) = diag(V^3)_i and the two clustering measures are the local clustering
 * coefficients of the graph; for an asymmetric matrix the formula is the definition (nothing is symmetrised, the
 * value is not bounded by 1).  A subject without edges gives zeros.  A kept +inf propagates as IEEE says through the
 * weight-valued measures; degree and clustering do not see weights: T_i(b) is an exact integer below 2^24.
 *   measures   HOST array of num_measures distinct ids, 1 <= num_measures <= CGNN_NUM_MEASURES: the columns of x
 *   x          float [S, n, num_measures]
 *   workspace  cgnn_ingest_measures_workspace_bytes(S, n, measures, num_measures) bytes, 16-byte aligned: k_i, s_i,
 *              (max_i s_i, wmax) and, per clustering measure asked for, the partial sums float [S, nt, nt * 96],
 *              nt = ceil(n / 96)
 * Launches on `stream`: a row pass (k_i, s_i, wmax; the row summation of cgnn_ingest_count); per clustering measure
 * asked for one product kernel -- a persistent grid of 2 * cgnn_fused_grid() workgroups over the (subject, 96 x 96
 * tile pair bi <= bj) items of V^T V, K-steps of 32 matrix rows on the fp32 matrix pipe, the edge test and the
 * value map applied as the panels are staged; the item (min(blk(i), b), max(blk(i), b)) writes partial [s][b][i],
 * exactly once -- and a finish that sums each node's nt partials in ascending b.  No atomics: the same bits on every
 * run and for every grid.  A NULL, misaligned or short buffer, S < 0, n <= 0, S * n >= 2^31, n * n >= 2^31,
 * num_measures outside [1, CGNN_NUM_MEASURES], an id outside [0, CGNN_NUM_MEASURES) or a repeated id return
 * CGNN_EINVAL before any launch (the byte count: a negative value); S == 0 returns CGNN_OK with nothing launched.
 * Element offsets into `matrices` are 64-bit.
 * ------------------------------------------------------------------------------------- */
#define CGNN_MEASURE_STRENGTH 0
#define CGNN_MEASURE_DEGREE 1
#define CGNN_MEASURE_MEAN_WEIGHT 2
#define CGNN_MEASURE_CLUSTERING 3
#define CGNN_MEASURE_WEIGHTED_CLUSTERING 4
#define CGNN_NUM_MEASURES 5
int64_t cgnn_ingest_measures_workspace_bytes(int64_t S, int32_t n, const int32_t* measures, int32_t num_measures);
int cgnn_ingest_measures(const float* matrices, int64_t S, int32_t n, const float* thr, const int32_t* measures,
                         int32_t num_measures, void* workspace, int64_t workspace_bytes, float* x, int64_t x_bytes,
                         void* stream);

/* ---------------------------------------------------------------------------------------
 * Shortest-path node measures of the thresholded cohort.  matrices and thr as for
 * cgnn_ingest_measures; weights play no part beyond the edge test.  Per subject with matrix A and threshold t:
 *   e_ij    iff i != j, A_ij > t and A_ij > 0 (the edge test above; a NaN is never an edge, a kept +inf is an
 *           ordinary edge); nothing is symmetrised
 *   d_ij    the number of edges on a shortest directed path i -> ... -> j along kept edges (the out-neighbours of
 *           a row), infinite if there is none
 *   R_i = { j != i : d_ij finite }, r_i = |R_i|;  N_i = { j : e_ij }, k_i = |N_i|
 *   d^(i)   the distances inside the subgraph induced on N_i (only edges e_jh with both ends in N_i)
 *   CGNN_PATH_NODAL_EFFICIENCY  (1 / (n - 1)) sum_{j in R_i} 1 / d_ij; 0 for n == 1
 *   CGNN_PATH_CLOSENESS         (r_i / (n - 1)) (r_i / sum_{j in R_i} d_ij) if r_i > 0, else 0 (Wasserman-Faust)
 *   CGNN_PATH_ECCENTRICITY      max_{j in R_i} d_ij / (n - 1); 0 if r_i == 0 or n == 1
 *   CGNN_PATH_LOCAL_EFFICIENCY  (1 / (k_i (k_i - 1))) sum_{j != h in N_i} 1 / d^(i)_jh if k_i >= 2, else 0
 *                               (unreachable pairs add 0)
 * All values lie in [0, 1]; a subject without edges gives zeros.  Level counts, r_i, sum d (<= n (n - 1) / 2 < 2^24)
 * and the eccentricity are exact integers: eccentricity is the correctly rounded fp32 quotient of two of them; the
 * other three are formed in fp64 from the integers (sum_l count_l / l in ascending l) and rounded to fp32 once.
 *   measures   HOST array of num_measures distinct ids, 1 <= num_measures <= CGNN_NUM_PATH_MEASURES
 *   cols, ldx  HOST array of num_measures distinct columns in [0, ldx): measure m of node i of subject s is written
 *              to x[(s * n + i) * ldx + cols[m]]; the other columns of x are not touched, so the path measures land
 *              inside a wider feature tensor
 *   x          float [S, n, ldx]
 *   workspace  cgnn_ingest_paths_workspace_bytes(S, n, measures, num_measures) bytes, 16-byte aligned.  The one
 *              kernel keeps its state in LDS and registers: the count is 0 today and workspace may then be NULL.
 * One launch on `stream`: min(S, w * cgnn_fused_grid()) workgroups of 8 waves (w = what the LDS of a CU admits, at
 * most 4), a workgroup per subject with a grid stride.  It builds the subject's out-neighbour bitset [n][ceil(n / 64)]
 * x 64 bits in LDS (one wave-wide ballot of the edge test per word), runs a level-synchronous BFS from every source
 * over word-wide OR / AND-NOT and popcounts (2^ceil(log2 ceil(n / 64)) lanes own a source), and for the local
 * efficiency the same BFS confined to N_i from every j in N_i: ~ n k^2 ceil(n / 64) word reads per subject, which grows
 * with the density.  No atomics, nothing depends on the grid: the same bits on every run and for every grid.
 * n > CGNN_PATH_MAX_NODES (the bitset must fit LDS: 128 KB at 1024), a NULL, misaligned or short buffer, S < 0,
 * n <= 0, S * n >= 2^31, num_measures outside [1, CGNN_NUM_PATH_MEASURES], an unknown or repeated id, ldx < 1, a
 * column outside [0, ldx) or a repeated column return CGNN_EINVAL before any launch (the byte count: a negative
 * value); S == 0 returns CGNN_OK with nothing launched.  Element offsets into `matrices` and `x` are 64-bit.
 * ------------------------------------------------------------------------------------- */
#define CGNN_PATH_NODAL_EFFICIENCY 0
#define CGNN_PATH_CLOSENESS 1
#define CGNN_PATH_ECCENTRICITY 2
#define CGNN_PATH_LOCAL_EFFICIENCY 3
#define CGNN_NUM_PATH_MEASURES 4
#define CGNN_PATH_MAX_NODES 1024
int64_t cgnn_ingest_paths_workspace_bytes(int64_t S, int32_t n, const int32_t* measures, int32_t num_measures);
int cgnn_ingest_paths(const float* matrices, int64_t S, int32_t n, const float* thr, const int32_t* measures,
                      int32_t num_measures, const int32_t* cols, int32_t ldx, void* workspace,
                      int64_t workspace_bytes, float* x, int64_t x_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Weighted shortest-path node measures of the thresholded cohort.  matrices and thr as for
 * cgnn_ingest_measures.  Everything is per subject, with matrix A, threshold t and the existing edge test: e_ij iff
 * i != j, A_ij > t and A_ij > 0.  Nothing is symmetrised.
 * Connection lengths
 *   wmax = max_{e_ij} A_ij.
 *   l_ij = wmax / A_ij where e_ij, formed as one correctly rounded fp32 division.  Otherwise l_ij = +inf.
 *   So every length is >= 1, and the strongest edge has length exactly 1.0.
 *   Scaling a subject's matrix by a constant changes nothing.  This is the same normalisation that
 *   CGNN_MEASURE_WEIGHTED_CLUSTERING uses.
 *   If all kept weights are equal, every length is exactly 1 and the weighted measures reduce to the binary ones.
 * Distances
 *   dw_ij is the smallest sum of lengths along a directed path i -> ... -> j of kept edges.
 *   dw_ii = 0.
 *   dw_ij = +inf when there is no path.
 *   R_i = { j != i : dw_ij finite } and r_i = |R_i|.  This is the same set as the binary R_i.
 * Measures
 *   CGNN_WPATH_NODAL_EFFICIENCY  (1 / (n - 1)) sum_{j in R_i} 1 / dw_ij.  It is 0 for n == 1.
 *   CGNN_WPATH_CLOSENESS         (r_i / (n - 1)) (r_i / sum_{j in R_i} dw_ij) if r_i > 0, else 0 (Wasserman-Faust).
 *   CGNN_WPATH_ECCENTRICITY      max_{j in R_i} dw_ij / (n - 1).  It is 0 if r_i == 0 or n == 1.  It may exceed 1.
 * Special cases
 *   A subject without edges gives zeros.
 *   NaN entries are never edges.
 *   A subject with a kept non-finite weight gets unspecified values in these columns.  The call must still return,
 *   which a fixed round count guarantees.
 * Arithmetic
 *   Distances are fp32 sums of fp32 lengths.
 *   The three row reductions (sum 1/dw, sum dw, the max) are taken in fp64 in a fixed order and rounded to fp32 once.
 *   No atomics.
 *   No work assignment depends on the grid, so every run and every grid gives the same bits.
 *
 *   measures   HOST array of num_measures distinct ids, 0 <= num_measures <= CGNN_NUM_WPATH_MEASURES; 0 (measures,
 *              cols and x may then be NULL) when only `dist` is asked for
 *   cols, ldx  as for cgnn_ingest_paths: measure m of node i of subject s is written to
 *              x[(s * n + i) * ldx + cols[m]]; the other columns of x are not touched
 *   x          float [S, n, ldx]
 *   dist       float [S, n, n] or NULL: dw itself, +inf where unreachable, a zero diagonal.  At least one of x and
 *              dist is required.
 *   workspace  cgnn_ingest_wpaths_workspace_bytes(S, n, measures, num_measures) bytes, 16-byte aligned: one distance
 *              slab float [npad][npad] per WORKGROUP of the launch (not per subject), npad = n rounded up to the
 *              block size; the count depends on cgnn_fused_grid() as it is when the call is made
 * One launch on `stream`: min(S, w * cgnn_fused_grid()) workgroups of 8 waves (w = what the LDS of a CU admits, at
 * most 4), a workgroup per subject with a grid stride, a batched blocked Floyd-Warshall (min-plus) on the subject's
 * slab.  Blocks of 32 nodes while n rounded up to 32 is at most 512, of 16 beyond: the two panels of a round,
 * 2 * block * npad floats, stay in LDS (136 KB at the largest n of either rule).  npad^3 relaxations per subject
 * whatever the density.
 * n > CGNN_WPATH_MAX_NODES, a NULL, misaligned or short buffer (the workspace included), S < 0, n <= 0,
 * S * n >= 2^31, num_measures outside [0, CGNN_NUM_WPATH_MEASURES], an unknown or repeated id, ldx < 1, a column
 * outside [0, ldx) or a repeated column, or neither x nor dist return CGNN_EINVAL before any launch (the byte count: a
 * negative value); S == 0 returns CGNN_OK with nothing launched.  Element offsets are 64-bit.
 * ------------------------------------------------------------------------------------- */
#define CGNN_WPATH_NODAL_EFFICIENCY 0
#define CGNN_WPATH_CLOSENESS 1
#define CGNN_WPATH_ECCENTRICITY 2
#define CGNN_NUM_WPATH_MEASURES 3
#define CGNN_WPATH_MAX_NODES 1024
int64_t cgnn_ingest_wpaths_workspace_bytes(int64_t S, int32_t n, const int32_t* measures, int32_t num_measures);
int cgnn_ingest_wpaths(const float* matrices, int64_t S, int32_t n, const float* thr, const int32_t* measures,
                       int32_t num_measures, const int32_t* cols, int32_t ldx, void* workspace,
                       int64_t workspace_bytes, float* x, int64_t x_bytes, float* dist, int64_t dist_bytes,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * Partial-correlation matrices from correlation matrices.  matrices: float [U, n, n], as
 * cgnn_ingest_corr writes them (signed).  Per unit with matrix R, read from its UPPER triangle (i <= j) only:
 *   excluded   ROI i iff R_ii == 0 (a constant column: the zero row and column of cgnn_ingest_corr).  Its pivot is
 *              taken as 1, so the others are untouched; its row and column of the output, diagonal included, are 0.
 *   C          (1 - shrinkage) R + shrinkage I over the ROIs that are not excluded, shrinkage in [0, 1]
 *   output     P = C^-1;  out_ij = -P_ij / sqrt(P_ii P_jj) clamped to [-1, 1] for i != j, out_ii = 1 exactly; out_ij
 *              and out_ji are the same bits (one is the mirror store of the other); absolute != 0 stores |out|.
 *   failure    a unit whose factorisation meets a pivot that is not > 0 (a NaN is not), or a P_ii that is not finite
 *              and positive, gets an all-NaN matrix.  The round counts are fixed: the call always returns.
 *   arithmetic C = U^T U, W = U^-T, P = W^T W.  Storage and products are fp32, every sum k ascending, the trailing
 *              updates and W^T W on the fp32 matrix pipe.  The reciprocal pivots 1 / u_kk, the shrunk diagonal and the
 *              scales 1 / sqrt(P_ii) (P_ii summed in fp64) are formed in fp64 and rounded to fp32 once.
 *   out        float [U, n, n]; may be `matrices` itself: a unit is read whole before its first entry is written
 *   workspace  cgnn_ingest_partial_workspace_bytes(U, n) bytes, 16-byte aligned: one slab float [npad][npad] per
 *              WORKGROUP of the launch (not per unit), npad = n rounded up to 32; the count depends on
 *              cgnn_fused_grid() as it is when the call is made
 * One launch on `stream`: min(U, w * cgnn_fused_grid()) workgroups of 4 waves (w = what the LDS of a CU admits), a
 * workgroup per unit with a grid stride: a right-looking blocked factorisation of [C | I] in blocks of 32 (the row
 * panel of a round, 32 * (npad + 16) floats, stays in LDS: 151 KB of it at n = 1024), then the 96 x 96 tile walk of
 * cgnn_ingest_corr over W^T W.  ~ n^3 multiply-adds per unit.  No atomics, nothing depends on the grid: the same bits
 * on every run and for every grid.
 * n > CGNN_PARTIAL_MAX_NODES, a NULL, misaligned or short buffer (the workspace included), U < 0, n <= 0,
 * U * n >= 2^31, shrinkage outside [0, 1] or NaN return CGNN_EINVAL before any launch (the byte count: a negative
 * value); U == 0 returns CGNN_OK with nothing launched.  Element offsets are 64-bit.
 * ------------------------------------------------------------------------------------- */
#define CGNN_PARTIAL_MAX_NODES 1024
int64_t cgnn_ingest_partial_workspace_bytes(int64_t U, int32_t n);
int cgnn_ingest_partial(const float* matrices, int64_t U, int32_t n, double shrinkage, int32_t absolute,
                        void* workspace, int64_t workspace_bytes, float* out, int64_t out_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * A shrinkage per unit: cgnn_ingest_partial with shrinkage[u], double [U] on the device and 8-byte
 * aligned, in place of the one scalar.  The kernel reads shrinkage[u] when it starts unit u; the host never does.  A
 * unit whose value is not in [0, 1] (a NaN is not) takes the failure path: an all-NaN matrix, its neighbours untouched.
 * A unit whose value equals the scalar of cgnn_ingest_partial gets the bits of that call.  The workspace, its query, the
 * launch and every other refusal are cgnn_ingest_partial's; a NULL or misaligned shrinkage returns CGNN_EINVAL.
 * ------------------------------------------------------------------------------------- */
int cgnn_ingest_partial_each(const float* matrices, int64_t U, int32_t n, const double* shrinkage, int32_t absolute,
                             void* workspace, int64_t workspace_bytes, float* out, int64_t out_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * The Ledoit-Wolf shrinkage of every unit, estimated from its frames: what cgnn_ingest_partial_each
 * takes.  ts, S, T, n, window, stride: as given to cgnn_ingest_corr, which defines the units; stats: float [U, n, 2],
 * the statistics that call left; matrices: float [U, n, n], the SIGNED correlations it wrote (absolute == 0).
 *   per unit   of L frames, with z[t,i] = (x[t,i] - m_i) rs_i formed in fp32 as cgnn_ingest_corr stages it (rs_i = 0 for
 *              a constant column) and R the unit's matrix, so that the estimate is for the R that was built:
 *                p   = the number of columns with rs_i != 0
 *                s_t = sum_i z[t,i]^2,   B = L sum_t s_t^2
 *                O   = 2 sum_{i<j} R_ij^2 (from the entries above the diagonal, never as F - p),   F = p + O
 *                a   = 0 if O == 0, else (B - F) / (L O) clipped to [0, 1]
 *              This is sklearn.covariance.ledoit_wolf_shrinkage of the standardised frames (the constant columns
 *              left out), whose target mu I is the identity cgnn_ingest_partial shrinks towards.  Squares, sums and the
 *              quotient are fp64.  L == 2 makes B - F zero identically: a = 0 there, not what rounding leaves.  n == 1
 *              or a single column that is not constant gives O == 0 and a = 0.  Non-finite inputs are not checked: a
 *              NaN in a unit's sums gives that unit a NaN (which cgnn_ingest_partial_each turns into an all-NaN unit).
 *   output     alpha: double [U], 8-byte aligned, alpha_bytes >= 8 U.
 * One launch on `stream`: min(U, 4 * cgnn_fused_grid()) workgroups of 4 waves, a workgroup per unit with a grid stride;
 * one read of the unit's frames (a wave per frame, a lane per column) and one of the upper triangle of its matrix.
 * Overlapping windows read their frames again.  No atomics, every merge in a fixed order, nothing depends on the grid:
 * the same bits on every run and for every grid.
 * n > CGNN_PARTIAL_MAX_NODES (the unit's statistics wait in LDS; the estimate feeds a call with that bound), a NULL,
 * misaligned or short buffer, S < 0, n <= 0, T < 2, window outside {0} u [2, T], stride < 1 with a window or
 * U * n >= 2^31 return CGNN_EINVAL before any launch; S == 0 returns CGNN_OK with nothing launched.  Element offsets
 * into ts and matrices are 64-bit.
 * ------------------------------------------------------------------------------------- */
int cgnn_ingest_shrinkage(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride,
                          const float* stats, const float* matrices, double* alpha, int64_t alpha_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Band-pass / detrend of ROI time series by projection on the orthonormal DCT-II basis: what comes
 * in front of cgnn_ingest_corr.  ts: float [S, T, n] as cgnn_ingest_corr takes it.  Per subject and column i, on the T
 * frames of the whole run:
 *   basis      b_k[t] = sqrt(2 / T) cos(pi (2 t + 1) k / (2 T)), k = 1 .. T - 1 (component k: k / (2 T t_r) Hz): an
 *              fp64 cospi of the exactly reduced argument ((2 t + 1) k mod 4 T) / (2 T), scaled in fp64, rounded to
 *              fp32 once
 *   centring   m_i = the column mean, summed in fp64 in a fixed order; xc[t,i] = fl32(double(x[t,i]) - m_i)
 *   comps      K ascending components in [1, T - 1], a HOST array the call reads before it returns
 *   output     complement == 0:  y = sum_{k in comps} b_k (b_k . xc)        (the components are what is kept)
 *              complement != 0:  y = xc - sum_{k in comps} b_k (b_k . xc)   (the components are what is dropped)
 *              K == 0 with complement != 0 is pure centring, y = xc, and launches no product.
 *   arithmetic the products on the fp32 matrix pipe, every sum in ascending order of its index.  Columns never mix: a
 *              constant column gives exactly 0 in every frame, a non-finite entry makes its own column of its own
 *              subject non-finite and changes no other bit.
 *   out        float [S, T, n]; may be `ts` itself (a workgroup owns all T frames of the columns it writes); any other
 *              overlap is not checked
 *   workspace  cgnn_ingest_filter_workspace_bytes(S, T, n, K) bytes, 16-byte aligned: the basis table float [T, Kpad]
 *              (Kpad = K rounded up to 32) and the means double [S, n]; nothing cohort-sized
 * Launches on `stream`: the table (K > 0), the means (a streaming pass of its own: a lane per column, a wave per frame
 * phase, merged in wave order), then a persistent grid over the items (subject, 64 columns), grid stride: the
 * coefficients C = B^T xc [Kpad, 64] with the frames 32 at a time, kept in LDS, then y chunk by chunk of 32 frames (the
 * complement form reads x again).  No atomics, nothing depends on the grid: the same bits on every run and for every
 * grid.
 * K > CGNN_FILTER_MAX_COMPONENTS, K < 0, K == 0 with complement == 0 (nothing is kept), a component outside
 * [1, T - 1] or not ascending, T < 2, T > 2^30, S < 0, n <= 0, S * n >= 2^31, a NULL, misaligned or short buffer
 * return CGNN_EINVAL before any launch (the byte count: a negative value); S == 0 returns CGNN_OK with nothing
 * launched.  Element offsets are 64-bit.
 * ------------------------------------------------------------------------------------- */
#define CGNN_FILTER_MAX_COMPONENTS 256
int64_t cgnn_ingest_filter_workspace_bytes(int64_t S, int32_t T, int32_t n, int32_t K);
int cgnn_ingest_filter(const float* ts, int64_t S, int32_t T, int32_t n, const int32_t* comps, int32_t K,
                       int32_t complement, void* workspace, int64_t workspace_bytes, float* out, int64_t out_bytes,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * Confound regression of ROI time series: head motion, tissue signals and their expansions taken out
 * of every column, per subject.  Two calls: the orthonormal basis of a subject's confounds, and its projection out of
 * the frames by cgnn_ingest_filter's kernel in complement form with a table per subject.
 *
 * cgnn_ingest_confound_basis.  confounds: float [S, T, q], one row per frame, 1 <= q <= CGNN_CONFOUND_MAX.  Per subject,
 * in fp64:
 *   norms      m_j = the mean of column j, cc_j = c_j - m_j, s_j = sqrt(sum_t cc_j[t]^2).  A column with s_j == 0 (exactly
 *              constant) is dropped; the others are u_j = cc_j / s_j.
 *   basis      Gram-Schmidt in the given order: r_j = u_j - sum_{k < j, kept} q_k (q_k . u_j), d_j = |r_j|^2; column j is
 *              kept iff d_j > CGNN_CONFOUND_RANK_TOL, and then q_j = r_j / sqrt(d_j) (a positive coefficient on u_j);
 *              otherwise it is dropped: the columns before it explain it.
 *   output     basis: float [S, T, qpad], qpad = q rounded up to 32, 16-byte aligned: fl32(q_j) in a kept column,
 *              exactly 0.0 in a dropped one and in the padding.  rank: int32 [S], the number of kept columns.
 *   non-finite a subject with a NaN or Inf anywhere in its confounds (a non-finite s_j) gets an all-NaN basis and rank
 *              -1, so that the regression gives it NaN and never "nothing regressed"; other subjects keep their bits.
 *   arithmetic CholeskyQR2 in fp64: G = U^T U with a fixed owner per pair (j, k) summing over the frames in ascending
 *              order, a q x q Cholesky in LDS whose pivot of column j is d_j (the rank rule is applied to it), the same
 *              again on U R1^-1 with the kept set held fixed, and Q = fl32(U (R2 R1)^-1): one rounding to fp32.
 *   bytes      cgnn_ingest_confound_basis_bytes(S, T, q) = 4 S T qpad is what `basis` must hold; rank_bytes >= 4 S.
 * One launch on `stream`: a persistent grid over the subjects, a workgroup of 4 waves per subject; five passes over the
 * subject's confounds, nothing in LDS depends on T.  No workspace.  No atomics, nothing depends on the grid: the same
 * bits on every run and for every grid.
 * q < 1, q > CGNN_CONFOUND_MAX, T < 2, T > 2^30, S < 0, S >= 2^31, a NULL, misaligned or short buffer return CGNN_EINVAL
 * before any launch (the byte count: a negative value); S == 0 returns CGNN_OK with nothing launched.
 *
 * cgnn_ingest_regress.  ts: float [S, T, n] as cgnn_ingest_filter takes it; basis: float [S, T, qpad] as above (any
 * table whose columns are orthonormal or zero), qpad 32 or 64, 16-byte aligned, basis_bytes >= 4 S T qpad.
 *   output     xc[t,i] = fl32(double(x[t,i]) - m_i) as cgnn_ingest_filter centres; out = xc - Q (Q^T xc), the products on
 *              the fp32 matrix pipe, every sum in ascending order of its index.  Columns never mix: a constant column
 *              gives exactly 0, a NaN stays in its column of its subject; a subject with a NaN basis is all NaN.
 *   out        float [S, T, n]; may be `ts` itself, with the same bits as out of place
 *   workspace  cgnn_ingest_regress_workspace_bytes(S, T, n) = 8 S n bytes, 16-byte aligned: the means double [S, n]
 * Two launches on `stream`: cgnn_ingest_filter's means and its k_filter<qpad> in complement form, whose table pointer
 * advances by T * qpad floats per subject.  The same bits on every run and for every grid.
 * qpad outside {32, 64}, T < 2, T > 2^30, S < 0, n <= 0, S * n >= 2^31, a NULL, misaligned or short buffer return
 * CGNN_EINVAL before any launch; S == 0 returns CGNN_OK with nothing launched.  Element offsets are 64-bit.
 * ------------------------------------------------------------------------------------- */
#define CGNN_CONFOUND_MAX 64
#define CGNN_CONFOUND_RANK_TOL 1e-10
int64_t cgnn_ingest_confound_basis_bytes(int64_t S, int32_t T, int32_t q);
int cgnn_ingest_confound_basis(const float* confounds, int64_t S, int32_t T, int32_t q, float* basis,
                               int64_t basis_bytes, int32_t* rank, int64_t rank_bytes, void* stream);
int64_t cgnn_ingest_regress_workspace_bytes(int64_t S, int32_t T, int32_t n);
int cgnn_ingest_regress(const float* ts, int64_t S, int32_t T, int32_t n, const float* basis, int64_t basis_bytes,
                        int32_t qpad, void* workspace, int64_t workspace_bytes, float* out, int64_t out_bytes,
                        void* stream);

/* ---------------------------------------------------------------------------------------
 * Frame censoring (scrubbing) of ROI time series: every time-series call above with a per-subject frame
 * mask.  keep: uint8 [S, T] on the device, nonzero = the frame is kept, keep_bytes >= S T; no alignment is asked of it.
 * Frames keep their place in time and no shape changes.  A censored frame takes part in no mean, norm, inner product or
 * count; its stored values are never looked at, whatever they are (selection, never multiplication).  For subject s, K is
 * the set of its kept frames and Tk = |K|.
 *   centring   m_i = the mean of column i over K, summed in fp64 in a fixed order; xc[t,i] = fl32(double(x[t,i]) - m_i)
 *              for t in K and exactly 0.0 elsewhere; Tk == 0 gives m_i = 0 and zeros everywhere.
 *
 * cgnn_ingest_confound_basis_masked.  cgnn_ingest_confound_basis's statement with every mean, norm s_j, inner product and
 * pivot d_j taken over K.  Rows of Q at censored frames are exactly 0.0.  The rank rule is unchanged: once Tk - 1
 * independent columns are kept it drops the rest.  A non-finite value in a KEPT frame makes the subject's Q NaN (on its
 * kept frames) and its rank -1; one in a censored frame changes nothing.  With every frame kept the bits are
 * cgnn_ingest_confound_basis's.  The same launch, buffers and refusals; a NULL or short keep returns CGNN_EINVAL.
 *
 * cgnn_ingest_regress_masked.  out = xc - Q (Q^T xc) with xc as above and Q a basis whose rows at censored frames are
 * zero (cgnn_ingest_confound_basis_masked's, for the same keep): on the kept frames the fp64 least-squares residual of
 * x[K] on [1 | c[K]], at censored frames exactly 0.0.  qpad == 0 with a NULL basis is masked centring alone, out = xc, and
 * launches no product; qpad 32 or 64 needs the basis.  The workspace is cgnn_ingest_regress_workspace_bytes(S, T, n).  The
 * same two launches and refusals as cgnn_ingest_regress; with every frame kept its bits.  out may be ts.
 *
 * cgnn_ingest_corr_masked / cgnn_ingest_shrinkage_masked.  A unit's frames are its window intersected with K, L_u of
 * them.  m_i and q_i run over those frames (centred fp64 sums, as in cgnn_ingest_corr); z[t,i] is cgnn_ingest_corr's on
 * them and 0 elsewhere; everything after that -- clamp, exact unit diagonal, mirror store, absolute -- is unchanged.  A
 * unit with L_u < 2 has q_i == 0 for every ROI: an exactly all-zero matrix.  The estimate uses L_u wherever
 * cgnn_ingest_shrinkage uses L: B = L_u sum_{t kept} s_t^2, a = (B - F) / (L_u O), and L_u <= 2 or O == 0 give exactly 0;
 * L_u is counted by the kernel.  stats and matrices are what cgnn_ingest_corr_masked left for the same keep, and come with
 * their byte counts (8 U n and 4 U n n).  With every frame kept the bits are the unmasked calls'.  The same launches and
 * refusals as the unmasked calls; a NULL or short keep, stats or matrices returns CGNN_EINVAL.
 *
 * cgnn_ingest_design.  The design of a band removed by regression (the cosines are not orthogonal on K): float
 * [S, T, K + q] = [fl32(b_k[t]) for the K components named, ascending in [1, T - 1] | the q confound columns], every
 * b_k[t] at the frame's own t on the grid of the whole run, the value cgnn_ingest_filter's table holds.  0 <= K, 0 <= q,
 * 1 <= K + q <= CGNN_CONFOUND_MAX; confounds: float [S, T, q], NULL iff q == 0; comps: a HOST array read before the call
 * returns.  cgnn_ingest_design_bytes(S, T, K, q) = 4 S T (K + q) is what `design` must hold.  One launch, a thread per
 * entry.  The band under censoring is then cgnn_ingest_confound_basis_masked of the design and
 * cgnn_ingest_regress_masked: the joint residual on [1 | dropped cosines | confounds] sampled at the kept frames.
 *
 * Every call: a NULL (keep included), misaligned or short buffer and every bad size return CGNN_EINVAL before any launch
 * (a byte-count query: a negative value); S == 0 returns CGNN_OK with nothing launched.  No atomics, nothing depends on
 * the grid: the same bits on every run and for every grid.
 * ------------------------------------------------------------------------------------- */
int cgnn_ingest_confound_basis_masked(const float* confounds, int64_t S, int32_t T, int32_t q, const uint8_t* keep,
                                      int64_t keep_bytes, float* basis, int64_t basis_bytes, int32_t* rank,
                                      int64_t rank_bytes, void* stream);
int cgnn_ingest_regress_masked(const float* ts, int64_t S, int32_t T, int32_t n, const uint8_t* keep, int64_t keep_bytes,
                               const float* basis, int64_t basis_bytes, int32_t qpad, void* workspace,
                               int64_t workspace_bytes, float* out, int64_t out_bytes, void* stream);
int cgnn_ingest_corr_masked(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride,
                            int32_t absolute, const uint8_t* keep, int64_t keep_bytes, float* stats, int64_t stats_bytes,
                            float* out, int64_t out_bytes, void* stream);
int cgnn_ingest_shrinkage_masked(const float* ts, int64_t S, int32_t T, int32_t n, int32_t window, int32_t stride,
                                 const uint8_t* keep, int64_t keep_bytes, const float* stats, int64_t stats_bytes,
                                 const float* matrices, int64_t matrices_bytes, double* alpha, int64_t alpha_bytes,
                                 void* stream);
int64_t cgnn_ingest_design_bytes(int64_t S, int32_t T, int32_t K, int32_t q);
int cgnn_ingest_design(const float* confounds, int64_t S, int32_t T, int32_t q, const int32_t* comps, int32_t K,
                       float* design, int64_t design_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Interpolation of censored frames: every censored frame of ts (float [S, T, n]; confounds [S, T, q]
 * are served alike) replaced by a cubic spline through the subject's kept frames, so that cgnn_ingest_filter's orthogonal
 * projection can run under a frame mask.  keep: uint8 [S, T] as in the block above.  Per subject and column i, in fp64
 * unless it says otherwise: t_0 < .. < t_{m-1} the kept frame indices (as numbers), y_k = double(x[t_k,i]),
 * h_k = t_{k+1} - t_k, delta_k = (y_{k+1} - y_k) / h_k.  (The sampling period plays no part: the spline through the
 * points does not change when time is rescaled.)
 *   kept       frames are bit copies of the input; what a censored frame holds is never looked at (selection)
 *   m == 0     every frame is exactly 0.0;  m == 1: every frame is y_0
 *   ends       a censored frame before t_0 takes x[t_0,i], one after t_{m-1} takes x[t_{m-1},i], as bit copies (NOT the
 *              cubic continued, which scipy's CubicSpline(extrapolate=True) and nilearn give: over a long censored
 *              head it grows without bound)
 *   inside     (t_k, t_{k+1}): the C2 cubic spline with not-a-knot ends in Hermite form on the knot derivatives s_k; with
 *              u = (t - t_k) / h_k,
 *                v = (1+2u)(1-u)^2 y_k + u(1-u)^2 h_k s_k + u^2(3-2u) y_{k+1} + u^2(u-1) h_k s_{k+1},
 *              rounded to fp32 once
 *   s_k        m == 2: s_0 = s_1 = delta_0.   m == 3: s_0 + s_1 = 2 delta_0;
 *              h_1 s_0 + 2(h_0+h_1) s_1 + h_0 s_2 = 3(h_1 delta_0 + h_0 delta_1);  s_1 + s_2 = 2 delta_1.
 *              m >= 4: h_k s_{k-1} + 2(h_{k-1}+h_k) s_k + h_{k-1} s_{k+1} = 3(h_k delta_{k-1} + h_{k-1} delta_k) for
 *              1 <= k <= m-2;  with d = t_2 - t_0:  h_1 s_0 + d s_1 = ((h_0 + 2d) h_1 delta_0 + h_0^2 delta_1) / d;  with
 *              d = t_{m-1} - t_{m-3}:  d s_{m-2} + h_{m-3} s_{m-1} = (h_{m-2}^2 delta_{m-3} + (2d + h_{m-2}) h_{m-3}
 *              delta_{m-2}) / d   (scipy's rows)
 *   arithmetic the Thomas recurrence in fp64; the matrix depends on the mask alone, so its factors are formed once per
 *              subject and a column multiplies by them: no division per column.  Columns never mix: a column constant
 *              over its kept frames gives exactly that constant in every frame, a non-finite value in a KEPT frame
 *              stays in its column of its subject, and with every frame kept the output is a bit copy.
 *   out        float [S, T, n]; may be `ts` itself (a wave owns all T frames of the columns it writes, reads kept frames
 *              only and writes censored frames only), with the same bits; any other overlap is not checked
 *   workspace  cgnn_ingest_interpolate_workspace_bytes(S, T, n) bytes, 16-byte aligned: per (subject, frame) the knot
 *              index and five fp64 factors (44 bytes), the kept count per subject, and per wave of the launch a slab
 *              fp64 [ceil(T / 12)][64] of the recurrence at chunk boundaries; the count depends on cgnn_fused_grid() as
 *              it is when the call is made
 * Three launches on `stream`: the knots (a wave per subject: the kept frames compacted in order), the factors (a wave
 * per subject, a sequential fp64 recurrence), and a persistent grid of 3 * cgnn_fused_grid() workgroups of 4 independent
 * waves over the items (subject, 64 columns), a lane per column: a forward sweep that keeps the recurrence at every 12th
 * knot only, then the chunks of 12 knots last to first, each formed again in registers from its boundary, substituted
 * back and its gaps evaluated and stored (two reads of the kept frames).  No atomics, nothing depends on the grid: the
 * same bits on every run, for every grid, in place and out of place.
 * T < 2, T > 2^30, S < 0, n <= 0, S * n >= 2^31, S * T > 2^50, a NULL (keep included), misaligned or short buffer return
 * CGNN_EINVAL before any launch (the byte count: a negative value); S == 0 returns CGNN_OK with nothing launched.  Element
 * offsets are 64-bit.  No allocation or synchronisation inside.
 * ------------------------------------------------------------------------------------- */
int64_t cgnn_ingest_interpolate_workspace_bytes(int64_t S, int32_t T, int32_t n);
int cgnn_ingest_interpolate(const float* ts, int64_t S, int32_t T, int32_t n, const uint8_t* keep, int64_t keep_bytes,
                            void* workspace, int64_t workspace_bytes, float* out, int64_t out_bytes, void* stream);

/* GCN degree normalisation, models.py:97-105, every step: dis[i] = (sum of row i of w_src
 * (COO order) + 1 + 1e-8)^-1/2 with w_src the edge weights in src-CSR slot order. */
int cgnn_gcn_dis(const float* w_src, const int32_t* rowptr_src, int64_t num_nodes, float* dis,
                 void* stream);

/* HOST-side parameter block (plain device pointers) describing the tiling of one batch. */
typedef struct cgnn_tiles {
  int64_t num_nodes;
  int32_t num_tiles;
  int32_t max_tile_rows;        /* <= CGNN_FUSED_MAX_ROWS */
  const int32_t* tile_ptr;      /* [num_tiles+1] node offsets; tiles are unions of whole graphs */
  const int32_t* tile_blk;      /* [num_tiles+1] first 16-row block of each tile */
  const int32_t* blk_off_dst; const void* ent_dst;   /* blocked-ELL, rows = destinations */
  const int32_t* blk_off_src; const void* ent_src;   /* blocked-ELL, rows = sources */
  const float* dis;             /* [num_nodes] */
} cgnn_tiles;

/* Layer 0's output in factored form.  For F0 <= 8 input features the fused path never writes
 * Y0 [Nn,64] to HBM: consumers rebuild a row from the narrow aggregate P0 = A_hat X0 (32 bytes per
 * node) as  y[c] = b0[c] + sum_{k<F0} P0[row][k] * W0[c][k]  (k ascending, fused multiply-adds --
 * the same expression in every kernel, so all of them see the same bits).  Saves one 256-byte
 * write and three 256-byte reads per node and step for 5 FMAs per rebuilt element. */
typedef struct cgnn_l0src {
  const float* P0;              /* [num_nodes, 8], columns >= F0 zero */
  const float* W0;              /* [64, F0] */
  const float* b0;              /* [64] */
  int32_t F0;                   /* 1..8 */
} cgnn_l0src;

/* Number of persistent workgroups every fused kernel launches (= rows of every slab). */
int cgnn_fused_grid(void);
/* TEST HOOK: make every persistent kernel launch `workgroups` workgroups instead of one per CU
 * (0 restores the device's CU count), so that small parity batches put several tiles / row blocks
 * on one workgroup -- the regime the benchmarks run in.  Process-wide; slabs sized with the old
 * value must not be reused across a change.  Not for production callers. */
int cgnn_set_fused_grid(int32_t workgroups);

/* Tiled edge-weighted aggregation for wide features (F % 64 == 0), the LDS-staged form of
 * cgnn_aggregate_f32 (models.py:112-114, :146-149 and their autograd transposes):
 *     Y[r, :] = post(r) * sum_{e in row r} w_e * pre(c_e) * X[c_e, :]  (+ bias) (+ Yadd[r, :])
 * over the blocked-ELL of `t` (rows = destinations, or sources when CGNN_AGG_TRANSPOSED), one
 * persistent workgroup per (tile, 64-column slice): the slice of the tile is staged in LDS once and
 * every neighbour row is read from there.  pre/post: float [Nn] or NULL; with CGNN_AGG_PRE_DIV /
 * CGNN_AGG_POST_DIV the row is divided by the vector instead of multiplied (SAGE's
 * sum / (wsum + 1e-8)).  Yadd (nullable, may alias Y) is added row-wise: the SAGE backward's
 * dX = dPre W1 + A^T(dPre W2) in one pass.  Whether the ELL carries a self-loop is decided when
 * it is filled (cgnn_bell_fill self_weight).  t->dis is not read. */
#define CGNN_AGG_TRANSPOSED 1
#define CGNN_AGG_PRE_DIV 2
#define CGNN_AGG_POST_DIV 4
int cgnn_aggregate_tiled_f32(const cgnn_tiles* t, int32_t flags, const float* X, int64_t ldx,
                             int32_t F, const float* pre, const float* post, const float* bias,
                             const float* Yadd, int64_t ldadd, float* Y, int64_t ldy, void* stream);
/* The same with BatchNorm(+ReLU)+dropout of the input applied while staging: X = drop(act(a Z + b)),
 * coef = [a | b | ..] of cgnn_bn_act_finalize over the F columns; X is also written to Xout and its
 * keep bytes to mask_out ([num_nodes][F/4], may be NULL) -- cgnn_bn_act_fwd_apply +
 * cgnn_aggregate_tiled_f32 in one launch, bit for bit. */
int cgnn_aggregate_tiled_bn_f32(const cgnn_tiles* t, int32_t flags, const float* Z, int64_t ldz,
                                int32_t F, const float* pre, const float* post, const float* bias,
                                float* Y, int64_t ldy, const float* coef, int32_t relu,
                                float p_drop, uint64_t seed, const uint32_t* seed_dev,
                                uint8_t* mask_out, float* Xout, int64_t ldxo, void* stream);

/* fp16-storage / fp32-accumulate form of cgnn_aggregate_tiled_f32 for large dense parcellations
 * (BASELINE config 5: 1000-ROI graphs, 10 % density, hidden 256): X, Y are IEEE half [Nn, F],
 * tiles of up to CGNN_H16_MAX_ROWS rows (a whole 1000-ROI graph x 64 columns = 128 KB of LDS),
 * entries streamed 16 steps at a time (any degree).  pre/post/bias stay fp32.  The reference has
 * no fp16 path; results are the fp32 oracle's to fp16 resolution (tests use 2e-3 of the scale). */
#define CGNN_H16_MAX_ROWS 1024
int cgnn_aggregate_tiled_f16(const cgnn_tiles* t, int32_t flags, const void* X, int64_t ldx,
                             int32_t F, const float* pre, const float* post, const float* bias,
                             void* Y, int64_t ldy, void* stream);

/* Dense form of the same aggregation for large dense parcellations, on the fp16 matrix cores
 * (v_mfma_f32_32x32x16_f16, fp32 accumulate): Y_g = M_g X_g per graph.
 * cgnn_dense_adj_f16 builds M [B][P][P] half once per batch from a CSR ordering: M_g[r][c] = sum of
 * coef over the slots (row r, column c) (+ selfc[r] on the diagonal, nullable); rows/columns past a
 * graph's size are zero.  The element order inside M is the kernel's own (MFMA-fragment-major):
 * M is only ever passed back to cgnn_dense_aggregate_f16.  Pass the dst-sorted CSR + coef_dst for the forward operator, the
 * src-sorted CSR + coef_src for its transpose.  P: common pitch, multiple of 64, <= 1024, >= the
 * largest graph.  X, Y half [Nn, F], F % 64 == 0; bias fp32 or NULL. */
int cgnn_dense_adj_f16(const int32_t* rowptr, const int32_t* col, const float* coef,
                       const float* selfc, const int32_t* gptr, int32_t num_graphs, int32_t P,
                       void* M, void* stream);
int cgnn_dense_aggregate_f16(const void* M, int32_t P, const int32_t* gptr, int32_t num_graphs,
                             const void* X, int64_t ldx, int32_t F, const float* bias, void* Y,
                             int64_t ldy, double* stat_slab, int64_t stat_slab_bytes, void* stream);

/* stat_slab (both aggregates; NULL = none): [cgnn_fused_grid()][2 * F] fp64 per-workgroup column sums
 * and sums of squares of the half-rounded result (BatchNorm statistics in the epilogue; finalise with
 * cgnn_bn_act_finalize(slab, cgnn_fused_grid(), F, ...)). */
/* The same operator stored per MFMA A fragment (32 rows x 16 sources) in the form that fits it:
 * fragments with more than 64 non-zeros in a DENSE list (1 KB each, operand-major, `dfrag`), those
 * with 1..64 in a SPARSE list (one chunk of 64 (slot | half value << 16) words each, padding slot
 * 0xFFFF, four chunks interleaved per lane, `sent`), empty ones nowhere; `dstep` / `sstep` hold the
 * k-step of every item, `doff` / `soff` [num_graphs * P/32 + 1] the item ranges of the (graph, row
 * block)s (sparse ranges are multiples of four chunks).  Building (P as above):
 *   1. cgnn_dense_pack_count: counts[num_graphs * P/32 * P/16] <- non-zeros per fragment;
 *   2. the caller classifies, forms doff / soff and fpos[fragment] (list position; | 0x80000000 for
 *      the dense list; 0xFFFFFFFF = empty), allocates dfrag / sent (sent pre-filled with 0xFFFF
 *      words, sstep with 0) and calls cgnn_dense_pack_fill.
 * cgnn_dense_aggregate_c16 computes what cgnn_dense_aggregate_f16 computes with the same MFMAs,
 * accumulated dense-list-first (equal up to the order of the fp32 accumulation).  On small-world
 * graphs at 10 % density the operator shrinks ~3x and the dense form is HBM-bound on it. */
int cgnn_dense_pack_count(const int32_t* rowptr, const int32_t* col, const float* coef,
                          const float* selfc, const int32_t* gptr, int32_t num_graphs, int32_t P,
                          uint32_t* counts, void* stream);
int cgnn_dense_pack_fill(const int32_t* rowptr, const int32_t* col, const float* coef,
                         const float* selfc, const int32_t* gptr, int32_t num_graphs, int32_t P,
                         const uint32_t* fpos, void* dfrag, int32_t* dstep, uint32_t* sent,
                         int32_t* sstep, void* stream);
int cgnn_dense_aggregate_c16(const void* dfrag, const int32_t* dstep, const uint32_t* doff,
                             const uint32_t* sent, const int32_t* sstep, const uint32_t* soff,
                             int32_t P, const int32_t* gptr, int32_t num_graphs, const void* X,
                             int64_t ldx, int32_t F, const float* bias, void* Y, int64_t ldy,
                             double* stat_slab, int64_t stat_slab_bytes, void* stream);
/* The backward product dT = A_hat^T dY of a GCN layer with dY never materialised: the slice handed to
 * the matrix cores is formed while it is staged,
 *     dY = a * (dX' * f - c1 - xhat * c2),   f = relu' * keep / (1-p),   xhat = (Yl - mean) * invstd
 * (the arithmetic of cgnn_bn_act_bwd_apply_f16, models.py:208-210 through autograd), from the gradient
 * of the layer's activation -- dX' [M, F] half, or for the last layer the readout gradient dP [B, F]
 * fp32 (row gradient dP[graph] / (n_g + 1e-8)); exactly one of the two -- the layer's pre-BatchNorm
 * output Yl, keep bytes, coefficient block `coef` and the backward coefficients `bwc`.  dY feeds
 * nothing else but the bias gradient: its column sums are left per graph in cs_slab [B][F] fp64
 * (combine with cgnn_slab_reduce_f64_multi: B rows of width F -> db). */
int cgnn_dense_aggregate_c16_bnbwd(const void* dfrag, const int32_t* dstep, const uint32_t* doff,
                                   const uint32_t* sent, const int32_t* sstep, const uint32_t* soff,
                                   int32_t P, const int32_t* gptr, int32_t num_graphs, const void* dX,
                                   int64_t lddx, const float* dP, const void* Yl, int64_t ldyl,
                                   const uint8_t* mask, const float* coef, const float* bwc, int32_t relu,
                                   float p_drop, int32_t F, void* dT, int64_t lddt, double* cs_slab, int64_t cs_slab_bytes,
                                   void* stream);

/* The DENSE FRAGMENTS of an aggregation operator applied in fp32 on the bf16 matrix pipe with exactly
 * split operands (band_aggregate.hip) -- for graphs of more than 384 nodes in the reference's own
 * arithmetic (models.py:112-114 / :146-149 and their autograd transposes at 1000 ROI), where the gather
 * kernel cgnn_aggregate_f32 is bound by reading ~100 neighbour rows per output row out of L2.
 *   cgnn_band_pack_f32: from one CSR ordering (as cgnn_dense_pack_count/fill: P = dense pitch, fpos
 *     [num_graphs * P/32 * P/16] = position of a fragment in the dense list or 0xFFFFFFFF) the listed
 *     fragments as MFMA A operands cut into three bf16 pieces: bfrag [items][3][64 lanes][8 bf16]
 *     (3 KB per fragment), bstep [items] = k-step.  Duplicate edges add up in fp32.  Static per batch.
 *   cgnn_band_aggregate_f32: Y[r,:] = (sum over the listed fragments of row block r/32) (/ rowdiv[r]) for
 *     every row (0 where the row block lists nothing), + Yadd[r,:] when Yadd is not NULL (GraphSAGE's
 *     dX = dX1 + A^T(dA / den), models.py:146-152 backward; Yadd may not alias Y); boff [num_graphs * P/32 + 1] = item ranges of the
 *     (graph, row block)s; F % 32 == 0, ldx / ldy even, X / Y 8-byte aligned, Y != X.  The caller then
 *     runs cgnn_aggregate_acc_f32 on the CSR of the edges OUTSIDE the listed fragments (it also carries
 *     the self-loop term, the row division and the bias) on top: together the full operator, each matrix
 *     product exact to 2^-24 relative, the sums in another order than the reference's. */
int cgnn_band_pack_f32(const int32_t* rowptr, const int32_t* col, const float* coef, const int32_t* gptr,
                       int32_t num_graphs, int32_t P, const uint32_t* fpos, void* bfrag, int32_t* bstep,
                       void* stream);
int cgnn_band_aggregate_f32(const void* bfrag, const int32_t* bstep, const int32_t* boff, int32_t P,
                            const int32_t* gptr, int32_t num_graphs, const float* X, int64_t ldx, int32_t F,
                            const float* rowdiv, const float* Yadd, int64_t ldadd, float* Y, int64_t ldy,
                            void* stream);


/* BatchNorm finalisation in the PRODUCER's tail (round 4; csrc/bn_tail.h): instead of writing its
 * per-workgroup partial sums to a slab for cgnn_bn_stats_finalize_rng / cgnn_bn_bwd_stats_finalize to fold
 * in a launch of their own, a tile kernel adds them to an accumulator (fixed-point 64-bit atomic adds:
 * order-independent, bit-identical reruns) and the workgroup that arrives last writes the layer's
 * coefficient block.  `acc`: CGNN_BN_ACC_BYTES bytes of device memory, ZERO before the first launch that
 * uses it; every launch leaves it zero again.  One accumulator may serve launches on ONE stream.
 *   mode 0 (statistics of a forward layer): the arithmetic of cgnn_bn_stats_finalize_rng -- count rows,
 *     gamma/beta, running statistics and num_batches_tracked updated in place, bn_out float[4*64], rng_state /
 *     rng_n as there (the step's dropout words, refreshed by the tail; NULL / 0 = none);
 *   mode 1 (sums of a backward layer): the arithmetic of cgnn_bn_bwd_stats_finalize -- dgamma, dbeta
 *     float[64], bwc float[2*64], zero_coef as there.
 * Passed as the last argument of cgnn_gcn_l0_fwd / cgnn_gcn_l0_stats (mode 0; factored layer 0: the centred
 * form's mean offset is the kernel's own), cgnn_gcn_fused_fwd (mode 0) and cgnn_gcn_fused_bwd (mode 1, the sums of the layer
 * BELOW); NULL = the slab protocol.  With a tail the corresponding slab argument may be NULL. */
#define CGNN_BN_ACC_BYTES 16448
typedef struct cgnn_bn_tail {
  void* acc;
  double count;
  int32_t mode, zero_coef;
  const float* gamma; const float* beta;
  float* running_mean; float* running_var;
  float momentum, eps;
  int64_t* num_batches_tracked;
  float* bn_out;
  uint32_t* rng_state; int32_t rng_n; int32_t reserved;
  float* dgamma; float* dbeta; float* bwc;
} cgnn_bn_tail;

/* Layer 0 forward.  X0 [Nn,F0] (F0 <= 16), W0 [64,F0], bias [64] -> Y [Nn,64];
 * stat_slab [grid][128] fp64 (sum(y) | sum(y^2)) or NULL (eval). */
int cgnn_gcn_fused_fwd_first(const cgnn_tiles* t, const float* X0, int32_t F0, const float* W0,
                             const float* bias, float* Y, double* stat_slab, int64_t stat_slab_bytes, void* stream);

/* Layer l>0 forward.  Yprev [Nn,64] + bn_prev -> X on the fly; W [64,64]; mask_out nullable.
 * Yprev == NULL: the previous layer is layer 0 in factored form, rows rebuilt from *l0. */
/* seed_dev (nullable): device word XOR-ed into the dropout key at kernel start.  Under HIP-graph
 * replay the by-value `seed` is frozen in the graph; a captured cgnn_rng_advance on the same
 * stream then makes every replay draw fresh masks. */
int cgnn_rng_advance(uint32_t* state, int32_t n, void* stream);
int cgnn_gcn_fused_fwd(const cgnn_tiles* t, const float* Yprev, const cgnn_l0src* l0,
                       const float* bn_prev, float p_drop, uint64_t seed, const uint32_t* seed_dev,
                       uint8_t* mask_out, const float* W, const float* bias, float* Y,
                       double* stat_slab, int64_t stat_slab_bytes, const cgnn_bn_tail* tail, void* stream);

/* slab [rows][width] fp64 -> sums [width] fp64 (fixed-order tree). */
int cgnn_bn_reduce(const double* slab, int32_t rows, int32_t width, double* sums, void* stream);

/* BatchNorm1d forward coefficients (models.py:191-193 semantics: biased batch variance,
 * eps, momentum; running_var gets the unbiased variance).  training != 0: from sums
 * (sum(y)|sum(y^2), [128]) over `count` rows, and running stats are updated in place;
 * training == 0: from running stats.  bn_out float[4*64]. */
/* count_dev (nullable): device double that overrides `count` -- the all-reduced row count of a
 * multi-rank batch stays on the device, no host read-back between reduce and finalise. */
int cgnn_bn_finalize(const double* sums, double count, const double* count_dev, const float* gamma,
                     const float* beta, float* running_mean, float* running_var, float momentum,
                     float eps, int32_t training, float* bn_out, const float* mean_offset, void* stream);

/* Readout: P[g,:] = mean over nodes of drop(relu(a*Y+b)) (models.py:209-211,57-59).
 * F1, F2 (both or neither; [num_graphs,64]): per graph and column the sums over the graph's rows
 * of f = relu'(z)*keep/(1-p) and of f*xhat -- what cgnn_gcn_fused_pool_bwd_sums needs. */
int cgnn_gcn_fused_pool_fwd(const float* Y, const float* bn, float p_drop, uint64_t seed,
                            const uint32_t* seed_dev, uint8_t* mask_out, const int32_t* gptr,
                            int32_t num_graphs, float* P, float* F1, float* F2, void* stream);

/* BatchNorm-backward sums of the LAST layer without re-reading Y: the readout's gradient is
 * dP[g]/(n_g+1e-8) for every row of graph g, so  sum dZ = sum_g dP[g]/n_g * F1[g]  and
 * sum dZ*xhat = sum_g dP[g]/n_g * F2[g].  s_slab [cgnn_fused_grid()][128] fp64 partials. */
int cgnn_gcn_fused_pool_bwd_sums(const float* dP, const float* F1, const float* F2,
                                 const int32_t* gptr, int32_t num_graphs, double* s_slab, int64_t s_slab_bytes,
                                 void* stream);
/* (cgnn_gcn_fused_pool_bwd_sums + cgnn_bn_bwd_stats_finalize) in one launch: dgamma/dbeta [64] and
 * the c1|c2 block bwc [128] of the last layer, for per-rank BatchNorm statistics (no exchange
 * between the sums and the coefficients).  count = rows of the batch. */
int cgnn_gcn_fused_pool_bwd_finalize(const float* dP, const float* F1, const float* F2,
                                     const int32_t* gptr, int32_t num_graphs, double count,
                                     int32_t zero_coef, float* dgamma, float* dbeta, float* bwc,
                                     void* stream);

/* Backward of the readout through dropout/ReLU: dZ = dP[g]/(n_g+1e-8) * drop' * relu';
 * also the BatchNorm-backward sums of the last layer: s_slab [grid][128] = sum dZ | sum dZ*xhat.
 * dZ may be NULL (sums only) when the last layer's backward rebuilds dZ itself (dP != NULL there). */
int cgnn_gcn_fused_pool_bwd(const float* dP, const float* Y, const float* bn, float p_drop,
                            const uint8_t* mask, const int32_t* gptr, int32_t num_graphs,
                            float* dZ, double* s_slab, int64_t s_slab_bytes, void* stream);

/* BatchNorm backward coefficients: dgamma = sum dZ*xhat, dbeta = sum dZ, bwc = [c1|c2]. */
int cgnn_bn_bwd_finalize(const double* sums, double count, const double* count_dev,
                         int32_t zero_coef, float* dgamma, float* dbeta, float* bwc, void* stream);

/* Layer l>0 backward.  Inputs: dZ (grad wrt BN output of layer l), Y (its pre-BN output), bn,
 * bwc; previous layer's Yprev/bn_prev/mask_prev (to rebuild X_l and apply relu'/drop').
 * Outputs: dZprev [Nn,64]; s_slab_prev [grid][128]; dW_slab [grid][64*64]; db_slab [grid][64]. */
/* Last layer only: pass dP != NULL (then dZ is ignored and may be NULL) together with
 * node_graph int32 [Nn], gptr int32 [B+1] and mask_cur (this layer's keep bits): the incoming
 * gradient is rebuilt per row as dP[g]/(n_g+1e-8) * relu' * dropout'.  Otherwise dP = NULL.
 * Yprev == NULL: the previous layer is layer 0 in factored form, rows rebuilt from *l0.
 * mask_prev (when p_drop > 0) is read as 32-bit words and must be 4-byte aligned (CGNN_EINVAL
 * otherwise); node_graph must be non-decreasing (the batch vector of whole graphs). */
int cgnn_gcn_fused_bwd(const cgnn_tiles* t, const float* dZ, const float* Y, const float* bn,
                       const float* bwc, const float* Yprev, const cgnn_l0src* l0,
                       const float* bn_prev, float p_drop, const uint8_t* mask_prev, const float* W,
                       float* dZprev, double* s_slab_prev, int64_t s_slab_prev_bytes, float* dW_slab, int64_t dW_slab_bytes, double* db_slab, int64_t db_slab_bytes,
                       const float* dP, const int32_t* node_graph, const int32_t* gptr,
                       const uint8_t* mask_cur, const cgnn_bn_tail* tail, void* stream);

/* Layer 0 backward: dW0 = dT^T X0 only.  dW_slab [grid][64*16] (columns >= F0 are zero). */
int cgnn_gcn_fused_bwd_first(const cgnn_tiles* t, const float* dZ, const float* Y,
                             const float* bn, const float* bwc, const float* X0, int32_t F0,
                             float* dW_slab, int64_t dW_slab_bytes, double* db_slab, int64_t db_slab_bytes, float p_drop, const float* dP,
                             const int32_t* node_graph, const int32_t* gptr,
                             const uint8_t* mask_cur, void* stream);

/* Layer 0, narrow form (F0 <= 8): Y0 = (A_hat X0) W0^T + b with P0 = A_hat X0 kept for backward
 * ([Nn,8] fp32, columns >= F0 zero); dW0 = dY0^T P0, db0 = sum dY0 need no aggregation.
 * Slabs have cgnn_l0_grid(num_nodes) rows: stat_slab [..][128] fp64, dW_slab [..][64*8] f32,
 * db_slab [..][64] fp64.  (cgnn_gcn_fused_fwd_first/bwd_first remain for 8 < F0 <= 16 and for
 * one-layer models.) */
int cgnn_l0_grid(int64_t num_nodes);
/* Y (forward) may be NULL: only P0 and the statistics are produced and every consumer rebuilds
 * Y0's rows from a cgnn_l0src.  Backward: Y == NULL -> rebuilt from P0 with l0->W0/b0/F0.
 *
 * Centred form (Y == NULL, F0 <= 7; round 3).  With `center` (float[8], device): c = center[0..F0)
 * near the column means of X0 and rbar = center[7] near the mean of r = A_hat 1 (the normalised
 * operator's row sums) -- cgnn_gcn_l0_center computes both from the batch's first non-empty tile;
 * any finite values give the same result up to rounding --
 *     A_hat X0 = A_hat (X0 - 1 c^T) + r c^T
 *     P0' = [A_hat (X0 - 1 c^T) | r - rbar | 0..]   ([Nn,8]; column F0 = the aggregated ones column,
 *                                                     summed in fp64)
 *     W'  = [W0 | W0 c]                              (`w_eff`, float[64][F0 + 1], written by the launch)
 *     Y0  = P0 W0^T + b = P0' W'^T + mean_offset,    mean_offset = b + rbar W0 c  (float[64], written)
 * The layer is handed on WITHOUT its constant term: consumers take cgnn_l0src{P0', w_eff, zeros, F0 + 1},
 * the statistics in stat_slab are those of y_c = Y0 - mean_offset, and the BatchNorm finalisation
 * (cgnn_bn_stats_finalize_rng / cgnn_bn_finalize with the same mean_offset) describes y_c -- BatchNorm
 * is invariant under a per-channel shift; only the running mean sees the constant.  The SAME function
 * of the parameters, evaluated at the scale of the features' spread: with node features far from
 * zero (un-normalised strength / degree columns) the raw form puts rounding of the size
 * 2^-24 * mean into every aggregated row and every rebuilt y, and loses log2((mean/sigma)^2) bits of
 * the BatchNorm variance.  cgnn_gcn_l0_bwd (same `center`, l0->F0 = F0 + 1) returns
 * dW0[:, k] = dW'[:, k] + c[k] (dW'[:, F0] + rbar db0) in the first F0 of the 8 slab columns. */
int cgnn_gcn_l0_center(const cgnn_tiles* t, const float* X0, int32_t F0, float* center, void* stream);
int cgnn_gcn_l0_fwd(const cgnn_tiles* t, const float* X0, int32_t F0, const float* W0,
                    const float* bias, float* P0, float* Y, double* stat_slab, int64_t stat_slab_bytes, const float* center,
                    float* w_eff, float* mean_offset, const cgnn_bn_tail* tail, void* stream);
int cgnn_gcn_l0_bwd(const float* dZ, const float* Y, const cgnn_l0src* l0, const float* bn,
                    const float* bwc, const float* P0, int64_t num_nodes, float* dW_slab, int64_t dW_slab_bytes,
                    double* db_slab, int64_t db_slab_bytes, const float* center, void* stream);
/* The factored forward (Y == NULL) in two halves, for a batch that is kept and trained on repeatedly: what
 * depends on the batch alone, once, and what depends on W0 / bias, per step.  Together they write, bit for
 * bit, what cgnn_gcn_l0_fwd writes.
 *   cgnn_gcn_l0_agg    P0 (P0' with `center`, as above) and, per workgroup of its cgnn_l0_grid(num_nodes)
 *                      grid, the 9 x 9 fp64 second moments of the P0 rows it aggregated (columns p_0..p_7
 *                      and 1, row-major): moments[cgnn_l0_grid][81], moments_bytes >= grid * 81 * 8.
 *                      Every set is written by every call.
 *   cgnn_gcn_l0_stats  moments -> the 128 sums (sum y | sum y^2) of every set, with the W0 / bias of this
 *                      step: to stat_slab[sets][128] (stat_slab_bytes >= sets * 128 * 8; the rows
 *                      cgnn_gcn_l0_fwd writes) or through `tail` (one atomic pair per column and workgroup of
 *                      a grid of at most cgnn_fused_grid() workgroups; the accumulator ends as after
 *                      cgnn_gcn_l0_fwd).  Writes w_eff and mean_offset as cgnn_gcn_l0_fwd does (`center` as
 *                      given to cgnn_gcn_l0_agg); with neither a slab nor a tail (eval mode) only those.
 *                      `sets` must be cgnn_l0_grid(num_nodes) of the batch: a value outside cgnn_l0_grid's
 *                      range, or with a tail one that is not cgnn_l0_grid(tail->count), is CGNN_EINVAL. */
int cgnn_gcn_l0_agg(const cgnn_tiles* t, const float* X0, int32_t F0, const float* center, float* P0,
                    double* moments, int64_t moments_bytes, void* stream);
int cgnn_gcn_l0_stats(const double* moments, int32_t sets, int32_t F0, const float* W0, const float* bias,
                      const float* center, float* w_eff, float* mean_offset, double* stat_slab,
                      int64_t stat_slab_bytes, const cgnn_bn_tail* tail, void* stream);
/* Node-feature gradient of the narrow layer 0 (ROI saliency).  With Y0 = (A_hat X0) W0^T + b:
 *     G0  = dY0 W0          [Nn, 8] fp32, columns >= F0 zero: the 64 -> F0 narrowing of dY0 = BatchNorm'(dZ0)
 *     dX0 = A_hat^T G0      [Nn, F0]: one narrow transposed aggregate over the source-side blocked-ELL
 * cgnn_gcn_l0_bwd_dx is cgnn_gcn_l0_bwd in its rebuilding form (Y == NULL) that also writes G0
 * (G0_bytes >= num_nodes * 8 * 4); the slabs it fills are those of cgnn_gcn_l0_bwd, bit for bit.  In the
 * centred form (same `center`, l0->F0 = F0 + 1) G0 uses the first F0 columns of l0->W0 (`w_eff`): the
 * function does not depend on the centring constants.  cgnn_gcn_l0_dx then writes dX0 unpadded
 * (dX0_bytes >= num_nodes * F0 * 4) with F0 the TRUE feature count, 1..8; `t` as in cgnn_gcn_l0_fwd. */
int cgnn_gcn_l0_bwd_dx(const float* dZ, const cgnn_l0src* l0, const float* bn, const float* bwc, const float* P0,
                       int64_t num_nodes, float* dW_slab, int64_t dW_slab_bytes, double* db_slab,
                       int64_t db_slab_bytes, const float* center, float* G0, int64_t G0_bytes, void* stream);
int cgnn_gcn_l0_dx(const cgnn_tiles* t, const float* G0, int32_t F0, float* dX0, int64_t dX0_bytes, void* stream);

/* fp16-storage forms of the BatchNorm(+ReLU)+dropout kernels (cgnn_bn_act_*): the [M,N] activation
 * arrays (Y, X, dX, dY) are IEEE half, the arithmetic is fp32, the statistics fp64, coefficient
 * blocks / masks / slabs / pooled rows exactly as in the fp32 forms.  Used by the fp16-storage
 * GCN encoder for large dense parcellations (BASELINE config 5); the reference has no fp16 path
 * (models.py is fp32-only), results are the fp32 oracle's to fp16 resolution. */
int cgnn_bn_act_fwd_stats_f16(const void* Y, int64_t M, int32_t N, double* slab, int64_t slab_bytes, void* stream);
int cgnn_bn_act_fwd_apply_f16(const void* Y, const float* coef, int32_t relu, float p_drop, uint64_t seed,
                              const uint32_t* seed_dev, uint8_t* mask_out, void* X, int64_t M,
                              int32_t N, void* stream);
int cgnn_bn_act_pool_fwd_f16(const void* Y, const float* coef, int32_t relu, float p_drop, uint64_t seed,
                             const uint32_t* seed_dev, uint8_t* mask_out, const int32_t* gptr,
                             int32_t num_graphs, float* P, int32_t N, float* Fsum, void* stream);
int cgnn_bn_act_bwd_stats_f16(const void* dX, const void* Y, const uint8_t* mask, const float* coef,
                              int32_t relu, float p_drop, int64_t M, int32_t N, double* slab, int64_t slab_bytes,
                              const float* dP, const int32_t* node_graph, const int32_t* gptr,
                              void* stream);
int cgnn_bn_act_bwd_apply_f16(const void* dX, const void* Y, const uint8_t* mask, const float* coef,
                              const float* bwc, int32_t relu, float p_drop, int32_t relu_in,
                              double* colsum_slab, int64_t colsum_slab_bytes, void* dY, int64_t M, int32_t N, const float* dP,
                              const int32_t* node_graph, const int32_t* gptr, void* stream);

/* ---- optimizer: torch.optim.Adam's update (L2 weight decay, no amsgrad) for up to
 * CGNN_ADAM_MAX_JOBS fp32 tensors in ONE launch (reference: torch.optim.Adam in demo.py:105-134).
 * `step` is the shared fp32 step counter on the device (t = *step + 1 is used); with advance != 0
 * the same launch stores *step + 1 once every workgroup has read it (`arrivals`: a zeroed uint32
 * the launch leaves zero again).  Graph-capturable: nothing comes from the host but lr/betas, which
 * a captured launch therefore keeps; cgnn_adam_step_dev (cgnn_optim.h) reads them from the device. */
#define CGNN_ADAM_MAX_JOBS 32
typedef struct cgnn_adam_jobs {
  int32_t n;
  int64_t numel[CGNN_ADAM_MAX_JOBS];
  float* param[CGNN_ADAM_MAX_JOBS];
  const float* grad[CGNN_ADAM_MAX_JOBS];
  float* exp_avg[CGNN_ADAM_MAX_JOBS];
  float* exp_avg_sq[CGNN_ADAM_MAX_JOBS];
} cgnn_adam_jobs;
int cgnn_adam_step(const cgnn_adam_jobs* jobs, float* step, uint32_t* arrivals, int32_t advance,
                   double lr, double beta1, double beta2, double eps, double weight_decay, void* stream);

/* Single-launch forms of (cgnn_bn_reduce + cgnn_bn_finalize [+ num_batches_tracked += 1]) and
 * (cgnn_bn_reduce + cgnn_bn_bwd_finalize): used when no cross-rank exchange sits between the
 * reduction and the finalisation.
 * zero_coef != 0 writes c1 = c2 = 0 (eval-mode BatchNorm backward is a fixed affine map).
 * cgnn_bn_stats_finalize_rng also refreshes the rng_n (<= 64) device dropout words of a graph-captured
 * step (cgnn_rng_advance's arithmetic) in the same launch; rng_state NULL / rng_n 0: no refresh.
 * mean_offset (float[64], nullable; also cgnn_bn_finalize): the slab holds the statistics of
 * y - mean_offset[c] (the centred factored layer 0 is handed on without its constant term, which
 * BatchNorm's output does not depend on): bn_out describes that shifted variable, the module's
 * running_mean is updated with (resp. in eval mode read as) the mean of y itself. */
int cgnn_bn_stats_finalize_rng(const double* slab, int32_t rows, double count, const float* gamma,
                               const float* beta, float* running_mean, float* running_var,
                               float momentum, float eps, int64_t* num_batches_tracked, float* bn_out,
                               uint32_t* rng_state, int32_t rng_n, const float* mean_offset, void* stream);
int cgnn_bn_bwd_stats_finalize(const double* slab, int32_t rows, double count, int32_t zero_coef,
                               float* dgamma, float* dbeta, float* bwc, void* stream);
/* The weight and bias gradients of up to CGNN_DW_MAX_JOBS layers from their per-workgroup slabs in one
 * launch: dw_slab f32 [rows][64*out_cols] -> dW[i] dense [64][take_cols[i]], db_slab f64 [rows][64] ->
 * db[i] [64].  The reductions do not feed the backward chain, so all of a model's layers wait for its end. */
#define CGNN_DW_MAX_JOBS 8
typedef struct cgnn_dw_jobs {
  int32_t n;
  const float* dw_slab[CGNN_DW_MAX_JOBS];
  const double* db_slab[CGNN_DW_MAX_JOBS];
  int32_t rows[CGNN_DW_MAX_JOBS], out_cols[CGNN_DW_MAX_JOBS], take_cols[CGNN_DW_MAX_JOBS];
  float* dW[CGNN_DW_MAX_JOBS];
  float* db[CGNN_DW_MAX_JOBS];
} cgnn_dw_jobs;
int cgnn_dw_db_reduce_multi(const cgnn_dw_jobs* jobs, void* stream);

/* Fixed-order combination of per-workgroup partials (fp64 accumulate):
 * f32 slab [rows][width] -> out[r*ld_out + c] for width = out_rows*out_cols (take the first
 * `take_cols` of every `out_cols` columns). */
int cgnn_slab_reduce_f32(const float* slab, int32_t rows, int32_t out_rows, int32_t out_cols,
                         int32_t take_cols, float* out, int32_t ld_out, void* stream);
/* f32 slab [rows][width] -> out[0..split) and out_tail[0..width-split): the same fold with its result in two
 * places -- the classifier's parameter gradients straight into a caller-owned gradient buffer (data-parallel
 * training: the flat all-reduce buffer) and the loss column of cgnn_head_loss_f32's slab next to it. */
int cgnn_slab_reduce_f32_split(const float* slab, int32_t rows, int32_t width, int32_t split, float* out,
                               float* out_tail, void* stream);
/* f64 slabs [rows[j]][width[j]] -> f32 out[j] [width[j]], up to CGNN_REDUCE_MAX_JOBS in ONE launch (the
 * bias gradients of every layer of a backward pass: their per-block column sums are final long before
 * the pass ends) */
#define CGNN_REDUCE_MAX_JOBS 8
typedef struct cgnn_reduce_jobs {
  int32_t n;
  const double* slab[CGNN_REDUCE_MAX_JOBS];
  int32_t rows[CGNN_REDUCE_MAX_JOBS];
  int32_t width[CGNN_REDUCE_MAX_JOBS];
  float* out[CGNN_REDUCE_MAX_JOBS];
} cgnn_reduce_jobs;
int cgnn_slab_reduce_f64_multi(const cgnn_reduce_jobs* jobs, void* stream);

/* ---------------------------------------------------------------------------------------
 * BatchNorm1d (+ReLU) + dropout for the layered path (any power-of-two width 4..1024),
 * models.py:208-210 (GCN: BN, ReLU, dropout) and :260-261 (SAGE: BN, dropout):
 *   forward : cgnn_bn_act_fwd_stats -> cgnn_bn_act_finalize -> cgnn_bn_act_fwd_apply
 *             X' = drop(act(a*Y + b)); coef float[4N] = a | b | mean | invstd
 *   backward: cgnn_bn_act_bwd_stats -> cgnn_bn_act_bwd_finalize -> cgnn_bn_act_bwd_apply
 *             dY = a*(dX'*drop'*act' - c1 - xhat*c2); bwc float[2N] = c1 | c2
 * slabs: fp64 [cgnn_bn_act_slab_rows(M)][2N]; mask: one byte (4 keep bits) per 4-column chunk,
 * [M*N/4] bytes, may be NULL when p_drop == 0.  Semantics of nn.BatchNorm1d as in
 * cgnn_bn_finalize (training: batch stats + running update; eval: running stats).
 * ------------------------------------------------------------------------------------- */
int cgnn_bn_act_width_ok(int32_t N);
int64_t cgnn_bn_act_slab_rows(int64_t M);
int cgnn_bn_act_fwd_stats(const float* Y, int64_t M, int32_t N, double* slab, int64_t slab_bytes, void* stream);
/* count_dev (nullable): the row count read from device memory instead of `count` -- under
 * full-batch BatchNorm across ranks the caller all-reduces [sum | sumsq | rows] and passes the
 * reduced block as a 1-row slab with count_dev = &block[2N]; nothing returns to the host. */
int cgnn_bn_act_finalize(const double* slab, int32_t rows, int32_t N, double count,
                         const double* count_dev, int32_t training,
                         const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float momentum, float eps,
                         int64_t* num_batches_tracked, float* coef, void* stream);
int cgnn_bn_act_fwd_apply(const float* Y, const float* coef, int32_t relu, float p_drop,
                          uint64_t seed, const uint32_t* seed_dev, uint8_t* mask_out, float* X,
                          int64_t M, int32_t N, void* stream);
/* Readout fused with the last layer's BatchNorm(+act)+dropout (models.py:211 / :262):
 * P[g,:] = sum_{rows of g} drop(act(a*Y+b)) / (n_g + 1e-8); X' is never materialised.  gptr int32
 * [B+1].  Its backward is the dP form of the two kernels below: dP != NULL replaces dX by
 * dP[node_graph[r],:] / (n_g + 1e-8), rebuilt per row (dX may then be NULL). */
int cgnn_bn_act_pool_fwd(const float* Y, const float* coef, int32_t relu, float p_drop, uint64_t seed,
                         const uint32_t* seed_dev, uint8_t* mask_out, const int32_t* gptr,
                         int32_t num_graphs, float* P, int32_t N, float* Fsum, void* stream);
/* Fsum (nullable, float [2][B][N]): the pooled pass also leaves the per-graph factor sums
 * F1[g][c] = sum_rows f, F2[g][c] = sum_rows f * xhat (f = act' * keep / (1-p)); the readout's
 * gradient is constant per graph, so this layer's BatchNorm-backward sums follow from them without
 * a pass over Y:  cgnn_bn_act_pool_bwd_finalize == cgnn_bn_act_bwd_stats(dP form) + cgnn_bn_act_bwd_finalize. */
int cgnn_bn_act_pool_bwd_finalize(const float* dP, const float* Fsum, const int32_t* gptr, int32_t num_graphs,
                                  int32_t N, double count, int32_t zero_coef, float* dgamma, float* dbeta,
                                  float* bwc, void* stream);
int cgnn_bn_act_bwd_stats(const float* dX, const float* Y, const uint8_t* mask, const float* coef,
                          int32_t relu, float p_drop, int64_t M, int32_t N, double* slab, int64_t slab_bytes,
                          const float* dP, const int32_t* node_graph, const int32_t* gptr,
                          void* stream);
int cgnn_bn_act_bwd_finalize(const double* slab, int32_t rows, int32_t N, double count,
                             const double* count_dev, int32_t zero_coef, float* dgamma,
                             float* dbeta, float* bwc, void* stream);
/* relu_in != 0: Y is itself the output of a ReLU (SAGELayer, models.py:152): dY is additionally
 * masked by Y > 0, i.e. it is the gradient of the layer's pre-activation.  colsum_slab (nullable):
 * fp64 [cgnn_bn_act_apply_blocks(M, N)][N] per-block column sums of dY (the bias gradient),
 * combined with cgnn_slab_reduce_f64_multi. */
int64_t cgnn_bn_act_apply_blocks(int64_t M, int32_t N);
int cgnn_bn_act_bwd_apply(const float* dX, const float* Y, const uint8_t* mask, const float* coef,
                          const float* bwc, int32_t relu, float p_drop, int32_t relu_in,
                          double* colsum_slab, int64_t colsum_slab_bytes, float* dY, int64_t M, int32_t N, const float* dP,
                          const int32_t* node_graph, const int32_t* gptr, void* stream);

/* ---------------------------------------------------------------------------------------
 * Graph-level classifier head, models.py:196-201 + :213-216:
 *   logits = Linear2(dropout(relu(Linear1(P)))),  P [B,H] (one row per graph), W1 [H2,H], W2 [C,H2].
 * One kernel each way instead of six small library GEMM/elementwise launches.
 * forward also writes H1 [B,H2] (the activations after ReLU and dropout) and fac [B,H2] (relu' *
 * dropout' factor).  backward: dP [B,H] and a slab [cgnn_head_grid(B,H2)][WD] of per-workgroup
 * partial parameter gradients, row layout dW1 [H2*H] | db1 [H2] | dW2 [C*H2] | db2 [C]
 * (WD = their sum), combined with cgnn_slab_reduce_f32(slab, rows, 1, WD, WD, out, WD).
 * cgnn_head_supported: H <= 128, H2 <= 64 and a divisor of 256, C <= 16.
 * ------------------------------------------------------------------------------------- */
int cgnn_head_supported(int32_t H, int32_t H2, int32_t C);
int cgnn_head_grid(int32_t B, int32_t H, int32_t H2, int32_t C);   /* rows of cgnn_head_bwd_f32's slab */
int cgnn_head_fwd_f32(const float* P, int32_t B, int32_t H, int32_t H2, int32_t C, const float* W1,
                      const float* b1, const float* W2, const float* b2, float p_drop,
                      uint64_t seed, const uint32_t* seed_dev, float* H1, float* fac, float* logits,
                      void* stream);
int cgnn_head_bwd_f32(const float* dlogits, const float* P, const float* H1, const float* fac,
                      int32_t B, int32_t H, int32_t H2, int32_t C, const float* W1, const float* W2,
                      float* dP, float* slab, int64_t slab_bytes, void* stream);

/* Mean cross-entropy of the step (torch.nn.CrossEntropyLoss defaults; reference train.py:39,49):
 * loss[0] = mean_i(logsumexp(logits[i,:]) - logits[i, labels[i]]); dlogits [B,C] = its gradient
 * for a unit upstream gradient, (softmax - onehot) / V.  labels int64 [B].  Rows labelled -100
 * (torch's default ignore_index) contribute nothing, get a zero gradient and are left out of
 * the row count V; any other label outside [0, C) -- where torch raises -- turns the loss and
 * that row's gradient into NaN (a kernel cannot raise; the NaN surfaces at the next read-back). */
int cgnn_cross_entropy_f32(const float* logits, const int64_t* labels, int32_t B, int32_t C,
                           float* loss, float* dlogits, void* stream);

/* The classifier's whole training step in one launch -- cgnn_head_fwd_f32, cgnn_cross_entropy_f32 and
 * cgnn_head_bwd_f32 (models.py:196-201,213-216 and train.py:46-50 with the loss's unit upstream gradient),
 * the same arithmetic row by row -- for the register-tiled head shapes (C = 2, H = 2 * H2 in {32, 64, 128,
 * 256}; else CGNN_EUNSUPPORTED).  Outputs: H1, fac, logits as the forward; dP [B,H]; slab
 * [cgnn_head_loss_grid(B,H,H2,C)][WD + 1]: the backward's row layout plus one column holding the workgroup's share
 * of the loss (sum of its rows' losses / V), so cgnn_slab_reduce_f32(slab, rows, 1, WD + 1, WD + 1, out,
 * WD + 1) yields the parameter gradients and out[WD] = the mean loss.  V is counted from `labels` by every
 * workgroup (no cross-workgroup wait); label rules as cgnn_cross_entropy_f32. */
int cgnn_head_loss_grid(int32_t B, int32_t H, int32_t H2, int32_t C);   /* rows of cgnn_head_loss_f32's slab */
int cgnn_head_loss_f32(const float* P, int32_t B, int32_t H, int32_t H2, int32_t C, const float* W1,
                       const float* b1, const float* W2, const float* b2, const int64_t* labels,
                       float p_drop, uint64_t seed, const uint32_t* seed_dev, float* H1, float* fac,
                       float* logits, float* dP, float* slab, int64_t slab_bytes, void* stream);

#ifdef __cplusplus
}
#endif

/* Entry points declared in headers of their own; including cgnn.h includes them. */
#include "cgnn_butterworth.h"
#include "cgnn_optim.h"
#include "cgnn_knn.h"
#include "cgnn_modules.h"
#include "cgnn_mst.h"
#include "cgnn_activity.h"
#include "cgnn_pagerank.h"
#include "cgnn_group.h"
#include "cgnn_core.h"
#include "cgnn_rw.h"
#include "cgnn_rank.h"
#include "cgnn_kendall.h"

#endif /* CGNN_H */
