/*
 * msha_gnn.h -- C ABI of the MI355X (gfx950) MSHA-GNN attention library.
 *
 * The reference (Sienna12321/MSHA--GNN @ 2025-01-17) has no FFI: its hot path is
 * the Python nn.Module surface that train.py / LLP.py call, computed by dense
 * ATen ops.  Each entry point below replaces one dense op chain of that surface;
 * the comment on each cites the reference lines it stands in for.  The Python
 * host layer (msha--gnn_amd/) binds these with ctypes.
 *
 * Conventions
 *   - All pointers are DEVICE pointers to caller-owned, contiguous buffers; the
 *     library never allocates.  Temporary space is passed in as a workspace whose
 *     size a *_workspace_size() query returns.
 *   - Every call is stream-ordered and asynchronous on `stream` (a hipStream_t;
 *     NULL = the legacy default stream).  No host synchronisation, no global
 *     mutable state: calls are re-entrant and graph-capturable.
 *   - Return 0 (MSHA_OK) or a negative MSHA_ERR_* code; msha_last_error() gives a
 *     thread-local message.  No C++ exception crosses the ABI.
 *   - Floating-point buffers are fp32 unless stated.  Node tables are row-major
 *     (rows, heads, feat) with the head index outer; per-edge arrays are
 *     (edges, heads) in CSR edge order.
 *   - Graph = the mask `adj > 0` of an (n_rows x n_cols) adjacency as CSR
 *     (row-major edge order == torch.nonzero order).  A row without edges is
 *     stored as a VIRTUAL FULL ROW (all n_cols columns, rowflag = 1): the
 *     reference's softmax of an all -9e15 row is uniform over every column
 *     (Ablation.py:268-270), and so is the GAL's mask/deg (GAT.py:29-31).
 */
#ifndef MSHA_GNN_H_
#define MSHA_GNN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSHA_ABI_VERSION 16

#if defined(__GNUC__) || defined(__clang__)
#define MSHA_API __attribute__((visibility("default")))
#else
#define MSHA_API
#endif

enum {
  MSHA_OK = 0,
  MSHA_ERR_ARG = -1,         /* bad size / null pointer / unsupported shape */
  MSHA_ERR_UNSUPPORTED = -2, /* shape combination without a compiled kernel */
  MSHA_ERR_HIP = -3          /* a HIP runtime call failed (see msha_last_error) */
};

typedef void* msha_stream_t; /* hipStream_t */

/* Storage type of node-feature tables (h, u, v, dU, dV, dh): fp32, or bf16 with
 * fp32 arithmetic (loads widen, stores round to nearest even).  Scores, softmax
 * statistics, per-edge values and their gradients are always fp32. */
enum { MSHA_DTYPE_F32 = 0, MSHA_DTYPE_BF16 = 1 };

/* Graph descriptor.  Built by msha_graph_count / msha_graph_fill from a dense
 * adjacency, or by the caller from its own CSR.  The CSC view and the column
 * chunk plan are needed only by msha_csc_aggregate. */
typedef struct msha_graph {
  int64_t n_rows, n_cols, n_edges;
  const int32_t* rowptr;  /* n_rows + 1 */
  const int32_t* col;     /* n_edges, column of each edge */
  const uint8_t* rowflag; /* n_rows, 1 = virtual full row (nullable: none) */
  const int32_t* colptr;  /* n_cols + 1 (CSC) */
  const int32_t* csc_row; /* n_edges, source row of each CSC slot */
  const int32_t* csc_eid; /* n_edges, CSR edge id of each CSC slot (NULL: the slot IS the
                           * edge id -- a CSR presented as a CSC, msha_csc_aggregate only) */
  /* CSC work split: chunk c covers CSC slots [chunk_start[c], chunk_end[c]) of
   * column chunk_col[c]; a column with more than one chunk is listed in
   * multi_col with its first chunk and chunk count (partials summed in order). */
  int64_t n_chunks;
  const int32_t* chunk_col;
  const int32_t* chunk_start;
  const int32_t* chunk_end;
  int64_t n_multi;
  const int32_t* multi_col;
  const int32_t* multi_first;
  const int32_t* multi_count;
  /* n_edges, CSC slot of each CSR edge (the inverse of csc_eid; nullable).  When set,
   * msha_edge_attention_bwd_fused may keep its per-edge de scratch in CSC slot order
   * (large graphs): the column pass writes it contiguously and the row pass gathers it
   * through this map (ABI 3). */
  const int32_t* csr_slot;
  /* n_rows, graphs with n_cols <= 32 (ABI 13; nullable): bit j of rowmask[i] is set when
   * row i has an edge to column j (virtual full rows: every column).  Built from the CSR
   * by msha_graph_rowmask; the bipartite kernels walk these masks instead of col. */
  const uint32_t* rowmask;
} msha_graph;

/* Same-group adjacency of the full MSHA layer (city and province, dataset.py:260-277
 * builds them as dense N x N masks): group id per node, and per group the sorted
 * member list (CSR: gptr over gmem). */
typedef struct msha_groups {
  int64_t n_nodes;
  const int32_t* gid3;  /* n_nodes: city group of each node */
  const int32_t* gptr3; /* n_city_groups + 1 */
  const int32_t* gmem3; /* n_nodes: members, grouped, ascending */
  const int32_t* gid4;  /* province */
  const int32_t* gptr4;
  const int32_t* gmem4;
  int64_t max_group; /* largest group (either kind): sizes the backward's chunking */
} msha_groups;

MSHA_API int msha_abi_version(void);
MSHA_API const char* msha_last_error(void);
/* Diagnostic (ABI 9): per-wave timeline of the skinny projection / weight-gradient kernels
 * into a device buffer of `slots` x 64 uint64 words (NULL: off).  Only a library built with
 * -DSK_TIMELINE records (build.py --variant timeline); otherwise MSHA_ERR_UNSUPPORTED. */
MSHA_API int msha_debug_timeline(void* buf, int64_t slots);
/* Diagnostic: the model head's split backward row pass (head_bwd_rows2) stamps per-block
 * marks into buf (>= 2048 x 64 uint64, device memory; NULL removes it).  Same build
 * condition as msha_debug_timeline. */
MSHA_API int msha_debug_head_timeline(void* buf);
/* Diagnostic: the MFMA bipartite kernels (edge_bip3.hip) stamp per-wave marks into buf
 * (slots x 64 uint64 words, device memory: forward waves in the first half of the slots,
 * backward waves in the second; NULL removes it).  Same build condition. */
MSHA_API int msha_debug_bip_timeline(void* buf, int64_t slots);

/* ---------------------------------------------------------------- dropout --- */
/* Dropout under HIP-graph replay.  Every dropout draw of the library is Philox4x32-10
 * keyed on (seed, offset, element); seeds are kernel arguments, so a captured graph
 * would replay the same masks.  With a device counter installed here (a uint64 in
 * device memory, NULL = none), each draw adds (*counter << 32) to its offset, read on
 * the device at draw time: the caller increments *counter inside the captured region
 * and every replay draws fresh masks.  One slot per device: a launch on a stream of
 * device d uses device d's counter (device < 0: the current device).  Set it before the
 * launches it should apply to (launch-time snapshot of the pointer, not the value). */
MSHA_API int msha_set_rng_counter(int32_t device, const uint64_t* counter);
/* the counter installed for `device` (< 0: current device), NULL if none */
MSHA_API const uint64_t* msha_get_rng_counter(int32_t device);
/* (ABI 15) A replayed step's feed: copies `bytes` from src to dst (device memory) and adds 1
 * to *counter (NULL: no counter) in ONE stream-ordered launch, so a graph whose counter
 * increment is left to its feed (msha_gnn_amd.step.GraphedStep.replay(feed=...)) starts
 * with its first kernel instead of an add node. */
MSHA_API int msha_feed_step(void* dst, const void* src, int64_t bytes, uint64_t* counter,
                            msha_stream_t stream);

/* keep[i] = 1 iff element i survives F.dropout(p) under (seed, offset).  The
 * kernels below draw exactly these masks (stream-ordered Philox4x32-10), which
 * is how tests inject the same mask into the CPU oracle. */
MSHA_API int msha_dropout_keep_mask(uint64_t seed, uint64_t offset, int64_t n, float p, uint8_t* keep,
                           msha_stream_t stream);

/* ------------------------------------------------------- graph ingestion --- */
/* dataset.py:279-288 (HigherDataset.inter_adjacent): adj[source[k], recipient[k]] += 1.
 * Counts are accumulated exactly in int32 (workspace: n_rows*n_cols int32). */
MSHA_API int msha_inter_adjacency(const int64_t* source, const int64_t* recipient, int64_t n_flows,
                         int64_t n_rows, int64_t n_cols, float* adj, int32_t* counts_ws,
                         msha_stream_t stream);

/* model.py:95-100 (normalize_adjacency_matrix): out = (adj * d) * d, d = colsum^-1/2;
 * a zero column sum spreads NaN to every entry, as the reference's two mm's do.
 * Workspace: n_cols + 1 floats. */
MSHA_API int msha_normalize_adjacency(const float* adj, int64_t n_rows, int64_t n_cols, float* out,
                             float* col_ws, msha_stream_t stream);

/* Ablation.py:268 / GAT.py:30 mask `adj > 0` -> CSR + CSC.  Two phases: count
 * (row/column degrees incl. virtual rows, rowptr/colptr scans), then the caller
 * reads rowptr[n_rows] (= n_edges), allocates, and fills.  Deterministic:
 * CSC slots of a column are in ascending row order. */
MSHA_API size_t msha_graph_workspace_size(int64_t n_rows, int64_t n_cols);
MSHA_API int msha_graph_count(const float* adj, int64_t n_rows, int64_t n_cols, int32_t* rowptr,
                     int32_t* colptr, uint8_t* rowflag, void* ws, size_t ws_bytes,
                     msha_stream_t stream);
/* rowmask[i] = OR over row i's CSR edges of (1 << col) for a graph with n_cols <= 32
 * (g->rowptr, g->col; g->rowmask is not read).  ABI 13. */
MSHA_API int msha_graph_rowmask(const msha_graph* g, uint32_t* rowmask, msha_stream_t stream);
MSHA_API int msha_graph_fill(const float* adj, int64_t n_rows, int64_t n_cols, const int32_t* rowptr,
                    const int32_t* colptr, const uint8_t* rowflag, int32_t* col,
                    int32_t* csc_row, int32_t* csc_eid, void* ws, size_t ws_bytes,
                    msha_stream_t stream);

/* --------------------------------------------------------- attention core --- */
/* Fused edge score + per-row segmented softmax + attention-weighted gather.
 * Replaces Ablation.py:266-271,274 (OursLayer3: e12 = lrelu(cat(h1_j,h2_i) @ a),
 * where/softmax/dropout, u = att @ h1), per head h:
 *   s_e   = lrelu(el[i,h] + er[j,h], neg_slope)      (0 on virtual rows)
 *   att_e = softmax over row i of s
 *   u[i]  = sum_e dropout(att_e) * hc[j]             hc: (n_cols, heads, feat)
 * Outputs u (n_rows, heads, feat), lse (n_rows, heads) = log-sum-exp of the row's
 * scores (the backward recomputes att from it) and, if attd != NULL, the
 * post-dropout attention (n_edges, heads).  u_lo (nullable, bf16 tables only): the
 * rounding residual of the bf16 u (u32 - bf16(u32), stored bf16); the backward's
 * D = dU . u then reads u + u_lo, so a degree-1 row's d_el stays ~0 instead of
 * carrying the 2^-9 rounding of u.
 * Supported (heads, feat): heads in {1,2,4,8}, feat in {8,16,32,64,128} (see
 * msha_edge_attention_supported).  dtype (MSHA_DTYPE_*) is the storage type of the
 * tables hc / u (and hs, dU, dV, d_hs, table, out below); fp32 arithmetic either way. */
MSHA_API int msha_edge_attention_supported(int32_t heads, int32_t feat);
MSHA_API int msha_edge_attention_fwd(const msha_graph* g, int32_t heads, int32_t feat,
                                     int32_t dtype, const float* el, const float* er,
                                     const void* hc, float neg_slope, float drop_p,
                                     uint64_t seed, uint64_t offset, void* u, void* u_lo,
                                     float* lse, float* attd, msha_stream_t stream);
/* The same forward that also writes the row terms of the fused backward (ABI 8), with
 * c_ij = lrelu'(el_i + er_j) (1 when > 0, else neg_slope):
 *   uc (n_rows, heads, feat) fp32 = sum_j c_ij attd_ij hc[j]   (attd: post-dropout)
 *   qc (n_rows, heads)       fp32 = sum_j c_ij att_ij          (att: pre-dropout)
 * so d_el_i = dU_i . uc_i - D_i qc_i (D_i = dU_i . u_i) needs no per-edge de in CSR
 * order.  uc and qc together or both NULL (= msha_edge_attention_fwd).  Needs the
 * batched forward (MSHA_ERR_UNSUPPORTED otherwise); msha_edge_attention_rowterms_preferred
 * says whether a graph should use them (once the per-edge de of
 * msha_edge_attention_bwd_fused would leave the Infinity Cache, and for fp32 tables on
 * graphs whose rows average >= 8 edges). */
MSHA_API int msha_edge_attention_rowterms_preferred(const msha_graph* g, int32_t heads,
                                                    int32_t feat, int32_t dtype);
MSHA_API int msha_edge_attention_fwd_ex(const msha_graph* g, int32_t heads, int32_t feat,
                                        int32_t dtype, const float* el, const float* er,
                                        const void* hc, float neg_slope, float drop_p,
                                        uint64_t seed, uint64_t offset, void* u, void* u_lo,
                                        float* lse, float* attd, float* uc, float* qc,
                                        msha_stream_t stream);

/* Row half of the backward (autograd of the chain above; Ablation.py:266-274):
 *   g_e  = dU[i]·hc[j] (+ dV[j]·hs[i] when dV != NULL: the v = att^T @ h2 branch,
 *          Ablation.py:273)
 *   ds_e = att_e * (drop(g_e) - sum_row att*drop(g)),  de_e = ds_e * lrelu'(pre_e)
 * Writes d_el (n_rows, heads) = row sums of de, de (n_edges, heads), attd
 * (n_edges, heads) = post-dropout attention, and d_hs (n_rows, heads, feat) =
 * sum_e attd_e dV[j] when dV != NULL.  The column half (d_er, d_hc) is
 * msha_csc_aggregate over (attd, de).  row_coef (n_rows, heads), nullable: an extra
 * gradient row_coef[i] * exp(attd_e) on the attention of row i -- the full MSHA
 * layer's normaliser sums exp(attention_inter) of its batch rows (Ours.py:84-86).
 * edge_ld: floats between consecutive edges in de / attd (0 = heads); with
 * edge_ld = 2*heads and attd = de + heads the two share one 2H-float record per edge,
 * which msha_csc_aggregate then reads as one 64-B segment (w = attd, x = de).
 * u_lo: the forward's u_lo (nullable; bf16 tables). */
MSHA_API int msha_edge_attention_bwd_rows(const msha_graph* g, int32_t heads, int32_t feat,
                                          int32_t dtype, const float* el, const float* er,
                                          const void* hc, const float* lse, const void* u,
                                          const void* u_lo, const void* dU, const void* hs, const void* dV,
                                          const float* row_coef, float neg_slope, float drop_p,
                                          uint64_t seed, uint64_t offset, float* d_el, float* de,
                                          float* attd, int32_t edge_ld, void* d_hs,
                                          msha_stream_t stream);

/* Bipartite small-M attention (ABI 11): the repo's own adjacency shape, N sources x
 * M recipients with M * heads * feat <= 4096 (M = 32 at 2 heads x 64: every shipped
 * year).  The column side (hc, er, dV) stays in LDS and the column reductions run in
 * per-wave LDS slabs beside the row work, so one launch (+ a block-partial reduce)
 * replaces msha_edge_attention_fwd + msha_csc_aggregate (v) and one replaces
 * msha_edge_attention_bwd_rows + msha_csc_aggregate (d_hc, d_er).  Deterministic (wave
 * and block order), no atomics; the rows of g must have distinct columns (every CSR the
 * library builds does).  Reference: Ablation.py:266-274, Ours.py:84-86.
 *   fwd: u, lse, attd (nullable), v = attd^T hs (hs, v: both or neither).  u_lo as in
 *        msha_edge_attention_fwd.  Same dropout stream (element e * heads + h).
 *   bwd: d_el, d_er, d_hc, and with dV: d_hs = attd dV (hs, dV, d_hs together);
 *        row_coef (nullable) as in msha_edge_attention_bwd_rows.  No u / u_lo needed:
 *        D_i = sum_e attd_e g_e.
 * ws: msha_bip_workspace_size bytes (block partials; fwd needs it only with hs). */
MSHA_API int msha_bip_supported(const msha_graph* g, int32_t heads, int32_t feat, int32_t dtype);
MSHA_API size_t msha_bip_workspace_size(const msha_graph* g, int32_t heads, int32_t feat);
MSHA_API int msha_bip_attention_fwd(const msha_graph* g, int32_t heads, int32_t feat,
                                    int32_t dtype, const float* el, const float* er,
                                    const void* hc, const void* hs, float neg_slope,
                                    float drop_p, uint64_t seed, uint64_t offset, void* u,
                                    void* u_lo, float* lse, float* attd, void* v, void* ws,
                                    size_t ws_bytes, msha_stream_t stream);
MSHA_API int msha_bip_attention_bwd(const msha_graph* g, int32_t heads, int32_t feat,
                                    int32_t dtype, const float* el, const float* er,
                                    const void* hc, const float* lse, const void* dU,
                                    const void* hs, const void* dV, const float* row_coef,
                                    float neg_slope, float drop_p, uint64_t seed,
                                    uint64_t offset, float* d_el, float* d_er, void* d_hc,
                                    void* d_hs, void* ws, size_t ws_bytes,
                                    msha_stream_t stream);
/* The source-row count from which msha_bip_attention_fwd / _bwd take the MFMA row-mask
 * kernels (graphs with msha_graph.rowmask, 2 heads x 64; below it the mask forward and the
 * CSR-walk backward; default 131072, or MSHA_BIP2_BWD_MIN_ROWS): rows >= 0 sets it for
 * the process and returns the previous value, rows < 0 only returns it. */
MSHA_API int64_t msha_bip2_bwd_min_rows(int64_t rows);
/* (ABI 16, added: a new symbol only, MSHA_ABI_VERSION stays 16) Host-only query: which
 * kernel family msha_bip_attention_fwd (called with / without u_lo) and _bwd run for these
 * arguments under the process's knobs (MSHA_BIP2, MSHA_BIP3, MSHA_BIP3_BWD32, the row count
 * above), as fwd + 16 * bwd with MSHA_BIP_* below; 0 = not covered (msha_bip_supported is
 * 0).  The launches ask the same function (csrc/bip_route.h).  Reads g's sizes and whether
 * rowmask is set, no device memory; nothing is launched. */
#define MSHA_BIP_NONE 0
#define MSHA_BIP_WALK 1 /* CSR walk */
#define MSHA_BIP_MASK 2 /* row masks */
#define MSHA_BIP_MFMA 3 /* row masks on the matrix cores */
MSHA_API int32_t msha_bip_route(const msha_graph* g, int32_t heads, int32_t feat, int32_t dtype,
                                float neg_slope, float drop_p, int32_t has_u_lo);
/* (ABI 15) The Ours intra forward's dropout draws: mode 1 packs the matched (batch entry,
 * node) pairs of consecutive nodes into one Philox draw per <= 64 pairs (default), mode 0
 * draws per node for the whole batch (MSHA_OURS_PACK_DRAWS=0 starts with it); both give
 * the same bits.  Returns the previous mode; mode < 0 only queries. */
MSHA_API int32_t msha_ours_pack_draws(int32_t mode);
/* (ABI 15) The fp32 weight gradient's kernel (projection backward, dW = X^T D'): mode 0 =
 * auto (default: from 131,072 rows -- MSHA_WGRAD_S3_MIN_ROWS -- the operands split into
 * three bf16 terms in registers, six products on the bf16 MFMA; the exact-fp32 MFMA below),
 * 1 = exact-fp32 MFMA, 3 = the register split at any size (MSHA_WGRAD=fp32 / s3 start the
 * process with 1 / 3; any other word is ignored).  Returns the previous mode; any other
 * value of mode (negative, 2 -- a removed kernel's number --, above 3) only queries. */
MSHA_API int32_t msha_wgrad_kernel(int32_t mode);

/* Column-side (transposed) aggregate over the CSC view:
 *   out[j]   = sum_{e in col j} w[e] * table[row(e)]   (per head; table (n_rows,heads,feat))
 *   out_x[j] = sum_{e in col j} x[e]                   (when x != NULL)
 * Forward v = attd^T @ h2 (Ablation.py:273) and backward d_hc = attd^T @ dU,
 * d_er = colsum(de).  With heads = 1 and w = the adjacency values it is the GCN
 * SpMM adj^T @ support (model.py:37); on a CSR-as-CSC view (colptr = rowptr,
 * csc_row = col, csc_eid = NULL, chunks over rows) it is adj @ support.
 * edge_ld: floats between consecutive edges in w / x (0 = heads).
 * Long columns are split into chunks whose partial sums are added in a fixed order:
 * deterministic, no atomics. */
MSHA_API size_t msha_csc_aggregate_workspace_size(const msha_graph* g, int32_t heads, int32_t feat);
MSHA_API int msha_csc_aggregate(const msha_graph* g, int32_t heads, int32_t feat, int32_t dtype,
                                const float* w, const float* x, int32_t edge_ld,
                                const void* table, void* out, float* out_x, void* ws,
                                size_t ws_bytes, msha_stream_t stream);

/* Fused backward of u = drop(att) @ hc alone (no v branch, no row coefficients):
 * the same d_el, d_er, d_hc as msha_edge_attention_bwd_rows + msha_csc_aggregate,
 * bitwise, from one pass over the CSC (the column owns hc_j, so dU_i . hc_j comes from
 * the dU[i] gather the column pass makes anyway) plus two light row passes.
 * Replaces the reference's autograd of Ablation.py:266-274 for that case.
 * de (n_edges, heads) fp32: scratch (left holding de in CSR edge order, or in CSC slot
 * order when g->csr_slot is set and de exceeds 192 MB).
 * ws: msha_edge_attention_bwd_fused_workspace_size bytes.  Needs the CSC view with
 * csc_eid.  u_lo: the forward's u_lo (nullable; bf16 tables). */
MSHA_API size_t msha_edge_attention_bwd_fused_workspace_size(const msha_graph* g,
                                                             int32_t heads, int32_t feat);
MSHA_API int msha_edge_attention_bwd_fused(const msha_graph* g, int32_t heads, int32_t feat,
                                           int32_t dtype, const float* el, const float* er,
                                           const void* hc, const float* lse, const void* u,
                                           const void* u_lo, const void* dU, float neg_slope,
                                           float drop_p,
                                           uint64_t seed, uint64_t offset, float* d_el,
                                           float* d_er, void* d_hc, float* de, void* ws,
                                           size_t ws_bytes, msha_stream_t stream);
/* The same with the forward's row terms (uc, qc from msha_edge_attention_fwd_ex, same
 * dropout seed/offset): d_el is finished in the row-statistics pass, the column pass
 * stores no de and no row sum runs (de may be NULL).  uc = qc = NULL: the call above. */
MSHA_API int msha_edge_attention_bwd_fused_ex(
    const msha_graph* g, int32_t heads, int32_t feat, int32_t dtype, const float* el,
    const float* er, const void* hc, const float* lse, const void* u, const void* u_lo,
    const void* dU, float neg_slope, float drop_p, uint64_t seed, uint64_t offset,
    const float* uc, const float* qc, float* d_el, float* d_er, void* d_hc, float* de, void* ws,
    size_t ws_bytes, msha_stream_t stream);

/* The column pass with the projection's weight gradient inside (ABI 16, added: new symbols
 * only, MSHA_ABI_VERSION stays 16).  Precondition: the graph is square and hc is the
 * projection's own output, hc = h = X W (row j of the projection is column j of the
 * attention), X (n_cols, K = 128) fp32 with row pitch ldx floats, a_l, a_r (heads * feat)
 * fp32, all 16-byte aligned.  Arguments and outputs as msha_edge_attention_bwd_fused_ex with
 * row terms (uc, qc required; d_el, d_er, d_hc are the same bits); in addition the column
 * pass leaves, in wg_ws, nb slabs of 128 x 128 floats (block b: X^T D' over its columns,
 * D'_j = d_hc_j + d_el_j (x) a_l + d_er_j (x) a_r) and the partial sums of d_el (x) h and
 * d_er (x) h; msha_wgrad_reduce adds them in block order into dW (128 x 128, pitch ldc), dal
 * and dar (heads * feat).  cut (nb + 1 int32, device): the blocks' column ranges,
 * msha_col_ranges over a host copy of colptr (int64) -- a function of the graph and nb only,
 * so results repeat bit for bit.  nb = msha_edge_attention_bwd_fused_wgrad_route(...), a
 * host-only query (rowterms / er_table: the call has row terms / reads the er table, not
 * a_r); 0 = not covered (fp32, heads x feat = 8 x 16, 4 x 32, 2 x 64 or 1 x 128, K 128, no multi-chunk column, tables under
 * 2 GiB, MSHA_BWD_WGRAD != 0) and the entry returns MSHA_ERR_UNSUPPORTED: the caller runs
 * msha_edge_attention_bwd_fused_ex and its own weight gradient. */
MSHA_API int32_t msha_edge_attention_bwd_fused_wgrad_route(
    const msha_graph* g, int32_t heads, int32_t feat, int32_t dtype, int64_t K, int64_t ldx,
    int32_t rowterms, int32_t er_table, const void* X, const float* al, const float* ar);
MSHA_API int32_t msha_col_range_blocks(int64_t n_cols); /* the nb the route answers with */
MSHA_API int msha_col_ranges(const int64_t* colptr, int64_t n_cols, int32_t nb, int32_t* cut);
MSHA_API size_t msha_edge_attention_bwd_fused_wgrad_workspace_size(int32_t nb);
MSHA_API int msha_edge_attention_bwd_fused_wgrad(
    const msha_graph* g, int32_t heads, int32_t feat, int32_t dtype, const float* el,
    const float* er, const void* hc, const float* lse, const void* u, const void* u_lo,
    const void* dU, float neg_slope, float drop_p, uint64_t seed, uint64_t offset,
    const float* uc, const float* qc, float* d_el, float* d_er, void* d_hc, float* de, void* ws,
    size_t ws_bytes, const void* X, int64_t ldx, int64_t K, const float* a_l, const float* a_r,
    const int32_t* cut, int32_t nb, void* wg_ws, size_t wg_ws_bytes, msha_stream_t stream);
MSHA_API int msha_wgrad_reduce(const void* wg_ws, int32_t nb, float* dW, int64_t ldc, float* dal,
                               float* dar, msha_stream_t stream);

/* Scores from the gathered row (ABI 9).  Every caller of the u = att @ hc path scores
 * the gathered table itself: er[j,h] = hc[j,h,:] . a_r[h,:] (Ablation.py:266-267 --
 * a[:F] against h1_j, the rows u aggregates).  Given a_r ((heads, feat) fp32, 16-byte
 * aligned) instead of er, the forward computes er_j from the row its gather lanes hold
 * (no per-edge er gather: a 4*heads-byte piece that costs a cache line per edge once
 * the er table leaves L2) and the fused backward's column pass recomputes it from hc_j
 * in the same order, so both passes see the same scores bit for bit.  The outputs and
 * their meaning are those of msha_edge_attention_fwd_ex (without attd) and
 * msha_edge_attention_bwd_fused_ex; d_er is still the gradient w.r.t. er (the caller
 * routes it to whatever produced er = hc . a_r).  Supported where
 * msha_edge_attention_row_scores_supported says so (one 16-byte piece per lane:
 * heads*feat*sizeof <= 1024 B; tables under 2 GiB); MSHA_ERR_UNSUPPORTED otherwise. */
MSHA_API int msha_edge_attention_row_scores_supported(const msha_graph* g, int32_t heads,
                                                      int32_t feat, int32_t dtype);
/* whether the library's default is to use them (wherever supported, fp32 and bf16,
 * since round 4); MSHA_ROW_SCORES=0/1 in the environment forces it */
MSHA_API int msha_edge_attention_row_scores_preferred(const msha_graph* g, int32_t heads,
                                                      int32_t feat, int32_t dtype);
MSHA_API int msha_edge_attention_fwd_rs(const msha_graph* g, int32_t heads, int32_t feat,
                                        int32_t dtype, const float* el, const float* ar,
                                        const void* hc, float neg_slope, float drop_p,
                                        uint64_t seed, uint64_t offset, void* u, void* u_lo,
                                        float* lse, float* uc, float* qc, msha_stream_t stream);
MSHA_API int msha_edge_attention_bwd_fused_rs(
    const msha_graph* g, int32_t heads, int32_t feat, int32_t dtype, const float* el,
    const float* ar, const void* hc, const float* lse, const void* u, const void* u_lo,
    const void* dU, float neg_slope, float drop_p, uint64_t seed, uint64_t offset,
    const float* uc, const float* qc, float* d_el, float* d_er, void* d_hc, float* de, void* ws,
    size_t ws_bytes, msha_stream_t stream);

/* ----------------------------------------------- GraphAttentionLayer (GAL) --- */
/* GAT.py:20-35 / Ablation.py:100-115.  The layer's score is constant along a row
 * (it concatenates h_i with itself), so its attention is mask/deg (uniform on
 * virtual rows) and the layer is out = elu(dropout(mask/deg) * h), h (n_rows, n_cols).
 * The bwd returns dh = dout * elu'(z) * dropout(mask/deg). */
MSHA_API int msha_gal_fwd(const msha_graph* g, const float* h, float drop_p, uint64_t seed,
                 uint64_t offset, float* out, msha_stream_t stream);
MSHA_API int msha_gal_bwd(const msha_graph* g, const float* h, const float* dout, float drop_p,
                 uint64_t seed, uint64_t offset, float* dh, msha_stream_t stream);

/* ------------------------------------------------ projections (MFMA, fp32) --- */
/* Ablation.py:262-263 (h1 = R @ W1, h2 = S @ W2), GAT.py:21 (h = input @ W) and the
 * gradients of those products.  C = A @ B with arbitrary element strides
 * (A[m,k] = A[m*sAm + k*sAk], B[k,n] = B[k*sBk + n*sBn]), C row-major with ldc.
 * v_mfma_f32_16x16x4_f32: exact fp32 FMA chains.  splits > 1 splits K over
 * workgroups (for long reductions such as dW = X^T dH over all rows); partial
 * slabs are added in split order (deterministic) and beta (0 or 1) selects
 * C = sum or C += sum.  Workspace: msha_gemm_workspace_size(M, N, splits). */
MSHA_API size_t msha_gemm_workspace_size(int64_t M, int64_t N, int32_t splits);
MSHA_API int msha_gemm_f32(int64_t M, int64_t N, int64_t K, const float* A, int64_t sAm,
                           int64_t sAk, const float* B, int64_t sBk, int64_t sBn, float* C,
                           int64_t ldc, float beta, int32_t splits, void* ws, size_t ws_bytes,
                           msha_stream_t stream);

/* host-only (ABI 16, added): the operand staging the tiled kernels would use for these
 * operands -- MSHA_GEMM_LOADER_SCALAR (element-wise, any strides) or MSHA_GEMM_LOADER_VEC
 * (16-byte loads) or'ed with _AK (A's k is contiguous, else its m) and _BNF (B's n is
 * contiguous, else its k).  The answer of the function the launch itself asks.
 * msha_gemm_f32_loader: 16-byte staging needs, for each operand, unit stride along one
 * dimension (B's n is tried before its k, A's k before its m), the other stride a multiple
 * of 4, a 16-byte aligned base, and a multiple of 4 for the extent along the unit stride
 * (K for a k-contiguous operand, M for an m-contiguous A, N for an n-contiguous B); one
 * operand failing sends both to the scalar loader.  (The resident weight-gradient kernel
 * takes M = N = 128, K >= 4096, splits >= 16 before the tiled kernel is asked.)
 * msha_gemm_bf16_loader: -1 where msha_gemm_bf16 returns MSHA_ERR_UNSUPPORTED for an
 * operand's layout (its rule is with msha_gemm_bf16 below; A's and B's k are tried first). */
#define MSHA_GEMM_LOADER_SCALAR 0
#define MSHA_GEMM_LOADER_BNF 1
#define MSHA_GEMM_LOADER_AK 2
#define MSHA_GEMM_LOADER_VEC 4
MSHA_API int32_t msha_gemm_f32_loader(int64_t M, int64_t N, int64_t K, const float* A,
                                      int64_t sAm, int64_t sAk, const float* B, int64_t sBk,
                                      int64_t sBn);
MSHA_API int32_t msha_gemm_bf16_loader(int64_t M, int64_t N, int64_t K, const void* A,
                                       int64_t sAm, int64_t sAk, const void* B, int64_t sBk,
                                       int64_t sBn);

/* host-only (ABI 16, added): which kernel family a call with these arguments runs -- the
 * answer of the predicates the launches themselves ask; nothing is launched and no pointer
 * is dereferenced (only its alignment and NULL-ness enter).
 *   MSHA_ROUTE_TILED     the tiled GEMM (gemm.hip / gemm_bf16.hip)
 *   MSHA_ROUTE_RESIDENT  a resident-W kernel on the operands' own type (exact-fp32 MFMA or bf16)
 *   MSHA_ROUTE_SPLIT     a resident-W kernel on split-bf16 products of fp32 operands
 * The resident kernels take K and heads*feat (N) in {64, 128}, at least 1,024 rows, 16-byte
 * aligned X / W / h (G / G2 / W / out), and row byte counts below 2^31.  The environment
 * knob MSHA_SKINNY=0 sends every call to the tiled kernels.
 * msha_project_scores_route (dtype MSHA_DTYPE_F32 / _BF16; al, ar as the call's; h the output):
 *   with a score vector feat must be 16, 32, 64 or heads*feat (bf16: feat 8 is tiled; fp32:
 *   feat 4 and 8 are tiled); fp32 from MSHA_PROJ_SPLIT_MIN_ROWS (65,536) rows is _SPLIT.
 *   sched (nullable, 3 ints): waves per block, column parts per tail tile and staged columns
 *   per pass of the chosen instance (0 0 0 when tiled).
 * msha_pair_linear_route: both gathers given (gi, gj), ldg / ldg2 multiples of 4; _SPLIT is
 *   the windowed gather (known g_rows / g2_rows, tables within 4 GiB less 512 bytes, n_pairs * N * 4 < 2^31),
 *   _RESIDENT the plain one.  msha_pair_linear_bf16_route: ldg / ldg2 multiples of 8.
 * msha_gemm_f32_head_outer_route: _RESIDENT where msha_gemm_f32_head_outer with operand 0
 *   computes dX = (dh + de (x) a [+ de2 (x) a2]) W^T on the resident-W kernel: beta 0, A
 *   (M x K) and C dense row-major, B given as W (N x K) row-major, feat >= 16. */
#define MSHA_ROUTE_TILED 0
#define MSHA_ROUTE_RESIDENT 1
#define MSHA_ROUTE_SPLIT 2
MSHA_API int32_t msha_project_scores_route(int64_t M, int64_t K, int32_t heads, int32_t feat,
                                           int32_t dtype, const void* X, const void* W,
                                           const float* al, const float* ar, const void* h,
                                           int32_t* sched);
MSHA_API int32_t msha_pair_linear_route(int64_t n_pairs, int64_t K, int64_t N, const float* G,
                                        int64_t ldg, const int64_t* gi, const float* G2,
                                        int64_t ldg2, const int64_t* gj, int64_t g_rows,
                                        int64_t g2_rows, const float* W, const float* out);
MSHA_API int32_t msha_pair_linear_bf16_route(int64_t n_pairs, int64_t K, int64_t N, const void* G,
                                             int64_t ldg, const int64_t* gi, const void* G2,
                                             int64_t ldg2, const int64_t* gj, const void* W,
                                             const void* out);
MSHA_API int32_t msha_gemm_f32_head_outer_route(int64_t M, int64_t N, int64_t K, const float* A,
                                                int64_t sAm, int64_t sAk, const float* B,
                                                int64_t sBk, int64_t sBn, const float* C,
                                                int64_t ldc, float beta, int32_t operand,
                                                int32_t heads, int32_t feat, const float* de,
                                                const float* a, const float* a2);

/* msha_gemm_f32 with the backward of msha_project_scores folded into one operand's
 * loads: operand 0 (A, M x K, K = heads*feat, sAk = 1) or 1 (B, K x N, N = heads*feat,
 * sBn = 1) is read as X + de (x) a [+ de2 (x) a2], i.e. X[r, c] + de[r, c/feat] a[c].
 * dX = (dh + de (x) a) W^T and dW = X^T (dh + de (x) a) without materialising the sum
 * (replaces msha_add_head_outer + msha_gemm_f32).  MSHA_ERR_UNSUPPORTED when the
 * operands cannot take the 16-byte path (then use those two calls). */
MSHA_API int msha_gemm_f32_head_outer(int64_t M, int64_t N, int64_t K, const float* A,
                                      int64_t sAm, int64_t sAk, const float* B, int64_t sBk,
                                      int64_t sBn, float* C, int64_t ldc, float beta,
                                      int32_t splits, void* ws, size_t ws_bytes, int32_t operand,
                                      int32_t heads, int32_t feat, const float* de,
                                      const float* a, const float* de2, const float* a2,
                                      msha_stream_t stream);

/* The projection's whole parameter backward in one pass over the rows (replaces
 * msha_gemm_f32_head_outer with operand 1 + msha_head_colsum, Ablation.py:262-267
 * backward): C = A (B + de (x) a [+ de2 (x) a2]) (dW = X^T dh'), and
 * cs1[n] = sum_k de[k, n / feat] T[k, n], cs2 likewise with de2 (d_al, d_ar with T the
 * forward's h), T laid out as B (row pitch sBk, unit column stride).  beta = 0.  Only
 * the resident-accumulator weight-gradient shape (M = N = 128, K >= 4096, splits >= 16);
 * MSHA_ERR_UNSUPPORTED (nothing launched) otherwise.  cs_ws: at least
 * msha_head_outer_colsum_workspace_size(N) bytes; ws as msha_gemm_f32. */
MSHA_API size_t msha_head_outer_colsum_workspace_size(int64_t N);
MSHA_API int msha_gemm_f32_head_outer_colsum(
    int64_t M, int64_t N, int64_t K, const float* A, int64_t sAm, int64_t sAk, const float* B,
    int64_t sBk, int64_t sBn, float* C, int64_t ldc, int32_t splits, void* ws, size_t ws_bytes,
    int32_t heads, int32_t feat, const float* de, const float* a, const float* de2,
    const float* a2, const float* T, float* cs1, float* cs2, void* cs_ws, size_t cs_ws_bytes,
    msha_stream_t stream);
/* (ABI 15) The same, where T is the projection's own output X W (Ablation.py:262, h = X @ W;
 * A = X^T): cs1[n] = sum_a W[a, n] G[n / feat, a] with G = de^T X accumulated from the rows
 * the weight gradient already reads, so T is never read.  Equal in real arithmetic; in fp32
 * it differs from the T form by T's own rounding.  heads == 2 and the split-bf16
 * weight-gradient kernel (msha_wgrad_kernel mode 0) only; MSHA_ERR_UNSUPPORTED otherwise. */
MSHA_API int msha_gemm_f32_head_outer_colsum_w(
    int64_t M, int64_t N, int64_t K, const float* A, int64_t sAm, int64_t sAk, const float* B,
    int64_t sBk, int64_t sBn, float* C, int64_t ldc, int32_t splits, void* ws, size_t ws_bytes,
    int32_t heads, int32_t feat, const float* de, const float* a, const float* de2,
    const float* a2, const float* W, int64_t ldw, float* cs1, float* cs2, void* cs_ws,
    size_t cs_ws_bytes, msha_stream_t stream);

/* Projection with the attention-score halves fused into its epilogue:
 *   h = X @ W  (M x heads*feat),  el[m,h] = h[m,h,:] . al[h,:],  er[m,h] = h[m,h,:] . ar[h,:]
 * Replaces Ablation.py:262-267's projection + the (N, M, 2F) score tensor: the
 * score of edge (i, j) is lrelu(el_i + er_j).  al/el and ar/er are optional pairs;
 * feat must be 4, 8, 16, 32, 64 or 128 when a score vector is given. */
/* 1 when msha_project_scores(_bf16) / msha_project_small at this shape compute el / er
 * from the STORED h in the order the row-score edge kernels recompute er_j = h_j . a_r
 * from a gathered row (per 16-byte piece: last element first, fma downwards; then the
 * xor tree over the head's pieces): er is then bit-identical to that recomputation and
 * msha_edge_attention_bwd_fused_ex may read it in place of msha_edge_attention_bwd_fused_rs
 * (ABI 9: every projection path; feat a multiple of 4). */
MSHA_API int msha_project_scores_row_order(int64_t M, int64_t K, int32_t heads, int32_t feat,
                                           int32_t dtype);
MSHA_API int msha_project_scores(int64_t M, int64_t K, int32_t heads, int32_t feat,
                                 const float* X, const float* W, const float* al,
                                 const float* ar, float* h, float* el, float* er,
                                 msha_stream_t stream);

/* bf16 projections (config C3: the same model in bf16), v_mfma_f32_16x16x32_bf16 with
 * fp32 accumulation.  A, B bf16 with element strides as msha_gemm_f32; each operand
 * needs one unit stride (its extent along it a multiple of 8; the other stride a
 * multiple of 8; 16-byte aligned base), else MSHA_ERR_UNSUPPORTED.  C (ldc, N
 * multiples of 8) is fp32 or bf16 (c_dtype).  ho_operand 0 / 1 reads A / B as
 * X + de (x) a [+ de2 (x) a2] (as msha_gemm_f32_head_outer; feat % 8 == 0, A
 * k-contiguous / B n-contiguous), -1 = none.  splits > 1: deterministic split-K with
 * an fp32 slab workspace of msha_gemm_bf16_workspace_size(M, N, splits) bytes. */
MSHA_API size_t msha_gemm_bf16_workspace_size(int64_t M, int64_t N, int32_t splits);
MSHA_API int msha_gemm_bf16(int64_t M, int64_t N, int64_t K, const void* A, int64_t sAm,
                            int64_t sAk, const void* B, int64_t sBk, int64_t sBn, void* C,
                            int64_t ldc, int32_t c_dtype, int32_t splits, void* ws,
                            size_t ws_bytes, int32_t ho_operand, int32_t heads, int32_t feat,
                            const float* de, const float* a, const float* de2, const float* a2,
                            msha_stream_t stream);
/* msha_project_scores on bf16 X (M x K) and W (K x heads*feat): h bf16, el / er fp32
 * from the fp32 accumulators.  K, heads*feat multiples of 8. */
MSHA_API int msha_project_scores_bf16(int64_t M, int64_t K, int32_t heads, int32_t feat,
                                      const void* X, const void* W, const float* al,
                                      const float* ar, void* h, float* el, float* er,
                                      msha_stream_t stream);

/* out = dh + de (x) a [+ de2 (x) a2]  (rows x heads*feat; de (rows, heads), a (heads, feat)):
 * the gradient reaching h through el = h . a (the backward of msha_project_scores). */
MSHA_API int msha_add_head_outer(int64_t rows, int32_t heads, int32_t feat, const float* dh,
                                 const float* de, const float* a, const float* de2,
                                 const float* a2, float* out, msha_stream_t stream);

/* Gradient of the score vectors of msha_project_scores (el = h . al):
 * out1[h, f] = sum_r s1[r, h] h[r, h, f] (and out2 with s2); deterministic row-block
 * partials.  Workspace: msha_head_colsum_workspace_size(rows, heads, feat). */
MSHA_API size_t msha_head_colsum_workspace_size(int64_t rows, int32_t heads, int32_t feat);
MSHA_API int msha_head_colsum(int64_t rows, int32_t heads, int32_t feat, int32_t dtype,
                              const float* s1, const float* s2, const void* T, float* out1,
                              float* out2, void* ws, size_t ws_bytes, msha_stream_t stream);

/* bf16 link scoring (config C5 names a bf16 embedding table): msha_pair_inner_fwd and
 * msha_pair_linear on bf16 tables G / G2 (and a bf16 nn.Linear weight W); fp32
 * products and accumulation, fp32 scores out.  feat / K, N multiples of 8. */
MSHA_API int msha_pair_inner_fwd_bf16(int64_t n_pairs, int32_t feat, const void* G, int64_t ldg,
                                      const int64_t* gi, const void* G2, int64_t ldg2,
                                      const int64_t* gj, float* out, msha_stream_t stream);
MSHA_API int msha_pair_linear_bf16(int64_t n_pairs, int64_t K, int64_t N, const void* G,
                                   int64_t ldg, const int64_t* gi, const void* G2, int64_t ldg2,
                                   const int64_t* gj, const void* W, const float* bias,
                                   int32_t act, float drop_p, uint64_t seed, uint64_t offset,
                                   float* out, msha_stream_t stream);
/* The same with the output dtype chosen (MSHA_DTYPE_F32 or MSHA_DTYPE_BF16): a bf16
 * LinkPredictor in PyTorch returns bf16 scores, and the (n_pairs, N) output is the
 * dominant byte stream of the scorer.  The epilogue (bias, ReLU, dropout, sigmoid) runs
 * in fp32 and rounds once. */
MSHA_API int msha_pair_linear_bf16_ex(int64_t n_pairs, int64_t K, int64_t N, const void* G,
                                      int64_t ldg, const int64_t* gi, const void* G2,
                                      int64_t ldg2, const int64_t* gj, const void* W,
                                      const float* bias, int32_t act, float drop_p,
                                      uint64_t seed, uint64_t offset, int32_t out_dtype,
                                      void* out, msha_stream_t stream);

/* ------------------------------------------------- BatchNorm + LeakyReLU --- */
/* Ablation.py:273-274 / Ours.py:100-101 epilogue: y = lrelu(bn(x)) on (rows, channels)
 * tables (dtype fp32 / bf16; weight, bias, statistics fp32; weight / bias nullable =
 * 1 / 0).  training != 0: batch statistics (mean, invstd = 1/sqrt(var_biased + eps)
 * written to mean / invstd), running_mean / running_var (nullable pair) updated with
 * momentum and the unbiased variance, as torch.nn.BatchNorm1d; training == 0: the
 * running statistics normalise.  Deterministic (fixed-order Welford / Chan combines).
 * Backward (training statistics): dx, dweight = sum dz xhat, dbias = sum dz with
 * dz = dy lrelu'(z).  Workspace: msha_bn_workspace_size(rows, channels) (0 for
 * rows <= 256: one workgroup). */
MSHA_API size_t msha_bn_workspace_size(int64_t rows, int32_t channels);
MSHA_API int msha_bn_lrelu_fwd(int64_t rows, int32_t channels, int32_t dtype, const void* x,
                               const float* weight, const float* bias, float eps, float slope,
                               int32_t training, float momentum, float* running_mean,
                               float* running_var, float* mean, float* invstd, void* y,
                               void* ws, size_t ws_bytes, msha_stream_t stream);
MSHA_API int msha_bn_lrelu_bwd(int64_t rows, int32_t channels, int32_t dtype, const void* x,
                               const void* dy, const float* weight, const float* bias,
                               const float* mean, const float* invstd, float slope, void* dx,
                               float* dweight, float* dbias, void* ws, size_t ws_bytes,
                               msha_stream_t stream);

/* ----------------------------------------------------------- link scoring --- */
/* LLP.py:104-115 LinkPredictor with the caller's gather (LLP.py:233) fused:
 * x_i = G[gi[b]], x_j = G2[gj[b]] (gi / gj NULL: row b).
 * 'mlp' layer: out = act((x_i * x_j) @ W^T + bias), W an nn.Linear weight (N x K);
 * with G2 == NULL and gj == NULL the input is x_i alone (deeper predictor layers);
 * act bits: 1 bias, 2 relu, 4 dropout(drop_p, seed, offset), 8 sigmoid.
 * g_rows / g2_rows: the row counts of G / G2 (every gi / gj index below them; 0 =
 * unknown).  Known counts whose tables fit 4 GiB (less 512 bytes) select the gather kernel with 32-bit
 * buffer offsets (an index outside [0, rows) then reads zeros: negative indices are not
 * wrapped as torch indexing would wrap them, so callers pass valid indices). */
MSHA_API int msha_pair_linear(int64_t n_pairs, int64_t K, int64_t N, const float* G, int64_t ldg,
                              const int64_t* gi, const float* G2, int64_t ldg2,
                              const int64_t* gj, int64_t g_rows, int64_t g2_rows,
                              const float* W, const float* bias, int32_t act,
                              float drop_p, uint64_t seed, uint64_t offset, float* out,
                              msha_stream_t stream);
/* 'inner': out[b] = sigmoid(sum_f x_i[b,f] x_j[b,f]); feat a power of two in [4, 256]. */
MSHA_API int msha_pair_inner_fwd(int64_t n_pairs, int32_t feat, const float* G, int64_t ldg,
                                 const int64_t* gi, const float* G2, int64_t ldg2,
                                 const int64_t* gj, float* out, msha_stream_t stream);
/* 'inner' with the gathered tables' row counts (ABI 14): a pair whose gi / gj index lies
 * outside [0, g_rows) / [0, g2_rows) scores NaN and sets *err = 1 (err nullable) instead
 * of reading past the table.  dtype MSHA_DTYPE_F32 (feat in [4, 256]) or
 * MSHA_DTYPE_BF16 (feat in [8, 512]); replaces the gather of LLP.py:233 + LLP.py:112-115. */
MSHA_API int msha_pair_inner_fwd_ex(int64_t n_pairs, int32_t feat, int32_t dtype, const void* G,
                                    int64_t ldg, const int64_t* gi, int64_t g_rows,
                                    const void* G2, int64_t ldg2, const int64_t* gj,
                                    int64_t g2_rows, int32_t* err, float* out,
                                    msha_stream_t stream);
/* Index validation of a pair batch before a fused gather (LLP.py:233: torch's h[idx]
 * raises for idx outside [-rows, rows) and wraps a negative idx to rows + idx): flags[0]
 * is set to 1 when any gi (gj) lies outside [-g_rows, g_rows) ([-g2_rows, g2_rows)),
 * flags[1] when any is negative.  flags (2 x int32, device) are OR-ed into, never
 * cleared: the caller zeroes them.  gi / gj nullable. */
MSHA_API int msha_pair_index_check(int64_t n_pairs, const int64_t* gi, int64_t g_rows,
                                   const int64_t* gj, int64_t g2_rows, int32_t* flags,
                                   msha_stream_t stream);
/* backward of 'inner' given its output s: dx_i = dout*s*(1-s)*x_j, dx_j = ...*x_i */
MSHA_API int msha_pair_inner_bwd(int64_t n_pairs, int32_t feat, const float* G, int64_t ldg,
                                 const int64_t* gi, const float* G2, int64_t ldg2,
                                 const int64_t* gj, const float* s, const float* dout,
                                 float* dxi, float* dxj, msha_stream_t stream);
/* backward through y = [sigmoid](dropout(relu(z))) given its output y: dz */
MSHA_API int msha_pair_mlp_dz(int64_t n, const float* s, const float* dout, float drop_p,
                              int32_t sigmoid, float* dz, msha_stream_t stream);
/* x = x_i * x_j (dx == NULL), or dx_i = dx * x_j, dx_j = dx * x_i */
MSHA_API int msha_pair_hadamard(int64_t n_pairs, int32_t feat, const float* G, int64_t ldg,
                                const int64_t* gi, const float* G2, int64_t ldg2,
                                const int64_t* gj, const float* dx, float* x_or_dxi, float* dxj,
                                msha_stream_t stream);

/* LinkPredictor with a predictor string other than 'mlp' / 'inner' (LLP.py:104-115 takes
 * neither branch): y = sigmoid(x_i * x_j), (B, F).  dy == NULL: forward into y_or_dxi;
 * else the backward from the forward's y: dx_i into y_or_dxi, dx_j into dxj. */
MSHA_API int msha_pair_hadamard_sigmoid(int64_t n_pairs, int32_t feat, const float* G,
                                        int64_t ldg, const int64_t* gi, const float* G2,
                                        int64_t ldg2, const int64_t* gj, const float* y,
                                        const float* dy, float* y_or_dxi, float* dxj,
                                        msha_stream_t stream);

/* ----------------------------------------------- full MSHA layer (Ours.py) --- */
/* Intra-source attention of a batch (Ours.py:71-101) on top of the inter forward:
 *   e3_b = lrelu(h2[src_b] . a3s), E3 = exp(e3_b); e4/E4 with a4s (a3s = a3[:F] + a3[F:])
 *   SUM_b = |city(src_b)| E3 + |prov(src_b)| E4 + sum_j exp(attd[src_b, j]) (all M columns)
 *   u_out[n] = u_inter[n] + sum_{b: same city} drop E3/SUM h2[src_b]
 *                         + sum_{b: same province} drop E4/SUM h2[src_b]
 * (per head; heads*feat <= 512).  el/er/lse are the inter forward's.  bstat (B, heads, 8)
 * keeps the per-batch statistics for the backward.  Dropout of att3/att4 uses Philox
 * offsets offset+1+2h / offset+2+2h on the dense (B, N) index. */
MSHA_API int msha_ours_intra_fwd(const msha_graph* g, const msha_groups* grp, int64_t B,
                                 const int64_t* src, int32_t heads, int32_t feat, int32_t dtype,
                                 const void* h2, const float* a3s, const float* a4s,
                                 const float* el, const float* er, const float* lse,
                                 const void* u_inter, float neg_slope, float drop_p,
                                 uint64_t seed, uint64_t offset, float* bstat, void* u_out,
                                 msha_stream_t stream);
/* Backward, two stages around msha_edge_attention_bwd_rows:
 *   stage 0: G (B, 2, heads*feat) = group sums of dropout * dU; bgrad (B, heads, 4);
 *            row_coef (n_rows, heads; written in full) = dL/dSUM at the batch rows, 0
 *            elsewhere;
 *            da3s, da4s (heads, feat).
 *   stage 1: d_hs[src_b] += the intra gradient of h2's batch rows.
 * Per-row sums follow batch order (deterministic).  Stage 0 needs a workspace of
 * msha_ours_workspace_size(grp, B, heads, feat) bytes (chunked group sums). */
MSHA_API size_t msha_ours_workspace_size(const msha_groups* grp, int64_t B, int32_t heads,
                                         int32_t feat);
MSHA_API int msha_ours_intra_bwd(const msha_graph* g, const msha_groups* grp, int64_t B,
                                 const int64_t* src, int32_t heads, int32_t feat, int32_t dtype,
                                 const void* h2, const float* a3s, const float* a4s,
                                 const float* bstat, const void* dU, int32_t stage,
                                 float neg_slope, float drop_p, uint64_t seed, uint64_t offset,
                                 float* G, float* bgrad, float* row_coef, float* da3s,
                                 float* da4s, void* d_hs, void* ws, size_t ws_bytes,
                                 msha_stream_t stream);

/* Split intra mode (Ablation.py:140-205, OursLayer2) (ABI 16, added: new symbols only, no
 * existing signature or behaviour changes, so MSHA_ABI_VERSION stays 16).  City and
 * province attention are normalised each by its own softmax; the score is constant along
 * n, so the weights are 1 / |city(src_b)| and 1 / |prov(src_b)| and depend on no table:
 *   u_out[n] = u_inter[n] + sum_{b: same city} drop h2[src_b] / |city(src_b)|
 *                         + sum_{b: same province} drop h2[src_b] / |prov(src_b)|
 * Arguments as msha_ours_intra_fwd without the score vectors and the inter statistics; the
 * dropout draws are the same Philox keys.  bstat (B, heads, 8): the weights in slots 5 / 6,
 * zeros elsewhere. */
MSHA_API int msha_ours_split_fwd(const msha_graph* g, const msha_groups* grp, int64_t B,
                                 const int64_t* src, int32_t heads, int32_t feat, int32_t dtype,
                                 const void* h2, const void* u_inter, float drop_p,
                                 uint64_t seed, uint64_t offset, float* bstat, void* u_out,
                                 msha_stream_t stream);
/* Its backward, two stages around the inter backward (which takes no row_coef here: the
 * weights do not depend on the inter attention):
 *   stage 0: G (B, 2, heads*feat) = group sums of dropout * dU; da3s, da4s (heads, feat)
 *            are written as zeros (the score vectors cannot change the output).
 *   stage 1: d_hs[src_b] += G3_b / |city| + G4_b / |prov| (per row, batch order; no float
 *            atomics: bitwise repeatable).
 * Stage 0 needs msha_ours_split_workspace_size(grp, B, heads, feat) bytes. */
MSHA_API size_t msha_ours_split_workspace_size(const msha_groups* grp, int64_t B,
                                               int32_t heads, int32_t feat);
MSHA_API int msha_ours_split_bwd(const msha_graph* g, const msha_groups* grp, int64_t B,
                                 const int64_t* src, int32_t heads, int32_t feat, int32_t dtype,
                                 const float* bstat, const void* dU, int32_t stage,
                                 float drop_p, uint64_t seed, uint64_t offset, float* G,
                                 float* da3s, float* da4s, void* d_hs, void* ws,
                                 size_t ws_bytes, msha_stream_t stream);


/* ---- Model head (Ablation.py:273-277 + :298-301, Ours.py:100-109
 * + :163-167): for every row i of the source side
 *   u_out_h = lrelu(bn2_h(u[:, h]))       v_out_h = lrelu(bn1_h(v[:, h]))   (per head h)
 *   x[i]    = dropout(cat_h elu(u_out_h[i] @ v_out_h^T), p_x)               (H*M values)
 *   out[i]  = log_softmax(elu(elu(dropout(mask_i / deg_i, p_att) * (x[i] @ W))))
 * i.e. the heads' BatchNorm + LeakyReLU epilogue, u_out @ v_out.T, elu, the heads'
 * concatenation, the model's dropout, the GraphAttentionLayer out_att (its score is
 * constant along a row: attention = mask / deg, 1/M on a virtual full row), the model's
 * elu and log_softmax, in three launches (u statistics partials, statistics finalize +
 * the whole v side, one row pass).  u (N, H, F) and v (M, H, F) are the attention
 * aggregates (dtype storage, fp32 arithmetic), W the out_att weight (H*M, M) fp32,
 * out (N, M) log-probabilities (dtype).  training: batch statistics, running statistics
 * updated as nn.BatchNorm1d (momentum, unbiased variance; the num_batches_tracked
 * counters given are advanced on the device); otherwise running statistics and no dropout.  Dropout: Philox keyed on
 * (seed_x, element i*H*M + k) and (seed_att, element i*M + j), offset 0.
 * stats (4, H*F) fp32 out: u mean, u invstd, v mean, v invstd (the backward's input).
 *
 * Backward (training statistics): given dout (N, M), writes du (N, H, F), dv (M, H, F),
 * dW (H*M, M) fp32 and the per-head BatchNorm weight / bias gradients, and zeroes
 * dzero[0 .. n_zero) (nullable: the out_att score vector's gradient, which is exactly 0).  Rows whose dout
 * is all zero (train.py's nll on out[source_index] touches 64 rows) contribute only
 * through the BatchNorm batch terms and cost one row read.  Deterministic: per-wave
 * partials over ascending row ranges, added in wave order.
 * Limits: heads <= 8, heads*feat <= 512, n_cols <= 256, heads*n_cols <= 512,
 * msha_head_supported() for the LDS budget (backward row pass <= 150 KB per wave). */
#define MSHA_HEAD_MAX_HEADS 8
typedef struct msha_head_params {
  int32_t heads, feat;
  float eps, momentum, slope;                     /* BatchNorm eps / momentum, lrelu slope */
  const float* u_weight[MSHA_HEAD_MAX_HEADS];     /* bn2 of head h (u side), feat each */
  const float* u_bias[MSHA_HEAD_MAX_HEADS];
  float* u_running_mean[MSHA_HEAD_MAX_HEADS];
  float* u_running_var[MSHA_HEAD_MAX_HEADS];
  const float* v_weight[MSHA_HEAD_MAX_HEADS];     /* bn1 of head h (v side) */
  const float* v_bias[MSHA_HEAD_MAX_HEADS];
  float* v_running_mean[MSHA_HEAD_MAX_HEADS];
  float* v_running_var[MSHA_HEAD_MAX_HEADS];
  float* du_weight[MSHA_HEAD_MAX_HEADS];          /* backward outputs (nullable) */
  float* du_bias[MSHA_HEAD_MAX_HEADS];
  float* dv_weight[MSHA_HEAD_MAX_HEADS];
  float* dv_bias[MSHA_HEAD_MAX_HEADS];
  int64_t* num_batches_tracked[2 * MSHA_HEAD_MAX_HEADS]; /* nullable; +1 per training forward */
} msha_head_params;
MSHA_API int msha_head_supported(int64_t n_cols, int32_t heads, int32_t feat);
MSHA_API size_t msha_head_workspace_size(const msha_graph* g, int32_t heads, int32_t feat);
MSHA_API int msha_head_fwd(const msha_graph* g, const msha_head_params* hp, int32_t dtype,
                           const void* u, const void* v, const float* W, int32_t training,
                           float p_x, uint64_t seed_x, float p_att, uint64_t seed_att,
                           float* stats, void* out, void* ws, size_t ws_bytes,
                           msha_stream_t stream);
MSHA_API int msha_head_bwd(const msha_graph* g, const msha_head_params* hp, int32_t dtype,
                           const void* u, const void* v, const float* W, float p_x,
                           uint64_t seed_x, float p_att, uint64_t seed_att, const float* stats,
                           const void* dout, void* du, void* dv, float* dW, float* dzero,
                           int64_t n_zero, void* ws, size_t ws_bytes, msha_stream_t stream);
/* (ABI 16) msha_head_bwd with dout's row flags already computed by its producer
 * (msha_nll_rows_bwd_flags: rflag[i] = row i of dout has a nonzero, wmask[w] bit k = rflag[64w
 * + k]): the backward's own row scan is skipped.  Same outputs, bit for bit. */
MSHA_API int msha_head_bwd_flagged(const msha_graph* g, const msha_head_params* hp,
                                   int32_t dtype, const void* u, const void* v, const float* W,
                                   float p_x, uint64_t seed_x, float p_att, uint64_t seed_att,
                                   const float* stats, const void* dout, const uint8_t* rflag,
                                   const uint64_t* wmask, void* du, void* dv, float* dW,
                                   float* dzero, int64_t n_zero, void* ws, size_t ws_bytes,
                                   msha_stream_t stream);


/* ---- Training loss on gathered rows (train.py:227-229): F.nll_loss(logp[rows], cols),
 * mean reduction, and its backward, one launch each (ABI 8).  logp (N, M) row stride ld,
 * fp32 or bf16 (dtype); rows, cols int64 (B).
 *   msha_nll_rows_fwd: loss[0] = -(1/B) sum_b logp[rows[b], cols[b]]  (fp32)
 *   msha_nll_rows_bwd: dlogp = 0 except dlogp[rows[b], cols[b]] += -gloss[0] / B for b in
 *                      order (repeated pairs accumulate); gloss is a device scalar.
 * An entry outside [0, N) x [0, M) is never read or written (torch raises on it): the
 * forward returns NaN for it (and for B = 0, torch's mean over nothing), the backward
 * skips it.  (ABI 9: the forward takes N, M.) */
MSHA_API int msha_nll_rows_fwd(int64_t N, int64_t M, int64_t B, const int64_t* rows,
                               const int64_t* cols, int32_t dtype, const void* logp, int64_t ld,
                               float* loss, msha_stream_t stream);
MSHA_API int msha_nll_rows_bwd(int64_t N, int64_t M, int64_t B, const int64_t* rows,
                               const int64_t* cols, const float* gloss, int32_t dtype,
                               void* dlogp, int64_t ld, msha_stream_t stream);
/* (ABI 16) the backward that also flags dlogp's nonzero rows for the model head's backward
 * (msha_head_bwd_flagged): rflag (N bytes), wmask (ceil(N / 64) words), both or neither. */
/* (ABI 16) on = 1: the block-partial reduce of the next msha_bip_attention_fwd / _bwd on this
 * host thread is handed to the next msha_ours_intra_fwd / stage 1 of msha_ours_intra_bwd on
 * the same stream, which runs it as extra blocks of its own launch (one graph node fewer each
 * way).  on = 0: separate launches again; a reduce still pending is launched now.  The
 * outputs (v; d_hc, d_er) are complete once the taking launch (or the on = 0 call) is
 * enqueued. */
MSHA_API int msha_bip_defer_reduce(int32_t on);
MSHA_API int msha_nll_rows_bwd_flags(int64_t N, int64_t M, int64_t B, const int64_t* rows,
                                     const int64_t* cols, const float* gloss, int32_t dtype,
                                     void* dlogp, int64_t ld, uint8_t* rflag, uint64_t* wmask,
                                     msha_stream_t stream);

/* ---- Batched segment copies: the models' per-head parameter packing (Ablation.py:262-267,
 * Ours.py:58-75 read W1/W2/a/a3/a4 of every head; one launch stacks them, one scatters
 * their gradients back) and the feature dropout of Sfeatures / Rfeatures
 * (Ablation.py:296-297, Ours.py:161-162) in one launch forward and one backward.
 * For every segment:  dst[r*ldd + c] = (a[r*lda + c] (+ b[r*ldb + c])) * keep(r*cols + c)
 * for r < rows, c < cols; a NULL `a` writes zeros; keep is the dropout factor (0 or
 * 1/(1-p)) when p > 0, else 1: element e = r*cols + c keeps iff word e % 4 of the
 * Philox4x32-10 block (seed; counter {e / 4, offset}) is >= p * 2^32 (one generator call
 * per four elements; msha_dropout_keep_mask4 writes the same mask). */
#define MSHA_MAX_SEGMENTS 32
typedef struct msha_segment {
  const void* a;
  const void* b;
  void* dst;
  int64_t rows, cols, lda, ldb, ldd;
  float p;
  uint64_t seed, offset;
  /* storage types (MSHA_DTYPE_*) of a and b (shared) and of dst; arithmetic is fp32 and
   * a bf16 dst is rounded once (nearest-even), so a segment is also a dtype cast (the
   * bf16 models' parameter / gradient / running-statistics conversions, ABI 8) */
  int32_t a_dtype, dst_dtype;
} msha_segment;
MSHA_API int msha_segments(int32_t n, const msha_segment* segs, msha_stream_t stream);
MSHA_API int msha_dropout_keep_mask4(uint64_t seed, uint64_t offset, int64_t n, float p,
                                     uint8_t* keep, msha_stream_t stream);
/* keep[i] = word `word` (0..3) of the Philox4x32-10 block (seed; counter {i, offset}) >=
 * p * 2^32: the Ours intra masks (att3 / att4 of head h, batch entry b, node n: offset
 * drop_offset + 1 + h / 2, word 2 (h % 2) + kind, i = b * n_nodes + n), for tests. */
MSHA_API int msha_dropout_keep_mask_word(uint64_t seed, uint64_t offset, int64_t n, float p,
                                         int32_t word, uint8_t* keep, msha_stream_t stream);


/* ---- Optimizer step (train.py:207,232: optim.Adam(lr, weight_decay) ... step()) ------ */
/* torch.optim.Adam's update (L2 weight decay, no amsgrad / maximize) for up to
 * MSHA_MAX_ADAM tensors in ONE launch, per element (fp32 arithmetic, bias corrections in
 * double as torch computes them from its step count):
 *   g  = grad (* keep * 1/(1-p) when drop_p > 0) + weight_decay * param
 *   m  = m + (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g^2
 *   t  = *step + 1;  param -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * in one launch whose last block advances *step (capturable: the step lives on the
 * device, as torch's capturable Adam keeps it).  param, grad, exp_avg, exp_avg_sq share `dtype` (bf16 state for bf16
 * parameters, as torch keeps it), contiguous, n elements.  drop_p > 0 fuses a dropout
 * backward into the gradient read: grad is then the dropout's OUTPUT gradient and keep is
 * msha_segments' flat mask (element e: word e % 4 of the Philox4x32-10 block (drop_seed;
 * counter {e / 4, drop_offset})), so the parameter's own gradient never exists (the
 * feature dropout of Sfeatures, Ablation.py:296, Ours.py:161).  ws: device scratch of
 * msha_adam_workspace_size() bytes, ZERO-FILLED before its first use (the launch's
 * completion ticket, back at zero when the launch ends; stream-ordered reuse). */
#define MSHA_MAX_ADAM 64
typedef struct msha_adam_tensor {
  void* param;
  const void* grad;
  void* exp_avg;
  void* exp_avg_sq;
  float* step;
  int64_t n;
  int32_t dtype;
  float drop_p;
  uint64_t drop_seed, drop_offset;
} msha_adam_tensor;
MSHA_API size_t msha_adam_workspace_size(void);
MSHA_API int msha_adam_step(int32_t n, const msha_adam_tensor* tensors, double lr,
                            double beta1, double beta2, double eps, double weight_decay,
                            void* ws, msha_stream_t stream);
/* The same update at weight_decay 0 for the rows of a touched-row list only (ABI 16, added):
 * for i < n_rows[0] (a DEVICE count, at most cap) and r = rows[i], the rows param[r],
 * exp_avg[r], exp_avg_sq[r] of an (n, feat) contiguous fp32 or bf16 table are updated from
 * the gradient vals[i] ((cap, feat) fp32; for a bf16 table first rounded once to bf16, to
 * nearest even, as the dense path's cast does) with the scalars of t = *step + 1; then *step
 * = t, by a trailing one-thread launch, so every row of one call sees one t.  One step count
 * per table: a row's moments are not decayed in the steps that do not name it.  Rows outside
 * the list are neither read nor written; a step that names every row leaves the bits of
 * msha_adam_step.  rows must be distinct (msha_plan_rows); an entry outside [0, n) is skipped.
 * feat as msha_link_bce_supported; 1 <= cap <= n; no float atomics. */
MSHA_API int msha_adam_rows_step(int64_t n, int32_t feat, int32_t dtype, void* param,
                                 void* exp_avg, void* exp_avg_sq, float* step,
                                 const int32_t* rows, const int32_t* n_rows, int64_t cap,
                                 const float* vals, double lr, double beta1, double beta2,
                                 double eps, msha_stream_t stream); /* (ABI 16, added) */
/* The dense update (weight decay included) at the cost of the listed rows, by replaying the
 * steps a row missed (ABI 16, added).  T = (int)*step is the count of completed steps;
 * row_step[r] (int32, n entries, 0 for fresh state) is the step after which row r's param,
 * exp_avg, exp_avg_sq in memory are valid.  For each listed row r (rows[i], i < n_rows[0] <=
 * cap; rows == NULL: every row, cap == n, n_rows unused) and t = row_step[r] + 1 ...
 * min(T, row_step[r] + max_steps) the row takes msha_adam_step's update with gradient +0.0
 * (plus weight_decay * param) and step t's own bias corrections -- the bits the dense step
 * left at step t; a bf16 row is rounded through bf16 after every replayed step.  With vals
 * != NULL ((cap, feat) fp32, entry i the gradient of rows[i], or of row i with rows == NULL)
 * a row that has reached T then takes step T + 1 with its gradient (rounded once to bf16 for
 * a bf16 table), and a trailing one-thread launch sets *step = T + 1; give max_steps =
 * INT32_MAX there, or a row further behind than max_steps loses its gradient.  vals == NULL:
 * catch up only, *step is left alone.  Each row is read and written once per launch and
 * row_step[r] is set to the step reached; rows that have nothing to do are not read.  After
 * every row has been caught up (rows == NULL, ceil(T / max_steps) launches) the table and
 * its moments hold the bits of T msha_adam_step calls on the dense gradients.  One set of
 * hyperparameters serves all replayed steps: catch every row up before changing them.
 * rows must be distinct (msha_plan_rows, msha_row_grad_union); an entry outside [0, n) is
 * skipped.  feat as msha_link_bce_supported; 1 <= cap <= n; max_steps >= 1; no atomics. */
MSHA_API int msha_adam_rows_replay(int64_t n, int32_t feat, int32_t dtype, void* param,
                                   void* exp_avg, void* exp_avg_sq, float* step,
                                   int32_t* row_step, const int32_t* rows,
                                   const int32_t* n_rows, int64_t cap, const float* vals,
                                   int32_t max_steps, double lr, double beta1, double beta2,
                                   double eps, double weight_decay,
                                   msha_stream_t stream); /* (ABI 16, added) */

/* ---- Projection of a small node table in one workgroup (the recipient side: R15 has 32
 * recipients; Ablation.py:262, :266-267): h = X @ W (M x N, N = heads*feat) with optional
 * per-head score halves el = h . al, er = h . ar; backward with D = dh + d_el (x) al +
 * d_er (x) ar: dX = D @ W^T, dW = X^T @ D, dal / dar[h, f] = sum_m d_el / d_er[m, h]
 * h[m, h*feat + f] -- one launch each (any output pointer may be NULL).  fp32, M <= 256,
 * K <= 128, heads*feat <= 128 (msha_project_small_supported). */
MSHA_API int msha_project_small_supported(int64_t M, int64_t K, int32_t heads, int32_t feat);
MSHA_API int msha_project_small(int64_t M, int64_t K, int32_t heads, int32_t feat,
                                const float* X, const float* W, const float* al,
                                const float* ar, float* h, float* el, float* er,
                                msha_stream_t stream);
MSHA_API int msha_project_small_bwd(int64_t M, int64_t K, int32_t heads, int32_t feat,
                                    const float* X, const float* W, const float* al,
                                    const float* ar, const float* h, const float* dh,
                                    const float* d_el, const float* d_er, float* dX, float* dW,
                                    float* dal, float* dar, msha_stream_t stream);

/* ---- Device-side evaluation (train.py:239-282, model.py:66-92) (ABI 16, added) -------- */
/* One launch per test batch (ABI 16, added).  For b in [0, B), i = src[b] (src NULL: b)
 * and y = labels[b], at position r = row_offset + b of the caller's per-row buffers:
 *   store[r, :] = table[i, :] widened exactly to fp32   (store: (capacity, C), pitch C)
 *   labels_out[r] = y;  nll[r] = -table[i, y];  pred[r] = lowest index of the row maximum
 *   conf[y * C + pred[r]] += 1                           (int64 C x C, integer atomic)
 *   counters[0] += non-finite values in the row;  counters[1] += 1 for a bad row
 * table: (N, C) of dtype (MSHA_DTYPE_*), row pitch ld elements, 1 <= C <= 1024.  A src in
 * [-N, 0) wraps as torch's output[source_index]; any other src outside [0, N) or a label
 * outside [0, C) makes the row bad: nothing is read through either index, the row stores
 * zeros, nll 0, pred -1, labels_out -1 and touches counters[1] only.  conf and counters
 * are the caller's, zeroed before the first batch. */
MSHA_API int msha_eval_rows(int64_t N, int32_t C, int64_t B, int32_t dtype, const void* table,
                            int64_t ld, const int64_t* src, const int64_t* labels,
                            int64_t row_offset, float* store, int64_t* labels_out, float* nll,
                            int64_t* pred, int64_t* conf, int64_t* counters,
                            msha_stream_t stream);
/* (ABI 16, added) loss[0] = mean over the chunks [c * chunk, min(n, (c+1) * chunk)) of the
 * chunk's mean of nll (fp32) -- chunk = n: the mean over all rows; chunk = the batch size:
 * what train.py:253-254,274 prints.  Every sum runs in a fixed order; no float atomics. */
MSHA_API int msha_eval_loss(int64_t n, int64_t chunk, const float* nll, float* loss,
                            msha_stream_t stream);
/* Tie-aware rank statistic of each of C columns of an (n, >= C) fp32 score store, row
 * pitch ld (ABI 16, added).  Row b is positive in column k iff labels[b] == cls[k] (cls
 * NULL: cls[k] = k); binary != 0 (C = 1, cls NULL): iff labels[b] != 0.  Scores compare as
 * the order-preserving uint32 image of their bits with -0.0 folded onto +0.0 (denormals
 * stay distinct).  out[4 k + {0, 1, 2, 3}] = P, Nn, U2 = sum over groups of equal score of
 * pos_g (2 neg_below_g + neg_g), and the column's count of non-finite scores;
 * AUC_k = U2 / (2 P Nn) in the caller's fp64.  All device arithmetic is integer: the
 * result does not depend on execution order.  Columns of at most
 * msha_rank_auc_block_keys() rows are sorted in LDS by one block each and need no
 * workspace; longer ones take a stable 8-bit LSD radix sort through ws
 * (msha_rank_auc_workspace_size bytes, 16-byte aligned, contents irrelevant).
 * 1 <= n < 2^31, 1 <= C <= 65535. */
MSHA_API size_t msha_rank_auc_workspace_size(int64_t n, int32_t C);
MSHA_API int msha_rank_auc(int64_t n, int32_t C, const float* scores, int64_t ld,
                           const int64_t* labels, const int32_t* cls, int32_t binary,
                           int64_t* out, void* ws, size_t ws_bytes, msha_stream_t stream);
/* host-only: the largest n the one-block LDS path takes (ABI 16, added) */
MSHA_API int64_t msha_rank_auc_block_keys(void);

/* ---- Top-K link retrieval for the inner-product scorer (LLP.py:20 Hits@K,
 * Explainer.py:31-34) (ABI 16, added) ---------------------------------------------------
 * For query position b in [0, n_q): the k candidates j in [0, n_cand) with the highest
 * logit sum_f Q[q, f] * T[j, f], q = qi[b] (qi NULL: b), accumulated in fp32 on the matrix
 * cores (fp32 tables: the exact-f32 MFMA, an fma chain; bf16 tables: the bf16 MFMA), in an
 * order fixed by f alone: a candidate's logit does not depend on the tile, block or split
 * that computed it.  The (n_q, n_cand) score matrix is never written.
 *
 * Order: logit descending, then candidate index ascending -- a total order, so the result
 * is unique.  Logits compare through the order-preserving uint32 image of msha_rank_auc
 * (-0.0 folded onto +0.0); +inf ranks first, every NaN below -inf, NaNs among themselves
 * by index.
 *
 * out_val / out_idx: (n_q, k) fp32 / int64, each row best first.  out_idx = j + col_offset
 * (a shard reports global rows); out_val = the logit, or 1 / (1 + exp(-logit)) with
 * sigmoid != 0 -- the ranking is by the logit either way.  Slots past the number of
 * available candidates hold -inf (0.0 under sigmoid) and index -1.
 *
 * A qi[b] outside [0, rows_q) makes row b all filler and sets *err (nullable) to 1;
 * nothing is read through it.  excl_rowptr (int32, n_q + 1) / excl_col (int32, ascending
 * within a row, candidate-local numbering), both or neither: candidates never returned
 * for query POSITION b.
 *
 * splits: column splits of the candidate range (0: msha_topk_inner_splits); each split
 * writes a partial list into ws and a merge launch combines them; the result does not
 * depend on it.  ws: msha_topk_inner_workspace_size bytes, 16-byte aligned, contents
 * irrelevant.  Q, T: 16-byte aligned, row pitches ldq / ldt elements, multiples of 16
 * bytes; Q may be T.  feat a multiple of 16 in [16, 256], 1 <= k <= 128, n_cand < 2^31 - 1
 * (msha_topk_inner_supported); n_q = 0 launches nothing, n_cand = 0 only the filler.
 * Stateless; integer compares and ordinary stores only, no float atomics. */
/* host-only (ABI 16, added) */
MSHA_API int msha_topk_inner_supported(int32_t feat, int32_t k, int32_t dtype);
/* bytes of ws for msha_topk_inner; splits 0: for the default split count (ABI 16, added) */
MSHA_API size_t msha_topk_inner_workspace_size(int64_t n_q, int64_t n_cand, int32_t k,
                                               int32_t splits);
/* host-only: the default split count -- one block per CU from query tiles x splits, at
 * least 512 candidates per split; 1 when the query tiles alone fill the device
 * (ABI 16, added) */
MSHA_API int msha_topk_inner_splits(int64_t n_q, int64_t n_cand, int32_t feat, int32_t k,
                                    int32_t dtype);
/* the retrieval itself, as described above (ABI 16, added) */
MSHA_API int msha_topk_inner(int64_t n_q, int32_t feat, int32_t dtype, const void* Q,
                             int64_t ldq, const int64_t* qi, int64_t rows_q, const void* T,
                             int64_t ldt, int64_t n_cand, int64_t col_offset,
                             const int32_t* excl_rowptr, const int32_t* excl_col, int32_t k,
                             int32_t sigmoid, int32_t splits, float* out_val, int64_t* out_idx,
                             int32_t* err, void* ws, size_t ws_bytes, msha_stream_t stream);
/* Top k of `rows` rows of lists * len candidates under the same order and filler rule
 * (ABI 16, added): vals (rows, lists * len) fp32, idx the candidates' int64 indices in
 * [0, 2^32 - 1) -- an entry with idx < 0 is ignored -- or NULL: the position in the row.
 * The lists need not be sorted.  sigmoid != 0: out_val = 1 / (1 + exp(-value)) of the
 * selected values (lists of logits; the order is by the value given).  The second stage
 * of msha_topk_inner's column splits, the cross-rank merge of sharded lists, and on a
 * plain score vector (rows = 1, lists = 1) the selection behind hits@k.  A row longer than
 * 4096 is cut into chunks, each selected by
 * one wave, and the selections merged again through ws
 * (msha_topk_merge_workspace_size bytes, 16-byte aligned, contents irrelevant).
 * 1 <= k <= 128, lists * len < 2^32 - 1. */
MSHA_API size_t msha_topk_merge_workspace_size(int64_t rows, int64_t lists, int64_t len,
                                               int32_t k); /* (ABI 16, added) */
MSHA_API int msha_topk_merge(int64_t rows, int64_t lists, int64_t len, int32_t k,
                             const float* vals, const int64_t* idx, int32_t sigmoid,
                             float* out_val, int64_t* out_idx, void* ws, size_t ws_bytes,
                             msha_stream_t stream);

/* ---- Select over ragged segments: the attention explanation (Explainer.py:25-34)
 * (ABI 16, added) -----------------------------------------------------------------------
 * Segment s in [0, n_seg) is the slots t in [ptr[s], ptr[s + 1]) (ptr: int32, n_seg + 1,
 * ascending, ptr[n_seg] <= n_slots; a CSR rowptr or a CSC colptr).  A slot's value is
 * x_t = vals[(eid ? eid[t] : t) * ld + off] (fp32; vals has n_vals rows of pitch ld, so
 * ld / off pick one head of an (E, H) attention export and eid = csc_eid reads it in column
 * order; an eid outside [0, n_vals) reads as NaN), its id is ids ? ids[t] : t - ptr[s]
 * (int32, >= 0: col on the row side, csc_row on the column side).
 *
 * Order: msha_topk_inner's -- value descending, then id ascending; -0.0 folded onto +0.0,
 * +inf first, every NaN below -inf and all NaNs equal.  Integer compares and adds, ordinary
 * stores, no atomics: the results are unique, bitwise repeatable and independent of the
 * grid and of `chunk`.
 *
 * msha_segment_ties (Explainer.py:25-30, "argwhere(row == max(row))"):
 *   max_val (fp32, n_seg)    the segment's maximum (-inf for an empty segment, +0.0 for a
 *                            zero of either sign, a NaN when every slot is NaN)
 *   n_tie   (int32, n_seg)   the slots with x_t >= thr, thr = max - rtol * |max| formed once
 *                            per segment in fp32 (product and difference each rounded); with
 *                            rtol = 0 or a non-finite maximum: the slots whose image equals
 *                            the maximum's
 *   tie_ptr (int32, n_seg + 1)  the exclusive scan of n_tie, made on the device
 *   tie_idx (int32, n_slots) those slots' ids at tie_ptr[s] .. tie_ptr[s + 1], in slot
 *                            order; the rest of the buffer is left as it was.  Sized at the
 *                            number of slots, so no count is read back.
 *   0 <= rtol < 1.
 * msha_segment_topk (Explainer.py:31-34): out_val / out_idx (n_seg, k) fp32 / int64, each
 *   segment's k best, best first; slots past the segment's length hold -inf and -1, as in
 *   msha_topk_inner.  1 <= k <= 128: the k of 200 in the reference's commented-out variant
 *   is out of range and returns MSHA_ERR_ARG.
 *
 * Two regimes, chosen per segment on the device: a segment of at most W slots (W the power
 * of two in [4, 64] at or above twice the mean length n_slots / n_seg) is handled by a
 * group of W lanes; a longer one is cut into chunks of at most `chunk` slots (in
 * [64, 4096]; 0: 256 in tie mode, for top-K the power of two in [256, 4096] at or above
 * sqrt(n_slots / n_seg * k)), one wave per (segment, chunk), found through a scan of the
 * segments' chunk counts, and the chunks' partial results are combined in chunk order.
 *
 * Stateless; every buffer is the caller's.  ws: msha_segment_select_workspace_size bytes
 * (k = 0: tie mode), 16-byte aligned, contents irrelevant.  n_seg, n_slots < 2^31 - 1;
 * n_seg = 0 launches nothing. */
MSHA_API size_t msha_segment_select_workspace_size(int64_t n_seg, int64_t n_slots, int32_t k,
                                                   int32_t chunk); /* (ABI 16, added) */
MSHA_API int msha_segment_ties(int64_t n_seg, int64_t n_slots, const int32_t* ptr,
                               const float* vals, int64_t n_vals, int64_t ld, int64_t off,
                               const int32_t* eid, const int32_t* ids, float rtol,
                               int32_t chunk, float* max_val, int32_t* n_tie, int32_t* tie_ptr,
                               int32_t* tie_idx, void* ws, size_t ws_bytes,
                               msha_stream_t stream); /* (ABI 16, added) */
MSHA_API int msha_segment_topk(int64_t n_seg, int64_t n_slots, const int32_t* ptr,
                               const float* vals, int64_t n_vals, int64_t ld, int64_t off,
                               const int32_t* eid, const int32_t* ids, int32_t k, int32_t chunk,
                               float* out_val, int64_t* out_idx, void* ws, size_t ws_bytes,
                               msha_stream_t stream); /* (ABI 16, added) */

/* ---- Filtered link ranks, MRR and Hits@K for the inner-product scorer (LLP.py:20, the
 * ranking protocol around it) (ABI 16, added) ------------------------------------------
 * For query position b in [0, n_q) with target candidate t = target[b] (a GLOBAL row; it
 * is local when col_offset <= t < col_offset + n_cand):
 *   greater[b] = #{ j in [0, n_cand), j != t, j not excluded for b : z_bj >  z_bt }
 *   equal[b]   = the same set with ==
 * z_bj = sum_f Q[q, f] * T[j, f], q = qi[b] (qi NULL: b): msha_topk_inner's logits, bit for
 * bit (the same MFMA chain ordered by f alone), compared under its order: -0.0 folded onto
 * +0.0, +inf highest, every NaN below -inf and all NaNs equal among themselves.  The target's
 * own logit comes from the same chain (its row is staged as one more candidate), so a
 * candidate row bytewise equal to the target row ties with it exactly; out_logit[b]
 * (nullable) is that logit, the value msha_topk_inner(sigmoid = 0) reports for the pair.
 * The (n_q, n_cand) score matrix is never written; one pass serves every K:
 * rank = 1 + greater + {0, equal / 2, equal}.
 *
 * target_logit_in (nullable, fp32 n_q): the logit to rank against instead (the sharded
 * case: the target's owner computed it); then a target that is not local is allowed and
 * every non-excluded candidate is counted; a local target is still left out of the counts.
 * Without it a target that is not local gives greater = equal = -1 for the row and sets
 * bit 2 of *err (nullable).  A qi[b] outside [0, rows_q) gives -1 / -1 and sets bit 1;
 * nothing is read through it.  out_logit of such rows is NaN.
 *
 * excl_rowptr / excl_col, splits, Q / T alignment and pitches: as msha_topk_inner.  Each
 * column split writes partial counts into ws and a finishing launch sums them: integer adds
 * only, so the result does not depend on splits, bit for bit.  ws:
 * msha_rank_inner_workspace_size bytes, 16-byte aligned, contents irrelevant.  feat a
 * multiple of 16 in [16, 256], n_cand < 2^31 - 1; n_q = 0 launches nothing; n_cand = 0 with
 * target_logit_in returns zeros.  Stateless; ordinary stores, no float atomics. */
/* host-only (ABI 16, added) */
MSHA_API int msha_rank_inner_supported(int32_t feat, int32_t dtype);
/* host-only: the default split count -- one (fp32) or two (bf16) blocks per CU from query
 * tiles (128 rows) x splits, at least 512 candidates per split (ABI 16, added) */
MSHA_API int msha_rank_inner_splits(int64_t n_q, int64_t n_cand, int32_t feat, int32_t dtype);
/* bytes of ws for msha_rank_inner; splits 0: enough for either dtype's default split count
 * (ABI 16, added) */
MSHA_API size_t msha_rank_inner_workspace_size(int64_t n_q, int64_t n_cand, int32_t splits);
/* the ranking itself, as described above (ABI 16, added) */
MSHA_API int msha_rank_inner(int64_t n_q, int32_t feat, int32_t dtype, const void* Q,
                             int64_t ldq, const int64_t* qi, int64_t rows_q, const void* T,
                             int64_t ldt, int64_t n_cand, int64_t col_offset,
                             const int64_t* target, const float* target_logit_in,
                             const int32_t* excl_rowptr, const int32_t* excl_col,
                             int32_t splits, int64_t* out_greater, int64_t* out_equal,
                             float* out_logit, int32_t* err, void* ws, size_t ws_bytes,
                             msha_stream_t stream);
/* Sums over n ranked rows (ABI 16, added).  rank = 1 + greater + {0, equal / 2, equal} for
 * ties = 0 (optimistic), 1 (mean), 2 (pessimistic), carried as the integer 2 rank; rows with
 * greater < 0 are left out.  ks: nk <= 8 values of k >= 1 in HOST memory, read during the
 * call.  out_counts (device, int64, nk + 2): the rows with 2 rank <= 2 ks[i], the valid
 * rows, the sum of 2 rank.  out_rr (device, fp64): the sum of 1 / rank, in a fixed order
 * (lanes stride a block's rows, xor tree, waves in order, blocks in order): two calls give
 * the same bits.  ws: msha_rank_summary_workspace_size bytes, 16-byte aligned. */
MSHA_API size_t msha_rank_summary_workspace_size(int64_t n); /* (ABI 16, added) */
MSHA_API int msha_rank_summary(int64_t n, const int64_t* greater, const int64_t* equal,
                               int32_t ties, const int64_t* ks, int32_t nk, int64_t* out_counts,
                               double* out_rr, void* ws, size_t ws_bytes, msha_stream_t stream);

/* ---- Link-prediction training for the inner-product scorer (LLP.py:112-115 under a
 * binary cross-entropy on the logit) (ABI 16, added) ------------------------------------
 * sample -> score -> loss -> table gradient.  No entry point reads anything back to the
 * host or allocates, so the whole chain can be captured into one HIP graph; no (P, F)
 * array exists anywhere in it and no float atomic is used: every sum has a fixed order.
 *
 * Negative sampler.  For positive p in [0, n_pos) and j < k: src_rep[p k + j] = src[p] and
 * dst_neg[p k + j] = d + col_offset, d drawn uniformly from the candidates [0, n_cand) that
 * are not neighbours of src[p] in the CSR (rowptr int32 (n_rows + 1), col int32 (n_edges),
 * ascending within a row; a row with rowflag (nullable, one byte a row) set is a virtual
 * full row and counts as having no edges).  There is no rejection loop: with cnt = n_cand -
 * deg and r = (philox(seed, offset, p k + j) * cnt) >> 32, d is the r-th non-edge column,
 * r + t for the smallest t in [0, deg] with col[t] - t > r (binary search, at most 32
 * steps).  dst_neg is -1 when cnt <= 0 and when src[p] is outside [0, n_rows), which is
 * decided before any load through it.  The draw's offset follows the dropout draws: the
 * installed replay counter (msha_set_rng_counter) is added in its high word, so a captured
 * graph draws fresh negatives on every replay. */
MSHA_API int msha_negative_sample(int64_t n_pos, int32_t k, const int64_t* src, int64_t n_rows,
                                  int64_t n_cand, int64_t n_edges, const int32_t* rowptr,
                                  const int32_t* col, const uint8_t* rowflag, int64_t col_offset,
                                  uint64_t seed, uint64_t offset, int64_t* src_rep,
                                  int64_t* dst_neg, msha_stream_t stream);
/* Incidence plan of a pair list over a table of n rows (ABI 16, added).  The 2 n_pairs
 * endpoints are numbered e < n_pairs: the src end of pair e (row src[e], other end dst[e]);
 * e >= n_pairs: the dst end of pair e - n_pairs.  rowptr int32 (n + 1), ent int32
 * (2 n_pairs): row r's endpoint ids, ascending (a stable sort by row), at
 * ent[rowptr[r], rowptr[r + 1]).  A pair with either index outside [0, n) is padding: it is
 * in no row, and ent past rowptr[n] holds -1.  A self pair is twice in its row.  A pure
 * function of (src, dst, n): integer work, ranked placement.  chunk_tab: int32,
 * 2 * msha_pair_plan_chunk_slots(n_pairs) words, the backward's chunk table: rows of more
 * than msha_pair_plan_chunk() endpoints are cut into chunks of that size; a static bound, no
 * count is read back.  2 n_pairs < 2^31, n < 2^31 - 1.  ws: msha_pair_plan_workspace_size
 * bytes, 16-byte aligned, contents irrelevant.  n_pairs = 0 gives the empty plan. */
MSHA_API int32_t msha_pair_plan_chunk(void);                  /* host-only (ABI 16, added) */
MSHA_API int64_t msha_pair_plan_chunk_slots(int64_t n_pairs); /* host-only (ABI 16, added) */
MSHA_API size_t msha_pair_plan_workspace_size(int64_t n_pairs); /* (ABI 16, added) */
MSHA_API int msha_pair_plan(int64_t n_pairs, int64_t n, const int64_t* src, const int64_t* dst,
                            int32_t* rowptr, int32_t* ent, int32_t* chunk_tab, void* ws,
                            size_t ws_bytes, msha_stream_t stream);
/* Fused loss (ABI 16, added).  z[p] = sum_f h[src[p], f] h[dst[p], f] in fp32 (h: (n, feat)
 * fp32 or bf16, row pitch ld elements, 16-byte aligned rows; feat as msha_pair_inner_fwd_ex:
 * a power of two, 16 bytes to 64 lanes x 16 bytes of a row -- msha_link_bce_supported),
 * l = max(z, 0) - z y + log1p(exp(-|z|)) with target y in [0, 1] (soft targets allowed),
 * loss[0] = sum_p w_p l_p with weight w (nullable: 1 / n_pairs).  A pair with an index
 * outside [0, n) is padding: z = NaN, nothing added, counted in n_pad[0].  The sum is
 * ordered: blocks of 1024 pairs, each in a fixed order, then the partials in order.
 * ws: msha_link_bce_fwd_workspace_size bytes, 16-byte aligned.  1 <= n_pairs < 2^30. */
MSHA_API int msha_link_bce_supported(int32_t feat, int32_t dtype); /* host-only (ABI 16, added) */
MSHA_API size_t msha_link_bce_fwd_workspace_size(int64_t n_pairs);  /* (ABI 16, added) */
MSHA_API int msha_link_bce_fwd(int64_t n_pairs, int32_t feat, int32_t dtype, const void* h,
                               int64_t ld, int64_t n, const int64_t* src, const int64_t* dst,
                               const float* target, const float* weight, float* z, float* loss,
                               int32_t* n_pad, void* ws, size_t ws_bytes, msha_stream_t stream);
/* Its table gradient (ABI 16, added): dH (n, feat) fp32, contiguous, for either table type,
 * dH[r] = sum over row r's endpoints e in plan order of g_p h[other(e)], g_p = gloss[0] w_p
 * (sigmoid(z_p) - y_p) with z the forward's output and gloss a DEVICE scalar.  Every row is
 * written (zeros without endpoints): no memset is needed.  A row of at most one chunk is
 * summed by one wave in plan order, a longer one through chunk partials added in chunk
 * order: the result depends on the plan alone, never on the grid.  The plan must be the one
 * of (src, dst, n).  ws: msha_link_bce_bwd_workspace_size bytes, 16-byte aligned. */
MSHA_API size_t msha_link_bce_bwd_workspace_size(int64_t n_pairs, int32_t feat); /* (ABI 16, added) */
MSHA_API int msha_link_bce_bwd(int64_t n_pairs, int32_t feat, int32_t dtype, const void* h,
                               int64_t ld, int64_t n, const int64_t* src, const int64_t* dst,
                               const float* target, const float* weight, const float* z,
                               const float* gloss, const int32_t* plan_rowptr,
                               const int32_t* plan_ent, const int32_t* plan_chunk_tab, float* dH,
                               void* ws, size_t ws_bytes, msha_stream_t stream);
/* Touched-row list of a plan (ABI 16, added): rows int32, capacity cap = min(n, 2 n_pairs),
 * the ascending ids of the table rows r with rowptr[r + 1] > rowptr[r]; entries past the count
 * are -1; n_rows[0] the count, a DEVICE int32.  Flag, exclusive scan, compact: integer work,
 * no atomics, nothing read back, a pure function of the plan.  Padding pairs are in no row
 * and touch none.  A row whose rowptr pair is not a plan's (negative, decreasing, past
 * 2 n_pairs) is empty, as the gradient reads it; the list never passes cap.  rows may be
 * NULL when cap is 0.  ws: msha_plan_rows_workspace_size(n) bytes, 16-byte aligned. */
MSHA_API size_t msha_plan_rows_workspace_size(int64_t n); /* (ABI 16, added) */
MSHA_API int msha_plan_rows(int64_t n, int64_t n_pairs, const int32_t* plan_rowptr, int32_t* rows,
                            int32_t* n_rows, void* ws, size_t ws_bytes,
                            msha_stream_t stream); /* (ABI 16, added) */
/* msha_link_bce_bwd for the rows of the list only (ABI 16, added): vals (cap, feat) fp32,
 * vals[i] bit for bit what msha_link_bce_bwd writes to dH[rows[i]] (the same per-row sum, the
 * same chunk partials and chunk-order finish) for i < n_rows[0], zeros from there to cap.
 * The loops run to the list's DEVICE count and capacity, never to n: the cost is the touched
 * rows'.  cap must be min(n, 2 n_pairs); rows, n_rows from msha_plan_rows of the same plan.
 * ws: msha_link_bce_bwd_workspace_size bytes. */
MSHA_API int msha_link_bce_bwd_rows(int64_t n_pairs, int32_t feat, int32_t dtype, const void* h,
                                    int64_t ld, int64_t n, const int64_t* src, const int64_t* dst,
                                    const float* target, const float* weight, const float* z,
                                    const float* gloss, const int32_t* plan_rowptr,
                                    const int32_t* plan_ent, const int32_t* plan_chunk_tab,
                                    const int32_t* rows, const int32_t* n_rows, int64_t cap,
                                    float* vals, void* ws, size_t ws_bytes,
                                    msha_stream_t stream); /* (ABI 16, added) */
/* The sum of k row gradients of one (n, feat) table (ABI 16, added), 1 <= k <= 4.  List j: rows
 * int32 (cap_j, 1 <= cap_j <= n) ascending and distinct with -1 past its DEVICE count n_rows[0],
 * vals (cap_j, feat) fp32, 16-byte aligned.  Output: rows (cap = min(n, sum of cap_j)) the
 * ascending union, -1 past the count; n_rows[0] the count, a DEVICE int32; vals (cap, feat)
 * fp32, 16-byte aligned, vals[i] = x_1 + x_2 + .. + x_k added left to right in fp32, x_j the
 * row's value in list j or +0.0 where list j does not hold it (what accumulating k dense fp32
 * gradients gives, signed zeros included); zeros past the count.  The lists' rows are marked
 * in n ints, which go through msha_plan_rows' scan and compaction; each output row then finds
 * itself in each sorted list.  Integer compares, no atomics, nothing read back.  feat a
 * multiple of 4.  ws: msha_row_grad_union_workspace_size(n) bytes, 16-byte aligned. */
typedef struct msha_row_list {
  const int32_t* rows;
  const int32_t* n_rows;
  int64_t cap;
  const float* vals;
} msha_row_list;
MSHA_API size_t msha_row_grad_union_workspace_size(int64_t n); /* (ABI 16, added) */
MSHA_API int msha_row_grad_union(int64_t n, int32_t feat, int32_t k, const msha_row_list* lists,
                                 int32_t* rows, int32_t* n_rows, int64_t cap, float* vals,
                                 void* ws, size_t ws_bytes,
                                 msha_stream_t stream); /* (ABI 16, added) */

/* ---- Link-prediction distillation for the inner-product scorer (LLP.py:231-238: a
 * teacher-matching term added to the label loss) (ABI 16, added) ------------------------
 * context sample -> plan -> fused rank / KL / probability loss -> table gradient.  As the
 * training chain above: nothing is read back or allocated, no float atomic, every sum has a
 * fixed order, so the whole chain can be captured into one HIP graph.
 *
 * Context sampler.  context int64 (n_anchors, K), K = walks * hops + n_rand, 1 <= K <= 64.
 * Walk w < walks starts at v_0 = anchors[a]; at step s < hops, deg is the CSR degree of v_s,
 * 0 when v_s is outside [0, n_rows), the row is empty or its rowflag (nullable) is set (a
 * virtual full row has no edges); deg = 0 puts -1 in this and every later slot of the walk,
 * else v_{s+1} = col[rowptr[v_s] + ((word * deg) >> 32)] goes to slot w * hops + s.  Slot
 * walks * hops + j is (word * n_nodes) >> 32, -1 when the anchor is outside [0, n_rows).
 * word = philox(seed, offset, a * K + slot), the offset as msha_negative_sample's (replay
 * counter in its high word).  No rejection loop; every index is range-checked before a load
 * goes through it.  n_nodes in [1, 2^31) when n_rand > 0. */
MSHA_API int msha_context_sample(int64_t n_anchors, int32_t walks, int32_t hops, int32_t n_rand,
                                 const int64_t* anchors, int64_t n_rows, int64_t n_nodes,
                                 int64_t n_edges, const int32_t* rowptr, const int32_t* col,
                                 const uint8_t* rowflag, uint64_t seed, uint64_t offset,
                                 int64_t* context, msha_stream_t stream); /* (ABI 16, added) */
/* Fused distillation loss (ABI 16, added).  Per anchor a and slot k < K (2 <= K <= 64):
 * y_k = <h[anchors[a]], h[context[a, k]]> by msha_link_bce_fwd's own chain (bitwise its z on
 * the flat pairs); t_k = teacher_logits[a, k], or the same dot on the teacher table (exactly
 * one of teacher_logits / teacher is non-NULL; the teacher table has its own feat, dtype,
 * pitch and row count, under the same width rule).  A slot whose anchor or context index is
 * outside [0, n) (and [0, n_t) with a teacher table) is padding: logit NaN, g 0, in no term,
 * counted in n_pad[0].  Over an anchor's valid slots:
 *   L_R = sum_{i<j} max(0, margin - r (y_i - y_j)), r = sign(d) if |d| > margin else 0,
 *         d = t_i - t_j (one fp32 subtraction and one compare for each decision);
 *   L_D = sum_k p_k (log p_k - log q_k), p = softmax(t / tau), q = softmax(y / tau);
 *   L_P = sum_k (sigmoid(y_k) - sigmoid(t_k))^2.
 * terms[0..2] = (L_R, L_D, L_P) / n_anchors summed over the anchors, loss[0] = w_rank
 * terms[0] + w_dist terms[1] + w_prob terms[2]; logits (n_anchors, K) fp32 = y; g
 * (n_anchors, K) fp32 = d loss / d y, its rank part an integer count times w_rank.  L_D, L_P
 * and their part of g are evaluated in fp64 from the fp32 logits and rounded once.  The
 * sums are ordered: tiles of 64 anchors, each in a fixed order, then the partials in order.
 * ws: msha_link_distill_fwd_workspace_size bytes, 16-byte aligned.  n_anchors * K < 2^30. */
MSHA_API size_t msha_link_distill_fwd_workspace_size(int64_t n_anchors); /* (ABI 16, added) */
MSHA_API int msha_link_distill_fwd(int64_t n_anchors, int32_t k, int32_t feat, int32_t dtype,
                                   const void* h, int64_t ld, int64_t n, const int64_t* anchors,
                                   const int64_t* context, const float* teacher_logits,
                                   const void* teacher, int32_t t_feat, int32_t t_dtype,
                                   int64_t t_ld, int64_t n_t, float margin, float tau,
                                   float w_rank, float w_dist, float w_prob, float* logits,
                                   float* g, float* loss, float* terms, int32_t* n_pad, void* ws,
                                   size_t ws_bytes, msha_stream_t stream); /* (ABI 16, added) */
/* Table gradient from a per-pair factor (ABI 16, added): dH[r] = gloss[0] * sum over row r's
 * endpoints e in plan order of g[p] h[other(e)], with the pairs (src[p], dst[p]), their plan
 * and the chunk partials exactly as msha_link_bce_bwd (g loaded instead of recomputed).  dH
 * (n, feat) fp32, every row written.  ws: msha_pair_grad_bwd_workspace_size bytes. */
MSHA_API size_t msha_pair_grad_bwd_workspace_size(int64_t n_pairs, int32_t feat); /* (ABI 16, added) */
MSHA_API int msha_pair_grad_bwd(int64_t n_pairs, int32_t feat, int32_t dtype, const void* h,
                                int64_t ld, int64_t n, const int64_t* src, const int64_t* dst,
                                const float* g, const float* gloss, const int32_t* plan_rowptr,
                                const int32_t* plan_ent, const int32_t* plan_chunk_tab, float* dH,
                                void* ws, size_t ws_bytes, msha_stream_t stream); /* (ABI 16, added) */
/* msha_pair_grad_bwd for the rows of a touched-row list only (ABI 16, added): vals, rows,
 * n_rows and cap exactly as msha_link_bce_bwd_rows. */
MSHA_API int msha_pair_grad_bwd_rows(int64_t n_pairs, int32_t feat, int32_t dtype, const void* h,
                                     int64_t ld, int64_t n, const int64_t* src,
                                     const int64_t* dst, const float* g, const float* gloss,
                                     const int32_t* plan_rowptr, const int32_t* plan_ent,
                                     const int32_t* plan_chunk_tab, const int32_t* rows,
                                     const int32_t* n_rows, int64_t cap, float* vals, void* ws,
                                     size_t ws_bytes, msha_stream_t stream); /* (ABI 16, added) */

/* ---- Representation matching (LLP.py:34-35, :237: KD_cosine(h[rows], t_h[rows]) added to
 * the student's loss) (ABI 16, added) ---------------------------------------------------
 * loss[0] = 1 - mean over the valid entries p of cos(h[rows[p]], T[rows[p]]), the teacher T
 * never differentiated.  Student and teacher are indexed by the same id, so with c_r the
 * occurrences of r among the valid entries and P_v their number:
 *   loss  = 1 - (1 / P_v) sum_r c_r cos_r,        cos_r = <h[r], T[r]> / (ns_r nt_r),
 *   dH[r] = -(gloss / P_v) c_r (T[r] / (ns_r nt_r) - cos_r h[r] / (ns_r |h[r]|)),
 *   ns_r = max(|h[r]|, 1e-8), nt_r = max(|T[r]|, 1e-8)   (torch's cosine_similarity: each
 * norm clamped on its own, outside autograd, so the second term keeps the unclamped |h[r]|
 * of d|h| / dh; it is cos_r h[r] / ns_r^2 above 1e-8 and 0 for a zero row).
 * h (n, feat) and T (n_t, feat): fp32 or bf16 each, independently; row pitch ld / t_ld
 * elements, 16-byte aligned rows; feat under msha_link_bce_supported for both dtypes.
 * rows int64 (n_entries), 1 <= n_entries < 2^31; an entry outside [0, min(n, n_t)) is
 * padding: it enters nothing and is counted in n_pad[0], decided before any load through
 * it.  rows NULL: entry p is row p (no histogram pass).  n, n_t < 2^31.
 * Forward: count is zeroed and filled by exact integer atomics (equal indices of a block
 * aggregated in LDS first), then one pass over the n table rows; a row that does not occur
 * reads neither table.  The dot products accumulate in fp32 lanes, the per-row scalars are
 * fp64.  coef (n, 2) fp32 = (c_r / (P_v ns nt), c_r cos_r / (P_v ns |h[r]|)), zeros for absent
 * rows; cos_rows (n) fp32, nullable, NaN for absent rows; count (n) int32, nullable.  The
 * loss sum is ordered: blocks of 1024 table rows, each in a fixed order, then the partials
 * in order (fp64): a function of the multiset of entries, bitwise reproducible and
 * invariant under a permutation of rows.  P_v is read on the device; P_v = 0 gives loss 0
 * and zero coefficients.  ws: msha_link_match_fwd_workspace_size bytes, 16-byte aligned.
 * Nothing is read back or allocated: capturable. */
MSHA_API size_t msha_link_match_fwd_workspace_size(int64_t n_entries, int64_t n); /* (ABI 16, added) */
/* The forward's histogram on its own (ABI 16, added): count (n) int32 is zeroed, then
 * count[r] = the entries equal to r inside [0, n_valid), n_valid <= n; n_pad[0] = the others. */
MSHA_API int msha_link_match_count(int64_t n_entries, int64_t n, int64_t n_valid,
                                   const int64_t* rows, int32_t* count, int32_t* n_pad,
                                   msha_stream_t stream); /* (ABI 16, added) */
MSHA_API int msha_link_match_fwd(int64_t n_entries, int32_t feat, int32_t h_dtype, const void* h,
                                 int64_t ld, int64_t n, int32_t t_dtype, const void* teacher,
                                 int64_t t_ld, int64_t n_t, const int64_t* rows, float* coef,
                                 float* cos_rows, int32_t* count, float* loss, int32_t* n_pad,
                                 void* ws, size_t ws_bytes, msha_stream_t stream); /* (ABI 16, added) */
/* Its table gradient (ABI 16, added): dH (n, feat) fp32, contiguous, 16-byte aligned,
 * dH[r] = -gloss[0] (coef[r, 0] T[r] - coef[r, 1] h[r]) with the forward's coef and gloss a
 * DEVICE scalar.  Every row is written; a row whose coefficients are zero (absent, or
 * outside the teacher) is written as zeros without a table read.  One streaming pass, no
 * workspace. */
MSHA_API int msha_link_match_bwd(int32_t feat, int32_t h_dtype, const void* h, int64_t ld,
                                 int64_t n, int32_t t_dtype, const void* teacher, int64_t t_ld,
                                 int64_t n_t, const float* coef, const float* gloss, float* dH,
                                 msha_stream_t stream); /* (ABI 16, added) */
/* The list of the rows that occur (ABI 16, added): rows int32, capacity cap = min(n,
 * n_entries), the ascending r with count[r] > 0 (the forward's count), -1 past the count;
 * n_rows[0] the count, a DEVICE int32.  msha_plan_rows' three launches over another flag;
 * ws: msha_plan_rows_workspace_size(n) bytes, 16-byte aligned.  n < 2^31 - 1. */
MSHA_API int msha_link_match_rows(int64_t n_entries, int64_t n, const int32_t* count,
                                  int32_t* rows, int32_t* n_rows, void* ws, size_t ws_bytes,
                                  msha_stream_t stream); /* (ABI 16, added) */
/* msha_link_match_bwd for the rows of that list only (ABI 16, added): vals (cap, feat) fp32,
 * 16-byte aligned, vals[i] bit for bit msha_link_match_bwd's dH[rows[i]] (the same per-row
 * formula) for i < n_rows[0], zeros from there to cap.  cap must be min(n, n_entries). */
MSHA_API int msha_link_match_bwd_rows(int64_t n_entries, int32_t feat, int32_t h_dtype,
                                      const void* h, int64_t ld, int64_t n, int32_t t_dtype,
                                      const void* teacher, int64_t t_ld, int64_t n_t,
                                      const float* coef, const float* gloss, const int32_t* rows,
                                      const int32_t* n_rows, int64_t cap, float* vals,
                                      msha_stream_t stream); /* (ABI 16, added) */

/* ---- Link-prediction training of the 'mlp' predictor with one used Linear (LLP.py:233,
 * :235, :238) (ABI 16, added) ------------------------------------------------------------
 *   x_p   = h[src_p] * h[dst_p],  out_p = sigmoid(dropout(relu(W x_p + bias)))   (n_pairs, hidden)
 *   L_lab = -(1 / Pv) sum_p out_p[label_p]                     F.nll_loss(out, label), mean
 *   L_mse = (1 / (Pv hidden)) sum_p sum_j (out_pj - t_pj)^2    F.mse_loss(out, teacher_out), mean
 *   terms = {w_label L_lab + w_mse L_mse, L_lab, L_mse}
 * h (n, feat) fp32 or bf16 (row pitch ld elements, 16-byte aligned rows); W (hidden, feat) in
 * h's dtype, contiguous; bias fp32; label int64 (n_pairs), NULL: dst itself; teacher_out
 * (n_pairs, hidden) fp32, nullable (L_mse = 0).  feat and hidden powers of two in [16, 128]
 * (msha_link_mlp_supported; feat also under msha_link_bce_supported).  A pair whose src or
 * dst lies outside [0, n) or whose label lies outside [0, hidden) is padding: it enters no
 * sum and not Pv, its out row is NaN, and no index reads outside h.  out is written by the
 * gathered msha_pair_linear / msha_pair_linear_bf16 launch (act = bias | relu | [dropout] |
 * sigmoid, the same Philox keys p * hidden + j) on pair lists whose padding entries read
 * row 0; one pass then forms Pv (n_valid[0], counted on the device) and the two sums by
 * per-block partials added in a fixed order (no float atomics).  Pv = 0 gives zeros.
 * loss (nullable) receives terms[0] as a scalar of its own.
 * ws: msha_link_mlp_loss_fwd_workspace_size bytes, 16-byte aligned.  Nothing is read back. */
MSHA_API int msha_link_mlp_supported(int32_t feat, int32_t hidden, int32_t dtype); /* host-only (ABI 16, added) */
MSHA_API int32_t msha_link_mlp_wgrad_rows(void); /* host-only (ABI 16, added) */
MSHA_API size_t msha_link_mlp_loss_fwd_workspace_size(int64_t n_pairs); /* (ABI 16, added) */
MSHA_API int msha_link_mlp_loss_fwd(int64_t n_pairs, int32_t feat, int32_t hidden, int32_t dtype,
                                    const void* h, int64_t ld, int64_t n, const int64_t* src,
                                    const int64_t* dst, const int64_t* label, const void* W,
                                    const float* bias, const float* teacher_out, float w_label,
                                    float w_mse, float drop_p, uint64_t seed, uint64_t offset,
                                    float* out, float* terms, float* loss, int32_t* n_valid,
                                    void* ws, size_t ws_bytes, msha_stream_t stream); /* (ABI 16, added) */
/* Its backward from the stored out and n_valid, gloss a DEVICE scalar (ABI 16, added):
 *   g_pj = gloss (-w_label / Pv [j == label_p] + 2 w_mse (out_pj - t_pj) / (Pv hidden))
 *   dz   = g out (1 - out) / (1 - drop_p) where out > 0.5, else 0 (msha_pair_mlp_dz's rule);
 *          (n_pairs, hidden) fp32, rows of padding pairs zero
 *   dW   = dz^T (h[src] * h[dst]) (hidden, feat) and db = colsum(dz), fp32: the A operand is
 *          gathered and multiplied in the loader of a v_mfma_f32_16x16x4_f32 kernel; pairs
 *          are cut into blocks of msha_link_mlp_wgrad_rows(), one partial per block, added in
 *          block order.  dW and db both NULL: skipped.
 *   dx   = dz W32 (n_pairs, feat) fp32 on msha_gemm_f32 (W32: the forward's W as fp32)
 *   dH[r] = sum over r's endpoints e in plan order of dx[p(e)] * h[other(e)], (n, feat) fp32,
 *          every row written (zeros without endpoints), by the chunked row pass of
 *          msha_link_bce_bwd with a row factor.  dH NULL: dx and the plan are not used.
 * Bitwise reproducible: a function of the inputs and the plan alone.
 * ws: msha_link_mlp_bwd_workspace_size bytes, 16-byte aligned. */
MSHA_API size_t msha_link_mlp_bwd_workspace_size(int64_t n_pairs, int32_t feat, int32_t hidden); /* (ABI 16, added) */
MSHA_API int msha_link_mlp_bwd(int64_t n_pairs, int32_t feat, int32_t hidden, int32_t dtype,
                               const void* h, int64_t ld, int64_t n, const int64_t* src,
                               const int64_t* dst, const int64_t* label, const float* W32,
                               const float* teacher_out, const float* out,
                               const int32_t* n_valid, float w_label, float w_mse, float drop_p,
                               const float* gloss, const int32_t* plan_rowptr,
                               const int32_t* plan_ent, const int32_t* plan_chunk_tab, float* dz,
                               float* dx, float* dW, float* db, float* dH, void* ws,
                               size_t ws_bytes, msha_stream_t stream); /* (ABI 16, added) */
/* msha_link_mlp_bwd with the table gradient on the rows of the plan's touched-row list only
 * (ABI 16, added): dz, dx, dW and db as above; vals (cap, feat) fp32, 16-byte aligned, vals[i]
 * bit for bit what msha_link_mlp_bwd writes to dH[rows[i]] for i < n_rows[0], zeros from there
 * to cap.  rows, n_rows from msha_plan_rows of the same plan; cap must be min(n, 2 n_pairs).
 * The same workspace. */
MSHA_API int msha_link_mlp_bwd_rows(int64_t n_pairs, int32_t feat, int32_t hidden, int32_t dtype,
                                    const void* h, int64_t ld, int64_t n, const int64_t* src,
                                    const int64_t* dst, const int64_t* label, const float* W32,
                                    const float* teacher_out, const float* out,
                                    const int32_t* n_valid, float w_label, float w_mse,
                                    float drop_p, const float* gloss, const int32_t* plan_rowptr,
                                    const int32_t* plan_ent, const int32_t* plan_chunk_tab,
                                    float* dz, float* dx, float* dW, float* db,
                                    const int32_t* rows, const int32_t* n_rows, int64_t cap,
                                    float* vals, void* ws, size_t ws_bytes,
                                    msha_stream_t stream); /* (ABI 16, added) */

/* ---- The GraphSAGE baseline on sparse adjacency rows (SGAE.py:41-56) (ABI 16, added) ------
 *   x = table[src]  (B, in);  z1 = relu(x W1^T + b1)  (B, M);  y = adj[src] * z1  (hidden == M);
 *   z2 = relu(y W2^T + b2)  (B, out);  logp = log_softmax(z2, dim = 1)
 * with adj given by the graph's CSR (M = g->n_cols, table rows n = g->n_rows) and vals, the
 * fp32 adjacency value of every CSR edge: y_j is zero off the row's edges, so both Linears run
 * over the edges of row src_b alone, deg (in + out) multiply-adds an entry.  Only edges with
 * adj > 0 are in a graph: negative adjacency entries are not supported.  table (n, in) fp32
 * with row pitch ld elements; W1 (M, in), b1 (M), W2 (out, M), b2 (out) fp32, contiguous; in,
 * M and out each 16, 32 or 64 (msha_sage_supported).  src int64 (B), 0 <= B < 2^30.  An entry
 * whose source is outside [0, n) is padding: its logp row is NaN and it enters no gradient,
 * decided before any load through it.  A virtual row (rowflag set) is skipped: y = 0, logp =
 * log_softmax(relu(b2)), as for a real row whose values are all 0.  A CSR row longer than M
 * (repeated columns) is treated as empty.
 * Forward: one launch, 16 lanes an entry, the parameters staged in LDS, p2 in registers;
 * logp (B, out) fp32 is the only output and nothing else is kept. */
MSHA_API int msha_sage_supported(int32_t in, int32_t M, int32_t out); /* host-only (ABI 16, added) */
MSHA_API int msha_sage_fwd(const msha_graph* g, int64_t B, const int64_t* src, int32_t in,
                           int32_t out, const float* table, int64_t ld, const float* vals,
                           const float* W1, const float* b1, const float* W2, const float* b2,
                           float* logp, msha_stream_t stream); /* (ABI 16, added) */
/* Its backward for a general upstream dlogp (B, out) (ABI 16, added), from the forward's logp:
 *   rows    the entry recomputed (the same arithmetic, so the same ReLU branches),
 *           dr = (dlogp - exp(logp) sum_o dlogp) [p2 > 0]; per edge dy_j = W2[:, j] . dr,
 *           dz1_j = a dy_j [p1_j > 0], dx_b += dz1_j W1[j, :]
 *   wgrad   dW1[j, :] += dz1_j x_b, db1[j] += dz1_j, dW2[:, j] += y_j dr, db2 += dr in LDS
 *           accumulators with one writing wave each, batch order; blocks own runs of entries
 *           (at most 512 blocks, a function of B alone) and their partials are added in a
 *           fixed order.  dW1, db1, dW2, db2: all four or none (NULL: skipped).
 *   table   dS (n, in) fp32, contiguous, 16-byte aligned, nullable: dS[r] = the dx rows of the
 *           entries with src_b = r added in batch order under msha_pair_plan(src, src); every
 *           row is written, exact zeros outside the batch.
 * No float atomics: every output is a function of the inputs alone, bitwise reproducible.
 * Nothing is read back or allocated: capturable.  ws: msha_sage_workspace_size bytes,
 * 16-byte aligned (n = g->n_rows).  B = 0 writes zeros. */
MSHA_API size_t msha_sage_workspace_size(int64_t B, int64_t n, int32_t in, int32_t M,
                                         int32_t out); /* (ABI 16, added) */
MSHA_API int msha_sage_bwd(const msha_graph* g, int64_t B, const int64_t* src, int32_t in,
                           int32_t out, const float* table, int64_t ld, const float* vals,
                           const float* W1, const float* b1, const float* W2, const float* b2,
                           const float* logp, const float* dlogp, float* dS, float* dW1,
                           float* db1, float* dW2, float* db2, void* ws, size_t ws_bytes,
                           msha_stream_t stream); /* (ABI 16, added) */
/* msha_sage_bwd with the table gradient on the rows of the batch only (ABI 16, added): the same
 * row pass, weight gradients and (src, src) plan, then msha_plan_rows of that plan into rows
 * (cap = min(n, 2 B) int32) and n_rows (a DEVICE int32): the ascending distinct sources inside
 * [0, n), -1 past the count.  row_vals (cap, in) fp32, 16-byte aligned: row_vals[i] bit for bit
 * what msha_sage_bwd writes to dS[rows[i]] (the same entries in the same order), exact zeros
 * past the count.  rows, n_rows and row_vals are OUTPUTS; rows and row_vals may be NULL when
 * cap is 0.  ws: msha_sage_rows_workspace_size bytes (msha_sage_workspace_size plus
 * msha_plan_rows' workspace), 16-byte aligned. */
MSHA_API size_t msha_sage_rows_workspace_size(int64_t B, int64_t n, int32_t in, int32_t M,
                                              int32_t out); /* (ABI 16, added) */
MSHA_API int msha_sage_bwd_rows(const msha_graph* g, int64_t B, const int64_t* src, int32_t in,
                                int32_t out, const float* table, int64_t ld, const float* vals,
                                const float* W1, const float* b1, const float* W2, const float* b2,
                                const float* logp, const float* dlogp, float* dW1, float* db1,
                                float* dW2, float* db2, int32_t* rows, int32_t* n_rows,
                                int64_t cap, float* row_vals, void* ws, size_t ws_bytes,
                                msha_stream_t stream); /* (ABI 16, added) */

#ifdef __cplusplus
}
#endif

#endif /* MSHA_GNN_H_ */
