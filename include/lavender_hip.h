/* lavender_hip.h -- C ABI of the MI355X (gfx950) kernels behind the LAVENDER pretrain hot path.
 *
 * The reference (microsoft/LAVENDER) is pure Python on torch.nn: there is no FFI in it.  Each entry
 * point below replaces the device work that a reference torch op sequence does; the reference
 * file:line it stands in for is cited per function (paths relative to the reference root).
 *
 * Conventions, as the code really behaves (ABI 7):
 *   - C linkage, POD arguments, no torch types.  Every function returns 0 on success or a negative
 *     LAV_E_* code (-1 argument, -2 launch, -3 unsupported, -4 workspace); lav_last_error() returns a message for the calling
 *     thread.  Nothing throws/exits.
 *   - All data pointers are DEVICE pointers owned by the caller.  Scratch is caller-owned too: split-K partial tiles, the LayerNorm
 *     column partials and the deferred-reduction arena live in per-(stream, kind) WORKSPACES that the caller registers with
 *     lav_set_workspace (sizes from lav_workspace_bytes).  Only when nothing was registered does the library make ONE internal
 *     allocation per (stream, kind) on first use -- a documented fallback for tools and tests; it is never grown, re-made or freed.
 *     A call that needs more than the registered / internal size fails with LAV_E_WORKSPACE and a message that names the size.
 *     No entry point calls hipDeviceSynchronize, hipStreamSynchronize or hipFree.
 *   - `stream` is a hipStream_t passed as void*.  Functions only enqueue work (asynchronous).  Mutable library state is per stream
 *     (workspace table, deferred LayerNorm queues) and guarded by mutexes, so different host threads may call concurrently on
 *     DIFFERENT streams; calls on one stream must come from one thread at a time (they are ordered by that stream).
 *     What is process-wide: lav_gemm_select (a probe hook, see there) and the LAV_* environment switches listed at the end of this
 *     header, read once on first use; they choose between equivalent kernels and exist for A/B measurements.
 *   - One device per process (one rank per GPU): every launch checks it.
 *   - bf16 tensors are raw uint16 bit patterns, row-major; "ld*" are leading dimensions in ELEMENTS.
 *   - Gradient accumulators (dW, dbias, dgamma, ...) are fp32 and are ACCUMULATED INTO (read-modify-write by the owning tile or
 *     reduction pass, atomics for small vectors): the caller zeroes them once per step (this is what lets the MTM and VTM passes
 *     share weights).
 */
#ifndef LAVENDER_HIP_H
#define LAVENDER_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* lav_last_error(void);

/* Scratch workspaces (see the conventions above).  kind:
 *   LAV_WS_SPLITK       fp32 partial tiles of split-K GEMMs issued on `stream`: a call needs splits x tiles x tile bytes (at most
 *                       splits * ceil(M / 256) * ceil(N / 256) * 256 KiB; a grouped launch the sum over its jobs)
 *   LAV_WS_LN_PARTIALS  per-block column partials of a LayerNorm backward that finishes at once: 3 * min(768, row blocks) * C * 4 bytes
 *   LAV_WS_LN_DEFER     bump arena of the deferred LayerNorm column reductions of `stream` (lav_layernorm_set_defer): any size; a
 *                       reduction that does not fit finishes at once through LAV_WS_LN_PARTIALS
 * lav_workspace_bytes(kind): the size that covers every shape of the shipped configurations (cfg2 / cfg4 / cfg5): 256 / 32 / 384 MiB.
 * lav_set_workspace(stream, kind, ptr, bytes): `ptr` (256-byte aligned, caller-owned, alive until replaced) serves every later call on
 * that stream; (NULL, 0) un-registers.  Replace a workspace only when no enqueued work of that stream still uses the old one. */
#define LAV_WS_SPLITK 0
#define LAV_WS_LN_PARTIALS 1
#define LAV_WS_LN_DEFER 2
size_t lav_workspace_bytes(int kind);
int lav_set_workspace(void* stream, int kind, void* ptr, size_t bytes);
int lav_abi_version(void);   /* 7: lav_attention_rows / lav_bert_layer_fwd_rows / lav_mlm_pair_readout / lav_retrieval_rank (additive), lav_text_embed_pre_fwd / lav_text_embed_pre_bwd (additive), lav_bert_layer_desc.ln2_eps, lav_pair_key_mask, lav_gemm_epilogue.assign / lav_gemm_tn_job.assign / lav_*_bwd_desc.assign_mask (first-touch weight gradients), lav_winl_select declared, lav_set_error no longer exported; 6: lav_workspace_bytes / lav_set_workspace, lav_layernorm_set_defer per stream + lav_layernorm_flush_all, lav_ln_bwd_extra.finish_stream removed, LAV_E_WORKSPACE; 5: lav_gemm_tn_grouped (+ lav_*_bwd_desc.group_splits), fp16 rows (out_mode 3, residual_f32 / x_f32 = 2, lav_bert_layer_desc.stream_f16), lav_layernorm_set_defer / lav_layernorm_flush, lav_attn_desc.bias_map / lav_attention_build_bias_map; 4: lav_gemm_epilogue.c_pad_writable; 3: a_rowmap / res_rowmap / res_ln_*; 2: residual_f32, lav_ln_f32, causal_from, lav_scale_by_scalar, lav_v_* validation entries, lavender_pipeline.h */

/* ---------------------------------------------------------------------------------------------
 * GEMM with fused epilogue.  Replaces every nn.Linear on the path (video_swin.py:73-79,137-139,
 * 147,168,278,286; model.py:16-18,48-49; HF BertSelfAttention/BertSelfOutput/BertIntermediate/
 * BertOutput/BertLMPredictionHead as called from model.py:242, main_pretrain_mlm.py:69,115) and
 * their autograd backward.
 *   layout 0 (NT): C[M,N] = A[M,K] . B[N,K]^T        y = x W^T
 *   layout 1 (NN): C[M,N] = A[M,K] . B[K,N]          dx = dy W
 *   layout 2 (TN): C[M,N] = A[K,M]^T . B[K,N]        dW = dy^T x   (K = token rows; `splits` > 1 allowed)
 * Epilogue, applied in this order to v = alpha*acc:
 *   v += bias[col]; [preact <- v]; v = gelu(v) if act==1; v *= gelu'(gelu_in) ; dropout(v);
 *   v *= row_scale[row / rows_per_group]; v += residual; [colsum[col] += v]; store per out_mode.
 * K-contiguous operands whose K is not a multiple of 8 must be padded with finite values up to the
 * next multiple of 8 (their last 16-byte chunk is read whole).
 * Split-K (`splits` > 1): layout 2 with out_mode 2 (weight gradients), or layouts 0/1 with a bf16 output, no
 * epilogue and N % 8 == 0 (long-K problems with few output tiles, e.g. d_hidden = dlogits . W_dec).  Partial tiles
 * go to the stream's LAV_WS_SPLITK workspace and are summed by a reduction pass on that stream.
 */
typedef struct lav_gemm_epilogue {
    const float* bias;        /* [N] fp32 or NULL */
    int act;                  /* 0 none, 1 exact (erf) GELU, 2 ReLU */
    void* preact;             /* bf16 [M, ldp]: receives z = alpha*acc+bias before the activation (or GELU'(z) when
                                 preact_is_grad), or NULL */
    long ldp;
    const void* gelu_in;      /* bf16 [M, ldg]: multiply by gelu'(gelu_in) (or by gelu_in itself when gelu_in_is_grad) */
    long ldg;
    float dropout_p;          /* hidden dropout (BertSelfOutput/BertOutput), mask = f(seed, row*N+col) */
    uint32_t seed;
    const float* row_scale;   /* per-sample stochastic-depth factor (video_swin.py:46-54), or NULL */
    int rows_per_group;
    const void* residual;     /* bf16 [M, ldr] or NULL */
    long ldr;
    float* colsum;            /* fp32 [N]: atomically accumulates the column sums of the stored values */
    float alpha;              /* 0 is read as 1 */
    int out_mode;             /* 0 bf16 store, 1 fp32 store, 2 fp32 atomicAdd, 3 fp16 store (saturating at +-65504; ldc % 8 == 0, layouts 0 / 1) */
    const float* k_keep;      /* layout 2 only: contraction rows whose k_keep[row / k_rows_per_group]==0 are skipped */
    int k_rows_per_group;
    float* rowsum_a;          /* layout 2 only: fp32 [M] += alpha * sum_k A[k, m] -- the bias gradient sum(dy), fused
                                 into the weight-gradient GEMM on the matrix cores (no extra pass over dy) */
    int preact_is_grad;       /* forward: store act'(z) instead of z (the backward then needs one multiply, no erf); 2 = GELU only,
                                 as ONE BYTE per element: q = round((g + 0.25) * 256 / 1.5), preact is uint8 [M, ldp] */
    int gelu_in_is_grad;      /* backward: gelu_in already holds GELU'(z) (1: bf16, 2: the one-byte code above, ldg in bytes) */
    int residual_f32;         /* 1: residual is fp32 [M, ldr] (the wide residual stream of the post-LN fusion encoder:
                                 pre = x + dropout(dense(.)) is then stored fp32 with out_mode 1); 2: residual is fp16 [M, ldr]
                                 (the same stream as halves -- the shipped form, out_mode 3: 11 mantissa bits against bf16's 8, half the bytes of fp32) */
    const int* a_rowmap;      /* layout 0, N % 256 == 0, K % 64 == 0, splits == 1: logical row m of A is physical row a_rowmap[m]
                                 (int32 [M], device).  The B x B pair expansion of the retrieval / VTM callers
                                 (main_retrieval_mlm.py:62-87, main_pretrain_mlm.py:74-111): the (pairs, L, H) fusion input is never
                                 materialised, the first layer's QKV GEMM reads the video / text rows of each pair through this map */
    const int* res_rowmap;    /* residual row of output row m is res_rowmap[m] (same use: the first layer's residual is the un-expanded input) */
    const float* res_ln_mean; /* non-NULL (with residual_f32 and an fp32 output): `residual` holds the PRE-LayerNorm rows and the epilogue adds */
    const float* res_ln_rstd; /* LayerNorm(residual) = (r - mean[row]) * rstd[row] * gamma[col] + beta[col] -- the same arithmetic as          */
    const float* res_ln_gamma;/* lav_layernorm_fwd, so the fp32 copy of a LayerNorm output that only feeds the next residual add              */
    const float* res_ln_beta; /* (post-LN BERT: BertSelfOutput / BertOutput) is never written: 138 MB per LayerNorm at the cfg2 shape         */
    int hm_heads;             /* > 0 (bf16 output, N % (hm_heads * hm_head_dim) == 0, hm_head_dim % 8 == 0): HEAD-MAJOR store -- element (row, col) goes
                                 to C[((col / HW) * hm_heads + (col % HW) / hm_head_dim) * hm_rows + row) * hm_head_dim + col % hm_head_dim], HW = hm_heads *
                                 hm_head_dim: the fused q | k | v projection of WindowAttention3D (video_swin.py:145-150) written as [q|k|v][head][row][dim], the
                                 layout the window-attention kernels fetch in whole lines (lav_attn_desc.qkv_headmajor).  ldc is ignored */
    int hm_head_dim;
    long hm_rows;             /* rows of one (plane, head) block, >= M */
    int c_pad_writable;       /* N % 8 != 0 and ldc >= N rounded up to 8: the caller allows columns [N, round_up(N, 8)) of C to be overwritten
                                 with unspecified values (layout 0, bf16 output, bias-only epilogue): the product then runs with full 16-byte
                                 chunks instead of the ragged-N generic epilogue (the 30522-wide vocabulary projection of BertOnlyMLMHead,
                                 main_pretrain_mlm.py:46-48, into its 30528-wide logits buffer).  B and bias are still read for N entries only */
    int assign;               /* (ABI 7) layout 2, out_mode 2 only: 1 = C is ASSIGNED (C = alpha A^T B) instead of accumulated into -- the first writer of a
                                 weight gradient in a step then needs neither a zeroed C nor the read of a read-modify-write.  Split-K needs N % 4 == 0
                                 (the reduction pass assigns); a ragged long contraction assigns with its first part and accumulates the tail */
} lav_gemm_epilogue;

int lav_gemm_bf16(void* stream, int layout, int M, int N, int K, const void* A, long lda, const void* B, long ldb,
                  void* C, long ldc, const lav_gemm_epilogue* epi, int splits);
/* Grouped weight gradients: C_j[M_j, N_j] (fp32) += alpha_j * A_j[K_j, M_j]^T . B_j[K_j, N_j] for 1 ... 4 independent jobs in ONE launch -- the
 * four nn.Linear weight gradients of a Swin block (video_swin.py:73-79,137-139,168) or of a fusion layer (HF BertLayer).  One by one each of
 * them needs 8 ... 32 split-K parts to fill the machine; together their tiles need `splits` = 1 ... 3.  rowsum_a (fp32 [M_j], += alpha * column
 * sums of A: the bias gradient) and k_keep / k_rows_per_group (stochastic depth: contraction rows of dropped samples are skipped) as in
 * lav_gemm_epilogue.  Jobs that do not fit the 256 x 256 weight-gradient kernel (M_j >= 160, N_j % 256 == 0, K_j % 32 == 0) make the call run
 * every job through lav_gemm_bf16(layout 2) with its own fallback_splits instead: same results up to fp32 summation order. */
typedef struct lav_gemm_tn_job {
    int M, N, K;
    const void* A; long lda;      /* bf16 [K, lda >= M] */
    const void* B; long ldb;      /* bf16 [K, ldb >= N] */
    float* C; long ldc;           /* fp32 [M, ldc >= N], accumulated */
    float* rowsum_a;              /* or NULL */
    const float* k_keep;          /* or NULL */
    int k_rows_per_group;
    float alpha;                  /* 0 is read as 1 */
    int fallback_splits;
    int assign;                   /* (ABI 7) 1 = C is assigned, not accumulated into (lav_gemm_epilogue.assign) */
} lav_gemm_tn_job;
int lav_gemm_tn_grouped(void* stream, int n_jobs, const lav_gemm_tn_job* jobs, int splits);

/* Tuning / probe hook: selects between kernel variants at run time (within-process A/B measurements in tools/): which 2 = ping-pong
 * weight-gradient kernel on/off, 5 = probe bits of the 256x256 kernel (timing only, wrong results), 6 = column-group width of the tile
 * walk, 7 / 9 = 192-row tiles / their loader-wave form on/off, 11 = phase-shifted two-group tile (bit 0: 256-row, bit 1: 192-row;
 * results bit-identical to the tiles it replaces), 12 = fewest output rows for the 256-row weight-gradient tiles (LAV_GEMM_TN_MINM), 13 = grouped
 * weight-gradient launches on/off (LAV_GEMM_TN_GROUP).  2, 12 and 13 also move the split factors lav_gemm_splits / lav_gemm_tn_splits answer with.  Returns the
 * previous value, -1 for an unknown selector.  Results are identical up to fp32 summation order (except selector 5). */
int lav_gemm_select(int which, int value);
/* Probe hooks, not part of the contract: the launches lav_gemm_bf16 / lav_gemm_tn_grouped would make for a call, in order, without making them (no
 * device is needed; tests/ compare the route with their host copy of it).  Arguments as for those entries minus the stream and the operand
 * pointers (lav_gemm_tn_job.A / B / C may be NULL); pointers of the epilogue are only tested for presence.  Writes at most max_out entries and
 * returns the number of launches (1 ... 4, grouped fallback: up to 16), or the error code the entry itself would return for the call. */
typedef struct lav_gemm_launch_info {
    const char* kernel;           /* the kernel's name without template arguments, e.g. "gemm_ps_kernel" */
    int tile_rows, tile_cols;     /* output tile of the launch (a reduction: the tile of the partial sums it reads) */
    unsigned grid, block;         /* workgroups, threads per workgroup */
} lav_gemm_launch_info;
int lav_gemm_plan(int layout, int M, int N, int K, long lda, long ldb, long ldc, const lav_gemm_epilogue* epi, int splits,
                  lav_gemm_launch_info* out, int max_out);
int lav_gemm_tn_grouped_plan(int n_jobs, const lav_gemm_tn_job* jobs, int splits, lav_gemm_launch_info* out, int max_out);
/* Split-K policy (additive in ABI 7; no device is needed).  Scratch is caller-owned, so the caller has to know a call's split factor and workspace
 * bytes BEFORE the call: these two entries answer both from the route plan the call itself will take.
 * lav_gemm_splits: arguments as lav_gemm_plan.  splits <= 0 asks for the library's own factor -- layout 2: a weight gradient on the tile the plan gives it
 * (epi->k_keep only tested for presence); layouts 0 / 1: a long-K product without epilogue whose output under-fills the machine, else 1 -- and splits > 0
 * keeps the caller's.  Returns that factor (>= 1), or the error code lav_gemm_bf16 would return.  With ws_bytes != NULL the call is validated as by
 * lav_gemm_bf16 and *ws_bytes receives the LAV_WS_SPLITK bytes it will request (0: none); with NULL only the factor is worked out (epi may be NULL then).
 * lav_gemm_tn_splits: jobs as for lav_gemm_tn_grouped_plan (up to four weight gradients of one stage, a common contraction).  A job whose fallback_splits
 * is <= 0 has it REPLACED by the library's factor for that job alone.  Returns the group factor to hand lav_gemm_tn_grouped (splits > 0: the caller's;
 * else the library's), 0 when that entry would run the jobs one by one, or a negative error code.  *ws_bytes (may be NULL) receives the LAV_WS_SPLITK
 * bytes that cover the grouped launch AND each job run alone with its fallback_splits (the stage entries do the latter without a second stream). */
int lav_gemm_splits(int layout, int M, int N, int K, long lda, long ldb, long ldc, const lav_gemm_epilogue* epi, int splits, size_t* ws_bytes);
int lav_gemm_tn_splits(int n_jobs, lav_gemm_tn_job* jobs, int splits, size_t* ws_bytes);
/* Same kind of hook for the large-window attention kernels (windows of up to 768 tokens without the precomputed tables, attention_winl.hip): parts = 0
 * lets the library split a problem into query parts by its own rule (the default), 1 / 3 force that many, -1 routes large windows to the generic
 * kernels (tests compare the two).  Process-wide; returns the previous value. */
int lav_winl_select(int parts);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm over the last dimension (nn.LayerNorm at video_swin.py:209,245,282,399-403,476-478;
 * model.py:85; HF BertEmbeddings/BertSelfOutput/BertOutput/BertPredictionHeadTransform LayerNorm).
 *   gather_mode 0: row r of x is x + r*ldx.
 *   gather_mode 1: PatchMerging gather (video_swin.py:271-284): logical row (b,t,h2,w2) of width 4*C0 is
 *                  the concat [x(2h2,2w2), x(2h2+1,2w2), x(2h2,2w2+1), x(2h2+1,2w2+1)] of C0-wide source
 *                  rows of a (BT, H, W, C0) token tensor (H, W even).
 * mean/rstd (fp32 [rows]) are written for the backward.
 */
typedef struct lav_ln_gather {
    int mode;                 /* 0 plain, 1 patch-merge 2x2 */
    int H, W, C0;             /* source token grid (per frame) and channel count, mode 1 */
} lav_ln_gather;

/* Optional fp32 side of the LayerNorm I/O (NULL = all-bf16): the fusion encoder keeps its residual stream in fp32 --
 * the pre-LN sums are fp32 GEMM outputs (x_f32 = 1) and the normalised rows are written twice, bf16 for the next GEMM's
 * operand and fp32 (y32) for the next residual add.  y (bf16) may be NULL when only the fp32 copy is wanted. */
typedef struct lav_ln_f32 {
    int x_f32;                /* 1: x is fp32 [rows, ldx]; 2: x is fp16 [rows, ldx] (the residual stream stored as halves) */
    void* y32; long ldy32;    /* fp32 copy of the output, or NULL */
} lav_ln_f32;

int lav_layernorm_fwd(void* stream, int rows, int C, const void* x, long ldx, const lav_ln_gather* gather,
                      const float* gamma, const float* beta, float eps, void* y, long ldy, float* mean, float* rstd,
                      const lav_ln_f32* f32io);

/* Backward.  dx = LNbwd(dy) [+ add_in]  (add_in: the residual-branch gradient, bf16, same layout as dx).
 * dgamma/dbeta (fp32 [C]) are accumulated atomically.  With gather.mode==1 dx is scattered back to the
 * (BT,H,W,C0) source layout.
 * Optional `extra`: a second output dx2 = row_scale[row/rows_per_group] * dropout_mask(seed; row*C+col)/(1-p)
 * * dx -- the gradient entering the dense layer that FED this residual stream (hidden dropout of
 * BertSelfOutput/BertOutput, or the stochastic-depth factor of a Swin block) -- with its column sums
 * accumulated into colsum (that dense layer's bias gradient). */
typedef struct lav_ln_bwd_extra {
    void* dx2; long lddx2;
    const float* row_scale; int rows_per_group;
    float dropout_p; uint32_t seed;
    float* colsum;
    int x_f32;                /* the saved LayerNorm input x is fp32 (1) or fp16 (2) (see lav_ln_f32) */
} lav_ln_bwd_extra;

int lav_layernorm_bwd(void* stream, int rows, int C, const void* dy, long lddy, const void* x, long ldx,
                      const lav_ln_gather* gather, const float* gamma, const float* mean, const float* rstd,
                      const void* add_in, long ldadd, void* dx, long lddx, float* dgamma, float* dbeta,
                      const lav_ln_bwd_extra* extra);

/* Deferred column reductions, per stream.  lav_layernorm_set_defer(stream, 1): every following lav_layernorm_bwd on that stream (also
 * the ones the stage-level entries issue) only runs its row pass -- dx (and dx2) are complete as before -- and QUEUES the reduction of its
 * per-block partials (kept in the stream's LAV_WS_LN_DEFER workspace) into dgamma / dbeta / colsum.  lav_layernorm_flush(stream) completes
 * all queued reductions of that stream in ONE launch on it; lav_layernorm_flush_all(join_stream) does so for EVERY stream, each on its
 * own stream, and makes join_stream wait (event) for the others -- use it where the stream that ran the backward is not known.  The three
 * vectors are parameter gradients (nn.LayerNorm weight / bias, the bias of the dense layer in front): nothing in the dy -> dx chain reads
 * them, so the caller flushes where gradients become final (before the gradient exchange, the norm, the optimizer).  A call flushes by
 * itself when 48 reductions are queued or the arena is full; switching the mode off flushes.  set_defer returns the previous mode (0 / 1)
 * or a NEGATIVE error code.  At most 16 streams hold a queue: on a 17th the mode stays off (its reductions finish at once) and set_defer
 * returns 0.  Default: off.  Every queue has its own lock: an append publishes a complete job, a flush takes whole jobs, so
 * lav_layernorm_flush_all may run on one host thread while others are inside LayerNorm backwards on THEIR streams (what it flushes of a
 * stream that is mid-backward are the reductions queued so far; the rest follow at that stream's next flush).  The arena pointer is re-read
 * from the workspace table whenever a queue is empty, and lav_set_workspace(stream, LAV_WS_LN_DEFER, ...) flushes that stream's queue first:
 * after it returns, only enqueued work of the stream still reads the old buffer (the general rule for replacing a workspace). */
int lav_layernorm_set_defer(void* stream, int on);
int lav_layernorm_flush(void* stream);
int lav_layernorm_flush_all(void* join_stream);

/* Row-wise helper: out = row_scale[row/rpg] * gelu'(gelu_in) * dropout(seed; in), column sums into colsum.
 * Produces a dense-branch gradient from a residual-stream gradient (inverse of the GEMM epilogue's dropout /
 * stochastic depth / GELU).  out may be NULL (column sums only); gelu_in may be NULL. */
int lav_scale_mask_rows(void* stream, int rows, int C, const void* in, long ldi, void* out, long ldo,
                        const float* row_scale, int rows_per_group, float dropout_p, uint32_t seed, float* colsum,
                        const void* gelu_in, long ldg);

/* Column sums of a bf16 matrix into fp32 (bias gradients of the QKV and decoder linears). */
int lav_colsum_bf16(void* stream, int rows, int C, const void* x, long ldx, float* out);

/* ---------------------------------------------------------------------------------------------
 * Attention.  One kernel family for
 *   (a) shifted-window 3D attention: roll + window_partition + WindowAttention3D core + window_reverse
 *       + roll back (video_swin.py:82-91,145-167,218-239,290-305) as pure index math on the un-rolled
 *       (B,D,H,W,3C) qkv token tensor, relative-position bias gathered from the (table_rows, heads)
 *       parameter with index = code(i)-code(j)+const, shift mask from region ids;
 *   (b) fusion-encoder self-attention (HF BertSelfAttention eager path as called at model.py:242) with the
 *       additive key mask (1-m)*finfo.min of model.py:239 and attention-probability dropout.
 * qkv: bf16 (tokens, 3*heads*hd), rows ordered [q | k | v], head-major inside each (video_swin.py:147).
 * out: bf16 (tokens, heads*hd).  lse: fp32 (problems*heads, Npad) log-sum-exp per query for the backward.
 */
typedef struct lav_attn_desc {
    int mode;                 /* 0 window, 1 sequence */
    int heads, head_dim;      /* head_dim 32 (Swin) or 64 (BERT) */
    /* window mode: token grid and (already clamped) window / shift, video_swin.py:93-106 */
    int B, D, H, W;
    int wd, wh, ww, sd, sh, sw;
    int cfg_wh, cfg_ww;       /* CONFIGURED window (h,w) extents: define the bias-table index stride (:121-135) */
    int cfg_wd;
    const float* bias_table;  /* fp32 ((2cfg_wd-1)(2cfg_wh-1)(2cfg_ww-1), heads) */
    /* sequence mode */
    int n_seq, L;
    const int32_t* key_mask;  /* int32 (n_seq, L) 1 = attend, 0 = masked; or NULL */
    float dropout_p; uint32_t seed;
    float scale;              /* head_dim^-0.5 */
    /* window mode, N <= 256: optional precomputed tables (see lav_attention_window_tables / _build_bias).  When
     * `comb` is non-NULL the kernels read token rows from tok_table and the (bias + shift mask + key padding)
     * term from the fragment-ordered bf16 tables instead of re-deriving them per element. */
    const int32_t* tok_table; /* int32 (windows_per_sample, 256): token row within the sample, -1 = padding */
    const uint8_t* win_type;  /* uint8 (windows_per_sample): mask type of the window (which shifted axes are last) */
    const uint8_t* type_region; /* uint8 (n_types, 256): shift-region id of in-window token i for that type */
    int n_types;
    const void* comb;         /* bf16 (n_types, heads, 8 q-tiles, 8 k-tiles, 64 lanes, 16): keys x queries fragments */
    const void* combT;        /* same, queries x keys fragments (dK/dV pass) */
    int causal_from;          /* sequence mode: 0 = plain key mask ("full", model.py:219); > 0 = the seq2seq mask of
                                 LAVENDER_Base.get_attn_mask (model.py:208-218) with this many prefix (video / pre-text) keys:
                                 prefix keys follow key_mask for every query, text keys are causal among the text queries
                                 and invisible to the prefix queries */
    int qkv_headmajor;        /* window mode with the precomputed tables (comb != NULL) only: the qkv operand is laid out
                                 [q | k | v][head][token row][head_dim] (as lav_gemm_epilogue.hm_heads writes it) instead of row-major
                                 (rows, 3 * heads * head_dim); a window's operand pieces are then whole 128-byte lines.  dqkv stays row-major */
    const int32_t* bias_map;  /* window mode with the precomputed tables, optional: int32 (2, n_types, 65536) filled ONCE per geometry by
                                 lav_attention_build_bias_map -- the bias-table row (and shift-mask / padding class) of every element of comb / combT;
                                 lav_attention_build_bias then only gathers the current table values through it (same bits, ~4x less time) */
} lav_attn_desc;

int lav_attention_fwd(void* stream, const lav_attn_desc* d, const void* qkv, void* out, float* lse);
/* dqkv: bf16 same layout as qkv (fully written).  dbias_table: fp32, atomically accumulated (window mode). */
int lav_attention_bwd(void* stream, const lav_attn_desc* d, const void* qkv, const void* out, const void* dout,
                      const float* lse, void* dqkv, float* dbias_table);
/* Window mode, N <= 256 with the precomputed tables or N <= 768 without them (lav_attention_bias_split(d) == 1): the bias-table gradient
 * ALONE.  Call lav_attention_bwd with dbias_table = NULL first (it leaves delta behind the lse in the lse buffer), then this on any stream ordered after it --
 * the table gradient is a parameter gradient and does not have to sit in the dy -> dx chain (the reference computes it inside
 * autograd of video_swin.py:153-160). */
int lav_attention_bwd_bias(void* stream, const lav_attn_desc* d, const void* qkv, const void* dout, const float* lse,
                           float* dbias_table);
/* 1 when the bias-table gradient of this descriptor can run as its own launch (lav_attention_bwd_bias), 0 when
 * lav_attention_bwd has to produce it (sequence mode has none; windows of more than 768 tokens use the generic kernels). */
int lav_attention_bias_split(const lav_attn_desc* d);
size_t lav_attention_lse_elems(const lav_attn_desc* d);
/* Probe hook, not part of the contract: the launches an attention entry would make for a descriptor, in order, without making them (no device is
 * needed; tests/ assert the route they exercise).  pass: 0 = lav_attention_fwd, 1 = lav_attention_bwd with dbias_table = NULL, 2 = with a table,
 * 3 = lav_attention_bwd_bias.  Pointers of the descriptor are only tested for presence.  Writes at most max_out entries and returns the number of
 * launches (1 ... 3), or the error code the entry itself would return for the descriptor. */
typedef struct lav_attn_launch_info {
    const char* kernel;           /* the kernel's name without template arguments, e.g. "win_bwd1" */
    const char* route;            /* "window persistent", "window large", "sequence one-image", "sequence chunked", "generic window", "generic sequence" */
    unsigned grid_x, grid_y, block;   /* workgroups, threads per workgroup */
    unsigned lds_bytes;           /* dynamic LDS of the launch */
    int split;                    /* the kernel's partition scalar: batch slices (win_*), query parts (winl_fwd / dq / dkv), window slices (winl_dbias),
                                     8-tile parts (seql_*), tile rounds per wave (generic kernels); 0 = none */
    int delta_negated;            /* 1: the route's backward leaves -delta behind the lse (window persistent), 0: +delta */
} lav_attn_launch_info;
int lav_attention_plan(const lav_attn_desc* d, int pass, lav_attn_launch_info* out, int max_out);
/* Fills d->comb and d->combT (each n_types*heads*8*8*64*16 bf16) from the current bias table: value(q,k) =
 * table[index(q,k), head] + (region(q) != region(k) ? -100 : 0), -30000 for padded keys (video_swin.py:153-160). */
int lav_attention_build_bias(void* stream, const lav_attn_desc* d);
/* Fills d->bias_map (see lav_attn_desc.bias_map) for the descriptor's geometry: depends on the window, the configured window and the shift
 * pattern only (relative_position_index and compute_mask, video_swin.py:118-135,290-305), not on the parameters. */
int lav_attention_build_bias_map(void* stream, const lav_attn_desc* d);

/* ---------------------------------------------------------------------------------------------
 * Patch embedding im2col (PatchEmbed3D, video_swin.py:388-405): (B,3,T,H,W) fp32 NCDHW clip ->
 * bf16 (B*T*(H/4)*(W/4), 96) rows [c][kt][kh][kw] with the zero frame appended at t = T (:396);
 * the Conv3d itself is lav_gemm_bf16 on the (E, 96) flattened weight.
 * img may be given as (B,T,3,H,W) (the EncVideo input, model.py:44) with frame_major = 1.
 */
int lav_patch_im2col(void* stream, const float* img, int B, int T, int H, int W, int frame_major, void* out);

/* Video token assembly (EncVideo.forward, model.py:69-85): rows (b,t,0) = emb_cls, (b,t,1+p) = feat[b,t,p];
 * + emb_pos[p'] + emb_len[t]; LayerNorm(eps) -> out row [b*seq_rows + t*(1+hw) + p'] (bf16, width Hd <= 1024).
 * The backward recomputes the pre-LN sum from feat and the embeddings (nothing but mean/rstd is saved). */
int lav_video_embed_fwd(void* stream, int B, int T, int hw, int Hd, const void* feat, const float* emb_cls,
                        const float* emb_pos, const float* emb_len, const float* gamma, const float* beta, float eps,
                        void* out, long seq_rows, float* mean, float* rstd);
int lav_video_embed_bwd(void* stream, int B, int T, int hw, int Hd, const void* dout, long seq_rows, const void* feat,
                        const float* emb_cls, const float* emb_pos, const float* emb_len, const float* gamma,
                        const float* mean, const float* rstd, void* dfeat, float* d_cls, float* d_pos, float* d_len,
                        float* dgamma, float* dbeta);

/* Text embedding (HF BertEmbeddings via EncTxt.forward, model.py:125-129): word[ids] + pos[0..X) + type[0]
 * -> LayerNorm(eps) -> dropout -> bf16 (n, X, Hd). */
int lav_text_embed_fwd(void* stream, int n, int X, int Hd, const int64_t* ids, const float* word, const float* pos,
                       const float* type0, const float* gamma, const float* beta, float eps, float dropout_p,
                       uint32_t seed, void* out, float* mean, float* rstd);
int lav_text_embed_bwd(void* stream, int n, int X, int Hd, const int64_t* ids, const void* dout, const float* word,
                       const float* pos, const float* type0, const float* gamma, const float* mean, const float* rstd,
                       float dropout_p, uint32_t seed, float* d_word, float* d_pos, float* d_type0, float* dgamma,
                       float* dbeta);

/* (ABI 7, additive) Text embedding behind a pre-text segment (LAVENDER_Base.get_pretxt / prepro_txt_inputs, model.py:250-307: a task token
 * emb_task[task_tok2id[task]] or an embedded prompt between the video rows and the text rows).  Text j's block of `out` is Lp + X rows
 * [pre-text ; text]: the Lp pre-text rows are copied from the bf16 rows pre + j * pre_stride (pre_stride 0: ONE (Lp, Hd) block for every
 * text; Lp * Hd: a block per text), the X text rows are those of lav_text_embed_fwd bit for bit (same dropout keys; mean / rstd (n * X)
 * indexed as there).  Lp = 0 is lav_text_embed_fwd.  pre: 16-byte aligned. */
int lav_text_embed_pre_fwd(void* stream, int n, int Lp, int X, int Hd, const int64_t* ids, const float* word, const float* pos,
                           const float* type0, const float* gamma, const float* beta, float eps, float dropout_p, uint32_t seed,
                           const void* pre, long pre_stride, void* out, float* mean, float* rstd);
/* Backward of lav_text_embed_pre_fwd over the (n, Lp + X, Hd) dout: the parameter gradients of lav_text_embed_bwd from the text rows, and
 * the pre-text gradient.  pre_stride 0: d_pre = sum_j dout[j, 0:Lp], summed in fp32 in a fixed order (run-to-run identical, no float
 * atomics; n >= 8 texts are split over workgroups whose fp32 partials go to the stream's LAV_WS_LN_PARTIALS workspace, groups * Lp * Hd * 4
 * bytes, and a second launch sums them in group order); d_pre_mode 0 accumulates that sum into the fp32 (Lp, Hd) d_pre (a parameter-gradient
 * row), 1 writes it as bf16 rows.  pre_stride Lp * Hd: d_pre_mode must be 1 and d_pre (n, Lp, Hd) bf16 receives each text's own rows. */
int lav_text_embed_pre_bwd(void* stream, int n, int Lp, int X, int Hd, const int64_t* ids, const void* dout, const float* word,
                           const float* pos, const float* type0, const float* gamma, const float* mean, const float* rstd,
                           float dropout_p, uint32_t seed, float* d_word, float* d_pos, float* d_type0, float* dgamma,
                           float* dbeta, long pre_stride, void* d_pre, int d_pre_mode);

/* Row gather / gather-sum: builds the fusion input [video rows of sample vi | text rows of sample ti]
 * (go_cross concat model.py:235 + VTM pairing main_pretrain_mlm.py:74-111) and its backward. */
int lav_gather_rows(void* stream, int n_rows, int C, const void* src, long lds_, const int32_t* src_row, void* dst,
                    long ldd);
/* out[r] = sum_{k in [start[r], start[r+1])} src[list[k]]  (bf16 in, bf16 out, fp32 accumulate) */
int lav_gather_sum_rows(void* stream, int n_out, int C, const void* src, long lds_, const int32_t* start,
                        const int32_t* list, void* out, long ldo);
/* (ABI 7) Key mask of a pair list (get_attn_mask "full", model.py:194-221, over the pairs of main_pretrain_mlm.py:74-111):
 * out[k][c] = c < Lv ? mask_img[vi[k]][c] : mask_txt[ti[k]][c - Lv]; masks are the reference's int64 0 / 1 tensors (B, Lv) / (nt, X),
 * out is the (n, Lv + X) int32 key mask the sequence-attention kernels read (lav_attn_desc.key_mask). */
int lav_pair_key_mask(void* stream, int n, int Lv, int X, const int64_t* mask_img, const int64_t* mask_txt, const int32_t* vi,
                      const int32_t* ti, int32_t* out);

/* ---------------------------------------------------------------------------------------------
 * Cross entropy with ignore_index = -1, mean over labelled rows (agent.py:72, main_pretrain_mlm.py:158-163).
 * logits: bf16 (rows, ld) with V valid columns.  Accumulates loss_sum[0] += sum_i nll_i, loss_sum[1] += #labelled
 * (fp32, caller zeroes) and overwrites logits IN PLACE with grad_scale * (softmax - onehot); rows with label -1
 * and the padding columns [V, ld) become 0.  grad_scale is 1/#labelled when the host knows the count (the
 * labels are built on the host, main_pretrain_mlm.py:178-200); otherwise pass 1 and call lav_scale_by_count,
 * which multiplies by gscale / loss_sum[1] read on the device. */
int lav_cross_entropy_fwd_bwd(void* stream, int rows, int V, void* logits, long ld, const int64_t* labels,
                              float* loss_sum, float grad_scale, int write_grad /* 0: loss only, logits untouched */);
int lav_scale_by_count(void* stream, long n_elems, void* x_bf16, const float* loss_sum, float gscale);
/* x (bf16, or fp32 when x_is_f32) *= scalar_dev[0], the scalar read on the device: applies the upstream autograd gradient
 * of a loss (gradient accumulation loss / k, loss weights, a GradScaler) to the stored d(loss)/d(logits) without a host
 * sync; a scalar of exactly 1 returns after one load.  n_elems % 8 == 0. */
int lav_scale_by_scalar(void* stream, long n_elems, void* x, int x_is_f32, const float* scalar_dev);
/* same contract on FP32 logits with few classes (the (B, O) matching scores of the task-specific variant) */
int lav_cross_entropy_f32_fwd_bwd(void* stream, int rows, int V, float* logits, long ld, const int64_t* labels,
                                  float* loss_sum, float grad_scale, int write_grad);

/* ---------------------------------------------------------------------------------------------
 * Captioning loss (model_for_captioning.py:10-37 on the labelled rows, main_caption.py:225-230): label smoothing as the KL
 * divergence to q (q_t = 1 - label_smoothing, q_c = label_smoothing / (V - 1) elsewhere), "drop the worst" rows, the arg-max
 * accuracy read-out and the in-place logit gradient.  logits: bf16 (rows, ld), V valid columns, ld % 8 == 0; labels int64 in
 * [0, V), -1 = ignore (a label outside [0, V) is treated as -1, never read as a column).  Per labelled row r, in fp32:
 *   row_loss[r] = sum_c q_c (log q_c - log p_c), row_lse[r] = log sum exp, correct[r] = (arg-max column, lowest index on a tie, == label);
 * unlabelled rows write 0.  k = number of rows whose loss is averaged, computed by the caller from the labelled-row count it knows:
 * that count when select == 0 (every labelled row is kept: one launch over the logits, the passes of lav_cross_entropy_fwd_bwd), and
 * int(count * (1 - drop_worst_ratio)) when select != 0: kept[r] = 1 for the k labelled rows that come first by (loss ascending, row
 * ascending; NaN last), found by counting -- no sort, no atomics -- and the gradient is written by a second launch behind the row losses.
 * out[0] = sum of the kept losses, out[1] = k, out[2] = sum of correct, out[3] = number of labelled rows, added in a fixed order
 * (identical bits run to run); the loss is out[0] / out[1].  write_grad != 0 overwrites the logits IN PLACE with (p - q) / k on kept
 * rows and 0 on dropped rows, unlabelled rows and the padding columns [V, ld); write_grad == 0 leaves them untouched.
 * row_loss, row_lse (fp32) and correct, kept (int32) hold `rows` elements each, out four floats; nothing needs zeroing. */
int lav_caption_loss_fwd_bwd(void* stream, int rows, int V, void* logits, long ld, const int64_t* labels, float label_smoothing,
                             int k, int select, float* row_loss, float* row_lse, int32_t* correct, int32_t* kept, float* out,
                             int write_grad);

/* ---------------------------------------------------------------------------------------------
 * Video-text matching score head of the task-specific pre-training variant: the last layer of
 * self.fc = Sequential(Dropout, Linear(H,2H), ReLU, Linear(2H,1)) (main_pretrain_task_specific.py:128-133)
 * and "out_vtm = fc(out[:, Lv]).view(B, O) / temp" (:168-170).  Dropout and Linear+ReLU run through
 * lav_scale_mask_rows / lav_gemm_bf16 (act = 2); these two entries do the (n, F) x (F,) row dots.
 *   fwd: logits[r / O][r % O] = (h[r,:] . w + bias[0]) * inv_temp        (logits: FP32 (n/O, ld), ld >= O)
 *   bwd: dz = dlogits (fp32) * inv_temp; dh[r,:] = dz_r * w * act_grad[r,:] (act_grad = ReLU'(z1) stored by the GEMM,
 *        or NULL); dw += sum_r dz_r h[r,:]; db[0] += sum_r dz_r      (fp32 atomics into the gradient arena) */
int lav_pair_score_fwd(void* stream, int n, int F, const void* h, long ldh, const void* w_bf16, const float* bias,
                       float inv_temp, int O, void* logits, long ld);
int lav_pair_score_bwd(void* stream, int n, int F, const void* dlogits, long ld, int O, float inv_temp, const void* h,
                       long ldh, const void* act_grad, long ldg, const void* w_bf16, void* dh, long lddh, float* dw,
                       float* db);

/* ---------------------------------------------------------------------------------------------
 * Optimizer over the flat parameter arena (Agent_Base.backward_step, agent.py:241-250: unscale/clip by
 * global L2 norm, AdamW with betas (0.9,0.98), per-group lr / weight decay from agent.py:96-140).
 *   lav_sumsq: out[0] += sum g^2 (fp32).   lav_adamw_step: one fused pass over the whole arena (parameters
 *   are laid out in execution order, 64-element aligned; block_group maps each 64-element block to one of the
 *   four (swin|other) x (decay|no-decay) groups of agent.py:96-140):
 *   g *= min(1, max_norm/(sqrt(sumsq)+1e-6)); p *= 1-lr*wd; m,v update; p -= lr*mhat/(sqrt(vhat)+eps);
 *   writes the bf16 working copy used by the GEMMs. */
int lav_sumsq_f32(void* stream, long n, const float* g, float* out);
/* (ABI 7) base[blocks[i] * block_elems .. + block_elems) = 0 for i < n_blocks: the per-step zeroing of the gradient arena's atomically
 * accumulated parts (bias / LayerNorm vectors, embedding and bias tables); the weight matrices are ASSIGNED by their first writer
 * (lav_gemm_epilogue.assign) and need no fill (optimizer.zero_grad(), agent.py:250). */
int lav_zero_blocks(void* stream, float* base, const int32_t* blocks, long n_blocks, int block_elems);
int lav_adamw_step(void* stream, long n, float* p, const float* g, float* m, float* v, void* p_bf16,
                   const uint8_t* block_group /* per 64-element block of the arena: bits 0-1 group id (0..3), bit 2 = the
                                                 block belongs to a parameter that never gets a gradient on this path
                                                 (grad None in the reference: AdamW skips it, no decay) */,
                   const float lr[4], const float wd[4], float beta1, float beta2, float eps, int step,
                   const float* gradsq, float max_norm, float grad_div);
/* Transposed bf16 working copy of the weight matrices: every nn.Linear backward-to-input (dx = dy W, the autograd of
 * video_swin.py:73-79,137-139 / the HF BERT linears) then runs in the forward GEMM layout.  One launch over all
 * matrices: dst[dst_off + c * ld_dst + r] = src[src_off + r * cols + c]; tile0 = index of the matrix's first 64x64
 * tile in the launch (exclusive prefix sum of ceil(rows/64) * ceil(cols/64)); src_off / dst_off in elements, 8-aligned,
 * ld_dst % 8 == 0. */
typedef struct lav_mat_desc {
    long src_off, dst_off;
    int rows, cols, ld_dst, tile0;
} lav_mat_desc;
int lav_transpose_bf16_batched(void* stream, int n_mats, const lav_mat_desc* descs_dev, int total_tiles, const void* src_bf16,
                               void* dst_bf16);
int lav_cast_f32_to_bf16(void* stream, long n, const float* in, void* out);
/* bf16 -> fp32: the summed half-precision gradient buckets of the data-parallel exchange (utils/deepspeed.py:20-28 trains with
 * fp16 gradients) back into the fp32 gradient arena; both buffers 16-byte aligned. */
int lav_cast_bf16_to_f32(void* stream, long n, const void* in, float* out);
int lav_fill_droppath(void* stream, int n_blocks, int B, const float* keep_prob, uint32_t seed, float* scale);

/* ---------------------------------------------------------------------------------------------
 * fp32-I/O VALIDATION mode (SURVEY.md section 8c tier T2; north_star "MLM logits within 1e-3 of reference"): the forward
 * path with fp32 activations end to end.  Forward only, eval arithmetic, speed irrelevant.  LayerNorm uses
 * lav_layernorm_fwd with lav_ln_f32 {x_f32 = 1, y32}.
 *   lav_v_gemm_f32       every nn.Linear of the path (same call sites as lav_gemm_bf16) on v_mfma_f32_32x32x2_f32 (exact fp32):
 *                        C[M,N] = act(A[M,K] . B[N,K]^T + bias) + residual; act 0 none, 1 erf-GELU, 2 ReLU
 *   lav_v_attention_f32  window / sequence attention of lav_attention_fwd for ANY geometry, including token grids that
 *                        are not window multiples: the zero-pad branch of video_swin.py:211-215,241-242 (padding is applied
 *                        after norm1, so a padded token's q/k/v is the qkv bias = pad_qkv[3C]); qkv fp32 (tokens, 3C), out fp32
 *   lav_v_im2col_f32     lav_patch_im2col with fp32 rows
 *   lav_v_video_embed_f32 / lav_v_text_embed_f32   lav_video_embed_fwd / lav_text_embed_fwd (no dropout) with fp32 I/O
 *   lav_v_gather_rows_f32 lav_gather_rows on fp32 rows */
int lav_v_gemm_f32(void* stream, int M, int N, int K, const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                   const float* bias, int act, const float* residual, long ldr);
int lav_v_attention_f32(void* stream, const lav_attn_desc* d, const float* qkv, float* out, const float* pad_qkv);
int lav_v_im2col_f32(void* stream, const float* img, int B, int T, int H, int W, int frame_major, float* out);
int lav_v_video_embed_f32(void* stream, int B, int T, int hw, int Hd, const float* feat, const float* emb_cls,
                          const float* emb_pos, const float* emb_len, const float* gamma, const float* beta, float eps,
                          float* out, long seq_rows);
int lav_v_text_embed_f32(void* stream, int n, int X, int Hd, const int64_t* ids, const float* word, const float* pos,
                         const float* type0, const float* gamma, const float* beta, float eps, float* out);
int lav_v_gather_rows_f32(void* stream, int n_rows, int C, const float* src, long lds_, const int32_t* src_row, float* dst,
                          long ldd);

/* ---------------------------------------------------------------------------------------------
 * Stage-level entries (round 4; SURVEY section 8(b): lav_bert_layer_{fwd,bwd}).  ONE call enqueues every kernel of a stage on the caller's
 * stream(s) -- the same kernels, in the same order and with the same arguments as the per-kernel entries above would be called by the
 * host layer (lavender_amd/engine.py), so results are bit-identical; what it removes is ~20 host -> C transitions and their argument
 * marshalling per stage.  All buffers are the caller's (nothing is allocated here); NULL for an optional buffer means "not wanted".
 *
 * One post-LN BertLayer of the fusion encoder (HF BertLayer as called from model.py:242), fp32 residual stream:
 *   qkv = x Wqkv^T + b;  cx = attention(qkv, key_mask, dropout p_attn);  pre1 = res + dropout(cx Wao^T + b);  x1 = LN1(pre1);
 *   h = gelu(x1 Wff1^T + b) (+ stored GELU');  pre2 = x1_f32 + dropout(h Wff2^T + b);  y = LN2(pre2)
 * where `res` is the bf16 input x (first layer) or LayerNorm(res_pre) recomputed from the producing layer's saved pre-LN rows
 * (res_pre / res_mean / res_rstd / res_gamma / res_beta, see lav_gemm_epilogue.res_ln_*), and x1_f32 = LayerNorm(pre1) likewise.
 */
typedef struct lav_bert_layer_desc {
    int n_seq, L, hidden, heads, ffn;
    float p_hidden, p_attn, ln_eps;
    uint32_t seed_attn, seed1, seed2;
    int causal_from;
    const int32_t* key_mask;
    /* parameters: bf16 working copies of the matrices, fp32 vectors */
    const void* w_qkv; const float* b_qkv;               /* fused (3 hidden, hidden) */
    const void* w_ao; const float* b_ao; const float* ln1_gamma; const float* ln1_beta;
    const void* w_ff1; const float* b_ff1;
    const void* w_ff2; const float* b_ff2; const float* ln2_gamma; const float* ln2_beta;
    /* input */
    const void* x;                                         /* bf16 (rows, hidden), rows = n_seq * L */
    const void* res_pre; const float* res_mean; const float* res_rstd; const float* res_gamma; const float* res_beta;   /* or all NULL */
    /* outputs / activations kept for the backward (lse, h_pre: NULL in a forward that will not be differentiated) */
    void* qkv; void* cx; float* lse; void* pre1; float* mean1; float* rstd1; void* x1; void* h_pre; void* h;
    void* pre2; float* mean2; float* rstd2; void* y;
    int stream_f16;                                        /* 0: res_pre / pre1 / pre2 (the pre-LayerNorm residual stream) are fp32 rows; 1: fp16 rows */
    float ln2_eps;                                         /* (ABI 7) eps of the output LayerNorm (ln2_*); 0 = the same as ln_eps, which then serves both */
} lav_bert_layer_desc;
int lav_bert_layer_fwd(void* stream, const lav_bert_layer_desc* d);

/* Backward of the same layer.  side_stream (may equal stream, or NULL = stream): the four weight-gradient GEMMs are enqueued there,
 * each ordered after its operands' producers on `stream` by an event; the caller joins side_stream before it reads the gradients and
 * keeps their operands (d_dense2, h, dh, x1, d_dense1, cx, dqkv, x) alive until then. */
typedef struct lav_bert_layer_bwd_desc {
    lav_bert_layer_desc f;                                 /* the forward's descriptor (saved activations, parameters, seeds) */
    const void* dy;                                        /* bf16 (rows, hidden) */
    const void* wt_qkv; const void* wt_ao; const void* wt_ff1; const void* wt_ff2;   /* transposed bf16 copies (in, out) */
    long ldt_qkv, ldt_ao, ldt_ff1, ldt_ff2;                /* their row pitches */
    /* fp32 gradient accumulators */
    float* g_w_qkv; float* g_b_qkv; float* g_w_ao; float* g_b_ao; float* g_ln1_gamma; float* g_ln1_beta;
    float* g_w_ff1; float* g_b_ff1; float* g_w_ff2; float* g_b_ff2; float* g_ln2_gamma; float* g_ln2_beta;
    int splits_qkv, splits_ao, splits_ff1, splits_ff2;     /* split-K factors of the weight-gradient GEMMs */
    /* temporaries (bf16) and the result */
    void* d_pre2; void* d_dense2; void* dh; void* d_x1; void* d_pre1; void* d_dense1; void* d_cx; void* dqkv;
    void* dx;                                              /* bf16 (rows, hidden) */
    int group_splits;                                      /* > 0: the four weight-gradient GEMMs run as ONE grouped launch (lav_gemm_tn_grouped) with this split
                                                              factor, issued when the last of their operands (dqkv) exists; splits_* are then the fallback factors */
    int assign_mask;                                       /* (ABI 7) bit 0 / 1 / 2 / 3: g_w_ff2 / g_w_ff1 / g_w_ao / g_w_qkv is ASSIGNED by this call (first writer of the step), not accumulated into */
} lav_bert_layer_bwd_desc;
int lav_bert_layer_bwd(void* stream, void* side_stream, const lav_bert_layer_bwd_desc* d);

/* One SwinTransformerBlock3D (video_swin.py:204-261) on (rows, C) channels-last tokens whose grid is a multiple of the window (the zero-pad
 * branches stay with the per-kernel entries):
 *   y1 = LN1(x);  qkv = y1 Wqkv^T + b;  ao = window_attention(qkv);  x_mid = x + s_attn * (ao Wproj^T + b);
 *   y2 = LN2(x_mid);  h = gelu(y2 Wfc1^T + b) (+ stored GELU');  out = x_mid + s_mlp * (h Wfc2^T + b)
 * s_* = per-sample stochastic-depth factors (dp_attn / dp_mlp, fp32 [rows / rows_per_group], or NULL).  `attn` is the window descriptor
 * the caller prepared (token tables, bias fragments: lav_attention_build_bias already enqueued on `stream`). */
typedef struct lav_swin_block_desc {
    int rows, C, heads, rows_per_group;
    int qkv_headmajor;
    float ln_eps;
    const lav_attn_desc* attn;
    const float* ln1_gamma; const float* ln1_beta; const void* w_qkv; const float* b_qkv; const void* w_proj; const float* b_proj;
    const float* ln2_gamma; const float* ln2_beta; const void* w_fc1; const float* b_fc1; const void* w_fc2; const float* b_fc2;
    const float* dp_attn; const float* dp_mlp;
    const void* x;                                         /* bf16 (rows, C) */
    /* outputs / activations kept for the backward (mean*, rstd*, lse, h_pre: NULL in a forward that will not be differentiated) */
    void* y1; float* mean1; float* rstd1; void* qkv; void* ao; float* lse; void* x_mid; void* y2; float* mean2; float* rstd2;
    void* h_pre; void* h; void* out;
} lav_swin_block_desc;
int lav_swin_block_fwd(void* stream, const lav_swin_block_desc* d);

typedef struct lav_swin_block_bwd_desc {
    lav_swin_block_desc f;
    const void* dy;                                        /* bf16 (rows, C) */
    float alpha_attn, alpha_mlp;                           /* 1 / keep probability of the two stochastic-depth branches (1 without drop-path) */
    const void* wt_qkv; const void* wt_proj; const void* wt_fc1; const void* wt_fc2;
    long ldt_qkv, ldt_proj, ldt_fc1, ldt_fc2;
    float* g_ln1_gamma; float* g_ln1_beta; float* g_w_qkv; float* g_b_qkv; float* g_bias_table; float* g_w_proj; float* g_b_proj;
    float* g_ln2_gamma; float* g_ln2_beta; float* g_w_fc1; float* g_b_fc1; float* g_w_fc2; float* g_b_fc2;
    int splits_qkv, splits_proj, splits_fc1, splits_fc2;
    void* dh; void* d_y2; void* d_mid; void* d_ao; void* dqkv; void* d_y1;     /* temporaries, bf16 */
    void* dx;                                              /* bf16 (rows, C) */
    int group_splits;                                      /* as lav_bert_layer_bwd_desc.group_splits */
    int assign_mask;                                       /* (ABI 7) bit 0 / 1 / 2 / 3: g_w_fc2 / g_w_fc1 / g_w_proj / g_w_qkv is assigned, not accumulated into */
} lav_swin_block_bwd_desc;
/* side_stream as in lav_bert_layer_bwd; the relative-position-bias-table gradient runs there too when lav_attention_bias_split(attn). */
int lav_swin_block_bwd(void* stream, void* side_stream, const lav_swin_block_bwd_desc* d);

/* ---------------------------------------------------------------------------------------------
 * Caption decoding with a key / value cache (csrc/decode.hip; LAVENDER_Captioning.generate, model_for_captioning.py:139-500).  Eval only:
 * no dropout, nothing kept for a backward, no atomics (two runs give the same bits).  Nothing is allocated or synchronised: the caller
 * owns the cache and every workspace.
 *
 * Skinny GEMM: out[M, N] = x[M, K] . W[N, K]^T (+ bias[N]) for 1 <= M <= 64, K a multiple of 32, 16-byte aligned rows.  epi:
 *   LAV_SKINNY_BF16     bf16 out
 *   LAV_SKINNY_GELU     bf16 out = gelu(v) (the exact-erf GELU of the fusion GEMM epilogue)
 *   LAV_SKINNY_RES_F32  fp32 out = v + residual (fp32 rows, or bf16 rows when residual_bf16) -- the post-LN residual adds
 *   LAV_SKINNY_F32      fp32 out (the MLM decoder logits)
 * lav_gemm_bf16's tile selection is not affected. */
#define LAV_SKINNY_BF16 0
#define LAV_SKINNY_GELU 1
#define LAV_SKINNY_RES_F32 2
#define LAV_SKINNY_F32 3
int lav_gemm_skinny_bf16(void* stream, int M, int N, int K, const void* x, long ldx, const void* w, long ldw, const float* bias, int epi,
                         const void* residual, long ldr, int residual_bf16, void* out, long ldo);

/* Decode attention, head_dim 64, q_len <= 8 new query rows per (clip, head).  The keys of clip b are, in order:
 *   [0, Lv)                  video rows read in place from the prefix pass's qkv buffer (row b * Lv + i, stride ld_prefix = 3 hidden),
 *                            visible where key_mask[b, i] != 0 (key_mask may be NULL: all visible)
 *   [Lv, Lv + n_cached)      the text cache (B, heads, max_len, 64) bf16, cache_k / cache_v: visible to every new row
 *   the q_len new rows       their own k / v in qkv_new (row b * q_len + j, stride ld_new): new key j is visible to new rows >= j
 * out (row b * q_len + j, column head * 64 + d, stride ldo) = softmax(q k^T * scale) v in fp32, stored bf16.  The same launch writes the k / v
 * of new rows 0 .. n_append - 1 to cache positions n_cached .. n_cached + n_append - 1.  When B * heads is below the CU count the keys are
 * split over lav_attention_decode_splits(d) workgroups per (clip, head), combined by a second launch in split order: `partials` then needs
 * B * heads * splits * q_len * 66 floats, and `partials_capacity` states how many it holds (a smaller workspace fails with LAV_E_WORKSPACE
 * before anything is launched).  The split count never decreases as n_cached grows: a workspace sized for the last step covers every step. */
typedef struct lav_attn_decode_desc {
    int B, heads, head_dim, q_len, Lv, n_cached, n_append, max_len;
    float scale;
    const void* prefix_qkv; long ld_prefix; const int32_t* key_mask;
    const void* qkv_new; long ld_new;
    void* cache_k; void* cache_v;
    void* out; long ldo;
    float* partials; long partials_capacity;               /* workspace of the key splits and its size in floats */
} lav_attn_decode_desc;
int lav_attention_decode_splits(const lav_attn_decode_desc* d);
int lav_attention_decode(void* stream, const lav_attn_decode_desc* d);

/* BERT embeddings of n single rows with explicit positions (eval: no dropout): word[ids[r]] + pos[pos_ids[r]] + type0 -> LayerNorm(eps) -> bf16
 * (n, Hd), Hd <= 1024.  lav_text_embed_fwd hard-wires positions 0 .. X - 1. */
int lav_text_embed_rows_fwd(void* stream, int n, int Hd, const int64_t* ids, const int32_t* pos_ids, const float* word, const float* pos,
                            const float* type0, const float* gamma, const float* beta, float eps, void* out);

/* One greedy decoding step over fp32 logits (B, V) with row pitch ld, one workgroup per row (model_for_captioning.py:430-480):
 *   penalty != 1: every distinct id of ids[b, 0 .. cur) scales its logit IN PLACE (x * penalty if x < 0, else x / penalty);
 *   tok = argmax (lowest index on a tie), score = log_softmax(logits)[tok];
 *   u = unfinished[b]: ids[b, cur] = u ? tok : pad_id (also written to next_ids[b * ld_next] when next_ids is not NULL),
 *   score_sum[b] += u ? score : 0, count[b] += u, unfinished[b] = u && ids[b, cur] != eos_id. */
int lav_greedy_step(void* stream, int B, int V, float* logits, long ld, int64_t* ids, long ld_ids, int cur, float penalty, int32_t* unfinished,
                    float* score_sum, float* count, int64_t pad_id, int64_t eos_id, int64_t* next_ids, long ld_next);

/* Stage-level entry of the decode path: one post-LN BertLayer (the arithmetic of lav_bert_layer_fwd, eval) over the q_len new rows of
 * every clip (rows = B * q_len, row b * q_len + j), with the attention of lav_attention_decode:
 *   qkv = x Wqkv^T + b;  cx = decode_attention(qkv);  pre1 = res + cx Wao^T + b;  x1 = LN1(pre1);  h = gelu(x1 Wff1^T + b);
 *   pre2 = x1 + h Wff2^T + b;  y = LN2(pre2)
 * `res` is x_res (fp32 rows, or bf16 when x_res_bf16: the embeddings in front of the first layer).  pre1, pre2, x1_32 and y32 are fp32
 * (rows, hidden); y32 is the next layer's residual.  ln_stats: 2 * rows floats of scratch.  rows = B * q_len <= 64 (the skinny GEMM's limit:
 * LAVENDER_Captioning.generate decodes larger batches in chunks of 32 clips). */
typedef struct lav_bert_layer_decode_desc {
    int B, q_len, hidden, heads, ffn, Lv, n_cached, n_append, max_len;
    float ln_eps, ln2_eps;
    const int32_t* key_mask;
    const void* w_qkv; const float* b_qkv;
    const void* w_ao; const float* b_ao; const float* ln1_gamma; const float* ln1_beta;
    const void* w_ff1; const float* b_ff1;
    const void* w_ff2; const float* b_ff2; const float* ln2_gamma; const float* ln2_beta;
    const void* prefix_qkv;                                /* this layer's qkv of the video rows, (B * Lv, 3 hidden) bf16 */
    void* cache_k; void* cache_v;                          /* this layer's text cache, (B, heads, max_len, 64) bf16 each */
    const void* x;                                         /* bf16 (rows, hidden) */
    const void* x_res; int x_res_bf16;
    void* qkv; void* cx; float* pre1; void* x1; float* x1_32; void* h; float* pre2; float* ln_stats;
    void* y; float* y32;                                   /* outputs: bf16 (next GEMM operand) and fp32 (next residual) */
    float* attn_partials; long attn_partials_capacity;     /* lav_attention_decode's partials and their size in floats (NULL, 0 when it needs none) */
} lav_bert_layer_decode_desc;
int lav_bert_layer_decode(void* stream, const lav_bert_layer_decode_desc* d);

/* ---------------------------------------------------------------------------------------------
 * Beam search on the cached decoder (csrc/decode.hip; Oscar / SwinBERT's _generate_beam_search + BeamHypotheses, HF 2.x).  The rows of a
 * step are beams x clips, row r = clip * beams + beam.  Everything stays on the device: a whole generation needs no host synchronisation.
 *
 * lav_attention_decode_beam / lav_bert_layer_decode_beam: lav_attention_decode / lav_bert_layer_decode with d->B = clips * beams row groups
 * (text cache, new rows and outputs per row group) whose video keys [0, Lv) and key mask are those of clip b / beams, read in place from a
 * prefix pass over the clips alone (prefix_qkv (clips * Lv, 3 hidden), key_mask (clips, Lv)).  beams 1 is the plain entry, bit for bit. */
#define LAV_BEAM_MAX 8
int lav_attention_decode_beam(void* stream, const lav_attn_decode_desc* d, int beams);
int lav_bert_layer_decode_beam(void* stream, const lav_bert_layer_decode_desc* d, int beams);

/* Beam step, one workgroup per row of fp32 logits (rows, V), row pitch ld, in one pass over the row:
 *   penalty != 1: every distinct id of ids[r, 0 .. cur) scales its logit IN PLACE (the rule of lav_greedy_step);
 *   the row's top 2 * beams logits (value descending, lower index on a tie) and its log-sum-exp;
 *   cand_score[r, j] = log_softmax(row)[word] + beam_scores[r], cand_word[r, j] = word  (rows, 2 * beams) fp32 / int32. */
int lav_beam_step(void* stream, int rows, int beams, int V, float* logits, long ld, const int64_t* ids, long ld_ids, int cur, float penalty,
                  const float* beam_scores, float* cand_score, int32_t* cand_word);

/* Beam select, one workgroup per clip, for step cur (1 <= cur < max_len).  The clip's beams * 2 * beams candidates of lav_beam_step are
 * ordered by score descending, flat index beam * V + word ascending on a tie; the first 2 * beams are the clip's candidates.  Then:
 *   a clip not done becomes done when it holds `keep` hypotheses and early_stopping, or worst >= best candidate / max_norm;
 *   a clip not done walks its candidates: a [SEP] word (eos_id), or any word when cur + 1 == max_len, offers the hypothesis (the parent's
 *   ids [0, cur), normalised score s = score / cur_norm), kept while fewer than `keep` are held or when s > worst; on overflow the lowest s
 *   goes (the earliest insertion among equals) and worst is the new minimum, a plain add sets worst = min(worst, s); any other word is a
 *   next beam (parent, word, score); the walk stops at `beams` next beams;
 *   beams of a done clip (and the unfilled ones of the last step) keep their row, score and ids and get [PAD] (pad_id).
 * Writes ids[r, 0 .. cur) (gathered from the parent) and ids[r, cur] = word, next_ids[r * ld_next] = word (when not NULL), parent[r] (global
 * row), beam_scores[r]; a kept hypothesis row of hyp_ids (clips, keep, max_len) is the parent's ids, [SEP], then [PAD], with hyp_score (clips,
 * keep), hyp_seq (its insertion number), state (clips, 3) int32 = (held, done, insertions so far) and worst (clips).  Start state: beam
 * scores 0 for beam 0 and -1e9 for the others, state 0, worst 1e9.  cur_norm = cur ** length_penalty and max_norm = max_len ** length_penalty
 * (fp32; the divisions are IEEE fp32). */
typedef struct lav_beam_select_desc {
    int clips, beams, keep, V, cur, max_len, early_stopping;
    float cur_norm, max_norm;
    int64_t eos_id, pad_id;
    const float* cand_score; const int32_t* cand_word;     /* (clips * beams, 2 * beams) */
    float* beam_scores;                                    /* (clips * beams) */
    int64_t* ids; long ld_ids;                             /* (clips * beams, >= max_len) */
    int64_t* next_ids; long ld_next;
    int32_t* parent;                                       /* (clips * beams) */
    int64_t* hyp_ids; float* hyp_score; int32_t* hyp_seq; int32_t* state; float* worst;
} lav_beam_select_desc;
int lav_beam_select(void* stream, const lav_beam_select_desc* d);

/* Re-parenting of the text caches of every layer in one launch: dst_x[l][r, h, 0 .. n_pos) = src_x[l][parent[r], h, 0 .. n_pos) for x = k, v,
 * caches (rows, heads, max_len, 64) bf16, 16-byte aligned.  A parent outside [0, rows) copies the row itself. */
#define LAV_REPARENT_MAX_LAYERS 24
typedef struct lav_beam_reparent_desc {
    int layers, rows, heads, n_pos, max_len;
    const int32_t* parent;
    const void* src_k[LAV_REPARENT_MAX_LAYERS]; const void* src_v[LAV_REPARENT_MAX_LAYERS];
    void* dst_k[LAV_REPARENT_MAX_LAYERS]; void* dst_v[LAV_REPARENT_MAX_LAYERS];
} lav_beam_reparent_desc;
int lav_beam_reparent(void* stream, const lav_beam_reparent_desc* d);

/* ---------------------------------------------------------------------------------------------
 * Text-to-video retrieval evaluation (csrc/retrieval.hip, csrc/stages.cpp; eval_retrieval_mlm.py:138-247, eval only: no dropout, no atomics,
 * two runs give identical bits).  Every (caption, video) pair runs the fusion encoder and the MLM head, and only the appended [MASK] row of
 * the last layer and two vocabulary columns reach its score p_true / (p_true + p_false): the last layer runs everything after its QKV GEMM
 * on that one row per pair, and the head reads out two decoder rows instead of the full vocabulary.  (ABI 7, additive.)
 *
 * lav_attention_rows: out[s] (bf16, row pitch ldo) = softmax(q_s K_s^T * scale + mask) V_s per head, where q_s is row q_row[s] of sequence s
 * of the (n * L, ldq >= 3 * heads * 64) qkv rows of the full-width QKV GEMM and K_s / V_s are all L rows of that sequence; key_mask (n, L)
 * int32 as lav_pair_key_mask builds it.  head_dim 64, L <= 4096, fp32 softmax.  A q_row outside [0, L) gives a zero row; a row whose keys are
 * all masked gives a zero row. */
int lav_attention_rows(void* stream, int n, int L, int heads, int head_dim, const void* qkv, long ldq, const int32_t* key_mask,
                       const int32_t* q_row, float scale, void* out, long ldo);

/* lav_bert_layer_fwd_rows: lav_bert_layer_fwd at eval with every step after the QKV GEMM restricted to the n_seq selected rows (row q_row[s] of
 * sequence s):  qkv = x Wqkv^T + b over all n_seq * L rows (x read through x_rowmap when given: lav_gemm_epilogue.a_rowmap);
 * cx = lav_attention_rows(qkv);  pre1 = res + cx Wao^T + b;  x1 = LN1(pre1);  h = gelu(x1 Wff1^T + b);  pre2 = x1 + h Wff2^T + b;  y = LN2(pre2).
 * `res` row s is row res_rowmap[s] of the residual the layer would read in full: bf16 (res_dtype 0: the embeddings, or the un-expanded pair
 * source), fp32 (1) or fp16 (2) rows, with res_mean / res_rstd / res_gamma / res_beta when those rows are the PRE-LayerNorm rows of the
 * producing layer (lav_gemm_epilogue.res_ln_*).  pre1 / pre2 / y32 are fp32 (n_seq, hidden); mean* / rstd* are n_seq floats (mean2 / rstd2 may
 * be NULL); every buffer is the caller's. */
typedef struct lav_bert_layer_rows_desc {
    int n_seq, L, hidden, heads, ffn;
    float ln_eps, ln2_eps;                                 /* ln2_eps 0: the same as ln_eps */
    const int32_t* key_mask;                               /* (n_seq, L) */
    const int32_t* q_row;                                  /* (n_seq) */
    const void* w_qkv; const float* b_qkv;
    const void* w_ao; const float* b_ao; const float* ln1_gamma; const float* ln1_beta;
    const void* w_ff1; const float* b_ff1;
    const void* w_ff2; const float* b_ff2; const float* ln2_gamma; const float* ln2_beta;
    const void* x; const int32_t* x_rowmap;                /* bf16 rows, (n_seq * L) of them or read through x_rowmap (int32 [n_seq * L]) */
    const void* res; long ldr; int res_dtype; const int32_t* res_rowmap;   /* res_rowmap: int32 [n_seq], required */
    const float* res_mean; const float* res_rstd; const float* res_gamma; const float* res_beta;   /* or all NULL */
    void* qkv;                                             /* bf16 (n_seq * L, 3 hidden) */
    void* cx; float* pre1; float* mean1; float* rstd1; void* x1; void* h; float* pre2; float* mean2; float* rstd2;
    void* y; float* y32;                                   /* outputs: bf16 and fp32 (n_seq, hidden) */
} lav_bert_layer_rows_desc;
int lav_bert_layer_fwd_rows(void* stream, const lav_bert_layer_rows_desc* d);

/* lav_mlm_pair_readout: the MLM head (BertOnlyMLMHead) on n rows, read out at two vocabulary entries.  t = gelu(x Wt^T + b) (fp32, the tile GEMM
 * with the GELU epilogue, into the caller's (n, hidden) scratch), then per row in fp32: LayerNorm(t) (ln_eps), p_true / p_false = its dot products
 * with rows true_id / false_id of the decoder weight + the tied bias, s = p_true / (p_true + p_false) (raw logits, no softmax).  s goes to
 * scores[out_row[k] * ld_scores + out_col[k]] (entries outside score_rows x score_cols are skipped), (p_true, p_false) to logits (n, 2) when given. */
typedef struct lav_mlm_pair_readout_desc {
    int n, hidden, vocab, true_id, false_id;
    float ln_eps;
    const void* x; long ldx;                               /* bf16 (n, hidden) */
    const void* w_dense; const float* b_dense;             /* transform dense (hidden, hidden) bf16 / fp32 */
    const float* ln_gamma; const float* ln_beta;
    const void* w_dec; long ldw_dec; const float* b_dec;   /* decoder weight (vocab, ldw_dec) bf16 and its (tied) bias */
    float* t;                                              /* scratch fp32 (n, hidden) */
    const int32_t* out_row; const int32_t* out_col;        /* (n) */
    float* scores; long ld_scores; int score_rows, score_cols;
    float* logits;                                         /* (n, 2) fp32 or NULL */
} lav_mlm_pair_readout_desc;
int lav_mlm_pair_readout(void* stream, const lav_mlm_pair_readout_desc* d);

/* lav_retrieval_rank: out[t] = 1-based position of column gt[t] when the columns of row t of S (n_text, ldS) fp32 are sorted by score descending,
 * stably in column order (eval_retrieval_mlm.py:223-227): 1 + #{v : S[t,v] > S[t,gt]} + #{v < gt : S[t,v] == S[t,gt]}.  NaN sorts after every
 * number and NaNs keep their column order.  A gt outside [0, n_video) gives 0.  One workgroup per row. */
int lav_retrieval_rank(void* stream, int n_text, int n_video, const float* S, long ldS, const int32_t* gt, int32_t* out);

/* lav_answer_readout: the video-QA read-out of n logit rows of width V (logits (n, ld), ld >= V; dtype 0 = bf16, 1 = fp32), one pass per row
 * (csrc/qa.hip).  Order of the columns of a row: value descending, a NaN above every number (the order of torch.topk / torch.argmax), the LOWER
 * index first among equal values (-0 = +0) and among NaNs.
 *   pred[r]    the first column in that order (arg-max, lowest index on a tie)
 *   rank[r]    number of columns before column labels[r] in that order: #{c : x_c > x_t, or x_c == x_t and c < t}; -1 where labels[r] == -1.
 *              A top-k hit is 0 <= rank < k (main_qaoe_mlm_lsmdc_fib.py:115-126; torch.topk leaves the order of ties open, this rule fixes it)
 *   choice[r]  arg-max over c < n_cand of x[cand[c]] / sum_c x[cand[c]] (main_qamc_mlm.py:159-166: RAW logits, so a negative sum reverses the
 *              order); the sum and the quotients are fp32, the sum runs in candidate order, the first index wins a tie, a NaN quotient is
 *              above every number; -1 when n_cand == 0
 * labels (n) int32 on the device; labels_host: the same values in host memory or NULL -- when given, a label outside [0, V) other than -1 is
 * rejected (without it the caller vouches for them; the kernel reads no column outside the row either way and treats such a label as -1).
 * cand_host: n_cand <= LAV_ANSWER_MAX_CAND token ids in HOST memory (they travel as a kernel argument), each in [0, V).  pred / rank / choice:
 * caller-owned (n) int32 on the device.
 * splits (1 .. LAV_ANSWER_MAX_SPLITS): each row is cut into that many column ranges, one workgroup each; for splits > 1 a second launch merges
 * the partials held in `workspace` (device, 8-byte aligned, >= lav_answer_readout_workspace_bytes(n, splits) bytes, else LAV_E_WORKSPACE).
 * Counts are integers and the best column an integer max, so every split count gives identical outputs.  No atomics, no allocation, no
 * synchronisation.  A rejected call launches nothing. */
#define LAV_ANSWER_MAX_CAND 32
#define LAV_ANSWER_MAX_SPLITS 16
size_t lav_answer_readout_workspace_bytes(int n, int splits);
int lav_answer_readout(void* stream, int n, int V, const void* logits, long ld, int dtype, const int32_t* labels, const int32_t* labels_host,
                       const int32_t* cand_host, int n_cand, int splits, void* workspace, size_t workspace_bytes, int32_t* pred, int32_t* rank,
                       int32_t* choice);

/* lav_match_readout: the in-batch matching read-out of the MLM retrieval callers (main_retrieval_mlm.py:107-118, main_retmc_mlm.py:129-140): G groups
 * of O candidates, candidate k = g * O + o.  t = logits[row[k], true_col], f = logits[row[k], false_col] (logits (n_rows, ld); dtype 0 = bf16,
 * 1 = fp32; row == NULL means row[k] = k), both widened to fp32, s = t / (t + f) in fp32 on the RAW logits as the reference has it.
 *   score[k]   s, when score is given; every NaN is stored as the one pattern 0x7fc00000
 *   choice[g]  arg-max of s over o in the order of lav_answer_readout's choice: a NaN above every number, -0 = +0, the LOWEST o first among equal
 *              values and among NaNs
 *   hit[g]     choice[g] == gt[g], when hit is given (then gt must be); 0 where gt[g] lies outside [0, O)
 * A row[k] outside [0, n_rows) reads nothing and its candidate scores "NaN-last": score[k] is that NaN pattern, but in the order it stands BELOW
 * every number and below a NaN quotient (lowest o first among such candidates).  This is the one place where the order has a fourth class: a
 * candidate that was not read must never win against one that was.  hip.match_readout rejects such an entry of a host row array instead.
 * The same entry serves the (n, 2) fp32 block of lav_mlm_pair_readout (ld = 2, columns 0 / 1, row = NULL) and the reference's formulation (the
 * bf16 (pairs * X, ld) logits, row[k] = the [MASK] row of pair k, columns = the "true" / "false" token ids).
 * Rejected before any launch: G < 1, O < 1, a column outside [0, ld), dtype not 0 / 1, row == NULL with n_rows < G * O, hit without gt.
 * One wave per group, lanes stride over o, the max is taken over the (key, ~o) integer word: identical results for every O and lane mapping; groups
 * are walked with a grid-stride loop (any G).  No atomics, no workspace, no allocation, no synchronisation. */
int lav_match_readout(void* stream, int G, int O, const void* logits, long ld, int dtype, const int32_t* row, long n_rows, int true_col,
                      int false_col, const int32_t* gt, float* score, int32_t* choice, int32_t* hit);

/* ---------------------------------------------------------------------------------------------
 * Process-wide probe switches: environment variables read ONCE by the library on first use (not part of the contract; every setting
 * computes the same results up to fp32 summation order unless stated).  They exist so that tools/ and profiles/ can A/B a kernel
 * choice on one box.
 *   LAV_GEMM_TN_KIND (0 / 1: weight-gradient tiles of at most 128x128 / 256x128), LAV_GEMM_PP_TN (0: no ping-pong 256x256
 *   weight-gradient kernel), LAV_GEMM_TN_MINM (fewest output rows for the 256-row weight-gradient tiles, default 160),
 *   LAV_GEMM_TN_GROUP (0: grouped weight-gradient launches run job by job), LAV_TN_BLOCKS / LAV_TN_GROUP_BLOCKS / LAV_TN_GROUP_BLOCKS_WIDE (workgroups the
 *   split-K policy aims one weight-gradient GEMM / a grouped launch / a grouped launch of >= 96 tiles at: 128 / 192 / as the one before), LAV_GEMM_GROUP_N (column-group width of the 256x256 tile
 *   walk), LAV_GEMM_H192 / LAV_GEMM_H192L (0: no 192-row tiles / no loader waves), LAV_GEMM_PS (bit 0 / bit 1: phase-shifted two-group form of
 *   the 256-row / 192-row tile, default 3), LAV_NT_STORES (read twice, with different defaults: by the GEMM epilogue, default 5 -- bit 0: GELU'
 *   stored non-temporally, bit 2: loaded non-temporally; by lav_adamw_step, default 1 -- bit 1: non-temporal parameter / moment
 *   stores), LAV_GEMM_DBG (timing ablations of the 256x256 kernel: WRONG results),
 *   LAV_LN_ATOMIC_FLUSH (LayerNorm backward column sums by per-block atomics), LAV_LN_G32 (bit 0 / bit 1: 32-lane x 3-chunk rows for C = 768 in the
 *   forward / backward, default 1), LAV_WINL / LAV_SEQL (0: large windows / long sequences on the generic kernels).
 * lav_gemm_select(which, value) changes these GEMM ones at run time (same caveat: process-wide, for probes): 2 = LAV_GEMM_PP_TN, 5 = LAV_GEMM_DBG,
 * 6 = LAV_GEMM_GROUP_N, 7 = LAV_GEMM_H192, 9 = LAV_GEMM_H192L, 11 = LAV_GEMM_PS, 12 = LAV_GEMM_TN_MINM, 13 = LAV_GEMM_TN_GROUP; the others (LAV_GEMM_TN_KIND,
 * LAV_TN_BLOCKS, LAV_TN_GROUP_BLOCKS, LAV_TN_GROUP_BLOCKS_WIDE, LAV_NT_STORES) are fixed when the library is loaded.
 * lav_probe_win_prof(buf): NULL = off; else the next stage-2-sized window backward runs the s_memtime-stamped build of win_bwd1 and
 * writes 160 uint64 stamps to the device buffer `buf` (tools/win_prof.py; profiles/r05_win_bwd1.md).
 * --------------------------------------------------------------------------------------------- */
void lav_probe_win_prof(void* buf);

#ifdef __cplusplus
}
#endif
#endif
