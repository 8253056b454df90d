/* rgbnm.h -- C ABI of librgbnm.so: the MI355X (gfx950) hot path of RGB-no-more.
 *
 * Drop-in boundary.  The reference has no native FFI for this path except
 * dct_manip (pybind11); everything else is PyTorch ops reached from Python, so the binding a maintainer
 * adds is a ctypes stub.  Each entry point below names the reference code it
 * replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - plain pointers + sizes; device pointers unless the name says host; no C++/torch types.
 *   - returns 0 on success, negative RGBNM_E* otherwise; never throws; never allocates device memory;
 *     keeps no per-call state; all work is enqueued on `stream` (a hipStream_t passed as void*), no sync.
 *   - dtype: 0 = fp32 ("strict" mode, exact-fp32 MFMA), 1 = bf16 (fp32 accumulate), 2 = fp16 (IEEE half, fp32
 *     accumulate; conversions round to nearest even and overflow to +-inf, like torch's .half()).  Activations and
 *     MFMA operands use that type; parameters, gradients, statistics and optimizer state are fp32.
 *     RGBNM_DT_F16 is accepted by: rgbnm_gemm_nt, rgbnm_gemm_tn, rgbnm_prep_weights[_chain] (without chain images),
 *     rgbnm_layernorm_fwd / _bwd, rgbnm_head_pool_fwd / _bwd, rgbnm_attention_fwd / _bwd, rgbnm_subblock_embed[_mix]
 *     (out_dtype; in_dtype fp32 / bf16 / fp16 with an fp16 output), rgbnm_softxent / _grad / _grad_mix (dl_dtype) and,
 *     through rgbnm_vit_cfg.dtype, the ViT composites (patch embedding, blocks, head); and SwinV2's own entries:
 *     rgbnm_window_attention_fwd / _bwd, rgbnm_swin_embed (out_dtype fp16 from any in_dtype; in_dtype fp16 to any
 *     out_dtype), rgbnm_ln_generic_fwd / _bwd, rgbnm_merge_gather and rgbnm_token_mean.  By default they run the generic
 *     kernels.  With the option "f16_tuned" set, rgbnm_gemm_nt and rgbnm_gemm_tn (and every composite that calls them) take
 *     fp16 through the plain GEMM kernels tuned for 16-bit operands, at the shapes where bf16 takes them: the small-M kernel
 *     (none / tanh / dtanh), the weight-resident and the k-pipelined row-panel kernels (none / residual / GELU with the erf
 *     arithmetic / dGELU), the pipelined and wide weight-gradient kernels, and the rgbnm_gemm_tn_group_* brackets (a queue holds
 *     jobs of one dtype: a job of another dtype runs what is queued first).  At "f16_tuned" >= 2 fp16 also takes the per-block fused
 *     kernels where bf16 takes them: attention v2 (rgbnm_attention_fwd / _bwd, N <= 224), the fused MLP forward / backward and the
 *     LayerNorm-chained row-panel epilogues (rgbnm_vit_block_fwd[_chain] / _bwd, rgbnm_vit_ln_chain; E = 192, >= 8192 rows), with
 *     the erf arithmetic for GELU.  The one-launch chains and the bf16 GELU table are bf16 only and are skipped for fp16 whatever
 *     the option says.  The data stage has fp16 through entries of its own: rgbnm_dct_augment_chain writes it
 *     (RGBNM_AUG_OUT_F16) and rgbnm_mixup_any mixes to it; the three rgbnm_dct_augment* entries and rgbnm_mixup keep to fp32 / bf16.
 *   - tensors are dense row-major; "ld*" are row strides in elements.
 */
#ifndef RGBNM_H
#define RGBNM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGBNM_ABI_VERSION 3
#define RGBNM_DT_F32 0
#define RGBNM_DT_BF16 1
#define RGBNM_DT_F16 2   /* see the list of entries above */
#define RGBNM_DT_I16 2   /* only as out_dtype of rgbnm_dct_augment[_ex / _packed]; their fp16 output is rgbnm_dct_augment_chain's
                            RGBNM_AUG_OUT_F16, a code of its own because 2 is taken here */

/* epilogues of rgbnm_gemm_nt */
#define RGBNM_EPI_NONE 0   /* C = A.W^T (+bias)                                         */
#define RGBNM_EPI_RES 1    /* C = A.W^T + bias + R            (ResidualAdd, plainvit.py:475-479)       */
#define RGBNM_EPI_GELU 2   /* u = A.W^T + bias ; C = gelu_erf(u), C2 = gelu_erf'(u)  (FeedForwardBlock :487-488) */
#define RGBNM_EPI_POS 3    /* C = A.W^T + bias + pos[row % period]      (SinCosEmbedding :97-121)      */
#define RGBNM_EPI_DGELU 4  /* C = (A.W^T) * R, R = the C2 (gelu') saved by RGBNM_EPI_GELU         */
#define RGBNM_EPI_TANH 5   /* C = tanh(A.W^T + bias)                    (ClassificationHead :553-554)  */
#define RGBNM_EPI_DTANH 6  /* C = (A.W^T) * (1 - R^2)                                             */
/* dropout epilogues (nn.Dropout after the attention projection, after GELU and after fc2, plainvit.py:485-529): rgbnm_gemm_nt_drop
 * only.  keep / scale as in the dropout mask contract below; the mask is applied to the fp32 value EPI_RES adds to R and to the
 * gelu / gelu' values EPI_GELU stores, so p = 0 gives EPI_RES's / EPI_GELU's bits. */
#define RGBNM_EPI_RES_DROP 7   /* C = R + keep scale (A.W^T + bias)                                         */
#define RGBNM_EPI_GELU_DROP 8  /* u = A.W^T + bias ; C = keep scale gelu_erf(u), C2 = keep scale gelu_erf'(u) */

int rgbnm_abi_version(void);
/* Runtime switches: every one selects between parity-tested kernels (tests/ run both sides); defaults in the middle column.
 * Round 6 removed the switches whose alternative had measured slower in every configuration and nothing else used
 * (tn_square, nt_dmawave, kp_split, nt_kstream, attn_proj -- numbers in DESIGN.md 7).
 *   GEMM  C = A . W^T (nn.Linear forward, dX)
 *   "nt_staged"    1  coalesced LDS-staged epilogue of the generic tile kernel (0: direct fragment stores)
 *   "nt_wres"      1  K = 192 layers on the weight-resident persistent kernel (csrc/gemm_nt_wres.hip)
 *   "nt_kpipe"     1  N % 192 == 0, K >= 256 on the row-panel kernel with the k-tile DMA ring (csrc/gemm_nt_kpipe.hip)
 *   "kp8"          1  ... its 8-wave / 256-row geometry for row counts that are multiples of 256 (the SwinV2 stages)
 *   "kp_persist"   1  ... its persistent form for several column tiles (JPEG-S: E = 384)
 *   "nt_small"     1  at most 512 rows (the classification head) on 32 x 32 tiles with an in-workgroup split of K
 *   "f16_tuned"    0  fp16 on the kernels of nt_small / nt_wres / nt_kpipe / tn_pipe / tn_wide and in the grouped dW launches, as bf16
 *                     (0: fp16 runs the generic tile kernels only, as it did before the option existed: same launches, same bits)
 *                     levels: 0 off | 1 the plain GEMMs above | 2 level 1 plus attention v2 (attn_v2, attn_persist), the fused MLP
 *                     (mlp_fuse, mlp_bwd, mlp_dmast, nt_cold) and the LayerNorm-chained epilogues (ln_fuse) in their fp16 instantiations,
 *                     under the shape conditions of bf16; fp16 GELU is always the erf arithmetic (no table).  Levels 0 and 1 launch
 *                     what they launched before level 2 existed and give the same bits
 *   "ln_fuse"      1  LayerNorm forward / backward in the row-panel kernel's epilogues (E = 192)
 *   GEMM  dW = dY^T . X (weight gradients)
 *   "tn_pipe"      1  pipelined kernel (csrc/gemm_tn_pipe.hip; 0: the generic one)     "tn_tr"  1  its ds_read_b64_tr_b16 fragments
 *   "tn_group"     2  dW GEMMs of a ViT block: 0 one per launch, 1 pairs, 2 all four in one launch
 *   "tn_direct"    1  a grouped launch that ends up without a token split writes dW / db itself (no partial sums, no reduction)
 *   "tn_pack"      1  ... and places its tiles so that no GEMM straddles two XCDs (L2 locality)
 *   "tn_wide"      1  weight-gradient launches whose GEMMs all have No % 192 == 0 and Ki % 384 == 0 (E = 384 and wider) run 192 x 384
 *                     tiles (128 flops per byte taken in instead of 77: the kernel is bound by its intake there, not by HBM)
 *   "tn_wgs"     512  workgroup budget of the generic kernel's token split
 *   attention
 *   "attn_v2"      1  LDS-DMA / transpose-read attention kernels (0: first-generation kernels, also used for 294 tokens)
 *   "attn_persist" 1  persistent forward / backward with a DMA wave (>= 256 (image, head) pairs)
 *   FeedForwardBlock, E = 192
 *   "mlp_fuse"     1  fc1 + GELU + fc2 + residual [+ next LayerNorm] as one launch          "mlp_bwd"  1  its backward data path as one
 *   "mlp_dmast"    1  ... the DMA wave stores the saved-tensor tiles of waves 4-6           "nt_cold"  0  ... non-temporal hint on them
 *   "gelu_table"   1  table GELU in the bf16 kernels once rgbnm_gelu_table_init has run (0: the erf arithmetic; same bits)
 *   the one-launch encoder (E = 192, 3 heads, 196 tokens, bf16)
 *   "fwd_chain"    1  rgbnm_vit_chain_fwd eligible        "bwd_chain"  1  rgbnm_vit_chain_bwd eligible (0: the per-operation kernels)
 *   SwinV2
 *   "ln_rows"      1  lanes-per-row LayerNorm kernels for the four stage widths            "win_xcd"  1  XCD-aware window walk
 *   JPEG entropy decode
 *   "jpeg_lanes"   0  runs per wave of rgbnm_jpeg_decode_batch, 1..64 (0: chosen per launch so that about 2048 waves share the runs);
 *                     in rgbnm_jpeg_decode_batch_split also the segments per wave of its segment launches
 *   "jpeg_min_seg" 0  rgbnm_jpeg_decode_batch_split splits runs of at least this many segments (0: 16; at least 2)
 *   "jpeg_split_wgs" 0  cap on the workgroups of each of its launches (0: 4096; tests send the grid-stride loops round again)
 *   "jpeg_encode_wgs" 0  the same cap for the launches of rgbnm_jpeg_encode_batch
 *   measurement
 *   "trace"        0  bit mask of kernel classes to bracket with HIP events, see rgbnm_trace_collect */
int rgbnm_set_option(const char* name, int value);
int rgbnm_get_option(const char* name);
/* With option "trace" = (1 << tag) the launchers bracket kernels of that class with HIP events recorded on the launch
 * stream (tags: 1 gemm_nt, 2 gemm_tn, 3 attention fwd, 4 attention bwd, 5 one-launch encoder forward, 6 one-launch encoder backward,
 * 7 augment stage, 8 sub-block embed, 9 clip + AdamW + WeightDecay, 10 the four GEMM stages of rgbnm_dct_dft_ops).  collect() synchronises those events and
 * returns their summed elapsed ms plus the algorithmic FLOPs / bytes of the bracketed launches, then forgets them. */
int rgbnm_trace_collect(int tag, double* ms_total, double* flops_total, double* bytes_total, int* count);
/* Create the events of the next n_events / 2 bracketed launches NOW (call outside a timed region: the runtime grows its signal
 * pool in chunks, and the chunk that a traced step happens to trigger costs the host tens of milliseconds -- 70 - 85 ms measured in
 * the 9th traced step of bench.py, enough to drain a 16-step queue). */
int rgbnm_trace_reserve(int n_events);
/* human readable text for a negative return code */
const char* rgbnm_strerror(int code);

/* ---------------------------------------------------------------------------------------------
 * GEMMs (replace nn.Linear forward/backward: plainvit.py:195,441,443,487,490,553,555)
 * ------------------------------------------------------------------------------------------- */
/* C[M,N] = epi(A[M,K] . W[N,K]^T).  bias fp32 [N] or NULL.  R/C2/pos as required by `epi`.
 * c_f32 != 0 stores C as fp32 regardless of dtype (logits). */
int rgbnm_gemm_nt(int dtype, int epi, const void* A, int lda, const void* W, int ldw, void* C, int ldc,
                  const float* bias, const void* R, int ldr, void* C2, int ldc2, const float* pos, int pos_period,
                  int M, int N, int K, int c_f32, void* stream);

/* Dropout mask contract (every kernel that draws a mask uses csrc/philox.h):
 *   element (row, col) of dropout site `site` (0 after the attention projection, 1 after GELU, 2 after fc2) of encoder block `block`
 *   is KEPT when  word >= thr,  word = word (col & 3) of Philox4x32-10 with
 *     counter = (col >> 2, row, block * 4 + site, 0),  key = (low 32 bits, high 32 bits) of the 64-bit seed at `seed`
 *     (device memory, read by the kernels: a captured graph replays with the seed the step drew),  thr = llround(p 2^32);
 *   kept elements are multiplied by the fp32 scale = 1.0f / (1.0f - p), dropped ones become 0 (nn.Dropout's inverted scaling;
 *   the bits are this library's, not torch's).  row = the token row in [0, B N), col = the feature.  p in [0, 1); p = 0 keeps all.
 * One counter covers 4 consecutive columns: the staged epilogue and rgbnm_dropout_apply take 8 columns per thread (two counters);
 * the direct (fp32) epilogue holds one column per lane and evaluates a counter per element, using one of its four words. */
/* rgbnm_gemm_nt with epi RGBNM_EPI_RES_DROP or RGBNM_EPI_GELU_DROP (pos must be NULL) on the generic gemm_nt kernel (staged or
 * direct epilogue, never the bf16-tuned variants). */
int rgbnm_gemm_nt_drop(int dtype, int epi, const void* A, int lda, const void* W, int ldw, void* C, int ldc,
                       const float* bias, const void* R, int ldr, void* C2, int ldc2, const float* pos, int pos_period,
                       int M, int N, int K, int c_f32, const void* seed, float p, int site, int block, void* stream);
/* y[M,N] = keep scale x (in place allowed: y == x, ldy == ldx). */
int rgbnm_dropout_apply(int dtype, const void* seed, float p, int site, int block, const void* x, int ldx, void* y, int ldy,
                        int M, int N, void* stream);

/* dW[No,Ki] (fp32) = dY[M,No]^T . X[M,Ki]; db[No] = column sums of dY (db may be NULL).
 * perm_heads > 0: rows of dW/db are written in the reference's interleaved '(h d qkv)' order
 * (plainvit.py:447) although dY's columns are [q|k|v] blocks.  accumulate != 0: += into dW/db. */
size_t rgbnm_gemm_tn_workspace(int M, int No, int Ki);
/* ... or room for `splits` (1 .. 128) slices of fp32 partial sums only: rgbnm_gemm_tn takes any workspace of at least one slice and
 * splits the token axis no further than the workspace allows (a job queued in a group bracket is split at most 256 / its own
 * 128 x 192 output tiles ways: swinv2.py sizes its queued jobs' workspaces by that -- 13 GB of scratch per backward before) */
size_t rgbnm_gemm_tn_workspace_splits(int No, int Ki, int splits);
int rgbnm_gemm_tn(int dtype, const void* dY, int ldy, const void* X, int ldx, float* dW, float* db, int M, int No,
                  int Ki, int perm_heads, int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* Grouped weight gradients.  Between _begin and _end (same host thread) bf16 rgbnm_gemm_tn calls over the SAME row count are
 * queued -- up to four -- and run as ONE launch at _end (or when the queue fills / the row count changes): with T output tiles
 * in total every job is split 256 / T ways instead of 256 / its own tiles, so fewer fp32 partial sums are written and re-read,
 * and one reduction launch serves all jobs.  dW / db hold nothing until _end returns; every queued call needs ITS OWN workspace
 * (the partial sums live there until _end).  The ViT block backward groups its four dW GEMMs this way internally; this pair is
 * for callers that drive the Linears one by one (swinv2.py: the two dW GEMMs of an MLP).  Reference: autograd computes each
 * Linear's weight gradient as its own GEMM (torch.nn.Linear backward). */
void rgbnm_gemm_tn_group_begin(void);
int rgbnm_gemm_tn_group_end(void* stream);
/* The same with room for up to max_jobs (<= 48) queued GEMMs: a caller that brackets a whole backward pass (swinv2.py: every
 * Linear of a stage has the same row count) gets launches of up to 256 output tiles -- what is queued runs when the next job
 * would pass 256 tiles, when the row count changes, when max_jobs are queued, and at _end.  With no token split left the kernel
 * writes dW / db itself: no partial sums, no reduction.  The operands of a queued call must stay alive and unmodified, and its
 * dW / db hold nothing, until _end returns. */
void rgbnm_gemm_tn_group_begin_n(int max_jobs);
/* Brackets nest by joining: a _begin inside an open bracket (also the ones rgbnm_head_bwd / rgbnm_vit_block_bwd open internally)
 * only counts, its _end neither launches nor closes anything; the jobs run at the OUTERMOST _end.  The library cannot tell a bracket
 * whose pass died before its _end from one that is still open -- the next _begin on that thread would join it, and neither pass's
 * jobs would run at that _begin's _end --, so an UNNAMED bracket (_begin, _begin_n) must be closed by the thread that opened it, on
 * every path.  A pass that can die before its _end takes a NAMED bracket and _abort:
 * _begin_id names the bracket (id != 0; only an outermost one: inside an open bracket it joins like _begin_n and the open bracket
 * keeps its name or its lack of one): rgbnm_gemm_tn_group_abort(id), callable from ANY host thread, makes the thread that owns
 * the bracket drop its queue without launching and close the bracket -- at once when called on the owning thread, else the next
 * time the owner touches its queue -- for callers whose backward nodes run on an autograd worker thread while the pass is found
 * abandoned on another one (swinv2.py).  _abort of 0 does nothing; _abort of an id that names no open bracket changes nothing for
 * the brackets that are open (it waits for a bracket of that name: ids are one per pass, never reused for a live one).
 * Reference: none (torch launches every GEMM at once). */
void rgbnm_gemm_tn_group_begin_id(int max_jobs, unsigned long long id);
void rgbnm_gemm_tn_group_abort(unsigned long long id);

/* One nn.Linear in the flat fp32 master buffer and where its shadows go (offsets in elements). */
typedef struct rgbnm_linear_desc {
  long long w_off;     /* master: weight [N,K] fp32                                   */
  long long b_off;     /* master: bias [N] fp32                                       */
  long long ws_off;    /* shadow: [N,K] in dtype (rows de-interleaved if perm_heads)  */
  long long wst_off;   /* shadow: [K,N] in dtype (transpose of the above)             */
  long long bperm_off; /* bias_perm: [N] fp32 de-interleaved bias (only if perm_heads) */
  int N, K;
  int perm_heads;      /* >0 for the qkv Linear: number of heads                      */
  int add_identity;    /* shadows hold W + I (residual Linear y = x W^T + x, plainvit.py:345-347) */
  int ldn;             /* row stride of the [K,N] shadow; 0 = N.  > N pads N for 16-byte rows (a class count that is not a
                          multiple of 8: the [N,K] shadow then has ldn rows too, the extra ones left as the caller zeroed them) */
  int pair;            /* != 0: block-diagonal shadows diag(W, W) [2N,2K] and diag(W^T, W^T) [2K,2N] (off-diagonal blocks left as
                          the caller zeroed them).  x [M,K] read as [M/2,2K] times diag(W,W)^T is y [M,N] read as [M/2,2N]: a
                          96-wide Linear (SwinV2-T stage 1) then runs on the kernels tuned for 192-wide rows            */
  int chain_kind;      /* rgbnm_prep_weights_chain: 0, or which Linear of an encoder block this is: 1 qkv, 2 projection, 3 fc1, 4 fc2 */
  long long chain_off; /* ... and the element offset of that block's image inside the forward / backward chain images */
  int bias_mode;       /* bias_perm[bperm_off ..] also receives (perm_heads == 0): 1 the bias b_off as it is; 2 the SwinV2 qkv bias
                          q_bias | 0 | v_bias (swinv2.py:150-152: k has no bias), q_bias at b_off, v_bias at b2_off, N / 3 each.
                          With `pair` the N values are written twice (the operand of the row-paired GEMM): 2N floats */
  int _pad2;
  long long b2_off;
} rgbnm_linear_desc;

/* master fp32 -> per-step operand shadows for every Linear (descs_dev: device array of ndesc descriptors). */
int rgbnm_prep_weights(int dtype, const rgbnm_linear_desc* descs_dev, int ndesc, const float* master, void* shadow,
                       float* bias_perm, void* stream);
/* The same launch also writes the chain images of the one-launch encoder kernels (rgbnm_vit_chain_fwd / _bwd below; bf16,
 * E = 192, 3 heads) straight from the fp32 masters: for every descriptor with chain_kind != 0 the weight goes to its place in
 * chain_fwd ([N, K] orientation) and chain_bwd ([K, N]) -- either may be NULL -- exactly where rgbnm_chain_gather over the
 * shadows would put it (rgb-no-more_amd/chain.py documents the layout; the kernel carries its arithmetic inverse).
 * skip_chain_shadows != 0: the [N, K] / [K, N] shadows of those descriptors are NOT written (nothing reads them while the
 * one-launch kernels run the encoder).  Before round 6 this was four launches per step (prep, bias gather, two image gathers). */
int rgbnm_prep_weights_chain(int dtype, const rgbnm_linear_desc* descs_dev, int ndesc, const float* master, void* shadow,
                             float* bias_perm, void* chain_fwd, void* chain_bwd, int skip_chain_shadows, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm (nn.LayerNorm(emb), plainvit.py:513,522,551) and head pooling (:551-552)
 * ------------------------------------------------------------------------------------------- */
int rgbnm_layernorm_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* y, float* mean,
                        float* rstd, int M, int E, float eps, void* stream);
size_t rgbnm_layernorm_bwd_workspace(int M, int E);
/* dx = [dres +] LN'(dy); dgamma/dbeta fp32.  dres may be NULL. */
int rgbnm_layernorm_bwd(int dtype, const void* dy, const void* x, const float* gamma, const float* mean,
                        const float* rstd, const void* dres, void* dx, float* dgamma, float* dbeta, int M, int E,
                        int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* pooled[b,:] = mean_t LN(x[b,t,:]) */
int rgbnm_head_pool_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* pooled, float* mean,
                        float* rstd, int B, int N, int E, float eps, void* stream);
int rgbnm_head_pool_bwd(int dtype, const void* dpooled, const void* x, const float* gamma, const float* mean,
                        const float* rstd, void* dx, float* dgamma, float* dbeta, int B, int N, int E, int accumulate,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Attention (MultiHeadAttention.forward, plainvit.py:445-464): qkv [B*N, 3*heads*64] as [q|k|v] column
 * blocks, out [B*N, heads*64] ('b n (h d)'), lse [B*heads*N] fp32.  scale = 1/sqrt(emb_size) (!).
 * ------------------------------------------------------------------------------------------- */
int rgbnm_attention_fwd(int dtype, const void* qkv, void* out, float* lse, int B, int N, int heads, float scale,
                        void* stream);
int rgbnm_attention_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                        int B, int N, int heads, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sub-block reshuffle (patch2rearrange + apply_subblock + collapser + cat, plainvit.py:71-88,50-69,192,
 * 200-216) for patch_size 16: y [B,1,Hb,Wb,8,8], cbcr [B,2,Hb/2,Wb/2,8,8] -> feat [B*(Hb/2)*(Wb/2), 384].
 * conv16: the 16x16 fp32 conversion matrix A (dct_ops.py:180-208).
 * ------------------------------------------------------------------------------------------- */
int rgbnm_subblock_embed(int in_dtype, int out_dtype, const void* y, const void* cbcr, const float* conv16,
                         void* feat, int B, int Hb, int Wb, int transpose_a, void* stream);
/* The same on a batch that RandomMixup_DCT (utils/cls_transforms.py:163-176) has NOT been applied to yet: lam_dev (device, two
 * floats, may be NULL = no mixing) mixes image b with image b - 1 (mod B) as the values are loaded:
 *   x[b] <- round_in_dtype( fma(x[b - 1], lam[1], x[b] * lam[0]) )       (fp32 product, fp32 fma, ONE rounding to in_dtype)
 * for every in_dtype the entry accepts, fp16 included.  For fp32 and bf16 input that is what rgbnm_mixup(in_dtype -> in_dtype)
 * stores (fp16: rgbnm_mixup_any): the same bits as rgbnm_mixup followed by rgbnm_subblock_embed without the mixed
 * batch ever existing in memory (two launches and a round trip of the batch less per step). */
int rgbnm_subblock_embed_mix(int in_dtype, int out_dtype, const void* y, const void* cbcr, const float* lam_dev, const float* conv16,
                             void* feat, int B, int Hb, int Wb, int transpose_a, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DCT-domain data path: replaces, per batch and on device, what the reference does per sample
 * on the CPU inside DataLoader workers: dequantise+clamp (datasets.py:288-293), RandomResizedCrop_DCT
 * (custom_transforms.py:631-663 -> dct_ops.py crop :584-599, resize :529-580), RandomFlip_DCT (:926-942),
 * RandAugment_dct / _apply_op_dct (:944-1127), ToRange (:436-454).  All random draws are made by the caller.
 * ------------------------------------------------------------------------------------------- */
#define RGBNM_OP_IDENTITY 0
#define RGBNM_OP_AUTOCONTRAST 1    /* autocontrast_dct on Y                 (dct_ops.py:862-887)  */
#define RGBNM_OP_POSTERIZE 2       /* iarg0 = bit offset, iarg1 = table length round(2040/2^b)+1 (:889-914) */
#define RGBNM_OP_SOLARIZEADD 3     /* iarg0 = addition                      (:653-679)            */
#define RGBNM_OP_COLOR 4           /* contrast_dct on CbCr, fmag = factor   (:839-860)            */
#define RGBNM_OP_CONTRAST 5        /* contrast_dct on Y, fmag = factor                            */
#define RGBNM_OP_BRIGHTNESS 6      /* fmag = factor - 1                     (:817-837)            */
#define RGBNM_OP_MIDFREQAUG 7      /* iarg0 = index of the 8x8 fp32 multiplier in `filters` (:710-746) */
#define RGBNM_OP_CUTOUT 8          /* iarg0 = pad (luma, even), iarg1/iarg2 = centre h/w (luma blocks) (:776-815) */
#define RGBNM_OP_TRANSLATEX 9      /* iarg0 = luma block shift int(m - m%2) (:748-774)            */
#define RGBNM_OP_TRANSLATEY 10
#define RGBNM_OP_ROTATE90 11       /* iarg0 = +1 counter-clockwise / -1 clockwise (:99-130)       */
#define RGBNM_OP_AUTOSATURATION 12 /* autocontrast_dct on CbCr jointly                            */
#define RGBNM_OP_GRAYSCALE 13      /* CbCr *= 0                             (custom_transforms.py:1004-1005) */
#define RGBNM_OP_CHROMADROP 14     /* iarg0 != 0 drops Cb, else Cr          (:1011-1015)          */
#define RGBNM_OP_SHARPNESS 15      /* sharpblur_dct, iarg0 = filter index   (dct_ops.py:681-708)  */
#define RGBNM_OP_INVERT 16         /* invert_dct: all coefficients * -1     (dct_ops.py:623-629)  */
#define RGBNM_OP_SOLARIZE 17       /* iarg0 = floor(threshold): blocks with luma DC > threshold negated (:631-651) */
#define RGBNM_OP_FREQENHANCE 18    /* fmag = factor: AC coefficients * factor, rounded (:1015-1035) */
#define RGBNM_OP_EQUALIZE 19       /* equalize_dct: histogram equalisation of the luma DCs (:916-955) */

typedef struct rgbnm_aug_params {
  int crop_i, crop_j, crop_h, crop_w; /* luma blocks; chroma box = luma box / 2 (custom_transforms.py:647-652) */
  int flip;                           /* horizontal flip after the resize */
  int op[2];
  float fmag[2];
  int iarg0[2], iarg1[2], iarg2[2];
} rgbnm_aug_params;

size_t rgbnm_dct_augment_workspace(int B);
/* Yq [B,1,Hy,Wy,8,8], CbCrq [B,2,Hc,Wc,8,8] (NULL: grayscale -> zero chroma), quant [B,3,8,8]: int16 as returned by
 * read_coefficients.  crop_w must be 56, 28 or 14 (resize /2, identity, x2 -> 28x28 luma / 14x14 chroma blocks).
 * params are needed twice: on the device (kernels) and on the host (validated before launch).
 * conv16: A(8,2) 16x16 fp32; filters: [n][64] fp32 multipliers for MIDFREQAUG/SHARPNESS.  filters may be NULL only if none of
 * the first nops ops of any image is MIDFREQAUG or SHARPNESS: otherwise the call returns RGBNM_EINVAL.  iarg0 of those two ops
 * must index a table of the bank (not checked: the bank's length is not an argument).
 * outY [B,1,28,28,8,8], outC [B,2,14,14,8,8] in out_dtype, after ToRange(-1,1; -1024,1016); out_dtype 2 (RGBNM_DT_I16)
 * stores the int16 coefficients themselves, WITHOUT ToRange (the per-transform classes of custom_transforms.py chain on it).
 * entry_clamp bit 0: clamp before the first op (RandAugment_dct.forward, :1106-1108); bit 1: the input is already
 * de-quantised (unit tables) and must NOT be clamped in front of the crop / resize / flip stage (the reference's per-transform
 * classes pass out-of-range coefficients of a preceding resize through unchanged).  nops in {0,1,2}.
 * Flat images (every DC of the op's plane set equal), as the reference's CPU kernels leave them (tests/golden/g24_flat.npz):
 * AUTOCONTRAST / AUTOSATURATION keep the DCs when min = max = 0 and otherwise set every DC to 0 (0 / 0 = NaN, which the int16
 * cast turns into 0); EQUALIZE sets every luma DC to -1024 (the same NaN, shifted back by the range minimum).
 * Every argument is validated on the host before anything is launched: a NULL pointer (CbCrq and filters excepted, see above),
 * B <= 0, nops or size or out_dtype outside their sets, a crop box that is odd, negative, outside the luma or chroma grid, not
 * square or of a side other than size/2, size, 2 size, or an op id outside 0..19 return RGBNM_EINVAL, a short workspace
 * RGBNM_EWORKSPACE; no kernel has then run and no buffer has been touched. */
int rgbnm_dct_augment(const int16_t* Yq, const int16_t* CbCrq, const int16_t* quant, const rgbnm_aug_params* params_dev,
                      const rgbnm_aug_params* params_host, const float* conv16, const float* filters, void* outY,
                      void* outC, int out_dtype, int B, int Hy, int Wy, int Hc, int Wc, int entry_clamp, int nops,
                      void* workspace, size_t workspace_bytes, void* stream);
/* The same pipeline for a `size` x `size` output block grid: 28 (ViT pipelines, get_transform('imagenet_dct')) or 32
 * (SwinV2, 'imagenet_dct_swin', datasets.py:370-382; crop sides 16 / 32 / 64).  outY [B,1,size,size,8,8],
 * outC [B,2,size/2,size/2,8,8]. */
size_t rgbnm_dct_augment_workspace_ex(int B, int size);
int rgbnm_dct_augment_ex(const int16_t* Yq, const int16_t* CbCrq, const int16_t* quant, const rgbnm_aug_params* params_dev,
                         const rgbnm_aug_params* params_host, const float* conv16, const float* filters, void* outY,
                         void* outC, int out_dtype, int size, int B, int Hy, int Wy, int Hc, int Wc, int entry_clamp,
                         int nops, void* workspace, size_t workspace_bytes, void* stream);

/* The same pipeline on HOST-CROPPED input (loader.DCTBatchLoader(crop_on_host=True); SURVEY.md 8f f2: "ship only the crop
 * box"): image b's crop box alone, as contiguous int16 blocks [crop_h][crop_w][64] at Ypacked + y_off[b] and
 * [2][crop_h/2][crop_w/2][64] at Cpacked + c_off[b] (element offsets, device arrays of B entries; Cpacked NULL: grayscale).
 * params[b].crop_* still hold the box in the ORIGINAL Hy x Wy grid (validated against it on the host exactly as in
 * rgbnm_dct_augment); the kernels read the box from origin 0 with its own row pitch.  Output bit-identical to
 * rgbnm_dct_augment_ex on the whole grids.  Replaces datasets.py:274-297 + pipeline_utils.py:70-73 (.to(device) of whole
 * coefficient tensors). */
int rgbnm_dct_augment_packed(const int16_t* Ypacked, const int16_t* Cpacked, const long long* y_off, const long long* c_off,
                             const int16_t* quant, const rgbnm_aug_params* params_dev, const rgbnm_aug_params* params_host,
                             const float* conv16, const float* filters, void* outY, void* outC, int out_dtype, int size, int B,
                             int Hy, int Wy, int Hc, int Wc, int entry_clamp, int nops, void* workspace, size_t workspace_bytes,
                             void* stream);

/* The same two kernels behind one entry that also writes fp16 and takes RandAugment chains of more than two ops
 * (train.py --ampdtype float16, --num_ops N).
 * y_off / c_off both NULL: Y / C are the whole grids, as rgbnm_dct_augment_ex; both set: the host-cropped buffers of
 * rgbnm_dct_augment_packed.  ops_dev / ops_host both NULL: the ops are the two slots of the parameters and nops is 0..2; both set:
 * [B][nops] records (device and host copy, like the parameters), image b's chain at ops[b * nops], nops 0..RGBNM_AUG_MAX_OPS, and
 * the op / fmag / iarg* fields of the parameters are ignored (pad a shorter chain with RGBNM_OP_IDENTITY).
 * out_code: RGBNM_AUG_OUT_*.  F16 is ToRange in fp32 as for the other types, rounded once to IEEE half (nearest even): the bits
 * of torch's .half() of the fp32 output.  Kernel 2 is one launch per batch whatever nops is; the clamp rules are unchanged (entry
 * clamp in kernel 1's store, one full pass after the FIRST op of an image that entered unclamped, none for later ops: every op
 * clamps what it writes).  For out_code 0 / 1 / 2 and nops <= 2 the output is bit-identical to rgbnm_dct_augment_ex / _packed,
 * with the ops from the parameters or from an array holding the same ops.
 * Crop boxes, entry_clamp, filters, workspace (rgbnm_dct_augment_workspace_ex) and the validation are those of the entries
 * above; also refused with RGBNM_EINVAL: nops < 0 or > RGBNM_AUG_MAX_OPS, nops > 2 without an ops array, only one of ops_dev /
 * ops_host (or of y_off / c_off), out_code outside 0..3, an op id outside 0..19 or MIDFREQAUG / SHARPNESS with filters == NULL in
 * any of the nops slots. */
#define RGBNM_AUG_MAX_OPS 8
#define RGBNM_AUG_OUT_F32 0
#define RGBNM_AUG_OUT_BF16 1
#define RGBNM_AUG_OUT_I16 2
#define RGBNM_AUG_OUT_F16 3
typedef struct rgbnm_aug_op { int op; float fmag; int iarg0, iarg1, iarg2; } rgbnm_aug_op;   /* 20 bytes; fields as in rgbnm_aug_params */
int rgbnm_dct_augment_chain(const int16_t* Y, const int16_t* C, const long long* y_off, const long long* c_off,
                            const int16_t* quant, const rgbnm_aug_params* params_dev, const rgbnm_aug_params* params_host,
                            const rgbnm_aug_op* ops_dev, const rgbnm_aug_op* ops_host, const float* conv16,
                            const float* filters, void* outY, void* outC, int out_code, int size, int B, int Hy, int Wy,
                            int Hc, int Wc, int entry_clamp, int nops, void* workspace, size_t workspace_bytes, void* stream);

/* The DFT-plane operations of RandAugment_dct -- Rotate, ShearX, ShearY (utils/dct_ops.py:367-434, 957-1013) -- for a list of
 * samples of a batch, in place, as four launches per call (csrc/dft_ops.hip).  Y [B,1,S,S,8,8] and C [B,2,S/2,S/2,8,8] (NULL:
 * luma only) int16; S even, 2..32.  Each plane is zero-padded to Hp x Hp blocks (S <= Hp_y <= 48, S/2 <= Hp_c <= 48; margins
 * (Hp - Hb) / 2, the larger one behind when the difference is odd), turned by rot90s exact quarter turns (0..3, counter-clockwise,
 * of the PADDED grid), block-shifted, taken to the DFT plane F = L.X.L^H with L = conv (interleaved complex64 [N][N], N = 8 Hp:
 * dct_ops.generate_conversion_matrix_dft(8, Hp)), resampled G[p] = F[map[p]] (map[p] = -1 or anything outside 0..N*N-1: zero) with
 * map number map_y / map_c of maps_y [nmaps][Ny*Ny] / maps_c [nmaps][Nc*Nc], taken back, un-shifted, cropped, rounded half to even
 * and stored as int16; clamp = 1 then clamps to [-1024, 1016] (the reference's per-op clamp, custom_transforms.py:1019-1020).
 * The twelve real products per plane run on the exact f32-input MFMA; a sample's result does not depend on the other jobs and is
 * the same from run to run.  Samples not listed are not touched.  The jobs are needed on the device (kernels) and on the host
 * (validated before launch).  workspace: rgbnm_dct_dft_workspace(njobs, Hp_y, Hp_c) bytes.
 * RGBNM_EINVAL with nothing launched and no buffer touched: S odd or outside 2..32, B <= 0, Hp below the plane's grid or above 48,
 * njobs < 0, only one of jobs_dev / jobs_host, a sample outside 0..B-1 or listed twice, rot90s outside 0..3, a map index outside
 * 0..nmaps-1, clamp outside 0..1, a NULL Y / conv_y / maps_y (conv_c / maps_c with C), a workspace that is NULL or too small.
 * njobs == 0 returns 0 without a launch. */
typedef struct rgbnm_dft_job { int sample; int rot90s; int map_y; int map_c; } rgbnm_dft_job;
size_t rgbnm_dct_dft_workspace(int njobs, int Hp_y, int Hp_c);
int rgbnm_dct_dft_ops(int16_t* Y, int16_t* C, int B, int S, int Hp_y, int Hp_c, const rgbnm_dft_job* jobs_dev,
                      const rgbnm_dft_job* jobs_host, int njobs, const float* conv_y, const float* conv_c,
                      const int32_t* maps_y, const int32_t* maps_c, int nmaps, int clamp, void* workspace, size_t workspace_bytes,
                      void* stream);

/* RGB (or gray) pixels to quantised DCT coefficients and back (csrc/pixel_dct.hip): what the reference gets from libjpeg (IJG 9,
 * 4:2:0) through dct_manip.quantize_at_quality / decode_coeff (dct_manip.cpp:315-375, 485-576), for a batch on the device.  One
 * launch per call, no allocation, no copy, no synchronisation: a call can be captured into a HIP graph.
 * Layouts: pixels uint8 [B,C,H,W]; Y int16 [B,1,H/8,W/8,8,8]; CbCr int16 [B,2,H/16,W/16,8,8] -- the read_coefficients layout.
 * C = 3 needs H and W divisible by 16, C = 1 (Y only, CbCr unused) by 8: libjpeg's edge replication is not done.
 * quant_host: int16 [C][64] in HOST memory, natural order; it travels in the kernel arguments.  With C = 3 table 0 is luma's and
 * table 1 serves BOTH chroma planes, as in libjpeg's component setup (decode_coeff copies two tables, dct_manip.cpp:180-187);
 * table 2 is read only for the entry check.
 * rgbnm_pixels_to_dct.  Luma is integer arithmetic and equals libjpeg bit for bit: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,
 * minus 128, the "islow" forward DCT (13-bit constants, 2 pass-1 bits: 8 x the DCT), then sign(c) (|c| + 4 q) / (8 q).  Chroma is
 * the low 8 x 8 of the 16 x 16-point DCT of the MCU's integer Cb / Cr samples, in fp32, divided by the table entry and rounded half
 * away from zero: within 1 of libjpeg, whose fixed-point 16-point routine is up to 0.08 off the exact value.
 * rgbnm_dct_to_pixels (CbCr == NULL: one channel).  Dequantise; 8 x 8 inverse DCT for luma, the 8 -> 16 scaled inverse DCT for chroma,
 * in fp32; every plane sample is floor(x + 0.5) clamped to [0, 255]; then libjpeg's fixed-point YCbCr -> RGB (16-bit scale, + 32768
 * before the shift), clamped: within 3 of libjpeg wherever the exact samples of all three planes lie in [-128, 383].  Outside that
 * range libjpeg's range-limit table wraps around; this call saturates.
 * RGBNM_EINVAL with nothing launched: B, H or W <= 0, C not 1 or 3, H or W not divisible as above, B C H W >= 2^31, a NULL
 * pixels / quant_host / Y (CbCr with C = 3 in rgbnm_pixels_to_dct), pixels not 4-byte or Y / CbCr not 16-byte aligned, a table entry
 * below 1 in rgbnm_pixels_to_dct.  RGBNM_ELAUNCH if the launch failed. */
int rgbnm_pixels_to_dct(const uint8_t* pixels, int B, int C, int H, int W, const int16_t* quant_host, int16_t* Y, int16_t* CbCr,
                        void* stream);
int rgbnm_dct_to_pixels(const int16_t* Y, const int16_t* CbCr, int B, int H, int W, const int16_t* quant_host, uint8_t* pixels,
                        void* stream);

/* Entropy decoding of baseline JPEG files on the device (csrc/jpeg_scan.h, jpeg_walk.h, jpeg_decode.hip): from file bytes to the
 * int16 coefficient tensors of rgbnm_read_coefficients_batch (include/rgbnm_reader.h), bit for bit.  A baseline scan is a set of
 * independent bit streams -- the whole scan, or one per restart interval -- so the host only FINDS them (rgbnm_jpeg_prepare: marker
 * parse, removal of the stuffed FF 00, split at RSTn; a byte scan, no Huffman decode, callable without a GPU) and the device walks
 * them, one lane per run (rgbnm_jpeg_decode_batch).
 * Accepted: SOF0 / SOF1, 8 bit, Huffman, ONE scan holding all components; one component, or three whose block grids are Hb x Wb,
 * Hbc x Wbc, Hbc x Wbc with at most 10 blocks per MCU and sampling factors <= 4 (4:2:0 gives 2x2, 1x1, 1x1).  Anything else gets a
 * negative per-file status and leaves the other files of the batch untouched.
 *
 * Per-file status (rgbnm_jpeg_image.status, and the device status array, which starts as a copy of it): */
#define RGBNM_JPEG_ETRUNCATED (-10)    /* a marker segment or the scan runs past the end of the file (no EOI) */
#define RGBNM_JPEG_EMARKER (-11)       /* inconsistent marker segment: no SOI / SOF / table, bad length, bad table, bad scan header */
#define RGBNM_JPEG_EUNSUPPORTED (-12)  /* progressive, arithmetic, lossless, 12 bit, several scans, DNL, 2 or 4 components, sampling */
#define RGBNM_JPEG_EGRID (-13)         /* the file's block grids are not the requested ones */
#define RGBNM_JPEG_ERESTART (-14)      /* RSTn out of sequence (D0..D7 cyclic), or the run count is not ceil(MCUs / interval) */
#define RGBNM_JPEG_ECAPACITY (-15)     /* the plan's stream / runs / tables buffer is too small for this file */
#define RGBNM_JPEG_ECODE (-20)         /* device: a bit pattern that no Huffman code of the table matches, or a DC category > 15 */
#define RGBNM_JPEG_EINDEX (-21)        /* device: a coefficient index past 63 */
#define RGBNM_JPEG_EOVERRUN (-22)      /* device: more bits consumed than the run holds */
#define RGBNM_JPEG_ETRAILING (-23)     /* device: more than a byte of bits left over after the run's last MCU */
#define RGBNM_JPEG_ERECORD (-24)       /* device: a run / image record that does not fit the buffers it points into */
#define RGBNM_JPEG_ERANGE (-25)        /* encode: an AC coefficient beyond +-1023, a DC difference beyond +-2047 or a quantisation value
                                          outside 1..255: baseline Huffman coding cannot express it */
#define RGBNM_JPEG_EBOX (-26)          /* device, crop decode: a crop box that is not even or not inside the grid, or a packed offset
                                          that is misaligned or does not leave room for the box in its buffer */

/* One run: the entropy-coded bytes between two markers, un-stuffed.  offset is a multiple of 4; behind the nbytes bytes the stream
 * holds zeros up to the next multiple of 4 and 4 more, so that 32-bit reads of a run never leave the buffer.  nmcu == 0: a record of
 * a file that was refused after its records had been laid out; the device skips it. */
typedef struct rgbnm_jpeg_run { uint32_t offset, nbytes; int32_t image, mcu0, nmcu, _pad[3]; } rgbnm_jpeg_run;            /* 32 bytes */
/* One image.  An MCU is nblk blocks; block j of it belongs to component blk_comp[j] and sits at (blk_dy[j], blk_dx[j]) inside the
 * MCU's vs[c] x hs[c] patch of that component.  dc_tab / ac_tab: index of each component's table in the batch's table array.
 * The kept grids are the call's Hb x Wb (component 0) and Hbc x Wbc (components 1, 2): blocks of the MCU padding beyond them are
 * decoded and dropped. */
typedef struct rgbnm_jpeg_image {
  int32_t ncomp, mcus_x, mcus_y, nblk, status;
  int32_t dc_tab[3], ac_tab[3], hs[3], vs[3];
  int32_t blk_comp[10], blk_dx[10], blk_dy[10];
  int32_t nruns;                        /* runs of this image (consecutive records) */
} rgbnm_jpeg_image;                                                                                                       /* 192 bytes */
/* One Huffman table in the form the walk looks up: look[next 9 bits] = (code length << 8) | symbol, 0 for codes longer than 9 bits;
 * for those, libjpeg's canonical search: the first l in 10..16 with (next l bits) <= maxcode[l] (-1: no code of that length) gives
 * symbol vals[(next l bits) + valoff[l]].  bits / vals are the DHT segment's (the key tables are de-duplicated by). */
typedef struct rgbnm_jpeg_hufftab {
  uint16_t look[512];
  int32_t maxcode[18], valoff[18];
  uint8_t vals[256], bits[16];
} rgbnm_jpeg_hufftab;                                                                                                     /* 1440 bytes */
/* What rgbnm_jpeg_prepare fills.  The caller owns every buffer (pinned, when the plan is to be copied to the device) and sets the
 * pointers, the capacities and `threads`; the call sets the counts.  stream_cap of sum(lens) + 8 * runs_cap always suffices;
 * an image has at most min(MCUs, len / 2 + 1) runs; a batch has at most 65535 distinct tables.
 *   stream   the runs' bytes (FF 00 -> FF, fill FFs and markers dropped), each run aligned and padded as above; a file's runs
 *            lie in the file's own region (laid out from its header before the scan is read), so the regions have small gaps
 *   runs     [nruns] in file order, a file's runs in scan order          images  [n]
 *   tables   [ntables]: every distinct table of the batch once           quant   int16 [n][3][64], natural order, unit tables
 *   messages [n][message_len] (may be NULL): why a file was refused              for the chroma slots of a one-component file
 *   threads  files are un-stuffed by up to this many threads (1..16; the header pass is serial) */
typedef struct rgbnm_jpeg_plan {
  uint8_t* stream; size_t stream_cap;
  rgbnm_jpeg_run* runs; rgbnm_jpeg_image* images; rgbnm_jpeg_hufftab* tables;
  int16_t* quant; char* messages;
  int32_t runs_cap, tables_cap, message_len, threads;
  size_t stream_bytes;                  /* out: used prefix of stream */
  int32_t nruns, ntables, nbad, _pad;   /* out: records used, tables used, files with a negative status */
} rgbnm_jpeg_plan;
/* bufs[i] / lens[i]: file i in host memory.  Returns the number of refused files (>= 0), or RGBNM_EINVAL (NULL pointer, n <= 0, a
 * grid outside 1..4096, capacities <= 0) with nothing written.  Host only: no HIP call. */
int rgbnm_jpeg_prepare(const uint8_t* const* bufs, const size_t* lens, int n, int Hb, int Wb, int Hbc, int Wbc, rgbnm_jpeg_plan* plan);
/* The plan's buffers on the device (copies of the used prefixes) and its counts. */
typedef struct rgbnm_jpeg_device_plan {
  const uint8_t* stream; size_t stream_bytes;
  const rgbnm_jpeg_run* runs; const rgbnm_jpeg_image* images; const rgbnm_jpeg_hufftab* tables;
  int32_t nruns, ntables;
} rgbnm_jpeg_device_plan;
/* One launch, one lane per run: Y int16 [n][Hb][Wb][64], CbCr int16 [n][2][Hbc][Wbc][64] (16-byte aligned).  Every element of an
 * accepted image is written, zeros included (the chroma of a one-component file too); images with a negative host status are not
 * touched.  status: int32 [n] on the device, holding the host statuses on entry (copy rgbnm_jpeg_image.status there, or zeros); a run
 * that ends in an error lowers its image's entry to the RGBNM_JPEG_E* code (atomicMin) and zero-fills the blocks it has not written.
 * The kernel checks every record against the buffer sizes given here, bounds every loop by counts known at entry, waits for no other
 * lane, and cannot write outside Y / CbCr / status whatever the stream holds.  No allocation, no copy, no synchronisation: capturable.
 * RGBNM_EINVAL with nothing launched: NULL pointers, n <= 0, a grid outside 1..4096, nruns < 0, misaligned outputs.  nruns == 0
 * returns 0 without a launch. */
int rgbnm_jpeg_decode_batch(const rgbnm_jpeg_device_plan* plan, int n, int Hb, int Wb, int Hbc, int Wbc, int16_t* Y, int16_t* CbCr,
                            int32_t* status, void* stream);
/* The same decode with long runs cut into bit segments of seg_bits, ONE LANE PER SEGMENT (csrc/jpeg_split.h): for files without
 * restart markers, whose single run is one dependent chain for the call above.  Y, CbCr and status come out as from
 * rgbnm_jpeg_decode_batch, bit for bit, for every input, damaged ones included.
 * A run of at least 16 segments (option "jpeg_min_seg") is split: every segment is walked from a guessed state (scout), then `rounds`
 * times every segment whose entry state differs from its predecessor's exit of the round before walks again from that exit
 * (Huffman codes self-synchronise, so most segments agree after a few rounds; a run of at most rounds + 1 segments is CERTAIN to).
 * A run passes if every entry equals the predecessor's exit, its nmcu * nblk blocks are complete with at most 8 bits left, and no
 * walk met an impossible symbol on the way; then one lane per segment writes the blocks whose DC symbol starts in it.  Every image
 * with a run that did not pass is decoded once more, whole, by the one-lane walk of the call above, which also takes the runs that
 * were not split and alone lowers `status`: the worst case costs that call plus the passes.
 *   path      int32 [n] on the device, written for every image: 0 no run split, 1 split and passed, 2 split, then the one-lane walk
 *   scratch   device memory, 16-byte aligned, at least rgbnm_jpeg_split_scratch_bytes(plan->stream_bytes, plan->nruns, seg_bits)
 *             bytes (about 76 per segment); nothing is kept in it between calls
 *   seg_bits  128..65536, a multiple of 32 (2048 measured best with 16 rounds)         rounds  0..64 sync launches
 * 6 + rounds launches whatever the data; no lane waits for another; no lane reads what the same launch writes, except path[] in the
 * write pass (a lane whose walk fails raises it to 2 while others read it: harmless, the one-lane walk then rewrites that image);
 * every record, trip count, stream read and store is bounded as in the call above.
 * Precondition, met by every plan of rgbnm_jpeg_prepare: the runs lie in `stream` in record order without overlap (the segments'
 * scratch slots follow from the offsets).  A plan that breaks it stays memory-safe; a run whose slots another run took fails verify
 * and is decoded by the one-lane walk.  No allocation, no copy, no synchronisation: capturable.
 * RGBNM_EINVAL with nothing launched: whatever the call above refuses, path NULL or misaligned, scratch NULL, misaligned or too
 * small, seg_bits or rounds out of range.  nruns == 0: path is zeroed, nothing else.
 * rgbnm_jpeg_split_scratch_bytes is host only (no HIP call) and gives 0 for nruns < 0 or seg_bits out of range. */
size_t rgbnm_jpeg_split_scratch_bytes(size_t stream_bytes, int nruns, int seg_bits);
int rgbnm_jpeg_decode_batch_split(const rgbnm_jpeg_device_plan* plan, int n, int Hb, int Wb, int Hbc, int Wbc, int16_t* Y, int16_t* CbCr,
                                  int32_t* status, int32_t* path, void* scratch, size_t scratch_bytes, int seg_bits, int rounds,
                                  void* stream);
/* The decode of rgbnm_jpeg_decode_batch for a CROP BOX per image: what the fused train transform reads of a file is the box its
 * sampler drew, about half the grid, and restart intervals let the device leave the rest alone.
 *   boxes     device int32 [n][4]: (top, left, h, w) in luma blocks, all even, h, w > 0, inside Hb x Wb; the chroma box is the luma
 *             box halved (and must lie inside Hbc x Wbc).  The contract of rgbnm_read_coefficients_batch_crop (rgbnm_reader.h).
 *   y_off, c_off  device int64 [n]: element offsets of image i's crops in the packed buffers, multiples of 8
 *   Ypacked   int16 [y_elems], 16-byte aligned: image i's luma crop [h][w][64] at Ypacked + y_off[i]
 *   Cpacked   int16 [c_elems], 16-byte aligned: its chroma crop [2][h/2][w/2][64] at Cpacked + c_off[i]; zeros for a
 *             one-component file.  The layout is the host crop reader's, exactly.
 *   walked    device uint32 [nruns] or NULL: the number of MCUs the lane of run ri walked; 0 for a run that was skipped or refused
 * One launch, one lane per run, as above.  From the boxes of the components, mapped through their sampling factors, a lane knows
 * which MCUs of its run hold a block of the box.  A run that holds none is NOT WALKED: it reads no word of the stream.  Any other
 * run is walked from its first MCU (predictors and bit position cannot be skipped) and STOPS after its last MCU, in raster order,
 * that holds one.  A block is stored only if it lies inside its component's box; nothing else of the packed buffers is written,
 * and every element of the crops of an accepted image is.
 * For every input, damaged ones included, with the status arrays of the two calls starting from the same values:
 *   (a) the packed output equals the box cut out of what rgbnm_jpeg_decode_batch writes for the same plan;
 *   (b) status_whole <= status_crop <= 0: the crop decode sees a subset of each run's first errors, with their codes;
 *   (c) status_crop == 0 wherever status_whole == 0.
 * So a status of 0 here says NOTHING about the bytes of the stream behind the last MCU a box needed: a walk that stops early has
 * not seen the run's tail and makes neither the RGBNM_JPEG_EOVERRUN check for missing MCUs nor the RGBNM_JPEG_ETRAILING check; a run
 * walked to its end makes both.  After an error only the blocks of the box still owed by the run are zero-filled.
 * Each lane checks its image's box and offsets against the grids, y_elems and c_elems before any store (they are device data,
 * untrusted like the records): a failure lowers status[image] to RGBNM_JPEG_EBOX and nothing of that image is written.
 * No allocation, no copy, no synchronisation: capturable, and a captured call reads the boxes and offsets at replay.
 * RGBNM_EINVAL with nothing launched: whatever rgbnm_jpeg_decode_batch refuses (Ypacked / Cpacked for Y / CbCr), NULL boxes, y_off
 * or c_off, boxes misaligned to 4 bytes, offsets to 8, walked to 4, y_elems or c_elems of 0.  nruns == 0 returns 0 without a launch.
 * rgbnm_jpeg_decode_batch_split takes no box (its scout and sync passes must see the whole run whatever the box); the split decode
 * for a box per image is rgbnm_jpeg_decode_batch_split_crop below. */
int rgbnm_jpeg_decode_batch_crop(const rgbnm_jpeg_device_plan* plan, int n, int Hb, int Wb, int Hbc, int Wbc, const int32_t* boxes,
                                 const long long* y_off, const long long* c_off, int16_t* Ypacked, size_t y_elems, int16_t* Cpacked,
                                 size_t c_elems, int32_t* status, uint32_t* walked, void* stream);
/* The split decode for a CROP BOX per image: for files without restart markers, whose single run the call above can neither skip nor
 * cut short.  init, map, scout, the `rounds` sync launches and verify's checks are rgbnm_jpeg_decode_batch_split's and look at no box,
 * so path[] is what that call writes for the same plan, seg_bits, rounds and options, for every input.  Behind verify's scan every
 * segment knows the blocks that start in it; segment j of a run that passed is LIVE iff one of them belongs to an MCU that holds a
 * block of the box of some component (the box mapped through the sampling factors, as in the call above).  The wave that verifies a
 * run lists its live segments in a list shared by the batch (one atomic add per run); the write launch runs over that list, so its
 * waves are full whatever the boxes, and a segment that is not live reads no word of the stream.  A live segment decodes every block
 * that starts in it and stores those inside the box, packed as by the call above.  The order of the runs in the list may differ from
 * call to call; the outputs do not, since every block of a box starts in exactly one segment and that segment alone stores it.
 * The last launch is the call above's walk for the runs that were not split and for every run of an image with path 2.  In an image
 * with path 1 a run that was not split is walked to its END, whatever the box.
 *   boxes, y_off, c_off, Ypacked, y_elems, Cpacked, c_elems, status     as in rgbnm_jpeg_decode_batch_crop
 *   path, scratch, seg_bits, rounds                                      as in rgbnm_jpeg_decode_batch_split; scratch of at least
 *             rgbnm_jpeg_split_crop_scratch_bytes(plan->stream_bytes, plan->nruns, seg_bits) bytes: the split call's, plus the list
 *             (4 bytes per segment), 8 bytes per run and the list's counter
 *   walked    device uint32 [nruns] or NULL: the MCUs the one-lane walk of the last launch walked of run ri; 0 for a run it skipped,
 *             a refused one, and a split run of a path 1 image (the segment lanes wrote it)
 *   seg_live  device uint32 [nruns] or NULL: for a split run of an image with path 1 the number of its segments the write pass
 *             walked; 0 for every other run
 * For every input, damaged ones included, with the status arrays starting from the same values: (a), (b) and (c) of the call above,
 * and (d) for an image with path 1 the status IS the whole decode's: verify has seen every bit of its split runs and the others are
 * walked to their end, so a 0 there does speak for the bytes behind the box.  (e) For path 0 or 2 the call above's caveat stands: a
 * status of 0 says nothing about the bytes behind the last MCU a box needed.
 * Every write lane and every lane of the last launch checks its image's box and offsets before any store: a failure lowers
 * status[image] to RGBNM_JPEG_EBOX and nothing of that image is written.  The list's count and entries are device data: the count is
 * clamped to the number of slots and every entry is checked against the slot's run record again, as in every segment launch; every
 * record, trip count, stream read and store is bounded as in the two calls above.
 * 6 + rounds launches whatever the data (the write launch's grid follows from the scratch's slot count; it reads the list's length on
 * the device).  No allocation, no copy, no synchronisation: capturable, and a captured call reads the boxes and offsets at replay.
 * RGBNM_EINVAL with nothing launched: whatever rgbnm_jpeg_decode_batch_crop or rgbnm_jpeg_decode_batch_split refuses, seg_live
 * misaligned to 4 bytes, scratch smaller than the bound above.  nruns == 0: path is zeroed, nothing else.
 * rgbnm_jpeg_split_crop_scratch_bytes is host only, at least rgbnm_jpeg_split_scratch_bytes, and 0 where that is 0. */
size_t rgbnm_jpeg_split_crop_scratch_bytes(size_t stream_bytes, int nruns, int seg_bits);
int rgbnm_jpeg_decode_batch_split_crop(const rgbnm_jpeg_device_plan* plan, int n, int Hb, int Wb, int Hbc, int Wbc, const int32_t* boxes,
                                       const long long* y_off, const long long* c_off, int16_t* Ypacked, size_t y_elems, int16_t* Cpacked,
                                       size_t c_elems, int32_t* status, int32_t* path, uint32_t* walked, uint32_t* seg_live, void* scratch,
                                       size_t scratch_bytes, int seg_bits, int rounds, void* stream);

/* Entropy ENCODING on the device (csrc/jpeg_emit.h, jpeg_encode.hip): from the int16 coefficient tensors back to whole files, SOI to
 * EOI.  The file is the one libjpeg's jpeg_write_coefficients writes with its defaults, byte for byte (the reference's
 * write_coefficients, dct_manip.cpp:265-313): SOI, APP0 JFIF 1.01, one 8-bit DQT segment per table (table 0 luma, table 1 BOTH chroma
 * planes), SOF0 (ids 1 2 3, sampling 22 11 11, or one component 11), the T.81 Annex K Huffman tables as four (two) DHT segments,
 * DRI when restart != 0, SOS, the interleaved scan, EOI.  A luma block of the MCU padding beyond the kept grid is coded with zero AC
 * and the DC of the block before it in its MCU, as libjpeg's transcoder fills it.
 *   Y, CbCr   device int16 [n][Hb][Wb][64], [n][2][Hbc][Wbc][64] (16-byte aligned), natural order; CbCr NULL: one component.
 *             Three components need Hbc = ceil(Hb / 2), Wbc = ceil(Wb / 2); grids 1..4096 with at most 2^32 / 1660 blocks per image
 *   quant     device int16 [n][C][64], natural order, C = 3 or 1: the layout the decode writes; tables 0 and 1 are used
 *   dims      device int32 [n][2]: height, width in pixels; the kept grids of that size must be the call's (else RGBNM_JPEG_EGRID)
 *   restart   restart interval in MCUs, 0..65535 (0: no DRI, no RSTn); a value above the MCU count is written to DRI and has one run
 *   out       device uint8 [n][stride]: each file from SOI on         nbytes  device int32 [n]: the file's size, 0 for a failed image
 *   status    device int32 [n], written for every image: 0, RGBNM_JPEG_ERANGE, RGBNM_JPEG_ECAPACITY (the file is longer than
 *             stride; rgbnm_jpeg_encode_bound always suffices) or RGBNM_JPEG_EGRID.  A failed image's slot of `out` is not touched
 *             and the other images are unaffected
 *   scratch   device memory, 16-byte aligned, at least rgbnm_jpeg_encode_scratch_bytes(...) bytes; nothing is kept between calls
 * Four launches whatever n and the data (measure, place, emit, stuff: csrc/jpeg_encode.hip); no allocation, no copy, no
 * synchronisation: capturable.  The bytes are the same on every run: shared words are merged by integer OR.  Every store is checked
 * against its buffer and every loop is bounded by the grid or by counts the kernels computed.  Option "jpeg_encode_wgs" caps the
 * workgroups per launch.  RGBNM_EINVAL with nothing launched: a NULL pointer other than CbCr, n <= 0, grids or restart out of
 * range, stride 0 or >= 2^31, misaligned pointers, scratch too small.
 * rgbnm_jpeg_encode_bound: the worst-case file size for a grid (every block at its 1660 bits, every scan byte stuffed); 0 for
 * arguments the encode refuses.  rgbnm_jpeg_encode_scratch_bytes: 0 likewise, or for n <= 0 or stride 0.  rgbnm_jpeg_encode_header:
 * the header bytes (SOI through the SOS header) of one image, written to out[cap]; returns their count (623 / 328, + 6 with DRI), or
 * RGBNM_EINVAL (NULL, ncomp not 1 or 3, a size outside 1..65535, a quant value outside 1..255, restart out of range, cap too small);
 * quant is host int16 [ncomp][64].  The kernel writes the same bytes from the same code.  All three are host only: no HIP call. */
size_t rgbnm_jpeg_encode_bound(int Hb, int Wb, int Hbc, int Wbc, int ncomp, int restart);
size_t rgbnm_jpeg_encode_scratch_bytes(int n, int Hb, int Wb, int Hbc, int Wbc, int ncomp, int restart, size_t stride);
int rgbnm_jpeg_encode_header(int ncomp, int height, int width, const int16_t* quant, int restart, uint8_t* out, size_t cap);
int rgbnm_jpeg_encode_batch(const int16_t* Y, const int16_t* CbCr, const int16_t* quant, const int32_t* dims, int n, int Hb, int Wb,
                            int Hbc, int Wbc, int restart, uint8_t* out, size_t stride, int32_t* nbytes, int32_t* status,
                            void* scratch, size_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Train-step tail
 * ------------------------------------------------------------------------------------------- */
/* CrossEntropyLoss (pipeline_utils.py:535) with soft [B,C] fp32 or hard int64 [B] targets (exactly one non-NULL).
 * loss[0] = mean over rows; dlogits (dtype dl_dtype, may be NULL) = d loss / d logits * grad_scale*B... see .hip:
 * dlogits = (softmax*sum(t) - t) * grad_scale, pass grad_scale = 1/B for the mean reduction.
 * Hard labels must lie in [0, C): the kernels do not check them.  A label outside that range matches no class, so its row has
 * target mass 0, loss row 0 and dlogits 0 (with mixing: the in-range partner alone counts) and no memory outside the row is
 * touched.  That is the contract of all three entry families (checking on the host would cost the step a device sync). */
int rgbnm_softxent(int dl_dtype, const float* logits, const float* soft_target, const long long* hard_target,
                   float* loss_rows, float* loss, void* dlogits, int B, int C, float grad_scale, void* stream);
/* The same loss as one launch per direction (round 6).  _loss: loss_rows [B], row_stats [2B] (log-sum-exp, target mass per row)
 * and loss[0] = the mean in ONE launch: the workgroup that finishes last sums the rows in a fixed order; `ticket` is one zeroed
 * 32-bit word of caller-owned device memory that the launch leaves zero again (one ticket per stream that may run the call).
 * _grad: dlogits (dl_dtype) = (softmax * sum(t) - t) * grad_scale * gout_dev[0] from the saved row statistics; gout_dev (device,
 * may be NULL = 1) is autograd's output gradient of the loss (GradScaler's scale under fp16 AMP, train.py:159): no host sync and
 * no element-wise launches to scale or convert it. */
int rgbnm_softxent_loss(const float* logits, const float* soft_target, const long long* hard_target, float* loss_rows,
                        float* row_stats, float* loss, unsigned* ticket, int B, int C, void* stream);
int rgbnm_softxent_grad(int dl_dtype, const float* logits, const float* soft_target, const long long* hard_target,
                        const float* row_stats, const float* gout_dev, void* dlogits, int B, int C, float grad_scale, void* stream);
/* The same two launches on the target RandomMixup_DCT would have built (cls_transforms.py:163-176: one-hot labels, rolled by one, mixed
 * with lam): target[b][c] = (labels[b] == c ? lam[0] : 0) + (labels[b-1] == c ? lam[1] : 0) is evaluated where it is used, the
 * dense [B, C] target and the launch that writes it do not exist (cls_transforms.LazyTarget).  Same bits as rgbnm_mixup_target
 * followed by rgbnm_softxent_loss / _grad on its output. */
int rgbnm_softxent_loss_mix(const float* logits, const long long* labels, const float* mix_lam_dev, float* loss_rows,
                            float* row_stats, float* loss, unsigned* ticket, int B, int C, void* stream);
int rgbnm_softxent_grad_mix(int dl_dtype, const float* logits, const long long* labels, const float* mix_lam_dev,
                            const float* row_stats, const float* gout_dev, void* dlogits, int B, int C, float grad_scale,
                            void* stream);
/* RandomMixup_DCT (cls_transforms.py:163-176): out[b] = lam[0]*in[b] + lam[1]*in[b-1]; lam on device. */
int rgbnm_mixup(int in_dtype, int out_dtype, const void* in, void* out, const float* lam_dev, int B,
                long long per_sample, void* stream);
/* rgbnm_mixup's contract with fp16: fp32 -> fp32 / bf16 and bf16 -> bf16 launch rgbnm_mixup's kernels (same bits); fp32 -> fp16
 * and fp16 -> fp16 store round_f16(fma(in[b-1], lam[1], in[b] * lam[0])) -- fp32 product, fp32 fma, ONE rounding, the expression of
 * rgbnm_subblock_embed_mix.  Every other pair, and per_sample % 4 != 0, returns RGBNM_EINVAL. */
int rgbnm_mixup_any(int in_dtype, int out_dtype, const void* in, void* out, const float* lam_dev, int B,
                    long long per_sample, void* stream);
int rgbnm_mixup_target(const long long* labels, float* target, const float* lam_dev, int B, int C, void* stream);
/* clip_grad_norm_(max_norm) + AdamW(weight_decay=0) + WeightDecay (train.py:163-165; custom_optims.py:37-42)
 * over flat fp32 buffers of n elements (n % 256 == 0; every tensor starts on a 256-element boundary);
 * wd_flag_per_256[i] != 0 marks chunks that belong to a decayed tensor; wd_factor = (lr/base_lr)*wd.
 * step = 1-based Adam step.  norm_out (may be NULL) receives the pre-clip global norm. max_norm<=0: no clip. */
size_t rgbnm_clip_adamw_wd_workspace(void);
int rgbnm_clip_adamw_wd_step(float* p, const float* g, float* m, float* v, const unsigned char* wd_flag_per_256,
                             long long n, float lr, float beta1, float beta2, float eps, int step, float wd_factor,
                             float max_norm, float* norm_out, void* workspace, size_t workspace_bytes, void* stream);
/* The same tail for float16 training under a loss scale that lives on the device: what the reference's default AMP step does
 * around its optimizers (utils/configs.py:18, 37-40: AMPDTYPE fp16, GradScaler(1.6, 0.625, 600); pipeline_utils.py:541; train.py:
 * 160-167: scale(loss).backward(), unscale_, clip_grad_norm_, step, step, update(); pipeline_utils.py:399-409: clip_gradscaler to
 * [2^-4, 2^18]) inside the tail's two launches, with no host sync and never a third launch.
 * The state block is caller-owned device memory, written by the second launch only, with ordinary stores: */
typedef struct rgbnm_loss_scale_state {
  float scale;         /* current loss scale: what the loss was multiplied by, what the gradients in g carry */
  int growth_tracker;  /* unskipped steps since the last change of the scale (GradScaler._growth_tracker) */
  int step;            /* Adam steps actually taken: the step a call takes is step + 1 */
  int skipped;         /* running total of skipped steps */
  float found_inf;     /* 0 or 1, of the latest call */
  int reserved[3];     /* bias corrections need no state: they are an fp64 pow of beta and step + 1 on the device */
} rgbnm_loss_scale_state;
/* rgbnm_clip_adamw_wd_step's arguments without `step`, then the state and the scaler's constants.
 * Launch 1 reads scale, forms inv = (float)(1.0 / (double)scale) (GradScaler.unscale_'s reciprocal) and sums (g inv)^2 in the order
 * of the unscaled entry; it leaves inv, step, scale and the bias corrections of step + 1 (bc1 = (float)(1 - beta1^t), bc2_sqrt =
 * (float)sqrt(1 - beta2^t), fp64 pow on the device: the expressions of the unscaled entry's host code) in the workspace.
 * Launch 2 reads those from the workspace only.  Total norm non-finite: p, m, v are not written, skipped += 1, found_inf = 1,
 * scale = (float)((double)scale * backoff_factor), growth_tracker = 0.  Otherwise g' = (g inv) coef (two roundings, unscale
 * first), then the arithmetic of the unscaled entry; step += 1, found_inf = 0, growth_tracker += 1, and when it reaches
 * growth_interval: scale = (float)((double)scale * growth_factor) if that is finite, growth_tracker = 0 -- the arithmetic of
 * torch._amp_update_scale_.  Then scale is clamped to [scale_min, scale_max].  norm_out (may be NULL) receives the norm of the
 * UNSCALED gradients (non-finite on a skipped step).
 * RGBNM_EINVAL for a NULL pointer (norm_out excepted), n <= 0 or n % 256 != 0, growth_interval < 1, a factor that is not > 0,
 * scale_min > scale_max (or either NaN); RGBNM_EWORKSPACE for a short workspace: nothing is launched, the state is untouched. */
size_t rgbnm_clip_adamw_wd_scaled_workspace(void);
int rgbnm_clip_adamw_wd_step_scaled(float* p, const float* g, float* m, float* v, const unsigned char* wd_flag_per_256,
                                    long long n, float lr, float beta1, float beta2, float eps, float wd_factor, float max_norm,
                                    float* norm_out, rgbnm_loss_scale_state* state, double growth_factor, double backoff_factor,
                                    int growth_interval, float scale_min, float scale_max, void* workspace,
                                    size_t workspace_bytes, void* stream);
/* The scaled tail with the learning-rate schedule on the device as well: what train.py's loop does around it with a host
 * scheduler (train.py:149-152 warm-up, 174-176 scheduler.step(); custom_optims.py:37-42 reads group['lr'] / group['base_lr']).
 * lr and wd_factor leave the argument list, so no argument of the two launches changes between steps and a captured call
 * (hipGraph) replays correctly.  The schedule has a state block of its own, caller-owned device memory, written by the second
 * launch only, with ordinary stores: */
typedef struct rgbnm_lr_sched_state {
  int iter;            /* calls seen so far, skipped steps included: the index the NEXT call looks up */
  float lr;            /* the lr the latest call used (logging) */
  float wd_factor;     /* the wd_factor the latest call used (logging) */
  int reserved[5];
} rgbnm_lr_sched_state;
/* rgbnm_clip_adamw_wd_step_scaled with (lr, wd_factor) replaced by (lr_table, table_len, base_lr, weight_decay) and `sched` behind
 * `state`.  lr_table is device memory of table_len doubles; entry k is the host scheduler's param_groups[0]['lr'] at the
 * optimizer.step() of iteration k.  Launch 1 additionally reads sched->iter, takes k = min(iter, table_len - 1), lr_d = lr_table[k]
 * and leaves lr = (float)lr_d, wd_factor = (float)((lr_d / base_lr) * weight_decay) (one fp64 divide, one fp64 multiply, one
 * rounding: the host expression of the scaled entry's caller) and iter in the workspace, next to inv, step, scale and the bias
 * corrections.  Launch 2 reads them from the workspace only and performs the scaled entry's arithmetic: same bits as
 * rgbnm_clip_adamw_wd_step_scaled called with those two floats.  Its workgroup 0 then writes sched->iter = iter + 1, sched->lr and
 * sched->wd_factor -- on a skipped step too (the reference steps its scheduler every iteration); state->step keeps its rule.
 * RGBNM_EINVAL for what the scaled entry refuses, a NULL lr_table or sched, table_len < 1, base_lr not > 0, weight_decay NaN or
 * < 0; RGBNM_EWORKSPACE for a short workspace: nothing is launched, both state blocks are untouched. */
size_t rgbnm_clip_adamw_wd_sched_workspace(void);
int rgbnm_clip_adamw_wd_step_sched(float* p, const float* g, float* m, float* v, const unsigned char* wd_flag_per_256,
                                   long long n, const double* lr_table, int table_len, double base_lr, double weight_decay,
                                   float beta1, float beta2, float eps, float max_norm, float* norm_out,
                                   rgbnm_loss_scale_state* state, rgbnm_lr_sched_state* sched, double growth_factor,
                                   double backoff_factor, int growth_interval, float scale_min, float scale_max, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Composite stages: one call per autograd node (ViT, plainvit.py:559-611)
 * ------------------------------------------------------------------------------------------- */
typedef struct rgbnm_vit_cfg {
  int dtype, B, N, E, heads;
  float ln_eps, attn_scale;
} rgbnm_vit_cfg;

typedef struct rgbnm_block_params {      /* TransformerEncoderBlock, plainvit.py:493-529 */
  const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  const float *bqkv_perm, *bproj, *b1, *b2;
  const void *wqkv, *wqkv_t, *wproj, *wproj_t, *w1, *w1_t, *w2, *w2_t;
} rgbnm_block_params;

typedef struct rgbnm_block_acts {        /* saved for backward; caller-owned */
  void* x_in;   /* [M,E]   block input (residual stream)   */
  void* xn1;    /* [M,E]   LN1 output                      */
  float *mean1, *rstd1;
  void* qkv;    /* [M,3I]  q|k|v                           */
  float* lse;   /* [B*heads*N]                             */
  void* attn;   /* [M,I]   merged heads, pre-projection    */
  void* x_mid;  /* [M,E]   after attention residual        */
  void* xn2;    /* [M,E]                                   */
  float *mean2, *rstd2;
  void* u;      /* [M,4E]  gelu'(fc1 pre-activation)       */
  void* gl;     /* [M,4E]  gelu(u)                         */
  void* x_out;  /* [M,E]                                   */
} rgbnm_block_acts;

typedef struct rgbnm_block_grads {       /* fp32, reference layouts */
  float *dln1_g, *dln1_b, *dln2_g, *dln2_b;
  float *dwqkv, *dbqkv, *dwproj, *dbproj, *dw1, *db1, *dw2, *db2;
} rgbnm_block_grads;

typedef struct rgbnm_block_scratch {     /* backward temporaries, caller-owned, reusable across blocks */
  void* du;      /* [M,4E] */
  void* dxn;     /* [M,E]  */
  void* dx_mid;  /* [M,E]  */
  void* dattn;   /* [M,I]  */
  void* dqkv;    /* [M,3I] */
  void* ws;      /* generic workspace */
  size_t ws_bytes;
} rgbnm_block_scratch;

size_t rgbnm_vit_workspace(const rgbnm_vit_cfg* cfg);                      /* heads of up to 1024 classes */
size_t rgbnm_vit_workspace_ex(const rgbnm_vit_cfg* cfg, int n_classes);    /* any head width (n_classes % 8 == 0) */
int rgbnm_vit_block_fwd(const rgbnm_vit_cfg* cfg, const rgbnm_block_params* p, const rgbnm_block_acts* a,
                        void* stream);
/* Chained forward over consecutive blocks: when rgbnm_vit_ln_chain(cfg) is 1 the epilogue of this block's fc2 can
 * also produce the NEXT block's LN1 (next_a->xn1 / mean1 / rstd1 from next_p->ln1_g / ln1_b; requires
 * next_a->x_in == a->x_out), and flags bit 0 tells a block that its own LN1 was produced that way and must be
 * skipped.  next_p / next_a may be NULL.  rgbnm_vit_block_fwd(cfg, p, a, s) == rgbnm_vit_block_fwd_chain(cfg, p, a, 0,
 * NULL, NULL, s).  (LayerNorm stays reference arithmetic; only the launch and one read of x are saved.) */
int rgbnm_vit_ln_chain(const rgbnm_vit_cfg* cfg);
int rgbnm_vit_block_fwd_chain(const rgbnm_vit_cfg* cfg, const rgbnm_block_params* p, const rgbnm_block_acts* a,
                              int flags, const rgbnm_block_params* next_p, const rgbnm_block_acts* next_a,
                              void* stream);
/* dy = grad wrt x_out, dx = grad wrt x_in (dx may alias dy). */
int rgbnm_vit_block_bwd(const rgbnm_vit_cfg* cfg, const rgbnm_block_params* p, const rgbnm_block_acts* a,
                        const rgbnm_block_grads* g, const rgbnm_block_scratch* s, const void* dy, void* dx,
                        void* stream);

/* Encoder block with dropout p > 0 (training; reference: eb_drop1, the FeedForwardBlock's nn.Dropout and eb_drop2 of
 * plainvit.py:485-529, all p = drop_p).  The forward runs LN1, qkv and attention as rgbnm_vit_block_fwd, then proj with
 * RGBNM_EPI_RES_DROP (site 0), LN2, fc1 with RGBNM_EPI_GELU_DROP (site 1: a->gl and a->u hold the masked gelu / gelu') and fc2 with
 * RGBNM_EPI_RES_DROP (site 2); no LayerNorm chaining, no fused MLP.  The backward regenerates the masks from the same seed:
 * dy_m = mask2(dy) feeds dW2 / db2 and d(gl), dxmid_m = mask0(d x_mid) feeds dWproj / dbproj and d(attn); the residual paths keep
 * the unmasked gradients.  dy_m / dxmid_m: caller-owned [M,E] buffers of the compute dtype (backward only), alive until the call
 * returns.  No mask is stored.
 * Both entries check d before they enqueue anything: a NULL d, seed, dy_m or dxmid_m (backward), dy_m == dxmid_m, p outside [0, 1)
 * or block < 0 return RGBNM_EINVAL, a short workspace RGBNM_EWORKSPACE, with no kernel launched. */
typedef struct rgbnm_dropout {
  const void* seed;   /* device pointer to the step's 64-bit seed */
  float p;            /* [0, 1) */
  int block;          /* encoder block index (counter word 2 = block * 4 + site) */
  void *dy_m, *dxmid_m;
} rgbnm_dropout;
int rgbnm_vit_block_fwd_drop(const rgbnm_vit_cfg* cfg, const rgbnm_block_params* p, const rgbnm_block_acts* a,
                             const rgbnm_dropout* d, void* stream);
int rgbnm_vit_block_bwd_drop(const rgbnm_vit_cfg* cfg, const rgbnm_block_params* p, const rgbnm_block_acts* a,
                             const rgbnm_block_grads* g, const rgbnm_block_scratch* s, const rgbnm_dropout* d, const void* dy,
                             void* dx, void* stream);

/* ---- The whole encoder forward as ONE launch, one workgroup per image (csrc/vit_chain.hip) --------------------------------
 * Reference: the `depth` TransformerEncoderBlocks of models/plainvit.py:493-529 applied in sequence (:601-611).  bf16, E = 192,
 * 3 heads, 196 tokens (JPEG-Ti); needs rgbnm_gelu_table_init on the device.  The residual stream, LayerNorm outputs, q and the
 * attention output stay in registers, K / V of one head in LDS; every tensor the backward reads (rgbnm_block_acts) is written
 * exactly as rgbnm_vit_block_fwd writes it, so rgbnm_vit_block_bwd runs unchanged behind it.
 * rgbnm_chain_block: one block's parameters and outputs (device pointers); `blocks` is a HOST array of `depth` (<= 12) of them,
 *   copied into the kernel's argument segment (no upload: the call may be captured into a HIP graph).  x_in of block 0 is the
 *   x0 argument; block i's x_out is block i + 1's input.
 * wimg: the block's "chain image" -- its four weight matrices as they lie in LDS (rows permuted, 16-byte chunks swizzled,
 *   consumption order), rgbnm_chain_image_elems() bf16 elements, written per step by rgbnm_chain_gather(src = operand shadows,
 *   idx = constant int32 table built on the host: rgb-no-more_amd/chain.py documents the layout).
 * Returns RGBNM_OK, 1 when the configuration is not eligible (the caller runs the blocks one by one), or a negative error.
 * Not eligible: anything but bf16, E = 192, 3 heads, N = 196, B >= 1, depth <= 12, or no GELU table on the device.  A NULL cfg /
 * blocks / x0 or depth <= 0 is RGBNM_EINVAL.  Both are decided before anything is launched: the call has then touched no buffer
 * (tests/test_block_edges.py), so the caller can run the per-operation entries on the same arguments. */
typedef struct rgbnm_chain_block {
  const void* wimg;
  const float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *bqkv_perm, *bproj, *b1, *b2;
  void* xn1; float *mean1, *rstd1;
  void* qkv; float* lse; void* attn; void* x_mid; void* xn2; float *mean2, *rstd2;
  void* u; void* gl; void* x_out;
} rgbnm_chain_block;
size_t rgbnm_chain_block_bytes(void);          /* sizeof(rgbnm_chain_block) as the library was built */
long long rgbnm_chain_image_elems(void);       /* bf16 elements of one block's chain image */
int rgbnm_chain_gather(const void* src, const int* idx, void* dst, long long n, void* stream);   /* dst[i] = src[idx[i]], bf16, n % 8 == 0 */
int rgbnm_vit_chain_fwd(const rgbnm_vit_cfg* cfg, const rgbnm_chain_block* blocks, int depth, const void* x0, void* stream);

/* ---- The data path of the whole encoder BACKWARD as ONE launch, one workgroup per image (csrc/vit_chain_bwd.hip) -----------
 * Reference: the backward of the same `depth` blocks as autograd runs it (models/plainvit.py:493-529).  For every block, last to
 * first: du = (dy . W2) * gelu'(u), d(x_mid) = dy + LN2'(du . W1), d(attention output) = d(x_mid) . Wproj, attention backward,
 * dx = d(x_mid) + LN1'(d(qkv) . Wqkv) -- the kernels rgbnm_vit_block_bwd launches one by one, same arithmetic, same bits.  It
 * leaves du / dx_mid / dqkv / dx of EVERY block in the caller's buffers (operands of the weight-gradient GEMMs) and the
 * per-image partial sums of the LayerNorm parameter gradients in part2 / part1 ([B][2][192] each: d(gamma) | d(beta)); the caller
 * then runs rgbnm_vit_block_bwd_dw per block (any order), which launches the four weight-gradient GEMMs and submits the
 * reductions exactly as rgbnm_vit_block_bwd does.  blocks: HOST array of `depth` (<= 12) rgbnm_chain_bwd_block (copied into the
 * kernel's argument segment); blk[i].dy must be blk[i + 1].dx for i < depth - 1.  wimg: the backward chain image (rgb-no-more_amd/chain.py, from the TRANSPOSED operand
 * shadows by rgbnm_chain_gather).  dattn: [B * 196, 192] scratch.  Returns RGBNM_OK, 1 = not eligible, negative = error; the
 * same contract as rgbnm_vit_chain_fwd (it does not need the GELU table): 1 or RGBNM_EINVAL (NULL cfg / blocks / dattn, depth <= 0)
 * means that nothing was launched and no buffer was touched. */
typedef struct rgbnm_chain_bwd_block {
  const void* wimg;
  const float *ln1_g, *ln2_g;
  const void* x_in; const float *mean1, *rstd1;
  const void* qkv; const float* lse; const void* attn; const void* x_mid; const float *mean2, *rstd2; const void* u;
  const void* dy;
  void* du; void* dx_mid; void* dqkv; void* dx;
  float *part2, *part1;
} rgbnm_chain_bwd_block;
size_t rgbnm_chain_bwd_block_bytes(void);
int rgbnm_vit_chain_bwd(const rgbnm_vit_cfg* cfg, const rgbnm_chain_bwd_block* blocks, int depth, void* dattn, void* stream);
/* The weight / bias / LayerNorm-parameter gradients of one block from what rgbnm_vit_chain_bwd left behind: the dW part of
 * rgbnm_vit_block_bwd (scratch->du / dx_mid / dqkv as filled by the chain kernel; dy = the block's output gradient). */
int rgbnm_vit_block_bwd_dw(const rgbnm_vit_cfg* cfg, const rgbnm_block_acts* a, const rgbnm_block_grads* g,
                           const rgbnm_block_scratch* s, const void* dy, const float* part2, const float* part1, void* stream);
/* The same for n <= 12 blocks in ONE grouped weight-gradient launch (arrays of n pointers; every block with its own workspace
 * scratch[i]->ws): the 4 n GEMMs share the 256 workgroups, so the token axis is split 256 / (21 n) ways instead of 12 -- all twelve
 * blocks of JPEG-Ti: no split, no fp32 partial sums to write and re-read. */
int rgbnm_vit_blocks_bwd_dw(const rgbnm_vit_cfg* cfg, int n, const rgbnm_block_acts* const* a, const rgbnm_block_grads* const* g,
                            const rgbnm_block_scratch* const* s, const void* const* dy, const float* const* part2,
                            const float* const* part1, void* stream);
/* ... and the patch embedding's weight gradient (what rgbnm_patch_embed_bwd computes: pe_dw [E,384] / pe_db [E] = pe_dx0^T . pe_feat
 * over the same token axis; pe_dx0 = the gradient rgbnm_vit_chain_bwd left for block 0's input) as one more job of the same
 * grouped launch -- 252 + 4 = 256 output tiles at JPEG-Ti's B = 256: still no token split.  pe_dx0 NULL = the call above. */
int rgbnm_vit_blocks_bwd_dw_pe(const rgbnm_vit_cfg* cfg, int n, const rgbnm_block_acts* const* a, const rgbnm_block_grads* const* g,
                               const rgbnm_block_scratch* const* s, const void* const* dy, const float* const* part2,
                               const float* const* part1, const void* pe_dx0, const void* pe_feat, float* pe_dw, float* pe_db,
                               void* pe_ws, size_t pe_ws_bytes, void* stream);

/* Table GELU of the bf16 path (csrc/mlp_fused.hip): in bf16 mode the pre-activation is rounded to bf16 before the GELU
 * (models/plainvit.py:487-488 under autocast), so gelu / gelu' are functions of 16 bits.  _init is a SET-UP call (it
 * synchronises `stream`; not capturable; idempotent per device): it builds the table of the library's own GELU arithmetic for
 * all 65536 inputs plus a compact LDS image of it, and reads the window back.  On devices where it has been called and the
 * image fits, the fused FeedForwardBlock forward looks gelu / gelu' up instead of computing them (option gelu_table) -- the
 * same bits as the arithmetic for every finite input except those whose u or u / 2 is a bf16 denormal (|u| < 2.36e-38), which
 * give a denormal of the right sign instead of u / 2.  Non-finite inputs: a NaN gives a NaN gelu and +inf gives +inf, as the
 * arithmetic does; gelu' and -inf differ (lookup: gelu(-inf) = -0, gelu' = 1 / 0 beyond the window; arithmetic: NaN).  Never
 * called: the arithmetic runs.
 * _info (test / diagnostics, synchronises): win16 = {valid, A0, P1, N1, image dwords, ...}, full65536 (may be NULL) =
 * gelu(u) | gelu'(u) << 16 per bf16 bit pattern u. */
int rgbnm_gelu_table_init(void* stream);
int rgbnm_gelu_table_info(int* win16, unsigned* full65536);

/* Held gradient reductions.  Every backward entry point of this header (rgbnm_vit_block_bwd, rgbnm_head_bwd,
 * rgbnm_patch_embed_bwd, rgbnm_gemm_tn, rgbnm_layernorm_bwd, ...) finishes with a small reduction of its split partial
 * sums (reference: autograd accumulates straight into .grad, models/plainvit.py runs under torch.autograd).  A caller that
 * reads no gradient before the END of the backward pass -- one GPU, or one all-reduce after the pass -- may bracket the pass:
 *   rgbnm_reduce_hold_begin();  ... backward calls, each with ITS OWN workspace region ...
 *   rgbnm_reduce_hold_end(table, table_host, rgbnm_reduce_hold_table_bytes(), stream);
 * and all reductions issued in between (on this host thread) run as ONE launch at _end, with the same summation order (same
 * bits).  `table` is a device buffer and `table_host` a HOST buffer of the same size, both owned by the caller, allocated
 * together (table_host zero-filled) and freed together, untouched between steps: table_host records what the device table
 * holds, and the job table is uploaded only when it differs from that record (so a graph capture of a steady-state pass
 * contains no copy; a pass whose table changed while the stream is capturing is captured WITH its upload when table_host is
 * page-locked -- the copy node reads table_host at every replay, so it must stay untouched while the graph lives -- and returns
 * RGBNM_EINVAL when it is pageable).  The partial sums live in
 * the workspaces until _end: regions must not be shared between the calls of one bracket.  One bracket per host thread:
 * _begin inside an open bracket returns RGBNM_EINVAL.  rgbnm_reduce_hold_cancel() leaves the mode without running anything
 * (error paths). */
int rgbnm_reduce_hold_begin(void);
int rgbnm_reduce_hold_end(void* table, void* table_host, size_t table_bytes, void* stream);
void rgbnm_reduce_hold_cancel(void);
size_t rgbnm_reduce_hold_table_bytes(void);

/* PatchEmbedding_DCT_Group (plainvit.py:157-218): feat = subblock(y,cbcr); x0 = feat.Wpe^T + b + sincos */
int rgbnm_patch_embed_fwd(const rgbnm_vit_cfg* cfg, int in_dtype, const void* y, const void* cbcr,
                          const float* conv16, const void* wpe, const float* bpe, const float* pos, void* feat,
                          void* x0, int Hb, int Wb, void* stream);
/* ... with the batch mixup applied on the way in (rgbnm_subblock_embed_mix; lam_dev NULL = rgbnm_patch_embed_fwd) */
int rgbnm_patch_embed_fwd_mix(const rgbnm_vit_cfg* cfg, int in_dtype, const void* y, const void* cbcr, const float* lam_dev,
                              const float* conv16, const void* wpe, const float* bpe, const float* pos, void* feat, void* x0,
                              int Hb, int Wb, void* stream);
int rgbnm_patch_embed_bwd(const rgbnm_vit_cfg* cfg, const void* dx0, const void* feat, float* dwpe, float* dbpe,
                          void* ws, size_t ws_bytes, void* stream);

typedef struct rgbnm_head_params {       /* ClassificationHead, plainvit.py:542-557 */
  const float *ln_g, *ln_b, *b1, *b2;
  const void *w1, *w1_t, *w2, *w2_t;
  int n_classes;
  int _pad;
} rgbnm_head_params;
typedef struct rgbnm_head_acts {
  void* x;        /* [M,E] encoder output */
  float *mean, *rstd;
  void* pooled;   /* [B,E] */
  void* h1;       /* [B,E] tanh output */
  float* logits;  /* [B,C] fp32 */
} rgbnm_head_acts;
typedef struct rgbnm_head_grads {
  float *dln_g, *dln_b, *dw1, *db1, *dw2, *db2;
} rgbnm_head_grads;
int rgbnm_head_fwd(const rgbnm_vit_cfg* cfg, const rgbnm_head_params* p, const rgbnm_head_acts* a, void* stream);
/* dlogits [B,C] in cfg->dtype; da, dpooled: [B,E] scratch; dx [M,E] out.
 * n_classes: rgbnm_head_fwd takes any C >= 1; rgbnm_head_bwd reads dlogits as a GEMM operand of row pitch C and needs whole 16-byte
 * rows, C % 8 == 0 in the 16-bit modes and C % 4 == 0 in fp32 -- any other C returns RGBNM_EINVAL before anything is launched
 * (callers pad the head: plainvit.py _ncls_pad). */
/* Workspace that lets rgbnm_head_bwd keep its three sets of split partial sums side by side (REQUIRED when the call sits inside
 * a rgbnm_reduce_hold_begin / _end bracket: with less the call returns RGBNM_EWORKSPACE there and launches nothing, because the
 * held reductions would read a region the later producers have overwritten; outside a bracket any workspace that holds the
 * largest of the three regions -- rgbnm_gemm_tn_workspace(B, C, E), rgbnm_gemm_tn_workspace(B, E, E), B 2 E floats; also
 * rgbnm_vit_workspace_ex where that is the smaller one -- is re-used by the three producers one after the other). */
size_t rgbnm_head_bwd_workspace(const rgbnm_vit_cfg* cfg, int n_classes);
int rgbnm_head_bwd(const rgbnm_vit_cfg* cfg, const rgbnm_head_params* p, const rgbnm_head_acts* a,
                   const rgbnm_head_grads* g, const void* dlogits, void* da, void* dpooled, void* dx, void* ws,
                   size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SwinV2 DCT (models/swinv2.py; BASELINE config 5) - the parts that are not plain Linears (those use rgbnm_gemm_nt/tn).
 * dtype of the entries below: RGBNM_DT_F32, RGBNM_DT_BF16 or RGBNM_DT_F16 (the position-bias entries are fp32 only).
 * ------------------------------------------------------------------------------------------- */
/* PatchEmbedding_DCT_Group with patch 4 (swinv2.py:505-576, plainvit.py:50-88): every 8x8 block is decomposed,
 * X' = A^T X A with convY = conversion_matrix(4,2) / convC = conversion_matrix(2,4) (8x8 fp32 each), tokens on the
 * 2Hb x 2Wb grid, feat [B, 2Hb*2Wb, 24] = Y 4x4 | Cb 2x2 | Cr 2x2 (einops split '(p1 pdh)(p2 pdw)', coefficient-major). */
int rgbnm_swin_embed(int in_dtype, int out_dtype, const void* y, const void* cbcr, const float* convY, const float* convC,
                     void* feat, int B, int Hb, int Wb, void* stream);
/* LayerNorm of any width E % 4 == 0, E <= 768:  y = [res +] [sample_scale[row / rows_per_sample] *] LN(x)
 * (res-post-norm + DropPath scale, swinv2.py:302-307).  Backward: dx = LN'(scale * dy), dgamma / dbeta fp32. */
int rgbnm_ln_generic_fwd(int dtype, const void* x, const float* gamma, const float* beta, const void* res,
                         const float* sample_scale, int rows_per_sample, void* y, float* mean, float* rstd, int M, int E,
                         float eps, void* stream);
size_t rgbnm_ln_generic_bwd_workspace(int M, int E);
int rgbnm_ln_generic_bwd(int dtype, const void* dy, const void* x, const float* gamma, const float* mean,
                         const float* rstd, const float* sample_scale, int rows_per_sample, void* dx, float* dgamma,
                         float* dbeta, int M, int E, int accumulate, void* workspace, size_t workspace_bytes,
                         void* stream);
/* WindowAttention + cyclic shift + window partition / reverse (swinv2.py:143-182, 273-300) on token-major tensors:
 * qkv [B, res*res, 3C] (q | k | v, heads of 32), bias [heads, 64, 64] fp32 (= 16 sigmoid(cpb_mlp(table))[index]),
 * scale [heads] fp32 (= exp(min(logit_scale, ln 100))), 0 <= shift < 8 (the model uses 0 and 4; else RGBNM_EINVAL): window 8x8,
 * cosine attention, shift mask -100.
 * out [B, res*res, C]; lse [B * nW * heads * 64] saved for backward.  Backward writes dbias (per-wave partials in the
 * workspace, deterministic reduction), one partial d(scale) per (window, head) into dscale_part [B * nW * heads] and -- when
 * dscale is not NULL -- their sum into dscale [heads] (a job of the same batched reduction).
 * Normalisation contract, forward and backward: q^ = q / max(|q|, eps), eps = 1e-12 as F.normalize, for rows with |q|^2 finite in
 * fp32 (likewise k).  A row with |q| < eps is scaled by 1 / eps (an all-zero row stays zero) and its gradient is
 * dq = dq^ / eps WITHOUT the projection (I - q^ q^T): the clamp passes no gradient to the norm, as autograd of F.normalize;
 * every other row gets (I - q^ q^T) dq^ / |q|.  The kernel decides by its fp32 reciprocal norm reaching 1e12f, so rows whose norm
 * lies within fp32 rounding of eps may fall on either side.  Results that leave the element type's range (fp16: the 1 / eps of a
 * clamped row) are stored as +-inf. */
int rgbnm_window_attention_fwd(int dtype, const void* qkv, const float* bias, const float* scale, void* out, float* lse,
                               int B, int res, int C, int heads, int shift, void* stream);
size_t rgbnm_window_attention_bwd_workspace(int B, int res, int heads);
int rgbnm_window_attention_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* bias,
                               float* dscale /* [heads] or NULL */, const float* scale, const float* lse, void* dqkv,
                               float* dbias, float* dscale_part, int B, int res, int C, int heads, int shift, void* workspace,
                               size_t workspace_bytes, void* stream);
/* Continuous position bias + logit scale of EVERY WindowAttention of the model (swinv2.py:158-168: cpb_mlp on the 15 x 15
 * relative_coords_table, gathered by relative_position_index, 16 sigmoid; exp of the clamped logit_scale) in two launches per
 * direction.  blocks: HOST array (copied into the kernels' arguments; any count, heads <= 24).  Per block: w1 [512,2], b1 [512],
 * w2 [heads,512], ls [heads] fp32 parameters; forward writes bias [heads,64,64] and scale [heads]; backward reads dbias
 * [heads,64,64] and dscale [heads] and writes dw1, db1, dw2, dls.  coords [225,2] fp32; index [4096] int32 (= relative_position_index);
 * inv_index [225,64] int32: the positions that read each table entry, ascending, padded with 4096 (fixed summation order: run-to-run
 * identical bits).  table / dtable: caller-owned fp32 scratch of rgbnm_swin_cpb_table_elems(nblocks) elements; `table` carries the
 * forward's MLP outputs to the backward. */
typedef struct rgbnm_cpb_block {
  const float *w1, *b1, *w2, *ls;
  float *bias, *scale;
  const float *dbias, *dscale;
  float *dw1, *db1, *dw2, *dls;
  int heads, _pad;
} rgbnm_cpb_block;
size_t rgbnm_swin_cpb_table_elems(int nblocks);
int rgbnm_swin_cpb_fwd(const rgbnm_cpb_block* blocks, int nblocks, const float* coords, const int* index, float* table, void* stream);
int rgbnm_swin_cpb_bwd(const rgbnm_cpb_block* blocks, int nblocks, const float* coords, const int* inv_index, const float* table,
                       float* dtable, void* stream);
/* PatchMerging's concat (swinv2.py:357-362): [B, res*res, C] -> [B, (res/2)^2, 4C] (inverse != 0: the reverse copy). */
int rgbnm_merge_gather(int dtype, const void* in, void* out, int B, int res, int C, int inverse, void* stream);
/* mean over tokens [B,N,C] -> [B,C] (backward != 0: [B,C] -> [B,N,C], dy / N). */
int rgbnm_token_mean(int dtype, const void* in, void* out, int B, int N, int C, int backward, void* stream);


/* ---- calibration micro-kernels (measurement only, SURVEY.md section 8d: attainable peaks on the box) ----------------
 * rgbnm_calib_mfma_bf16: `workgroups` x 4 waves each issue iters x 4 independent 32x32x16 bf16 MFMAs (32768 flop each),
 * no memory traffic.  rgbnm_calib_stream: 16 B per lane grid-stride; mode 0 copy, 1 read-only, 2 write-only.
 * `sink` is a 4-byte device word that is never actually written. */
int rgbnm_calib_mfma_bf16(int workgroups, int iters, float* sink, void* stream);
int rgbnm_calib_stream(const void* src, void* dst, size_t bytes, int mode, int workgroups, void* sink, void* stream);
/* One wave issues 16 back-to-back 1 KB stores (mode 0) / loads (mode 1), 8 rows x 128 B at row stride ld bytes:
 * out[(wg * waves + w) * 2 + {0, 1}] = cycles to issue them / cycles until they have all completed. */
int rgbnm_calib_vmem_issue(int mode, int workgroups, int waves, void* buf, size_t wave_bytes, int ld,
                           unsigned long long* out, void* stream);
/* Every workgroup (`waves` waves) re-reads its own L2-resident slice of `slice_bytes` (a multiple of waves * 8 KB) `iters`
 * times: mode 0 plain 16-byte loads, mode 1 LDS-DMA.  Prices L2 -> CU traffic (weight re-streaming of the row-panel kernels). */
int rgbnm_calib_l2(const void* buf, size_t slice_bytes, int iters, int mode, int workgroups, int waves, void* sink,
                   void* stream);
/* What two waves of one SIMD share: wave w of a `waves`-wave workgroup (w and w + 4 share a SIMD) runs role_dev[w] for `iters`
 * rounds -- 0 idle, 1: 8 MFMAs (32x32x16 bf16, independent accumulators), 2: 64 v_fma_f32, 3: 32 v_pk_fma_f32, 4: 16 v_exp_f32 +
 * 16 v_rcp_f32, 5: 32 v_cvt_pk_bf16_f32, 6: 8 MFMAs and 64 v_fma_f32 in ONE stream; out[wg * waves + w] = cycles of the loop. */
int rgbnm_calib_pipes(const int* role_dev, int waves, int iters, int workgroups, unsigned long long* out, float* sink,
                      void* stream);

/* Stand-in for a collective's channels: `workgroups` x 256 threads, each holding `lds_bytes` of LDS, stay resident for `ticks`
 * s_memtime ticks (or until *stop != 0; stop may be NULL), re-reading their 4 KB-multiple slice of buf meanwhile (mode 1) or sleeping
 * (mode 0).  Measurement / test perturber only (tools/cu_steal_probe.py, tests/test_chain_soak.py). */
int rgbnm_calib_occupy(const void* buf, size_t slice_bytes, int workgroups, int lds_bytes, long long ticks, int mode,
                       const int* stop, void* sink, void* stream);
/* the same with a residency log (device memory, 3 x workgroups 64-bit words): [3 wg] = s_memrealtime (100 MHz) at the workgroup's
 * start, [3 wg + 1] at its end, [3 wg + 2] = (XCC id << 32) | HW_ID */
int rgbnm_calib_occupy_log(const void* buf, size_t slice_bytes, int workgroups, int lds_bytes, long long ticks, int mode,
                           const int* stop, void* sink, unsigned long long* log, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RGBNM_H */
