/* clover_hip.h — C ABI of libclover_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the Clover video-text pre-training hot path.  The
 * reference (LeeYN-43/Clover) is 100 % Python over torch/cuDNN/cuBLAS and has no
 * native FFI of its own; each entry point below replaces the torch op group that
 * the cited reference lines execute (paths relative to /root/reference/).  A
 * reference maintainer binds them with ctypes from the registered nn.Modules —
 * see INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers + sizes; no torch / C++ types cross the ABI;
 *   - every pointer is DEVICE memory unless its name ends in _host;
 *   - bf16 tensors are `void*` (uint16 storage), row-major, innermost contiguous;
 *   - `stream` is a hipStream_t passed as void*; all calls are asynchronous on it,
 *     allocate nothing, and are capturable into a hipGraph;
 *   - return 0 on success, negative CLV_ERR_* otherwise; no exceptions.  CLV_ERR_LAUNCH: a kernel launch, or the
 *     once-per-process opt-in of a kernel to more than 64 KB of dynamic LDS, failed;
 *   - the library reads three environment variables, each per call because tests flip them between two live paths:
 *     CLV_ATTN_BWD_ONE, CLV_GEMM_SPLITK, CLV_GEMM_ROT.  Every other choice — tile classes,
 *     grids, slice counts — is fixed at build time.
 */
#ifndef CLOVER_HIP_H
#define CLOVER_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLV_ABI_VERSION 20
#define CLV_ERR_ARG (-1)
#define CLV_ERR_UNSUPPORTED (-2)
#define CLV_ERR_LAUNCH (-3)

int clv_abi_version(void);
/* The 16-bit element type this build of the library computes in: 0 = bf16 (libclover_hip.so), 1 = IEEE fp16
 * (libclover_hip_f16.so: the same sources compiled with -DCLV_HALF_F16 — the reference's own arithmetic type,
 * configs/exp_local/pretrain_webvid_cc3m.py:21, mmaction/core/hooks/fp16_utils.py:215-259).  Every `bf16` in the comments
 * below reads "the library's 16-bit element type". */
int clv_half_type(void);

/* ------------------------------------------------------------------ attention
 * One kernel family serves both attention flavours of the path:
 *   mode 1: 3-D shifted-window MHA — WindowAttention3D.forward
 *           (mmaction/models/backbones/swin_transformer_3d.py:375-400) fused with
 *           the cyclic roll + window_partition before it (:459-466) and the
 *           window_reverse + un-roll after it (:470-476): q/k/v are read from, and
 *           o is written to, the natural [B,D,H,W,*] token layout;
 *   mode 0: full self-attention over [video ‖ text] / text with an additive key
 *           mask — transformers 4.6.1 BertSelfAttention as called from
 *           bert_from_hugface.py:30 and cross_transformer.py:109-110.
 * softmax( q·kᵀ·scale + bias[h][i][j] + (rid[i]!=rid[j] ? -100 : 0) + kmask[b][j] ) · v
 *
 * Relative-position bias (mode 1): the kernels take the TABLE, not a gathered [nH][N][N] tensor:
 *   bias[h][i][j] = table[ lin(i) - lin(j) + c ][h],   lin(n) = (n / (bwh*bww)) * (2bwh-1)(2bww-1)
 *                                                              + ((n / bww) % bwh) * (2bww-1) + n % bww
 * which is relative_position_bias_table[relative_position_index[:N,:N]] of :343-360,386 for the window
 * (bwd,bwh,bww) the table was built for (the module's full window_size; N may be a clipped window's
 * token count).  The head's table lives in LDS (2535 entries for (8,7,7)); the backward sums the per-window dS
 * over the windows and scatters the sums into d table — no gathered [nH][N][N] bias or bias gradient exists.
 */
typedef struct ClvAttnGeom {
    int32_t mode;           /* 0 sequence, 1 shifted 3-D window */
    int32_t groups;         /* B (mode 0) or B*nW (mode 1) */
    int32_t N;              /* tokens per group: S or wd*wh*ww */
    int32_t nH;             /* heads */
    int32_t hd;             /* head dim: 16, 32 or 64 */
    int32_t D, H, W;        /* mode 1: (padded) feature dims */
    int32_t wd, wh, ww;     /* mode 1: effective window (get_window_size, :302-315) */
    int32_t sd, sh, sw;     /* mode 1: effective shift */
    int32_t ldq, ldk, ldv, ldo; /* row strides (elements) of q,k,v and o/do/dq.. */
    int32_t bwd, bwh, bww;  /* window the bias table was built for: the table has (2bwd-1)(2bwh-1)(2bww-1) rows; 0,0,0 = none */
    float scale;            /* head_dim^-0.5 */
    float dropout_p;        /* dropout on the attention probabilities (HF attention_probs_dropout_prob), 0 = off */
    const int32_t* dbias_index; /* backward, optional: the device table clv_attn_dbias_index() built for this window
                                   geometry (N, bwd, bwh, bww) — the table-gradient gather then does no index arithmetic */
    void* work;                 /* mode 0 with 448 < N <= clv_attn_seq_max_keys() = 4096 (the 32-frame fusion sequence, 816
                                   tokens, cross_transformer.py:89-110; the 64-frame one, 1600): clv_attn_seq_work_bytes() of
                                   scratch.  K / V (Q / dO) of one (sample, head) then exceed the LDS, so the staged tokens are
                                   split in P = clv_attn_seq_parts() = ceil(ceil(N / 16) / 28) <= 10 parts, each with its own
                                   workgroups; the parts' results ([part][o] + [part][lse] forward, [part][dq | dk | dv]
                                   [tokens][C] backward) meet in a merge kernel.
                                   mode 1, backward with a bias table, optional: clv_attn_dbias_partial_bytes() of 16-byte
                                   aligned memory that receives the slices' fp32 partial sums of the table gradient INSTEAD
                                   of the tail of clv_attn_bwd's `work` — a caller that gathers later (stage bit 8 +
                                   clv_attn_dbias_gather_batch) keeps only this and releases the dS scratch (GBs at 32
                                   frames).  Not read otherwise.
                                   mode 1 with 448 < N <= clv_attn_window_max_tokens() = 1024 (the (16, 7, 7) windows of the
                                   32-frame checkpoints, 784 tokens; 12 x 12 spatial windows), forward and backward, required:
                                   clv_attn_seq_work_bytes() of scratch for the same part plan — P = clv_attn_seq_parts() =
                                   ceil(ceil(N / 16) / 25) parts of clv_attn_part_tokens() staged tokens, beside which the
                                   head's table band stays in LDS.  A caller that gathers later (stage bit 8) passes
                                   clv_attn_dbias_partial_bytes() instead, which for such a window is that scratch rounded up
                                   to 256 bytes FOLLOWED by the partial sums; without bit 8 the partial sums of such a window
                                   go to the tail of clv_attn_bwd's `work`.  Between the stages of a backward run stage by
                                   stage (1, 2, 4) the buffer must stay untouched. */
} ClvAttnGeom;

/* lse: float [groups][nH][N].  bias: the module's relative_position_bias_table, float [rows][nH], or NULL.  rid: int32 [nW][N] region
 * ids of compute_mask (:548-562) or NULL.  kmask: float [groups][N] additive or NULL.
 * seed: device uint64[1], read when dropout_p > 0; the mask is a counter-based hash of
 * (seed, group, head, query, key), so the backward regenerates it from the same seed. */
int64_t clv_attn_seq_work_bytes(const ClvAttnGeom* geom);
int clv_attn_seq_max_keys(void);
/* The number of parts the staged tokens of this geometry are split in: 1 = not split (no scratch needed), 0 = the 16-bit
 * kernels do not take the geometry (clv_attn_fwd / clv_attn_bwd report an error). */
int clv_attn_seq_parts(const ClvAttnGeom* geom);
/* Host-only plan of a geometry run in parts (both modes): the tokens each part stages, a multiple of 16 — the last
 * part may stage fewer; N rounded up to 16 for a geometry of one part; 0 where clv_attn_seq_parts() is 0. */
int clv_attn_part_tokens(const ClvAttnGeom* geom);
/* Which windows the 16-bit kernels take (host only, no GPU needed — the single statement of the set):
 * window (wd, wh, ww) under a table built for (bwd, bwh, bww) (0, 0, 0 = no table), head dim hd.  0 = supported, else
 * 1 bad extents, 2 head dim not 16 / 32 / 64, 3 more than clv_attn_window_max_tokens() tokens, 4 the window has more tokens
 * than the table's window, 5 staged part + table band exceed the 160 KB of LDS. */
int clv_attn_window_supported(int32_t wd, int32_t wh, int32_t ww, int32_t bwd, int32_t bwh, int32_t bww, int32_t hd);
int clv_attn_window_max_tokens(void);
int clv_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                 const float* bias, const int32_t* rid, const float* kmask, const void* seed,
                 const ClvAttnGeom* geom_host, void* stream);

/* dq/dk/dv use strides ldq/ldk/ldv; dout uses ldo.  dbias (float [rows][nH], the gradient of the table)
 * is ACCUMULATED into (caller zeroes).  dsum: float scratch [groups][nH][N].
 * work: scratch of clv_attn_bwd_work_bytes() bytes (the bf16 dS of every (group, head), summed over the groups
 * and scattered into dbias by a second kernel), required iff bias != NULL. */
int64_t clv_attn_bwd_work_bytes(const ClvAttnGeom* geom_host);
/* 1 if clv_attn_bwd runs this geometry (with a bias table) as ONE kernel for dQ / dK / dV (round 4: window mode, head dim 32,
 * 196- / 392-token windows) — `stages` then knows the masks 5 (that kernel) and 2 (the table gradient) instead of 1 / 2 / 4. */
int clv_attn_bwd_one_kernel(const ClvAttnGeom* geom_host);
/* int32 [clv_attn_dbias_index_count()]: fragment offset of the (query, key) pair of every (bias-table row, key), -1 = none;
 * depends on (N, bwd, bwh, bww) only — build once, pass in ClvAttnGeom.dbias_index of every backward call. */
int64_t clv_attn_dbias_index_count(const ClvAttnGeom* geom_host);
int clv_attn_dbias_index(const ClvAttnGeom* geom_host, int32_t* out, void* stream);
int clv_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout,
                 const float* lse, const float* bias, const int32_t* rid, const float* kmask,
                 void* dq, void* dk, void* dv, float* dbias, float* dsum, void* work,
                 const void* seed, int32_t stages, const ClvAttnGeom* geom_host, void* stream);
/* Deferred table gradient (swin_transformer_3d.py:382-386, the backward of the relative_position_bias_table gather): with
 * bit 8 set in `stages` (e.g. 15 = everything but the gather) clv_attn_bwd leaves the slices' partial sums of dS in `work` and
 * does NOT add them into dbias; clv_attn_dbias_gather_entry describes that pending gather (work / dbias / geom as passed to
 * clv_attn_bwd, geom->dbias_index required) and clv_attn_dbias_gather_batch runs up to CLV_DBIAS_GATHER_MAX of them as ONE
 * launch (dbias is accumulated into).  `work` must stay untouched in between.  Nothing reads a table gradient before the
 * optimizer, so a backward pass gathers all its attention blocks at its end. */
#define CLV_DBIAS_GATHER_MAX 32
typedef struct ClvDbiasGather {
    const void* partial;       /* float partial sums inside the work buffer (16-byte aligned; the batch call CONSUMES them:
                                  it adds the slices into slice 0 before it gathers) */
    void* dtable;              /* float [rows][nH] */
    const void* index;         /* int32 table of clv_attn_dbias_index() */
    int64_t split_stride;
    int32_t nkt, nH, N, nsplit, slot0, nslots, block_begin, pad;    /* block_begin, pad: set by the batch call (block range;
                                                                       heads per wave) — whatever the caller leaves there */
} ClvDbiasGather;
int clv_attn_dbias_gather_entry(const ClvAttnGeom* geom_host, void* work, float* dbias, ClvDbiasGather* out);
int64_t clv_attn_dbias_partial_bytes(const ClvAttnGeom* geom_host);    /* size of ClvAttnGeom.work in mode 1 (see there) */
int clv_attn_dbias_gather_batch(const ClvDbiasGather* entries, int32_t n, void* stream);

/* ---- unfused attention for long sequences (N > 448 keys: K/V of one (group, head) no longer fit LDS in the
 * kernels above; the fusion encoder at 32 frames has 16*49 + 32 = 816 tokens).  Q.K^T, P.V and their gradients are
 * batched library GEMMs; these two kernels are what sits between them (HF BertSelfAttention, transformers 4.6.1
 * modeling_bert.py, reached through cross_transformer.py:95-108): one wave per row.
 * fwd: p[r][j] = softmax_j(scores[r][j]*scale + kmask[r / rows_per_group][j]); pd = p * keep/(1-p_drop) with the
 *      same counter-based mask as clv_attn_* (row id r, key j).  scores/p/pd bf16 [rows][ld]; a row of up to 2048 keys is
 *      held in registers, a longer one is walked from memory once per pass.
 *      kmask float [groups][S] or NULL; pd / seed may be NULL when dropout_p == 0.
 * bwd: ds = p * (dp - sum_j p_j dp_j) * scale with dp = dpd * keep/(1-p_drop); ds may alias dpd. */
int clv_softmax_rows_fwd(const void* scores, const float* kmask, void* p, void* pd, const void* seed, int64_t rows,
                         int32_t S, int32_t ld, int32_t rows_per_group, float scale, float dropout_p, void* stream);
int clv_softmax_rows_bwd(const void* p, const void* dpd, void* ds, const void* seed, int64_t rows, int32_t S,
                         int32_t ld, float scale, float dropout_p, void* stream);
/* stages: 0 = everything; otherwise a bit mask 1 = dQ (+ dS scratch, dsum) kernel, 2 = dS -> table-gradient
 * reduction, 4 = dK/dV kernel — lets a profiler bracket each kernel of the call with its own events. */

/* ------------------------------------------------------------------ LayerNorm
 * nn.LayerNorm over the last dim (every norm site: swin_transformer_3d.py:450,483,
 * 541,685,238; HF BERT LayerNorm eps 1e-12; cross_transformer.py:97).
 * x,y [rows][C] bf16 (is_f32 = 0) or float (is_f32 = 1: the fp32 projection heads and
 * losses, ssl_head.py:50-56, contrastive_loss.py:102); gamma,beta float [C]; mean,rstd
 * float [rows].  res (same type as x, may be NULL): y = LN(x + res) (BERT post-LN residual;
 * the Swin residual adds of :498,503 fused into the following norm).  sum_out (may be NULL)
 * receives x + res — the updated residual stream. */
/* Optional operand transforms / extra operands (pass NULL for a plain LayerNorm; C % 8 == 0 and C <= 3072 only):
 *   forward   t = keep(x) * x / (1 - drop_p) * xscale[row / rows_per_sample] + res,  y = LN(t)
 * i.e. the nn.Dropout on the sub-layer output (BertSelfOutput / BertOutput: LayerNorm(dropout(dense(h)) + input))
 * and the per-sample DropPath factor (swin_transformer_3d.py:498,503) applied while the row is loaded.  The
 * dropout mask is a pure function of (*seed, row, column); the backward regenerates it.
 *   backward  d t = LN-backward(dy + dy2) + dsum;  dres (may be NULL) receives d t, dx receives d t times the
 * multiplier x carried.  x_is_sum = 1: the x argument of the backward already holds t (a saved sum_out). */
typedef struct ClvLnExtra {
    const float* xscale;       /* per-sample factor on x, or NULL */
    int32_t rows_per_sample;
    float drop_p;              /* dropout probability on x, 0 = off */
    const void* seed;          /* device uint64, required when drop_p > 0 */
    const void* dy2;           /* backward: second upstream gradient (same type as dy), or NULL */
    void* dres;                /* backward: gradient wrt res when it differs from dx, or NULL */
    int32_t x_is_sum;
    /* PatchMerging (swin_transformer_3d.py:531-539) folded into the LayerNorm that follows it: with gather_c > 0 the
     * normalised row of width C = 4*gather_c is [x(2h,2w) | x(2h+1,2w) | x(2h,2w+1) | x(2h+1,2w+1)] of the UN-gathered
     * x / res [.., 2*gather_h2, 2*gather_w2, gather_c]; rows = .. * gather_h2 * gather_w2; y stays [rows][C]; the
     * backward writes dx / dres in the un-gathered layout (every element exactly once).  No sum_out / dsum / dropout. */
    int32_t gather_c, gather_h2, gather_w2;
    /* backward: leave the per-block partials in `partial` and skip the reduction launch — the caller folds the
     * partials of many LayerNorms into their dgamma / dbeta with ONE clv_ln_reduce_batch launch (needs_reduce tells
     * whether this launch wrote partials at all: up to 256 blocks add into dgamma / dbeta directly) */
    int32_t no_reduce;
    /* forward, fp8 path (vector kernels: C % 8 == 0 and one of their widths): also emit y as OCP e4m3 with one scale per row
     * — q8 [rows][C] bytes = y / qscale[row], qscale[row] = max |y[row]| / 448 — the activation operand of clv_gemm_nt_fp8,
     * produced here instead of by a clv_quant_fp8_rows pass over y.  Both NULL: off. */
    void* q8;
    float* qscale;
} ClvLnExtra;
int clv_layernorm_fwd(const void* x, const void* res, const float* gamma, const float* beta,
                      void* y, void* sum_out, float* mean, float* rstd, int64_t rows, int32_t C,
                      float eps, int32_t is_f32, const ClvLnExtra* extra, void* stream);
/* dx [rows][C] (gradient wrt x and, identically, wrt res unless extra says otherwise) = LN backward of dy
 * (+ dsum, the gradient arriving on sum_out, may be NULL); dgamma,dbeta float [C]
 * ACCUMULATED into (caller zeroes); partial: float scratch [2][nblk][C] with nblk = clv_layernorm_bwd_blocks(). */
int clv_layernorm_bwd_blocks(int64_t rows, int32_t C);
int clv_layernorm_bwd(const void* dy, const void* x, const void* res, const float* gamma,
                      const float* mean, const float* rstd, const void* dsum, void* dx, float* dgamma, float* dbeta,
                      float* partial, int64_t rows, int32_t C, int32_t is_f32, const ClvLnExtra* extra, void* stream);

/* Batched reduction of LayerNorm-backward partials (launches made with extra->no_reduce): dgamma[c] += sum_i
 * partial[0][i][c], dbeta[c] += sum_i partial[1][i][c] for up to CLV_LN_REDUCE_MAX entries (HOST array) in one launch. */
#define CLV_LN_REDUCE_MAX 64
typedef struct ClvLnReduceEntry {
    const float* partial;      /* [2][nblk][C] */
    float* dgamma;
    float* dbeta;
    int32_t nblk, C, block_begin, pad;
} ClvLnReduceEntry;
int clv_layernorm_bwd_needs_reduce(int64_t rows, int32_t C);
int clv_ln_reduce_batch(const ClvLnReduceEntry* entries, int32_t n, void* stream);

/* LayerNorm affine folded into the following Linear (the fused LN + projection kernels, clv_rowgemm with
 * standardise = 1, consume standardised rows):  wf[n][k] = bf16(w[n][k] * gamma[k]),  bf[n] = b[n] + sum_k w[n][k] beta[k]
 * (w float [N][K], b float [N] or NULL).  Backward: given d wf (float [N][K]) and d bf (float [N]),
 * dw / db / dgamma / dbeta are ACCUMULATED into. */
int clv_ln_fold_fwd(const float* w, const float* b, const float* gamma, const float* beta, void* wf, float* bf,
                    int32_t N, int32_t K, void* stream);
int clv_ln_fold_bwd(const float* dwf, const float* dbf, const float* w, const float* gamma, const float* beta,
                    float* dw, float* db, float* dgamma, float* dbeta, int32_t N, int32_t K, void* stream);

/* ------------------------------------------------------------------ BatchNorm1d of the projection heads
 * nn.BatchNorm1d on [B][D] fp32 rows — the ln=False / text_bn=True variants of NCEHeadForMM / NCEHeadForVision /
 * NCEHeadForText (mmaction/models/heads/ssl_head.py:50-66,175-186,252-262).  training != 0: batch statistics (biased
 * variance), running_mean / running_var (may both be NULL) updated with `momentum` and the unbiased variance; training == 0:
 * the running statistics normalise.  save_mean / save_rstd (float [D]) are outputs the backward reads.  Backward: dx (or NULL),
 * dgamma, dbeta (or NULL) are WRITTEN; in training mode dx carries the dependence of the statistics on the batch. */
int clv_batchnorm1d_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                        float* y, float* save_mean, float* save_rstd, int32_t B, int32_t D, float eps, float momentum,
                        int32_t training, void* stream);
int clv_batchnorm1d_bwd(const float* dy, const float* x, const float* gamma, const float* save_mean, const float* save_rstd,
                        float* dx, float* dgamma, float* dbeta, int32_t B, int32_t D, int32_t training, void* stream);

/* ------------------------------------------------------------------ GELU (erf)
 * nn.GELU / HF 'gelu' (swin_transformer_3d.py:264; BertIntermediate; ssl_head.py:53). */
int clv_gelu_fwd(const void* x, void* y, int64_t n, int32_t is_f32, void* stream);
int clv_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, int32_t is_f32, void* stream);

/* ------------------------------------------------------------------ patch embed
 * PatchEmbed3D.forward (swin_transformer_3d.py:671-688: conv3d as a GEMM over patches + bias + LayerNorm(C)) fused with
 * the mask-token blend of SwinTransformer3D.forward (:222-230), for any patch size (pt,ph,pw) and stride (st,sh,sw) of
 * the supported set.  clv_patch_embed_gen_supported is the single statement of that set (host only, no GPU needed):
 * 0 when the geometry is covered, else the reason —
 *   CLV_PE_GEN_BAD_PATCH   a patch extent < 1
 *   CLV_PE_GEN_BAD_STRIDE  not 1 <= stride <= patch on every axis (no gaps between patches)
 *   CLV_PE_GEN_BAD_VOLUME  pt*ph*pw % 8 != 0 (K = 3*pt*ph*pw must be a multiple of 8 for the weight-gradient kernels)
 *   CLV_PE_GEN_BAD_K       K > 384
 *   CLV_PE_GEN_BAD_WIDTH   C not in {48, 96, 128}
 * x float [B][3][T][H][W], padded by the caller to multiples of the PATCH (:675-680).  Token grid: T' = (T - pt) / st + 1
 * (floor), likewise H' and W' (T >= pt, H >= ph, W >= pw); M = B*T'*H'*W'.
 * clv_patch_embed_gen_fwd: w bf16 [C][K] (= proj.weight.flatten(1), K = 3*pt*ph*pw, columns in (c, dt, dy, dx) order);
 * out_clean / out_masked bf16 [B][T'][H'][W'][C] channels-last; either may be NULL.  vmask int64 [B][mh][mw] (the
 * v_token_mask) and mask_token float [C] — required iff out_masked != NULL; mh must divide H' and mw W' (else CLV_ERR_ARG).
 * gamma/beta float [C] or both NULL (patch_norm=False).  z_out (bf16 [M][C] pre-norm conv output), mean, rstd (float [M]):
 * saved for backward, may be NULL.  3*T*H*W <= INT32_MAX.  It computes in the library's 16-bit element type.
 * clv_patch_embed_fwd: the same for patch = stride = (2,4,4) (T even, H, W multiples of 4; w [C][96]) with the weight held in
 * registers; bit-identical to clv_patch_embed_gen_fwd at that geometry. */
#define CLV_PE_GEN_BAD_PATCH 1
#define CLV_PE_GEN_BAD_STRIDE 2
#define CLV_PE_GEN_BAD_VOLUME 3
#define CLV_PE_GEN_BAD_K 4
#define CLV_PE_GEN_BAD_WIDTH 5
int clv_patch_embed_gen_supported(int32_t pt, int32_t ph, int32_t pw, int32_t st, int32_t sh, int32_t sw, int32_t C);
int clv_patch_embed_fwd(const float* x, const void* w, const float* bias, const float* gamma,
                        const float* beta, const float* mask_token, const int64_t* vmask,
                        void* out_clean, void* out_masked, void* z_out, float* mean, float* rstd,
                        int32_t B, int32_t T, int32_t H, int32_t W, int32_t C, int32_t mh,
                        int32_t mw, float eps, void* stream);
int clv_patch_embed_gen_fwd(const float* x, const void* w, const float* bias, const float* gamma, const float* beta,
                            const float* mask_token, const int64_t* vmask, void* out_clean, void* out_masked,
                            void* z_out, float* mean, float* rstd, int32_t B, int32_t T, int32_t H, int32_t W,
                            int32_t C, int32_t mh, int32_t mw, int32_t pt, int32_t ph, int32_t pw, int32_t st,
                            int32_t sh, int32_t sw, float eps, void* stream);
/* Backward of the mask-token blend (:222-230) on the token grid [B][Tp][Hp][Wp]: dy = d_clean + d_masked (1 - w)
 * (bf16 [M][C], 16-byte aligned; either input may be NULL) and dmask_token float [C] += sum over tokens of d_masked w
 * (ACCUMULATED; caller zeroes), w from vmask as above. */
int clv_patch_embed_blend_bwd(const void* dclean, const void* dmasked, const int64_t* vmask, void* dy,
                              float* dmask_token, int32_t B, int32_t Tp, int32_t Hp, int32_t Wp, int32_t C,
                              int32_t mh, int32_t mw, void* stream);
/* im2col of the clip into bf16 patches [M][K] (16-byte aligned; columns in the weight's (c, dt, dy, dx) order): the operand
 * of the weight-gradient GEMM dW = dZ^T * patches (the conv3d weight grad of :681). */
int clv_im2col_patches(const float* x, void* patches, int32_t B, int32_t T, int32_t H, int32_t W, int32_t pt,
                       int32_t ph, int32_t pw, int32_t st, int32_t sh, int32_t sw, void* stream);

/* ------------------------------------------------------------------ Linear weight/bias gradient
 * dW[n][k] += sum_m dY[m][n] X[m][k], db[n] += sum_m dY[m][n] — the weight gradient of every
 * token-parallel nn.Linear on the path (qkv/proj/fc1/fc2/reduction, swin_transformer_3d.py:257-259,
 * 361-363,518; the conv3d weight of :665 through clv_im2col_patches) for huge M and small N x K,
 * where the contraction (token) dimension is split over the whole chip.  dy bf16 [M][N] (row stride
 * ldy), x bf16 [M][K] (row stride ldx); dw float [N][K], db float [N] or NULL — both ACCUMULATED
 * into.  N, K, ldy, ldx multiples of 8.  work: float scratch, clv_linear_wgrad_work_floats().
 * xmean / xrstd (float [M], both or neither): X rows are standardised on load,
 * x_hat = (x - mean) * rstd — the LayerNorm output the fused clv_rowgemm forward never stored. */
int64_t clv_linear_wgrad_work_floats(int64_t M, int32_t N, int32_t K);
int clv_linear_wgrad(const void* dy, const void* x, float* dw, float* db, float* work, int64_t M,
                     int32_t N, int32_t K, int32_t ldy, int32_t ldx, const float* xmean,
                     const float* xrstd, int32_t stages, void* stream);
/* stages: 0 = both kernels; bit 1 = split-M partial kernel, bit 2 = fold of the partials (profiling, or a deferred
 * fold: a backward pass may run its weight-gradient launches with stages = 1 and fold all their partials at once).
 * clv_linear_wgrad_splits: the number of M-slices (= fp32 partial slabs [N*K dW | N db] in work) the launch uses; a fold
 * is needed when it is > 1 or xmean is given.  clv_wgrad_fold_batch: dw[e] += sum_s partial[s][e], db likewise, for up
 * to CLV_FOLD_MAX launches in one kernel (entries is a HOST array; sg_shift / block_begin are filled in by the callee). */
#define CLV_FOLD_MAX 64
typedef struct ClvFoldEntry {
    const void* partial;   /* work of that clv_linear_wgrad call */
    void* dw;              /* float [N][K], accumulated into */
    void* db;              /* float [N] or NULL */
    int64_t nk, e2;        /* N*K and N*K + N */
    int32_t splits, sg_shift, block_begin;
    int32_t overwrite;     /* bit 0: dw = the sum, bit 1: db = the sum (an uninitialised temporary, or the step's first
                              gradient of a weight the engine does not clear), instead of += */
} ClvFoldEntry;
/* Grouped launch: the weight gradients of up to 80 Linear layers (a whole backward segment: nothing reads a weight
 * gradient before the optimizer) as ONE grid.  clv_linear_wgrad_batch_plan fills splits and work_floats of every entry
 * (fewer M-slices per problem than a stand-alone launch needs); the caller points `work` at work_floats floats,
 * clv_linear_wgrad_batch writes the fp32 partials [splits][N*K dW | N db] there, and clv_wgrad_fold_batch (entries with
 * the same work / splits) adds them into dW / db.  entries are HOST arrays. */
typedef struct ClvWgradEntry {
    const void* dy;            /* bf16 [M][N], row stride ldy */
    const void* x;             /* bf16 [M][K], row stride ldx */
    void* work;                /* float [work_floats] */
    float* dw;                 /* work_floats == 0 only (few rows, or a very large output: one slice, no partials, no fold): */
    float* db;                 /*   float [N][K] / [N] (or NULL) gradients, accumulated in place                        */
    int64_t M, work_floats;
    int32_t N, K, ldy, ldx, want_bias, splits;
    int32_t overwrite;         /* work_floats == 0 only; bit 0: dw = (stored, not added: its previous content is stale) */
    int32_t pad;
} ClvWgradEntry;
int clv_linear_wgrad_batch_plan(ClvWgradEntry* entries, int32_t n);
/* 1 if the plan gives this problem work_floats == 0 (one slice added into dw / db in place, without atomics): two such
 * problems with the SAME dw must not share a clv_linear_wgrad_batch call. */
int clv_linear_wgrad_in_place(int64_t M, int32_t N, int32_t K);
/* Tile class clv_linear_wgrad_batch gives the problem: 0 = wgrad_dma2_group_kernel (128 x 128 tiles), 1 =
 * wgrad_big_group_kernel<2, 2> (256 x 256; N and K multiples of 256, M > 1024) — the Linears of swin_transformer_3d.py:257-259,
 * 361-363,518; one launch per class present in the call.  (Round 5's opt-in class 4, shape-fitted (96 a) x (96 b) tiles,
 * moved 1.39 x the algorithmic bytes instead of 2.23 x but cost the step +0.15..0.25 ms and was removed in round 6:
 * profiles/r05_wgrad_tile_class.txt.) */
int clv_linear_wgrad_class(int64_t M, int32_t N, int32_t K);
int clv_linear_wgrad_batch(const ClvWgradEntry* entries, int32_t n, void* stream);
/* Gradient-norm partial sums from the kernels that write a weight gradient (round 6; the optimizer's norm pass of
 * mmcv_Fp16OptimizerHook.py:126-131 `clip_grads` without re-reading those gradients).  sumsq_slots: CLV_SUMSQ_SLOTS
 * accumulators, 16 floats (64 bytes) apart, zero before the backward.  An entry with overwrite bit 2 (value 4) set — in-place
 * entries of clv_linear_wgrad_batch_ss, any entry of clv_wgrad_fold_batch_ss — adds the sum of squares of the dW it STORES
 * (the final value: stored or accumulated) to a slot picked by its block index; clv_optim_prep_slots adds the slots to the
 * norm.  The caller's own clv_sumsq pass must then skip those tensors (clv_sumsq_ranges).  sumsq_slots = NULL: the plain
 * entry points. */
#define CLV_SUMSQ_SLOTS 64
int clv_linear_wgrad_batch_ss(const ClvWgradEntry* entries, int32_t n, float* sumsq_slots, void* stream);
int clv_wgrad_fold_batch_ss(const ClvFoldEntry* entries, int32_t n, float* sumsq_slots, void* stream);
int clv_linear_wgrad_splits(int64_t M, int32_t N, int32_t K);
int clv_wgrad_fold_batch(const ClvFoldEntry* entries, int32_t n, void* stream);

/* ------------------------------------------------------------------ token-parallel projections
 * Y[M][N] = epilogue( prologue(X)[M][K] * Wt[N][K]^T + bias ) — the QKV / proj / fc1 / fc2 Linears of
 * the high-resolution Swin stages and their input-gradient GEMMs (swin_transformer_3d.py:376,398,
 * 263-266), HBM-bound (K, N of a few hundred, M = 10^4..10^5 tokens), with the neighbouring
 * memory-bound ops folded in:
 *   prologue  standardise != 0: x = X (+ res; the sum is written to sum_out), then (x - mean) * rstd —
 *             nn.LayerNorm (:450,483) with its affine part folded into Wt/bias by the caller; mean, rstd
 *             (float [M]) are outputs; xhat_out (bf16 [M][K], row stride ldx, or NULL) receives the standardised rows —
 *             the operand of the weight gradient dW = dY^T x_hat;
 *   epilogue  0: + bias;  1: + bias, erf-GELU (:264), the pre-activation goes to pre_out;
 *             2: multiply by gelu'(pre_in) (GELU backward fused into the fc2 input-gradient GEMM).
 * X, res, sum_out bf16 [M][K] (row stride ldx); Wt bf16 [N][K] contiguous; bias float [N] or NULL;
 * Y, pre_in, pre_out bf16 [M][N] (row stride ldy).  K in {96,128,192,256,288,384,512,576,768}
 * (<= 256 with standardise), N % 8 == 0: query clv_rowgemm_supported(). */
int clv_rowgemm_supported(int32_t N, int32_t K, int32_t standardise);
int clv_rowgemm(const void* x, const void* res, void* sum_out, float* mean, float* rstd, void* xhat_out,
                const void* wt, const float* bias, const void* pre_in, void* y, void* pre_out, int64_t M, int32_t N,
                int32_t K, int32_t ldx, int32_t ldy, int32_t standardise, int32_t epilogue, float eps,
                void* stream);
/* The same with a per-sample factor on X inside the residual-add prologue: x = xscale[row / rows_per_sample] * X + res — the
 * DropPath factor of the attention branch whose residual add (swin_transformer_3d.py:498) the LayerNorm + fc1 kernel performs
 * (res required).  Round 5: the stage-0 block multiplied the branch by its factor with an elementwise pass each way. */
int clv_rowgemm_xs(const void* x, const void* res, void* sum_out, float* mean, float* rstd, void* xhat_out,
                   const void* wt, const float* bias, const void* pre_in, void* y, void* pre_out, int64_t M, int32_t N,
                   int32_t K, int32_t ldx, int32_t ldy, int32_t standardise, int32_t epilogue, float eps,
                   const float* xscale, int32_t rows_per_sample, void* stream);
/* What clv_rowgemm / clv_rowgemm_xs launch for a shape (host only, no GPU needed; ABI 19).  The launch dispatches on the same
 * record, so the entry cannot drift from it.  Returns CLV_ERR_ARG / CLV_ERR_UNSUPPORTED as clv_rowgemm does for the same
 * M, N, K, standardise and epilogue, and CLV_ERR_ARG for out == NULL.
 *   TN         columns of the weight tile a workgroup keeps in LDS;  ny = ceil(N / TN) column tiles
 *   waves      per workgroup (4, 8 or 12): a function of K, prologue and epilogue alone
 *   gx         persistent row slices; the grid is gx * ny workgroups
 *   lds_bytes  dynamic LDS of the launch
 *   trips      ceil(ceil(M / 16) / (gx * waves)): 16-row tiles the busiest wave walks; >= 2 means the wave loop repeats */
typedef struct ClvRowgemmPlan {
    int32_t TN, waves, ny, gx, lds_bytes, trips;
} ClvRowgemmPlan;
int clv_rowgemm_plan(int64_t M, int32_t N, int32_t K, int32_t standardise, int32_t epilogue, ClvRowgemmPlan* out);

/* ------------------------------------------------------------------ the MLP half of a stage-0 block as one kernel each way
 * (round 6) norm2 + Mlp + the residual add in front of them — swin_transformer_3d.py:482-483 (norm2, mlp), :262-268
 * (fc1, GELU, fc2), :498 / :503 (residual, DropPath) — for VideoSwin-T's stage-0 widths, C = 96 and hidden = 384
 * (clv_mlp_fused_supported): both weight matrices stay in LDS, the [M][hidden] activations never reach HBM.
 *   forward:  t = xscale[row / rows_per_sample] * a + res (written to sum_out: the new residual stream; res / xscale may be
 *             NULL), xhat = (t - mean) * rstd (mean, rstd float [M] are outputs, statistics of the fp32 t),
 *             out = GELU(xhat W1f^T + b1f) W2^T + b2.  a, res, sum_out, out bf16 [M][C] contiguous; w1f bf16 [hidden][C] and
 *             b1f float [hidden]: fc1 with the norm's affine part folded in (clv_ln_fold_fwd); w2 bf16 [C][hidden], b2 float
 *             [C] or NULL.
 *   backward: from tsum (= sum_out, or a when there was no res), mean, rstd, d out and the gradient d sum that arrives on the
 *             residual stream (bf16 [M][C] or NULL): recomputes xhat, the pre-activation, GELU and GELU'; d act = d out W2
 *             (w2t = W2^T, bf16 [hidden][C]); d pre = d act GELU'; d xhat = d pre W1f; d t = LayerNorm backward of d xhat
 *             (+ d sum).  Outputs: da = xscale * d t (gradient of a), dres = d t (gradient of res; NULL: not written — without
 *             xscale it equals da), and the operands of the weight-gradient GEMMs that follow (clv_linear_wgrad_batch):
 *             act_out bf16 [M][hidden] (dW2 = d out^T act), dpre_out bf16 [M][hidden] and xhat_out bf16 [M][C] (may be NULL)
 *             (dW1f = d pre^T xhat, un-folded by clv_ln_fold_bwd). */
int clv_mlp_fused_supported(int32_t C, int32_t hidden);
int clv_mlp_fused_fwd(const void* a, const void* res, void* sum_out, float* mean, float* rstd, const void* w1f,
                      const float* b1f, const void* w2, const float* b2, void* out, int64_t M, int32_t C, int32_t hidden,
                      float eps, const float* xscale, int32_t rows_per_sample, void* stream);
int clv_mlp_fused_bwd(const void* tsum, const float* mean, const float* rstd, const void* dout, const void* dsum,
                      const void* w1f, const float* b1f, const void* w2t, void* da, void* dres, void* act_out,
                      void* dpre_out, void* xhat_out, int64_t M, int32_t C, int32_t hidden, const float* xscale,
                      int32_t rows_per_sample, void* stream);
/* How clv_mlp_fused_fwd / _bwd cut M rows into workgroups (host only; ABI 19); the kernels take their row ranges from the
 * same helper.  CLV_ERR_ARG for M <= 0 or out == NULL.
 *   grid                  workgroups, each with a contiguous range of 16-token tiles
 *   tiles_min, tiles_max  the smallest / largest tile count of a workgroup
 *   trips                 groups of two tiles per wave in the fullest workgroup (8 waves); >= 2: the forward's row prefetch runs
 *   half_group            1: some workgroup has an odd tile count, so its last group runs the one-tile body */
typedef struct ClvMlpFusedPlan {
    int32_t grid, tiles_min, tiles_max, trips, half_group;
} ClvMlpFusedPlan;
int clv_mlp_fused_plan(int64_t M, ClvMlpFusedPlan* out);

/* db[n] += sum_m dy[m][n] (bf16 dy, row stride ld; N, ld multiples of 8): the bias gradient of the
 * library-GEMM Linear layers (BERT / fusion / MLM head), ACCUMULATED into db. */
int clv_colsum(const void* dy, float* db, int64_t M, int32_t N, int32_t ld, void* stream);

/* ------------------------------------------------------------------ focal MLM loss
 * SoftmaxFocalLossMultiClass.forward (mmaction/models/losses/focal_loss.py:61-72) on the
 * masked rows selected by multimodal_transformer_pretrain.py:137-139, fused:
 * rows with label == -100 are skipped; loss = mean over the others of (1-pt)^gamma * ce.
 * logits bf16 or float [rows][V] (is_bf16); labels int64 [rows]; row_ce,row_lse float
 * [rows] saved for backward; loss float [1]; count float [1] (number of masked rows) —
 * both must be ZERO on entry (they double as the accumulators). */
int clv_focal_ce_fwd(const void* logits, int32_t is_bf16, const int64_t* labels, float* row_ce,
                     float* row_lse, float* loss, float* count, int64_t rows, int32_t V,
                     float gamma, void* stream);
/* dlogits (same dtype as logits) = dloss * d loss / d logits (zero for skipped rows). */
int clv_focal_ce_bwd(const void* logits, int32_t is_bf16, const int64_t* labels, const float* row_ce,
                     const float* row_lse, const float* count, const float* dloss, void* dlogits,
                     int64_t rows, int32_t V, float gamma, void* stream);
/* The same on rows of stride ld >= V elements (logits and dlogits alike): the padded score buffer of the MLM decoder (V =
 * 30522 is not a multiple of 8, ld = 30528 is).  The backward zeroes the padding columns [V, ld) of dlogits. (ABI 8) */
int clv_focal_ce_fwd_ld(const void* logits, int32_t is_bf16, const int64_t* labels, float* row_ce, float* row_lse,
                        float* loss, float* count, int64_t rows, int32_t V, int64_t ld, float gamma, void* stream);
int clv_focal_ce_bwd_ld(const void* logits, int32_t is_bf16, const int64_t* labels, const float* row_ce,
                        const float* row_lse, const float* count, const float* dloss, void* dlogits, int64_t rows,
                        int32_t V, int64_t ld, float gamma, void* stream);

/* ------------------------------------------------------------------ exclusive InfoNCE + rank
 * ExclusiveNCEwithRankingLoss.forward after the all-gather
 * (mmaction/models/losses/contrastive_loss.py:112-161): cos_norm of the four gathered
 * embeddings, three G×G similarity matmuls / temperature, the three exclusive [G,3G] row
 * log-softmaxes, the [3G,G] column log-softmax, diagonals, MarginRankingLoss(margin).
 * e0..e3 float [G][Dm] with row stride ld floats (video, text, text_mask, text_recon) — ld > Dm lets
 * the four be slots of one packed [G][k][Dm] tensor, as the all-gather delivers them.  out float [2] =
 * {nce_loss, rank_t_tm_loss}.  work: float scratch, >= clv_infonce_work_floats(G, Dm). */
int64_t clv_infonce_work_floats(int32_t G, int32_t Dm);
int clv_infonce_fwd(const float* e0, const float* e1, const float* e2, const float* e3, float* out,
                    float* work, int32_t G, int32_t Dm, int32_t ld, float temperature, float margin,
                    void* stream);
/* dout float [2] = upstream grads of {nce, rank}; d0..d3 float [G][Dm] with row stride ldd.  `work`
 * must be the buffer the matching forward filled (e0..e3 are not re-read and may be NULL). */
int clv_infonce_bwd(const float* e0, const float* e1, const float* e2, const float* e3,
                    const float* dout, const float* work, float* d0, float* d1, float* d2, float* d3,
                    int32_t G, int32_t Dm, int32_t ldd, float temperature, float margin, void* stream);
/* The pre-training step evaluates the loss twice on slots of ONE packed fp32 [G][k][Dm] tensor — video -> text on
 * (video, text, masked text, video-recon) and text -> video on (text, video, masked video, text-recon)
 * (multimodal_transformer_pretrain.py:147-169).  The pair form runs both evaluations in the same launches (3 forward,
 * 4 backward).  slots: HOST int32 [8] = the four slot indices of evaluation 0, then of evaluation 1 (distinct within an
 * evaluation, < k).  out float [4] = {nce_0, rank_0, nce_1, rank_1}; work >= 2 * clv_infonce_work_floats(G, Dm) floats.
 * Backward: dout = HOST array of four DEVICE pointers to the fp32 upstream gradients of out[0..3] (each where autograd left
 * it; NULL = 0); dpacked [G][k][Dm] is WRITTEN in full (a slot read by both evaluations receives the sum, a slot read by
 * none zeros). */
int clv_infonce_pair_fwd(const float* packed, const int32_t* slots, float* out, float* work, int32_t G, int32_t k,
                         int32_t Dm, float temperature, float margin, void* stream);
int clv_infonce_pair_bwd(const float* const* dout, const float* work, const int32_t* slots, float* dpacked, int32_t G,
                         int32_t k, int32_t Dm, float temperature, float margin, void* stream);

/* NormSoftmaxLoss (mmaction/models/losses/contrastive_loss.py:26-68), the retrieval fine-tuning loss
 * (multimodal_transformer_finetune.py:83-86): x = normalise(video) . normalise(text)^T / temperature,
 * out[0] = -mean diag(log_softmax(x, 1)) - mean diag(log_softmax(x^T, 1)).  video/text float [G][Dm];
 * eps = the norm clamp (1e-12 for F.normalize :51-52, 1e-8 for cos_sim :10-18).  When sim_mat (float
 * [G][G]) is given it is used as x and video/text/Dm/temperature/eps are ignored (:55-56).
 * work: float scratch >= clv_normsoftmax_work_floats(G, Dm). */
int64_t clv_normsoftmax_work_floats(int32_t G, int32_t Dm);
int clv_normsoftmax_fwd(const float* video, const float* text, const float* sim_mat, float* out, float* work,
                        int32_t G, int32_t Dm, float temperature, float eps, void* stream);
/* dout float [1]; `work` is the buffer the forward filled.  Without sim_mat: dvideo/dtext float [G][Dm]
 * (dsim ignored); with sim_mat: dsim float [G][G] (dvideo/dtext ignored). */
int clv_normsoftmax_bwd(const float* sim_mat, const float* dout, const float* work, float* dvideo, float* dtext,
                        float* dsim, int32_t G, int32_t Dm, float temperature, void* stream);

/* The same six entry points for a GLOBAL batch (virtual ranks: G = k * B rows, 1024 at the reference's headline
 * configuration).  The functions above compute every log-sum-exp in ONE workgroup; these spread them over the device — one
 * wave per exclusive row, 64 adjacent columns per workgroup, one pass each with a running (max, sum) — reduce the per-row
 * terms in a fixed order in a finish kernel (no float atomics: the losses are bit-reproducible from run to run) and run
 * their GEMMs as 64 x 64 LDS tiles.  Arguments, `work` layout and sizes are those of the function without the suffix, so a
 * `work` either forward filled serves either backward.  clv_infonce_large_min_g(): the row count from which the callers
 * (clover_amd.ops) take these — the measured crossover; below it the functions above run, bit for bit as before. */
int32_t clv_infonce_large_min_g(void);
int clv_infonce_fwd_large(const float* e0, const float* e1, const float* e2, const float* e3, float* out,
                          float* work, int32_t G, int32_t Dm, int32_t ld, float temperature, float margin,
                          void* stream);
int clv_infonce_bwd_large(const float* e0, const float* e1, const float* e2, const float* e3,
                          const float* dout, const float* work, float* d0, float* d1, float* d2, float* d3,
                          int32_t G, int32_t Dm, int32_t ldd, float temperature, float margin, void* stream);
int clv_infonce_pair_fwd_large(const float* packed, const int32_t* slots, float* out, float* work, int32_t G, int32_t k,
                               int32_t Dm, float temperature, float margin, void* stream);
int clv_infonce_pair_bwd_large(const float* const* dout, const float* work, const int32_t* slots, float* dpacked,
                               int32_t G, int32_t k, int32_t Dm, float temperature, float margin, void* stream);
int clv_normsoftmax_fwd_large(const float* video, const float* text, const float* sim_mat, float* out, float* work,
                              int32_t G, int32_t Dm, float temperature, float eps, void* stream);
int clv_normsoftmax_bwd_large(const float* sim_mat, const float* dout, const float* work, float* dvideo, float* dtext,
                              float* dsim, int32_t G, int32_t Dm, float temperature, void* stream);

/* What the loss entries above launch (host only, no GPU needed; four symbols added to ABI 20 — new symbols, nothing existing
 * changes, the version stays).  The launch code decides on the same records, so the entries cannot drift from it.  Each
 * returns CLV_ERR_ARG where the entry it describes would (and for out == NULL).
 *
 * clv_loss_gemm_plan: one fp32 GEMM of the loss section, C = alpha A[M][K] . B[N][K]^T, `batch` of them per evaluation with
 * operand strides sA, sB and s2 floats between the two evaluations of the pair form (0 without).  a_align / b_align: the base
 * addresses of A and B modulo 16 (bytes); tiled: 1 on the *_large entries.
 *   kernel           0 one wave per 16 x 16 tile; 1 eight waves split the contraction of a tile (K >= 256 and at most 512
 *                    tiles per evaluation); 2 LDS tiles 64 x 64 x 16 staged with 16-byte loads; 3 the same staged element by
 *                    element with row and contraction guards (K % 16 != 0, a stride that is no multiple of 4 floats, or a
 *                    base address off a 16-byte boundary)
 *   waves            per workgroup (1, 8, 4);  gx, gy: tiles across N and M;  tiles = gx * gy * batch
 *   kchunk           contraction elements per wave (kernels 0, 1: a multiple of 16) or per LDS stage (16)
 *   waves_with_work  waves whose first element wave * kchunk lies below K (kernel 1 with K < 7 kchunk + 1: the rest idle)
 *   k_tail           K % 16: elements of the last, guarded 16-step (0: none) */
typedef struct ClvLossGemmPlan {
    int32_t kernel, waves, gx, gy, tiles, kchunk, waves_with_work, k_tail;
} ClvLossGemmPlan;
int clv_loss_gemm_plan(int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t batch, int64_t sA, int64_t sB,
                       int64_t s2, int32_t a_align, int32_t b_align, int32_t tiled, ClvLossGemmPlan* out);
/* clv_focal_plan: clv_focal_ce_fwd(_ld) / _bwd(_ld) for rows of V scores with stride ld.  logits_align / dlogits_align: the
 * base addresses modulo 4 (bytes).  The forward looks at logits alone, the backward at both.
 *   fwd_kernel, bwd_kernel  0 fp32, 256 threads; 1 16-bit, one 2-byte element per access, 256 threads; 2 16-bit PAIRS (one
 *                           4-byte access), 1024 threads: V and ld even and the base addresses on 4-byte boundaries
 *   fwd_threads, bwd_threads
 *   fwd_trips               accesses of the busiest thread over a row (2-byte / fp32: per pass); >= 2 on the pair kernel: a
 *                           thread rescales its own running sum
 *   fwd_waves_with_work     waves of the forward workgroup that own at least one element */
typedef struct ClvFocalPlan {
    int32_t fwd_kernel, bwd_kernel, fwd_threads, bwd_threads, fwd_trips, fwd_waves_with_work;
} ClvFocalPlan;
int clv_focal_plan(int32_t is_16bit, int32_t V, int64_t ld, int32_t logits_align, int32_t dlogits_align, ClvFocalPlan* out);
/* clv_infonce_plan / clv_normsoftmax_plan: one evaluation (pair: 1 = the pair entries, whose second work area starts
 * clv_infonce_work_floats(G, Dm) floats after the first) on a work buffer at a 16-byte boundary.  large: 0 the entries
 * without suffix, 1 the *_large entries.  sim_mat: 1 = NormSoftmaxLoss on a given score matrix (no GEMM runs: the three GEMM
 * records are zero).  ld is checked as clv_infonce_fwd checks it; no launch class depends on it.
 *   fwd, bwd0, bwd1  the score GEMM(s); d en of the first operand (K = 3 G, NormSoftmax: G); d en of the others (K = G)
 *   loss_threads, loss_trips   large == 0: the one-workgroup loss kernel and the exclusive rows / columns its busiest thread
 *                              walks (6 G of them, NormSoftmax: 2 G)
 *   rows_grid, cols_gx, cols_gy, finish_threads   large == 1: workgroups of the row kernel (4 rows each), of the column
 *                              kernel (64 columns x one score block each), threads of the finish kernel
 *   cols_last         columns of the last column group (< 64: ragged)
 *   idle_row_lanes    lanes of a row's wave without an element (G < 64);  idle_col_waves: the same for the 16 waves of a
 *                     column group (G < 16) */
typedef struct ClvLossPlan {
    ClvLossGemmPlan fwd, bwd0, bwd1;
    int32_t large, loss_threads, loss_trips, rows_grid, cols_gx, cols_gy, finish_threads, cols_last, idle_row_lanes,
        idle_col_waves;
} ClvLossPlan;
int clv_infonce_plan(int32_t G, int32_t Dm, int32_t ld, int32_t pair, int32_t large, ClvLossPlan* out);
int clv_normsoftmax_plan(int32_t G, int32_t Dm, int32_t sim_mat, int32_t large, ClvLossPlan* out);

/* Dual-softmax loss (DSL): NormSoftmaxLoss under the prior that clv_retrieval_* applies at evaluation (dual_softmax = T >= 0,
 * finite; T multiplies the cosine).  Not in the reference.  Six symbols added to ABI 20 — new symbols, nothing existing
 * changes, the version stays.  With c[i][j] the cosine of video i and text j (normalised with the clamp eps as above),
 * a = G / temperature:
 *   Pr[i][j] = softmax over i of T c[i][j]     Pc[i][j] = softmax over j of T c[i][j]
 *   yr = a c Pr  (video -> text logits)        yc = a c Pc  (text -> video logits)
 *   out[0] = -mean_i log_softmax_j(yr)[i][i] - mean_j log_softmax_i(yc)[j][j]
 * T = 0 is NormSoftmaxLoss (P = 1 / G).  The gradient flows through the priors: with gr = (softmax_j(yr) - I) / G,
 * gc = (softmax_i(yc) - I) / G, u[j] = sum_i gr c Pr, w[i] = sum_j gc c Pc,
 *   d out / d c = a ( Pr (gr (1 + T c) - T u[j]) + Pc (gc (1 + T c) - T w[i]) ).
 * video / text float [G][Dm]; out float [1]; dout float [1]; work >= clv_dsl_loss_work_floats(G, Dm) floats; the backward
 * reads only the work the forward filled.  *_large: the multi-workgroup form (one wave per row, 64 adjacent columns per
 * workgroup, a finish kernel that sums in a fixed order; LDS-tiled GEMMs), taken by the callers from
 * clv_infonce_large_min_g() rows on; neither form uses float atomics, and a work either forward filled serves either
 * backward.  clv_dsl_loss_plan: the launches of one evaluation, the record of clv_normsoftmax_plan without sim_mat (host
 * only); the two statistics passes of the forward and the reductions of the backward run on the same launch shapes. */
int64_t clv_dsl_loss_work_floats(int32_t G, int32_t Dm);
int clv_dsl_loss_fwd(const float* video, const float* text, float* out, float* work, int32_t G, int32_t Dm,
                     float temperature, float eps, float dual_softmax, void* stream);
int clv_dsl_loss_bwd(const float* dout, const float* work, float* dvideo, float* dtext, int32_t G, int32_t Dm,
                     float temperature, float dual_softmax, void* stream);
int clv_dsl_loss_fwd_large(const float* video, const float* text, float* out, float* work, int32_t G, int32_t Dm,
                           float temperature, float eps, float dual_softmax, void* stream);
int clv_dsl_loss_bwd_large(const float* dout, const float* work, float* dvideo, float* dtext, int32_t G, int32_t Dm,
                           float temperature, float dual_softmax, void* stream);
int clv_dsl_loss_plan(int32_t G, int32_t Dm, int32_t large, ClvLossPlan* out);

/* ------------------------------------------------------------------ optimizer
 * Grad-norm (clip_grad_norm_, mmcv_Fp16OptimizerHook.py:127-137) + AdamW step on flat
 * buffers (optimizer cfg pretrain_webvid_cc3m.py:129-137).
 * clv_sumsq: acc[0] += sum(g^2) over n floats (caller zeroes acc). */
int clv_sumsq(const float* g, float* acc, int64_t n, void* stream);
/* One fused AdamW step over a flat fp32 segment.  sumsq: float[1] device = total grad norm²
 * (all segments); the clip coefficient min(1, max_norm/(sqrt(sumsq)+1e-6)) is applied on
 * device, and the step is skipped when sumsq is not finite.  shadow (bf16, may be NULL)
 * receives the updated weights for the bf16 compute path.  grad_scale multiplies g first. */
int clv_adamw_step(float* p, const float* g, float* m, float* v, void* shadow, const float* sumsq,
                   int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                   float bias_c1, float bias_c2, float max_norm, float grad_scale, void* stream);

/* ------------------------------------------------------------------ Linear layers: LDS-tiled MFMA GEMM (gemm_nt.hip)
 * C[M][N] = A[M][K] . B[N][K]^T with fused epilogues — the forward and input-gradient GEMMs of nn.Linear as the
 * reference's Mlp / qkv / proj / PatchMerging.reduction and the HF BERT layers run them
 * (mmaction/models/backbones/swin_transformer_3d.py:262-268, 376, 398, 543; transformers 4.6.1 BertIntermediate /
 * BertOutput), replacing torch's addmm + separate GELU kernels:
 *   forward   y  = x W^T + b        A = x  [M][K], B = W   [N][K]          epilogue BIAS | BIAS_GELU | NONE
 *   dgrad     dx = dy W             A = dy [M][N], B = W^T [K][N]          epilogue NONE | DGELU
 * a, b, c, c2, aux: bf16, row strides lda / ldb / ldc elements (multiples of 8; c2 and aux share ldc); bias fp32 [N].
 *   CLV_GEMM_EPI_NONE       c = acc
 *   CLV_GEMM_EPI_BIAS       c = acc + bias
 *   CLV_GEMM_EPI_BIAS_GELU  c2 = acc + bias (the pre-activation, kept for backward), c = GELU_erf(acc + bias)
 *   CLV_GEMM_EPI_DGELU      c = acc * GELU_erf'(aux)      (aux = the forward's pre-activation)
 *   CLV_GEMM_EPI_BIAS_GELU_D  c2 = GELU_erf'(acc + bias) (what the backward needs of the pre-activation, computed where its
 *                             erf / exp are in hand anyway), c = GELU_erf(acc + bias)
 *   CLV_GEMM_EPI_MUL        c = acc * aux                 (aux = that c2: the GELU backward without a transcendental)
 * Needs N % 8 == 0, K % 64 == 0, 16-byte aligned pointers (clv_gemm_nt_supported); fp32 accumulation.
 * The bias is ROUNDED TO THE 16-BIT TYPE before it is added (on every path: the row kept in LDS, the read from global
 * memory for N > 3072, the reduce kernel of a sliced launch) — part of the result, pinned by tests/test_gemm_nt_gpu.py.
 * aux and c2 are addressed with ldc, like c: element (m, n) of each lies at m * ldc + n.  Columns [N, ldc) of c / c2 are
 * never written. */
#define CLV_GEMM_EPI_NONE 0
#define CLV_GEMM_EPI_BIAS 1
#define CLV_GEMM_EPI_BIAS_GELU 2
#define CLV_GEMM_EPI_DGELU 3
#define CLV_GEMM_EPI_BIAS_GELU_D 4
#define CLV_GEMM_EPI_MUL 5
int clv_gemm_nt_supported(int64_t M, int32_t N, int32_t K);
int clv_gemm_nt(const void* a, const void* b, const float* bias, const void* aux, void* c, void* c2, int64_t M,
                int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc, int32_t epilogue, void* stream);
/* The same GEMM with a work buffer (ABI 8).  Few-tile long-contraction layers (K >= 1536 and <= 256 tiles of 128 x 128:
 * fc2 / the fc1 input gradient of Swin stage 3 — swin_transformer_3d.py:262-268 —, of the fusion encoder and of the text
 * tower) cut the contraction into slices that run as workgroups of their own: each slice leaves an fp32 partial sum in
 * `work` ([slices][M][N]) and a second kernel adds the slices and applies the epilogue.  clv_gemm_nt_work_bytes(M, N, K) =
 * the bytes that plan needs (0: the shape runs in one pass — then `work` may be NULL); with work == NULL or a buffer that
 * is too small the call runs in one pass, as clv_gemm_nt does.  work: 16-byte aligned, used only inside the call. */
int64_t clv_gemm_nt_work_bytes(int64_t M, int32_t N, int32_t K);
int clv_gemm_nt_ex(const void* a, const void* b, const float* bias, const void* aux, void* c, void* c2, int64_t M,
                   int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc, int32_t epilogue, void* work,
                   int64_t work_bytes, void* stream);
/* What clv_gemm_nt_ex launches for a shape under the current CLV_GEMM_SPLITK / CLV_GEMM_ROT (host only, no GPU needed;
 * added to ABI 18 — a new symbol, nothing existing changes).  with_work: 0 = as with work == NULL (never sliced), 1 = as
 * with a work buffer large enough for the plan.  The launch dispatches on the same record, so the entry cannot drift from
 * it.  Returns CLV_ERR_ARG / CLV_ERR_UNSUPPORTED like the GEMM itself.
 *   kernel         0 gemm_nt_kernel (every wave stages and multiplies), 1 gemm_ws_kernel 128 x 128, 2 gemm_ws_kernel 64 x 128
 *                  (wave-specialised: producer waves stage, consumer waves multiply)
 *   BM, BN         output tile;  waves: per workgroup (the wave-specialised classes: consumers + 2 producers = 10 / 6)
 *   ring           stages of the LDS ring
 *   splitk         K slices (> 1: fp32 slabs in `work` + the reduce kernel, which applies the epilogue)
 *   rot            1: the K walk of each unit starts at a rotated stage (CLV_GEMM_ROT=1, K >= 192, kernel 0 only)
 *   pc             column partitions of the XCD split: XCD x owns row blocks = x / pc (mod 8 / pc), column tiles = x % pc (mod pc)
 *   grid           workgroups = 8 * min(units_max_xcd, slots_xcd)
 *   units_max_xcd  (tile, slice) units of the fullest XCD;  slots_xcd: persistent workgroups per XCD — more units than
 *                  slots means some workgroup walks several units
 *   bias_in_lds    1: the bias row is staged in LDS as 16-bit values; 0: read from global memory (N > 3072, or splitk > 1:
 *                  by the reduce kernel) and rounded to 16 bits there */
typedef struct ClvGemmPlan {
    int32_t kernel, BM, BN, waves, ring, splitk, rot, pc, grid, units_max_xcd, slots_xcd, bias_in_lds;
} ClvGemmPlan;
int clv_gemm_nt_plan(int64_t M, int32_t N, int32_t K, int32_t with_work, ClvGemmPlan* out);
/* Batched transposes of bf16 matrices in one launch (the engine's W^T shadows, refreshed after every optimizer step).
 * table: n_entries x {int64 src_off, dst_off (elements from src_base / dst_base); int32 rows, cols, tile_begin,
 * tiles_c} on the device; entry e covers ceil(rows/64) * tiles_c tiles starting at tile_begin (tiles_c =
 * ceil(cols/64)); total_tiles = the grid.  dst[c][r] = src[r][c]. */
#define CLV_TRANSPOSE_ENTRY_BYTES 32
int clv_transpose_batch(const void* src_base, void* dst_base, const void* table, int32_t n_entries,
                        int32_t total_tiles, void* stream);

/* The same step with the optimizer's scalars held on the DEVICE (no host sync, hipGraph-safe):
 * state = CLV_OPTIM_STATE_BYTES bytes {float coef, bc1, bc2_sqrt, norm; int32 skip, t, skipped; float grad_loss_scale (the
 * loss_scale of the last prep's gradients, for clv_grad_report; padding before it existed); float loss_scale,
 * scale_factor; int32 scale_window, scale_iter, last_overflow, dynamic, pad, pad}, zeroed once by the caller.  The second
 * half is the reference's LossScaler (mmaction/core/hooks/fp16_utils.py:285-389) held on the device: with loss_scale > 0
 * the caller multiplies the root gradient of its backward by state.loss_scale (a device read: it stays inside a hipGraph),
 * clv_optim_prep divides it out of the norm and the update, and with dynamic = 1 applies update_scale (:351-362): an
 * overflow (non-finite norm) halves the scale (floor 1) and records the iteration, scale_window overflow-free iterations
 * since then grow it by scale_factor (the host sets last_overflow = -1, scale_factor and scale_window once).  clv_optim_prep (one thread, after every segment's clv_sumsq): reads and re-zeroes sumsq, computes the
 * clip coefficient (grad_scale * min(1, max_norm/(norm+1e-6)); max_norm <= 0: no clipping); a finite norm advances
 * Adam's step count t and refreshes the bias corrections, a non-finite one sets skip — the reference skips
 * optimizer.step() on overflow (mmcv_Fp16OptimizerHook.py:123-141), so Adam's step count does not advance either.
 * clv_adamw_step_dev: clv_adamw_step with coefficient / bias corrections / skip read from state. */
#define CLV_OPTIM_STATE_BYTES 64
int clv_optim_prep(float* sumsq, void* state, float beta1, float beta2, float max_norm, float grad_scale,
                   void* stream);
/* clv_optim_prep with the norm slots of clv_linear_wgrad_batch_ss / clv_wgrad_fold_batch_ss: the CLV_SUMSQ_SLOTS partial sums
 * are added to sumsq[0] and re-zeroed.  clv_sumsq_ranges: sumsq over a list of ranges of ONE buffer in one launch — table
 * (device) = n_blocks x {int64 offset, int64 count} in floats from base, one entry per 256-thread block (the host cuts the
 * ranges into chunks of <= CLV_SUMSQ_CHUNK floats; offsets are multiples of 4): acc[0] += sum g^2. */
#define CLV_SUMSQ_CHUNK 16384
int clv_optim_prep_slots(float* sumsq, float* sumsq_slots, void* state, float beta1, float beta2, float max_norm,
                         float grad_scale, void* stream);
int clv_sumsq_ranges(const float* base, const void* table, int32_t n_blocks, float* acc, void* stream);
int clv_adamw_step_dev(float* p, const float* g, float* m, float* v, void* shadow, const void* state, int64_t n,
                       float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ------------------------------------------------------------------ weight EMA (csrc/ema.hip)
 * The reference's `ema_hook` (mmaction/core/hooks/ema.py:68-97: per tensor `buf.mul_(1 - m).add_(p, alpha=m)` every
 * iteration, and a clone + two copies per tensor to exchange weights and averages around evaluation / checkpoints) as one
 * launch per model each.  Both walk a device TABLE the caller builds once:
 *     n_entries x entry, then n_blocks x {int64 entry index, int64 start}   (8-byte aligned, contiguous)
 * with one block record per chunk of <= CLV_EMA_CHUNK floats of an entry (start = a multiple of CLV_EMA_CHUNK, < n); every
 * element of every entry is covered by exactly one record.  A chunk whose pointers are 16-byte aligned is moved 16 bytes per
 * lane; any other one element by element (tensors of any length and 4-byte alignment are legal).  No atomics.
 *   clv_ema_update: entry = {const float* p; float* ema; int64 n}:  ema = (1 - m) * ema + m * p in fp32, with 1 - m formed
 *     in double on the host and rounded to fp32 once.  m is a launch argument (0 <= m <= 1): it may change every call.
 *   clv_ema_swap: entry = {float* p; float* ema; void* shadow; int64 n}: p and ema exchange their bit patterns in place
 *     (every address stays valid: captured graphs keep reading p); shadow (bf16, may be NULL) receives the 16-bit copy of
 *     the new p, rounded exactly as clv_adamw_step_dev rounds the one it writes. */
#define CLV_EMA_CHUNK 4096
#define CLV_EMA_UPDATE_ENTRY_BYTES 24
#define CLV_EMA_SWAP_ENTRY_BYTES 32
#define CLV_EMA_BLOCK_BYTES 16
int clv_ema_update(const void* table, int32_t n_entries, int32_t n_blocks, double momentum, void* stream);
int clv_ema_swap(const void* table, int32_t n_entries, int32_t n_blocks, void* stream);

/* ------------------------------------------------------------------ overflow report (csrc/grad_report.hip)
 * Which parameters hold the non-finite gradients behind a skipped step.  The reference asks every parameter in turn, with a
 * host synchronisation each (LossScaler.has_overflow / _has_inf_or_nan, mmaction/core/hooks/fp16_utils.py:328-349), and
 * its hook announces every overflow (mmcv_Fp16OptimizerHook.py:123-141); here the skip decision is on the device
 * (clv_optim_prep), so the report is taken there as well: two launches over ONE gradient buffer that return at once unless
 * state.skip is set.
 *   buf    the gradients: elem = CLV_GRAD_REPORT_F32 fp32 (a slab), CLV_GRAD_REPORT_HALF the library's 16-bit element type
 *          (the wire copy of a data-parallel job); naturally aligned
 *   table  (8-byte aligned) n_params x {int64 first_chunk, n_chunks_of_it}, then n_chunks x {int64 parameter, start, count}:
 *          the caller cuts every parameter into chunks of 1 .. CLV_SUMSQ_CHUNK elements (start in elements from buf), the
 *          chunks of one parameter adjacent and in order; every chunk is one 256-thread block
 *   state  the CLV_OPTIM_STATE_BYTES record of clv_optim_prep.  Its former padding word behind `skipped` now holds the
 *          loss_scale the gradients of the last clv_optim_prep carried (a dynamic scale has moved by the time skip is known)
 *   report (16-byte aligned) CLV_GRAD_REPORT_HEADER_BYTES + (n_params + n_chunks) * CLV_GRAD_REPORT_STAT_BYTES bytes:
 *          {int32 t, skipped; float loss_scale; int32 n_params; 4 x int32 0}, then per parameter, then per chunk (scratch)
 *          {int32 nonfinite; float max_abs, sumsq, norm}: the count of NaN / infinite elements, and over the FINITE ones the
 *          largest magnitude, the fp32 sum of squares and its square root, all in the buffer's units (loss scale included)
 *   mode   0: "on skip" — every block reads state.skip first and returns when it is 0, leaving the report of the last
 *          skipped step readable; loss_scale = the one those gradients carried.  1: always; loss_scale = state.loss_scale
 *          (for use BEFORE clv_optim_prep)
 * 16-byte loads wherever a chunk allows, fixed-order reductions, no atomics: the report is a pure function of buffer and
 * table, bit-reproducible, rewritten whole by every reporting call.  Plain launches on `stream`; capturable. */
#define CLV_GRAD_REPORT_F32 0
#define CLV_GRAD_REPORT_HALF 1
#define CLV_GRAD_REPORT_PARAM_BYTES 16
#define CLV_GRAD_REPORT_CHUNK_BYTES 24
#define CLV_GRAD_REPORT_HEADER_BYTES 32
#define CLV_GRAD_REPORT_STAT_BYTES 16
int clv_grad_report(const void* buf, int32_t elem, const void* table, int32_t n_params, int32_t n_chunks,
                    const void* state, void* report, int32_t mode, void* stream);

/* ------------------------------------------------------------------ activation report (csrc/act_report.hip)
 * Which forward output went non-finite first.  The reference's overflow check looks at gradients only
 * (LossScaler.has_overflow / _has_inf_or_nan, mmaction/core/hooks/fp16_utils.py:328-349) and its hook announces the
 * overflow without a place (mmcv_Fp16OptimizerHook.py:123-141); an fp16 forward value above 65504 is stored as inf, every
 * gradient behind it is non-finite, and the gradient report above then lists the whole model.  These two entries keep one
 * 16-byte record per watched forward output, on the device and inside the step's hipGraphs.
 *
 * clv_act_report folds x into the record at slot:
 *   x      count elements, elem = CLV_GRAD_REPORT_F32 or CLV_GRAD_REPORT_HALF (the library's 16-bit type), naturally
 *          aligned; may be NULL when count == 0, which is legal and only bumps `calls`
 *   slot   (16-byte aligned) {int32 nonfinite; uint32 max_abs; int32 calls; int32 zero}: nonfinite += the number of NaN and
 *          +-inf elements, max_abs = max(max_abs, bits of the largest FINITE |x| as fp32) — ordered like an integer, as in
 *          the gradient report's records — and calls += 1.  The caller clears the record (16 zero bytes).
 * One launch: a bounded grid with a grid-stride loop, 16-byte loads from the first 16-byte boundary on, the elements before
 * it and behind the last full vector one by one, a reduction over the wave and the block, then at most one 32-bit integer
 * atomicAdd and one atomicMax per block.  Integer add and max commute: the record is a pure function of what was folded in.
 * No float accumulation.  count > INT32_MAX: CLV_ERR_UNSUPPORTED; NULL / misaligned arguments, count < 0, an unknown elem:
 * CLV_ERR_ARG.
 *
 * clv_act_report_latch, for use behind clv_optim_prep: when state.skip == 0 it returns at once and `latched` keeps every
 * byte (mode 0 of clv_grad_report); on a skipped step it writes {int32 t, skipped; float loss_scale (the one the gradients
 * carried: state.grad_loss_scale); int32 n_slots; 4 x int32 0} — the gradient report's header — followed by a copy of the
 * n_slots records at `live`.  latched: CLV_GRAD_REPORT_HEADER_BYTES + CLV_ACT_REPORT_SLOT_BYTES * n_slots bytes; live and
 * latched 16-byte aligned.  One small launch.
 * Both are plain launches on `stream`: capturable, they allocate nothing and synchronise nothing. */
#define CLV_ACT_REPORT_SLOT_BYTES 16
int clv_act_report(const void* x, int64_t count, int32_t elem, void* slot, void* stream);
int clv_act_report_latch(const void* state, const void* live, void* latched, int32_t n_slots, void* stream);

/* ------------------------------------------------------------------ parity mode (fp32 storage + fp32 arithmetic)
 * The reference's CPU path is fp32 (north_star: "match the reference mmaction CPU path ... losses within 1e-3").  The
 * training path above computes on bf16 MFMA operands; these two entry points let the SAME host graph (registered modules,
 * window geometry, token maps, bias-table indexing, masks, heads, losses) run with fp32 storage and fp32 arithmetic so the
 * step losses can be asserted at 1e-3 against the reference goldens, and the gradients at fp32 tolerances.
 *
 * clv_sgemm_nt: C[M][N] (ldc) = A[M][K] (lda) . B[N][K]^T (ldb) + bias[N] — every nn.Linear of the path
 *   (swin_transformer_3d.py:257-259,361-366,527; transformers BertSelfAttention / BertIntermediate / BertOutput as called
 *   from bert_from_hugface.py:30, cross_transformer.py:109-110; mlm_itm_head.py:33-41) on the exact-f32 MFMA 16x16x4.
 * clv_attn_f32_fwd: clv_attn_fwd's arithmetic (both modes, same ClvAttnGeom, strides in floats) on fp32 q / k / v / o;
 *   round_p != 0 rounds the un-normalised probabilities to bf16 before P.V (emulates the MFMA kernels' P operand — used
 *   by the error-isolation runs recorded in DESIGN.md). */
int clv_sgemm_nt(const float* A, const float* B, const float* bias, float* C, int64_t M, int32_t N, int32_t K,
                 int64_t lda, int64_t ldb, int64_t ldc, void* stream);
/* fp32 GEMM with general strides — the [batch, D]-sized projection heads of the contrastive losses (ssl_head.py:24-35,
 * 158-166,240-245; the reference forces fp32 there, contrastive_loss.py:102), on the training path too:
 * C[i][j] (ldc) (+)= sum_k A[i*sai + k*sak] * B[j*sbj + k*sbk] (+ bias[j]);  accumulate != 0: added into C (the fp32 gradient
 * slab).  Forward x W^T, input gradient dy W and weight gradient dy^T x are this one kernel with different strides. */
int clv_sgemm_strided(const float* A, const float* B, const float* bias, float* C, int64_t M, int32_t N, int32_t K,
                      int64_t sai, int64_t sak, int64_t sbj, int64_t sbk, int64_t ldc, int32_t accumulate, void* stream);
/* The same with rowsum[i] (+)= sum_k A[i*sai + k*sak] from the same launch (ABI 13): the weight-gradient form of a head layer
 * (A = dy^T) delivers the bias gradient with it.  Contractions K <= 96 only (the rows of a batch), else CLV_ERR_UNSUPPORTED. */
int clv_sgemm_strided_rowsum(const float* A, const float* B, float* C, float* rowsum, int64_t M, int32_t N, int32_t K,
                             int64_t sai, int64_t sak, int64_t sbj, int64_t sbk, int64_t ldc, int32_t accumulate,
                             void* stream);
int clv_attn_f32_fwd(const float* q, const float* k, const float* v, float* o, const float* bias, const int32_t* rid,
                     const float* kmask, const ClvAttnGeom* geom, int32_t round_p, void* stream);
/* Backward of clv_attn_f32_fwd in fp32 (ABI 8): dq / dk / dv with the strides of q / k / v, dbias (may be NULL) ACCUMULATED
 * into the [rows, nH] relative-position table gradient (WindowAttention3D, swin_transformer_3d.py:375-400; HF
 * BertSelfAttention in mode 0), work = clv_attn_f32_bwd_work_floats(geom) floats (lse and delta per (group, head, query)).
 * Two recompute passes, one writer per output element: parity mode checks the step's gradients with it. */
int64_t clv_attn_f32_bwd_work_floats(const ClvAttnGeom* geom);
int clv_attn_f32_bwd(const float* q, const float* k, const float* v, const float* dout, const float* bias,
                     const int32_t* rid, const float* kmask, float* dq, float* dk, float* dv, float* dbias, float* work,
                     const ClvAttnGeom* geom, void* stream);

/* ------------------------------------------------------------------ fp8 forward GEMMs (BASELINE config 5)
 * "fp8 MFMA QKV / patch-proj path": the forward GEMM of a Linear on OCP e4m3 operands with one fp32 scale per row of
 * each operand (per token for the activation, per output channel for the weight), fp32 accumulation on the K = 128 matrix
 * instruction (v_mfma_f32_16x16x128_f8f6f4, twice the bf16 MFMA rate), bf16 output; gradients stay bf16 (the backward
 * takes the bf16 activation and weight).  Replaces, under CLOVER_FP8=1, the same torch.nn.Linear sites as clv_gemm_nt
 * (swin_transformer_3d.py:257-268,361-366,527; the transformers BERT layers called from bert_from_hugface.py:30 and
 * cross_transformer.py:109-110); precision policy site: mmaction/core/hooks/fp16_utils.py:215-259.
 *
 * clv_quant_fp8_rows: q[r][k] = e4m3(x[r][k] / scale[r]), scale[r] = max_k |x[r][k]| / 448; x bf16 [rows][K] (ldx),
 *   q bytes [rows][K] (ldq); K % 8 == 0, K <= 4096.
 * clv_gemm_nt_fp8: c[M][N] bf16 = (a8[M][K] . b8[N][K]^T) * sa[m] * sb[n] (+ bias; CLV_GEMM_EPI_NONE / _BIAS / _BIAS_GELU_D
 *   with c2 = GELU'(pre) as clv_gemm_nt); K % 128 == 0, lda / ldb in bytes and % 16 == 0. */
/* clv_patch_embed_fwd with the projection on the fp8 matrix instruction: w8 [C][96] e4m3 bytes + wscale [C] (the conv
 * weight through clv_quant_fp8_rows); each token's 96 patch values are scaled by 448 / their maximum and converted to
 * e4m3 inside the kernel.  Everything else (bias, LayerNorm, blend, outputs, saved tensors) as clv_patch_embed_fwd; the
 * backward is the bf16 one. */
int clv_patch_embed_fwd_fp8(const float* x, const void* w8, const float* wscale, const float* bias, const float* gamma,
                            const float* beta, const float* mask_token, const int64_t* vmask, void* out_clean,
                            void* out_masked, void* z_out, float* mean, float* rstd, int32_t B, int32_t T, int32_t H,
                            int32_t W, int32_t C, int32_t mh, int32_t mw, float eps, void* stream);
int clv_quant_fp8_rows(const void* x, void* q, float* scale, int64_t rows, int32_t K, int64_t ldx, int64_t ldq,
                       void* stream);
int clv_gemm_nt_fp8_supported(int64_t M, int32_t N, int32_t K);
int clv_gemm_nt_fp8(const void* a8, const void* b8, const float* sa, const float* sb, const float* bias, void* c, void* c2,
                    int64_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc, int32_t epilogue,
                    void* stream);

/* Data-parallel gradient exchange in bf16 (the reference all-reduces the fp16 model gradients:
 * mmaction/core/hooks/mmcv_Fp16OptimizerHook.py:119-122): clv_pack_bf16 writes the bf16 wire copy of an fp32 gradient-slab
 * slice (RCCL all-reduces THAT over xGMI: half the bytes), clv_sumsq_bf16 / clv_adamw_step_dev_bf16g are clv_sumsq /
 * clv_adamw_step_dev reading the reduced bf16 gradient — the update itself (moments, master weights) stays fp32. */
int clv_pack_bf16(const float* src, void* dst, int64_t n, void* stream);
int clv_sumsq_bf16(const void* g, float* acc, int64_t n, void* stream);
int clv_adamw_step_dev_bf16g(float* p, const void* g, float* m, float* v, void* shadow, const void* state, int64_t n,
                             float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);
/* clv_optim_plan (host only, no GPU needed; one symbol added to ABI 20 — a new symbol, nothing existing changes, the version
 * stays): the launch of one optimizer pass over n elements.  kind 0: clv_sumsq /
 * clv_sumsq_bf16; 1: clv_adamw_step / clv_adamw_step_dev / clv_adamw_step_dev_bf16g; 2: clv_pack_bf16.  The launchers take
 * their grid from the helper this entry reports, so the two cannot drift apart.
 *   grid, block  workgroups (kind 0: at most 2048, grid-stride; kind 1: at most 2^20, grid-stride; kind 2: one 4-element
 *                group per thread and no loop — n beyond 2^30 is CLV_ERR_UNSUPPORTED, here and in clv_pack_bf16) and threads
 *   trips        4-element groups the busiest thread walks (0 when n < 4)
 *   tail         n % 4: elements the first `tail` threads of workgroup 0 take one by one */
typedef struct ClvOptimPlan {
    int32_t grid, block, trips, tail;
} ClvOptimPlan;
int clv_optim_plan(int32_t kind, int64_t n, ClvOptimPlan* out);

/* ------------------------------------------------------------------ video QA / fill-in-the-blank fine-tuning (csrc/qa.hip)
 * clv_qa_answer_rows: the row table of the QA head into the fusion output [N, Ltot, D] viewed as [N * Ltot, D], built on
 *   the device from the captions (no host sync, capturable):
 *     mode 0 (answer_cls, multimodal_transformer_finetune.py:103-107 / :173-177): rows[n] = n * Ltot + base (the text CLS
 *       row, base = n_vis, or the fusion CLS row, base = n_vis - 1), counts[n] = 1;
 *     mode 1 (answer_mask, :100-102 / :170-172 `torch.where(token_ids == 103)`): rows[n] = n * Ltot + base + the FIRST
 *       position l < L with token_ids[n][l] == mask_id, counts[n] = how many there are (the data contract is exactly one;
 *       a sequence without one points at offset 0).  token_ids int64 [N, L]; counts may be NULL. */
int clv_qa_answer_rows(const int64_t* token_ids, int32_t N, int32_t L, int32_t Ltot, int32_t base, int32_t mode,
                       int64_t mask_id, int32_t* rows, int32_t* counts, void* stream);
/* The fused QA head (QA_MC_head / QA_OE_Head, mmaction/models/heads/qa_head.py:8-85):
 *   logits = Linear(H, K)(GELU(LayerNorm(Linear(D, H)(Dropout(p)(x[rows])))))  (LayerNorm eps, erf-GELU)
 * x: bf16 rows of width D (row stride D) addressed by rows int32 [M]; w1 fp32 [H][D], b1 / gamma / beta [H], w2 [K][H],
 * b2 [K]; seed: the device-resident uint64 dropout seed (keep_scale of (seed, head row, column); NULL when drop_p == 0).
 * Outputs fp32: z = the Linear(D, H) output and g = GELU(LayerNorm(z)) [M][H], mean / rstd [M], logits [M][K].  Two
 * launches for K > 1 (row-block kernel + the H -> K GEMM), one for K == 1 (the dot product rides in the row-block kernel).
 * Supported: D <= 1024, H <= 512 (clv_qa_head_supported). */
int clv_qa_head_supported(int32_t D, int32_t H, int32_t K);
int clv_qa_head_fwd(const void* x, const int32_t* rows, const float* w1, const float* b1, const float* gamma,
                    const float* beta, const float* w2, const float* b2, const uint64_t* seed, float drop_p, float eps,
                    float* z, float* g, float* mean, float* rstd, float* logits, int32_t M, int32_t D, int32_t H, int32_t K,
                    void* stream);
/* Multiple-choice loss (:109-121 `qa_head(x).view(-1, C)` + CrossEntropyLoss): logits fp32 [B][C], labels int64 [B];
 * out[0] = mean CE over the samples with 0 <= label < C, out[1] = 1 / their count; dprob [B][C] = softmax - onehot (the
 * loss gradient before out[1] and the incoming gradient).  One launch. */
int clv_qa_mc_ce_fwd(const float* logits, const int64_t* labels, float* dprob, float* out, int32_t B, int32_t C,
                     void* stream);
/* Backward of clv_qa_head_fwd for dlogits = dl [M][K] * (*s1) * (*s2) (either scale pointer may be NULL = 1): the input
 * gradient is STORED as bf16 into dx_full at rows[i] (the caller zero-fills the rest of it), the parameter gradients are
 * ADDED into fp32 dw1 [H][D], db1, dgamma, dbeta [H], dw2 [K][H], db2 [K]; dy / dz fp32 [M][H] are scratch.  Two launches;
 * the dropout mask is regenerated from the forward's seed. */
int clv_qa_head_bwd(const void* x, const int32_t* rows, const float* w1, const float* gamma, const float* beta,
                    const float* w2, const float* z, const float* g, const float* mean, const float* rstd, const float* dl,
                    const float* s1, const float* s2, const uint64_t* seed, float drop_p, float* dy, float* dz,
                    void* dx_full, float* dw1, float* db1, float* dgamma, float* dbeta, float* dw2, float* db2, int32_t M,
                    int32_t D, int32_t H, int32_t K, void* stream);
/* Multiple-choice fusion input (multimodal_transformer_finetune.py:90-95 `visual_token.unsqueeze(1).expand(-1, C, ...)` +
 * cross_transformer.py:112 `torch.cat([visual_token, text_embeddings], dim=1)`): feat bf16 [B*C][n_vis + L][D] =
 * [visual[b] ; text[b*C + c]] from the per-video rows visual [B][n_vis][D] and the captions text [B*C][L][D].  The
 * backward writes dvisual [B][n_vis][D] = the sum over the C candidates (fp32, one rounding) and dtext [B*C][L][D].
 * D % 8 == 0; one launch each. */
int clv_qa_choice_assemble(const void* visual, const void* text, void* feat, int32_t B, int32_t C, int32_t n_vis,
                           int32_t L, int32_t D, void* stream);
int clv_qa_choice_assemble_bwd(const void* dfeat, void* dvisual, void* dtext, int32_t B, int32_t C, int32_t n_vis,
                               int32_t L, int32_t D, void* stream);
/* forward_test's `output['attentions'][-1].mean(dim=1)` (:189): from the last fusion layer's packed qkv bf16 [N][S][3 nH hd]
 * and its additive key mask fp32 [N][S] (may be NULL), out fp32 [N][S][S] = mean over the nH heads of
 * softmax(q_h k_h^T * scale + kmask).  S <= 4096, hd <= 128 and even. */
int clv_attn_probs_mean(const void* qkv, const float* kmask, float* out, int32_t N, int32_t S, int32_t nH, int32_t hd,
                        float scale, void* stream);
/* The fp32-storage forms of the entries above, for parity mode (CLOVER_PARITY: fp32 storage and fp32 arithmetic, as
 * clv_attn_f32_fwd / _bwd): the SAME kernel bodies instantiated with float activations, so the same arithmetic, the same
 * dropout mask of (seed, row, column), the same limits (clv_qa_head_supported; S <= 4096, hd <= 128 and even) and return
 * codes as their 16-bit counterparts, argument for argument.
 *   clv_qa_head_f32_fwd / _bwd (qa_head.py:8-85): x and dx_full are fp32 rows of width D; the input gradient is stored
 *     unrounded at rows[i].
 *   clv_qa_choice_assemble_f32 / _f32_bwd (multimodal_transformer_finetune.py:87-123, :90-95 the expand over the
 *     candidates): 16-byte copies of 4 floats, so D % 4 == 0; dvisual = the fp32 sum over the C candidates, stored as it
 *     is (no rounding at all).
 *   clv_attn_probs_mean_f32 (multimodal_transformer_finetune.py:157-193, :189 the head mean): qkv fp32 [N][S][3 nH hd]. */
int clv_qa_head_f32_fwd(const float* x, const int32_t* rows, const float* w1, const float* b1, const float* gamma,
                        const float* beta, const float* w2, const float* b2, const uint64_t* seed, float drop_p,
                        float eps, float* z, float* g, float* mean, float* rstd, float* logits, int32_t M, int32_t D,
                        int32_t H, int32_t K, void* stream);
int clv_qa_head_f32_bwd(const float* x, const int32_t* rows, const float* w1, const float* gamma, const float* beta,
                        const float* w2, const float* z, const float* g, const float* mean, const float* rstd,
                        const float* dl, const float* s1, const float* s2, const uint64_t* seed, float drop_p, float* dy,
                        float* dz, float* dx_full, float* dw1, float* db1, float* dgamma, float* dbeta, float* dw2,
                        float* db2, int32_t M, int32_t D, int32_t H, int32_t K, void* stream);
int clv_qa_choice_assemble_f32(const float* visual, const float* text, float* feat, int32_t B, int32_t C, int32_t n_vis,
                               int32_t L, int32_t D, void* stream);
int clv_qa_choice_assemble_f32_bwd(const float* dfeat, float* dvisual, float* dtext, int32_t B, int32_t C, int32_t n_vis,
                                   int32_t L, int32_t D, void* stream);
int clv_attn_probs_mean_f32(const float* qkv, const float* kmask, float* out, int32_t N, int32_t S, int32_t nH,
                            int32_t hd, float scale, void* stream);

/* Text -> video retrieval ranks without the score matrix (the metric of mmaction/core/evaluation/accuracy.py:430-462 with
 * normalize_fn of mmaction/utils/numpy_norm.py:5-8).  query fp32 [Nq][D] (row stride ldq), gallery fp32 [Ng][D] (ldg): rows
 * are scaled to unit L2 norm (IEEE sqrt and division; an all-zero row stays zero), s[i][j] = q_i . g_j on the exact-f32
 * MFMA 16x16x4.  gt int32 [Nq]: the gallery row that is query i's ground truth (NULL: gt[i] = i, needs Nq <= Ng).
 *   rank[i]     = #{j : s[i][j] > s[i][g]} + #{j < g : s[i][j] == s[i][g]}: the 0-based position of g = gt[i] in the STABLE
 *                 descending order of row i (j == g is excluded by index); -1 where gt[i] < 0 or gt[i] >= Ng
 *   gt_score[i] = s[i][g] (NaN where rank[i] = -1)
 *   topk_idx / topk_score [Nq][topk] (topk 1..16; 0 = off, both may be NULL): the first topk entries of that same order,
 *                 padded with -1 / -inf when Ng < topk.
 * work: clv_retrieval_work_bytes(...) bytes, 16-byte aligned; nothing is allocated inside, every launch goes to `stream`
 * (capturable).  D % 4 == 0, 4 <= D <= 4096, topk <= 16, Nq, Ng >= 1, else CLV_ERR_UNSUPPORTED (the size query returns the
 * same code).  Results are deterministic: counts meet through int32 adds. */
int64_t clv_retrieval_work_bytes(int64_t Nq, int64_t Ng, int32_t D, int32_t topk);
int clv_retrieval_rank(const float* query, const float* gallery, const int32_t* gt, int32_t* rank, float* gt_score,
                       int32_t* topk_idx, float* topk_score, void* work, int64_t Nq, int64_t Ng, int32_t D, int64_t ldq,
                       int64_t ldg, int32_t topk, void* stream);

/* The best gallery row inside a per-query range, and its rank (zero-shot multiple choice: acc_for_msrvtt_mc,
 * mmaction/core/evaluation/accuracy.py:396-427, without the [N][C N] matrix whose block diagonal it keeps; the video -> text
 * direction of a test set whose videos have several captions each).  query / gallery as clv_retrieval_rank, rows scaled by
 * 1 / max(norm, eps) (sim_matrix, accuracy.py:385-394, passes 1e-8; eps = 0 is clv_retrieval_rank's normalisation: an
 * all-zero row stays zero), s[i][j] by the tile loop of clv_retrieval_rank: bit-equal to the scores it compares.
 * lo, hi int32 [Nq]: query i looks at the gallery rows [lo[i], hi[i]); both NULL: at the whole gallery.
 *   best_idx[i]   = the FIRST j in [lo[i], hi[i]) that attains max s[i][j] over that range (torch.argmax's tie rule);
 *                   -1 where the range is empty or leaves [0, Ng]
 *   best_score[i] = that maximum (NaN where best_idx[i] = -1)
 *   rank[i]       (may be NULL: not computed) = clv_retrieval_rank's rank with gt = best_idx: the 0-based position of
 *                   best_idx[i] in the stable descending order of the WHOLE row i; -1 where best_idx[i] = -1.  With the
 *                   range = the captions of video i this is the usual video -> text rank: no other caption of the set
 *                   scores higher than the best one or ties in front of it.
 * A workgroup (64 queries) walks only the gallery tiles that meet [min lo, max hi) of its queries.
 * work: clv_retrieval_group_work_bytes(...) bytes, 16-byte aligned; nothing is allocated inside, every launch goes to
 * `stream` (capturable).  Shape limits and error codes of clv_retrieval_rank.  Results are deterministic: the chunks of a
 * long gallery meet in a merge ordered by (score descending, index ascending), ranks through int32 adds. */
int64_t clv_retrieval_group_work_bytes(int64_t Nq, int64_t Ng, int32_t D);
int clv_retrieval_group_best(const float* query, const float* gallery, const int32_t* lo, const int32_t* hi,
                             int32_t* best_idx, float* best_score, int32_t* rank, void* work, int64_t Nq, int64_t Ng,
                             int32_t D, int64_t ldq, int64_t ldg, float eps, void* stream);

/* Dual-softmax re-scoring of text -> video retrieval at inference: s'[i][j] = s[i][j] * softmax_i(T s[i][j]), the softmax
 * taken down the QUERY axis (a gallery row that scores high for every query is damped for all of them).  Two entries, no
 * [Nq][Ng] matrix; query / gallery / normalisation / s[i][j] as clv_retrieval_rank (bit-equal scores).
 *
 * clv_retrieval_col_stats: for every gallery row j, over ALL Nq queries,
 *   col_max[j] = m_j = max_i T s[i][j]            col_sum[j] = l_j = sum_i exp(T s[i][j] - m_j)        (float [Ng] each)
 * A workgroup owns 64 gallery rows and walks the queries with an online max / sum; a long query set is split over
 * workgroups whose partials are joined in chunk order (no float atomics): results are deterministic.  T = 0 gives
 * m_j = 0 and l_j = Nq exactly (Nq <= 2^24).
 *
 * clv_retrieval_rank_prior: clv_retrieval_rank's outputs and rules (rank, gt_score, topk_idx / topk_score, stable
 * descending order, ties by index, -1 / NaN where gt is out of range) on the compared value
 *   s'[i][j] = s[i][j] * exp(T s[i][j] - col_max[j]) / col_sum[j]                (fp32, one rounding per operation)
 * with col_max / col_sum as clv_retrieval_col_stats wrote them for the same operands and T; gt_score and topk_score are s'.
 *
 * work: clv_retrieval_col_stats_work_bytes(...) / clv_retrieval_rank_prior_work_bytes(...) bytes, 16-byte aligned (the two
 * calls may share one area of the larger size); nothing is allocated inside, every launch goes to `stream` (capturable).
 * Shape limits and error codes of clv_retrieval_rank; T finite and >= 0 (T s must stay finite), else CLV_ERR_ARG. */
int64_t clv_retrieval_col_stats_work_bytes(int64_t Nq, int64_t Ng, int32_t D);
int clv_retrieval_col_stats(const float* query, const float* gallery, int64_t Nq, int64_t Ng, int32_t D, int64_t ldq,
                            int64_t ldg, float T, float* col_max, float* col_sum, void* work, void* stream);
int64_t clv_retrieval_rank_prior_work_bytes(int64_t Nq, int64_t Ng, int32_t D, int32_t topk);
int clv_retrieval_rank_prior(const float* query, const float* gallery, const int32_t* gt, int32_t* rank, float* gt_score,
                             int32_t* topk_idx, float* topk_score, void* work, int64_t Nq, int64_t Ng, int32_t D,
                             int64_t ldq, int64_t ldg, int32_t topk, const float* col_max, const float* col_sum, float T,
                             void* stream);

/* ------------------------------------------------------------------ clip preparation (csrc/clip_prep.hip)
 * Decoded uint8 frames -> the normalised clip the recognizers take, in one launch: the reference's
 * RandomResizedCrop / CenterCrop -> Resize(S, bilinear) -> Flip -> Normalize -> FormatShape('NCTHW_TSN')
 * (mmaction/datasets/pipelines/augmentations.py:894-942, 1090-1180, 1560-1640, 1690-1740; formating.py FormatShape), run on
 * the device from one crop box and one flip flag per sample.  Three symbols added to ABI 20 — new symbols, nothing existing
 * changes, the version stays.
 *   src      uint8 [B, T, Hs, Ws, 3]: channel-last as decoded, channel order as stored (the reference normalises with
 *            to_rgb=False); mean / inv_std follow that order
 *   boxes    int32 [B, 4] (left, top, right, bottom) in source pixels, right / bottom exclusive; one box per sample, shared
 *            by its T frames
 *   flips    uint8 [B], non-zero = mirror horizontally
 *   mean, inv_std  float [3]
 *   out      [B, 1, 3, T, S, S], fp32 (out_dtype 0) or the library's 16-bit element type (out_dtype 1); 16-byte aligned
 * Per output element (c, t, y, x) of sample b, with bw = right - left, bh = bottom - top:
 *   xe = flips[b] ? S - 1 - x : x;   sx = clamp((xe + 0.5) * bw / S - 0.5, 0, bw - 1)   (half-pixel centres, clamped to the
 *   crop's first and last pixel centre);  x0 = floor(sx), x1 = min(x0 + 1, bw - 1), fx = sx - x0;  sy, y0, y1, fy likewise.
 *   The four neighbours are clamped to the CROP BOX, not the frame — the geometry of mmcv.imresize(crop, 'bilinear').
 *   v = bilinear blend in fp32;  out = (v - mean[c]) * inv_std[c], rounded once on store.  No antialiasing (the reference
 *   has none).  The blend stays in fp32 where the reference rounds the resized image to uint8 first (deviation D2).
 * Supported set — clv_clip_prep_supported is its single statement (host only, no GPU needed; box_w = right - left, box_h =
 * bottom - top of one box); it returns 0 or
 *   CLV_CLIP_BAD_CHANNELS  C != 3
 *   CLV_CLIP_BAD_FRAME     Hs < 1 or Ws < 1
 *   CLV_CLIP_BAD_SIZE      S not a multiple of 8 in [8, 2048] (a lane owns 8 adjacent x: every store a 16-byte vector)
 *   CLV_CLIP_BAD_BOX       not 1 <= box_w <= Ws and 1 <= box_h <= Hs
 * Any Hs, Ws, T, B (B * T * strips < 2^31).
 * clv_clip_prep_plan (host only): the launch of a shape — the launcher takes its grid from the same helper.
 *   cls            CLV_CLIP_CLASS_PLANE: S * S / 8 <= 256, one workgroup per frame writes the whole plane in one pass;
 *                  CLV_CLIP_CLASS_STRIPS: `strips` workgroups per frame, each `passes` passes of `rows_per_pass` rows
 *   grid, block    workgroups (B * T * strips) and threads
 *   lanes_per_row  S / 8;  idle_lanes: threads of a workgroup behind its last whole row
 *   tail_rows      rows of a frame's last strip when that strip is a partial one, else 0
 * clv_clip_prep: the launcher (asynchronous on `stream`, allocates nothing, capturable).  Outside the supported set:
 * CLV_ERR_UNSUPPORTED; NULL / misaligned pointers, B or T < 1, an unknown out_dtype: CLV_ERR_ARG.  `boxes` lives on the
 * device, so the launcher cannot read it without a sync: a caller that has the boxes on the host hands them in
 * geom->boxes_host (int32 [B, 4], may be NULL) and gets CLV_ERR_UNSUPPORTED for a box extent outside the set and
 * CLV_ERR_ARG for a box outside the frame, before any launch.  Whatever `boxes` holds, the kernel clamps the box into the
 * frame and to at least one pixel, so no box reads outside src. */
#define CLV_CLIP_BAD_CHANNELS 1
#define CLV_CLIP_BAD_FRAME 2
#define CLV_CLIP_BAD_SIZE 3
#define CLV_CLIP_BAD_BOX 4
#define CLV_CLIP_OUT_F32 0
#define CLV_CLIP_OUT_HALF 1
#define CLV_CLIP_CLASS_PLANE 0
#define CLV_CLIP_CLASS_STRIPS 1
typedef struct ClvClipPrepGeom {
    int32_t B, T, Hs, Ws, C, S, out_dtype, pad;
    const int32_t* boxes_host;
} ClvClipPrepGeom;
typedef struct ClvClipPrepPlan {
    int32_t cls, grid, block, lanes_per_row, rows_per_pass, passes, strips, tail_rows, idle_lanes;
} ClvClipPrepPlan;
int clv_clip_prep_supported(int32_t C, int32_t Hs, int32_t Ws, int32_t S, int32_t box_w, int32_t box_h);
int clv_clip_prep_plan(const ClvClipPrepGeom* geom, ClvClipPrepPlan* out);
int clv_clip_prep(const uint8_t* src, const int32_t* boxes, const uint8_t* flips, const float* mean, const float* inv_std,
                  void* out, const ClvClipPrepGeom* geom, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLOVER_HIP_H */
