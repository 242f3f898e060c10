/* d3pm_hip.h -- C ABI of the MI355X (gfx950) D3PM codec-token sampler.
 *
 * The upstream project has no FFI layer: its boundary is the Python module API
 * (vall_e.vall_e.get_model / AR.generate_audio).  This header is the C-ABI that
 * sits *below* that Python surface; each entry point names the reference statements it replaces
 * (paths relative to /root/reference/vall_e/vall_e/).
 *
 * Conventions
 *   - the library keeps NO mutable process-wide state (thread-compatible): schedule choices travel in `d3pm_tuning`
 *     through the shape structs, timing hooks in a caller-owned `d3pm_prof`; the only thread-local is the error string;
 *   - every pointer marked "device" is HBM memory owned by the caller (e.g. a torch tensor's
 *     data_ptr()); nothing is allocated, freed or synchronised inside the library;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*), so calls are capturable
 *     in a hipGraph and ordered with the caller's other work on that stream;
 *   - return value: 0 = ok, <0 = error (see D3PM_E_*); nothing throws across the ABI;
 *     d3pm_last_error() gives a thread-local message for the last failure;
 *   - `dtype` selects storage *and* arithmetic of the denoiser: F32 (exact-f32 FMA path, the
 *     1e-3 logits-parity mode), F16 (the only dtype the reference sampler runs in) or BF16.
 *     Accumulation is always fp32; every op output is rounded to `dtype` where the reference's
 *     eager model rounds.  The posterior/sampling arithmetic is fp16 in every mode, as upstream
 *     (its tables are hard-cast to fp16, ar_discrete.py:257-277).
 *   - token ids are int32, row-major [batch][canvas]; activations are [batch*canvas][d_model].
 */
#ifndef D3PM_HIP_H
#define D3PM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only what this header declares is exported */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* 2: + d3pm_ce_loss_rows, the fp8 entry points (d3pm_*_fp8), D3PM_FLAG_SEED_IN_HBM, tuning knobs 2..3, GEMM variant 5
 *    (additions only) */
/* 3: + d3pm_op_final_sample, d3pm_op_cond_embed, the fp32 training ops (d3pm_op_*_f32), d3pm_op_linear_rowpanel / _lnpro,
 *    d3pm_prof_read_class, d3pm_debug_gemm_clock [since removed], tuning knobs 4..11, GEMM variants 6..8; the kernel class D3PM_K_GEMM_LN took
 *    the value 4, so "every class" (D3PM_K_COUNT) is now 5 */
/* 4: the tuning knobs moved from process-wide state (d3pm_set_tuning) into `d3pm_tuning`, reached through the shape structs
 *    (and a trailing argument of d3pm_op_linear / d3pm_op_attention); the profiling hooks became a handle (d3pm_prof);
 *    the library keeps no mutable global state besides the thread-local error string.  The experiment-only entry points
 *    (d3pm_set_tuning's ablation arms, d3pm_op_final_sample, d3pm_op_linear_lnpro, d3pm_debug_gemm_clock) left the product:
 *    built, measured, not shipped; the experiment library that carried them afterwards (libd3pm_hip_ab.so) is retired, source up to
 *    commit d54b189. */
/* 5: + d3pm_op_attention_pair; new VALUES of existing tuning fields (row_panel bit 3, attn_query_groups 4, attn_cross_resident
 *    4 / 5); layouts unchanged */
/* 6: LayerNorm folded into the projections (d3pm_fold_block, d3pm_weights.fold, d3pm_fold_bytes / d3pm_fold_build,
 *    d3pm_op_linear_fold / d3pm_op_linear_stats / d3pm_op_row_stats); d3pm_tuning gained regime_batch and ln_fold (layout change);
 *    d3pm_workspace_bytes grew by the row-moment buffer and the fp8 path's scale slot;
 *    later additions only: the condition encoders' training-step dropout (d3pm_op_dropout_f32, d3pm_op_attention_dropout_f32,
 *    d3pm_op_attention_bwd_dropout_f32); per-utterance canvases (d3pm_canvas, d3pm_denoise_step_canvas,
 *    d3pm_posterior_sample_known, d3pm_sample_loop_canvas, d3pm_sample_loop_fp8_canvas); temperature / top-k on the x0-logits
 *    (d3pm_sampling, d3pm_posterior_sample_sampling, d3pm_sample_loop_sampling); the nucleus (top-p) cut behind them
 *    (d3pm_nucleus, d3pm_posterior_sample_nucleus, d3pm_sample_loop_nucleus); the confidence-ordered reveal schedule
 *    (d3pm_reveal, d3pm_reveal_plan, d3pm_reveal_step, d3pm_reveal_loop); the per-utterance key mask at kernel level
 *    (d3pm_op_attention_keylen); key-padding masks through the denoiser (d3pm_keys, d3pm_encode_conditions_keys,
 *    d3pm_denoise_step_keys, d3pm_sample_loop_keys, d3pm_reveal_loop_keys, d3pm_op_attention_pair_keylen); classifier-free guidance
 *    inside the sampler launch (d3pm_guidance, d3pm_posterior_sample_guided, d3pm_sample_loop_guided); block-0 QKV from a per-id
 *    table (d3pm_op_embed_qkv_bytes, d3pm_op_embed_qkv; ln_fold value 2; d3pm_workspace_bytes grew by the table and one
 *    [rows][d_model] region for 16-bit models with d_model a multiple of 256 and n_q <= 1); one row per distinct token of an
 *    utterance in the unguided loops (d3pm_op_dedup_index, d3pm_op_linear_live; ln_fold value 3 = every row); its self-attention
 *    with the keys read through a row index (d3pm_op_attention_gather); the segment granularity of that index
 *    (d3pm_op_dedup_index_align: 1 = dense segments, what the loop runs; d3pm_op_attention_gather and
 *    d3pm_op_attention_pair_segments take a segment of any length at any row); key-padding masks in the training step
 *    (d3pm_op_attention_bwd_keylen_f32, d3pm_op_attention_dropout_keylen_f32); the NAR stage's own kernels one at a time
 *    (d3pm_op_nar_embed, d3pm_op_adaln, d3pm_op_nar_sample); the latency GEMM family in the iterations of the deduplicated loop
 *    that have few live rows (d3pm_op_linear_live_est; ln_fold value 4 = the deduplicated loop without that switch); the per-frame
 *    log-probability of the revealed id from either loop (d3pm_frame_scores, d3pm_frame_scores_init, d3pm_frame_scores_step,
 *    d3pm_sample_loop_scored, d3pm_reveal_loop_scored); the reveal schedule whose held frames compete again in every step
 *    (d3pm_revise, d3pm_reveal_step_revise, d3pm_reveal_loop_revise); the self-attention of the few-row iterations of the
 *    deduplicated loop with an utterance's distinct K | V rows pooled in LDS (d3pm_op_attention_gather_pool); the NAR stage's
 *    training step (d3pm_op_adaln_bwd_f32, d3pm_op_nar_embed_bwd_f32, d3pm_op_nar_ce_f32); the NAR stage's level draw with known
 *    frames, top-k / top-p and log-probabilities (d3pm_nar_draw, d3pm_nar_level_draw, d3pm_op_nar_draw); classifier-free guidance
 *    in that draw (d3pm_nar_level_guided, d3pm_op_nar_draw_guided); the two-output LayerNorm -> MX launch as a single op
 *    (d3pm_op_layernorm_mx_pair) */
#define D3PM_ABI_VERSION 6

enum { D3PM_F32 = 0, D3PM_F16 = 1, D3PM_BF16 = 2 };

enum {
  D3PM_OK = 0,
  D3PM_E_ARG = -1,        /* null pointer / inconsistent sizes                     */
  D3PM_E_WORKSPACE = -2,  /* workspace smaller than d3pm_workspace_bytes()         */
  D3PM_E_HIP = -3,        /* a HIP runtime call or kernel launch failed            */
  D3PM_E_SHAPE = -4       /* shape not supported by any kernel in this build       */
};

/* flags for d3pm_sample_loop / d3pm_denoise_step */
enum {
  D3PM_FLAG_GREEDY = 1,        /* argmax of the posterior without Gumbel noise   */
  D3PM_FLAG_FORCE_GENERIC = 2, /* never take the MFMA kernels (cross-check / debugging)          */
  D3PM_FLAG_SEED_IN_HBM = 4    /* d3pm_sample_loop: `seed` is the address of a uint64 in HBM, read by the sampling
                                  kernel at run time -- a captured HIP graph of the loop can then be replayed with a
                                  new seed (measured: no faster than eager launches, 66.6 vs 66.3 ms per utterance) */
};

/* Schedule choices.  A NULL `tuning` pointer anywhere means d3pm_tuning_default().  The struct is read during the call and never
 * retained; two threads may use different tunings at the same time.  The GEMM / workspace / row-panel fields select between
 * schedules that give bit-identical results.  Three choices change the ORDER of a floating-point accumulation, i.e. results that
 * agree to rounding noise, not bit for bit: the attention instruction shape (attn_query_groups 32 / 33, attn_cross_resident 4 / 5,
 * and -- in auto mode -- the batch regime, see regime_batch) and ln_fold.  Within one setting of those a result never depends on
 * the batch an utterance rides in, nor on how a batch is split over ranks or streams.
 *   gemm_variant       0 = auto (default): the big-tile persistent schedule when the shape divides into whole tiles that fill >= 85 %
 *                          of their rounds over the CUs -- 192 x 128 tiles (four waves, two workgroups per CU) first, then 192 x 256,
 *                          then 96 x 512 (eight waves, one workgroup per CU); 192 x 128 also for mid-size batches that give at
 *                          least every (long K: every second) CU a tile; else the latency schedule (64 x 64 tiles, whole-K operand
 *                          panels in flight) for M <= 1536 rows, the 128 x 128 throughput schedule otherwise;
 *                      2 = always the throughput schedule (one LDS stage, 4 workgroups per CU; persistent over the 128 x 128
 *                          tiles when M and N are multiples of 128 and there are >= 512 tiles, else as 5);
 *                      3 = always the round-1 latency schedule (128 x 128 tiles, two stages, asm DMA prefetch);
 *                      4 = always the latency schedule (64 x 64 tiles, every DMA piece of K <= 512 in flight at once);
 *                      5 = throughput schedule with one tile per workgroup (the non-persistent form of 2);
 *                      6 / 7 / 8 = as auto, but only the 192 x 256 / 96 x 512 / 192 x 128 (two 4-wave workgroups per CU) big
 *                          tile is considered, for any shape made of whole tiles;
 *                      9 / 10 = as auto, but a projection onto the residual stream that leaves its row moments as quads (and the
 *                          dual cross-attention out-projection) takes the 96 x 128 / 128 x 128 tile (four waves of three / four
 *                          16-row blocks) for any shape made of whole tiles.  In auto mode the deduplicated sampler loop gives
 *                          these projections the shortest such tile whose tiles of the estimated distinct rows fit two per CU
 *                          in one round (12 288 / 16 384 rows at d_model = 512), and the 192 x 128 tile beyond.
 *   gemm_persist_slots resident workgroups of the persistent 128 x 128 schedule, a multiple of 8 (default 1024 = 4 per CU).
 *   lat_tile           tile of the latency GEMM: 0 = auto (fewest rounds over the 256 CUs, then most workgroups),
 *                      1 / 2 / 3 = always 64 x 64 / 96 x 64 / 32 x 64.
 *   attn_query_groups  schedule of the MFMA self-attention: 0 = auto -- the software-pipelined 32 x 32 x 16 kernel (one 32-query
 *                      group per wave, three workgroups per CU) for whole 128-query blocks and 64-key tiles once that grid has two
 *                      workgroups per CU, else the 16 x 16 x 32 kernel with 2 sixteen-query groups per wave when that still gives
 *                      >= 4 workgroups per CU, else 1; 1 or 2 = the 16 x 16 x 32 kernel with that many groups; 4 = the key-split
 *                      kernel (four waves share 32 queries and each walks every fourth 64-key tile, the partial softmax states
 *                      combined at the end; measured 2 % faster at one utterance and slower from two on, so never automatic);
 *                      32 = the 32 x 32 x 16 kernel wherever it applies; 33 = as 32 without the software pipeline.  (The schedules
 *                      accumulate in different orders: results agree to rounding noise, not bit for bit; within one schedule a
 *                      result does not depend on the batch it rides in.)
 *   attn_pair_sequential  a paired attention launch (text + prompt cross-attention) on the tile-by-tile kernel: 2 = every
 *                      workgroup runs both problems one after the other; 0 = the second half of the grid takes problem 2;
 *                      1 (default) = auto: sequential while that still leaves >= 2 workgroups per CU.
 *   attn_cross_resident  the cross-attention pair of a block (<= 64 and <= 256 keys) with every K / V tile of both problems
 *                      fetched into LDS once per (utterance, head) by a workgroup of eight waves that then walks that head's
 *                      256-query blocks: 2 = always, 0 = never (tile-by-tile kernel), 1 (default) = auto: when there is at least
 *                      one such workgroup per CU (batch >= 11 at 768 rows and 8 heads); 3 = as 2 with one query block per workgroup;
 *                      4 / 5 = as 2 on the 16 x 16 x 32 / the 32 x 32 x 16 instruction.  The resident kernel of 1 / 2 / 3 is the
 *                      32 x 32 x 16 one (the software-pipelined 32-key block of the self-attention kernel); the 16 x 16 x 32 form
 *                      (4) is bit-identical to the tile-by-tile kernel, the two instruction shapes accumulate in different orders.
 *   row_panel          bit mask of the block's projections that run as row-panel launches (d3pm_op_linear_rowpanel) when
 *                      d_model = 512, the dtype is 16-bit and batch * canvas is a multiple of 96: 1 = self-attention
 *                      out-projection + norm2 | norm22, 2 = both cross-attention out-projections + norm3 / FiLM, 4 = fc2 + the
 *                      next block's norm1; 8 = at one or two utterances (batch * canvas <= 2048 rows, where no row panel applies)
 *                      both cross-attention out-projections as ONE launch of the latency GEMM: two products through one resident
 *                      weight panel, the first result kept in registers (same bits as the two launches it replaces).
 *                      Default 10: in the sampler's loop the fc2 form (4) is slower fused, and since the plain projections run as two
 *                      4-wave workgroups per CU the self-attention form (1) is too (102.6 k vs 103.7 k tokens/s, round 3); the dual
 *                      cross-attention form (2) and the latency form (8) pay.
 *   workspace_alias    1 (default) = the packed qkv rows, the MLP hidden rows and the logits of an iteration share one
 *                      workspace region (never live together); 0 = separate regions.  d3pm_workspace_bytes and the step /
 *                      loop calls must see the same value.
 *   regime_batch       the batch size the AUTOMATIC attention choices (attn_query_groups = 0, attn_cross_resident = 1) are made
 *                      for: 0 (default) = the batch of the call itself; > 0 = as if the call carried that many utterances.  The two
 *                      instruction shapes accumulate in different orders, so a caller that splits one logical batch over ranks
 *                      or streams (vall_e/vall_e/dp.py, AR.generate_audio(streams=)) passes the GLOBAL batch here and every shard
 *                      then takes the kernels -- and produces the bits -- of the unsplit batch.
 *   ln_fold            1 (default) = when d3pm_weights.fold is given, the LayerNorm-fed projections (norm1 -> QKV, norm2 | norm22 ->
 *                      cross-attention queries, norm3 + FiLM -> fc1) read the raw residual stream and apply the LayerNorm in their
 *                      epilogue from row moments the producing projection left behind (d3pm_fold_block): no LayerNorm launch and
 *                      no row-panel launch in a block (one small launch per evaluation rebuilds fc1's FiLM-folded weights for
 *                      the timestep); 0 = the stand-alone / row-panel LayerNorm launches (the eager rounding points).  Ignored (= 0) for fp32 models, D3PM_FLAG_FORCE_GENERIC and the fp8 entry points.
 *                      With 1 the unguided sampler loops (d3pm_sample_loop and its _canvas / _sampling / _nucleus / _keys forms, n_q <= 1,
 *                      two iterations or more) also take the QKV rows of the FIRST block from a table: that projection reads
 *                      resps_emb[id] (zeros on a padded frame) under norm1 and nothing else, so it has n_classes + 1 distinct rows;
 *                      the loop computes them once per call with the folded projection itself and the launch that embeds a row
 *                      (the sampler launch of the previous iteration) copies its 3 d_model values.  One projection over all rows
 *                      less per iteration, same bits.  2 = the fold without the table: every block projects its QKV rows (the
 *                      guided loop, the reveal loop and d3pm_denoise_step do so under 1 as well).  1 and 2 give identical results;
 *                      d3pm_workspace_bytes is the same for every value.
 *                      With 1 those loops also evaluate ONE ROW PER DISTINCT TOKEN of an utterance wherever their launches run on
 *                      the big-tile GEMMs (moments as quads) and the 32 x 32 x 16 attention kernels: the denoiser adds no positional
 *                      term to the frames, so two frames of one utterance with the same id (or both padded) get the same logits bit
 *                      for bit; per iteration an index of the distinct rows is built on the device, every projection and attention
 *                      query runs on those rows alone (keys stay in canvas order), and the sampler, which is per position, reads
 *                      each frame's logits through the index.  3 = fold + table on every row (the launch list without the
 *                      deduplication).  1, 2 and 3 give identical ids.  3 is an A/B value OUTSIDE the shipped list: the library and
 *                      `bench.py --tune ln_fold=3` take it for measurements and tests, the Python `tuning()` context, which
 *                      admits shipped schedules only, refuses it (0, 1 and 2 are the shipped values).
 *                      With 1 an iteration of that loop whose live rows the host bounds by a small number -- batch * min(canvas,
 *                      2 + ceil(canvas * (1 - cbar[t]))) from the schedule, no read-back; loops without known frames -- runs the
 *                      projections of its blocks on the 64 x 64 latency family (moments as 32-column parts in that iteration) instead
 *                      of big tiles.  4 = the deduplicated loop with that switch off (big tiles in every iteration): like 3 an A/B
 *                      value outside the shipped list.  1, 3 and 4 give identical ids.
 *   prof               optional timing hooks (d3pm_prof_create below), NULL = none. */
struct d3pm_prof;
typedef struct d3pm_tuning {
  int32_t gemm_variant, gemm_persist_slots, lat_tile;
  int32_t attn_query_groups, attn_pair_sequential, attn_cross_resident;
  int32_t row_panel, workspace_alias;
  int32_t regime_batch, ln_fold;
  struct d3pm_prof *prof;
} d3pm_tuning;
void d3pm_tuning_default(d3pm_tuning *t);

typedef struct d3pm_shape {
  int32_t d_model;    /* 32 upstream (ar_discrete.py:208); 512 asked by get_model (__init__.py:26) */
  int32_t n_heads;    /* 16 upstream (ar_discrete.py:238)                                          */
  int32_t n_layers;   /* 8 upstream  (ar_discrete.py:238)                                          */
  int32_t canvas;     /* frames per utterance the denoiser sees, 448 upstream (:704)               */
  int32_t s_text;     /* phoneme keys, 50 upstream (:714)                                          */
  int32_t s_prompt;   /* prompt keys, 398 upstream (:726)                                          */
  int32_t n_classes;  /* 1025 (:255)                                                               */
  int32_t mask_id;    /* absorbing id 512 (:332)                                                   */
  int32_t timesteps;  /* 100 (:207); the loop runs t = timesteps-1 .. 1 (:750)                     */
  int32_t dtype;      /* D3PM_F32 / D3PM_F16 / D3PM_BF16                                           */
  int32_t n_q;        /* quantizer levels the D3PM generates jointly: 0 or 1 = level 0 only, as upstream (:699-709,
                         SURVEY.md section 0 #4).  n_q > 1 is this build's extension (SURVEY section 8d config 2,
                         BASELINE.json configs[1] "x 8 quantizers"; no reference counterpart): token grids are
                         [batch][canvas][n_q], a frame's input embedding is the sum of its n_q level embeddings
                         (resps_emb [n_q][n_classes][d], as MultiEmbedding sums the prompt levels, base.py:244-274), `final`
                         is [n_q * n_classes][d] and every (frame, level) is sampled like a level-0 token, level l > 0 on
                         Philox stream 16 + l.  With n_q = 1 every entry point is bit-identical to the level-0 path. */
  const d3pm_tuning *tuning;   /* schedule choices of the calls made with this shape, or NULL (defaults)   */
} d3pm_shape;

/* One DiT block's parameters (ar_discrete.py:103-124), device pointers, elements of `dtype`,
 * torch layouts: Linear weight [out][in]; MultiheadAttention in_proj [3d][d] (q|k|v rows).
 * cross_attn2.* is dead upstream (the prompt attention re-uses cross_attn, :142) and not passed. */
typedef struct d3pm_block_weights {
  const void *norm1_w, *norm1_b;          /* [d]               LayerNorm eps 1e-6 (:108)  */
  const void *attn_in_w, *attn_in_b;      /* [3d][d], [3d]     self-attention (:109)      */
  const void *attn_out_w, *attn_out_b;    /* [d][d], [d]                                  */
  const void *norm2_w, *norm2_b;          /* text-query LN (:112)                         */
  const void *norm22_w, *norm22_b;        /* prompt-query LN (:117)                       */
  const void *cross_in_w, *cross_in_b;    /* [3d][d], [3d]     cross_attn (:113)          */
  const void *cross_out_w, *cross_out_b;  /* [d][d], [d]                                  */
  const void *norm3_w, *norm3_b;          /* (:121)                                       */
  const void *fc1_w, *fc1_b;              /* [4d][d], [4d]     timm Mlp (:123)            */
  const void *fc2_w, *fc2_b;              /* [d][4d], [d]                                 */
  const void *tfc_w, *tfc_b;              /* [2d][d], [2d]     timestep_fc (:124)         */
} d3pm_block_weights;

/* A block's LayerNorms folded into the projections they feed (ar_discrete.py:131-132, 136-142, 145-159), built by
 * d3pm_fold_build from d3pm_block_weights; device pointers into the caller's `storage`.  For a projection
 * y = LN(x) W^T + b:  w = rn(W o gamma) in the model dtype,  s[n] = sum_k w[n][k] and b[n] = sum_k W[n][k] beta[k] + b[n] in fp32, so
 * that y = rstd_r (x_r . w^T - mean_r s) + b.  fc1 carries FiLM (gamma_k rn(1 + scale_t[k]), beta_k rn(1 + scale_t[k]) + shift_t[k]),
 * which depends on the timestep: its folded copy is rebuilt for t at the top of every denoiser evaluation, into the workspace
 * (one launch for all layers), and is not part of this struct. */
typedef struct d3pm_fold_block {
  const void *qkv_w;  const float *qkv_s, *qkv_b;     /* [3d][d]; [3d]                 norm1 -> attn in-projection                 */
  const void *q2_w;   const float *q2_s, *q2_b;       /* [2d][d]; [2d]                 norm2 -> q rows | norm22 -> the same q rows  */
} d3pm_fold_block;

typedef struct d3pm_weights {
  const void *resps_emb;                  /* [n_classes][d]  (:212); n_q > 1: [n_q][n_classes][d] */
  const void *time_emb;                   /* [timesteps+1][d] (:213)                      */
  const void *final_w, *final_b;          /* [n_classes][d], [n_classes] (:240); n_q > 1: [n_q * n_classes][d], [n_q * n_classes] */
  const d3pm_block_weights *blocks;       /* HOST array of n_layers entries               */
  const d3pm_fold_block *fold;            /* HOST array of n_layers entries (d3pm_fold_build), or NULL: stand-alone LayerNorms */
} d3pm_weights;

/* Block-scaled fp8 ("MX": OCP e4m3 codes + one e8m0 power-of-two scale per 32 elements along K) copies of a block's
 * projection weights for the fp8 fast path (BASELINE.json configs[4]; built by the caller, e.g. _hip.quantize_mx):
 *   codes  [N][K] one byte per element, row-major;
 *   scales [N][4][K / 128] bytes, value 2^(byte - 127): scales[n][g][s] applies to elements [128 s + 32 g, 128 s + 32 g + 32)
 *          of row n (g-major so that the matrix instruction's lane fetches four consecutive k-steps of its block as one dword;
 *          csrc/d3pm_mx.hip).
 * cross_in covers the q rows only ([d][d]).  fc2_w8 / fc2_scale may be NULL: then fc1 writes a 16-bit hidden layer and fc2
 * stays a 16-bit GEMM. */
typedef struct d3pm_fp8_block_weights {
  const void *attn_in_w8;  const void *attn_in_scale;    /* [3d][d], [3d][4][d/128]   */
  const void *cross_in_w8; const void *cross_in_scale;   /* [d][d],  [d][4][d/128]    */
  const void *fc1_w8;      const void *fc1_scale;        /* [4d][d], [4d][4][d/128]   */
  const void *fc2_w8;      const void *fc2_scale;        /* [d][4d], [d][4][4d/128] or NULL */
} d3pm_fp8_block_weights;

/* fp16 bit patterns of the absorbing-state schedule, HOST arrays.
 * betas[timesteps+1]; d,c,dbar,cbar[timesteps]:  Q_t = d_t I + c_t 1 e_M^T,  Qbar_t likewise. */
typedef struct d3pm_schedule {
  int32_t timesteps;
  const uint16_t *d, *c, *dbar, *cbar;
} d3pm_schedule;

int d3pm_abi_version(void);
const char *d3pm_last_error(void);

/* Replaces AR.cosine_beta_schedule + the 3 x [T,1025,1025] fp16 table build
 * (ar_discrete.py:257,268-277,286-304,315-334) by the 4 fp16 scalars per step they reduce to
 * (SURVEY.md §8a a14).  Pure host arithmetic; all outputs are HOST arrays of fp16 bit patterns. */
int d3pm_schedule_build(int timesteps, uint16_t *betas /*[timesteps+1]*/, uint16_t *d, uint16_t *c,
                        uint16_t *dbar, uint16_t *cbar /*[timesteps] each*/);

/* Bytes of device scratch the step/loop entry points need for `batch` utterances. */
size_t d3pm_workspace_bytes(const d3pm_shape *shape, int batch);

/* Step-invariant precomputation ----------------------------------------------------------- */

/* film[t][layer][2d] = timestep_fc_layer(time_emb[t])  (ar_discrete.py:145,752) for every t:
 * the FiLM scale/shift depends on weights and t only, so it is tabulated once per weight set. */
int d3pm_film_table(const d3pm_shape *shape, const d3pm_weights *w, void *film /*device*/,
                    void *stream);

/* LayerNorm folded into the projections: bytes of device storage for the tables of `shape` (0 when the shape does not qualify:
 * 16-bit dtype and d_model a multiple of 256), and the build; blocks_out is a HOST array of n_layers entries that receives
 * pointers into `storage` (pass it as d3pm_weights.fold).  Once per weight set; 5 d^2 elements + 10 d floats per layer. */
size_t d3pm_fold_bytes(const d3pm_shape *shape);
int d3pm_fold_build(const d3pm_shape *shape, const d3pm_weights *w, void *storage /*device*/, size_t storage_bytes,
                    d3pm_fold_block *blocks_out /*host*/, void *stream);

/* K/V projections of the step-invariant conditions with cross_attn's k/v rows
 * (the `k`/`v` halves of F.multi_head_attention_forward's in-projection for the calls at
 * ar_discrete.py:138,142).  cond_* are device [batch][S][d]; kv_* receive [n_layers][batch][S][2d]. */
int d3pm_cond_kv(const d3pm_shape *shape, const d3pm_weights *w, int batch, const void *cond_text,
                 const void *cond_prompt, void *kv_text, void *kv_prompt, void *stream);

/* Condition encoders (once per utterance) ------------------------------------------------------
 * Replaces the statements before the loop of AR.generate_audio (ar_discrete.py:736-746): text_emb / proms_emb
 * (base.py:244-274) gathers, the sinusoidal position add (:84-92 incl. the position-0 quirk for text), two
 * post-norm nn.TransformerEncoderLayer (nhead 16, ReLU FFN 2048, LayerNorm eps 1e-5, :216-230) and the
 * timm Mlp(SiLU) of each of `encodertext` / `encoder2`.  Dropout is identity (inference). */
typedef struct d3pm_encoder_layer_weights {
  const void *in_w, *in_b;      /* self_attn.in_proj [3d][d], [3d] */
  const void *out_w, *out_b;    /* self_attn.out_proj [d][d], [d]  */
  const void *lin1_w, *lin1_b;  /* linear1 [d_ff][d], [d_ff]       */
  const void *lin2_w, *lin2_b;  /* linear2 [d][d_ff], [d]          */
  const void *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} d3pm_encoder_layer_weights;

typedef struct d3pm_encoder_weights {
  const d3pm_encoder_layer_weights *layers;   /* HOST array of n_layers entries */
  int32_t n_layers, n_heads, d_ff, mlp_hidden;
  const void *fc1_w, *fc1_b;                  /* [mlp_hidden][d], [mlp_hidden]  */
  const void *fc2_w, *fc2_b;                  /* [d][mlp_hidden], [d]           */
} d3pm_encoder_weights;

typedef struct d3pm_cond_weights {
  const void *text_emb;    /* [n_classes][d]            (ar_discrete.py:210) */
  const void *proms_emb;   /* [n_levels][n_classes][d]  (:211)               */
  const void *pe_text0;    /* [d]           sinusoid of position 0, model dtype */
  const void *pe_prompt;   /* [s_prompt][d] sinusoid table, model dtype         */
  int32_t n_levels;
  d3pm_encoder_weights text_encoder;     /* encodertext (:216-222) */
  d3pm_encoder_weights prompt_encoder;   /* encoder2    (:224-230) */
} d3pm_cond_weights;

size_t d3pm_cond_workspace_bytes(const d3pm_shape *shape, const d3pm_cond_weights *cw, int batch);

/* text device int32 [batch][s_text] (zero padded), prompt device int32 [batch][s_prompt][n_levels];
 * cond_text [batch][s_text][d], cond_prompt [batch][s_prompt][d] of `dtype` (feed d3pm_cond_kv). */
int d3pm_encode_conditions(const d3pm_shape *shape, const d3pm_cond_weights *cw, int batch, const int32_t *text,
                           const int32_t *prompt, void *cond_text, void *cond_prompt, void *workspace,
                           size_t workspace_bytes, void *stream);

/* One denoiser evaluation --------------------------------------------------------------------
 * Replaces the loop body at ar_discrete.py:752-776: resps_emb gather, n_layers x DiTBlock.forward
 * (:126-161, incl. torch's multi_head_attention_forward need_weights branch and timm Mlp), final
 * Linear on the masked hidden state.  x_t device int32 [batch][canvas]; frame_mask device uint8
 * [canvas]; logits_out device [batch*canvas][n_classes] of `dtype`; hidden_out optional
 * [batch*canvas][d] (state after the last block, before the final mask) or NULL;
 * only_layers >= 0 stops after that many blocks (block-level parity tests). */
int d3pm_denoise_step(const d3pm_shape *shape, const d3pm_weights *w, int batch, const int32_t *x_t,
                      const uint8_t *frame_mask, int t, const void *film, const void *kv_text,
                      const void *kv_prompt, void *workspace, size_t workspace_bytes,
                      void *logits_out, void *hidden_out, int only_layers, uint32_t flags,
                      void *stream);

/* Replaces AR.p_sample / q_posterior_logits / _at / _at_onehot (ar_discrete.py:337-420):
 * fp16 softmax of the x0-logits, closed-form fact1/fact2, log+log in fp16, fp32 Gumbel add from
 * the Philox stream (seed, row = (utt0+b)*canvas+frame, t), first-index argmax.
 * logits device [batch*canvas][n_classes] of logits_dtype; posterior_out optional device fp16
 * bit patterns [batch*canvas][n_classes] or NULL. */
int d3pm_posterior_sample(const d3pm_shape *shape, int batch, const void *logits, int logits_dtype,
                          const int32_t *x_t, int32_t *x_next, int t, const d3pm_schedule *sched,
                          uint64_t seed, uint32_t utt0, uint32_t flags, uint16_t *posterior_out,
                          void *stream);

/* Replaces the whole reverse process of AR.generate_audio after the condition encoders
 * (ar_discrete.py:748-780): for t = t_start .. t_stop+1: denoise step + posterior sample.
 * x device int32 [batch][canvas], in: x_T, out: x_{t_stop}.  trace optional device int32
 * [t_start-t_stop][batch][canvas] receiving x after every step, or NULL. */
int d3pm_sample_loop(const d3pm_shape *shape, const d3pm_weights *w, int batch, int32_t *x,
                     const uint8_t *frame_mask, int t_start, int t_stop, const void *film,
                     const void *kv_text, const void *kv_prompt, const d3pm_schedule *sched,
                     uint64_t seed, uint32_t utt0, uint32_t flags, void *workspace,
                     size_t workspace_bytes, int32_t *trace, void *stream);

/* The fp8 fast path (BASELINE.json configs[4]): same contracts as d3pm_denoise_step / d3pm_sample_loop, but the K = d_model
 * projections fed by a LayerNorm -- norm1 -> QKV, norm2|norm22 -> the merged cross-attention query projection, norm3(+FiLM) ->
 * fc1 -- and (when fc2_w8 is given) fc2 run on the block-scaled matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4 with
 * e4m3 operands: LayerNorm rows are quantised on the fly in blocks of 32 (power-of-two scales), fc1's GELU epilogue writes
 * its output directly in that format for fc2, weights come from `fp8_blocks` (a HOST array of n_layers entries); fp32
 * accumulation, 16-bit residual stream.  Requires d_model = 512, a 16-bit model dtype and batch * canvas a multiple of 192;
 * D3PM_E_SHAPE otherwise (and D3PM_E_ARG under D3PM_FLAG_FORCE_GENERIC): a number labelled fp8 is never a 16-bit run.  The
 * reference has no such mode: tests report agreement against the 16-bit path. */
int d3pm_denoise_step_fp8(const d3pm_shape *shape, const d3pm_weights *weights,
                          const d3pm_fp8_block_weights *fp8_blocks, int batch, const int32_t *x_t,
                          const uint8_t *frame_mask, int t, const void *film, const void *kv_text,
                          const void *kv_prompt, void *workspace, size_t workspace_bytes, void *logits_out,
                          void *hidden_out, int only_layers, uint32_t flags, void *stream);
int d3pm_sample_loop_fp8(const d3pm_shape *shape, const d3pm_weights *weights,
                         const d3pm_fp8_block_weights *fp8_blocks, int batch, int32_t *x,
                         const uint8_t *frame_mask, int t_start, int t_stop, const void *film, const void *kv_text,
                         const void *kv_prompt, const d3pm_schedule *sched, uint64_t seed, uint32_t utt0,
                         uint32_t flags, void *workspace, size_t workspace_bytes, int32_t *trace, void *stream);

/* Per-utterance canvases ---------------------------------------------------------------------------
 * The entries above share ONE frame mask [canvas] between the utterances of a batch: every utterance has the same number of live
 * frames.  The *_canvas entries take one mask per utterance and, for the sampler, a map of the frames the caller already knows:
 *   frame_mask  device uint8 [batch][canvas]: utterance b's live frames (upstream builds it once from x_T != 0, :705-709, and keeps
 *               it for the whole loop).  Utterance b with L_b live frames is exactly the one-utterance run with that mask: padded
 *               rows are still keys of the self-attention and are still sampled from final.bias, no work is skipped for them.
 *   known       device uint8 [batch][canvas] or NULL: known[b][i] != 0 marks a frame whose id the caller gives.  `x` carries x_T
 *               with the given ids already in place (the mask id on every other live frame); after every reverse step
 *               x_{t-1}[b][i] = x_T[b][i] on the marked frames (replacement conditioning -- for an absorbing process the same as
 *               never resampling the row), so the denoiser sees them as revealed context from the first iteration on.  A marked
 *               row draws nothing; the Philox stream of every other row is keyed by its own (global row, t) and does not move.
 *               With n_q > 1 the map is per frame: all levels of a marked frame are kept.  Ids are taken verbatim from 0 .. 1023;
 *               512 is upstream's mask id (1025 // 2) and doubles as a codec id there, so a known 512 is legal and stays 512.
 *               Nothing is checked on the device: marking only live frames is the caller's contract (the Python layer raises).
 * With every row of frame_mask equal and known NULL or all zero, each entry is bit-identical to the one it generalises; utterance b
 * of a batch never depends on the lengths or maps of the others, nor on how the batch is split (utt0, regime_batch). */
typedef struct d3pm_canvas {
  const uint8_t *frame_mask;   /* device [batch][canvas]         */
  const uint8_t *known;        /* device [batch][canvas] or NULL */
} d3pm_canvas;

/* d3pm_denoise_step with a per-utterance frame mask (canvas->known is not read: the denoiser only reads ids). */
int d3pm_denoise_step_canvas(const d3pm_shape *shape, const d3pm_weights *w, int batch, const int32_t *x_t,
                             const d3pm_canvas *canvas, int t, const void *film, const void *kv_text,
                             const void *kv_prompt, void *workspace, size_t workspace_bytes, void *logits_out,
                             void *hidden_out, int only_layers, uint32_t flags, void *stream);

/* d3pm_posterior_sample with a known-frame map (device uint8 [batch][canvas] or NULL): x_next = x_t on the marked frames, the
 * posterior draw everywhere else (posterior_out rows of marked frames are left unwritten).  One step of what
 * d3pm_sample_loop_canvas does between two denoiser evaluations. */
int d3pm_posterior_sample_known(const d3pm_shape *shape, int batch, const void *logits, int logits_dtype,
                                const int32_t *x_t, int32_t *x_next, const uint8_t *known, int t,
                                const d3pm_schedule *sched, uint64_t seed, uint32_t utt0, uint32_t flags,
                                uint16_t *posterior_out, void *stream);

/* d3pm_sample_loop / d3pm_sample_loop_fp8 over per-utterance canvases; every other argument as there. */
int d3pm_sample_loop_canvas(const d3pm_shape *shape, const d3pm_weights *w, int batch, int32_t *x,
                            const d3pm_canvas *canvas, int t_start, int t_stop, const void *film,
                            const void *kv_text, const void *kv_prompt, const d3pm_schedule *sched,
                            uint64_t seed, uint32_t utt0, uint32_t flags, void *workspace,
                            size_t workspace_bytes, int32_t *trace, void *stream);
int d3pm_sample_loop_fp8_canvas(const d3pm_shape *shape, const d3pm_weights *weights,
                                const d3pm_fp8_block_weights *fp8_blocks, int batch, int32_t *x,
                                const d3pm_canvas *canvas, int t_start, int t_stop, const void *film,
                                const void *kv_text, const void *kv_prompt, const d3pm_schedule *sched,
                                uint64_t seed, uint32_t utt0, uint32_t flags, void *workspace,
                                size_t workspace_bytes, int32_t *trace, void *stream);

/* Temperature and top-k on the x0-logits ----------------------------------------------------------------
 * How sharply the reverse step draws (the reference has neither; the NAR stage's own temperature is d3pm_nar_level's).  Two numbers
 * per call, applied to every row's logits l_j right after the sampler has loaded them, exactly (no tolerance anywhere):
 *     z_j   = rn16(float(l_j))                           what the sampler reads today
 *     z'_j  = rn16(z_j / temperature)                    fp32 division, one rounding (temperature 1: z' = z bit for bit)
 *     theta = the top_k-th largest of z'_0 .. z'_{K-1}, counted with multiplicity      (top_k 0: -inf)
 *     z''_j = z'_j >= theta ? z'_j : -inf                ties at theta are all kept, so >= top_k classes survive
 *     x_{t-1} = the unfiltered routine on z'' (softmax, fact1 / fact2, logs, Gumbel add, first-index argmax: unchanged)
 * i.e. a filtered call equals the unfiltered entry fed with host-filtered logits, id for id.  All n_classes take part alike (no
 * special case for the mask id); with n_q > 1 each level's n_classes logits are filtered on their own.  The noise does not move:
 * every class keeps the uniform it had, a class that was cut carries p = 0 into the same arithmetic.  D3PM_FLAG_GREEDY, t = 0,
 * known frames, per-utterance masks, utt0 / regime_batch compose with it as they compose with each other.
 *   temperature  finite and > 0; 1 = off        top_k  0 = off, else 1 .. n_classes        (anything else: D3PM_E_ARG, nothing launched)
 * A NULL d3pm_sampling, or {1.0f, 0}, is bit-identical to the entry that is generalised and launches the very same kernels; any
 * other pair ({1.0f, n_classes} included) takes the kernels' filter arm. */
typedef struct d3pm_sampling {
  float temperature;
  int32_t top_k;
} d3pm_sampling;

/* d3pm_posterior_sample_known (known may be NULL: d3pm_posterior_sample) with sampling options. */
int d3pm_posterior_sample_sampling(const d3pm_shape *shape, int batch, const void *logits, int logits_dtype,
                                   const int32_t *x_t, int32_t *x_next, const uint8_t *known, int t,
                                   const d3pm_schedule *sched, uint64_t seed, uint32_t utt0, uint32_t flags,
                                   uint16_t *posterior_out, const d3pm_sampling *sampling, void *stream);

/* The four loops above in one entry, with sampling options: exactly one of `frame_mask` (device uint8 [canvas], shared by the
 * batch: d3pm_sample_loop) and `canvas` (d3pm_sample_loop_canvas) is given, the other is NULL; `fp8_blocks` NULL = the 16-bit
 * loop, else the fp8 fast path (d3pm_sample_loop_fp8 / _fp8_canvas, same shape requirements).  Every other argument as there. */
int d3pm_sample_loop_sampling(const d3pm_shape *shape, const d3pm_weights *weights,
                              const d3pm_fp8_block_weights *fp8_blocks, int batch, int32_t *x, const uint8_t *frame_mask,
                              const d3pm_canvas *canvas, int t_start, int t_stop, const void *film, const void *kv_text,
                              const void *kv_prompt, const d3pm_schedule *sched, uint64_t seed, uint32_t utt0,
                              uint32_t flags, void *workspace, size_t workspace_bytes, int32_t *trace,
                              const d3pm_sampling *sampling, void *stream);

/* Nucleus (top-p) cut on the x0-logits ------------------------------------------------------------------
 * One more number per call, `top_p`: "draw from the smallest set of classes that carries this share of the mass", per row and per
 * step (the reference has no such option).  It acts on a row's z'' -- the logits after temperature and top-k as defined above --
 * and, with n_q > 1, on each level's n_classes logits on their own:
 *     m       = max_j z''_j
 *     e_j     = expf(z''_j - m)                  the value the sampler computes for its softmax anyway (-inf -> 0)
 *     q_j     = (uint32) (e_j * 1048576.0f)      truncated; q of the maximum is 2^20; the sum over <= 1280 classes is < 2^31
 *     Q       = sum_j q_j                        an integer: the same whatever order lanes and waves add in
 *     mass(c) = sum_{key(z''_j) >= c} q_j        key = the 16-bit order key of the fp16 value (unsigned order = order of the values)
 *     theta   = value of the LARGEST key c with (double) mass(c) >= (double) top_p * (double) Q
 *     z'''_j  = z''_j >= theta ? z''_j : -inf    ties at theta are all kept; compared on VALUES, so -0 / +0 stand or fall together
 *     x_{t-1} = the unfiltered routine on z'''
 * i.e. a call equals the unfiltered entry fed with the host-filtered z'' cut at theta, id for id.  What follows from it:
 *   - mass is monotone in c, so the key of theta is built bit by bit from the top (16 rounds), exactly like the top-k one;
 *   - the largest such key is the key of a class of the row with q > 0: theta is one of the row's values;
 *   - the maximum is always kept; m and the e_j of the kept classes are unchanged, so the ids do not depend on whether the routine
 *     computes them again or reuses them;
 *   - Q <= n_classes * 2^20 and n_classes <= 1280: any top_p <= 1/1280 keeps exactly the classes tied at the maximum, which gives
 *     the ids of top_k = 1;
 *   - for every set S of classes |sum_S q / Q - sum_S softmax(z'')| <= n_classes / 2^20 + 2^-20 (<= 1.0e-3 at 1025 classes:
 *     truncation of less than one unit per class, Q >= 2^20, expf to within a few ulp).  This is the only slack in the contract: it
 *     bounds how far the kept mass may sit from top_p.  It bounds no id;
 *   - noise, D3PM_FLAG_GREEDY, t = 0, known frames, per-utterance masks, utt0 / regime_batch, the fp8 loop compose with top_p exactly
 *     as they do with top_k: a class that is cut carries p = 0 into the same arithmetic, and its uniform is still drawn;
 *   - a row whose logits are all -inf is outside the contract, as it is for the entries above.
 *   temperature, top_k  as in d3pm_sampling        top_p  finite, 0 < top_p <= 1; 1 = off      (anything else: D3PM_E_ARG, nothing launched)
 * A NULL d3pm_nucleus, or {1.0f, 0, 1.0f}, is bit-identical to the entry that is generalised and launches the very same kernels;
 * {temperature, top_k, 1.0f} is d3pm_sampling{temperature, top_k} and launches what that launches; top_p < 1 takes the kernels'
 * nucleus arm (kernels of their own: a call without top_p runs none of its code). */
typedef struct d3pm_nucleus {
  float temperature;
  int32_t top_k;
  float top_p;
} d3pm_nucleus;

/* d3pm_posterior_sample_sampling with the triple.  theta_out: optional device float [batch][canvas] ([batch][canvas][n_q] with
 * n_q > 1), NULL = not wanted: the wave that filtered a row writes the row's theta there (top_p = 1: -inf, nothing is cut); a known
 * row writes NaN.  A non-NULL theta_out takes the nucleus arm whatever top_p is; the ids are those of the same call without it. */
int d3pm_posterior_sample_nucleus(const d3pm_shape *shape, int batch, const void *logits, int logits_dtype,
                                  const int32_t *x_t, int32_t *x_next, const uint8_t *known, int t,
                                  const d3pm_schedule *sched, uint64_t seed, uint32_t utt0, uint32_t flags,
                                  uint16_t *posterior_out, const d3pm_nucleus *nucleus, float *theta_out, void *stream);

/* d3pm_sample_loop_sampling with the triple; every other argument as there. */
int d3pm_sample_loop_nucleus(const d3pm_shape *shape, const d3pm_weights *weights,
                             const d3pm_fp8_block_weights *fp8_blocks, int batch, int32_t *x, const uint8_t *frame_mask,
                             const d3pm_canvas *canvas, int t_start, int t_stop, const void *film, const void *kv_text,
                             const void *kv_prompt, const d3pm_schedule *sched, uint64_t seed, uint32_t utt0,
                             uint32_t flags, void *workspace, size_t workspace_bytes, int32_t *trace,
                             const d3pm_nucleus *nucleus, void *stream);

/* Confidence-ordered reveal in N denoiser evaluations ----------------------------------------------------
 * A second reverse schedule on the same canvas (MaskGIT / SoundStorm decoding; the reference has none): instead of revealing every
 * masked row at random with the schedule's probability over timesteps - 1 evaluations, each of N steps reveals the rows the model is
 * most sure of, under a quota that follows cbar -- the share of masked frames the denoiser was trained on at that timestep.  No
 * statement about audio quality is made; what follows is an exact definition.  n_q = 1 only; a batch is B independent one-utterance
 * runs.  T = sched->timesteps, 1 <= N <= T - 1.
 *   timesteps  t_i = (T-1) - floor(i (T-1) / N), i = 0 .. N-1, and t_N = 0: strictly decreasing, t_0 = T-1, t_{N-1} >= 1; N = T-1 gives
 *              T-1, T-2, .. 1 (d3pm_reveal_plan).  Evaluation i runs the denoiser at t_i.
 *   rows       a row of utterance b is FREE when it is live (frame_mask) and not known; F_b = number of free rows; a free row is
 *              MASKED when x == mask_id.  The canvas starts as for the D3PM loop (known ids in place, the mask id on the other
 *              live frames, 0 on the padding).
 *   quota      after step i utterance b keeps  keep = min(masked_now, floor((double) F_b * (double) float(cbar[t_{i+1}])))  rows
 *              masked (after the last step: 0) and reveals masked_now - keep.  An fp16 significand times a count < 2^20 is exact in
 *              fp64, so host and device agree on the count with no tolerance.  The kernel counts F_b and masked_now itself from
 *              frame_mask, known and x_t: no plan is uploaded, shards and stream chunks need nothing extra.
 *   candidate  of a masked row at step i:  z_j = rn16(float(l_j)) as the sampler reads the logits; z_{mask_id} = -inf (the mask is not
 *              a token to reveal); then temperature, top_k, top_p exactly as d3pm_sampling / d3pm_nucleus define them -> z''' (the
 *              neutral triple leaves only the -inf);  m = max z''',  e_j = expf(z'''_j - m),  S = sum_j e_j in fp32;
 *              cand = first-index argmax of z'''_j + gumbel(u_j) in fp32, u_j the uniform the posterior draw of that row would take:
 *              Philox key (seed; class group, global row, t_i, stream 0).  D3PM_FLAG_GREEDY: cand = first-index argmax of z'''_j, no
 *              draw.  A row whose z''' are all -inf is outside the contract.
 *   score      conf = z'''_cand - m - logf(S) in fp32;  score = conf + lambda_i * gumbel(v),  lambda_i = choice_temperature *
 *              float(cbar[t_{i+1}]) (fp32), lambda_{N-1} = 0;  v = word 0 of Philox key (seed; 0, global row, t_i, stream 4).
 *              choice_temperature = 0 and D3PM_FLAG_GREEDY draw no v and give score = conf bit for bit.  The score sits within
 *              1.0e-4 of the definition in exact arithmetic (1033 * 2^-24 on S, three fp32 roundings at magnitude <= 32); the bound
 *              limits how far a score may sit from the definition.  It bounds no id:
 *   selection  the order key is the monotone uint32 image of the score's fp32 bits; the rows revealed are the masked_now - keep
 *              masked rows that come first in the order (key descending, frame index ascending) -- given the scores the device
 *              reports, the revealed set is exact.  A revealed row takes cand (never mask_id) and is never drawn again; every other
 *              row keeps x_t.  Known rows and padded rows are never given a new id: padded rows stay 0 -- they are NOT "sampled from
 *              final.bias" as on the D3PM path.  After step N-1 no free row holds the mask id.
 * Refused with nothing launched: n_steps outside 1 .. T-1, choice_temperature negative or not finite (D3PM_E_ARG); n_q > 1,
 * canvas > 1024 (D3PM_E_SHAPE).  There is no fp8 entry. */
typedef struct d3pm_reveal {
  int32_t n_steps;
  float choice_temperature;     /* >= 0, finite; 0 = rows are revealed in the order of their confidence alone */
} d3pm_reveal;

/* t_out[i] = t_i for i = 0 .. n_steps - 1 (HOST array).  Host arithmetic only. */
int d3pm_reveal_plan(const d3pm_schedule *sched, int n_steps, int32_t *t_out /* host [n_steps] */);

/* One step between two denoiser evaluations: the evaluation ran at t (= t_i) and the next one runs at t_next (= t_{i+1}; 0 marks the
 * last step: keep = 0, lambda = 0), sched->timesteps > t > t_next >= 0.  Exactly one of frame_mask (device uint8 [canvas], shared by
 * the batch) and canvas (per utterance, with the optional known map) is given.  logits device [batch*canvas][n_classes] of
 * logits_dtype; x_next may be x_t (in place: only revealed rows are stored) or another grid (every row is stored).  cand_out (int32)
 * and score_out (fp32), device [batch][canvas], receive cand and score of every row that was masked at x_t, written by the wave that
 * scored the row; rows that were not masked are left unwritten.  They are also what the step's second launch reads, so both are
 * required.  nucleus NULL = the neutral triple. */
int d3pm_reveal_step(const d3pm_shape *shape, int batch, const void *logits, int logits_dtype, const int32_t *x_t,
                     int32_t *x_next, const uint8_t *frame_mask, const d3pm_canvas *canvas, int t, int t_next,
                     const d3pm_schedule *sched, uint64_t seed, uint32_t utt0, uint32_t flags, const d3pm_nucleus *nucleus,
                     float choice_temperature, int32_t *cand_out, float *score_out, void *stream);

/* The whole schedule: for i = 0 .. n_steps-1: denoiser evaluation at t_i + d3pm_reveal_step(t_i, t_{i+1}).  x device int32
 * [batch][canvas], in: the initial canvas, out: the result.  trace optional device int32 [n_steps][batch][canvas] receiving x after
 * every step, or NULL.  Workspace as for d3pm_sample_loop.  Two launches per step behind the final projection; with the folded
 * LayerNorms the second one also gathers the embedding rows of the next evaluation with their moments and rebuilds fc1 for t_{i+1}
 * (same ids as the step entry, step by step). */
int d3pm_reveal_loop(const d3pm_shape *shape, const d3pm_weights *weights, int batch, int32_t *x, const uint8_t *frame_mask,
                     const d3pm_canvas *canvas, const void *film, const void *kv_text, const void *kv_prompt,
                     const d3pm_schedule *sched, uint64_t seed, uint32_t utt0, uint32_t flags, void *workspace,
                     size_t workspace_bytes, int32_t *trace, const d3pm_nucleus *nucleus, const d3pm_reveal *reveal,
                     void *stream);

/* ---- key-padding masks (additions; ABI version unchanged) -------------------------------------------------------------------------
 * Upstream lets every utterance attend to its own padding: the canvas - L_b padded frames are keys of every self-attention, the
 * zero-padded phonemes and prompt frames are keys of both cross-attentions and of the two condition encoders.  With d3pm_keys
 * utterance b has three key counts, device int32 [batch] each:
 *   frames[b]   its live frames L_b            -> the keys of every DiT self-attention
 *   text[b]     its phonemes, <= s_text        -> the keys of the text cross-attention and of the text encoder's self-attention
 *   prompt[b]   its prompt frames, <= s_prompt -> the keys of the prompt cross-attention and of the prompt encoder's self-attention
 * A masked key carries probability exactly 0; its K / V rows need not be read and never influence a result (large finite garbage
 * there changes nothing; NaN is outside the contract).  Padded rows stay queries: no row of work is skipped and their outputs are
 * masked or trimmed as without d3pm_keys; the frame-mask multiply, the sampling of padded rows, the Philox keys, known frames,
 * sampling options and the reveal quota are unchanged.  The live rows of utterance b therefore compute what the model computes at
 * canvas = L_b, s_text = text[b], s_prompt = prompt[b] -- within accumulation order, not bit for bit: the MFMA kernels tile the keys
 * by the padded counts' grid, and padded rows, being queries, share a wave with live rows, where the flash kernels decide per wave
 * whether the running maximum moves.  Bit for bit it holds on the generic family (D3PM_FLAG_FORCE_GENERIC, fp32).
 * Contract (the values live on the device and are read by the kernels only, so nothing here can refuse them):
 *   1 <= frames[b] <= canvas, 1 <= text[b] <= s_text, 1 <= prompt[b] <= s_prompt, and frames[b] = the number of leading ones of
 *   frame_mask[b] (the live frames are a prefix of the canvas).
 * A shard or a stream chunk that starts at utterance u passes the three pointers offset by u.  Any of the three may be NULL (that
 * attention is not masked); a NULL d3pm_keys is the entry that is generalised and launches the very same kernels.  A masked
 * evaluation takes the schedules of the unmasked one (same regime rule): the mask does not switch the instruction shape.  There are
 * no fp8 entries: d3pm_sample_loop_keys refuses keys together with fp8_blocks (D3PM_E_ARG).  The training step takes no mask. */
typedef struct d3pm_keys {
  const int32_t *frames, *text, *prompt;      /* device int32 [batch] each */
} d3pm_keys;

/* d3pm_encode_conditions with keys->text / keys->prompt on the two encoders' self-attentions (keys->frames is not read).  The ids
 * behind a length are not read: those rows are embedded as padding (text: id 0; prompt: every level absent), so nothing that
 * `text` / `prompt` hold there reaches a result, in any bit.  (The rows stay queries of their encoder, and a query row can move the
 * last bit of a live row it shares a wave with; that is why the padding is made here and not left to the caller.) */
int d3pm_encode_conditions_keys(const d3pm_shape *shape, const d3pm_cond_weights *cw, int batch, const int32_t *text,
                                const int32_t *prompt, void *cond_text, void *cond_prompt, void *workspace,
                                size_t workspace_bytes, const d3pm_keys *keys, void *stream);
/* d3pm_denoise_step_canvas + keys */
int d3pm_denoise_step_keys(const d3pm_shape *shape, const d3pm_weights *w, int batch, const int32_t *x_t,
                           const d3pm_canvas *canvas, int t, const void *film, const void *kv_text, const void *kv_prompt,
                           void *workspace, size_t workspace_bytes, void *logits_out, void *hidden_out, int only_layers,
                           uint32_t flags, const d3pm_keys *keys, void *stream);
/* d3pm_sample_loop_nucleus + keys */
int d3pm_sample_loop_keys(const d3pm_shape *shape, const d3pm_weights *weights, const d3pm_fp8_block_weights *fp8_blocks, int batch,
                          int32_t *x, const uint8_t *frame_mask, const d3pm_canvas *canvas, int t_start, int t_stop,
                          const void *film, const void *kv_text, const void *kv_prompt, const d3pm_schedule *sched, uint64_t seed,
                          uint32_t utt0, uint32_t flags, void *workspace, size_t workspace_bytes, int32_t *trace,
                          const d3pm_nucleus *nucleus, const d3pm_keys *keys, void *stream);
/* d3pm_reveal_loop + keys */
int d3pm_reveal_loop_keys(const d3pm_shape *shape, const d3pm_weights *weights, int batch, int32_t *x, const uint8_t *frame_mask,
                          const d3pm_canvas *canvas, const void *film, const void *kv_text, const void *kv_prompt,
                          const d3pm_schedule *sched, uint64_t seed, uint32_t utt0, uint32_t flags, void *workspace,
                          size_t workspace_bytes, int32_t *trace, const d3pm_nucleus *nucleus, const d3pm_reveal *reveal,
                          const d3pm_keys *keys, void *stream);

/* ---- classifier-free guidance (additions; ABI version unchanged) -------------------------------------------------------------------
 * Each reverse step evaluates the denoiser with the utterance's conditions and with the NULL condition, and draws from the
 * extrapolated logits (1 + w) cond - w uncond (Ho & Salimans 2022; the reference has no such option).  Exact definition:
 *   null condition  the utterance with no phonemes and no prompt frames, padded the way every utterance is padded: what the condition
 *                   encoders give for an empty text (int64 [0]) and an empty prompt ([0][n_levels]), i.e. d3pm_encode_conditions on
 *                   the zero padding alone.  No new weights, no new embedding rule.  The library does not care what the second
 *                   half holds: a caller may encode any "negative" condition.
 *   guided logits   for weight w (finite, >= 0), a row's conditioned logits c_j and null logits u_j in the logits dtype:
 *                       z_j = rn16( fmaf(w, float(c_j) - float(u_j), float(c_j)) )
 *                   -- the subtraction in fp32, an explicit fma (no contraction left to the compiler), ONE rounding to fp16, at the
 *                   point where the row routines round a plain logit today.  Everything downstream is the existing routine on z:
 *                   temperature / top_k / top_p (d3pm_nucleus), softmax, posterior, Gumbel-max, the exact early-out of revealed rows,
 *                   D3PM_FLAG_GREEDY, t = 0.  All n_classes are combined alike, the mask class included.  Where c == u (w = anything)
 *                   z = rn16(c) exactly, and w = 0 gives the unguided ids from the conditioned half.
 *   evaluation      a guided step is ONE denoiser evaluation of 2 * batch utterances, not two of batch: utterance batch + b is the
 *                   null twin of b -- the same x_t, the same frame mask, its own K/V (and key counts).  What the caller sees -- x,
 *                   trace, the known map, frame_mask -- stays [batch][canvas]; the noise of row r is keyed by utt0 * canvas + r as
 *                   without guidance.  The attention regime rule sees twice the logical batch, 2 * max(regime_batch, batch), so a
 *                   shard or a stream chunk of a guided batch reproduces the unsplit guided batch bit for bit (regime_batch keeps
 *                   counting logical utterances).
 * Refused with D3PM_E_ARG and a message, nothing launched: a NULL d3pm_guidance, a negative or non-finite weight, n_q > 1, fp8 block
 * weights, D3PM_FLAG_SEED_IN_HBM (graph replay).  The reveal loop takes no guidance.  A call without d3pm_guidance runs none of this
 * code: the guided launches are kernels of their own (they always carry the nucleus arm, which with the neutral triple changes no
 * value).  No statement about audio quality is made: guidance is meaningful for weights trained with the conditions dropped some of
 * the time (vall_e/vall_e/train.py: cond_drop). */
typedef struct d3pm_guidance {
  float weight;     /* w: finite, >= 0 */
} d3pm_guidance;

/* One guided posterior draw between two evaluations.  logits device [2 * batch * canvas][n_classes] of logits_dtype (any of the
 * three): rows [0, batch * canvas) under the conditions, rows batch * canvas + r the null twin of row r.  x_t / x_next device int32
 * [batch][canvas].  canvas NULL or a d3pm_canvas whose `known` map ([batch][canvas] or NULL) marks frames that keep x_t (frame_mask
 * is not read); nucleus NULL = the neutral triple. */
int d3pm_posterior_sample_guided(const d3pm_shape *shape, int batch, const void *logits, int logits_dtype,
                                 const int32_t *x_t, int32_t *x_next, const d3pm_canvas *canvas, int t,
                                 const d3pm_schedule *sched, uint64_t seed, uint32_t utt0, uint32_t flags,
                                 const d3pm_nucleus *nucleus, const d3pm_guidance *guidance, void *stream);

/* d3pm_sample_loop_keys under guidance.  kv_text / kv_prompt hold 2 * batch utterances per layer ([L][2 batch][S][2d]: the null
 * twins behind the conditioned ones), keys (optional) 2 * batch entries per array, the workspace is
 * d3pm_workspace_bytes(shape, 2 * batch); x, canvas / frame_mask and trace are those of `batch` utterances.  fp8_blocks must be
 * NULL.  With the folded LayerNorms the sampler launch of iteration t also writes the embedding rows and moments of BOTH halves for
 * iteration t - 1 and rebuilds fc1; the ids are those of d3pm_denoise_step at 2 * batch chained with d3pm_posterior_sample_guided. */
int d3pm_sample_loop_guided(const d3pm_shape *shape, const d3pm_weights *weights, const d3pm_fp8_block_weights *fp8_blocks,
                            int batch, int32_t *x, const uint8_t *frame_mask, const d3pm_canvas *canvas, int t_start,
                            int t_stop, const void *film, const void *kv_text, const void *kv_prompt,
                            const d3pm_schedule *sched, uint64_t seed, uint32_t utt0, uint32_t flags, void *workspace,
                            size_t workspace_bytes, int32_t *trace, const d3pm_nucleus *nucleus, const d3pm_keys *keys,
                            const d3pm_guidance *guidance, void *stream);

/* ---- per-frame log-probability of the revealed id (additions; ABI version unchanged) -----------------------------------------------
 * How sure the model was of every frame it revealed, from either loop: what ranks seeds of one utterance, finds the span to
 * regenerate (known = ids, known_mask = logprob >= threshold) or compares two guidance weights.  n_q = 1 only.  Two device grids
 * [batch][canvas] travel in d3pm_frame_scores:
 *   step[r]     -1   row r was not a free masked row when the loop was entered: padding (frame mask 0), known, or already an id;
 *                0   the row is free and still masked (at loop exit only with t_stop > 0);
 *                t   (>= 1) the row left the mask in the iteration that evaluated the denoiser at timestep t (the reveal loop: the
 *                    t_i of the step that revealed it).
 *   logprob[r]  defined for a row with step[r] = t >= 1, 0.0f otherwise.  With j the id the row took in that iteration and l the
 *               logits of that evaluation:
 *                   z_k = rn16(float(l_k))        under guidance z_k = rn16(fmaf(w, float(c_k) - float(u_k), float(c_k)))
 *                   z_mask_id = -inf,  m = max_k z_k,  S = sum_k expf(z_k - m) in fp32,  logprob = z_j - m - logf(S) in fp32
 *               -- the model's own log-probability of j among the codec ids.  Temperature, top_k and top_p are deliberately NOT
 *               applied: the number then compares across sampling options, is always finite, and on the D3PM path a class the
 *               filter cut can still be drawn through the posterior's eps term.
 * The arithmetic order is that of the reveal step's confidence (K = 1025: 4 x 4 values per lane + the tail; otherwise the general
 * layout: per-lane partial sums in ascending class, the tail last, then the wave reductions), so under the neutral triple the value
 * is the conf of d3pm_reveal bit for bit.  Like that score it sits within 1.0e-4 of the definition in exact arithmetic (the same three
 * roundings and a sum of <= 1280 terms).
 * On the D3PM path a revealed row is still redrawn every iteration and may, with probability of order eps, change later: logprob
 * belongs to the id the row took at `step`, not necessarily to the id the loop returns.
 * State, not history: a step call touches only rows with step 0 whose x_next is no longer the mask id; every other entry of both
 * grids is left bit for bit as it was.
 * Refused with nothing launched: NULL scores or either grid NULL (D3PM_E_ARG), n_q > 1 (D3PM_E_SHAPE), D3PM_FLAG_SEED_IN_HBM
 * (D3PM_E_ARG), row_of together with guidance or with fp32 logits (D3PM_E_ARG). */
typedef struct d3pm_frame_scores {
  float *logprob;      /* device fp32 [batch][canvas] */
  int32_t *step;       /* device int32 [batch][canvas] */
} d3pm_frame_scores;

/* step = (live && !known && x == mask_id) ? 0 : -1 and logprob = 0 for the canvas x (device int32 [batch][canvas]) a loop is about
 * to start from.  Exactly one of frame_mask (device uint8 [canvas], shared by the batch) and canvas (per utterance, with the optional
 * known map) is given, as for the loops. */
int d3pm_frame_scores_init(const d3pm_shape *shape, int batch, const int32_t *x, const uint8_t *frame_mask,
                           const d3pm_canvas *canvas, const d3pm_frame_scores *scores, void *stream);

/* The launch behind one sampler launch: logits are those of the evaluation at t (1 <= t <= shape->timesteps), x_next (device int32
 * [batch][canvas]) the grid the sampler has just written.  logits device, rows of stride ldl >= n_classes elements of logits_dtype:
 *   plain     (row_of NULL, guidance NULL)  batch * canvas rows;
 *   guided    (guidance given)              2 * batch * canvas rows, the null twins behind the conditioned rows;
 *   indexed   (row_of device int32 [batch * canvas])  row r reads logits[row_of[r]], the index clamped into [0, batch * canvas - 1]:
 *             the buffer holds batch * canvas rows, as the deduplicated loop's does; 16-bit logits, no guidance. */
int d3pm_frame_scores_step(const d3pm_shape *shape, int batch, const void *logits, int logits_dtype, int ldl,
                           const int32_t *row_of, const d3pm_guidance *guidance, const int32_t *x_next, int t,
                           const d3pm_frame_scores *scores, void *stream);

/* d3pm_sample_loop_guided with the two grids: guidance may be NULL here (then d3pm_sample_loop_keys), and fp8_blocks is allowed when
 * keys and guidance are NULL.  The loop initialises both grids from x, then every iteration issues one more launch behind its sampler
 * launch (in the deduplicated loop in front of the next index).  x and trace are bit for bit those of the unscored loop; both grids
 * are those of d3pm_frame_scores_init + one d3pm_frame_scores_step behind each step of the chained step entries. */
int d3pm_sample_loop_scored(const d3pm_shape *shape, const d3pm_weights *weights, const d3pm_fp8_block_weights *fp8_blocks,
                            int batch, int32_t *x, const uint8_t *frame_mask, const d3pm_canvas *canvas, int t_start,
                            int t_stop, const void *film, const void *kv_text, const void *kv_prompt,
                            const d3pm_schedule *sched, uint64_t seed, uint32_t utt0, uint32_t flags, void *workspace,
                            size_t workspace_bytes, int32_t *trace, const d3pm_nucleus *nucleus, const d3pm_keys *keys,
                            const d3pm_guidance *guidance, const d3pm_frame_scores *scores, void *stream);

/* d3pm_reveal_loop_keys with the two grids: the launch goes behind the commit launch of every step and reads the grid it wrote. */
int d3pm_reveal_loop_scored(const d3pm_shape *shape, const d3pm_weights *weights, int batch, int32_t *x,
                            const uint8_t *frame_mask, const d3pm_canvas *canvas, const void *film, const void *kv_text,
                            const void *kv_prompt, const d3pm_schedule *sched, uint64_t seed, uint32_t utt0, uint32_t flags,
                            void *workspace, size_t workspace_bytes, int32_t *trace, const d3pm_nucleus *nucleus,
                            const d3pm_reveal *reveal, const d3pm_keys *keys, const d3pm_frame_scores *scores, void *stream);

/* ---- reveal with revision: later steps re-mask frames the model has come to doubt (additions; ABI version unchanged) ------------------
 * By its definition a row revealed by d3pm_reveal "is never drawn again": a frame committed from an almost empty canvas at step 0
 * stays, whatever the later evaluations say about it.  With d3pm_revise the frames that already hold an id compete again for their
 * place in every step (the Token-Critic / remasking family of decoders).  No statement about audio quality is made; what follows is
 * an exact definition.  Everything of d3pm_reveal holds unless changed here: the timesteps t_i, FREE rows, the Philox keys,
 * D3PM_FLAG_GREEDY, temperature / top_k / top_p on masked rows, canvas <= 1024 and n_q = 1.
 *   rows       a free row is MASKED (x_t == mask_id) or HELD (it holds an id j != mask_id): a row revealed by an earlier step is
 *              held, and so is a free row that was already an id when the loop started.
 * At the step that evaluates at t_i and is followed by t_{i+1}:
 *   masked row cand and score are those of d3pm_reveal, bit for bit: the same routine, arguments and noise.
 *   held row   with id j: cand = j.  conf_h is the logprob that d3pm_frame_scores defines for id j on this evaluation's logits:
 *              z = rn16(logit), mask class removed, NO temperature / top_k / top_p, the arithmetic order stated there -- bit for bit
 *              what d3pm_frame_scores_step reports for that row and id.  It is always finite, so a sampling filter can never force
 *              a re-mask.  score = (conf_h + hold_bonus) + lambda_i * gumbel(v): one fp32 add, then the same statement that turns
 *              a masked row's conf into its score; lambda_i and v (Philox key (seed; 0, global row, t_i, stream 4)) are unchanged.
 *              choice_temperature = 0, D3PM_FLAG_GREEDY and the last step draw no v.  An id j >= n_classes is outside the
 *              contract; no memory is read through j.
 *   quota      after the step utterance b holds  hold = F_b - floor((double) F_b * (double) float(cbar[t_{i+1}]))  ids on its free
 *              rows; after the last step it holds F_b.  The masked count after step i is therefore floor(F_b * cbar[t_{i+1}]),
 *              whatever the canvas looked like before; it does not grow from one step to the next, since cbar falls with t.
 *   selection  the order is the existing one: the uint32 image of the score, descending, then frame index ascending.  The `hold`
 *              free rows that come first among ALL free rows hold an id after the step: a selected masked row takes cand, a
 *              selected held row keeps its id, an unselected masked row stays masked, an unselected held row is re-masked (takes
 *              mask_id).  Known and padded rows are never given a value.  In place (x_next == x_t) only changed rows are stored.
 *              Given the scores the device reports, the result is exact.
 *   cand_out / score_out  receive a value for every free row; rows that are not free are left unwritten.
 *   frame scores  (optional d3pm_frame_scores) the commit launch sets step = 0, logprob = 0.0f on every row it re-masks, including a
 *              row whose step was -1 because it entered the loop as an id.  The existing launch behind it is unchanged: a re-masked
 *              row therefore records its next reveal, and at loop exit step / logprob describe the LAST time a row left the mask.
 *              Rows never re-masked keep what they had, bit for bit.
 * hold_bonus is the stickiness: 0 lets held and masked rows compete on equal terms; a bonus larger than any |conf| pins every held
 * row, so that rows are re-masked only where the quota demands it.
 * Refused with D3PM_E_ARG, nothing launched and no pointer read: a NULL d3pm_revise, a negative or non-finite hold_bonus; and
 * everything d3pm_reveal refuses.  Kernels of their own: a call without d3pm_revise runs none of this code. */
typedef struct d3pm_revise {
  float hold_bonus;     /* finite, >= 0 */
} d3pm_revise;

/* d3pm_reveal_step under d3pm_revise, the definition above: its arguments, then revise and the optional scores (NULL: no grids; else
 * both grids, which the commit launch resets on the rows it re-masks -- the launch behind it stays the caller's,
 * d3pm_frame_scores_step on x_next). */
int d3pm_reveal_step_revise(const d3pm_shape *shape, int batch, const void *logits, int logits_dtype, const int32_t *x_t,
                            int32_t *x_next, const uint8_t *frame_mask, const d3pm_canvas *canvas, int t, int t_next,
                            const d3pm_schedule *sched, uint64_t seed, uint32_t utt0, uint32_t flags, const d3pm_nucleus *nucleus,
                            float choice_temperature, int32_t *cand_out, float *score_out, const d3pm_revise *revise,
                            const d3pm_frame_scores *scores, void *stream);

/* d3pm_reveal_loop_scored under d3pm_revise, the definition above; keys and scores are optional (NULL).  The loop equals
 * d3pm_frame_scores_init + the chained d3pm_reveal_step_revise / d3pm_frame_scores_step entries, step by step; the second launch is
 * the fused one wherever d3pm_reveal_loop's is. */
int d3pm_reveal_loop_revise(const d3pm_shape *shape, const d3pm_weights *weights, int batch, int32_t *x,
                            const uint8_t *frame_mask, const d3pm_canvas *canvas, const void *film, const void *kv_text,
                            const void *kv_prompt, const d3pm_schedule *sched, uint64_t seed, uint32_t utt0, uint32_t flags,
                            void *workspace, size_t workspace_bytes, int32_t *trace, const d3pm_nucleus *nucleus,
                            const d3pm_reveal *reveal, const d3pm_keys *keys, const d3pm_revise *revise,
                            const d3pm_frame_scores *scores, void *stream);

/* Replaces AR.q_sample / q_probs (ar_discrete.py:467-502): forward noising of x0 at step t with
 * Philox stream 1.  x0, x_out device int32 [batch][canvas]. */
int d3pm_q_sample(const d3pm_shape *shape, int batch, const int32_t *x0, int32_t *x_out,
                  const uint8_t *frame_mask, int t, const d3pm_schedule *sched, uint64_t seed,
                  uint32_t utt0, void *stream);

/* Training-side loss of one denoiser evaluation (AR.forward, ar_discrete.py:683-690; SURVEY.md §8f row 3, forward
 * half): row_loss[b][i] = logsumexp(x) - x[target] with x = logits[b][i][:] * mask[i], target = targets[b][i] (already
 * multiplied by the mask by the caller), fp32.  A padded frame (mask 0) yields log(n_classes).  logits device
 * [batch][canvas][n_classes] contiguous in `logits_dtype`; targets device int32 [batch][canvas]; row_loss device fp32
 * [batch][canvas].  The reference's loss of one step is the mean of these rows; the backward pass is not part of
 * this library. */
int d3pm_ce_loss_rows(const d3pm_shape *shape, int batch, const void *logits, int logits_dtype,
                      const int32_t *targets, const uint8_t *frame_mask, float *row_loss, void *stream);

/* The raw uniform stream the two samplers consume (what the reference draws with torch.rand,
 * ar_discrete.py:402,480): out device fp32 [rows][n_classes] for global rows row0.. at step t. */
int d3pm_uniform(uint64_t seed, int t, uint32_t row0, int rows, int n_classes, int stream_id,
                 float *out, void *stream);

/* Stock NAR model: quantizer levels 1..7 given level 0 ----------------------------
 * Replaces one pass of NAR.forward's inference loop (nar.py:76-101) = Base.forward (base.py:403-499) at
 * `quant_levels = level`: input assembly [text | sep | prompt | sep | response] + sinusoid, n_layers x
 * {AdaLN -> masked attention -> residual, AdaLN -> GELU FFN -> residual} (:161-234), classifier, and the
 * temperature sampling of the response rows (Gumbel-max over Philox stream 2 instead of torch's multinomial). */
typedef struct d3pm_nar_shape {
  int32_t d_model, n_heads, n_layers, n_tokens, n_prom_levels, n_resp_levels, dtype;
  const d3pm_tuning *tuning;   /* as in d3pm_shape */
} d3pm_nar_shape;

typedef struct d3pm_nar_block_weights {
  const void *attn_norm_emb;        /* blocks.i.attn.norm.emb.weight [n_resp_levels][2d]  (AdaLN :139) */
  const void *to_qkv_w;             /* [3d][d], no bias (:100)                                         */
  const void *to_out_w, *to_out_b;  /* [d][d], [d] (:101)                                              */
  const void *ffn_norm_emb;         /* blocks.i.ffn.norm.emb.weight                                    */
  const void *ffn0_w, *ffn0_b;      /* [4d][d], [4d] (:216)                                            */
  const void *ffn3_w, *ffn3_b;      /* [d][4d], [d]  (:219)                                            */
} d3pm_nar_block_weights;

typedef struct d3pm_nar_weights {
  const void *text_emb;             /* [n_tokens][d]                 (:336) */
  const void *proms_emb;            /* [n_prom_levels][n_tokens][d]  (:339) */
  const void *resps_emb;            /* [n_resp_levels][n_tokens][d]  (:340) */
  const void *sep;                  /* [d]                           (:344) */
  const void *classifier_w, *classifier_b;   /* [n_tokens][d], [n_tokens] (:360) */
  const void *pe;                   /* [pe_rows][d] sinusoid table in the model dtype (:38-89) */
  int32_t pe_rows;
  const d3pm_nar_block_weights *blocks;      /* HOST array of n_layers entries */
} d3pm_nar_weights;

size_t d3pm_nar_workspace_bytes(const d3pm_nar_shape *shape, int batch, int t_max);

/* lens device int32 [batch][3] = (t_text, t_prompt, t_response); text device int32 [batch][tt_max];
 * prom device int32 [batch][tp_max][n_prom_levels] (-1 = level absent); resp device int32
 * [batch][tr_max][n_resp_levels+1], levels 0..level given, level+1 written; t_max >= max(t_text+t_prompt+t_resp+2);
 * logits_out optional device [batch][t_max][n_tokens] of `dtype` (all rows, before sampling) or NULL. */
int d3pm_nar_level(const d3pm_nar_shape *shape, const d3pm_nar_weights *w, int batch, int t_max, const int32_t *lens,
                   const int32_t *text, int tt_max, const int32_t *prom, int tp_max, int32_t *resp, int tr_max,
                   int level, float temperature, uint64_t seed, uint32_t utt0, uint32_t flags, void *workspace,
                   size_t workspace_bytes, void *logits_out, void *stream);

/* The level draw with options: known frames, top-k / top-p, log-probabilities ----------------------------------------------
 * What d3pm_sampling / d3pm_nucleus / `known` / d3pm_frame_scores are to the D3PM stage, for the draw of levels 1..7.  Per response
 * frame, on the row's n_tokens logits l_j of storage type T (no tolerance anywhere):
 *     v_j    = rn<T>(float(l_j) / temperature)         what the draw without options compares
 *     theta1 = the top_k-th largest v_j counted with multiplicity                          (top_k 0: -inf)
 *     v'_j   = v_j >= theta1 ? v_j : -inf              ties at theta1 are all kept, so >= top_k classes survive
 *     m      = max v'_j,  q_j = (uint32) (expf(v'_j - m) * 1048576.0f),  Q = sum_j q_j     (integers: the same in any order)
 *     theta  = value of the LARGEST order key c with (double) mass(c) >= (double) top_p * (double) Q,  mass(c) = sum_{key(v'_j) >= c} q_j
 *                                                                                          (top_p 1: -inf)
 *     v''_j  = v'_j >= theta ? v'_j : -inf             compared on VALUES: -0 / +0 stand or fall together
 *     id     = first-index argmax_j v''_j + gumbel(u_j)                                    (D3PM_FLAG_GREEDY: of v''_j)
 * i.e. d3pm_sampling / d3pm_nucleus above restated for the NAR's v, and a call equals the draw without options fed with the
 * host-filtered v'' stored in T at temperature 1, id for id.  The order key is that of the value in ITS OWN storage type: 16 bits of
 * the f16 / bf16 pattern, 32 bits of an fp32 (negative values reverse, the others move above them).  What d3pm_nucleus lists holds
 * here as well: theta is one of the row's values; the maximum is always kept; top_p <= 1/1280 keeps exactly the classes tied at the
 * maximum (the ids of top_k = 1); for every set S of classes |sum_S q / Q - sum_S softmax(v')| <= n_tokens / 2^20 + 2^-20.  The noise
 * does not move: u_j is the Philox word of (j >> 2, (utt0 + b) * 65536 + f, level, stream 2) whatever is cut, and a class that was
 * cut still draws its own.  A row that is -inf throughout is outside the top-p contract; it still gets an id in 0 .. n_tokens - 1.
 *   top_p        finite, 0 < top_p <= 1; 1 = off            top_k  0 = off, else 1 .. n_tokens
 *   known        device uint8 [batch][tr_max] or NULL: a frame with known[b][f] != 0 is not drawn, resp[b][f][level + 1] stays exactly
 *                as the caller put it; every other frame takes the id it takes without `known`.
 *   logprob_out  device float [batch][tr_max][n_resp_levels] or NULL: entry [b][f][level] = z_j - max z - logf(sum_k expf(z_k - max z))
 *                over z = float(l) -- the row's own logits: no temperature, no top-k, no top-p, no further rounding -- at the id j
 *                that stands in resp[b][f][level + 1] after the call (the drawn id, or a known frame's held id; an id outside
 *                0 .. n_tokens - 1 reads nothing and gives -inf).  Per-lane partial sums in ascending class, then the wave's sum, as in
 *                d3pm_frame_scores.  Finite whenever l_j is finite; within 1.0e-4 of the fp64 log-softmax.
 *   theta_out    device float [batch][tr_max] or NULL: the row's theta (-inf when nothing is cut), NaN on a known frame.  Non-NULL
 *                takes the kernel's nucleus arm whatever top_p is; the ids are those of the same call without it.
 * Frames outside an utterance (f >= t_response) or outside the grid write nothing to resp, logprob_out or theta_out.
 * A NULL d3pm_nar_draw, or {1.0f, 0, NULL, NULL, NULL}, launches what the entry without it launches, bit for bit; anything else
 * takes the kernel of csrc/d3pm_nar_draw.hip, which needs n_tokens <= 1280 (D3PM_E_SHAPE otherwise).  Refused with D3PM_E_ARG before
 * anything is launched: a temperature that is not finite and > 0, top_k outside 0 .. n_tokens, top_p not finite or outside (0, 1]. */
typedef struct d3pm_nar_draw {
  float top_p;
  int32_t top_k;
  const uint8_t *known;
  float *logprob_out;
  float *theta_out;
} d3pm_nar_draw;

/* d3pm_nar_level with draw options. */
int d3pm_nar_level_draw(const d3pm_nar_shape *shape, const d3pm_nar_weights *w, int batch, int t_max, const int32_t *lens,
                        const int32_t *text, int tt_max, const int32_t *prom, int tp_max, int32_t *resp, int tr_max,
                        int level, float temperature, uint64_t seed, uint32_t utt0, uint32_t flags, void *workspace,
                        size_t workspace_bytes, void *logits_out, const d3pm_nar_draw *draw, void *stream);

/* Classifier-free guidance in the level draw (additions; ABI version unchanged) ------------------------------------------------------
 * The d3pm_guidance struct above, for levels 1..7: every level draws from the extrapolated logits of its frame, as the D3PM stage does for
 * level 0.  Exact definition:
 *   null twin    the twin of utterance b is the same utterance with no phonemes and no prompt frames: input assembly
 *                [sep | sep | response], i.e. t_text = t_prompt = 0 and the same response levels.  No new weights, no new embedding
 *                rule: a twin is an ordinary utterance of the grid, and a caller may put any "negative" text or prompt there instead.
 *   evaluation   a guided level is ONE evaluation of 2 * batch utterances, utterance batch + b the twin of b: exactly what
 *                d3pm_nar_level launches for those 2 * batch utterances, up to and including the classifier.
 *   guided row   for frame f of pair b, with c_j = row t_text_b + t_prompt_b + 2 + f of utterance b and u_j = row t_text_n +
 *                t_prompt_n + 2 + f of utterance batch + b (the twin's own lengths), both of the logits' storage type T:
 *                    z_j = rn<T>( fmaf(w, float(c_j) - float(u_j), float(c_j)) )
 *                -- the subtraction in fp32, an explicit fma, ONE rounding to T (none for fp32).  Everything behind it is the draw of
 *                d3pm_nar_draw with z in place of l: v_j = rn<T>(z_j / temperature), top-k, top-p and the order key in T, Gumbel-max
 *                with the Philox words of (j >> 2, (utt0 + b) * 65536 + f, level, stream 2) -- b the LOGICAL index, so the noise is
 *                that of the unguided call --, D3PM_FLAG_GREEDY, theta_out, and logprob_out = the log-softmax of z (the guided
 *                logits, as d3pm_frame_scores has it under guidance).  Where c == u, z = c for any w; w = 0 is legal and gives z = c.
 *   frames       a frame is skipped (nothing read, nothing written) if f >= t_response of b or if either of its two rows lies
 *                outside the grid.  The drawn id goes to resp[b][f][level + 1] AND to resp[batch + b][f][level + 1]: two halves that
 *                start equal stay equal through all seven levels.  A known frame writes nothing: the caller put its codes into
 *                both halves.
 * `batch` counts LOGICAL utterances; lens / text / prom / resp hold 2 * batch utterances; the workspace is
 * d3pm_nar_workspace_bytes of (shape, 2 * batch, t_max); logits_out (optional) is [2 * batch][t_max][n_tokens]; draw may be NULL and
 * its known / logprob_out / theta_out are [batch]...  Under guidance every draw is the kernel of csrc/d3pm_nar_draw.hip, with no cut
 * where no option is set.  Refused, nothing launched: D3PM_E_ARG for a NULL d3pm_guidance, a negative or non-finite weight and
 * anything d3pm_nar_draw refuses; D3PM_E_SHAPE for n_tokens > 1280; D3PM_E_WORKSPACE for a workspace that is too small.  A call
 * without guidance runs none of this: the plain kernels take no further argument.  No statement about audio quality is made:
 * guidance is meaningful for weights trained with the conditions dropped some of the time (vall_e/vall_e/nar.py: cond_drop). */
int d3pm_nar_level_guided(const d3pm_nar_shape *shape, const d3pm_nar_weights *w, int batch, int t_max, const int32_t *lens,
                          const int32_t *text, int tt_max, const int32_t *prom, int tp_max, int32_t *resp, int tr_max,
                          int level, float temperature, uint64_t seed, uint32_t utt0, uint32_t flags, void *workspace,
                          size_t workspace_bytes, void *logits_out, const d3pm_nar_draw *draw, const d3pm_guidance *guidance,
                          void *stream);

/* Single-operator entry points (kernel-level parity tests and micro-benchmarks).  `family`:
 * 0 = auto (MFMA when the shape tiles, else generic), 1 = generic FMA kernels, 2 = MFMA (fails with
 * D3PM_E_SHAPE when unsupported).  Same contracts as inside the denoiser:
 *   linear:    Y[M][N] = epilogue(X[M][K] . W[N][K]^T + bias), act 0 none / 1 exact-erf GELU,
 *              optional residuals R1 (+R2) [M][N] and row mask (see csrc/d3pm_kernels.h)
 *   attention: per (utterance, head) softmax(rn(q*scale) . k^T) . v with Q [B*Tq][ldq], K/V [B*S][ldkv]
 *   layernorm: Y = LN(X)*w + b over the last dim (eps 1e-6), optional FiLM vector [2d] */
int d3pm_op_linear(int dtype, int family, const void *X, int ldx, const void *W, const void *bias, void *Y,
                   int ldy, const void *R1, const void *R2, int ldr, const uint8_t *row_mask,
                   int mask_period, int M, int N, int K, int act, const d3pm_tuning *tuning, void *stream);
/* Block-scaled fp8 single ops (BASELINE.json configs[4]; no reference counterpart: the reference is fp16 only).  Formats as
 * in d3pm_fp8_block_weights: codes [rows][K], scales [rows][4][K / 128].
 *   quantize_mx:   any 16-bit X [M][K] (K a multiple of 128) -> X8, SX; scale of a block = the smallest power of two with
 *                  absmax / scale <= 448, codes = rn_e4m3(x / scale) (never saturate);
 *   layernorm_mx:  Y8 [M][512], SX [M][4][4] = quantize_mx(LN(X) * w + b [FiLM]), the 16-bit LayerNorm result being exactly
 *                  d3pm_op_layernorm's;
 *   linear_mx:     epilogue(sum_k X8 2^sx . W8 2^sw + bias) with fp32 accumulation: act 0 none / 1 GELU, optional residual
 *                  R1 [M][N] and row mask as d3pm_op_linear, 16-bit output Y [M][ldy] in `out_dtype` -- or, with Y8 / SY given
 *                  (R1 = row_mask = NULL, Y ignored), the output itself in the MX format: Y8 [M][N], SY [M][4][N / 128].
 *                  M a multiple of 192, N of 128, K of 512.  tuning->gemm_variant 6 / 8 pins the 192 x 256 / 192 x 128 tile. */
int d3pm_op_quantize_mx(int dtype, const void *X, int ldx, void *X8, void *SX, int M, int K, void *stream);
int d3pm_op_layernorm_mx(int dtype, const void *X, void *Y8, void *SX, const void *w, const void *b, const void *film, int M,
                         int d, float eps, void *stream);
/* layernorm_mx with a second LayerNorm (w2, b2) of the same rows and the same moments -> Y8_2, SX_2, as the sampler's norm2 | norm22
 * launch; FiLM applies to the first output alone.  Every pointer but `film` is required. */
int d3pm_op_layernorm_mx_pair(int dtype, const void *X, void *Y8, void *SX, const void *w, const void *b, const void *film,
                              const void *w2, const void *b2, void *Y8_2, void *SX_2, int M, int d, float eps, void *stream);
int d3pm_op_linear_mx(int out_dtype, const void *X8, int ldx, const void *SX, const void *W8, const void *SW, const void *bias,
                      void *Y, int ldy, const void *R1, int ldr, const uint8_t *row_mask, int mask_period, void *Y8, void *SY,
                      int M, int N, int K, int act, const d3pm_tuning *tuning, void *stream);
/* The folded-LayerNorm pieces as single ops (MFMA family, 16-bit; d3pm_fold_block above):
 *   row_stats     per row and 32-column part the pair (sum x, sum x^2), fp32 -- what a producing projection leaves behind -- in the
 *                 layout [ceil(M / 16)][d / 32][16][2] (the 16 rows of a row block side by side: one part of one row block is one
 *                 128-byte line): the pair of (row, part) starts at float (((row / 16) * (d / 32) + part) * 16 + row % 16) * 2.
 *                 The buffer therefore holds slots for the rows M .. 16 ceil(M / 16) - 1 as well; no row owns them and no producer --
 *                 row_stats, linear_stats, linear_live, the sampler's launches -- writes them (every store of a pair is predicated on
 *                 row < M), and no consumer reads them (rows beyond M read the pair of row M - 1 and are not stored).  They keep
 *                 what the caller left there (tests/test_gpu_gemm_edges.py);
 *   linear_stats  d3pm_op_linear with a residual (R1 [+ R2] [+ row mask]) that also writes the moments of the rows it stores (N = d);
 *   linear_fold   Y = act(rstd_r (X_r . Wf^T - mean_r fold_s) + fold_b) with the moments of X's rows from `stats_in` (layout of row_stats, K columns)
 *                 (X = the raw rows, Wf / fold_s / fold_b as d3pm_fold_build makes them); act 0 / 1 (GELU). */
int d3pm_op_row_stats(int dtype, const void *X, int ldx, int M, int d, float *stats, void *stream);
int d3pm_op_linear_stats(int dtype, const void *X, int ldx, const void *W, const void *bias, void *Y, int ldy, const void *R1,
                         const void *R2, int ldr, const uint8_t *row_mask, int mask_period, int M, int N, int K, float *stats_out,
                         const d3pm_tuning *tuning, void *stream);
int d3pm_op_linear_fold(int dtype, const void *X, int ldx, const void *Wf, const float *fold_s, const float *fold_b,
                        const float *stats_in, float eps, void *Y, int ldy, int M, int N, int K, int act, const d3pm_tuning *tuning,
                        void *stream);
/* Row deduplication (tests; the unguided sampler loop runs it under ln_fold = 1, see d3pm_tuning).  tokens / frame_mask [batch][canvas].
 * The class of a position is its id (clamped to the classes), or n_classes where frame_mask is 0; the first position of each class of an
 * utterance is its representative, ranked in position order.  Utterance b owns the compact rows seg_start[b] .. + seg_len[b] (its class
 * count rounded up to 128), m_live = their sum, row_of [batch * canvas] maps a position to its compact row, cid / cmask
 * [batch * canvas] hold the class and the frame-mask byte of compact row r < the next multiple of 384 of m_live (n_classes / 0 on rows
 * no class owns).  With `table` [n_classes][d]: x [batch * canvas][d] receives the embedding rows of the compact rows (zeros on padded
 * or unowned rows) and stats their moments (quads when d = 512, else parts).  scratch: int32 [batch * canvas + batch].  canvas must be a
 * multiple of 128 and batch * canvas of 384, n_classes at most 4095, batch at most 12283 (the embedding launch keeps the prefix of the
 * counts in 48 KiB of LDS); D3PM_E_SHAPE otherwise, nothing launched. */
int d3pm_op_dedup_index(int dtype, const int32_t *tokens, const uint8_t *frame_mask, int batch, int canvas, int n_classes, int d,
                        const void *table, int32_t *seg_start, int32_t *seg_len, int32_t *m_live, int32_t *row_of, int32_t *cid,
                        uint8_t *cmask, void *x, float *stats, int32_t *scratch, void *stream);
/* The same index with the segment granularity chosen: seg_align = 128 is d3pm_op_dedup_index array for array; seg_align = 1 is the
 * layout the sampler loop runs on -- seg_len[b] = the class count of utterance b, seg_start[b] = the exclusive prefix sum of the
 * counts, m_live = their sum, no zero row inside a segment; rows m_live .. the next multiple of 384 stay zero rows with zero moments,
 * cid = n_classes, cmask = 0.  Any other seg_align is D3PM_E_ARG. */
int d3pm_op_dedup_index_align(int dtype, const int32_t *tokens, const uint8_t *frame_mask, int batch, int canvas, int n_classes, int d,
                              int seg_align, const void *table, int32_t *seg_start, int32_t *seg_len, int32_t *m_live, int32_t *row_of,
                              int32_t *cid, uint8_t *cmask, void *x, float *stats, int32_t *scratch, void *stream);
/* A projection whose live row count is read from device memory at kernel entry (tests): the arguments of d3pm_op_linear_stats /
 * d3pm_op_linear_fold (X2: the second operand of the dual out-projection or NULL; moments travel as quads at width 512), M = the
 * capacity the launch is planned for; only the tiles that hold a row < *m_live run.  Big-tile family or the 128 x 128 one-tile-per-
 * workgroup kernel, D3PM_E_SHAPE otherwise. */
int d3pm_op_linear_live(int dtype, const void *X, const void *X2, int ldx, const void *W, const void *bias, void *Y, int ldy,
                        const void *R1, int ldr, const uint8_t *row_mask, int mask_period, int M, int N, int K, int act,
                        const float *fold_s, const float *fold_b, const float *stats_in, float *stats_out, const int32_t *m_live,
                        const d3pm_tuning *tuning, void *stream);
/* The same with the host's estimate of *m_live (tests; 0 = none, which is d3pm_op_linear_live): an estimate within the latency bound of
 * the sampler loop (or gemm_variant = 4 with any estimate) plans the 64 x 64 latency family, whose grid covers min(M, m_est) rows and
 * whose workgroups walk the live tiles in rounds -- any *m_live in 0 .. M gives the same rows as every other family.  On that family the
 * moments travel as 32-column parts (the layout of d3pm_op_row_stats), and the dual form takes M a multiple of 32. */
int d3pm_op_linear_live_est(int dtype, const void *X, const void *X2, int ldx, const void *W, const void *bias, void *Y, int ldy,
                            const void *R1, int ldr, const uint8_t *row_mask, int mask_period, int M, int N, int K, int act,
                            const float *fold_s, const float *fold_b, const float *stats_in, float *stats_out, const int32_t *m_live,
                            int m_est, const d3pm_tuning *tuning, void *stream);
/* The same with the second estimate, the one the loop gives the projections onto the residual stream in the iterations that stay on big
 * tiles (tests; rows_est = 0 = none, which is d3pm_op_linear_live_est): with 0 < rows_est < M and gemm_variant = 0 the big-tile geometry
 * of a projection with R1 and quads out (the dual included) is chosen for the tiles of rows_est rows -- 96 x 128 or 128 x 128 instead
 * of 192 x 128 while those fit two per CU in one round.  Any *m_live in 0 .. M gives the same rows whatever the estimate. */
int d3pm_op_linear_live_rows(int dtype, const void *X, const void *X2, int ldx, const void *W, const void *bias, void *Y, int ldy,
                             const void *R1, int ldr, const uint8_t *row_mask, int mask_period, int M, int N, int K, int act,
                             const float *fold_s, const float *fold_b, const float *stats_in, float *stats_out, const int32_t *m_live,
                             int m_est, int rows_est, const d3pm_tuning *tuning, void *stream);
/* The block-0 QKV rows of `n` token ids as the sampler loop makes them under ln_fold = 1 (tests): builds the table [rows][3 d_model]
 * (row id = the folded QKV projection of resps_emb[id] with that row's moments, row n_classes = that of a zero row) in `storage`
 * (device, 256-byte aligned, >= d3pm_op_embed_qkv_bytes(shape, n)), then q_out[r] [n][d_model] | kv_out[r] [n][2 d_model] = the q and
 * the k | v columns of row (frame_mask[r] ? tokens[r] clamped to the classes : n_classes), as the loop keeps them.  weights->fold
 * must be set; 16-bit dtype, d_model a multiple of 256, n_q <= 1.  q | k | v of a row equal d3pm_op_linear_fold on the gathered
 * embedding rows with their d3pm_op_row_stats moments, bit for bit. */
size_t d3pm_op_embed_qkv_bytes(const d3pm_shape *shape, int n);
int d3pm_op_embed_qkv(const d3pm_shape *shape, const d3pm_weights *weights, const int32_t *tokens, const uint8_t *frame_mask, int n,
                      void *storage, size_t storage_bytes, void *q_out, void *kv_out, void *stream);
/* One projection's tables as d3pm_fold_build makes them (tests): W [N][K], bias [N] or NULL, gamma / beta [K], film NULL or
 * (scale [K] | shift [K]) -> Wf [N][K], fold_s / fold_b [N]. */
int d3pm_op_fold_weights(int dtype, const void *W, const void *bias, const void *gamma, const void *beta, const void *film, int N, int K,
                         void *Wf, float *fold_s, float *fold_b, void *stream);
int d3pm_op_attention(int dtype, int family, const void *Q, int ldq, const void *K, const void *V, int ldkv,
                      void *O, int ldo, int B, int Tq, int S, int H, int hd, float scale, const d3pm_tuning *tuning,
                      void *stream);
/* d3pm_op_attention with the per-utterance key mask of the stock NAR attention: key_len (device int32 [B]) = the number of valid
 * keys of each utterance, keys >= key_len[b] are masked out and S is the padded key count (the row stride of the K / V batches);
 * NULL = d3pm_op_attention.  1 <= key_len[b] <= S is the caller's contract: the values live on the device and are read by the
 * kernels only, so nothing here can refuse them.  Family 2: attn_query_groups 0 keeps the automatic choice between one and two
 * query groups of the 16 x 16 x 32 kernel (a masked call never moves to the 32 x 32 x 16 kernel by itself); 1 / 2 name them; 32 / 33
 * take the masked 32 x 32 x 16 kernels (pipelined / plain walk) where the shape is eligible -- Tq a multiple of 128 and S of 64 --
 * and fall back to the automatic choice elsewhere; 4 (the key-split kernel) refuses a mask and falls back likewise. */
int d3pm_op_attention_keylen(int dtype, int family, const void *Q, int ldq, const void *K, const void *V, int ldkv, void *O, int ldo,
                             int B, int Tq, int S, int H, int hd, float scale, const int32_t *key_len, const d3pm_tuning *tuning,
                             void *stream);
/* The self-attention of the deduplicated loop (tests): the pipelined 32 x 32 x 16 kernel with query segments and its keys read through
 * a row index, whatever the grid size.  Q / O [rows][ldq / ldo]: the queries and output rows of utterance b are the seg_len[b] rows (any
 * count from 1 to Tq) from row seg_start[b] (any row); rows no segment owns are neither read nor written.  K / V [kv_rows][ldkv], views of one pool:
 * key j of utterance b is row key_row[b * S + j] (device int32 [B][S]), clamped into [0, kv_rows - 1]; kv_rows * ldkv * the element
 * size must stay under 2^32 and S at or under 4096.  key_len as d3pm_op_attention_keylen, or NULL.  16-bit dtype, head width 64, Tq a
 * multiple of 128 and S of 64, D3PM_E_SHAPE otherwise.  The same key values in the same order as d3pm_op_attention on the gathered
 * rows under attn_query_groups = 32: the same bits. */
int d3pm_op_attention_gather(int dtype, const void *Q, int ldq, const void *K, const void *V, int ldkv, int kv_rows,
                             const int32_t *key_row, const int32_t *seg_start, const int32_t *seg_len, void *O, int ldo, int B, int Tq,
                             int S, int H, int hd, float scale, const int32_t *key_len, const d3pm_tuning *tuning, void *stream);
/* d3pm_op_attention_gather with the K | V rows of an utterance pooled in LDS (tests): what the deduplicated loop launches in the
 * iterations that expect few distinct rows per utterance.  The workgroups of an utterance with seg_len[b] <= pool_rows copy, per head,
 * pool row r = row pool_src[seg_start[b] + r] of K / V (pool_src NULL: row seg_start[b] + r), clamped into [0, kv_rows - 1], for
 * r < seg_len[b], and read key j from pool row seg_key[b * S + j] - seg_start[b], clamped into [0, seg_len[b] - 1] (seg_key: device
 * int32 [B][S]); those of an utterance with more rows walk key_row as d3pm_op_attention_gather does, in the same launch.  The caller
 * promises that both ways name rows with the same bytes: the result is then d3pm_op_attention_gather's, bit for bit.  The grid holds
 * qblocks_grid (1 .. Tq / 128) 128-query blocks per (utterance, head) and a workgroup strides over the blocks of its segment.  The
 * tiles (48 KiB), the index (4 S bytes) and the pool (256 bytes per row) must fit 160 KiB of LDS; D3PM_E_SHAPE otherwise. */
int d3pm_op_attention_gather_pool(int dtype, const void *Q, int ldq, const void *K, const void *V, int ldkv, int kv_rows,
                                  const int32_t *key_row, const int32_t *seg_start, const int32_t *seg_len, void *O, int ldo, int B,
                                  int Tq, int S, int H, int hd, float scale, const int32_t *key_len, const int32_t *seg_key,
                                  const int32_t *pool_src, int pool_rows, int qblocks_grid, const d3pm_tuning *tuning, void *stream);
/* The text and prompt cross-attentions of a DiT block (ar_discrete.py:138,142) as the block launches them: two independent
 * problems with the same B / Tq / H / hd -- queries Q1 / Q2 [B][Tq][ldq], keys and values K / V [B][S][ldkv] with S1 / S2 keys,
 * outputs O1 / O2 [B][Tq][ldo] -- in ONE launch (tuning->attn_cross_resident / attn_pair_sequential pick the schedule). */
int d3pm_op_attention_pair(int dtype, const void *Q1, const void *K1, const void *V1, void *O1, int S1, const void *Q2,
                           const void *K2, const void *V2, void *O2, int S2, int ldq, int ldkv, int ldo, int B, int Tq, int H,
                           int hd, float scale, const d3pm_tuning *tuning, void *stream);
/* d3pm_op_attention_pair with a key mask per problem: key_len1 / key_len2 (device int32 [B], either may be NULL) = the valid keys
 * among the S1 / S2 padded ones, which stay the row strides of the K / V batches.  Contract as d3pm_op_attention_keylen.  Every
 * pair schedule takes the masks except the key-split kernel (attn_query_groups = 4), which falls back to the tile-by-tile pair. */
int d3pm_op_attention_pair_keylen(int dtype, const void *Q1, const void *K1, const void *V1, void *O1, int S1, const void *Q2,
                                  const void *K2, const void *V2, void *O2, int S2, int ldq, int ldkv, int ldo, int B, int Tq,
                                  int H, int hd, float scale, const int32_t *key_len1, const int32_t *key_len2,
                                  const d3pm_tuning *tuning, void *stream);
/* The cross pair of the deduplicated loop (tests): d3pm_op_attention_pair_keylen with query segments.  Q1 / Q2 / O1 / O2 [rows][ldq / ldo]:
 * the queries and output rows of utterance b are the seg_len[b] rows (any count from 1 to Tq, the capacity per utterance) from row
 * seg_start[b] (any row; device int32 [B] each); rows no segment owns are neither read nor written.  K / V [B][S][ldkv] and key_len1 / key_len2
 * (either may be NULL) as in d3pm_op_attention_pair_keylen.  The kernel is the planner's choice under `tuning` like every other call;
 * only the resident 32 x 32 x 16 pair takes segments (S1 <= 64, S2 <= 256, attn_cross_resident on), any other plan is D3PM_E_SHAPE
 * with nothing launched.  A row's bits are those of d3pm_op_attention_pair on the segment's rows alone under attn_cross_resident = 5. */
int d3pm_op_attention_pair_segments(int dtype, const void *Q1, const void *K1, const void *V1, void *O1, int S1, const void *Q2,
                                    const void *K2, const void *V2, void *O2, int S2, int ldq, int ldkv, int ldo, int B, int Tq,
                                    int H, int hd, float scale, const int32_t *seg_start, const int32_t *seg_len,
                                    const int32_t *key_len1, const int32_t *key_len2, const d3pm_tuning *tuning, void *stream);
/* The sampler launch of the deduplicated loop on its own (tests; no fold of the next iteration): canvas row r of batch * canvas draws
 * x_next[r] from the logits of compact row row_of[r] (device int32 [batch * canvas], clamped into [0, batch * canvas - 1] by the
 * kernel); logits device [batch * canvas][ldl] of a 16-bit logits_dtype, ldl >= n_classes.  Everything else stays per canvas row: x_t,
 * the Philox row utt0 * canvas + r, `known` (uint8 [batch * canvas] or NULL: a marked row keeps x_t and reads neither its index nor
 * any logits).  x_next2 (or NULL) receives the same ids (the loop's trace).  flags: D3PM_FLAG_GREEDY; nucleus NULL = the neutral
 * triple.  The ids are those of d3pm_posterior_sample(_known / _sampling / _nucleus) on the gathered rows.  Refused with D3PM_E_ARG,
 * nothing launched: a NULL row_of, fp32 logits, n_q > 1, a non-NULL guidance (the deduplicated launch has no guided form). */
int d3pm_op_posterior_sample_rows(const d3pm_shape *shape, int batch, const void *logits, int logits_dtype, int ldl,
                                  const int32_t *row_of, const int32_t *x_t, int32_t *x_next, int32_t *x_next2, const uint8_t *known,
                                  int t, const d3pm_schedule *sched, uint64_t seed, uint32_t utt0, uint32_t flags,
                                  const d3pm_nucleus *nucleus, const d3pm_guidance *guidance, void *stream);
/* The three kernels of the stock NAR stage one at a time (tests): each entry validates on the host and then makes the one call
 * d3pm_nar_level makes, with no kernel choice of its own.  Refused with D3PM_E_ARG, nothing launched: a NULL pointer, an unknown
 * dtype, a size that is not positive, and what each entry names below.
 *   d3pm_op_nar_embed   the input assembly: arrays as in d3pm_nar_level (resp [batch][tr_max][resp_stride], levels 0 .. n_given - 1
 *                       summed; prom levels with a code < 0 skipped; ids clamped into [0, n_tokens - 1]); tables of `dtype`: w_text
 *                       [n_tokens][d], w_prom [n_prom_levels][n_tokens][d], w_resp [>= n_given][n_tokens][d], sep [d], pe [>= t_max][d].
 *                       Writes x [batch][t_max][d] (rows at or past an utterance's total = t_text + t_prompt + t_response + 2 are
 *                       zero; an utterance longer than t_max is cut at the grid), row_mask uint8 [batch][t_max] = (pos < total) and
 *                       key_len int32 [batch] = total.  1 <= n_given <= resp_stride.
 *   d3pm_op_adaln       y[r] = row_mask[r] ? AdaLN(x[r]) : 0 over [M][d] with emb_row [2d] = (log gamma | beta) of one level, every
 *                       intermediate rounded to `dtype`.  16-bit rows of width 512 / 1024 take the 16-byte kernels when x, y and
 *                       emb_row are 16-byte aligned and the scalar kernel otherwise (the launcher's rule, not this entry's).
 *   d3pm_op_nar_sample  the draw of level `level + 1`: logits [batch][t_max][ldl] of `dtype`, ldl >= n_tokens; frame f < t_response of
 *                       utterance b reads grid row t_text + t_prompt + 2 + f (a row outside the grid is skipped) and writes
 *                       resp[b][f][level + 1] = first-index argmax_j rn(logit_j / temperature) + gumbel(u_j), u from the Philox
 *                       counter (j >> 2, (utt0 + b) * 65536 + f, level, stream 2); flags: D3PM_FLAG_GREEDY = no noise.
 *                       temperature > 0, 0 <= level, level + 1 < resp_stride. */
int d3pm_op_nar_embed(int dtype, const int32_t *lens, const int32_t *text, int tt_max, const int32_t *prom, int tp_max, int n_prom_levels,
                      const int32_t *resp, int tr_max, int resp_stride, int n_given, const void *w_text, const void *w_prom,
                      const void *w_resp, const void *sep, const void *pe, void *x, uint8_t *row_mask, int32_t *key_len, int batch,
                      int t_max, int d, int n_tokens, void *stream);
int d3pm_op_adaln(int dtype, const void *x, void *y, const void *emb_row, const uint8_t *row_mask, int M, int d, void *stream);
int d3pm_op_nar_sample(int dtype, const void *logits, int ldl, const int32_t *lens, int32_t *resp, int tr_max, int resp_stride, int t_max,
                       int n_tokens, int level, float temperature, uint64_t seed, uint32_t utt0, uint32_t flags, int batch, void *stream);
/* d3pm_op_nar_sample with draw options (d3pm_nar_draw above, with n_resp_levels = resp_stride - 1 in logprob_out's layout): the call
 * d3pm_nar_level_draw makes behind its classifier.  Refusals as for d3pm_op_nar_sample, and those d3pm_nar_draw lists. */
int d3pm_op_nar_draw(int dtype, const void *logits, int ldl, const int32_t *lens, int32_t *resp, int tr_max, int resp_stride, int t_max,
                     int n_tokens, int level, float temperature, uint64_t seed, uint32_t utt0, uint32_t flags, int batch,
                     const d3pm_nar_draw *draw, void *stream);
/* d3pm_op_nar_draw under guidance: the one draw launch of d3pm_nar_level_guided on given logits [2 * batch][t_max][ldl], lens
 * [2 * batch][3] and resp [2 * batch][tr_max][resp_stride]; `batch` counts logical utterances, draw may be NULL.  Refusals as for
 * d3pm_op_nar_draw and as d3pm_nar_level_guided lists them. */
int d3pm_op_nar_draw_guided(int dtype, const void *logits, int ldl, const int32_t *lens, int32_t *resp, int tr_max, int resp_stride,
                            int t_max, int n_tokens, int level, float temperature, uint64_t seed, uint32_t utt0, uint32_t flags,
                            int batch, const d3pm_nar_draw *draw, const d3pm_guidance *guidance, void *stream);
int d3pm_op_layernorm(int dtype, const void *X, void *Y, const void *w, const void *b, const void *film,
                      int M, int d, float eps, void *stream);
/* Row-panel projection (d_model = 512): a Linear whose output is added to the residual stream, together with the LayerNorm(s)
 * the block applies to the new rows next, in ONE launch -- a workgroup owns whole rows (96 x 512 tiles), so the row moments
 * are reduced on chip.  Three forms, each bit-identical to the launches it replaces (d3pm_op_linear, then d3pm_op_layernorm):
 *   self-attention out-projection  (ar_discrete.py:132-136): X2 = film = row_mask = NULL, both LayerNorms:
 *       Y = rn(R1 + rn(X W^T + bias)),  ln_y = norm2(Y),  ln2_y = norm22(Y);
 *   both cross-attention out-projections (:138-143, the SAME weights): X2 given, film given, ln2_* = row_mask = NULL:
 *       Y = rn(rn(R1 + rn(X W^T + bias)) + rn(X2 W^T + bias)),  ln_y = FiLM(norm3(Y))  (:145-156);
 *   MLP down-projection (:159-161): row_mask given, X2 = film = ln2_* = NULL:
 *       Y = rn(R1 + rn(X W^T + bias)) * mask[row % mask_period],  ln_y = norm1 of the NEXT block (:131).
 * X (and X2) [M][ldx], W [512][K], Y / R1 / ln_y / ln2_y [M][512] (Y may alias R1), M a multiple of 96, K a multiple of 128.
 * fp8 fast path: with ln_sx (and ln2_sx) given -- first two forms only -- the LayerNorm rows leave in the block-scaled fp8
 * format (d3pm_op_quantize_mx of the 16-bit LayerNorm result, bit for bit): ln_y / ln2_y are then code buffers [M][512] bytes
 * and ln_sx / ln2_sx receive the scales [M][4][4].  D3PM_E_SHAPE for any other combination. */
int d3pm_op_linear_rowpanel(int dtype, const void *X, const void *X2, int ldx, const void *W, const void *bias, void *Y,
                            const void *R1, const uint8_t *row_mask, int mask_period, int M, int K, const void *ln_w,
                            const void *ln_b, void *ln_y, const void *ln2_w, const void *ln2_b, void *ln2_y,
                            const void *film, float eps, void *ln_sx, void *ln2_sx, void *stream);

/* Timing hooks for bench.py's roofline object.  A d3pm_prof attached to a tuning (d3pm_tuning.prof) makes every launch of the
 * kernel class `kclass` (D3PM_K_*; D3PM_K_COUNT = every class) made INSIDE d3pm_sample_loop with that tuning be bracketed by a
 * hipEvent pair on the launch stream -- in every 16th diffusion iteration only, so that the event pairs do not perturb the
 * timed region they measure; launches outside the loop (condition encoders, cond-K/V projections) are never bracketed.
 * d3pm_prof_read_class synchronises the events of one class and returns its launch count, total milliseconds and the
 * algorithmic flops / bytes of those launches; d3pm_prof_read returns the sums over the classes and resets.  A d3pm_prof is
 * owned by the caller (create / destroy) and must not be shared between threads that launch concurrently. */
/* D3PM_K_GEMM_LN: the launches that are a projection AND the LayerNorm(s) next to it (d3pm_op_linear_rowpanel) */
enum { D3PM_K_GEMM = 0, D3PM_K_ATTN = 1, D3PM_K_SAMPLE = 2, D3PM_K_LN = 3, D3PM_K_GEMM_LN = 4, D3PM_K_COUNT = 5 };
int d3pm_prof_create(int kclass, int max_events, struct d3pm_prof **out);
int d3pm_prof_read_class(struct d3pm_prof *prof, int kclass, int *launches, double *total_ms, double *flops, double *bytes);
int d3pm_prof_read(struct d3pm_prof *prof, int *launches, double *total_ms, double *flops, double *bytes);
int d3pm_prof_destroy(struct d3pm_prof *prof);

/* ---- Training side: gradients of the ops of AR.forward ------------------------------------------
 * The reference obtains them from autograd over ar_discrete.py:588-694 (DiT blocks :126-161, final Linear :776, masked
 * cross-entropy :683-690) inside engine.backward (utils/engines.py:144-147).  Here each is a single-op entry on fp32
 * tensors (the F32 precision mode); vall_e/vall_e/train.py replays the forward with a stash and walks it backwards.
 * All pointers are device pointers owned by the caller; nothing allocates or synchronises; 0 = ok.
 *
 * d3pm_op_matmul_f32      C[i][j] = beta C[i][j] + sum_k A[i sai + k sak] B[k sbk + j sbj]; rows of C whose row_mask entry
 *                         (row % mask_period) is 0 receive 0 (+ beta C).  dX = dY W and dW += dY^T X of every nn.Linear.
 * d3pm_op_colsum_f32      out[j] = beta out[j] + sum_i X[i][j]                              (bias gradients)
 * d3pm_op_act_bwd_f32     dU = dM act'(U), act = 1 exact-erf GELU (nn.GELU, :123), 2 ReLU, 3 SiLU (condition encoders)
 * d3pm_op_mask_rows_f32   X[i][:] = 0 where mask[i % period] == 0                           (x * mask, :128,161)
 * d3pm_op_layernorm_bwd_f32  LayerNorm (+ FiLM out = y (1 + film[c]) + film[d + c], :145-156) backward of one [M][d] block:
 *                         dX (overwritten or accumulated), dw / db / dfilm accumulated (fp32 atomics)
 * d3pm_op_attention_bwd_f32  softmax(scale q k^T) v backward (nn.MultiheadAttention core, :132,138,142): dQ overwritten,
 *                         dK / dV = beta_kv * old + new; stats = 2 B H Tq floats of scratch
 * d3pm_op_ce_bwd_f32      dlogits = mask (softmax(logits mask) - onehot(target)) gscale    (:683-690)
 * d3pm_op_embed_f32 / d3pm_op_embed_bwd_f32  nn.Embedding gather with the row mask, and its scatter-add (padding_idx row skipped)
 *
 * Dropout of the two condition encoders in train mode (ar_discrete.py:216-230: nn.TransformerEncoderLayer dropout 0.1 at four
 * sites per layer, timm Mlp drop 0.01 at two), from a counter-based mask that the backward pass regenerates (nothing stored):
 *   Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (idx >> 2, utt, site, 3), word idx & 3,
 *   u = (word >> 8) 2^-24, keep <=> u >= p, kept value x s with s = 1.0f / (1.0f - p) in fp32, dropped value 0;
 *   site = (which << 8) | (layer << 4) | kind  (which 0 text encoder, 1 prompt encoder; layer 0 .. cond_layers - 1 with kind
 *   0 attention probabilities, 1 after self-attn out_proj, 2 FFN hidden after ReLU, 3 after linear2; layer 15 = the Mlp with
 *   kind 0 after SiLU, 1 after fc2);  idx = r cols + c of an [rows][cols] activation (logical, independent of the row stride),
 *   (h Tq + i) S + j of the attention probabilities.  0 <= p < 1 (else D3PM_E_ARG); an extent whose idx would not fit in 32 bits
 *   is refused (D3PM_E_SHAPE).
 * d3pm_op_dropout_f32     Y = (R ? R + X z : X z), z = keep ? s : 0, over [M][N] (row strides ldx / ldr / ldy >= N; Y may be X with
 *                         ldy = ldx).  The backward pass of a site is the same call on the gradient.
 * d3pm_op_attention_dropout_f32  d3pm_op_attention (generic family, fp32) with every normalised probability multiplied by
 *                         z(h, i, j) before P V; utterance b draws with utt = utt0 + b
 * d3pm_op_attention_bwd_dropout_f32  d3pm_op_attention_bwd_f32 of that forward (O = (P o Z) V); Tq, S <= 4096
 *
 * Key-padding masks in the training step (forward_backward(mask_padding=True)).  key_len is a device int32 [B] with
 * 1 <= key_len[b] <= S, the caller's contract as in d3pm_op_attention_keylen (the values are read by the kernels only), or NULL =
 * unmasked.  S stays the padded key count: the row count of the K / V / dK / dV batches and the S of the mask index (h Tq + i) S + j,
 * so masking changes no draw of any other key.
 * d3pm_op_attention_dropout_keylen_f32  d3pm_op_attention_dropout_f32 with the mask: a key j >= key_len[b] is outside the softmax
 *                         (probability exactly 0), no factor is drawn for it and its K / V rows are not read; every query row is
 *                         written.  p = 0 is d3pm_op_attention_keylen on the generic fp32 family.
 * d3pm_op_attention_bwd_keylen_f32  the backward pass of d3pm_op_attention_keylen (generic family, fp32; p = 0, nothing drawn) or of
 *                         d3pm_op_attention_dropout_keylen_f32 (p > 0; Tq, S <= 4096 and the 32-bit mask index as above).  A masked
 *                         key reads nothing -- not its K / V rows, not Q / dO / stats, no dropout factor -- and its rows of dK / dV
 *                         receive exactly 0 (beta_kv = 0) or beta_kv * old, as the live rows' old contents are scaled; dQ and
 *                         stats are written for every query row from the live keys alone.  key_len = NULL with p = 0 runs the
 *                         kernels of d3pm_op_attention_bwd_f32, with p > 0 those of d3pm_op_attention_bwd_dropout_f32. */
/* The condition-side embeddings as a single op (ar_discrete.py:736-741): which = 0 text rows W[tok] + pe0 (`tables` [n_classes][d],
 * `pe` [d]); which = 1 prompt rows sum_l W[l][tok_l] + pe[s] (`tokens` [rows][n_levels], -1 = level absent; `tables`
 * [n_levels][n_classes][d]; `pe` [s_prompt][d]).  Used by the training step, which needs the encoder inputs it stashes. */
int d3pm_op_cond_embed(int dtype, int which, const int32_t *tokens, int n_levels, const void *tables, const void *pe, void *y, int rows,
                       int s_prompt, int d, int n_classes, void *stream);
int d3pm_op_matmul_f32(const float *A, long sai, long sak, const float *B, long sbk, long sbj, float *C, int ldc, int M, int N, int K,
                       float beta, const uint8_t *row_mask, int mask_period, void *stream);
int d3pm_op_colsum_f32(const float *X, int ldx, int M, int N, float *out, float beta, void *stream);
int d3pm_op_act_bwd_f32(const float *U, const float *dM, float *dU, size_t n, int act, void *stream);
int d3pm_op_mask_rows_f32(float *X, int ldx, int M, int N, const uint8_t *mask, int period, void *stream);
int d3pm_op_layernorm_bwd_f32(const float *X, const float *dOut, const float *w, const float *b, const float *film, float eps, int M,
                              int d, float *dX, int accumulate_dx, float *dw, float *db, float *dfilm, void *stream);
int d3pm_op_attention_bwd_f32(const float *Q, int ldq, const float *K, const float *V, int ldkv, const float *dO, int ldo, float *dQ,
                              int lddq, float *dK, float *dV, int lddkv, float *stats, int B, int Tq, int S, int H, int hd, float scale,
                              float beta_kv, void *stream);
int d3pm_op_ce_bwd_f32(const float *logits, int ldl, const int32_t *targets, const uint8_t *frame_mask, int canvas, int rows, int K,
                       float gscale, float *dlogits, int ldd, void *stream);
int d3pm_op_embed_f32(const int32_t *tok, const uint8_t *mask, int period, const float *table, float *Y, int rows, int d, int n_classes,
                      void *stream);
int d3pm_op_embed_bwd_f32(const int32_t *tok, const uint8_t *mask, int period, const float *dY, float *dTable, int rows, int d,
                          int n_classes, int padding_idx, void *stream);
int d3pm_op_dropout_f32(const float *X, int ldx, const float *R, int ldr, float *Y, int ldy, int M, int N, float p, uint64_t seed,
                        uint32_t utt, uint32_t site, void *stream);
int d3pm_op_attention_dropout_f32(const float *Q, int ldq, const float *K, const float *V, int ldkv, float *O, int ldo, int B, int Tq,
                                  int S, int H, int hd, float scale, float p, uint64_t seed, uint32_t utt0, uint32_t site, void *stream);
int d3pm_op_attention_bwd_dropout_f32(const float *Q, int ldq, const float *K, const float *V, int ldkv, const float *dO, int ldo,
                                      float *dQ, int lddq, float *dK, float *dV, int lddkv, float *stats, int B, int Tq, int S, int H,
                                      int hd, float scale, float beta_kv, float p, uint64_t seed, uint32_t utt0, uint32_t site,
                                      void *stream);
int d3pm_op_attention_dropout_keylen_f32(const float *Q, int ldq, const float *K, const float *V, int ldkv, float *O, int ldo, int B,
                                         int Tq, int S, int H, int hd, float scale, const int32_t *key_len, float p, uint64_t seed,
                                         uint32_t utt0, uint32_t site, void *stream);
int d3pm_op_attention_bwd_keylen_f32(const float *Q, int ldq, const float *K, const float *V, int ldkv, const float *dO, int ldo,
                                     float *dQ, int lddq, float *dK, float *dV, int lddkv, float *stats, int B, int Tq, int S, int H,
                                     int hd, float scale, float beta_kv, const int32_t *key_len, float p, uint64_t seed,
                                     uint32_t utt0, uint32_t site, void *stream);

/* ---- NAR training step: the three ops of the stock NAR model's backward pass that the entries above do not cover ----------
 * The reference trains the NAR with autograd over the training branch of NAR.forward (vall_e/vall_e/nar.py:53-74: a quantizer
 * level l_b per utterance, response levels 0 .. l_b in, level l_b + 1 the target) and Base.forward (base.py:403-488).  The host side
 * (vall_e/vall_e/nar_train.py) runs the forward through d3pm_op_nar_embed / d3pm_op_adaln / d3pm_op_linear /
 * d3pm_op_attention_keylen on fp32 tensors with a stash and walks it backwards through d3pm_op_matmul_f32, d3pm_op_colsum_f32,
 * d3pm_op_act_bwd_f32, d3pm_op_mask_rows_f32, d3pm_op_attention_bwd_keylen_f32 and these three.  Device pointers owned by the
 * caller, fp32, nothing allocates or synchronises; 0 = ok.  Refused with nothing launched: a NULL pointer or a size that is not
 * positive (D3PM_E_ARG), and what each entry names below.
 *
 * d3pm_op_adaln_bwd_f32      the backward pass of d3pm_op_adaln on fp32 rows (AdaLN.forward, base.py:145-158):
 *                         y = exp(lg) (f h) + beta, h = LayerNorm(x, eps 1e-5) without affine, f = c (1 - k h) with k = 0.1, c = 2, and
 *                         f a CONSTANT of the backward pass -- upstream writes `(self.k * h).detach()` (:154).  x, dy, dx [M][d] dense,
 *                         emb_row [2d] = (lg | beta) of one level, row_mask uint8 [M].  For a row with row_mask != 0:
 *                           dbeta += dy;  dlg += dy exp(lg) f h;  dh = dy exp(lg) f;
 *                           dx = r (dh - mean(dh) - h mean(dh h)),  r = 1 / sqrt(var + eps)   (added to dx when accumulate != 0);
 *                         a row with row_mask == 0 contributes nothing, neither x nor dy of it is read, and its dx row is 0 (left as
 *                         it was when accumulate != 0).  demb_row [2d] = (dlg | dbeta) is accumulated into (the caller zeroes it
 *                         or hands in the gradient row itself); each element has one writer that adds the rows in a fixed order,
 *                         so the sums are the same bits from run to run.  Any d > 0.
 * d3pm_op_nar_embed_bwd_f32  the backward pass of d3pm_op_nar_embed on fp32 tables (base.py:427-435; MultiEmbedding :244-274): the
 *                         index arrays and sizes of that entry, dx [batch][t_max][d]; each row below its utterance's total adds
 *                         its dx row to the rows that produced it -- d_text [n_tokens][d], d_prom [n_prom_levels][n_tokens][d] (a code
 *                         < 0 = level absent, skipped), d_resp [>= n_given][n_tokens][d] (levels 0 .. n_given - 1 only; the others are
 *                         not touched), d_sep [d] from the two separator rows of every utterance.  Rows at or past the total are not
 *                         read; the sinusoid table has no gradient.  An id outside [0, n_tokens - 1] is outside the contract: the
 *                         forward clamps it, here it adds nowhere, and no memory is written through it.  All four gradients are
 *                         accumulated into; a table row that several tokens share (inside an utterance or across the batch) has
 *                         one writer that adds their dx rows in grid order, so the result is the same bits from run to run.
 *                         1 <= n_given <= resp_stride; max(n_prom_levels, n_given) <= 65535, else D3PM_E_SHAPE.
 * d3pm_op_nar_ce_f32         F.cross_entropy over the response rows (base.py:445-488, resp_loss_only) per grid row: logits
 *                         [batch][t_max][ldl], ldl >= n_tokens; levels int32 [batch] on the device, 0 <= levels[b] <= resp_stride - 2
 *                         (the caller's contract; the column read is clamped into the row).  Frame f < t_response of utterance b is
 *                         grid row t_text + t_prompt + 2 + f (a row outside the grid does not exist) with target
 *                         resp[b][f][levels[b] + 1] (clamped into [0, n_tokens - 1]):
 *                           row_loss = logsumexp(logits) - logits[target],  dlogits = (softmax(logits) - onehot(target)) gscale;
 *                         every other row -- text, separators, prompt, padding -- gets row_loss 0 and an all-zero dlogits row.
 *                         row_loss [batch][t_max]; dlogits [batch][t_max][ldd], ldd >= n_tokens, or NULL = the loss alone.
 *                         The step's loss is sum(row_loss) / N and gscale = 1 / N, N the response frames of the call. */
int d3pm_op_adaln_bwd_f32(const float *x, const float *dy, const float *emb_row, const uint8_t *row_mask, int M, int d, float *dx,
                          int accumulate, float *demb_row, void *stream);
int d3pm_op_nar_embed_bwd_f32(const int32_t *lens, const int32_t *text, int tt_max, const int32_t *prom, int tp_max, int n_prom_levels,
                              const int32_t *resp, int tr_max, int resp_stride, int n_given, const float *dx, float *d_text,
                              float *d_prom, float *d_resp, float *d_sep, int batch, int t_max, int d, int n_tokens, void *stream);
int d3pm_op_nar_ce_f32(const float *logits, int ldl, const int32_t *lens, const int32_t *resp, int tr_max, int resp_stride,
                       const int32_t *levels, int batch, int t_max, int n_tokens, float gscale, float *row_loss, float *dlogits, int ldd,
                       void *stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* D3PM_HIP_H */
