// d3pm_kernels.h -- host-side launchers of the denoiser kernels (internal to the library).
// Two families implement the same contracts:
//   generic  (d3pm_generic.hip)  any shape, f32/f16/bf16, fp32 FMA arithmetic -- parity mode,
//                                MFMA-hostile shapes (head_dim 2 of the upstream model), cross-check
//   mfma     (d3pm_mfma_*.hip)   f16/bf16, LDS-tiled MFMA 16x16x32, shapes that tile by 128/64
#pragma once
#include "d3pm_common.h"

namespace d3pm {

enum { ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2, ACT_SILU = 3 };

// Schedule choices travel with the arguments of a launch (include/d3pm_hip.h: d3pm_tuning); nullptr = the defaults.
// The library has no mutable global state: the defaults are a constant.
inline const d3pm_tuning& tune_of(const d3pm_tuning* t) {
  static const d3pm_tuning kDefault = {/*gemm_variant*/ 0, /*gemm_persist_slots*/ 1024, /*lat_tile*/ 0, /*attn_query_groups*/ 0,
                                       /*attn_pair_sequential*/ 1, /*attn_cross_resident*/ 1, /*row_panel*/ 10, /*workspace_alias*/ 1,
                                       /*regime_batch*/ 0, /*ln_fold*/ 1, /*prof*/ nullptr};
  return t ? *t : kDefault;
}

// Y[M][N] = epilogue(X[M][K] . W[N][K]^T + bias)      (torch.nn.functional.linear layout)
// epilogue, with rn() = round to the storage dtype exactly where the eager reference rounds:
//   v = rn(acc + bias); if act: v = rn(act(v))   (exact-erf GELU, ReLU or SiLU);
//   if R1 && R2: v = rn(rn(R1 + R2) + v)  else if R1: v = rn(R1 + v);
//   if row_mask: v = v * row_mask[row % mask_period]
struct LinearArgs {
  const void* X = nullptr; int ldx = 0;
  const void* W = nullptr;
  const void* bias = nullptr;
  void* Y = nullptr; int ldy = 0;
  const void* R1 = nullptr; const void* R2 = nullptr; int ldr = 0;
  const uint8_t* row_mask = nullptr; int mask_period = 1;
  int M = 0, N = 0, K = 0;
  int act = ACT_NONE;
  const d3pm_tuning* tune = nullptr;
  // LayerNorm folded into this projection (MFMA family only, d3pm_mfma_tile.h): X = the raw residual rows [M][K = d_model], W = W o gamma,
  // `bias` unused; v = rn(rstd_r (acc - mean_r fold_s[n]) + fold_b[n]) [then act] with the row moments from stats_in [M][K / 32][2]
  const float* fold_s = nullptr; const float* fold_b = nullptr; const float* stats_in = nullptr; float fold_eps = 1e-6f;
  // moments of the rows this launch stores (N = d_model, after residual / mask): stats_out [M][N / 32][2] partial (sum, sum of squares)
  float* stats_out = nullptr;
  // stats_in / stats_out in the quad format [M / 16][d / 128][16][2] (d3pm_mfma_tile.h EpiFold) instead of 32-column parts: d_model = 512,
  // big-tile GEMM only (LIN_QUADS_REFUSED, d3pm_plan.h: mfma_linear fails with D3PM_E_SHAPE on any other family); one host decision per folded sequence (fold_plan, d3pm_sequence.h)
  bool moment_quads = false;
  // optional live row count in device memory (row deduplication, d3pm_dedup.hip): only the tiles that hold a row < *m_live run; M stays
  // the capacity the plan was made for.  Big-tile family, gemm_mfma_128_glds and gemm_mfma_panel64 (mfma_linear refuses it elsewhere).
  const int* m_live = nullptr;
  // host-side estimate of *m_live (d3pm_plan.h plan_live_rows), 0 = none: the planner chooses the family and sizes the grid of
  // gemm_mfma_panel64 for min(M, m_est) rows.  It only chooses speed: the kernel walks every live tile whatever the grid.  Without
  // an estimate a launch plans for the capacity, as it did before the field existed.
  int m_est = 0;
  // a second host-side estimate of *m_live for the launches that stay on big tiles (d3pm_plan.h plan_distinct_rows; set on the
  // projections onto the residual stream), 0 = none: where the capacity takes 192 x 128 tiles, big_tile gives a producer with quads
  // the 96- or 128-row tile while the tiles of rows_est rows fit two per CU in one round.  Speed only, as m_est: the kernel walks every live tile
  // of whichever geometry, and all of them give the same bits.
  int rows_est = 0;
};
// which LayerNorm-fold combinations the MFMA epilogues instantiate: LNF [+ GELU] without residual / mask; STATS with R1, R1 + R2, R1 + mask
inline bool fold_args_ok(const LinearArgs& a) {
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) % 16) == 0; };
  if (a.fold_s) {
    if (!a.fold_b || !a.stats_in || a.R1 || a.row_mask || a.stats_out || (a.act != ACT_NONE && a.act != ACT_GELU)) return false;
    if (a.K % 256 != 0 || a.N % 4 != 0 || !al16(a.fold_s) || !al16(a.fold_b) || !al16(a.stats_in)) return false;
  } else if (a.fold_b || a.stats_in) {
    return false;
  }
  if (a.stats_out) {
    if (!a.R1 || a.act != ACT_NONE || a.N % 32 != 0 || (reinterpret_cast<uintptr_t>(a.stats_out) % 8) != 0) return false;
  }
  if (a.moment_quads) {
    if (!a.fold_s && !a.stats_out) return false;
    if ((a.fold_s && a.K != 512) || (a.stats_out && a.N != 512)) return false;
  }
  return true;
}

// O[b][i][h*hd+c] = sum_j P[i][j] V[b][j][h*hd+c],  P = rn(softmax(rn(rn(q*scale) . k)))
// element (b, row, h, c) of Q lives at Q + (b*Tq+row)*ldq + h*hd + c; K/V likewise with S, ldkv.
struct AttnArgs {
  const void* Q = nullptr; int ldq = 0;
  const void* K = nullptr; const void* V = nullptr; int ldkv = 0;
  void* O = nullptr; int ldo = 0;
  int B = 0, Tq = 0, S = 0, H = 0, hd = 0;
  float scale = 1.f;
  // optional per-utterance number of valid keys (device int32[B]): keys >= key_len[b] are masked out
  // (the key-padding mask of the stock NAR attention, base.py:118-124); S is then the padded key count
  const int32_t* key_len = nullptr;
  // optional second, independent problem with the same B / Tq / H / hd launched in the same grid
  // (the text and prompt cross-attentions of one DiT block): its own Q, K/V (S2 keys) and output
  const void* Q2 = nullptr; const void* K2 = nullptr; const void* V2 = nullptr; void* O2 = nullptr; int S2 = 0;
  // the same mask for the second problem (device int32[B], 1 .. S2); key_len then belongs to the first problem alone
  const int32_t* key_len2 = nullptr;
  // set by the denoiser's launch sequence (d3pm_sequence.h with_frame_keys, d3pm_keys): a masked self-attention takes the automatic choice of the unmasked one,
  // so switching the mask on does not switch the instruction shape.  Unset, a masked call with attn_query_groups = 0 keeps the
  // 16 x 16 x 32 kernel it has always had (the stock NAR stage, d3pm_op_attention_keylen).
  bool masked_keeps_schedule = false;
  // optional query segments (device int32 [B] each; row deduplication, attn32p_hd64 and attn32_cross_hd64 only): the queries and the
  // output rows of utterance b are the seg_len[b] rows (any count in 1 .. Tq) from row seg_start[b] (any row) of Q / O: a query behind
  // its segment reads the segment's last row and stores nothing; keys stay [B][S]
  const int32_t* seg_start = nullptr; const int32_t* seg_len = nullptr;
  // optional key gather (device int32 [B][S]; attn32p_hd64 with query segments only): key j of utterance b is row key_row[b * S + j]
  // of K / V, which are then [kv_rows][ldkv] with no per-utterance base; the kernel clamps the index into [0, kv_rows - 1];
  // kv_rows * ldkv * the element size < 2^32
  const int32_t* key_row = nullptr; int kv_rows = 0;
  // optional key pool (with key_row; attn32p_hd64 POOL): seg_est = the rows per utterance the host expects (0 = none; it only chooses
  // speed).  Within attn_pool_rows() the workgroup of an utterance whose seg_len[b] fits the pool copies the K | V columns of its head
  // into LDS once -- pool row r = row pool_src[seg_start[b] + r] of K / V (null: row seg_start[b] + r), clamped into [0, kv_rows - 1] --
  // and key j is pool row seg_key[b * S + j] - seg_start[b], clamped into [0, seg_len[b] - 1]; any other workgroup of the launch walks
  // key_row as without a pool.  The caller's promise: the row named through key_row and the one named through seg_key / pool_src hold
  // the same bytes.  pool_rows / qblocks_grid (d3pm_op_attention_gather_pool): the pool's rows and the query blocks per (utterance,
  // head) in the grid, named by the caller instead of derived from seg_est
  int seg_est = 0;
  const int32_t* seg_key = nullptr; const int32_t* pool_src = nullptr;
  int pool_rows = 0, qblocks_grid = 0;
  const d3pm_tuning* tune = nullptr;
};

// Y = LN(X) * w + b (eps), optionally FiLM: Y = rn(rn(LN * rn(1 + film[c])) + film[d + c])
// second output (w2/b2/Y2) optional: a second LayerNorm of the same rows (norm2 + norm22).
struct LayerNormArgs {
  const void* X = nullptr; void* Y = nullptr;
  const void* w = nullptr; const void* b = nullptr;
  const void* w2 = nullptr; const void* b2 = nullptr; void* Y2 = nullptr;
  const void* film = nullptr;
  int M = 0, d = 0; float eps = 1e-6f;
  // optional gather in front (the first block's norm1 directly on the token embedding, ar_discrete.py:753,127,131): row m of the
  // input is table[tokens[m]] (zeros where frame_mask[m % mask_period] == 0) with X = the table; the gathered rows also go to Xout.
  // mask_period: canvas for a mask the utterances share, batch * canvas for a per-utterance one (d3pm_canvas)
  const int32_t* tokens = nullptr; const uint8_t* frame_mask = nullptr; int mask_period = 0, n_classes = 0; void* Xout = nullptr;
};

// what the row-panel projection (d3pm_mfma_gemm_big.hip) does to the rows it has just finished: N = d_model = 512
struct RowPanelFuse {
  const void* X2 = nullptr;                                  // second operand through the same weights (dual out-projection)
  const void* lnw = nullptr; const void* lnb = nullptr; void* lny = nullptr;        // LayerNorm of the new rows
  const void* lnw2 = nullptr; const void* lnb2 = nullptr; void* lny2 = nullptr;     // a second LayerNorm of the same rows
  const void* film = nullptr;                                // FiLM (scale | shift, 2 x 512) on the first
  float eps = 1e-6f;
  // fp8 fast path: with sx (and sx2) set, lny (lny2) receive the LayerNorm rows in the block-scaled fp8 format of d3pm_mx.hip --
  // codes [M][512] bytes -- and sx (sx2) their scales [M][4][4]
  void* sx = nullptr; void* sx2 = nullptr;
};

struct EmbedArgs {
  const int32_t* tokens = nullptr; const uint8_t* frame_mask = nullptr; int mask_period = 0;      // frame_mask[row % mask_period]
  const void* table = nullptr; void* Y = nullptr; int M = 0, d = 0, n_classes = 0;
  int n_q = 1;      // > 1: tokens [M][n_q], table [n_q][n_classes][d], row = rn(sum over the levels) (d3pm_shape.n_q)
  // embed_tokens_stats, n_q = 1 only: all or none -- also q0[row] [M][d] | kv0[row] [M][2d] = row (live ? id : n_classes) of the
  // block-0 QKV table [.][3d]
  const void* qkv_table = nullptr; void* q0 = nullptr; void* kv0 = nullptr;
};
// rows of the block-0 QKV table [rows][3d] (d3pm_api.hip build_qkv_table): one per id, the zero row of a padded frame at n_classes,
// then zero rows up to a multiple of both GEMM tile heights (192 and 128)
inline int qkv_table_rows(int n_classes) { return (n_classes + 1 + 383) / 384 * 384; }

// per-step scalars of the closed-form posterior (host-built from d3pm_schedule)
struct PosteriorConsts {
  float log_f1_zero;   // log16(rn16(0 + eps))
  float log_f1_d;      // log16(rn16(d_t + eps))      x_t != M, j == x_t
  float log_f1_c;      // log16(rn16(c_t + eps))      x_t == M, j != M
  float log_f1_one;    // log16(rn16(1 + eps))        x_t == M, j == M
  float dbar_prev;     // dbar_{t-1}
  float cbar_prev;     // cbar_{t-1}
  int t;
};

struct SampleArgs {
  const void* logits = nullptr; int logits_dtype = D3PM_F16; int ldl = 0;
  const int32_t* x_t = nullptr; int32_t* x_next = nullptr; int32_t* x_next2 = nullptr;
  uint16_t* posterior_out = nullptr;
  int rows = 0, n_classes = 0, mask_id = 0, canvas = 0;
  uint64_t seed = 0; uint32_t row0 = 0; int greedy = 0;
  const uint64_t* seed_hbm = nullptr;   // when set, the kernel reads the seed from HBM (lets a captured HIP graph be replayed with a new seed)
  int n_q = 1;      // > 1: row r = (frame row r / n_q, level r % n_q); Philox row = row0 + frame row, stream = level ? 16 + level : 0
  // known frames (d3pm_canvas.known, uint8 [frame rows]) or nullptr: a marked frame keeps x_t (all its levels) and draws nothing
  const uint8_t* known = nullptr;
  // d3pm_sampling, validated by the entry point: z' = rn16(z / temperature), then everything below the top_k-th largest z' becomes
  // -inf (0 = no cut).  The neutral pair launches the kernels without the filter arm.
  float temperature = 1.0f; int top_k = 0;
  bool filtered() const { return temperature != 1.0f || top_k != 0; }
  // d3pm_nucleus: behind them, everything below the nucleus threshold theta of z'' becomes -inf (top_p 1 = no cut); theta_out is the
  // step entry's optional device float [rows] (theta per row, NaN for a known row).  Either one takes the kernels' nucleus arm.
  float top_p = 1.0f; float* theta_out = nullptr;
  bool nucleus() const { return top_p < 1.0f || theta_out != nullptr; }
  // d3pm_guidance: `logits` holds 2 * rows rows (row rows + r = row r under the null condition) and the routine runs on
  // rn16(fmaf(guidance, c - u, c)); x_t / x_next / known stay `rows` long.  posterior_sample_guided / posterior_sample_prep_guided only.
  bool guided = false; float guidance = 0.f;
  PosteriorConsts pc{};
};

int generic_linear(int dtype, const LinearArgs& a, hipStream_t s);
int generic_attention(int dtype, const AttnArgs& a, hipStream_t s);
// probability dropout of a training-step attention (d3pm_common.h dropout_z): utterance b draws with utt = utt0 + b, s = 1 / (1 - p)
struct DropoutArgs {
  float p = 0.f, s = 1.f;
  uint64_t seed = 0;
  uint32_t utt0 = 0, site = 0;
};
// the fp32 generic attention with sc = rn(e / sum) * z(h, i, j) before P.V (training step; Q2 unsupported).  a.key_len as in
// generic_attention: a masked key is outside the softmax, draws no factor and its K / V rows are not read; z keeps its index
// (h Tq + i) S + j with the padded S
int generic_attention_dropout_f32(const AttnArgs& a, const DropoutArgs& dr, hipStream_t s);
int generic_layernorm(int dtype, const LayerNormArgs& a, hipStream_t s);
int embed_tokens(int dtype, const EmbedArgs& a, hipStream_t s);
// condition-side embeddings: text rows = rn(W[tok] + pe0); prompt rows = rn(rn(sum_l W[l][tok_l]) + pe[s])
// key_len (device int32 [rows / s_text] or [rows / s_prompt], or null): the rows of an utterance behind its length are padding --
// text id 0, prompt every level absent -- and their ids are not read (d3pm_keys.text / .prompt)
// head_dim hd -> 2 hd re-layout around an attention call (d3pm_headpad.hip): [rows][groups][hd] <-> [rows][groups][2 hd], zeros above
int pad_heads(const void* in, void* out, long long rows, int groups, int hd, hipStream_t s);
int unpad_heads(const void* in, void* out, long long rows, int groups, int hd, hipStream_t s);
int cond_embed_text(int dtype, const int32_t* tok, const void* table, const void* pe0, void* y, int rows, int s_text, int d,
                    int n_classes, const int32_t* key_len, hipStream_t s);
int cond_embed_prompt(int dtype, const int32_t* codes, int n_levels, const void* tables, const void* pe, void* y,
                      int rows, int s_prompt, int d, int n_classes, const int32_t* key_len, hipStream_t s);
int posterior_sample(const SampleArgs& a, hipStream_t s);
// What the sampler launch of iteration t can prepare for iteration t - 1 (folded-LayerNorm path, n_q = 1; d3pm_sample.hip): the
// embedding row of every id it has just drawn + the row's moments (ar_discrete.py:753,127), and -- in workgroups behind the
// sampler's -- fc1 of every block under norm3 + FiLM(t - 1) (:145-159).  Two launches less per iteration, same bits.
struct NextIterPrep {
  int dtype = D3PM_BF16;
  const void* table = nullptr; void* x = nullptr; float* stats = nullptr; const uint8_t* frame_mask = nullptr; int d = 0;
  int mask_period = 0;                                                                              // frame_mask[row % mask_period]
  bool quads = false;                                                                               // stats in the quad format
  const d3pm_block_weights* blocks = nullptr; int n_layers = 0; const void* film_t = nullptr;      // film_t: the FiLM table's row of the next evaluation's timestep (t - 1; the reveal loop: t_{i+1})
  void* Wf = nullptr; float* s_out = nullptr; float* b_out = nullptr;
  // optional, all or none: the block-0 QKV table and the [rows][d] | [rows][2d] regions that receive each drawn row's projection
  // (EmbedArgs).  posterior_sample_prep only: the guided and the reveal launches ignore them, and their loops keep the projection.
  const void* qkv_table = nullptr; void* q0 = nullptr; void* kv0 = nullptr;
};
bool posterior_sample_prep_supported(const SampleArgs& a, const NextIterPrep& n);
int posterior_sample_prep(const SampleArgs& a, const NextIterPrep& n, hipStream_t s);
// the two launches under classifier-free guidance (SampleArgs.guided; kernels of their own: an unguided call runs none of their code).
// The prep form embeds rows r and rows + r of n.x / n.stats and applies wherever posterior_sample_prep_supported(a, n) holds.
int posterior_sample_guided(const SampleArgs& a, hipStream_t s);

// ---- row deduplication (d3pm_dedup.hip): one compact row per distinct (id | padded) class of an utterance -------------------------
// The denoiser adds no positional term, so two frames of one utterance with the same id get the same logits bit for bit; every
// projection and every attention query runs on the compact rows, only the keys and the sampler stay per canvas position.
struct DedupIndex {      // all device memory, [n = batch * canvas] unless noted; carved from the workspace (d3pm_sequence.cpp)
  int32_t* cnt = nullptr;         // [batch] distinct classes of an utterance
  int32_t* seg_start = nullptr;   // [batch] first compact row of an utterance: the exclusive prefix sum of seg_len
  int32_t* seg_len = nullptr;     // [batch] cnt rounded up to DedupArgs::seg_align (1: cnt itself, no zero row inside a segment)
  int32_t* m_live = nullptr;      // [1] sum of seg_len (seg_align = 1: the distinct classes of the batch)
  int32_t* row_of = nullptr;      // canvas position -> compact row
  int32_t* key_cls = nullptr;     // class of a canvas position (n_classes on a padded frame) = its row of the block-0 QKV table; null: not written
  int32_t* rep_pos = nullptr;     // [batch][canvas]: position of the k-th representative (first occurrences in position order)
  int32_t* cid = nullptr;         // class of a compact row (n_classes = padded / unused)
  uint8_t* cmask = nullptr;       // frame-mask byte of a compact row (0 on unused rows)
};
struct DedupArgs {
  const int32_t* tokens = nullptr; const uint8_t* frame_mask = nullptr; int mask_period = 0;
  int batch = 0, canvas = 0, n_classes = 0, d = 0;
  DedupIndex ix;
  // rows of a segment: 1 = the count itself (dense, the loop's: every kernel that reads segments takes any length at any row), or 128 =
  // whole 128-query self-attention workgroups (the layout d3pm_op_dedup_index has always written)
  int seg_align = 128;
  // the compact embedding (all or none): table [n_classes][d]; x [n][d] + moments; block-0 q rows of the compact rows (q0 [n][d]) from
  // qkv_table [.][3d] (its k | v rows are read in place, through ix.key_cls); zero [2] = buffers [n][d] whose rows m_live .. the next
  // multiple of 384 are cleared (attention outputs: no attention workgroup writes them, the out-projections' last tile reads them)
  const void* table = nullptr; void* x = nullptr; float* stats = nullptr; bool quads = false;
  const void* qkv_table = nullptr; void* q0 = nullptr;
  void* zero[2] = {nullptr, nullptr};
};
constexpr int kDedupMaxClasses = 4095;      // classes + the padded one fit the index kernel's LDS table
constexpr int kDedupMaxBatch = 12 * 1024 - 5;      // the embedding launch's prefix of the counts (batch + 1 ints) and four wave sums fit 48 KiB of LDS
int dedup_index(int dtype, const DedupArgs& a, hipStream_t s);      // two launches: per-utterance index, then segments + embedding
// the sampler launch of the deduplicated loop: row r reads logits[row_of[r]]; with n.Wf set, the workgroups behind the sampler's fold
// fc1 of every block for the next timestep (NextIterPrep; nothing is embedded here)
int posterior_sample_dedup(const SampleArgs& a, const int32_t* row_of, const NextIterPrep& n, hipStream_t s);
int posterior_sample_prep_guided(const SampleArgs& a, const NextIterPrep& n, hipStream_t s);

// One step of the confidence-ordered reveal (d3pm_reveal, d3pm_reveal.hip; n_q = 1): reveal_candidates scores the masked free rows at
// timestep t into cand / score, then reveal_commit (one wave per utterance) or reveal_commit_prep (one wave per row + NextIterPrep
// with film_t = the row of the NEXT timestep of the plan; x_next != x_t) picks the step's rows and stores x_next.
// revise (d3pm_revise; the kRevise = true instantiations of the same kernels, which no call without it launches): reveal_candidates
// writes cand / score of every FREE row (a held row: its own id, and logprob of that id + hold_bonus + the order noise); the commits
// leave F - floor(F keep_frac) free rows with an id, may store mask_id, and reset logprob / step on the rows they re-mask.
struct RevealArgs {
  const void* logits = nullptr; int logits_dtype = D3PM_F16; int ldl = 0;
  const int32_t* x_t = nullptr; int32_t* x_next = nullptr; int32_t* x_next2 = nullptr;
  const uint8_t* frame_mask = nullptr; int mask_period = 0;      // frame_mask[row % mask_period]
  const uint8_t* known = nullptr;                                // [rows] or nullptr
  int32_t* cand = nullptr; float* score = nullptr;               // [rows]: written for masked free rows only (revise: for every free row)
  int rows = 0, canvas = 0, n_classes = 0, mask_id = 0;
  uint64_t seed = 0; uint32_t row0 = 0; int greedy = 0;
  int t = 0;                  // timestep of the evaluation: keys the uniforms
  float lambda = 0.f;         // choice_temperature * float(cbar[t_next]); 0 on the last step
  float keep_frac = 0.f;      // float(cbar[t_next]); 0 on the last step
  float temperature = 1.0f; int top_k = 0; float top_p = 1.0f;
  bool revise = false; float hold_bonus = 0.f;
  float* logprob = nullptr; int32_t* step = nullptr;             // revise: the grids of d3pm_frame_scores ([rows]), both or neither
  bool filtered() const { return temperature != 1.0f || top_k != 0 || top_p < 1.0f; }
};
int reveal_candidates(const RevealArgs& a, hipStream_t s);
int reveal_commit(const RevealArgs& a, hipStream_t s);
bool reveal_commit_prep_supported(const RevealArgs& a, const NextIterPrep& n);
int reveal_commit_prep(const RevealArgs& a, const NextIterPrep& n, hipStream_t s);

// ---- per-frame log-probability of the revealed id (d3pm_frame_scores, d3pm_logprob.hip; n_q = 1) -------------------------------------
// frame_scores_init: step = (live && !known && x == mask_id) ? 0 : -1, logprob = 0 over [rows].  frame_logprob, the launch behind a
// sampler launch: a row with step 0 whose x_next is no longer the mask id gets logprob = log-softmax over the codec ids of its logits
// at x_next and step = t; every other row is left as it is.
struct LogprobArgs {
  const void* logits = nullptr; int logits_dtype = D3PM_F16; int ldl = 0;
  const int32_t* row_of = nullptr;               // [rows] or nullptr: row r reads logits[row_of[r]] (clamped into the rows; 16-bit, unguided)
  bool guided = false; float guidance = 0.f;     // logits holds 2 * rows rows, z = rn16(fmaf(guidance, c - u, c)) (SampleArgs.guided)
  const int32_t* x_next = nullptr;               // [rows]: the grid the sampler launch has just written
  float* logprob = nullptr; int32_t* step = nullptr;      // [rows]
  int rows = 0, n_classes = 0, mask_id = 0, t = 0;
};
int frame_scores_init(const int32_t* x, const uint8_t* frame_mask, int mask_period, const uint8_t* known, float* logprob, int32_t* step, int rows,
                      int mask_id, hipStream_t s);
int frame_logprob(const LogprobArgs& a, hipStream_t s);

// fp8 fast path on the block-scaled MFMA (d3pm_mx.hip): e4m3 codes [rows][K] + e8m0 block scales [rows][4][K / 128]
//   Y[M][N] = epilogue(sum_k X8 2^sx . W8 2^sw + bias), epilogue as LinearArgs (plain, GELU, R1, R1 + mask); with Y8 / SY set the
//   output is written in the MX format itself (codes [M][N] + scales [M][4][N / 128]: the next projection's operand) instead of Y
struct MxLinearArgs {
  const void* X8 = nullptr; int ldx = 0; const void* SX = nullptr;
  const void* W8 = nullptr; const void* SW = nullptr;
  const void* bias = nullptr;
  void* Y = nullptr; int ldy = 0;
  const void* R1 = nullptr; int ldr = 0;
  const uint8_t* row_mask = nullptr; int mask_period = 1;
  void* Y8 = nullptr; void* SY = nullptr;
  int M = 0, N = 0, K = 0;
  int act = ACT_NONE;
  const d3pm_tuning* tune = nullptr;
};
bool mx_linear_supported(int dtype, const MxLinearArgs& a);
int mx_linear(int dtype, const MxLinearArgs& a, hipStream_t s);
int layernorm_mx(int dtype, const void* x, uint8_t* y8, uint8_t* sx, const void* w, const void* b, const void* film,
                 const void* w2, const void* b2, uint8_t* y8_2, uint8_t* sx_2, int M, int d, float eps, hipStream_t s);
int quantize_mx(int dtype, const void* x, int ldx, uint8_t* y8, uint8_t* sx, int M, int K, hipStream_t s);

// MFMA family.  Which kernel runs, on which grid, is a plan (d3pm_plan.h: plan_linear / plan_cross_out / plan_attention, host-only);
// the launchers instantiate what the plan names.  mfma_linear and mfma_attention take any plan with mfma() and forward to the others.
struct LinearPlan;
struct AttnPlan;
int mfma_linear(int dtype, const LinearArgs& a, const LinearPlan& p, hipStream_t s);
int big_linear(int dtype, const LinearArgs& a, const LinearPlan& p, hipStream_t s);             // d3pm_mfma_gemm_big.hip
int panel64_linear(int dtype, const LinearArgs& a, const LinearPlan& p, hipStream_t s);         // d3pm_mfma_gemm_lat.hip
int mfma_attention(int dtype, const AttnArgs& a, const AttnPlan& p, hipStream_t s);
int mfma_attention32(int dtype, const AttnArgs& a, const AttnPlan& p, hipStream_t s);           // d3pm_mfma_attn32.hip: self-attention on the 32 x 32 x 16 instruction
int mfma_attention32_cross(int dtype, const AttnArgs& a, const AttnPlan& p, hipStream_t s);     // the resident cross-attention pair on the same instruction
// d3pm_mfma_attn_lat.hip: the key tiles of a 32-query group split over the four waves of a workgroup
int mfma_attention_split(int dtype, const AttnArgs& a, const AttnPlan& p, hipStream_t s);
// two products through one weight panel or tile, Y = rn(rn(R1 + rn(X W^T + b)) + rn(X2 W^T + b)); `p` = CrossOutPlan::dual:
// the latency GEMM (d3pm_mfma_gemm_lat.hip) and the big-tile GEMM at throughput batch sizes (d3pm_mfma_gemm_big.hip; stats_out optional)
int panel64_dual(int dtype, const LinearArgs& a, const void* X2, const LinearPlan& p, hipStream_t s);
int big_dual(int dtype, const LinearArgs& a, const void* X2, const LinearPlan& p, hipStream_t s);
bool row_panel_supported(int dtype, const LinearArgs& a, const RowPanelFuse& f);
int row_panel_linear(int dtype, const LinearArgs& a, const RowPanelFuse& f, hipStream_t s);
bool fast_layernorm_supported(int dtype, const LayerNormArgs& a);
int fast_layernorm(int dtype, const LayerNormArgs& a, hipStream_t s);

PosteriorConsts make_posterior_consts(const d3pm_schedule* sched, int t);

// LayerNorm folded into the projections (d3pm_fold.hip): weight preparation and the non-GEMM producers of row moments
int fold_rows_launch(int dtype, const void* W, const void* bias, const void* gamma, const void* beta, const void* film, long film_ld,
                     int n_rows, int n_t, int K, void* Wf, float* s_out, float* b_out, hipStream_t s);
int fold_fc1_step_launch(int dtype, const d3pm_block_weights* blocks, int n_layers, const void* film_t, int d, void* Wf, float* s_out,
                         float* b_out, hipStream_t s);
// quads: the moments in the quad format of d3pm_mfma_tile.h (EpiFold; d = 512) instead of 32-column parts
int row_stats_launch(int dtype, const void* x, int ldx, int M, int d, float* stats, hipStream_t s, bool quads = false);
int embed_tokens_stats(int dtype, const EmbedArgs& a, float* stats, bool quads, hipStream_t s);
// the inputs of the block-0 QKV table: x [rows][d] = the embedding row of id `row` (zeros from n_classes on) and its moments (parts)
int qkv_table_rows_launch(int dtype, const void* table, void* x, float* stats, int rows, int d, int n_classes, hipStream_t s);

// ---- stock NAR model (levels 1..7): input assembly, AdaLN, temperature sampling (d3pm_nar.hip) ----
struct NarEmbedArgs {
  const int32_t* lens = nullptr;                 // [B][3] = (t_text, t_prompt, t_response)
  const int32_t* text = nullptr; int tt_max = 0;  // [B][tt_max]
  const int32_t* prom = nullptr; int tp_max = 0; int n_prom_levels = 8;   // [B][tp_max][n_prom_levels], -1 = level absent
  const int32_t* resp = nullptr; int tr_max = 0; int resp_stride = 8; int n_given = 1;   // [B][tr_max][resp_stride]
  const void *w_text = nullptr, *w_prom = nullptr, *w_resp = nullptr, *sep = nullptr, *pe = nullptr;
  void* x = nullptr; uint8_t* row_mask = nullptr; int32_t* key_len = nullptr;
  int batch = 0, t_max = 0, d = 0, n_tokens = 0;
};
int nar_embed(int dtype, const NarEmbedArgs& a, hipStream_t s);
int adaln(int dtype, const void* x, void* y, const void* emb_row, const uint8_t* row_mask, int M, int d, hipStream_t s);
int nar_sample(int dtype, const void* logits, int ldl, const int32_t* lens, int32_t* resp, int tr_max, int resp_stride,
               int t_max, int n_tokens, int level, float temperature, uint64_t seed, uint32_t utt0, int greedy, int batch,
               hipStream_t s);
// the same draw with options (d3pm_nar_draw.hip; d3pm_nar_draw of include/d3pm_hip.h, validated by the caller): n_tokens <= 1280
struct NarDrawArgs {
  float top_p = 1.0f;
  int top_k = 0;
  const uint8_t* known = nullptr;      // [B][tr_max], != 0: the frame keeps the id it holds
  float* logprob_out = nullptr;        // [B][tr_max][resp_stride - 1]
  float* theta_out = nullptr;          // [B][tr_max]; non-NULL takes the nucleus arm
};
// guidance non-NULL = the guided arm with that weight: logits / lens / resp hold 2 * batch utterances (batch + b the null twin of b), the
// frame's row is rn<T>(fmaf(w, c - u, c)) and the id goes to both halves of resp; d's arrays stay [batch]...
int nar_draw(int dtype, const void* logits, int ldl, const int32_t* lens, int32_t* resp, int tr_max, int resp_stride, int t_max,
             int n_tokens, int level, float temperature, uint64_t seed, uint32_t utt0, int greedy, int batch, const NarDrawArgs& d,
             hipStream_t s, const float* guidance = nullptr);

}  // namespace d3pm
