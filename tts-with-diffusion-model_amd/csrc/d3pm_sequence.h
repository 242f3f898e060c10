// d3pm_sequence.h -- the launch sequence of a denoiser evaluation and the plan of a sampler loop, as host-only code: the workspace
// carve-up, the argument builders, the launches of one folded block written once (folded_block) with the planners that walk them, and
// the decisions a call takes once before it loops (fold_plan, loop_plan).  The rule is the one of d3pm_plan.h: no kernel, no <<<>>>,
// no HIP runtime call here or in d3pm_sequence.cpp, so a test on a machine without a GPU links them and walks the real description
// (tests/test_launch_plan_api.py).  Everything that enqueues -- the visitor that launches a block included -- is d3pm_api.hip.
#pragma once
#include <cmath>

#include "d3pm_plan.h"

namespace d3pm {

float host_h2f(uint16_t h);      // d3pm_schedule.cpp

#define D3PM_TRY(expr)            \
  do {                            \
    int rc_ = (expr);             \
    if (rc_ != D3PM_OK) return rc_; \
  } while (0)

// which model shapes have folded-LayerNorm tables at all (d3pm_fold.hip builds them)
inline bool fold_shape_ok(int dtype, int d) { return (dtype == D3PM_F16 || dtype == D3PM_BF16) && d >= 256 && d % 256 == 0; }

// ---- workspace carve-up ----------------------------------------------------------------------
struct Workspace {
  char *x, *h, *h2, *qkv, *att, *att2, *mlp, *logits;
  float* stats;       // [n][d / 32][2] row moments of the residual stream (LayerNorm folded into the projections, d3pm_mfma_tile.h)
  char* fc1f;         // [L][4d][d] fc1 under norm3 + FiLM(t), rebuilt per evaluation (d3pm_fold.hip); then fp32 [L][4d] s and b'
  float *fc1f_s, *fc1f_b;
  // block-0 QKV from a per-id table (build_qkv_table; folded path, n_q = 1): the table's input rows [qkv_table_rows][d], their moments
  // (parts), the table [qkv_table_rows][3d], and the q rows [n][d] and k | v rows [n][2d] of block 0 of the next evaluation
  char *tab_x, *tab_qkv, *q0, *kv0;
  float* tab_stats;
  uint8_t* mxs;       // fp8 fast path: block scales [2n][d / 32] of the LayerNorm rows (a slot of their own: nothing else ever lives here)
  // row deduplication (d3pm_dedup.hip; never together with fp8): its index arrays live in the mxs slot, all null when they do not fit
  DedupIndex dd;
  size_t total;
};
inline size_t align256(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }
// internal logits rows are padded to a multiple of 8 elements (16-B aligned rows for vector stores/loads)
inline int logits_ld(const d3pm_shape& sh) { return (sh.n_classes + 7) & ~7; }
// quantizer levels generated jointly (d3pm_shape.n_q; 0 and 1 = the upstream level-0 path)
inline int levels(const d3pm_shape& sh) { return sh.n_q > 1 ? sh.n_q : 1; }
Workspace carve(const d3pm_shape& sh, int batch, char* base);      // base null: the sizes alone

inline const char* at(const void* p, size_t elems, size_t es) { return static_cast<const char*>(p) + elems * es; }
inline char* at(void* p, size_t elems, size_t es) { return static_cast<char*>(p) + elems * es; }

// ---- argument builders: the shapes the launch sequences repeat -----------------------------------------------------
// Y[M][N] = X[M][K] . W[N][K]^T + bias over packed rows (ldx = K, ldy = N); a caller with a wider output row sets ldy afterwards
inline LinearArgs projection(const void* X, const void* W, const void* bias, void* Y, int M, int N, int K, int act = ACT_NONE) {
  LinearArgs g;
  g.X = X; g.ldx = K; g.W = W; g.bias = bias; g.Y = Y; g.ldy = N; g.M = M; g.N = N; g.K = K; g.act = act;
  return g;
}
// ... + R1 (+ R2): rows of the output's width
inline LinearArgs with_residual(LinearArgs g, const void* R1, const void* R2 = nullptr) {
  g.R1 = R1; g.R2 = R2; g.ldr = g.N;
  return g;
}
// ... * row_mask[row % period]
inline LinearArgs with_row_mask(LinearArgs g, const uint8_t* mask, int period) {
  g.row_mask = mask; g.mask_period = period;
  return g;
}
// ... leaving the moments of the rows it stores (a producer of the folded LayerNorm, d3pm_mfma_tile.h EPI_STATS)
inline LinearArgs with_moments_out(LinearArgs g, float* stats, bool quads) {
  g.stats_out = stats; g.moment_quads = quads;
  return g;
}
// a LayerNorm-fed projection of the raw residual rows X [M][K] (a consumer, EPI_LNF): Wf = W o gamma, no bias operand
inline LinearArgs folded_projection(const void* X, const void* Wf, const float* fold_s, const float* fold_b, const float* stats, bool quads,
                                    void* Y, int M, int N, int K, int act) {
  LinearArgs g = projection(X, Wf, nullptr, Y, M, N, K, act);
  g.fold_s = fold_s; g.fold_b = fold_b; g.stats_in = stats; g.moment_quads = quads;
  return g;
}
inline float attn_scale(int hd) { return static_cast<float>(std::sqrt(1.0 / static_cast<double>(hd))); }
// self-attention over a packed [B * T][3 H hd] buffer of q | k | v rows
inline AttnArgs self_attention(const void* qkv, void* O, int B, int T, int H, int hd, size_t es) {
  const int d = H * hd;
  AttnArgs a;
  a.Q = qkv; a.ldq = 3 * d; a.K = at(qkv, d, es); a.V = at(qkv, 2 * d, es); a.ldkv = 3 * d; a.O = O; a.ldo = d;
  a.B = B; a.Tq = T; a.S = T; a.H = H; a.hd = hd; a.scale = attn_scale(hd);
  return a;
}
// the text | prompt cross-attentions of one block in one launch: queries with row stride ldq, keys and values packed [B * S][2 H hd]
inline AttnArgs cross_attention_pair(const void* q_text, const void* q_prompt, int ldq, const void* kv_text, int s_text, const void* kv_prompt,
                                     int s_prompt, void* o_text, void* o_prompt, int B, int T, int H, int hd, size_t es) {
  const int d = H * hd;
  AttnArgs a;
  a.Q = q_text; a.ldq = ldq; a.K = kv_text; a.V = at(kv_text, d, es); a.ldkv = 2 * d; a.O = o_text; a.ldo = d;
  a.B = B; a.Tq = T; a.S = s_text; a.H = H; a.hd = hd; a.scale = attn_scale(hd);
  a.Q2 = q_prompt; a.K2 = kv_prompt; a.V2 = at(kv_prompt, d, es); a.O2 = o_prompt; a.S2 = s_prompt;
  return a;
}
inline EmbedArgs embed_args(const d3pm_shape& sh, const d3pm_weights& w, int batch, const int32_t* x_t, const uint8_t* frame_mask, int mask_period,
                            void* Y) {
  EmbedArgs e;
  e.tokens = x_t; e.frame_mask = frame_mask; e.mask_period = mask_period; e.table = w.resps_emb; e.Y = Y;
  e.M = batch * sh.canvas; e.d = sh.d_model; e.n_classes = sh.n_classes; e.n_q = levels(sh);
  return e;
}

// The frame mask of a call and the period it repeats with over the packed [batch * canvas] rows: one mask [canvas] shared by every
// utterance (period canvas: d3pm_denoise_step, d3pm_sample_loop) or one per utterance [batch][canvas] (period batch * canvas: the
// *_canvas entries).  `known` is the known-frame map of d3pm_canvas ([batch][canvas] or null), read by the sampler only.
struct CanvasMask {
  const uint8_t* frame_mask; int period; const uint8_t* known;
};
inline CanvasMask shared_mask(const d3pm_shape* sh, const uint8_t* frame_mask) { return CanvasMask{frame_mask, sh ? sh->canvas : 0, nullptr}; }
inline CanvasMask per_utterance_mask(const d3pm_shape* sh, int batch, const d3pm_canvas* cv, bool with_known) {
  if (!cv || !sh) return CanvasMask{nullptr, 0, nullptr};
  return CanvasMask{cv->frame_mask, batch * sh->canvas, with_known ? cv->known : nullptr};
}

// d3pm_keys of a call (all null without one): the key counts of the self-attention and of the two cross-attentions
struct KeyCounts {
  const int32_t *frames = nullptr, *text = nullptr, *prompt = nullptr;
};
inline KeyCounts key_counts(const d3pm_keys* k) { return k ? KeyCounts{k->frames, k->text, k->prompt} : KeyCounts{}; }
// a masked self-attention of the denoiser: the schedule of the unmasked one
inline AttnArgs with_frame_keys(AttnArgs a, const KeyCounts& kc) {
  a.key_len = kc.frames; a.masked_keeps_schedule = kc.frames != nullptr;
  return a;
}
inline AttnArgs with_cond_keys(AttnArgs a, const KeyCounts& kc) {
  a.key_len = kc.text; a.key_len2 = kc.prompt;
  return a;
}

struct DenoiserArgs {      // what every block of one evaluation sees
  const d3pm_shape& sh; const d3pm_weights& w; int batch; const uint8_t* frame_mask; int mask_period; const void* kv_text; const void* kv_prompt;
  const Workspace& ws;
  KeyCounts keys = {};
  // classifier-free guidance (d3pm_sample_loop_guided): x_t holds token_rows = batch / 2 * canvas rows and rows token_rows .. of the
  // evaluation (the null twins) read the same ids; 0 = x_t has a row per row of the evaluation
  int token_rows = 0;
  // the block-0 QKV table of the call (ws.tab_qkv once build_qkv_table has filled it) or null: with it, an embedding launch of the
  // evaluation also gathers ws.q0 | ws.kv0
  const void* qkv_table = nullptr;
  // row deduplication (loop_plan decides, d3pm_dedup.hip): the index of this evaluation's compact rows, or null.  With it every
  // projection and attention query of the folded sequence runs on the compact rows (live count and segments read from device memory),
  // and the launch that prepares an evaluation is dedup_index.
  const DedupIndex* dd = nullptr;
  // with dd, per iteration: the host's estimate of the live rows (plan_live_rows) when the iteration takes the latency launch list --
  // every projection of a block on gemm_mfma_panel64, sized for the estimate, moments as parts -- or 0: the big-tile list, quads
  int m_est = 0;
  // with dd, per iteration: the rows per utterance the host expects (LoopPlan::seg_est), or 0.  With it the self-attention may pool an
  // utterance's K | V rows in LDS (AttnArgs::seg_est, plan_attention decides)
  int seg_est = 0;
  // with dd, per iteration that stays on the big-tile list: the distinct rows the host expects (LoopPlan::rows_est), or 0.  The
  // projections onto the residual stream carry it to big_tile (LinearArgs::rows_est), which sizes their tiles to it
  int rows_est = 0;
};

// ---- the block sequence with the LayerNorms folded into the projections (ar_discrete.py:126-161; d3pm_mfma_tile.h EPI_LNF / EPI_STATS)
//   embed (+ moments) -> n_layers x { QKV <- x [norm1 folded], self-attention, out-projection + x (+ moments),
//   merged query projection <- x [norm2 | norm22 folded, N = 2d], paired cross-attention, both out-projections + x (+ moments),
//   fc1 + GELU <- x [norm3 + FiLM(t) folded], fc2 + x, frame mask (+ moments) }: ten launches per block, none of them a LayerNorm.
// The launches of block l, written ONCE and handed to a visitor in order: FoldPlanner asks whether and on which tiles they would run,
// FoldLauncher (d3pm_api.hip) enqueues them.  Every LinearArgs that reads or writes ws.stats is constructed here and nowhere else.
// qkv_ready (block 0 only): ws.q0 | ws.kv0 already hold the q and k | v rows of ALL rows of this evaluation (gathered from the
// block-0 QKV table by the launch that embedded them), so the QKV projection is skipped and the self-attention reads them there.
template <class Visitor>
int folded_block(const DenoiserArgs& q, int l, bool quads, Visitor& v, bool qkv_ready = false) {
  const d3pm_shape& sh = q.sh;
  const Workspace& ws = q.ws;
  const int dt = sh.dtype, d = sh.d_model, H = sh.n_heads, hd = d / H, T = sh.canvas, n = q.batch * T;
  const size_t es = dtype_size(dt);
  const d3pm_block_weights& b = q.w.blocks[l];
  const d3pm_fold_block& f = q.w.fold[l];
  const int* m_live = q.dd ? q.dd->m_live : nullptr;
  auto consumer = [&](const void* Wf, const float* fs, const float* fb, void* Y, int N, int act) {
    LinearArgs g = folded_projection(ws.x, Wf, fs, fb, ws.stats, quads, Y, n, N, d, act);
    g.m_live = m_live; g.m_est = q.m_est;
    return v.linear(g);
  };
  auto segments = [&](AttnArgs a) {
    if (q.dd) { a.seg_start = q.dd->seg_start; a.seg_len = q.dd->seg_len; }
    return a;
  };
  // a projection onto the residual stream: x += X . W^T + bias (+ R2), then the moments of the new rows
  auto producer = [&](const void* X, int K, const void* W, const void* bias, const void* R2 = nullptr) {
    LinearArgs g = with_moments_out(with_residual(projection(X, W, bias, ws.x, n, d, K), ws.x, R2), ws.stats, quads);
    g.m_live = m_live; g.m_est = q.m_est; g.rows_est = q.rows_est;
    return g;
  };
  // ---- self-attention ----
  const bool from_table = l == 0 && qkv_ready;
  if (!from_table) D3PM_TRY(consumer(f.qkv_w, f.qkv_s, f.qkv_b, ws.qkv, 3 * d, ACT_NONE));
  AttnArgs sa = self_attention(ws.qkv, ws.att, q.batch, T, H, hd, es);
  if (from_table) { sa.Q = ws.q0; sa.ldq = d; sa.K = ws.kv0; sa.V = at(ws.kv0, d, es); sa.ldkv = 2 * d; }
  if (q.dd) {
    // the keys stay where they lie and the attention walks them through an index (attn32p_hd64 GATHER): the k | v columns of the compact
    // QKV rows through row_of, in block 0 those of the block-0 QKV table through the class of a canvas position (q: ws.q0, the compact copy)
    if (from_table) { sa.K = at(q.qkv_table, d, es); sa.V = at(q.qkv_table, 2 * d, es); sa.key_row = q.dd->key_cls; sa.kv_rows = qkv_table_rows(sh.n_classes); }
    else { sa.key_row = q.dd->row_of; sa.kv_rows = n; }
    sa.ldkv = 3 * d;
    // the pool names the same rows through the compact row of a position: row_of, and in block 0 the class of that compact row
    if (q.seg_est) { sa.seg_est = q.seg_est; sa.seg_key = q.dd->row_of; sa.pool_src = from_table ? q.dd->cid : nullptr; }
  }
  D3PM_TRY(v.attention(segments(with_frame_keys(sa, q.keys))));
  D3PM_TRY(v.linear(producer(ws.att, d, b.attn_out_w, b.attn_out_b)));
  // ---- cross-attention: q_text | q_prompt are the two halves of ONE [n][2d] projection of x (the same q rows under norm2 / norm22)
  D3PM_TRY(consumer(f.q2_w, f.q2_s, f.q2_b, ws.qkv, 2 * d, ACT_NONE));
  const void* kvt = at(q.kv_text, static_cast<size_t>(l) * q.batch * sh.s_text * 2 * d, es);
  const void* kvp = at(q.kv_prompt, static_cast<size_t>(l) * q.batch * sh.s_prompt * 2 * d, es);
  D3PM_TRY(v.attention(segments(with_cond_keys(cross_attention_pair(ws.qkv, at(ws.qkv, d, es), 2 * d, kvt, sh.s_text, kvp, sh.s_prompt, ws.att, ws.att2, q.batch, T, H, hd, es),
                                               q.keys))));
  // ---- x = (x + o_text) + o_prompt, rounded at each add like the eager sum ----
  LinearArgs g = producer(ws.att, d, b.cross_out_w, b.cross_out_b);
  g.tune = sh.tuning;      // plan_cross_out reads it
  const CrossOutPlan out = plan_cross_out(dt, g, ws.att2, false, true);
  if (out.form != CROSS_OUT_TWO_LAUNCHES) {
    D3PM_TRY(v.dual(out, g, ws.att2));
  } else {
    g.Y = ws.h; g.R1 = nullptr; g.stats_out = nullptr; g.moment_quads = false;   // o_text -> h (free: no LayerNorm output lives there any more)
    D3PM_TRY(v.linear(g));
    D3PM_TRY(v.linear(producer(ws.att2, d, b.cross_out_w, b.cross_out_b, ws.h)));
  }
  // ---- FiLM-modulated MLP: the (layer, t) copy of fc1 carries norm3 and the modulation ----
  const size_t ln = static_cast<size_t>(l) * 4 * d;
  D3PM_TRY(consumer(at(ws.fc1f, ln * d, es), ws.fc1f_s + ln, ws.fc1f_b + ln, ws.mlp, 4 * d, ACT_GELU));
  // (deduplicated: the mask byte of a compact row, period = the capacity)
  if (q.dd) return v.linear(with_row_mask(producer(ws.mlp, 4 * d, b.fc2_w, b.fc2_b), q.dd->cmask, n));
  return v.linear(with_row_mask(producer(ws.mlp, 4 * d, b.fc2_w, b.fc2_b), q.frame_mask, q.mask_period));
}

// asks: would every launch that touches the moments run on the MFMA family (D3PM_E_SHAPE if not), and all of them on big tiles?
struct FoldPlanner {
  int dt; const d3pm_tuning* tune; bool big;
  int linear(LinearArgs g) {
    if (!g.fold_s && !g.stats_out) return D3PM_OK;      // no moments: any family will do
    g.tune = tune;
    const LinearPlan plan = plan_linear(dt, g);
    if (!plan.mfma()) return D3PM_E_SHAPE;
    big = big && plan.big();
    return D3PM_OK;
  }
  int attention(const AttnArgs&) { return D3PM_OK; }
  int dual(const CrossOutPlan& c, const LinearArgs&, const void*) {
    big = big && c.dual.big();      // the 64 x 64 family keeps the 32-column parts
    return D3PM_OK;
  }
};
// asks: would the sequence run on the kernels that read a live row count and query segments from device memory -- every projection on
// `family` (big tiles; gemm_mfma_panel64 for the latency iterations, asked with DenoiserArgs::m_est set and the moments as parts), the
// self-attention on attn32p_hd64, the cross pair on attn32_cross_hd64?
struct DedupPlanner {
  int dt; const d3pm_tuning* tune; bool ok; int family = LIN_BIG;
  int linear(LinearArgs g) {
    g.tune = tune;
    ok = ok && plan_linear(dt, g).kernel == family;
    return D3PM_OK;
  }
  int attention(AttnArgs a) {
    a.tune = tune;
    const int k = plan_attention(dt, a).kernel;
    ok = ok && (a.Q2 ? k == ATTN_32_CROSS : (k == ATTN_32P || k == ATTN_32P_POOL));
    return D3PM_OK;
  }
  int dual(const CrossOutPlan& c, const LinearArgs&, const void*) {
    ok = ok && c.dual.kernel == family;
    return D3PM_OK;
  }
};

// Is this evaluation taking the folded-LayerNorm launch sequence, and in which format do its row moments travel?  FOLD_NONE: the
// LayerNorm launches (the fold is off, or a projection of the sequence would not run on the MFMA family, whose epilogues alone read
// and write moments).  FOLD_QUADS: every projection that reads or writes moments runs on big tiles (128-column aligned, d = 512), so
// the producers can leave one quad per 128 columns (d3pm_mfma_tile.h EpiFold).  FOLD_PARTS: 32-column parts, which the 128 x 128 and
// 64 x 64 (panel64, one or two utterances) families need.  One decision for the whole sequence -- every producer and consumer of
// ws.stats, the sampler's embedding rows included, must use the same format -- taken once per call over ALL layers (only_layers never
// changes the format).  The walk asks with the parts format and the sequence launches with the answer; at d = 512, the only width that
// gets quads, fold_args_ok accepts both formats for these arguments.
// The deduplicated loop alone refines the answer per ITERATION (LoopPlan::m_est): an iteration on the latency launch list runs its
// whole chain -- the index launch that prepares it included -- on parts, every other one on quads.  The consumers compute the same bits
// from either format, so the switch changes no id.
enum { FOLD_NONE = 0, FOLD_PARTS = 1, FOLD_QUADS = 2 };
int fold_plan(const DenoiserArgs& q, uint32_t flags, bool fp8);

// What a call decides once, before it enqueues anything: the moment format, and for a sampler loop which of the three things
// d3pm_tuning.ln_fold can switch on top of the fold (fold_features, d3pm_plan.h) it takes.  Asked with the DenoiserArgs of the
// evaluation -- for a guided loop the doubled batch, its regime_batch and token_rows -- before qkv_table and dd are set: they are its
// answers.
struct LoopCall {      // the defaults: one evaluation (d3pm_denoise_step), which folds and takes nothing else
  bool fp8 = false, guided = false, known = false;      // fp8 weights; classifier-free guidance; known frames (CanvasMask::known)
  int t_start = 1, t_stop = 0;                          // the iterations t_start .. t_stop + 1
};
struct LoopPlan {
  int fold = FOLD_NONE;      // fold_plan: the same for every iteration (the blocks and the sampler's prep share it) but a latency one
  bool table = false;        // build_qkv_table in front of the loop; DenoiserArgs::qkv_table = ws.tab_qkv
  bool dedup = false;        // DenoiserArgs::dd = &ws.dd
  bool latency = false;      // an iteration whose estimate is within live_latency_rows() takes the latency launch list
  int batch = 0, canvas = 0, t_stop = 0;
  // DenoiserArgs::m_est of iteration t: the estimate of its live rows, or 0 = the big-tile list.  A latency iteration's moments travel
  // as parts (its producers and consumers, and the index launch that prepared it), whatever `fold` says.
  int m_est(const d3pm_schedule* sched, int t) const {
    if (!latency || t <= t_stop) return 0;
    const int est = plan_live_rows(batch, canvas, host_h2f(sched->cbar[t]));
    return live_latency(est) ? est : 0;
  }
  // DenoiserArgs::seg_est of iteration t: the same estimate per utterance, rounded up.  It follows the `latency` switch (ln_fold = 4
  // keeps the gathered self-attention in every iteration) but not the bound of the GEMMs: plan_attention has its own.
  int seg_est(const d3pm_schedule* sched, int t) const {
    if (!latency || t <= t_stop || batch <= 0) return 0;
    return (plan_live_rows(batch, canvas, host_h2f(sched->cbar[t])) + batch - 1) / batch;
  }
  // DenoiserArgs::rows_est of iteration t: plan_distinct_rows, for every iteration of the deduplicated loop that does not take the
  // latency list (with ln_fold = 4 that is all of them), or 0.  Known frames are the caller's and cannot be counted: no estimate then.
  bool live_tiles = false;
  int n_classes = 0;
  int rows_est(const d3pm_schedule* sched, int t) const {
    if (!live_tiles || t <= t_stop || m_est(sched, t)) return 0;
    return plan_distinct_rows(batch, canvas, n_classes, host_h2f(sched->cbar[t]));
  }
};
LoopPlan loop_plan(const DenoiserArgs& q, uint32_t flags, const LoopCall& call);

}  // namespace d3pm
