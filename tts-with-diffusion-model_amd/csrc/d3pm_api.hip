// d3pm_api.hip -- extern "C" entry points (include/d3pm_hip.h) and everything that enqueues a launch.
//
// One denoiser evaluation = the loop body of AR.generate_audio (ar_discrete.py:752-776):
//   embed -> n_layers x { LN1, QKV GEMM, self-attention, out GEMM(+res), LN2/LN22, 2 x Q GEMM,
//   2 x cross-attention against the cached condition K/V, 2 x out GEMM(+res), LN3+FiLM,
//   fc1 GEMM(+GELU), fc2 GEMM(+res, *mask) } -> final GEMM -> posterior/sample.
// The workspace, the argument builders, the launches of a folded block (folded_block) and what a call decides before it loops
// (loop_plan) are host-only code in d3pm_sequence.{h,cpp}; which kernel a launch runs on is d3pm_plan.{h,cpp}.
// Nothing here allocates or synchronises; everything is enqueued on the caller's stream.
#include <cmath>
#include <new>
#include <vector>

#include "d3pm_sequence.h"

namespace d3pm {

int q_sample_launch(const d3pm_shape*, int, const int32_t*, int32_t*, const uint8_t*, int, const d3pm_schedule*,
                    uint64_t, uint32_t, hipStream_t);
int uniform_launch(uint64_t, int, uint32_t, int, int, int, float*, hipStream_t);
int ce_loss_launch(int, const void*, int, const int32_t*, const uint8_t*, int, int, int, float*, hipStream_t);

}  // namespace d3pm

// ---- profiling hooks (bench.py roofline object): a caller-owned handle, reached through d3pm_tuning.prof -----------------------
// Only launches made from inside d3pm_sample_loop are ever bracketed (sample_now is false outside it): the condition
// encoders and the cond-K/V projections run once per utterance and are not part of any class's per-launch figures.
struct d3pm_prof {
  int kclass = -1;                // D3PM_K_* one class, D3PM_K_COUNT every class
  std::vector<hipEvent_t> ev;     // pairs
  std::vector<int> cls;           // class of pair i
  int used = 0;
  double flops[D3PM_K_COUNT] = {}, bytes[D3PM_K_COUNT] = {};
  int stride = 16;       // only the iterations with t % stride == 0 are bracketed (event pairs cost ~3 us each: all launches 6 % of the step, every 8th 2.5 %)
  bool sample_now = false;
};

namespace d3pm {

// what a launch sequence carries besides its arguments: the caller's schedule choices and (optionally) its timing hooks
struct Ctx {
  const d3pm_tuning* tune;
  d3pm_prof* prof;
  explicit Ctx(const d3pm_tuning* t) : tune(t), prof(t ? t->prof : nullptr) {}
};

struct ProfScope {
  bool on;
  d3pm_prof* p;
  hipStream_t s;
  ProfScope(const Ctx& cx, int kclass, hipStream_t st, double flops, double bytes) : p(cx.prof), s(st) {
    on = p && (p->kclass == kclass || p->kclass == D3PM_K_COUNT) && p->sample_now && p->used + 2 <= static_cast<int>(p->ev.size());
    if (on) {
      (void)hipEventRecord(p->ev[p->used], s);
      p->cls[p->used / 2] = kclass;
      p->flops[kclass] += flops;
      p->bytes[kclass] += bytes;
    }
  }
  ~ProfScope() {
    if (on) {
      (void)hipEventRecord(p->ev[p->used + 1], s);
      p->used += 2;
    }
  }
};

// ---- kernel-family dispatch: the planner (d3pm_plan.cpp) names the kernel; "generic" is its answer like any other -----------------
static bool forced_generic(uint32_t flags) { return (flags & D3PM_FLAG_FORCE_GENERIC) != 0; }
static int run_linear(const Ctx& cx, int dtype, LinearArgs a, uint32_t flags, hipStream_t s) {
  const size_t es = dtype_size(dtype);
  a.tune = cx.tune;
  ProfScope p(cx, D3PM_K_GEMM, s, 2.0 * a.M * a.N * a.K,
              es * (static_cast<double>(a.M) * a.K + static_cast<double>(a.N) * a.K +
                    static_cast<double>(a.M) * a.N * (1 + (a.R1 ? 1 : 0) + (a.R2 ? 1 : 0))));
  const LinearPlan plan = plan_linear(dtype, a, forced_generic(flags));
  if (plan.mfma()) return mfma_linear(dtype, a, plan, s);
  // the generic family has no folded-LayerNorm epilogues: it would ignore the moments (read stale ones, or leave them unwritten)
  D3PM_REQUIRE(!a.fold_s && !a.stats_out && !a.moment_quads, D3PM_E_SHAPE, "folded-LayerNorm projection %d x %d x %d needs the MFMA family",
               a.M, a.N, a.K);
  return generic_linear(dtype, a, s);
}
// projection onto the residual stream + the LayerNorm(s) of the new rows, one launch (d3pm_mfma_gemm_big.hip)
static int run_row_panel(const Ctx& cx, int dtype, const LinearArgs& a, const RowPanelFuse& f, hipStream_t s) {
  const size_t es = dtype_size(dtype);
  const double prods = f.X2 ? 2.0 : 1.0, mn = static_cast<double>(a.M) * a.N;
  ProfScope p(cx, D3PM_K_GEMM_LN, s, prods * 2.0 * a.M * a.N * a.K,
              es * (prods * a.M * a.K + static_cast<double>(a.N) * a.K + mn * (3.0 + (f.lny2 ? 1.0 : 0.0))));
  return row_panel_linear(dtype, a, f, s);
}
static int run_attention(const Ctx& cx, int dtype, AttnArgs a, uint32_t flags, hipStream_t s) {
  a.tune = cx.tune;
  // algorithmic bytes: queries in + outputs out (of BOTH problems of a paired launch: rounds 1-3 counted one, which made the
  // pair look like 1.3x wasted traffic -- PMC says 118.8 MB against 118.6) + keys and values
  ProfScope p(cx, D3PM_K_ATTN, s, 4.0 * a.B * a.H * a.Tq * static_cast<double>(a.S + a.S2) * a.hd,
              dtype_size(dtype) * ((a.Q2 ? 4.0 : 2.0) * a.B * a.Tq * a.H * a.hd + 2.0 * a.B * (a.S + a.S2) * a.H * a.hd));
  const AttnPlan plan = plan_attention(dtype, a, forced_generic(flags));
  // query segments exist in two kernels only: any other choice would read Q at b * Tq and ignore them
  const bool self32p = plan.kernel == ATTN_32P || plan.kernel == ATTN_32P_POOL;
  D3PM_REQUIRE(!a.seg_len || self32p || plan.kernel == ATTN_32_CROSS, D3PM_E_SHAPE,
               "query segments: the planner names attention kernel %d, which does not take them", plan.kernel);
  // ... and a key index in one: attn32p_hd64 with segments
  D3PM_REQUIRE(!a.key_row || (self32p && a.seg_len && !a.Q2), D3PM_E_SHAPE,
               "gathered keys: the planner names attention kernel %d, or the call has no query segments", plan.kernel);
  if (plan.mfma()) return mfma_attention(dtype, a, plan, s);
  if (a.Q2) {   // the generic kernel takes one problem per launch
    AttnArgs first = a, second = a;
    first.Q2 = first.K2 = first.V2 = nullptr; first.O2 = nullptr; first.S2 = 0; first.key_len2 = nullptr;
    second = first;
    second.Q = a.Q2; second.K = a.K2; second.V = a.V2; second.O = a.O2; second.S = a.S2; second.key_len = a.key_len2;
    int rc = generic_attention(dtype, first, s);
    return rc != D3PM_OK ? rc : generic_attention(dtype, second, s);
  }
  return generic_attention(dtype, a, s);
}
static int run_layernorm(const Ctx& cx, int dtype, const LayerNormArgs& a, uint32_t flags, hipStream_t s) {
  ProfScope p(cx, D3PM_K_LN, s, 0.0, dtype_size(dtype) * static_cast<double>(a.M) * a.d * (a.Y2 ? 3.0 : 2.0));
  if (!(flags & D3PM_FLAG_FORCE_GENERIC) && fast_layernorm_supported(dtype, a)) return fast_layernorm(dtype, a, s);
  return generic_layernorm(dtype, a, s);
}

static int check_shape(const d3pm_shape* sh, int batch) {
  D3PM_REQUIRE(sh, D3PM_E_ARG, "null shape");
  D3PM_REQUIRE(batch > 0 && sh->d_model > 0 && sh->n_heads > 0 && sh->d_model % sh->n_heads == 0 && sh->n_layers > 0 &&
                   sh->canvas > 0 && sh->s_text > 0 && sh->s_prompt > 0 && sh->n_classes > 1 && sh->mask_id >= 0 &&
                   sh->mask_id < sh->n_classes && sh->timesteps >= 2 && sh->n_q >= 0 && sh->n_q <= 16,
               D3PM_E_ARG, "inconsistent d3pm_shape");
  D3PM_REQUIRE(sh->dtype == D3PM_F32 || sh->dtype == D3PM_F16 || sh->dtype == D3PM_BF16, D3PM_E_ARG, "bad dtype %d",
               sh->dtype);
  return D3PM_OK;
}

// ---- the cross-attention out-projection pair: x = (x + o_text) + o_prompt through the same weights (plan_cross_out, d3pm_plan.h) ----
static int run_cross_out_dual(const Ctx& cx, int dt, const CrossOutPlan& c, const LinearArgs& g, const void* X2, hipStream_t s) {
  ProfScope p(cx, D3PM_K_GEMM, s, 2.0 * 2.0 * g.M * g.N * g.K,
              dtype_size(dt) * (2.0 * g.M * g.K + static_cast<double>(g.N) * g.K + 2.0 * g.M * g.N));
  return c.form == CROSS_OUT_PANEL64_DUAL ? panel64_dual(dt, g, X2, c.dual, s) : big_dual(dt, g, X2, c.dual, s);
}

// the token embedding of an evaluation whose two halves read the same x_t (token_rows > 0): the gather, once per half
static int embed_twins(const DenoiserArgs& q, const int32_t* x_t, hipStream_t s) {
  const d3pm_shape& sh = q.sh;
  EmbedArgs e = embed_args(sh, q.w, q.batch / 2, x_t, q.frame_mask, q.mask_period, q.ws.x);
  const int rc = embed_tokens(sh.dtype, e, s);
  if (rc != D3PM_OK) return rc;
  e.Y = at(q.ws.x, static_cast<size_t>(q.token_rows) * sh.d_model, dtype_size(sh.dtype));
  return embed_tokens(sh.dtype, e, s);
}

struct FoldLauncher {
  const Ctx& cx; int dt; hipStream_t s;
  int linear(const LinearArgs& g) { return run_linear(cx, dt, g, 0, s); }      // (fails rather than take the generic family with moments)
  int attention(const AttnArgs& a) { return run_attention(cx, dt, a, 0, s); }
  int dual(const CrossOutPlan& c, const LinearArgs& g, const void* X2) { return run_cross_out_dual(cx, dt, c, g, X2, s); }
};

// The block-0 QKV table of a reverse process.  Block 0 reads x[row] = resps_emb[id] (zeros on a padded frame): no positional term, no
// time term and no FiLM enters before norm1, so its QKV projection takes at most n_classes + 1 distinct values, which depend on the
// weights alone.  They are computed once per call -- the folded projection itself over the n_classes embedding rows and the zero row,
// whose inputs embed_row_stats writes as it does for canvas rows, so the bits are those of the launch this replaces (every GEMM family
// accumulates in the same order, d3pm_mfma_gemm.hip; the moments travel as parts, which every family reads) -- and the launches that
// embed a row copy its 3d values into ws.q0 | ws.kv0 instead of the loop projecting all rows again at every iteration.
static int build_qkv_table(const Ctx& cx, const d3pm_shape& sh, const d3pm_weights& w, const Workspace& ws, hipStream_t s) {
  const int dt = sh.dtype, d = sh.d_model, mt = qkv_table_rows(sh.n_classes);
  D3PM_TRY(qkv_table_rows_launch(dt, w.resps_emb, ws.tab_x, ws.tab_stats, mt, d, sh.n_classes, s));
  const d3pm_fold_block& f = w.fold[0];
  return run_linear(cx, dt, folded_projection(ws.tab_x, f.qkv_w, f.qkv_s, f.qkv_b, ws.tab_stats, false, ws.tab_qkv, mt, 3 * d, d, ACT_NONE), 0, s);
}

// the index of an evaluation's compact rows + their embedding, moments and block-0 q (two launches, d3pm_dedup.hip)
static int run_dedup_index(const DenoiserArgs& q, const int32_t* x_t, bool quads, hipStream_t s) {
  const d3pm_shape& sh = q.sh;
  const Ctx cx(sh.tuning);
  // (algorithmic bytes at the capacity: the x and q0 rows written)
  ProfScope p(cx, D3PM_K_LN, s, 0.0, dtype_size(sh.dtype) * static_cast<double>(q.batch) * sh.canvas * sh.d_model * 2.0);
  DedupArgs a;
  a.tokens = x_t; a.frame_mask = q.frame_mask; a.mask_period = q.mask_period; a.batch = q.batch; a.canvas = sh.canvas; a.n_classes = sh.n_classes;
  a.d = sh.d_model; a.ix = *q.dd; a.table = q.w.resps_emb; a.x = q.ws.x; a.stats = q.ws.stats; a.quads = quads;
  // (no k | v row is gathered: the self-attention reads the table through key_cls.  att2 is h2 under workspace_alias, which nothing else of
  // this sequence writes any more, so both attention outputs are cleared behind the live rows)
  a.qkv_table = q.qkv_table; a.q0 = q.ws.q0; a.zero[0] = q.ws.att; a.zero[1] = q.ws.att2;
  // dense segments: every launch of the iteration costs in proportion to the live rows, and none of them needs a segment to be whole
  // 128-row workgroups (attn32p_hd64 SEG clamps its query rows and predicates its stores like the cross pair)
  a.seg_align = 1;
  return dedup_index(sh.dtype, a, s);
}

static int denoiser_blocks_folded(const DenoiserArgs& q, const int32_t* x_t, int t, const void* film, int layers, hipStream_t s, bool prepared,
                                  bool quads, bool qkv_ready) {
  const d3pm_shape& sh = q.sh;
  const int dt = sh.dtype, d = sh.d_model, n = q.batch * sh.canvas;
  const Ctx cx(sh.tuning);
  const size_t es = dtype_size(dt);
  if (!prepared) {      // (inside the loop the previous iteration's sampler launch has done both: posterior_sample_prep)
    {
      ProfScope p(cx, D3PM_K_LN, s, 0.0, es * static_cast<double>(n) * d * 2.0);
      qkv_ready = false;
      if (q.token_rows) {      // the first evaluation of a guided loop: both halves from the same ids, then the moments of all rows (same bits)
        D3PM_TRY(embed_twins(q, x_t, s));
        D3PM_TRY(row_stats_launch(dt, q.ws.x, d, n, d, q.ws.stats, s, quads));
      } else if (q.dd) {
        D3PM_TRY(run_dedup_index(q, x_t, quads, s));
        qkv_ready = true;
      } else {
        EmbedArgs e = embed_args(sh, q.w, q.batch, x_t, q.frame_mask, q.mask_period, q.ws.x);
        if (q.qkv_table && e.n_q == 1 && q.ws.q0) { e.qkv_table = q.qkv_table; e.q0 = q.ws.q0; e.kv0 = q.ws.kv0; }
        D3PM_TRY(embed_tokens_stats(dt, e, q.ws.stats, quads, s));
        qkv_ready = e.q0 != nullptr;
      }
    }
    {   // fc1 of every block under norm3 + FiLM(t): the weights this evaluation's fc1 launches read
      ProfScope p(cx, D3PM_K_LN, s, 0.0, es * 2.0 * layers * 4.0 * d * d);
      D3PM_TRY(fold_fc1_step_launch(dt, q.w.blocks, layers, at(film, static_cast<size_t>(t) * sh.n_layers * 2 * d, es), d, q.ws.fc1f, q.ws.fc1f_s,
                                    q.ws.fc1f_b, s));
    }
  }
  FoldLauncher launch{cx, dt, s};
  for (int l = 0; l < layers; ++l) D3PM_TRY(folded_block(q, l, quads, launch, qkv_ready));
  return D3PM_OK;
}

// One denoiser evaluation up to the final projection: the hidden state after `layers` blocks is left in ws.x.  `plan` is the moment format
// of the evaluation (LoopPlan::fold; FOLD_PARTS in a latency iteration): FOLD_NONE runs the LayerNorm / row-panel launches below (and the fp8 fast path, BASELINE.json configs[4]).
static int denoiser_blocks(const DenoiserArgs& q, const int32_t* x_t, int t, const void* film, int layers, uint32_t flags, hipStream_t s,
                           const d3pm_fp8_block_weights* f8, int plan, bool prepared = false, bool qkv_ready = false) {
  // LayerNorm folded into the projections (d3pm_tuning.ln_fold, d3pm_fold_block): every LayerNorm-fed projection reads the raw
  // residual stream and normalises in its epilogue; every projection that lands on the residual stream leaves the row moments
  if (plan != FOLD_NONE) return denoiser_blocks_folded(q, x_t, t, film, layers, s, prepared, plan == FOLD_QUADS, prepared && qkv_ready);

  const d3pm_shape& sh = q.sh;
  const d3pm_weights& w = q.w;
  const Workspace& ws = q.ws;
  const uint8_t* frame_mask = q.frame_mask;
  const int dt = sh.dtype, d = sh.d_model, H = sh.n_heads, hd = d / H, T = sh.canvas, batch = q.batch;
  const int n = batch * T, mask_period = q.mask_period;
  const Ctx cx(sh.tuning);
  const size_t es = dtype_size(dt);
  // fp8 fast path: the three LayerNorm-fed K = d projections take e4m3 operands; the e4m3 rows
  // and their scales live where the 16-bit LayerNorm outputs would (ws.h | ws.h2 are adjacent: 2 n d 2 bytes)
  const bool use8 = f8 != nullptr;
  if (use8) {   // the *_fp8 entry points never fall back to the 16-bit kernels silently: a number labelled fp8 is fp8
    D3PM_REQUIRE(!(flags & D3PM_FLAG_FORCE_GENERIC), D3PM_E_ARG, "fp8 fast path: D3PM_FLAG_FORCE_GENERIC selects the 16-bit generic kernels");
    D3PM_REQUIRE(d == 512 && (dt == D3PM_F16 || dt == D3PM_BF16) && n % 192 == 0 && ws.h2 == at(ws.h, static_cast<size_t>(n) * d, dtype_size(dt)),
                 D3PM_E_SHAPE, "fp8 fast path needs d_model = 512, a 16-bit model dtype and batch * canvas (%d) a multiple of 192", n);
  }
  // MX operands of the LayerNorm-fed projections live where the 16-bit LayerNorm outputs would: codes [2n][512] fill ws.h.
  // The shared qkv | q | hidden | logits region (n x 4d elements = 4096 n bytes) also holds fc1's MX output: codes [n][2048] at
  // its start and scales [n][64] at byte 2048 n.  The LayerNorm block scales [2n][16] have a workspace slot of their own (ws.mxs):
  // they are read by a persistent GEMM for the whole launch, so they must not share bytes with anything that launch writes (a
  // 16-bit fc1 output [n][2048] x 2 B covers the whole shared region).
  uint8_t* x8 = reinterpret_cast<uint8_t*>(ws.h);
  uint8_t* h8 = reinterpret_cast<uint8_t*>(ws.mlp);
  uint8_t* sh8 = h8 + static_cast<size_t>(n) * 4 * d;
  uint8_t* sx8 = ws.mxs;
  auto mx_gemm = [&](const uint8_t* X8, int ldx8, const uint8_t* SX8, const void* W8, const void* SW8, const void* bias, void* Y, int ldy,
                     const void* R1, const uint8_t* mask, int period, uint8_t* Y8, uint8_t* SY, int M, int N, int K, int act) -> int {
    MxLinearArgs m;
    m.X8 = X8; m.ldx = ldx8; m.SX = SX8; m.W8 = W8; m.SW = SW8; m.bias = bias; m.Y = Y; m.ldy = ldy; m.R1 = R1; m.ldr = ldy;
    m.row_mask = mask; m.mask_period = period; m.Y8 = Y8; m.SY = SY; m.M = M; m.N = N; m.K = K; m.act = act; m.tune = cx.tune;
    D3PM_REQUIRE(mx_linear_supported(dt, m), D3PM_E_SHAPE, "fp8 fast path: block-scaled GEMM %d x %d x %d not supported", M, N, K);
    ProfScope p(cx, D3PM_K_GEMM, s, 2.0 * M * N * K,
                1.03125 * (static_cast<double>(M) * K + static_cast<double>(N) * K) + static_cast<double>(M) * N * (Y8 ? 1.03125 : (R1 ? 2.0 : 1.0) * es));
    return mx_linear(dt, m, s);
  };
  auto layernorm = [&](const void* lw, const void* lb) {      // x -> h, eps 1e-6
    LayerNormArgs ln;
    ln.X = ws.x; ln.Y = ws.h; ln.w = lw; ln.b = lb; ln.M = n; ln.d = d; ln.eps = 1e-6f;
    return ln;
  };

  // the first block's norm1 reads the embedding rows straight from the table and writes x beside its own output: one launch and
  // one pass over x less per iteration (same bits: the gather is a copy)
  bool embed_fused = false;
  if (!use8 && !(flags & D3PM_FLAG_FORCE_GENERIC) && layers > 0 && levels(sh) == 1 && !q.token_rows) {
    LayerNormArgs ln0 = layernorm(w.blocks[0].norm1_w, w.blocks[0].norm1_b);
    ln0.X = w.resps_emb;
    ln0.tokens = x_t; ln0.frame_mask = frame_mask; ln0.mask_period = mask_period; ln0.n_classes = sh.n_classes; ln0.Xout = ws.x;
    if (fast_layernorm_supported(dt, ln0)) {
      ProfScope p(cx, D3PM_K_LN, s, 0.0, dtype_size(dt) * static_cast<double>(n) * d * 3.0);
      D3PM_TRY(fast_layernorm(dt, ln0, s));
      embed_fused = true;
    }
  }
  if (q.token_rows) D3PM_TRY(embed_twins(q, x_t, s));      // (the gather is a copy: the rows norm1 reads are those of the fused launch)
  else if (!embed_fused) D3PM_TRY(embed_tokens(dt, embed_args(sh, w, batch, x_t, frame_mask, mask_period, ws.x), s));

  // row-panel launches (D3PM_TUNE_ROW_PANEL): a projection that lands on the residual stream also writes the LayerNorm(s) the
  // block applies to the new rows next -- same bits, one launch and one pass over x less each
  // (one 96-row tile per workgroup: only when the tiles fill >= 85 % of whole rounds over the CUs, as for the other big tiles)
  const bool rp_fills = n % 96 == 0 && fills_rounds(n / 96, kCUs);
  const int panel = (!(flags & D3PM_FLAG_FORCE_GENERIC) && d == 512 && rp_fills && (dt == D3PM_F16 || dt == D3PM_BF16))
                        ? (tune_of(sh.tuning).row_panel & (use8 ? 3 : 7)) : 0;      // fp8: fc2 is a block-scaled GEMM of its own
  bool norm1_done = embed_fused;   // norm1(x) of this block is already in ws.h (the embedding launch, or the previous block's fc2)
  // a LayerNorm-fed projection g (g.X = the LayerNorm output): LayerNorm launch + projection, unless an earlier launch has written
  // the LayerNorm rows already
  auto ln_linear = [&](bool ln_done, const LayerNormArgs& ln, const LinearArgs& g) -> int {
    if (!ln_done) D3PM_TRY(run_layernorm(cx, dt, ln, flags, s));
    return run_linear(cx, dt, g, flags, s);
  };

  for (int l = 0; l < layers; ++l) {
    const d3pm_block_weights& b = w.blocks[l];
    // ---- self-attention ----
    LayerNormArgs ln = layernorm(b.norm1_w, b.norm1_b);
    if (use8) {
      {
        ProfScope p(cx, D3PM_K_LN, s, 0.0, static_cast<double>(n) * d * (es + 1.03125));
        D3PM_TRY(layernorm_mx(dt, ws.x, x8, sx8, b.norm1_w, b.norm1_b, nullptr, nullptr, nullptr, nullptr, nullptr, n, d, 1e-6f, s));
      }
      D3PM_TRY(mx_gemm(x8, d, sx8, f8[l].attn_in_w8, f8[l].attn_in_scale, b.attn_in_b, ws.qkv, 3 * d, nullptr, nullptr, 1, nullptr, nullptr,
                       n, 3 * d, d, ACT_NONE));
    } else {
      D3PM_TRY(ln_linear(norm1_done, ln, projection(ws.h, b.attn_in_w, b.attn_in_b, ws.qkv, n, 3 * d, d)));
    }
    norm1_done = false;
    D3PM_TRY(run_attention(cx, dt, with_frame_keys(self_attention(ws.qkv, ws.att, batch, T, H, hd, es), q.keys), flags, s));
    LinearArgs g = with_residual(projection(ws.att, b.attn_out_w, b.attn_out_b, ws.x, n, d, d), ws.x);
    // ---- cross-attention: text keys with LN2 queries, prompt keys with LN22 queries, SAME weights ----
    ln = layernorm(b.norm2_w, b.norm2_b);
    ln.Y2 = ws.h2; ln.w2 = b.norm22_w; ln.b2 = b.norm22_b;
    RowPanelFuse rp;
    rp.lnw = ln.w; rp.lnb = ln.b; rp.lny = ln.Y; rp.lnw2 = ln.w2; rp.lnb2 = ln.b2; rp.lny2 = ln.Y2; rp.eps = ln.eps;
    if (use8) {      // the LayerNorm rows leave the row-panel launch as MX codes + block scales: the query projection's operand
      rp.lny = x8; rp.lny2 = x8 + static_cast<size_t>(n) * d; rp.sx = sx8; rp.sx2 = sx8 + static_cast<size_t>(n) * 16;
    }
    const bool norm2_fused = (panel & 1) && row_panel_supported(dt, g, rp);
    if (norm2_fused) D3PM_TRY(run_row_panel(cx, dt, g, rp, s));
    else D3PM_TRY(run_linear(cx, dt, g, flags, s));
    char* q_text = ws.qkv;
    char* q_prom = at(ws.qkv, static_cast<size_t>(n) * d, es);
    if (use8) {
      // MX rows of norm2(x) | norm22(x) stacked [2n][d] (fills ws.h), block scales [2n][16]: ONE GEMM for both queries
      if (!norm2_fused) {
        ProfScope p(cx, D3PM_K_LN, s, 0.0, static_cast<double>(n) * d * (es + 2 * 1.03125));
        D3PM_TRY(layernorm_mx(dt, ws.x, x8, sx8, b.norm2_w, b.norm2_b, nullptr, b.norm22_w, b.norm22_b,
                              x8 + static_cast<size_t>(n) * d, sx8 + static_cast<size_t>(n) * 16, n, d, 1e-6f, s));
      }
      D3PM_TRY(mx_gemm(x8, d, sx8, f8[l].cross_in_w8, f8[l].cross_in_scale, b.cross_in_b, q_text, d, nullptr, nullptr, 1, nullptr, nullptr,
                       2 * n, d, d, ACT_NONE));
    } else if (ws.h2 == at(ws.h, static_cast<size_t>(n) * d, es)) {
      // both query projections share cross_attn's q rows: LN2|LN22 outputs and q_text|q_prompt are adjacent in
      // the workspace, so the pair is ONE [2n, d] x [d, d] GEMM (twice the workgroups of either alone)
      D3PM_TRY(ln_linear(norm2_fused, ln, projection(ws.h, b.cross_in_w, b.cross_in_b, q_text, 2 * n, d, d)));
    } else {
      if (!norm2_fused) D3PM_TRY(run_layernorm(cx, dt, ln, flags, s));
      D3PM_TRY(run_linear(cx, dt, projection(ws.h, b.cross_in_w, b.cross_in_b, q_text, n, d, d), flags, s));
      D3PM_TRY(run_linear(cx, dt, projection(ws.h2, b.cross_in_w, b.cross_in_b, q_prom, n, d, d), flags, s));
    }
    {   // text and prompt cross-attention are independent: one paired launch
      const void* kvt = at(q.kv_text, static_cast<size_t>(l) * batch * sh.s_text * 2 * d, es);
      const void* kvp = at(q.kv_prompt, static_cast<size_t>(l) * batch * sh.s_prompt * 2 * d, es);
      D3PM_TRY(run_attention(cx, dt, with_cond_keys(cross_attention_pair(q_text, q_prom, d, kvt, sh.s_text, kvp, sh.s_prompt, ws.att, ws.att2, batch, T, H, hd, es), q.keys),
                             flags, s));
    }
    // ---- both out-projections, then the FiLM-modulated MLP ----
    ln = layernorm(b.norm3_w, b.norm3_b);
    ln.film = at(film, (static_cast<size_t>(t) * sh.n_layers + l) * 2 * d, es);
    g = with_residual(projection(ws.att, b.cross_out_w, b.cross_out_b, ws.x, n, d, d), ws.x);
    rp = RowPanelFuse();
    rp.X2 = ws.att2; rp.lnw = ln.w; rp.lnb = ln.b; rp.lny = ln.Y; rp.film = ln.film; rp.eps = ln.eps;
    if (use8) { rp.lny = x8; rp.sx = sx8; }
    const bool norm3_fused = (panel & 2) && row_panel_supported(dt, g, rp);
    if (norm3_fused) {
      D3PM_TRY(run_row_panel(cx, dt, g, rp, s));
    } else {
      g.tune = cx.tune;
      const CrossOutPlan out = plan_cross_out(dt, g, ws.att2, forced_generic(flags), false);      // (throughput batches have the row-panel launch above: no big_dual here)
      if (out.form != CROSS_OUT_TWO_LAUNCHES) {
        D3PM_TRY(run_cross_out_dual(cx, dt, out, g, ws.att2, s));
      } else {
        D3PM_TRY(run_linear(cx, dt, projection(ws.att, b.cross_out_w, b.cross_out_b, ws.h, n, d, d), flags, s));
        D3PM_TRY(run_linear(cx, dt, with_residual(projection(ws.att2, b.cross_out_w, b.cross_out_b, ws.x, n, d, d), ws.x, ws.h), flags, s));
      }
    }
    const bool fc2_mx = use8 && f8[l].fc2_w8 && f8[l].fc2_scale;
    if (use8) {
      if (!norm3_fused) {
        ProfScope p(cx, D3PM_K_LN, s, 0.0, static_cast<double>(n) * d * (es + 1.03125));
        D3PM_TRY(layernorm_mx(dt, ws.x, x8, sx8, b.norm3_w, b.norm3_b, ln.film, nullptr, nullptr, nullptr, nullptr, n, d, 1e-6f, s));
      }
      // with an MX fc2 the GELU epilogue writes the hidden layer as codes + block scales (half the bytes out, half in again)
      D3PM_TRY(mx_gemm(x8, d, sx8, f8[l].fc1_w8, f8[l].fc1_scale, b.fc1_b, ws.mlp, 4 * d, nullptr, nullptr, 1, fc2_mx ? h8 : nullptr,
                       fc2_mx ? sh8 : nullptr, n, 4 * d, d, ACT_GELU));
    } else {
      D3PM_TRY(ln_linear(norm3_fused, ln, projection(ws.h, b.fc1_w, b.fc1_b, ws.mlp, n, 4 * d, d, ACT_GELU)));
    }
    g = with_row_mask(with_residual(projection(ws.mlp, b.fc2_w, b.fc2_b, ws.x, n, d, 4 * d), ws.x), frame_mask, mask_period);
    rp = RowPanelFuse();
    if (l + 1 < layers) { rp.lnw = w.blocks[l + 1].norm1_w; rp.lnb = w.blocks[l + 1].norm1_b; rp.lny = ws.h; rp.eps = 1e-6f; }
    if (fc2_mx) {
      D3PM_TRY(mx_gemm(h8, 4 * d, sh8, f8[l].fc2_w8, f8[l].fc2_scale, b.fc2_b, ws.x, d, ws.x, frame_mask, mask_period, nullptr, nullptr, n, d, 4 * d,
                       ACT_NONE));
    } else if ((panel & 4) && l + 1 < layers && row_panel_supported(dt, g, rp)) {
      D3PM_TRY(run_row_panel(cx, dt, g, rp, s));
      norm1_done = true;
    } else {
      D3PM_TRY(run_linear(cx, dt, g, flags, s));
    }
  }
  return D3PM_OK;
}

static int final_logits(const d3pm_shape& sh, const d3pm_weights& w, int batch, const Workspace& ws, void* logits,
                        int ldl, uint32_t flags, hipStream_t s, const int* m_live = nullptr) {
  // x is already multiplied by the frame mask at the end of every block (ar_discrete.py:161,773).
  // n_q > 1: one projection per level (final_w [n_q][n_classes][d]) into the level's [ldl]-wide slot of a frame's n_q * ldl logits
  const Ctx cx(sh.tuning);
  const size_t es = dtype_size(sh.dtype);
  for (int l = 0; l < levels(sh); ++l) {
    LinearArgs g = projection(ws.x, at(w.final_w, static_cast<size_t>(l) * sh.n_classes * sh.d_model, es),
                              at(w.final_b, static_cast<size_t>(l) * sh.n_classes, es), at(logits, static_cast<size_t>(l) * ldl, es),
                              batch * sh.canvas, sh.n_classes, sh.d_model);
    g.ldy = levels(sh) * ldl;
    g.m_live = m_live;
    D3PM_TRY(run_linear(cx, sh.dtype, g, flags, s));
  }
  return D3PM_OK;
}

}  // namespace d3pm

using namespace d3pm;

extern "C" {

int d3pm_abi_version(void) { return D3PM_ABI_VERSION; }

size_t d3pm_workspace_bytes(const d3pm_shape* shape, int batch) {
  if (check_shape(shape, batch) != D3PM_OK) return 0;
  return carve(*shape, batch, nullptr).total;
}

int d3pm_film_table(const d3pm_shape* sh, const d3pm_weights* w, void* film, void* stream) {
  D3PM_TRY(check_shape(sh, 1));
  D3PM_REQUIRE(w && w->blocks && w->time_emb && film, D3PM_E_ARG, "d3pm_film_table: null pointer");
  const int d = sh->d_model;
  for (int l = 0; l < sh->n_layers; ++l) {
    LinearArgs g = projection(w->time_emb, w->blocks[l].tfc_w, w->blocks[l].tfc_b, at(film, static_cast<size_t>(l) * 2 * d, dtype_size(sh->dtype)),
                              sh->timesteps + 1, 2 * d, d);
    g.ldy = sh->n_layers * 2 * d;
    D3PM_TRY(generic_linear(sh->dtype, g, static_cast<hipStream_t>(stream)));
  }
  return D3PM_OK;
}

// ---- LayerNorm folded into the projections: the tables ---------------------------------------------------------------
struct FoldLayout { size_t qkv_w, q2_w, qkv_s, qkv_b, q2_s, q2_b, per_layer; };
static FoldLayout fold_layout(const d3pm_shape& sh) {
  const size_t es = dtype_size(sh.dtype), d = sh.d_model;
  FoldLayout L{};
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at_ = off; off += align256(bytes); return at_; };
  L.qkv_w = take(3 * d * d * es); L.q2_w = take(2 * d * d * es);
  L.qkv_s = take(3 * d * 4); L.qkv_b = take(3 * d * 4); L.q2_s = take(2 * d * 4); L.q2_b = take(2 * d * 4);
  L.per_layer = off;
  return L;
}

size_t d3pm_fold_bytes(const d3pm_shape* sh) {
  if (check_shape(sh, 1) != D3PM_OK || !fold_shape_ok(sh->dtype, sh->d_model)) return 0;
  return fold_layout(*sh).per_layer * static_cast<size_t>(sh->n_layers);
}

int d3pm_fold_build(const d3pm_shape* sh, const d3pm_weights* w, void* storage, size_t storage_bytes, d3pm_fold_block* out, void* stream) {
  D3PM_TRY(check_shape(sh, 1));
  D3PM_REQUIRE(w && w->blocks && storage && out, D3PM_E_ARG, "d3pm_fold_build: null pointer");
  D3PM_REQUIRE(fold_shape_ok(sh->dtype, sh->d_model), D3PM_E_SHAPE, "d3pm_fold_build: needs a 16-bit dtype and d_model a multiple of 256");
  const FoldLayout L = fold_layout(*sh);
  D3PM_REQUIRE(storage_bytes >= L.per_layer * sh->n_layers, D3PM_E_WORKSPACE, "d3pm_fold_build: storage %zu < required %zu", storage_bytes,
               L.per_layer * static_cast<size_t>(sh->n_layers));
  D3PM_REQUIRE(reinterpret_cast<uintptr_t>(storage) % 256 == 0, D3PM_E_ARG, "d3pm_fold_build: storage must be 256-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int dt = sh->dtype, d = sh->d_model;
  const size_t es = dtype_size(dt);
  for (int l = 0; l < sh->n_layers; ++l) {
    const d3pm_block_weights& b = w->blocks[l];
    char* base = static_cast<char*>(storage) + L.per_layer * l;
    auto f32 = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    D3PM_TRY(fold_rows_launch(dt, b.attn_in_w, b.attn_in_b, b.norm1_w, b.norm1_b, nullptr, 0, 3 * d, 1, d, base + L.qkv_w, f32(L.qkv_s), f32(L.qkv_b), s));
    // cross_attn's q rows under norm2 (text queries) and under norm22 (prompt queries): the two halves of one [2d][d] operand
    D3PM_TRY(fold_rows_launch(dt, b.cross_in_w, b.cross_in_b, b.norm2_w, b.norm2_b, nullptr, 0, d, 1, d, base + L.q2_w, f32(L.q2_s), f32(L.q2_b), s));
    D3PM_TRY(fold_rows_launch(dt, b.cross_in_w, b.cross_in_b, b.norm22_w, b.norm22_b, nullptr, 0, d, 1, d, base + L.q2_w + static_cast<size_t>(d) * d * es,
                              f32(L.q2_s) + d, f32(L.q2_b) + d, s));
    d3pm_fold_block& o = out[l];
    o.qkv_w = base + L.qkv_w; o.qkv_s = f32(L.qkv_s); o.qkv_b = f32(L.qkv_b);
    o.q2_w = base + L.q2_w; o.q2_s = f32(L.q2_s); o.q2_b = f32(L.q2_b);
  }
  return D3PM_OK;
}

int d3pm_op_fold_weights(int dtype, const void* W, const void* bias, const void* gamma, const void* beta, const void* film, int N, int K,
                         void* Wf, float* fold_s, float* fold_b, void* stream) {
  D3PM_REQUIRE(W && gamma && beta && Wf && fold_s && fold_b && N > 0 && K > 0 && K % 8 == 0 && (dtype == D3PM_F16 || dtype == D3PM_BF16),
               D3PM_E_ARG, "d3pm_op_fold_weights: bad arguments");
  return fold_rows_launch(dtype, W, bias, gamma, beta, film, 0, N, 1, K, Wf, fold_s, fold_b, static_cast<hipStream_t>(stream));
}

int d3pm_op_row_stats(int dtype, const void* X, int ldx, int M, int d, float* stats, void* stream) {
  D3PM_REQUIRE(X && stats && M > 0 && d > 0 && d % 32 == 0 && ldx % 8 == 0 && (dtype == D3PM_F16 || dtype == D3PM_BF16), D3PM_E_ARG,
               "d3pm_op_row_stats: bad arguments");
  return row_stats_launch(dtype, X, ldx, M, d, stats, static_cast<hipStream_t>(stream));
}

int d3pm_op_linear_stats(int dtype, const void* X, int ldx, const void* W, const void* bias, void* Y, int ldy, const void* R1,
                         const void* R2, int ldr, const uint8_t* row_mask, int mask_period, int M, int N, int K, float* stats_out,
                         const d3pm_tuning* tuning, void* stream) {
  D3PM_REQUIRE(X && W && Y && R1 && stats_out && M > 0 && N > 0 && K > 0, D3PM_E_ARG, "d3pm_op_linear_stats: bad arguments");
  LinearArgs g;
  g.tune = tuning;
  g.X = X; g.ldx = ldx; g.W = W; g.bias = bias; g.Y = Y; g.ldy = ldy; g.R1 = R1; g.R2 = R2; g.ldr = ldr;
  g.row_mask = row_mask; g.mask_period = mask_period > 0 ? mask_period : 1; g.M = M; g.N = N; g.K = K; g.stats_out = stats_out;
  const LinearPlan plan = plan_linear(dtype, g);
  D3PM_REQUIRE(plan.mfma(), D3PM_E_SHAPE, "d3pm_op_linear_stats: needs the MFMA family (16-bit, K %% 64 == 0, N %% 32 == 0)");
  return mfma_linear(dtype, g, plan, static_cast<hipStream_t>(stream));
}

int d3pm_op_linear_fold(int dtype, const void* X, int ldx, const void* Wf, const float* fold_s, const float* fold_b, const float* stats_in,
                        float eps, void* Y, int ldy, int M, int N, int K, int act, const d3pm_tuning* tuning, void* stream) {
  D3PM_REQUIRE(X && Wf && fold_s && fold_b && stats_in && Y && M > 0 && N > 0 && K > 0, D3PM_E_ARG, "d3pm_op_linear_fold: bad arguments");
  LinearArgs g;
  g.tune = tuning;
  g.X = X; g.ldx = ldx; g.W = Wf; g.Y = Y; g.ldy = ldy; g.M = M; g.N = N; g.K = K; g.act = act;
  g.fold_s = fold_s; g.fold_b = fold_b; g.stats_in = stats_in; g.fold_eps = eps;
  const LinearPlan plan = plan_linear(dtype, g);
  D3PM_REQUIRE(plan.mfma(), D3PM_E_SHAPE,
               "d3pm_op_linear_fold: needs the MFMA family (16-bit), K a multiple of 256, N of 4, act 0 / 1 and 16-byte aligned tables");
  return mfma_linear(dtype, g, plan, static_cast<hipStream_t>(stream));
}

int d3pm_op_dedup_index(int dtype, const int32_t* tokens, const uint8_t* frame_mask, int batch, int canvas, int n_classes, int d,
                        const void* table, int32_t* seg_start, int32_t* seg_len, int32_t* m_live, int32_t* row_of, int32_t* cid, uint8_t* cmask,
                        void* x, float* stats, int32_t* scratch, void* stream) {
  return d3pm_op_dedup_index_align(dtype, tokens, frame_mask, batch, canvas, n_classes, d, 128, table, seg_start, seg_len, m_live, row_of, cid, cmask, x,
                                   stats, scratch, stream);
}

int d3pm_op_dedup_index_align(int dtype, const int32_t* tokens, const uint8_t* frame_mask, int batch, int canvas, int n_classes, int d, int seg_align,
                              const void* table, int32_t* seg_start, int32_t* seg_len, int32_t* m_live, int32_t* row_of, int32_t* cid,
                              uint8_t* cmask, void* x, float* stats, int32_t* scratch, void* stream) {
  D3PM_REQUIRE(batch > 0 && canvas > 0 && scratch && (!table || (x && stats)), D3PM_E_ARG, "d3pm_op_dedup_index: bad arguments");
  DedupArgs a;
  a.seg_align = seg_align;      // (dedup_index refuses anything but 1 and 128)
  a.tokens = tokens; a.frame_mask = frame_mask; a.mask_period = batch * canvas; a.batch = batch; a.canvas = canvas; a.n_classes = n_classes; a.d = d;
  a.ix.cnt = scratch; a.ix.rep_pos = scratch + batch; a.ix.seg_start = seg_start; a.ix.seg_len = seg_len; a.ix.m_live = m_live; a.ix.row_of = row_of;
  a.ix.cid = cid; a.ix.cmask = cmask;
  a.table = table; a.x = x; a.stats = stats; a.quads = d == 512;
  return dedup_index(dtype, a, static_cast<hipStream_t>(stream));
}

int d3pm_op_linear_live(int dtype, const void* X, const void* X2, int ldx, const void* W, const void* bias, void* Y, int ldy, const void* R1, int ldr,
                        const uint8_t* row_mask, int mask_period, int M, int N, int K, int act, const float* fold_s, const float* fold_b,
                        const float* stats_in, float* stats_out, const int32_t* m_live, const d3pm_tuning* tuning, void* stream) {
  return d3pm_op_linear_live_est(dtype, X, X2, ldx, W, bias, Y, ldy, R1, ldr, row_mask, mask_period, M, N, K, act, fold_s, fold_b, stats_in, stats_out,
                                 m_live, 0, tuning, stream);
}

int d3pm_op_linear_live_est(int dtype, const void* X, const void* X2, int ldx, const void* W, const void* bias, void* Y, int ldy, const void* R1,
                            int ldr, const uint8_t* row_mask, int mask_period, int M, int N, int K, int act, const float* fold_s, const float* fold_b,
                            const float* stats_in, float* stats_out, const int32_t* m_live, int m_est, const d3pm_tuning* tuning, void* stream) {
  return d3pm_op_linear_live_rows(dtype, X, X2, ldx, W, bias, Y, ldy, R1, ldr, row_mask, mask_period, M, N, K, act, fold_s, fold_b, stats_in, stats_out,
                                  m_live, m_est, 0, tuning, stream);
}

int d3pm_op_linear_live_rows(int dtype, const void* X, const void* X2, int ldx, const void* W, const void* bias, void* Y, int ldy, const void* R1,
                             int ldr, const uint8_t* row_mask, int mask_period, int M, int N, int K, int act, const float* fold_s, const float* fold_b,
                             const float* stats_in, float* stats_out, const int32_t* m_live, int m_est, int rows_est, const d3pm_tuning* tuning,
                             void* stream) {
  D3PM_REQUIRE(X && W && Y && m_live && M > 0 && N > 0 && K > 0 && m_est >= 0 && rows_est >= 0, D3PM_E_ARG, "d3pm_op_linear_live: bad arguments");
  LinearArgs g;
  g.rows_est = rows_est;
  g.tune = tuning;
  g.X = X; g.ldx = ldx; g.W = W; g.bias = bias; g.Y = Y; g.ldy = ldy; g.R1 = R1; g.ldr = ldr; g.M = M; g.N = N; g.K = K; g.act = act;
  g.row_mask = row_mask; g.mask_period = mask_period > 0 ? mask_period : 1;
  g.fold_s = fold_s; g.fold_b = fold_b; g.stats_in = stats_in; g.stats_out = stats_out;
  g.m_live = m_live; g.m_est = m_est;
  // gemm_mfma_panel64 reads and writes the moments as parts; where the planner names another family they travel as quads at width 512
  const bool quads = (fold_s || stats_out) && (fold_s ? K : N) == 512;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (X2) {      // both cross-attention out-projections in one launch
    CrossOutPlan c = plan_cross_out(dtype, g, X2, false, true);
    if (c.form == CROSS_OUT_PANEL64_DUAL) return panel64_dual(dtype, g, X2, c.dual, s);
    g.moment_quads = quads;
    c = plan_cross_out(dtype, g, X2, false, true);
    D3PM_REQUIRE(c.form == CROSS_OUT_BIG_DUAL, D3PM_E_SHAPE, "d3pm_op_linear_live: the dual form needs the big-tile or the panel64 family");
    return big_dual(dtype, g, X2, c.dual, s);
  }
  LinearPlan plan = plan_linear(dtype, g);
  // (a gemm_variant that forces a big-tile geometry is asked again with quads even where the parts format fell to the latency family:
  // the short tiles exist with quads only)
  if (plan.kernel != LIN_PANEL64 || tune_of(tuning).gemm_variant >= 6) {
    LinearArgs gq = g;
    gq.moment_quads = quads;
    const LinearPlan pq = plan_linear(dtype, gq);
    if (plan.kernel != LIN_PANEL64 || pq.big()) { g = gq; plan = pq; }
  }
  D3PM_REQUIRE(plan.big() || plan.kernel == LIN_128_GLDS || plan.kernel == LIN_PANEL64, D3PM_E_SHAPE,
               "d3pm_op_linear_live: %d x %d x %d takes a kernel without a device-side row count", M, N, K);
  return mfma_linear(dtype, g, plan, s);
}

size_t d3pm_op_embed_qkv_bytes(const d3pm_shape* sh, int n) {
  if (check_shape(sh, 1) != D3PM_OK || n < 1 || !fold_shape_ok(sh->dtype, sh->d_model) || levels(*sh) != 1) return 0;
  const size_t es = dtype_size(sh->dtype), d = sh->d_model, mt = qkv_table_rows(sh->n_classes), rows = (static_cast<size_t>(n) + 15) & ~static_cast<size_t>(15);
  return align256(mt * d * es) + align256(mt * (d / 32) * 2 * sizeof(float)) + align256(mt * 3 * d * es) + align256(rows * d * es) +
         align256(rows * (d / 32) * 2 * sizeof(float));
}

int d3pm_op_embed_qkv(const d3pm_shape* sh, const d3pm_weights* w, const int32_t* tokens, const uint8_t* frame_mask, int n, void* storage,
                      size_t storage_bytes, void* q_out, void* kv_out, void* stream) {
  D3PM_TRY(check_shape(sh, 1));
  D3PM_REQUIRE(w && w->resps_emb && w->fold && tokens && frame_mask && storage && q_out && kv_out && n > 0, D3PM_E_ARG, "d3pm_op_embed_qkv: null pointer");
  D3PM_REQUIRE(fold_shape_ok(sh->dtype, sh->d_model) && levels(*sh) == 1, D3PM_E_SHAPE,
               "d3pm_op_embed_qkv: needs a 16-bit dtype, d_model a multiple of 256 and n_q <= 1");
  const size_t need = d3pm_op_embed_qkv_bytes(sh, n);
  D3PM_REQUIRE(storage_bytes >= need, D3PM_E_WORKSPACE, "d3pm_op_embed_qkv: storage %zu < required %zu", storage_bytes, need);
  D3PM_REQUIRE(reinterpret_cast<uintptr_t>(storage) % 256 == 0 && reinterpret_cast<uintptr_t>(q_out) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(kv_out) % 16 == 0,
               D3PM_E_ARG, "d3pm_op_embed_qkv: storage must be 256-byte aligned, q_out and kv_out 16-byte aligned");
  const size_t es = dtype_size(sh->dtype), d = sh->d_model, mt = qkv_table_rows(sh->n_classes), rows = (static_cast<size_t>(n) + 15) & ~static_cast<size_t>(15);
  Workspace ws{};
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = static_cast<char*>(storage) + off; off += align256(bytes); return p; };
  ws.tab_x = take(mt * d * es);
  ws.tab_stats = reinterpret_cast<float*>(take(mt * (d / 32) * 2 * sizeof(float)));
  ws.tab_qkv = take(mt * 3 * d * es);
  ws.x = take(rows * d * es);
  ws.stats = reinterpret_cast<float*>(take(rows * (d / 32) * 2 * sizeof(float)));
  hipStream_t s = static_cast<hipStream_t>(stream);
  D3PM_TRY(build_qkv_table(Ctx(sh->tuning), *sh, *w, ws, s));
  EmbedArgs e;
  e.tokens = tokens; e.frame_mask = frame_mask; e.mask_period = n; e.table = w->resps_emb; e.Y = ws.x; e.M = n; e.d = sh->d_model;
  e.n_classes = sh->n_classes; e.qkv_table = ws.tab_qkv; e.q0 = q_out; e.kv0 = kv_out;
  return embed_tokens_stats(sh->dtype, e, ws.stats, false, s);
}

int d3pm_cond_kv(const d3pm_shape* sh, const d3pm_weights* w, int batch, const void* cond_text, const void* cond_prompt,
                 void* kv_text, void* kv_prompt, void* stream) {
  D3PM_TRY(check_shape(sh, batch));
  D3PM_REQUIRE(w && w->blocks && cond_text && cond_prompt && kv_text && kv_prompt, D3PM_E_ARG, "d3pm_cond_kv: null pointer");
  const int d = sh->d_model;
  const size_t es = dtype_size(sh->dtype);
  const Ctx cx(sh->tuning);
  for (int l = 0; l < sh->n_layers; ++l)
    for (int which = 0; which < 2; ++which) {
      const int S = which ? sh->s_prompt : sh->s_text;
      // the k | v rows of the packed in-projection
      const LinearArgs g = projection(which ? cond_prompt : cond_text, at(w->blocks[l].cross_in_w, static_cast<size_t>(d) * d, es),
                                      at(w->blocks[l].cross_in_b, d, es), at(which ? kv_prompt : kv_text, static_cast<size_t>(l) * batch * S * 2 * d, es),
                                      batch * S, 2 * d, d);
      D3PM_TRY(run_linear(cx, sh->dtype, g, 0, static_cast<hipStream_t>(stream)));
    }
  return D3PM_OK;
}

// ---- condition encoders ----------------------------------------------------------------------------
struct CondWs { char *x, *tmp, *qkv, *att, *ff, *qkv_pad, *att_pad; size_t total; };
#ifndef D3PM_ENC_HEAD_PAD
#define D3PM_ENC_HEAD_PAD 1      // A/B builds (tools/build_variant.py): 0 = the encoders' 32-wide heads stay on the generic attention kernel
#endif
// the encoder's self-attention on the 64-wide MFMA kernels through zero-padded heads (d3pm_headpad.hip)
static bool encoder_pads_heads(const d3pm_shape& sh, const d3pm_encoder_weights& e) {
  return D3PM_ENC_HEAD_PAD != 0 && (sh.dtype == D3PM_F16 || sh.dtype == D3PM_BF16) && e.n_heads > 0 && sh.d_model == 32 * e.n_heads;
}
static CondWs carve_cond(const d3pm_shape& sh, const d3pm_cond_weights& cw, int batch, char* base) {
  const size_t es = dtype_size(sh.dtype), d = sh.d_model;
  const size_t n = static_cast<size_t>(batch) * (sh.s_prompt > sh.s_text ? sh.s_prompt : sh.s_text);
  auto wide = [](const d3pm_encoder_weights& e) { return static_cast<size_t>(e.d_ff > e.mlp_hidden ? e.d_ff : e.mlp_hidden); };
  const size_t ffw = wide(cw.text_encoder) > wide(cw.prompt_encoder) ? wide(cw.text_encoder) : wide(cw.prompt_encoder);
  CondWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
  w.x = take(n * d * es);
  w.tmp = take(n * d * es);
  w.qkv = take(n * 3 * d * es);
  w.att = take(n * d * es);
  w.ff = take(n * ffw * es);
  if (encoder_pads_heads(sh, cw.text_encoder) || encoder_pads_heads(sh, cw.prompt_encoder)) {
    w.qkv_pad = take(n * 6 * d * es);
    w.att_pad = take(n * 2 * d * es);
  }
  w.total = off;
  return w;
}

// x (ws.x, [rows][d]) -> out ([rows][d]); `seq` rows per utterance
// key_len: the valid rows of each utterance (d3pm_keys.text / .prompt) or null: the keys of the encoder's self-attention
static int run_encoder(const d3pm_shape& sh, const d3pm_encoder_weights& e, int batch, int seq, const CondWs& ws, void* out,
                       const int32_t* key_len, hipStream_t s) {
  const int dt = sh.dtype, d = sh.d_model, n = batch * seq, hd = d / e.n_heads;
  const size_t es = dtype_size(dt);
  const Ctx cx(sh.tuning);
  for (int l = 0; l < e.n_layers; ++l) {
    const d3pm_encoder_layer_weights& w = e.layers[l];
    D3PM_TRY(run_linear(cx, dt, projection(ws.x, w.in_w, w.in_b, ws.qkv, n, 3 * d, d), 0, s));
    AttnArgs a = self_attention(ws.qkv, ws.att, batch, seq, e.n_heads, hd, es);
    a.key_len = key_len; a.masked_keeps_schedule = key_len != nullptr;
    if (encoder_pads_heads(sh, e) && ws.qkv_pad) {
      D3PM_TRY(pad_heads(ws.qkv, ws.qkv_pad, n, 3 * e.n_heads, hd, s));
      AttnArgs p = a;
      p.Q = ws.qkv_pad; p.K = at(ws.qkv_pad, 2 * d, es); p.V = at(ws.qkv_pad, 4 * d, es); p.ldq = p.ldkv = 6 * d;
      p.O = ws.att_pad; p.ldo = 2 * d; p.hd = 2 * hd;                // scale stays 1 / sqrt(hd)
      D3PM_TRY(run_attention(cx, dt, p, 0, s));
      D3PM_TRY(unpad_heads(ws.att_pad, ws.att, n, e.n_heads, hd, s));
    } else {
      D3PM_TRY(run_attention(cx, dt, a, 0, s));
    }
    // x + self_attn(x), then post-norm
    D3PM_TRY(run_linear(cx, dt, with_residual(projection(ws.att, w.out_w, w.out_b, ws.tmp, n, d, d), ws.x), 0, s));
    LayerNormArgs ln;
    ln.X = ws.tmp; ln.Y = ws.x; ln.w = w.norm1_w; ln.b = w.norm1_b; ln.M = n; ln.d = d; ln.eps = 1e-5f;
    D3PM_TRY(run_layernorm(cx, dt, ln, 0, s));
    // FFN: linear2(relu(linear1(x)))
    D3PM_TRY(run_linear(cx, dt, projection(ws.x, w.lin1_w, w.lin1_b, ws.ff, n, e.d_ff, d, ACT_RELU), 0, s));
    D3PM_TRY(run_linear(cx, dt, with_residual(projection(ws.ff, w.lin2_w, w.lin2_b, ws.tmp, n, d, e.d_ff), ws.x), 0, s));
    ln.w = w.norm2_w; ln.b = w.norm2_b;
    D3PM_TRY(run_layernorm(cx, dt, ln, 0, s));
  }
  // timm Mlp: fc2(silu(fc1(x)))
  D3PM_TRY(run_linear(cx, dt, projection(ws.x, e.fc1_w, e.fc1_b, ws.ff, n, e.mlp_hidden, d, ACT_SILU), 0, s));
  return run_linear(cx, dt, projection(ws.ff, e.fc2_w, e.fc2_b, out, n, d, e.mlp_hidden), 0, s);
}

static bool encoder_ok(const d3pm_encoder_weights& e, int d) {
  return e.layers && e.n_layers > 0 && e.n_heads > 0 && d % e.n_heads == 0 && e.d_ff > 0 && e.mlp_hidden > 0 && e.fc1_w &&
         e.fc1_b && e.fc2_w && e.fc2_b;
}

size_t d3pm_cond_workspace_bytes(const d3pm_shape* sh, const d3pm_cond_weights* cw, int batch) {
  if (check_shape(sh, batch) != D3PM_OK || !cw) return 0;
  return carve_cond(*sh, *cw, batch, nullptr).total;
}

static int encode_conditions_impl(const d3pm_shape* sh, const d3pm_cond_weights* cw, int batch, const int32_t* text,
                                  const int32_t* prompt, void* cond_text, void* cond_prompt, void* workspace,
                                  size_t workspace_bytes, const KeyCounts& keys, void* stream) {
  D3PM_TRY(check_shape(sh, batch));
  D3PM_REQUIRE(cw && text && prompt && cond_text && cond_prompt && workspace && cw->text_emb && cw->proms_emb &&
                   cw->pe_text0 && cw->pe_prompt && cw->n_levels > 0,
               D3PM_E_ARG, "d3pm_encode_conditions: null pointer");
  D3PM_REQUIRE(encoder_ok(cw->text_encoder, sh->d_model) && encoder_ok(cw->prompt_encoder, sh->d_model), D3PM_E_ARG,
               "d3pm_encode_conditions: incomplete encoder weights");
  CondWs ws = carve_cond(*sh, *cw, batch, static_cast<char*>(workspace));
  D3PM_REQUIRE(workspace_bytes >= ws.total, D3PM_E_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, ws.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  D3PM_TRY(cond_embed_text(sh->dtype, text, cw->text_emb, cw->pe_text0, ws.x, batch * sh->s_text, sh->s_text, sh->d_model, sh->n_classes,
                           keys.text, s));
  D3PM_TRY(run_encoder(*sh, cw->text_encoder, batch, sh->s_text, ws, cond_text, keys.text, s));
  D3PM_TRY(cond_embed_prompt(sh->dtype, prompt, cw->n_levels, cw->proms_emb, cw->pe_prompt, ws.x, batch * sh->s_prompt,
                             sh->s_prompt, sh->d_model, sh->n_classes, keys.prompt, s));
  return run_encoder(*sh, cw->prompt_encoder, batch, sh->s_prompt, ws, cond_prompt, keys.prompt, s);
}

int d3pm_encode_conditions(const d3pm_shape* sh, const d3pm_cond_weights* cw, int batch, const int32_t* text,
                           const int32_t* prompt, void* cond_text, void* cond_prompt, void* workspace,
                           size_t workspace_bytes, void* stream) {
  return encode_conditions_impl(sh, cw, batch, text, prompt, cond_text, cond_prompt, workspace, workspace_bytes, KeyCounts{}, stream);
}

int d3pm_encode_conditions_keys(const d3pm_shape* sh, const d3pm_cond_weights* cw, int batch, const int32_t* text,
                                const int32_t* prompt, void* cond_text, void* cond_prompt, void* workspace,
                                size_t workspace_bytes, const d3pm_keys* keys, void* stream) {
  return encode_conditions_impl(sh, cw, batch, text, prompt, cond_text, cond_prompt, workspace, workspace_bytes, key_counts(keys), stream);
}

// What the forms of an entry point add to the arguments they share; each extern "C" entry fills the fields it has.
struct CallOptions {
  const char* who;                                  // the entry's name, for messages
  CanvasMask mask;                                  // the frame mask (either_mask) and, for a sampler, the known frames
  const d3pm_fp8_block_weights* f8 = nullptr;       // the fp8 fast path
  const d3pm_nucleus* nucleus = nullptr;            // temperature, top-k, top-p (null = the neutral triple)
  KeyCounts keys = {};
  const d3pm_guidance* guide = nullptr;
  float* theta_out = nullptr;                       // d3pm_posterior_sample_nucleus
  const d3pm_frame_scores* scores = nullptr;        // d3pm_sample_loop_scored: the grids of the launch behind every sampler launch
  const d3pm_reveal* reveal = nullptr;              // the reveal loop: n_steps and the choice temperature
  const d3pm_revise* revise = nullptr;              // d3pm_reveal_loop_revise: the hold bonus
};
// one mask [canvas] shared by the batch, or one per utterance (+ the known frames): the entries that take either check that one is given
static CanvasMask either_mask(const d3pm_shape* sh, int batch, const uint8_t* frame_mask, const d3pm_canvas* canvas) {
  return canvas ? per_utterance_mask(sh, batch, canvas, true) : shared_mask(sh, frame_mask);
}

static int denoise_step_impl(const d3pm_shape* sh, const d3pm_weights* w, int batch, const int32_t* x_t, int t, const void* film,
                             const void* kv_text, const void* kv_prompt, void* workspace, size_t workspace_bytes, void* logits_out,
                             void* hidden_out, int only_layers, uint32_t flags, void* stream, const CallOptions& o) {
  const CanvasMask& cm = o.mask;
  D3PM_TRY(check_shape(sh, batch));
  D3PM_REQUIRE(w && w->blocks && x_t && cm.frame_mask && film && kv_text && kv_prompt && workspace, D3PM_E_ARG,
               "d3pm_denoise_step: null pointer");
  D3PM_REQUIRE(t >= 0 && t <= sh->timesteps, D3PM_E_ARG, "t=%d outside [0,%d]", t, sh->timesteps);
  Workspace ws = carve(*sh, batch, static_cast<char*>(workspace));
  D3PM_REQUIRE(workspace_bytes >= ws.total, D3PM_E_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, ws.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int layers = (only_layers >= 0 && only_layers < sh->n_layers) ? only_layers : sh->n_layers;
  const DenoiserArgs q{*sh, *w, batch, cm.frame_mask, cm.period, kv_text, kv_prompt, ws, o.keys};
  // (one evaluation: the moment format is all there is to plan)
  D3PM_TRY(denoiser_blocks(q, x_t, t, film, layers, flags, s, o.f8, loop_plan(q, flags, LoopCall{o.f8 != nullptr}).fold));
  if (hidden_out)
    D3PM_CHECK_HIP(hipMemcpyAsync(hidden_out, ws.x, static_cast<size_t>(batch) * sh->canvas * sh->d_model * dtype_size(sh->dtype),
                                  hipMemcpyDeviceToDevice, s));
  if (logits_out) {
    const size_t es = dtype_size(sh->dtype);
    D3PM_TRY(final_logits(*sh, *w, batch, ws, ws.logits, logits_ld(*sh), flags, s));
    D3PM_CHECK_HIP(hipMemcpy2DAsync(logits_out, sh->n_classes * es, ws.logits, logits_ld(*sh) * es, sh->n_classes * es,
                                    static_cast<size_t>(batch) * sh->canvas * levels(*sh), hipMemcpyDeviceToDevice, s));
  }
  return D3PM_OK;
}

int d3pm_denoise_step(const d3pm_shape* sh, const d3pm_weights* w, int batch, const int32_t* x_t,
                      const uint8_t* frame_mask, int t, const void* film, const void* kv_text, const void* kv_prompt,
                      void* workspace, size_t workspace_bytes, void* logits_out, void* hidden_out, int only_layers,
                      uint32_t flags, void* stream) {
  return denoise_step_impl(sh, w, batch, x_t, t, film, kv_text, kv_prompt, workspace, workspace_bytes, logits_out, hidden_out, only_layers, flags,
                           stream, CallOptions{"d3pm_denoise_step", shared_mask(sh, frame_mask)});
}

int d3pm_denoise_step_canvas(const d3pm_shape* sh, const d3pm_weights* w, int batch, const int32_t* x_t, const d3pm_canvas* canvas, int t,
                             const void* film, const void* kv_text, const void* kv_prompt, void* workspace, size_t workspace_bytes,
                             void* logits_out, void* hidden_out, int only_layers, uint32_t flags, void* stream) {
  D3PM_REQUIRE(canvas, D3PM_E_ARG, "d3pm_denoise_step_canvas: null canvas");
  return denoise_step_impl(sh, w, batch, x_t, t, film, kv_text, kv_prompt, workspace, workspace_bytes, logits_out, hidden_out, only_layers, flags,
                           stream, CallOptions{"d3pm_denoise_step_canvas", per_utterance_mask(sh, batch, canvas, false)});
}

int d3pm_denoise_step_keys(const d3pm_shape* sh, const d3pm_weights* w, int batch, const int32_t* x_t, const d3pm_canvas* canvas, int t,
                           const void* film, const void* kv_text, const void* kv_prompt, void* workspace, size_t workspace_bytes,
                           void* logits_out, void* hidden_out, int only_layers, uint32_t flags, const d3pm_keys* keys, void* stream) {
  D3PM_REQUIRE(canvas, D3PM_E_ARG, "d3pm_denoise_step_keys: null canvas");
  return denoise_step_impl(sh, w, batch, x_t, t, film, kv_text, kv_prompt, workspace, workspace_bytes, logits_out, hidden_out, only_layers, flags,
                           stream, CallOptions{"d3pm_denoise_step_keys", per_utterance_mask(sh, batch, canvas, false), nullptr, nullptr, key_counts(keys)});
}

int d3pm_denoise_step_fp8(const d3pm_shape* sh, const d3pm_weights* w, const d3pm_fp8_block_weights* fp8_blocks, int batch,
                          const int32_t* x_t, const uint8_t* frame_mask, int t, const void* film, const void* kv_text,
                          const void* kv_prompt, void* workspace, size_t workspace_bytes, void* logits_out, void* hidden_out,
                          int only_layers, uint32_t flags, void* stream) {
  D3PM_REQUIRE(fp8_blocks, D3PM_E_ARG, "d3pm_denoise_step_fp8: null fp8 weights");
  return denoise_step_impl(sh, w, batch, x_t, t, film, kv_text, kv_prompt, workspace, workspace_bytes, logits_out, hidden_out, only_layers, flags,
                           stream, CallOptions{"d3pm_denoise_step_fp8", shared_mask(sh, frame_mask), fp8_blocks});
}

// d3pm_nucleus of the *_nucleus entries (the *_sampling entries forward their pair with top_p = 1): NULL = the neutral triple.
// Refused before anything is launched.
static int check_sampling(const d3pm_shape* sh, const d3pm_nucleus* sm, const char* who) {
  if (!sm) return D3PM_OK;
  D3PM_REQUIRE(std::isfinite(sm->temperature) && sm->temperature > 0.f, D3PM_E_ARG, "%s: temperature %g is not a finite number > 0", who,
               static_cast<double>(sm->temperature));
  D3PM_REQUIRE(sm->top_k >= 0 && sm->top_k <= sh->n_classes, D3PM_E_ARG, "%s: top_k %d outside 0 (off) .. %d (n_classes)", who, sm->top_k,
               sh->n_classes);
  D3PM_REQUIRE(std::isfinite(sm->top_p) && sm->top_p > 0.f && sm->top_p <= 1.f, D3PM_E_ARG, "%s: top_p %g outside (0, 1] (1 = off)", who,
               static_cast<double>(sm->top_p));
  return D3PM_OK;
}
// the pair of a *_sampling entry as a triple (`out` lives in the caller)
static const d3pm_nucleus* with_top_p_off(const d3pm_sampling* sm, d3pm_nucleus* out) {
  if (!sm) return nullptr;
  *out = d3pm_nucleus{sm->temperature, sm->top_k, 1.0f};
  return out;
}

// The sampler launch of `batch` utterances at timestep t, whichever kernel takes it: logits rows of stride ldl, one Philox row per
// frame from utt0 * canvas on.  What only some callers have -- the trace grid, posterior_out, theta_out, the seed in HBM -- they set.
static SampleArgs sample_args(const d3pm_shape& sh, int batch, const void* logits, int logits_dtype, int ldl, const int32_t* x_t, int32_t* x_next,
                              const uint8_t* known, int t, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0, uint32_t flags,
                              const d3pm_nucleus* sm, const d3pm_guidance* guide) {
  SampleArgs a;
  a.logits = logits; a.logits_dtype = logits_dtype; a.ldl = ldl; a.x_t = x_t; a.x_next = x_next;
  a.rows = batch * sh.canvas * levels(sh); a.n_q = levels(sh); a.n_classes = sh.n_classes; a.mask_id = sh.mask_id; a.canvas = sh.canvas;
  a.seed = seed; a.row0 = utt0 * static_cast<uint32_t>(sh.canvas); a.greedy = (flags & D3PM_FLAG_GREEDY) ? 1 : 0;
  a.pc = make_posterior_consts(sched, t);
  a.known = known;
  if (sm) { a.temperature = sm->temperature; a.top_k = sm->top_k; a.top_p = sm->top_p; }
  if (guide) { a.guided = true; a.guidance = guide->weight; }
  return a;
}

static int posterior_sample_impl(const d3pm_shape* sh, int batch, const void* logits, int logits_dtype, const int32_t* x_t,
                                 int32_t* x_next, int t, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                                 uint32_t flags, uint16_t* posterior_out, void* stream, const CallOptions& o) {
  D3PM_TRY(check_shape(sh, batch));
  D3PM_TRY(check_sampling(sh, o.nucleus, o.who));
  D3PM_REQUIRE(logits && x_t && x_next && sched && sched->d && sched->c && sched->dbar && sched->cbar, D3PM_E_ARG,
               "d3pm_posterior_sample: null pointer");
  D3PM_REQUIRE(t >= 0 && t < sched->timesteps, D3PM_E_ARG, "t=%d outside the schedule", t);
  SampleArgs a = sample_args(*sh, batch, logits, logits_dtype, sh->n_classes, x_t, x_next, o.mask.known, t, sched, seed, utt0, flags, o.nucleus, nullptr);
  a.posterior_out = posterior_out;
  a.theta_out = o.theta_out;
  return posterior_sample(a, static_cast<hipStream_t>(stream));
}

int d3pm_posterior_sample(const d3pm_shape* sh, int batch, const void* logits, int logits_dtype, const int32_t* x_t,
                          int32_t* x_next, int t, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                          uint32_t flags, uint16_t* posterior_out, void* stream) {
  return posterior_sample_impl(sh, batch, logits, logits_dtype, x_t, x_next, t, sched, seed, utt0, flags, posterior_out, stream,
                               CallOptions{"d3pm_posterior_sample", CanvasMask{}});
}

int d3pm_posterior_sample_known(const d3pm_shape* sh, int batch, const void* logits, int logits_dtype, const int32_t* x_t,
                                int32_t* x_next, const uint8_t* known, int t, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                                uint32_t flags, uint16_t* posterior_out, void* stream) {
  return posterior_sample_impl(sh, batch, logits, logits_dtype, x_t, x_next, t, sched, seed, utt0, flags, posterior_out, stream,
                               CallOptions{"d3pm_posterior_sample_known", CanvasMask{nullptr, 0, known}});
}

int d3pm_posterior_sample_sampling(const d3pm_shape* sh, int batch, const void* logits, int logits_dtype, const int32_t* x_t,
                                   int32_t* x_next, const uint8_t* known, int t, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                                   uint32_t flags, uint16_t* posterior_out, const d3pm_sampling* sampling, void* stream) {
  d3pm_nucleus nu;
  return posterior_sample_impl(sh, batch, logits, logits_dtype, x_t, x_next, t, sched, seed, utt0, flags, posterior_out, stream,
                               CallOptions{"d3pm_posterior_sample_sampling", CanvasMask{nullptr, 0, known}, nullptr, with_top_p_off(sampling, &nu)});
}

int d3pm_posterior_sample_nucleus(const d3pm_shape* sh, int batch, const void* logits, int logits_dtype, const int32_t* x_t,
                                  int32_t* x_next, const uint8_t* known, int t, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                                  uint32_t flags, uint16_t* posterior_out, const d3pm_nucleus* nucleus, float* theta_out, void* stream) {
  return posterior_sample_impl(sh, batch, logits, logits_dtype, x_t, x_next, t, sched, seed, utt0, flags, posterior_out, stream,
                               CallOptions{"d3pm_posterior_sample_nucleus", CanvasMask{nullptr, 0, known}, nullptr, nucleus, {}, nullptr, theta_out});
}

// the sampler launch of the deduplicated loop on its own (tests): posterior_sample_dedup with no next-iteration fold
int d3pm_op_posterior_sample_rows(const d3pm_shape* sh, int batch, const void* logits, int logits_dtype, int ldl, const int32_t* row_of,
                                  const int32_t* x_t, int32_t* x_next, int32_t* x_next2, const uint8_t* known, int t,
                                  const d3pm_schedule* sched, uint64_t seed, uint32_t utt0, uint32_t flags, const d3pm_nucleus* nucleus,
                                  const d3pm_guidance* guidance, void* stream) {
  const char* who = "d3pm_op_posterior_sample_rows";
  D3PM_TRY(check_shape(sh, batch));
  D3PM_TRY(check_sampling(sh, nucleus, who));
  D3PM_REQUIRE(logits && x_t && x_next && sched && sched->d && sched->c && sched->dbar && sched->cbar, D3PM_E_ARG, "%s: null pointer", who);
  D3PM_REQUIRE(t >= 0 && t < sched->timesteps, D3PM_E_ARG, "t=%d outside the schedule", t);
  D3PM_REQUIRE(ldl >= sh->n_classes, D3PM_E_ARG, "%s: row stride %d below n_classes %d", who, ldl, sh->n_classes);
  D3PM_REQUIRE(!(flags & D3PM_FLAG_SEED_IN_HBM), D3PM_E_ARG, "%s: the seed travels by value", who);
  // (guidance is refused below: the deduplicated launch has no guided form)
  SampleArgs a = sample_args(*sh, batch, logits, logits_dtype, ldl, x_t, x_next, known, t, sched, seed, utt0, flags, nucleus, guidance);
  a.x_next2 = x_next2;
  return posterior_sample_dedup(a, row_of, NextIterPrep{}, static_cast<hipStream_t>(stream));
}

// What the launch that ends an evaluation prepares for the evaluation at t_next (NextIterPrep): fc1 of every block under norm3 +
// FiLM(t_next), and the embedding rows of the ids it draws with their moments -- in the block-0 QKV table's loop their q | k | v rows
// too (never under guidance).  The deduplicated loop embeds nothing here: run_dedup_index follows the launch.
static NextIterPrep next_iter_prep(const DenoiserArgs& q, const void* film, int t_next, bool quads) {
  const d3pm_shape& sh = q.sh;
  NextIterPrep nx;
  nx.dtype = sh.dtype; nx.d = sh.d_model; nx.blocks = q.w.blocks; nx.n_layers = sh.n_layers;
  nx.film_t = at(film, static_cast<size_t>(t_next) * sh.n_layers * 2 * sh.d_model, dtype_size(sh.dtype));
  nx.Wf = q.ws.fc1f; nx.s_out = q.ws.fc1f_s; nx.b_out = q.ws.fc1f_b;
  if (q.dd) return nx;
  nx.table = q.w.resps_emb; nx.x = q.ws.x; nx.stats = q.ws.stats; nx.frame_mask = q.frame_mask; nx.mask_period = q.mask_period;
  nx.quads = quads;
  if (q.qkv_table) { nx.qkv_table = q.qkv_table; nx.q0 = q.ws.q0; nx.kv0 = q.ws.kv0; }
  return nx;
}

// ---- per-frame log-probability of the revealed id (d3pm_frame_scores, d3pm_logprob.hip) ---------------------------------------------
static LogprobArgs logprob_args(const d3pm_shape& sh, int rows, const void* logits, int logits_dtype, int ldl, const int32_t* row_of, bool guided,
                                float guidance, const int32_t* x_next, int t, const d3pm_frame_scores* scores) {
  LogprobArgs a;
  a.logits = logits; a.logits_dtype = logits_dtype; a.ldl = ldl; a.row_of = row_of; a.guided = guided; a.guidance = guidance; a.x_next = x_next;
  a.logprob = scores->logprob; a.step = scores->step; a.rows = rows; a.n_classes = sh.n_classes; a.mask_id = sh.mask_id; a.t = t;
  return a;
}
// the launch behind a sampler launch, counted with the samplers (algorithmic bytes: two words per row + the logits of the rows that
// leave the mask, on average rows / (T - 1) of them)
static int run_frame_logprob(const Ctx& cx, const LogprobArgs& a, hipStream_t s) {
  ProfScope p(cx, D3PM_K_SAMPLE, s, 0.0, static_cast<double>(a.rows) * 8.0);
  return frame_logprob(a, s);
}
// what every entry that takes d3pm_frame_scores refuses before anything is launched
static int check_scores(const d3pm_shape* sh, const d3pm_frame_scores* scores, const char* who) {
  D3PM_REQUIRE(sh, D3PM_E_ARG, "null shape");
  D3PM_REQUIRE(scores && scores->logprob && scores->step, D3PM_E_ARG, "%s: null d3pm_frame_scores or a null grid in it", who);
  D3PM_REQUIRE(levels(*sh) == 1, D3PM_E_SHAPE, "%s: n_q = %d; frame scores are defined for n_q = 1", who, sh->n_q);
  return D3PM_OK;
}

// The sampler launch of an iteration in whichever of its five forms applies -- deduplicated (every canvas row draws from the logits of
// its compact row; then the index and the compact embedding of the next iteration), with the next iteration's preparation inside the
// launch (plain or guided), or alone (plain or guided).  `preps`: there is a next iteration on the folded path, at t_next, whose moments
// travel as quads_next says.  *prepared: the launch (or the index launch behind it) has embedded x_t and folded fc1 for t_next;
// *qkv_ready: ... and gathered ws.q0 | ws.kv0 for every row of that evaluation.
// `scores` (d3pm_sample_loop_scored): one more launch behind the sampler's, in front of the index launch that rebuilds row_of.
static int run_sampler(const Ctx& cx, const DenoiserArgs& q, const SampleArgs& a, const void* film, int t_next, bool preps, bool quads_next,
                       hipStream_t s, bool* prepared, bool* qkv_ready, const d3pm_frame_scores* scores = nullptr) {
  const d3pm_shape& sh = q.sh;
  const size_t es = dtype_size(sh.dtype);
  const NextIterPrep nx = preps ? next_iter_prep(q, film, t_next, quads_next) : NextIterPrep{};
  *prepared = *qkv_ready = false;
  {
    // (+ the block-0 q | k | v rows the launch stores for the next evaluation; their source, the table, stays in L2)
    ProfScope p(cx, D3PM_K_SAMPLE, s, 0.0,
                static_cast<double>(a.rows) * ((a.guided ? 2.0 : 1.0) * sh.n_classes * es + 8.0) +
                    (nx.q0 ? static_cast<double>(a.rows) * 3.0 * sh.d_model * es : 0.0));
    if (q.dd) {
      D3PM_TRY(posterior_sample_dedup(a, q.dd->row_of, nx, s));
    } else if (nx.table && posterior_sample_prep_supported(a, nx)) {
      // + the embedding rows, their moments and the fc1 fold of t_next (guided: the rows of both halves)
      D3PM_TRY(a.guided ? posterior_sample_prep_guided(a, nx, s) : posterior_sample_prep(a, nx, s));
      *prepared = true;
      *qkv_ready = nx.q0 != nullptr;
    } else {
      D3PM_TRY(a.guided ? posterior_sample_guided(a, s) : posterior_sample(a, s));
    }
  }
  if (scores) D3PM_TRY(run_frame_logprob(cx, logprob_args(sh, a.rows, a.logits, a.logits_dtype, a.ldl, q.dd ? q.dd->row_of : nullptr,
                                                          a.guided, a.guidance, a.x_next, a.pc.t, scores), s));
  if (q.dd && preps) {
    D3PM_TRY(run_dedup_index(q, a.x_next, quads_next, s));
    *prepared = *qkv_ready = true;
  }
  return D3PM_OK;
}

static int sample_loop_impl(const d3pm_shape* sh, const d3pm_weights* w, int batch, int32_t* x, int t_start, int t_stop, const void* film,
                            const void* kv_text, const void* kv_prompt, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                            uint32_t flags, void* workspace, size_t workspace_bytes, int32_t* trace, void* stream, const CallOptions& o) {
  const CanvasMask& cm = o.mask;
  const d3pm_guidance* guide = o.guide;
  D3PM_TRY(check_shape(sh, batch));
  D3PM_TRY(check_sampling(sh, o.nucleus, o.who));
  D3PM_REQUIRE(w && w->blocks && x && cm.frame_mask && film && kv_text && kv_prompt && sched && workspace, D3PM_E_ARG,
               "d3pm_sample_loop: null pointer");
  D3PM_REQUIRE(t_start < sched->timesteps && t_start <= sh->timesteps && t_stop >= 0 && t_stop <= t_start, D3PM_E_ARG,
               "bad step range %d..%d", t_start, t_stop);
  // Classifier-free guidance (d3pm_guidance): one evaluation of 2 * batch utterances per step -- utterance batch + b is the null twin of
  // b: the same x_t, the same frame mask (the mask period stays that of `batch`, so row r and row rows + r read the same byte), its own
  // K/V and key counts -- and a sampler over `batch` utterances that reads both halves of the logits.  The attention regime rule sees
  // twice the logical batch, so a shard of a guided batch takes the kernels of the unsplit one.
  d3pm_shape gsh;
  d3pm_tuning gtune;
  if (guide) {
    gtune = tune_of(sh->tuning);
    gtune.regime_batch = 2 * (gtune.regime_batch > batch ? gtune.regime_batch : batch);
    gsh = *sh;
    gsh.tuning = &gtune;
    sh = &gsh;
  }
  const int eval_batch = guide ? 2 * batch : batch;
  Workspace ws = carve(*sh, eval_batch, static_cast<char*>(workspace));
  D3PM_REQUIRE(workspace_bytes >= ws.total, D3PM_E_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, ws.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rows = batch * sh->canvas;
  const Ctx cx(sh->tuning);
  DenoiserArgs q{*sh, *w, eval_batch, cm.frame_mask, cm.period, kv_text, kv_prompt, ws, o.keys, guide ? rows : 0};
  const LoopPlan plan = loop_plan(q, flags, LoopCall{o.f8 != nullptr, guide != nullptr, cm.known != nullptr, t_start, t_stop});
  if (plan.table) {
    D3PM_TRY(build_qkv_table(cx, *sh, *w, ws, s));
    q.qkv_table = ws.tab_qkv;
  }
  if (plan.dedup) q.dd = &ws.dd;
  if (o.scores) D3PM_TRY(frame_scores_init(x, cm.frame_mask, cm.period, cm.known, o.scores->logprob, o.scores->step, rows, sh->mask_id, s));
  bool prepared = false, qkv_ready = false;      // by the previous iteration's sampler launch
  for (int t = t_start; t > t_stop; --t) {
    if (cx.prof) cx.prof->sample_now = (t % cx.prof->stride) == 0;
    q.m_est = plan.m_est(sched, t);
    q.seg_est = plan.seg_est(sched, t);
    q.rows_est = plan.rows_est(sched, t);
    D3PM_TRY(denoiser_blocks(q, x, t, film, sh->n_layers, flags, s, o.f8, q.m_est ? FOLD_PARTS : plan.fold, prepared, qkv_ready));
    D3PM_TRY(final_logits(*sh, *w, eval_batch, ws, ws.logits, logits_ld(*sh), flags, s, q.dd ? q.dd->m_live : nullptr));
    SampleArgs a = sample_args(*sh, batch, ws.logits, sh->dtype, logits_ld(*sh), x, x, cm.known, t, sched, seed, utt0, flags, o.nucleus, guide);
    a.x_next2 = trace ? trace + static_cast<size_t>(t_start - t) * rows * levels(*sh) : nullptr;
    if (flags & D3PM_FLAG_SEED_IN_HBM) a.seed_hbm = reinterpret_cast<const uint64_t*>(static_cast<uintptr_t>(seed));
    const bool preps = t - 1 > t_stop && plan.fold != FOLD_NONE;
    D3PM_TRY(run_sampler(cx, q, a, film, t - 1, preps, plan.fold == FOLD_QUADS && !plan.m_est(sched, t - 1), s, &prepared, &qkv_ready,
                         o.scores));
  }
  if (cx.prof) cx.prof->sample_now = false;
  return D3PM_OK;
}

int d3pm_sample_loop(const d3pm_shape* sh, const d3pm_weights* w, int batch, int32_t* x, const uint8_t* frame_mask,
                     int t_start, int t_stop, const void* film, const void* kv_text, const void* kv_prompt,
                     const d3pm_schedule* sched, uint64_t seed, uint32_t utt0, uint32_t flags, void* workspace,
                     size_t workspace_bytes, int32_t* trace, void* stream) {
  return sample_loop_impl(sh, w, batch, x, t_start, t_stop, film, kv_text, kv_prompt, sched, seed, utt0, flags, workspace, workspace_bytes, trace,
                          stream, CallOptions{"d3pm_sample_loop", shared_mask(sh, frame_mask)});
}

int d3pm_sample_loop_canvas(const d3pm_shape* sh, const d3pm_weights* w, int batch, int32_t* x, const d3pm_canvas* canvas,
                            int t_start, int t_stop, const void* film, const void* kv_text, const void* kv_prompt,
                            const d3pm_schedule* sched, uint64_t seed, uint32_t utt0, uint32_t flags, void* workspace,
                            size_t workspace_bytes, int32_t* trace, void* stream) {
  D3PM_REQUIRE(canvas, D3PM_E_ARG, "d3pm_sample_loop_canvas: null canvas");
  return sample_loop_impl(sh, w, batch, x, t_start, t_stop, film, kv_text, kv_prompt, sched, seed, utt0, flags, workspace, workspace_bytes, trace,
                          stream, CallOptions{"d3pm_sample_loop_canvas", per_utterance_mask(sh, batch, canvas, true)});
}

int d3pm_sample_loop_fp8(const d3pm_shape* sh, const d3pm_weights* w, const d3pm_fp8_block_weights* fp8_blocks, int batch,
                         int32_t* x, const uint8_t* frame_mask, int t_start, int t_stop, const void* film,
                         const void* kv_text, const void* kv_prompt, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                         uint32_t flags, void* workspace, size_t workspace_bytes, int32_t* trace, void* stream) {
  D3PM_REQUIRE(fp8_blocks, D3PM_E_ARG, "d3pm_sample_loop_fp8: null fp8 weights");
  return sample_loop_impl(sh, w, batch, x, t_start, t_stop, film, kv_text, kv_prompt, sched, seed, utt0, flags, workspace, workspace_bytes, trace,
                          stream, CallOptions{"d3pm_sample_loop_fp8", shared_mask(sh, frame_mask), fp8_blocks});
}

int d3pm_sample_loop_fp8_canvas(const d3pm_shape* sh, const d3pm_weights* w, const d3pm_fp8_block_weights* fp8_blocks, int batch,
                                int32_t* x, const d3pm_canvas* canvas, int t_start, int t_stop, const void* film,
                                const void* kv_text, const void* kv_prompt, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                                uint32_t flags, void* workspace, size_t workspace_bytes, int32_t* trace, void* stream) {
  D3PM_REQUIRE(fp8_blocks && canvas, D3PM_E_ARG, "d3pm_sample_loop_fp8_canvas: null fp8 weights or canvas");
  return sample_loop_impl(sh, w, batch, x, t_start, t_stop, film, kv_text, kv_prompt, sched, seed, utt0, flags, workspace, workspace_bytes, trace,
                          stream, CallOptions{"d3pm_sample_loop_fp8_canvas", per_utterance_mask(sh, batch, canvas, true), fp8_blocks});
}

int d3pm_sample_loop_sampling(const d3pm_shape* sh, const d3pm_weights* w, const d3pm_fp8_block_weights* fp8_blocks, int batch, int32_t* x,
                              const uint8_t* frame_mask, const d3pm_canvas* canvas, int t_start, int t_stop, const void* film,
                              const void* kv_text, const void* kv_prompt, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                              uint32_t flags, void* workspace, size_t workspace_bytes, int32_t* trace, const d3pm_sampling* sampling,
                              void* stream) {
  D3PM_REQUIRE(sh && (frame_mask != nullptr) != (canvas != nullptr), D3PM_E_ARG,
               "d3pm_sample_loop_sampling: give exactly one of frame_mask (shared by the batch) and canvas (per utterance)");
  d3pm_nucleus nu;
  return sample_loop_impl(sh, w, batch, x, t_start, t_stop, film, kv_text, kv_prompt, sched, seed, utt0, flags, workspace, workspace_bytes, trace,
                          stream, CallOptions{"d3pm_sample_loop_sampling", either_mask(sh, batch, frame_mask, canvas), fp8_blocks, with_top_p_off(sampling, &nu)});
}

int d3pm_sample_loop_nucleus(const d3pm_shape* sh, const d3pm_weights* w, const d3pm_fp8_block_weights* fp8_blocks, int batch, int32_t* x,
                             const uint8_t* frame_mask, const d3pm_canvas* canvas, int t_start, int t_stop, const void* film,
                             const void* kv_text, const void* kv_prompt, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                             uint32_t flags, void* workspace, size_t workspace_bytes, int32_t* trace, const d3pm_nucleus* nucleus,
                             void* stream) {
  D3PM_REQUIRE(sh && (frame_mask != nullptr) != (canvas != nullptr), D3PM_E_ARG,
               "d3pm_sample_loop_nucleus: give exactly one of frame_mask (shared by the batch) and canvas (per utterance)");
  return sample_loop_impl(sh, w, batch, x, t_start, t_stop, film, kv_text, kv_prompt, sched, seed, utt0, flags, workspace, workspace_bytes, trace,
                          stream, CallOptions{"d3pm_sample_loop_nucleus", either_mask(sh, batch, frame_mask, canvas), fp8_blocks, nucleus});
}

int d3pm_sample_loop_keys(const d3pm_shape* sh, const d3pm_weights* w, const d3pm_fp8_block_weights* fp8_blocks, int batch, int32_t* x,
                          const uint8_t* frame_mask, const d3pm_canvas* canvas, int t_start, int t_stop, const void* film,
                          const void* kv_text, const void* kv_prompt, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                          uint32_t flags, void* workspace, size_t workspace_bytes, int32_t* trace, const d3pm_nucleus* nucleus,
                          const d3pm_keys* keys, void* stream) {
  D3PM_REQUIRE(sh && (frame_mask != nullptr) != (canvas != nullptr), D3PM_E_ARG,
               "d3pm_sample_loop_keys: give exactly one of frame_mask (shared by the batch) and canvas (per utterance)");
  D3PM_REQUIRE(!(keys && fp8_blocks), D3PM_E_ARG, "d3pm_sample_loop_keys: the fp8 fast path takes no key mask");
  return sample_loop_impl(sh, w, batch, x, t_start, t_stop, film, kv_text, kv_prompt, sched, seed, utt0, flags, workspace, workspace_bytes, trace,
                          stream, CallOptions{"d3pm_sample_loop_keys", either_mask(sh, batch, frame_mask, canvas), fp8_blocks, nucleus, key_counts(keys)});
}

// ---- classifier-free guidance (d3pm_guidance) -----------------------------------------------------------------------------------------
// refused before anything is launched: a missing weight, a weight that is negative or not finite, more than one level
static int check_guidance(const d3pm_shape* sh, const d3pm_guidance* g, const char* who) {
  D3PM_REQUIRE(sh, D3PM_E_ARG, "null shape");
  D3PM_REQUIRE(g, D3PM_E_ARG, "%s: null d3pm_guidance", who);
  D3PM_REQUIRE(std::isfinite(g->weight) && g->weight >= 0.f, D3PM_E_ARG, "%s: guidance weight %g is not a finite number >= 0", who,
               static_cast<double>(g->weight));
  D3PM_REQUIRE(levels(*sh) == 1, D3PM_E_ARG, "%s: guidance is defined for n_q = 1 (got %d levels)", who, levels(*sh));
  return D3PM_OK;
}

int d3pm_posterior_sample_guided(const d3pm_shape* sh, int batch, const void* logits, int logits_dtype, const int32_t* x_t, int32_t* x_next,
                                 const d3pm_canvas* canvas, int t, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0, uint32_t flags,
                                 const d3pm_nucleus* nucleus, const d3pm_guidance* guidance, void* stream) {
  const char* who = "d3pm_posterior_sample_guided";
  D3PM_TRY(check_guidance(sh, guidance, who));
  D3PM_TRY(check_shape(sh, batch));
  D3PM_TRY(check_sampling(sh, nucleus, who));
  D3PM_REQUIRE(!(flags & D3PM_FLAG_SEED_IN_HBM), D3PM_E_ARG, "%s: D3PM_FLAG_SEED_IN_HBM (graph replay) is not supported under guidance", who);
  D3PM_REQUIRE(logits && x_t && x_next && sched && sched->d && sched->c && sched->dbar && sched->cbar, D3PM_E_ARG, "%s: null pointer", who);
  D3PM_REQUIRE(t >= 0 && t < sched->timesteps, D3PM_E_ARG, "t=%d outside the schedule", t);
  // (one level: check_guidance)
  const SampleArgs a = sample_args(*sh, batch, logits, logits_dtype, sh->n_classes, x_t, x_next, canvas ? canvas->known : nullptr, t, sched, seed,
                                   utt0, flags, nucleus, guidance);
  return posterior_sample_guided(a, static_cast<hipStream_t>(stream));
}

int d3pm_sample_loop_guided(const d3pm_shape* sh, const d3pm_weights* w, const d3pm_fp8_block_weights* fp8_blocks, int batch, int32_t* x,
                            const uint8_t* frame_mask,
                            const d3pm_canvas* canvas, int t_start, int t_stop, const void* film, const void* kv_text, const void* kv_prompt,
                            const d3pm_schedule* sched, uint64_t seed, uint32_t utt0, uint32_t flags, void* workspace, size_t workspace_bytes,
                            int32_t* trace, const d3pm_nucleus* nucleus, const d3pm_keys* keys, const d3pm_guidance* guidance, void* stream) {
  const char* who = "d3pm_sample_loop_guided";
  D3PM_TRY(check_guidance(sh, guidance, who));
  D3PM_REQUIRE((frame_mask != nullptr) != (canvas != nullptr), D3PM_E_ARG,
               "%s: give exactly one of frame_mask (shared by the batch) and canvas (per utterance)", who);
  D3PM_REQUIRE(!(flags & D3PM_FLAG_SEED_IN_HBM), D3PM_E_ARG, "%s: D3PM_FLAG_SEED_IN_HBM (graph replay) is not supported under guidance", who);
  D3PM_REQUIRE(!fp8_blocks, D3PM_E_ARG, "%s: the fp8 fast path takes no guidance", who);
  return sample_loop_impl(sh, w, batch, x, t_start, t_stop, film, kv_text, kv_prompt, sched, seed, utt0, flags, workspace, workspace_bytes, trace,
                          stream, CallOptions{who, either_mask(sh, batch, frame_mask, canvas), nullptr, nucleus, key_counts(keys), guidance});
}

// ---- per-frame log-probability of the revealed id (d3pm_frame_scores): the step entries and the D3PM loop ------------------------------
int d3pm_frame_scores_init(const d3pm_shape* sh, int batch, const int32_t* x, const uint8_t* frame_mask, const d3pm_canvas* canvas,
                           const d3pm_frame_scores* scores, void* stream) {
  const char* who = "d3pm_frame_scores_init";
  D3PM_TRY(check_scores(sh, scores, who));
  D3PM_TRY(check_shape(sh, batch));
  D3PM_REQUIRE((frame_mask != nullptr) != (canvas != nullptr), D3PM_E_ARG,
               "%s: give exactly one of frame_mask (shared by the batch) and canvas (per utterance)", who);
  D3PM_REQUIRE(x && (!canvas || canvas->frame_mask), D3PM_E_ARG, "%s: null pointer", who);
  const CanvasMask cm = either_mask(sh, batch, frame_mask, canvas);
  return frame_scores_init(x, cm.frame_mask, cm.period, cm.known, scores->logprob, scores->step, batch * sh->canvas, sh->mask_id,
                           static_cast<hipStream_t>(stream));
}

int d3pm_frame_scores_step(const d3pm_shape* sh, int batch, const void* logits, int logits_dtype, int ldl, const int32_t* row_of,
                           const d3pm_guidance* guidance, const int32_t* x_next, int t, const d3pm_frame_scores* scores, void* stream) {
  const char* who = "d3pm_frame_scores_step";
  D3PM_TRY(check_scores(sh, scores, who));
  D3PM_TRY(check_shape(sh, batch));
  if (guidance) D3PM_TRY(check_guidance(sh, guidance, who));
  D3PM_REQUIRE(logits && x_next, D3PM_E_ARG, "%s: null pointer", who);
  D3PM_REQUIRE(logits_dtype == D3PM_F32 || logits_dtype == D3PM_F16 || logits_dtype == D3PM_BF16, D3PM_E_ARG, "%s: unknown logits dtype %d", who,
               logits_dtype);
  D3PM_REQUIRE(ldl >= sh->n_classes, D3PM_E_ARG, "%s: row stride %d below n_classes %d", who, ldl, sh->n_classes);
  D3PM_REQUIRE(t >= 1 && t <= sh->timesteps, D3PM_E_ARG, "%s: t = %d outside 1 .. %d", who, t, sh->timesteps);
  D3PM_REQUIRE(!(row_of && guidance), D3PM_E_ARG, "%s: indexed logits take no guidance", who);
  D3PM_REQUIRE(!(row_of && logits_dtype == D3PM_F32), D3PM_E_ARG, "%s: indexed logits are 16-bit", who);
  return frame_logprob(logprob_args(*sh, batch * sh->canvas, logits, logits_dtype, ldl, row_of, guidance != nullptr, guidance ? guidance->weight : 0.f,
                                    x_next, t, scores),
                       static_cast<hipStream_t>(stream));
}

int d3pm_sample_loop_scored(const d3pm_shape* sh, const d3pm_weights* w, const d3pm_fp8_block_weights* fp8_blocks, int batch, int32_t* x,
                            const uint8_t* frame_mask, const d3pm_canvas* canvas, int t_start, int t_stop, const void* film, const void* kv_text,
                            const void* kv_prompt, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0, uint32_t flags, void* workspace,
                            size_t workspace_bytes, int32_t* trace, const d3pm_nucleus* nucleus, const d3pm_keys* keys, const d3pm_guidance* guidance,
                            const d3pm_frame_scores* scores, void* stream) {
  const char* who = "d3pm_sample_loop_scored";
  D3PM_TRY(check_scores(sh, scores, who));
  if (guidance) D3PM_TRY(check_guidance(sh, guidance, who));
  D3PM_REQUIRE((frame_mask != nullptr) != (canvas != nullptr), D3PM_E_ARG,
               "%s: give exactly one of frame_mask (shared by the batch) and canvas (per utterance)", who);
  D3PM_REQUIRE(!(flags & D3PM_FLAG_SEED_IN_HBM), D3PM_E_ARG, "%s: D3PM_FLAG_SEED_IN_HBM (graph replay) is not supported with frame scores", who);
  D3PM_REQUIRE(!(fp8_blocks && (keys || guidance)), D3PM_E_ARG, "%s: the fp8 fast path takes no key mask and no guidance", who);
  D3PM_REQUIRE(sh->n_classes <= 1280, D3PM_E_SHAPE, "%s: the frame scores support up to 1280 classes", who);
  CallOptions o{who, either_mask(sh, batch, frame_mask, canvas), fp8_blocks, nucleus, key_counts(keys), guidance};
  o.scores = scores;
  return sample_loop_impl(sh, w, batch, x, t_start, t_stop, film, kv_text, kv_prompt, sched, seed, utt0, flags, workspace, workspace_bytes, trace,
                          stream, o);
}

// ---- confidence-ordered reveal (d3pm_reveal) ------------------------------------------------------------------------------------------
// the timestep of plan index i of n_steps over a schedule of T timesteps: t_0 = T - 1, strictly decreasing, t_{N-1} >= 1
static int reveal_plan_t(int T, int n_steps, int i) { return (T - 1) - static_cast<int>((static_cast<long long>(i) * (T - 1)) / n_steps); }

int d3pm_reveal_plan(const d3pm_schedule* sched, int n_steps, int32_t* t_out) {
  D3PM_REQUIRE(sched && t_out, D3PM_E_ARG, "d3pm_reveal_plan: null pointer");
  const int T = sched->timesteps;
  D3PM_REQUIRE(T >= 2 && n_steps >= 1 && n_steps <= T - 1, D3PM_E_ARG, "d3pm_reveal_plan: n_steps %d outside 1 .. %d (timesteps - 1)", n_steps, T - 1);
  for (int i = 0; i < n_steps; ++i) t_out[i] = reveal_plan_t(T, n_steps, i);
  return D3PM_OK;
}

// what the reveal entries refuse before anything is launched
static int check_reveal(const d3pm_shape* sh, int batch, const d3pm_schedule* sched, float choice_temperature, uint32_t flags, const char* who) {
  D3PM_TRY(check_shape(sh, batch));
  D3PM_REQUIRE(sched && sched->cbar, D3PM_E_ARG, "%s: null schedule", who);
  D3PM_REQUIRE(std::isfinite(choice_temperature) && choice_temperature >= 0.f, D3PM_E_ARG, "%s: choice_temperature %g is not a finite number >= 0", who,
               static_cast<double>(choice_temperature));
  D3PM_REQUIRE(!(flags & D3PM_FLAG_SEED_IN_HBM), D3PM_E_ARG, "%s: D3PM_FLAG_SEED_IN_HBM belongs to the captured D3PM loop", who);
  D3PM_REQUIRE(levels(*sh) == 1, D3PM_E_SHAPE, "%s: n_q = %d; the reveal schedule is defined for n_q = 1", who, sh->n_q);
  D3PM_REQUIRE(sh->canvas <= 1024, D3PM_E_SHAPE, "%s: canvas %d; the selection supports up to 1024 frames", who, sh->canvas);
  return D3PM_OK;
}

// The two launches of the reveal step that evaluates at t and is followed by t_next (0: the last step, which keeps nothing and draws
// no v): logits rows of stride ldl.  revise (may be null): the step runs under d3pm_revise, with `scores` (may be null) the grids its
// commit resets on the rows it re-masks; a call without revise launches only the kRevise = false kernels of d3pm_reveal.hip.  The
// caller sets x_next (and the loop its trace grid).
static RevealArgs reveal_args(const d3pm_shape& sh, int batch, const void* logits, int logits_dtype, int ldl, const int32_t* x_t, const CanvasMask& cm,
                              int32_t* cand, float* score, int t, int t_next, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                              uint32_t flags, const d3pm_nucleus* nucleus, float choice_temperature, const d3pm_revise* revise,
                              const d3pm_frame_scores* scores) {
  RevealArgs a;
  a.logits = logits; a.logits_dtype = logits_dtype; a.ldl = ldl; a.x_t = x_t;
  a.frame_mask = cm.frame_mask; a.mask_period = cm.period; a.known = cm.known; a.cand = cand; a.score = score;
  a.rows = batch * sh.canvas; a.canvas = sh.canvas; a.n_classes = sh.n_classes; a.mask_id = sh.mask_id;
  a.seed = seed; a.row0 = utt0 * static_cast<uint32_t>(sh.canvas); a.greedy = (flags & D3PM_FLAG_GREEDY) ? 1 : 0;
  if (nucleus) { a.temperature = nucleus->temperature; a.top_k = nucleus->top_k; a.top_p = nucleus->top_p; }
  a.t = t;
  a.keep_frac = t_next > 0 ? host_h2f(sched->cbar[t_next]) : 0.f;
  a.lambda = t_next > 0 ? choice_temperature * a.keep_frac : 0.f;
  if (revise) {
    a.revise = true; a.hold_bonus = revise->hold_bonus;
    if (scores) { a.logprob = scores->logprob; a.step = scores->step; }
  }
  return a;
}

// d3pm_reveal_step (revise and scores null) and d3pm_reveal_step_revise, which has run check_revise
static int reveal_step_impl(const d3pm_shape* sh, int batch, const void* logits, int logits_dtype, const int32_t* x_t, int32_t* x_next,
                            const uint8_t* frame_mask, const d3pm_canvas* canvas, int t, int t_next, const d3pm_schedule* sched, uint64_t seed,
                            uint32_t utt0, uint32_t flags, const d3pm_nucleus* nucleus, float choice_temperature, int32_t* cand_out, float* score_out,
                            const d3pm_revise* revise, const d3pm_frame_scores* scores, void* stream, const char* who) {
  D3PM_TRY(check_reveal(sh, batch, sched, choice_temperature, flags, who));
  D3PM_TRY(check_sampling(sh, nucleus, who));
  if (scores) D3PM_TRY(check_scores(sh, scores, who));
  D3PM_REQUIRE((frame_mask != nullptr) != (canvas != nullptr), D3PM_E_ARG,
               "%s: give exactly one of frame_mask (shared by the batch) and canvas (per utterance)", who);
  D3PM_REQUIRE(logits && x_t && x_next && cand_out && score_out && (!canvas || canvas->frame_mask), D3PM_E_ARG, "%s: null pointer", who);
  D3PM_REQUIRE(t >= 1 && t < sched->timesteps && t_next >= 0 && t_next < t, D3PM_E_ARG, "%s: t = %d, t_next = %d outside %d > t > t_next >= 0", who, t,
               t_next, sched->timesteps);
  RevealArgs a = reveal_args(*sh, batch, logits, logits_dtype, sh->n_classes, x_t, either_mask(sh, batch, frame_mask, canvas), cand_out, score_out, t,
                             t_next, sched, seed, utt0, flags, nucleus, choice_temperature, revise, scores);
  a.x_next = x_next;
  hipStream_t s = static_cast<hipStream_t>(stream);
  D3PM_TRY(reveal_candidates(a, s));
  return reveal_commit(a, s);
}

int d3pm_reveal_step(const d3pm_shape* sh, int batch, const void* logits, int logits_dtype, const int32_t* x_t, int32_t* x_next,
                     const uint8_t* frame_mask, const d3pm_canvas* canvas, int t, int t_next, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                     uint32_t flags, const d3pm_nucleus* nucleus, float choice_temperature, int32_t* cand_out, float* score_out, void* stream) {
  return reveal_step_impl(sh, batch, logits, logits_dtype, x_t, x_next, frame_mask, canvas, t, t_next, sched, seed, utt0, flags, nucleus,
                          choice_temperature, cand_out, score_out, nullptr, nullptr, stream, "d3pm_reveal_step");
}

// what the entries that take d3pm_revise refuse before anything else is looked at
static int check_revise(const d3pm_revise* revise, const char* who) {
  D3PM_REQUIRE(revise, D3PM_E_ARG, "%s: null d3pm_revise", who);
  D3PM_REQUIRE(std::isfinite(revise->hold_bonus) && revise->hold_bonus >= 0.f, D3PM_E_ARG, "%s: hold_bonus %g is not a finite number >= 0", who,
               static_cast<double>(revise->hold_bonus));
  return D3PM_OK;
}

// d3pm_reveal_step under d3pm_revise (include/d3pm_hip.h, "reveal with revision")
int d3pm_reveal_step_revise(const d3pm_shape* sh, int batch, const void* logits, int logits_dtype, const int32_t* x_t, int32_t* x_next,
                            const uint8_t* frame_mask, const d3pm_canvas* canvas, int t, int t_next, const d3pm_schedule* sched, uint64_t seed,
                            uint32_t utt0, uint32_t flags, const d3pm_nucleus* nucleus, float choice_temperature, int32_t* cand_out, float* score_out,
                            const d3pm_revise* revise, const d3pm_frame_scores* scores, void* stream) {
  D3PM_TRY(check_revise(revise, "d3pm_reveal_step_revise"));
  return reveal_step_impl(sh, batch, logits, logits_dtype, x_t, x_next, frame_mask, canvas, t, t_next, sched, seed, utt0, flags, nucleus,
                          choice_temperature, cand_out, score_out, revise, scores, stream, "d3pm_reveal_step_revise");
}

// o.reveal: the plan; o.revise (null but for d3pm_reveal_loop_revise): every step runs under d3pm_revise; o.scores: the launch behind every
// commit; o.who: the entry.  o.mask is not used: the loop takes frame_mask / canvas as the entry received them, behind its own checks.
static int reveal_loop_impl(const d3pm_shape* sh, const d3pm_weights* w, int batch, int32_t* x, const uint8_t* frame_mask, const d3pm_canvas* canvas,
                            const void* film, const void* kv_text, const void* kv_prompt, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                            uint32_t flags, void* workspace, size_t workspace_bytes, int32_t* trace, void* stream, const CallOptions& o) {
  const d3pm_reveal* reveal = o.reveal;
  const d3pm_frame_scores* scores = o.scores;
  // (an entry that passes scores has run check_scores on them) the launch behind every commit reads whole rows of logits, d3pm_logprob.hip
  D3PM_REQUIRE(!scores || sh->n_classes <= 1280, D3PM_E_SHAPE, "%s: the frame scores support up to 1280 classes", o.who);
  D3PM_REQUIRE(reveal, D3PM_E_ARG, "d3pm_reveal_loop: null d3pm_reveal");
  D3PM_TRY(check_reveal(sh, batch, sched, reveal->choice_temperature, flags, "d3pm_reveal_loop"));
  D3PM_TRY(check_sampling(sh, o.nucleus, "d3pm_reveal_loop"));
  const int T = sched->timesteps, N = reveal->n_steps;
  D3PM_REQUIRE(N >= 1 && N <= T - 1 && T - 1 <= sh->timesteps, D3PM_E_ARG, "d3pm_reveal_loop: n_steps %d outside 1 .. %d (timesteps - 1)", N, T - 1);
  D3PM_REQUIRE((frame_mask != nullptr) != (canvas != nullptr), D3PM_E_ARG,
               "d3pm_reveal_loop: give exactly one of frame_mask (shared by the batch) and canvas (per utterance)");
  D3PM_REQUIRE(w && w->blocks && x && film && kv_text && kv_prompt && workspace && (!canvas || canvas->frame_mask), D3PM_E_ARG, "d3pm_reveal_loop: null pointer");
  Workspace ws = carve(*sh, batch, static_cast<char*>(workspace));
  D3PM_REQUIRE(workspace_bytes >= ws.total, D3PM_E_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, ws.total);
  const int rows = batch * sh->canvas;
  const size_t es = dtype_size(sh->dtype);
  // candidates and scores live in the attention-output region, dead behind the last block.  The second id grid of the fused launch has
  // to survive the next evaluation: it takes the fp8 path's scale slot, which a 16-bit evaluation never touches (2 d / 32 >= 16 bytes
  // per row wherever the fused launch applies, d a multiple of 256).
  D3PM_REQUIRE(static_cast<size_t>(sh->d_model) * es >= 2 * sizeof(int32_t), D3PM_E_SHAPE, "d3pm_reveal_loop: d_model %d too small", sh->d_model);
  int32_t* cand = reinterpret_cast<int32_t*>(ws.att);
  float* score = reinterpret_cast<float*>(ws.att) + rows;
  int32_t* x_alt = reinterpret_cast<int32_t*>(ws.mxs);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CanvasMask cm = either_mask(sh, batch, frame_mask, canvas);
  const Ctx cx(sh->tuning);
  const DenoiserArgs q{*sh, *w, batch, cm.frame_mask, cm.period, kv_text, kv_prompt, ws, o.keys};
  // Asked as for one evaluation: the reveal loop keeps the block-0 QKV projection and every row (reveal_commit_prep does not gather
  // from the table), so the moment format is all it plans.
  const int plan = loop_plan(q, flags, LoopCall{}).fold;
  if (scores) D3PM_TRY(frame_scores_init(x, cm.frame_mask, cm.period, cm.known, scores->logprob, scores->step, rows, sh->mask_id, s));
  bool prepared = false;
  int32_t* cur = x;      // where x_t of the step lives: the fused launch cannot store in place, so it alternates between x and x_alt
  for (int i = 0; i < N; ++i) {
    const int t = reveal_plan_t(T, N, i), t_next = i + 1 < N ? reveal_plan_t(T, N, i + 1) : 0;
    if (cx.prof) cx.prof->sample_now = (t % cx.prof->stride) == 0;
    D3PM_TRY(denoiser_blocks(q, cur, t, film, sh->n_layers, flags, s, nullptr, plan, prepared));
    prepared = false;
    D3PM_TRY(final_logits(*sh, *w, batch, ws, ws.logits, logits_ld(*sh), flags, s));
    RevealArgs a = reveal_args(*sh, batch, ws.logits, sh->dtype, logits_ld(*sh), cur, cm, cand, score, t, t_next, sched, seed, utt0, flags, o.nucleus,
                               reveal->choice_temperature, o.revise, scores);
    a.x_next2 = trace ? trace + static_cast<size_t>(i) * rows : nullptr;
    {
      ProfScope p(cx, D3PM_K_SAMPLE, s, 0.0, static_cast<double>(rows) * (sh->n_classes * es + 16.0));
      D3PM_TRY(reveal_candidates(a, s));
      const NextIterPrep nx = t_next > 0 && plan != FOLD_NONE ? next_iter_prep(q, film, t_next, plan == FOLD_QUADS) : NextIterPrep{};
      a.x_next = cur == x ? x_alt : x;
      if (nx.table && reveal_commit_prep_supported(a, nx)) {
        D3PM_TRY(reveal_commit_prep(a, nx, s));      // + the embedding rows, their moments and the fc1 fold of t_next
        prepared = true;
      } else {
        a.x_next = x;      // one wave per utterance: in place when cur is x, else back into x
        D3PM_TRY(reveal_commit(a, s));
      }
      cur = a.x_next;
    }
    // (d3pm_reveal_loop_scored) behind the commit, on the grid it wrote: the rows this step revealed
    if (scores) D3PM_TRY(run_frame_logprob(cx, logprob_args(*sh, rows, ws.logits, sh->dtype, logits_ld(*sh), nullptr, false, 0.f, a.x_next, t, scores), s));
  }
  if (cx.prof) cx.prof->sample_now = false;
  return D3PM_OK;      // the last step is never fused (no next evaluation): the result is in x
}

// what the reveal loop's entries fill of CallOptions: {who, -, -, nucleus, keys, -, -, scores, reveal, revise}
int d3pm_reveal_loop(const d3pm_shape* sh, const d3pm_weights* w, int batch, int32_t* x, const uint8_t* frame_mask, const d3pm_canvas* canvas,
                     const void* film, const void* kv_text, const void* kv_prompt, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0, uint32_t flags,
                     void* workspace, size_t workspace_bytes, int32_t* trace, const d3pm_nucleus* nucleus, const d3pm_reveal* reveal, void* stream) {
  return reveal_loop_impl(sh, w, batch, x, frame_mask, canvas, film, kv_text, kv_prompt, sched, seed, utt0, flags, workspace, workspace_bytes, trace,
                          stream, CallOptions{"d3pm_reveal_loop", {}, nullptr, nucleus, KeyCounts{}, nullptr, nullptr, nullptr, reveal, nullptr});
}

int d3pm_reveal_loop_keys(const d3pm_shape* sh, const d3pm_weights* w, int batch, int32_t* x, const uint8_t* frame_mask, const d3pm_canvas* canvas,
                          const void* film, const void* kv_text, const void* kv_prompt, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                          uint32_t flags, void* workspace, size_t workspace_bytes, int32_t* trace, const d3pm_nucleus* nucleus,
                          const d3pm_reveal* reveal, const d3pm_keys* keys, void* stream) {
  return reveal_loop_impl(sh, w, batch, x, frame_mask, canvas, film, kv_text, kv_prompt, sched, seed, utt0, flags, workspace, workspace_bytes, trace,
                          stream, CallOptions{"d3pm_reveal_loop_keys", {}, nullptr, nucleus, key_counts(keys), nullptr, nullptr, nullptr, reveal, nullptr});
}

int d3pm_reveal_loop_scored(const d3pm_shape* sh, const d3pm_weights* w, int batch, int32_t* x, const uint8_t* frame_mask, const d3pm_canvas* canvas,
                            const void* film, const void* kv_text, const void* kv_prompt, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                            uint32_t flags, void* workspace, size_t workspace_bytes, int32_t* trace, const d3pm_nucleus* nucleus,
                            const d3pm_reveal* reveal, const d3pm_keys* keys, const d3pm_frame_scores* scores, void* stream) {
  const char* who = "d3pm_reveal_loop_scored";
  D3PM_TRY(check_scores(sh, scores, who));
  return reveal_loop_impl(sh, w, batch, x, frame_mask, canvas, film, kv_text, kv_prompt, sched, seed, utt0, flags, workspace, workspace_bytes, trace,
                          stream, CallOptions{who, {}, nullptr, nucleus, key_counts(keys), nullptr, nullptr, scores, reveal, nullptr});
}

// d3pm_reveal_loop_scored under d3pm_revise (include/d3pm_hip.h, "reveal with revision"); keys and scores optional
int d3pm_reveal_loop_revise(const d3pm_shape* sh, const d3pm_weights* w, int batch, int32_t* x, const uint8_t* frame_mask, const d3pm_canvas* canvas,
                            const void* film, const void* kv_text, const void* kv_prompt, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0,
                            uint32_t flags, void* workspace, size_t workspace_bytes, int32_t* trace, const d3pm_nucleus* nucleus,
                            const d3pm_reveal* reveal, const d3pm_keys* keys, const d3pm_revise* revise, const d3pm_frame_scores* scores,
                            void* stream) {
  const char* who = "d3pm_reveal_loop_revise";
  D3PM_TRY(check_revise(revise, who));
  if (scores) D3PM_TRY(check_scores(sh, scores, who));
  return reveal_loop_impl(sh, w, batch, x, frame_mask, canvas, film, kv_text, kv_prompt, sched, seed, utt0, flags, workspace, workspace_bytes, trace,
                          stream, CallOptions{who, {}, nullptr, nucleus, key_counts(keys), nullptr, nullptr, scores, reveal, revise});
}

int d3pm_q_sample(const d3pm_shape* sh, int batch, const int32_t* x0, int32_t* x_out, const uint8_t* frame_mask, int t,
                  const d3pm_schedule* sched, uint64_t seed, uint32_t utt0, void* stream) {
  D3PM_TRY(check_shape(sh, batch));
  D3PM_REQUIRE(x0 && x_out && frame_mask && sched && sched->dbar && sched->cbar, D3PM_E_ARG, "d3pm_q_sample: null pointer");
  D3PM_REQUIRE(levels(*sh) == 1, D3PM_E_SHAPE, "d3pm_q_sample: the training side covers the upstream level-0 model only (n_q = 1)");
  D3PM_REQUIRE(t >= 0 && t < sched->timesteps, D3PM_E_ARG, "t=%d outside the schedule", t);
  return q_sample_launch(sh, batch, x0, x_out, frame_mask, t, sched, seed, utt0, static_cast<hipStream_t>(stream));
}

int d3pm_ce_loss_rows(const d3pm_shape* sh, int batch, const void* logits, int logits_dtype, const int32_t* targets,
                      const uint8_t* frame_mask, float* row_loss, void* stream) {
  D3PM_TRY(check_shape(sh, batch));
  D3PM_REQUIRE(logits && targets && frame_mask && row_loss, D3PM_E_ARG, "d3pm_ce_loss_rows: null pointer");
  D3PM_REQUIRE(levels(*sh) == 1, D3PM_E_SHAPE, "d3pm_ce_loss_rows: the training side covers the upstream level-0 model only (n_q = 1)");
  return ce_loss_launch(logits_dtype, logits, sh->n_classes, targets, frame_mask, sh->canvas, batch * sh->canvas,
                        sh->n_classes, row_loss, static_cast<hipStream_t>(stream));
}

int d3pm_uniform(uint64_t seed, int t, uint32_t row0, int rows, int n_classes, int stream_id, float* out, void* stream) {
  D3PM_REQUIRE(out && rows > 0 && n_classes > 0, D3PM_E_ARG, "d3pm_uniform: bad arguments");
  return uniform_launch(seed, t, row0, rows, n_classes, stream_id, out, static_cast<hipStream_t>(stream));
}

// ---- stock NAR model -------------------------------------------------------------------------------------
struct NarWs { char *x, *h, *qkv, *att, *ffn, *logits; uint8_t* mask; int32_t* key_len; size_t total; };
static NarWs carve_nar(const d3pm_nar_shape& sh, int batch, int t_max, char* base) {
  const size_t es = dtype_size(sh.dtype), n = static_cast<size_t>(batch) * t_max, d = sh.d_model;
  NarWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
  w.x = take(n * d * es);
  w.h = take(n * d * es);
  w.qkv = take(n * 3 * d * es);
  w.att = take(n * d * es);
  w.ffn = take(n * 4 * d * es);
  w.logits = take(n * sh.n_tokens * es);
  w.mask = reinterpret_cast<uint8_t*>(take(n));
  w.key_len = reinterpret_cast<int32_t*>(take(static_cast<size_t>(batch) * 4));
  w.total = off;
  return w;
}
static int check_nar(const d3pm_nar_shape* sh, int batch, int t_max) {
  D3PM_REQUIRE(sh && batch > 0 && t_max > 0 && sh->d_model > 0 && sh->n_heads > 0 && sh->d_model % sh->n_heads == 0 &&
                   sh->n_layers > 0 && sh->n_tokens > 1 && sh->n_prom_levels > 0 && sh->n_resp_levels > 0,
               D3PM_E_ARG, "inconsistent d3pm_nar_shape");
  D3PM_REQUIRE(sh->dtype == D3PM_F32 || sh->dtype == D3PM_F16 || sh->dtype == D3PM_BF16, D3PM_E_ARG, "bad dtype %d", sh->dtype);
  return D3PM_OK;
}

size_t d3pm_nar_workspace_bytes(const d3pm_nar_shape* sh, int batch, int t_max) {
  if (check_nar(sh, batch, t_max) != D3PM_OK) return 0;
  return carve_nar(*sh, batch, t_max, nullptr).total;
}

// d3pm_nar_draw: validated, then `opt` = the kernel's arguments and `neutral` = whether the call is the draw without options
static int check_nar_draw(const char* who, const d3pm_nar_draw* draw, float temperature, int n_tokens, NarDrawArgs* opt, bool* neutral) {
  D3PM_REQUIRE(std::isfinite(temperature) && temperature > 0.f, D3PM_E_ARG, "%s: temperature must be finite and > 0", who);
  *neutral = true;
  if (!draw) return D3PM_OK;
  D3PM_REQUIRE(draw->top_k >= 0 && draw->top_k <= n_tokens, D3PM_E_ARG, "%s: top_k %d outside 0 .. %d", who, draw->top_k, n_tokens);
  D3PM_REQUIRE(std::isfinite(draw->top_p) && draw->top_p > 0.f && draw->top_p <= 1.f, D3PM_E_ARG, "%s: top_p must be within (0, 1]", who);
  opt->top_p = draw->top_p; opt->top_k = draw->top_k; opt->known = draw->known; opt->logprob_out = draw->logprob_out;
  opt->theta_out = draw->theta_out;
  *neutral = draw->top_p == 1.0f && draw->top_k == 0 && !draw->known && !draw->logprob_out && !draw->theta_out;
  return D3PM_OK;
}

static int nar_level_run(const char* who, const d3pm_nar_shape* sh, const d3pm_nar_weights* w, int batch, int t_max, const int32_t* lens,
                         const int32_t* text, int tt_max, const int32_t* prom, int tp_max, int32_t* resp, int tr_max, int level,
                         float temperature, uint64_t seed, uint32_t utt0, uint32_t flags, void* workspace, size_t workspace_bytes,
                         void* logits_out, const NarDrawArgs* draw, void* stream, const float* guidance = nullptr) {
  // guidance: `batch` counts the 2 * logical utterances of the evaluation and the draw pairs utterance b with batch / 2 + b
  D3PM_TRY(check_nar(sh, batch, t_max));
  D3PM_REQUIRE(w && w->blocks && w->text_emb && w->proms_emb && w->resps_emb && w->sep && w->classifier_w && w->classifier_b &&
                   w->pe && lens && text && prom && resp && workspace,
               D3PM_E_ARG, "%s: null pointer", who);
  D3PM_REQUIRE(level >= 0 && level < sh->n_resp_levels && temperature > 0.f && w->pe_rows >= t_max && tt_max > 0 && tp_max > 0 &&
                   tr_max > 0,
               D3PM_E_ARG, "%s: bad level / temperature / sizes", who);
  NarWs ws = carve_nar(*sh, batch, t_max, static_cast<char*>(workspace));
  D3PM_REQUIRE(workspace_bytes >= ws.total, D3PM_E_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, ws.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int dt = sh->dtype, d = sh->d_model, n = batch * t_max, hd = d / sh->n_heads, stride = sh->n_resp_levels + 1;
  const size_t es = dtype_size(dt);
  const Ctx cx(sh->tuning);

  NarEmbedArgs e;
  e.lens = lens; e.text = text; e.tt_max = tt_max; e.prom = prom; e.tp_max = tp_max; e.n_prom_levels = sh->n_prom_levels;
  e.resp = resp; e.tr_max = tr_max; e.resp_stride = stride; e.n_given = level + 1;
  e.w_text = w->text_emb; e.w_prom = w->proms_emb; e.w_resp = w->resps_emb; e.sep = w->sep; e.pe = w->pe;
  e.x = ws.x; e.row_mask = ws.mask; e.key_len = ws.key_len; e.batch = batch; e.t_max = t_max; e.d = d; e.n_tokens = sh->n_tokens;
  D3PM_TRY(nar_embed(dt, e, s));

  for (int l = 0; l < sh->n_layers; ++l) {
    const d3pm_nar_block_weights& b = w->blocks[l];
    // x = (x + to_out(attention(AdaLN(x) * m)) * m) * m
    D3PM_TRY(adaln(dt, ws.x, ws.h, at(b.attn_norm_emb, static_cast<size_t>(level) * 2 * d, es), ws.mask, n, d, s));
    D3PM_TRY(run_linear(cx, dt, projection(ws.h, b.to_qkv_w, nullptr, ws.qkv, n, 3 * d, d), flags, s));
    AttnArgs a = self_attention(ws.qkv, ws.att, batch, t_max, sh->n_heads, hd, es);
    a.scale = 1.0f / std::sqrt(static_cast<float>(hd));      // rounded as the stock model rounds it
    a.key_len = ws.key_len;
    D3PM_TRY(run_attention(cx, dt, a, flags, s));
    D3PM_TRY(run_linear(cx, dt, with_row_mask(with_residual(projection(ws.att, b.to_out_w, b.to_out_b, ws.x, n, d, d), ws.x), ws.mask, n), flags, s));
    // x = (x + ffn(AdaLN(x) * m)) * m
    D3PM_TRY(adaln(dt, ws.x, ws.h, at(b.ffn_norm_emb, static_cast<size_t>(level) * 2 * d, es), ws.mask, n, d, s));
    D3PM_TRY(run_linear(cx, dt, projection(ws.h, b.ffn0_w, b.ffn0_b, ws.ffn, n, 4 * d, d, ACT_GELU), flags, s));
    D3PM_TRY(run_linear(cx, dt, with_row_mask(with_residual(projection(ws.ffn, b.ffn3_w, b.ffn3_b, ws.x, n, d, 4 * d), ws.x), ws.mask, n), flags, s));
  }
  D3PM_TRY(run_linear(cx, dt, projection(ws.x, w->classifier_w, w->classifier_b, ws.logits, n, sh->n_tokens, d), flags, s));
  if (logits_out)
    D3PM_CHECK_HIP(hipMemcpyAsync(logits_out, ws.logits, static_cast<size_t>(n) * sh->n_tokens * es, hipMemcpyDeviceToDevice, s));
  if (draw)
    return nar_draw(dt, ws.logits, sh->n_tokens, lens, resp, tr_max, stride, t_max, sh->n_tokens, level, temperature, seed, utt0,
                    (flags & D3PM_FLAG_GREEDY) ? 1 : 0, guidance ? batch / 2 : batch, *draw, s, guidance);
  return nar_sample(dt, ws.logits, sh->n_tokens, lens, resp, tr_max, stride, t_max, sh->n_tokens, level, temperature, seed, utt0,
                    (flags & D3PM_FLAG_GREEDY) ? 1 : 0, batch, s);
}

int d3pm_nar_level(const d3pm_nar_shape* sh, const d3pm_nar_weights* w, int batch, int t_max, const int32_t* lens,
                   const int32_t* text, int tt_max, const int32_t* prom, int tp_max, int32_t* resp, int tr_max, int level,
                   float temperature, uint64_t seed, uint32_t utt0, uint32_t flags, void* workspace, size_t workspace_bytes,
                   void* logits_out, void* stream) {
  return nar_level_run("d3pm_nar_level", sh, w, batch, t_max, lens, text, tt_max, prom, tp_max, resp, tr_max, level, temperature, seed,
                       utt0, flags, workspace, workspace_bytes, logits_out, nullptr, stream);
}

int d3pm_nar_level_draw(const d3pm_nar_shape* sh, const d3pm_nar_weights* w, int batch, int t_max, const int32_t* lens,
                        const int32_t* text, int tt_max, const int32_t* prom, int tp_max, int32_t* resp, int tr_max, int level,
                        float temperature, uint64_t seed, uint32_t utt0, uint32_t flags, void* workspace, size_t workspace_bytes,
                        void* logits_out, const d3pm_nar_draw* draw, void* stream) {
  D3PM_TRY(check_nar(sh, batch, t_max));
  NarDrawArgs opt;
  bool neutral = true;
  D3PM_TRY(check_nar_draw("d3pm_nar_level_draw", draw, temperature, sh->n_tokens, &opt, &neutral));
  D3PM_REQUIRE(neutral || sh->n_tokens <= 1280, D3PM_E_SHAPE, "d3pm_nar_level_draw: the draw with options supports up to 1280 tokens");
  return nar_level_run("d3pm_nar_level_draw", sh, w, batch, t_max, lens, text, tt_max, prom, tp_max, resp, tr_max, level, temperature,
                       seed, utt0, flags, workspace, workspace_bytes, logits_out, neutral ? nullptr : &opt, stream);
}

// d3pm_guidance for the NAR stage: any n_q (the levels are drawn one at a time), the draw kernel's token limit always
static int check_nar_guidance(const char* who, const d3pm_guidance* g, int batch, int n_tokens) {
  D3PM_REQUIRE(g, D3PM_E_ARG, "%s: null d3pm_guidance", who);
  D3PM_REQUIRE(std::isfinite(g->weight) && g->weight >= 0.f, D3PM_E_ARG, "%s: guidance weight %g is not a finite number >= 0", who,
               static_cast<double>(g->weight));
  D3PM_REQUIRE(batch > 0 && batch <= (1 << 30), D3PM_E_ARG, "%s: batch %d (logical utterances) out of range", who, batch);
  D3PM_REQUIRE(n_tokens <= 1280, D3PM_E_SHAPE, "%s: the guided draw supports up to 1280 tokens", who);
  return D3PM_OK;
}

int d3pm_nar_level_guided(const d3pm_nar_shape* sh, const d3pm_nar_weights* w, int batch, int t_max, const int32_t* lens,
                          const int32_t* text, int tt_max, const int32_t* prom, int tp_max, int32_t* resp, int tr_max, int level,
                          float temperature, uint64_t seed, uint32_t utt0, uint32_t flags, void* workspace, size_t workspace_bytes,
                          void* logits_out, const d3pm_nar_draw* draw, const d3pm_guidance* guidance, void* stream) {
  const char* who = "d3pm_nar_level_guided";
  D3PM_TRY(check_nar(sh, batch, t_max));
  NarDrawArgs opt;
  bool neutral = true;
  D3PM_TRY(check_nar_draw(who, draw, temperature, sh->n_tokens, &opt, &neutral));
  D3PM_TRY(check_nar_guidance(who, guidance, batch, sh->n_tokens));
  // every guided draw is the kernel of d3pm_nar_draw.hip, with the neutral options where none is set
  return nar_level_run(who, sh, w, 2 * batch, t_max, lens, text, tt_max, prom, tp_max, resp, tr_max, level, temperature, seed, utt0, flags,
                       workspace, workspace_bytes, logits_out, &opt, stream, &guidance->weight);
}

// the three kernels of the stage one at a time (tests): host validation, then the call d3pm_nar_level makes
static bool storage_dtype(int dtype) { return dtype == D3PM_F32 || dtype == D3PM_F16 || dtype == D3PM_BF16; }

int d3pm_op_nar_embed(int dtype, const int32_t* lens, const int32_t* text, int tt_max, const int32_t* prom, int tp_max, int n_prom_levels,
                      const int32_t* resp, int tr_max, int resp_stride, int n_given, const void* w_text, const void* w_prom,
                      const void* w_resp, const void* sep, const void* pe, void* x, uint8_t* row_mask, int32_t* key_len, int batch,
                      int t_max, int d, int n_tokens, void* stream) {
  D3PM_REQUIRE(storage_dtype(dtype), D3PM_E_ARG, "d3pm_op_nar_embed: bad dtype %d", dtype);
  D3PM_REQUIRE(lens && text && prom && resp && w_text && w_prom && w_resp && sep && pe && x && row_mask && key_len, D3PM_E_ARG,
               "d3pm_op_nar_embed: null pointer");
  D3PM_REQUIRE(batch > 0 && t_max > 0 && tt_max > 0 && tp_max > 0 && tr_max > 0 && d > 0 && n_tokens > 0 && n_prom_levels > 0 &&
                   n_given >= 1 && n_given <= resp_stride,
               D3PM_E_ARG, "d3pm_op_nar_embed: sizes must be positive and 1 <= n_given <= resp_stride");
  NarEmbedArgs e;
  e.lens = lens; e.text = text; e.tt_max = tt_max; e.prom = prom; e.tp_max = tp_max; e.n_prom_levels = n_prom_levels;
  e.resp = resp; e.tr_max = tr_max; e.resp_stride = resp_stride; e.n_given = n_given;
  e.w_text = w_text; e.w_prom = w_prom; e.w_resp = w_resp; e.sep = sep; e.pe = pe;
  e.x = x; e.row_mask = row_mask; e.key_len = key_len; e.batch = batch; e.t_max = t_max; e.d = d; e.n_tokens = n_tokens;
  return nar_embed(dtype, e, static_cast<hipStream_t>(stream));
}

int d3pm_op_adaln(int dtype, const void* x, void* y, const void* emb_row, const uint8_t* row_mask, int M, int d, void* stream) {
  D3PM_REQUIRE(storage_dtype(dtype), D3PM_E_ARG, "d3pm_op_adaln: bad dtype %d", dtype);
  D3PM_REQUIRE(x && y && emb_row && row_mask && M > 0 && d > 0, D3PM_E_ARG, "d3pm_op_adaln: bad arguments");
  return adaln(dtype, x, y, emb_row, row_mask, M, d, static_cast<hipStream_t>(stream));
}

int d3pm_op_nar_sample(int dtype, const void* logits, int ldl, const int32_t* lens, int32_t* resp, int tr_max, int resp_stride, int t_max,
                       int n_tokens, int level, float temperature, uint64_t seed, uint32_t utt0, uint32_t flags, int batch, void* stream) {
  D3PM_REQUIRE(storage_dtype(dtype), D3PM_E_ARG, "d3pm_op_nar_sample: bad dtype %d", dtype);
  D3PM_REQUIRE(logits && lens && resp, D3PM_E_ARG, "d3pm_op_nar_sample: null pointer");
  D3PM_REQUIRE(batch > 0 && t_max > 0 && tr_max > 0 && n_tokens > 0 && ldl >= n_tokens && level >= 0 && level + 1 < resp_stride &&
                   temperature > 0.f,
               D3PM_E_ARG, "d3pm_op_nar_sample: sizes must be positive, ldl >= n_tokens, 0 <= level < resp_stride - 1, temperature > 0");
  return nar_sample(dtype, logits, ldl, lens, resp, tr_max, resp_stride, t_max, n_tokens, level, temperature, seed, utt0,
                    (flags & D3PM_FLAG_GREEDY) ? 1 : 0, batch, static_cast<hipStream_t>(stream));
}

int d3pm_op_nar_draw(int dtype, const void* logits, int ldl, const int32_t* lens, int32_t* resp, int tr_max, int resp_stride, int t_max,
                     int n_tokens, int level, float temperature, uint64_t seed, uint32_t utt0, uint32_t flags, int batch,
                     const d3pm_nar_draw* draw, void* stream) {
  D3PM_REQUIRE(storage_dtype(dtype), D3PM_E_ARG, "d3pm_op_nar_draw: bad dtype %d", dtype);
  D3PM_REQUIRE(logits && lens && resp, D3PM_E_ARG, "d3pm_op_nar_draw: null pointer");
  D3PM_REQUIRE(batch > 0 && t_max > 0 && tr_max > 0 && n_tokens > 0 && ldl >= n_tokens && level >= 0 && level + 1 < resp_stride,
               D3PM_E_ARG, "d3pm_op_nar_draw: sizes must be positive, ldl >= n_tokens, 0 <= level < resp_stride - 1");
  NarDrawArgs opt;
  bool neutral = true;
  D3PM_TRY(check_nar_draw("d3pm_op_nar_draw", draw, temperature, n_tokens, &opt, &neutral));
  const int greedy = (flags & D3PM_FLAG_GREEDY) ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (neutral) return nar_sample(dtype, logits, ldl, lens, resp, tr_max, resp_stride, t_max, n_tokens, level, temperature, seed, utt0, greedy, batch, s);
  return nar_draw(dtype, logits, ldl, lens, resp, tr_max, resp_stride, t_max, n_tokens, level, temperature, seed, utt0, greedy, batch, opt, s);
}

int d3pm_op_nar_draw_guided(int dtype, const void* logits, int ldl, const int32_t* lens, int32_t* resp, int tr_max, int resp_stride,
                            int t_max, int n_tokens, int level, float temperature, uint64_t seed, uint32_t utt0, uint32_t flags, int batch,
                            const d3pm_nar_draw* draw, const d3pm_guidance* guidance, void* stream) {
  const char* who = "d3pm_op_nar_draw_guided";
  D3PM_REQUIRE(storage_dtype(dtype), D3PM_E_ARG, "%s: bad dtype %d", who, dtype);
  D3PM_REQUIRE(logits && lens && resp, D3PM_E_ARG, "%s: null pointer", who);
  D3PM_REQUIRE(batch > 0 && t_max > 0 && tr_max > 0 && n_tokens > 0 && ldl >= n_tokens && level >= 0 && level + 1 < resp_stride,
               D3PM_E_ARG, "%s: sizes must be positive, ldl >= n_tokens, 0 <= level < resp_stride - 1", who);
  NarDrawArgs opt;
  bool neutral = true;
  D3PM_TRY(check_nar_draw(who, draw, temperature, n_tokens, &opt, &neutral));
  D3PM_TRY(check_nar_guidance(who, guidance, batch, n_tokens));
  return nar_draw(dtype, logits, ldl, lens, resp, tr_max, resp_stride, t_max, n_tokens, level, temperature, seed, utt0,
                  (flags & D3PM_FLAG_GREEDY) ? 1 : 0, batch, opt, static_cast<hipStream_t>(stream), &guidance->weight);
}

int d3pm_op_linear(int dtype, int family, const void* X, int ldx, const void* W, const void* bias, void* Y, int ldy,
                   const void* R1, const void* R2, int ldr, const uint8_t* row_mask, int mask_period, int M, int N, int K,
                   int act, const d3pm_tuning* tuning, void* stream) {
  D3PM_REQUIRE(X && W && Y && M > 0 && N > 0 && K > 0, D3PM_E_ARG, "d3pm_op_linear: bad arguments");
  const Ctx cx(tuning);
  LinearArgs g;
  g.tune = tuning;
  g.X = X; g.ldx = ldx; g.W = W; g.bias = bias; g.Y = Y; g.ldy = ldy; g.R1 = R1; g.R2 = R2; g.ldr = ldr;
  g.row_mask = row_mask; g.mask_period = mask_period > 0 ? mask_period : 1; g.M = M; g.N = N; g.K = K; g.act = act;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (family == 1) return generic_linear(dtype, g, s);
  if (family == 2) {
    const LinearPlan plan = plan_linear(dtype, g);
    D3PM_REQUIRE(plan.mfma(), D3PM_E_SHAPE, "d3pm_op_linear: shape not supported by the MFMA kernel");
    return mfma_linear(dtype, g, plan, s);
  }
  return run_linear(cx, dtype, g, 0, s);
}

int d3pm_op_quantize_mx(int dtype, const void* X, int ldx, void* X8, void* SX, int M, int K, void* stream) {
  D3PM_REQUIRE(X && X8 && SX && M > 0 && K > 0, D3PM_E_ARG, "d3pm_op_quantize_mx: bad arguments");
  return quantize_mx(dtype, X, ldx, static_cast<uint8_t*>(X8), static_cast<uint8_t*>(SX), M, K, static_cast<hipStream_t>(stream));
}

int d3pm_op_layernorm_mx(int dtype, const void* X, void* Y8, void* SX, const void* w, const void* b, const void* film, int M, int d,
                         float eps, void* stream) {
  D3PM_REQUIRE(X && Y8 && SX && w && b && M > 0, D3PM_E_ARG, "d3pm_op_layernorm_mx: bad arguments");
  return layernorm_mx(dtype, X, static_cast<uint8_t*>(Y8), static_cast<uint8_t*>(SX), w, b, film, nullptr, nullptr, nullptr, nullptr, M, d,
                      eps, static_cast<hipStream_t>(stream));
}

int d3pm_op_layernorm_mx_pair(int dtype, const void* X, void* Y8, void* SX, const void* w, const void* b, const void* film, const void* w2,
                              const void* b2, void* Y8_2, void* SX_2, int M, int d, float eps, void* stream) {
  D3PM_REQUIRE(X && Y8 && SX && w && b && w2 && b2 && Y8_2 && SX_2 && M > 0, D3PM_E_ARG, "d3pm_op_layernorm_mx_pair: bad arguments");
  return layernorm_mx(dtype, X, static_cast<uint8_t*>(Y8), static_cast<uint8_t*>(SX), w, b, film, w2, b2, static_cast<uint8_t*>(Y8_2),
                      static_cast<uint8_t*>(SX_2), M, d, eps, static_cast<hipStream_t>(stream));
}

int d3pm_op_linear_mx(int out_dtype, const void* X8, int ldx, const void* SX, const void* W8, const void* SW, const void* bias, void* Y,
                      int ldy, const void* R1, int ldr, const uint8_t* row_mask, int mask_period, void* Y8, void* SY, int M, int N, int K,
                      int act, const d3pm_tuning* tuning, void* stream) {
  D3PM_REQUIRE(X8 && SX && W8 && SW && (Y || Y8) && M > 0 && N > 0 && K > 0, D3PM_E_ARG, "d3pm_op_linear_mx: bad arguments");
  MxLinearArgs m;
  m.X8 = X8; m.ldx = ldx; m.SX = SX; m.W8 = W8; m.SW = SW; m.bias = bias; m.Y = Y; m.ldy = ldy; m.R1 = R1; m.ldr = ldr;
  m.row_mask = row_mask; m.mask_period = mask_period > 0 ? mask_period : 1; m.Y8 = Y8; m.SY = SY; m.M = M; m.N = N; m.K = K; m.act = act;
  m.tune = tuning;
  D3PM_REQUIRE(mx_linear_supported(out_dtype, m), D3PM_E_SHAPE,
               "d3pm_op_linear_mx: needs M a multiple of 192, N of 128, K of 512, a 16-bit output type, 16-byte aligned operands and "
               "one of the epilogues plain / GELU / R1 / R1 + mask (MX output: plain / GELU)");
  return mx_linear(out_dtype, m, static_cast<hipStream_t>(stream));
}

static int op_attention_impl(const char* who, int dtype, int family, const void* Q, int ldq, const void* K, const void* V, int ldkv, void* O,
                             int ldo, int B, int Tq, int S, int H, int hd, float scale, const int32_t* key_len, const d3pm_tuning* tuning,
                             void* stream) {
  D3PM_REQUIRE(Q && K && V && O && B > 0 && Tq > 0 && S > 0 && H > 0 && hd > 0, D3PM_E_ARG, "%s: bad arguments", who);
  const Ctx cx(tuning);
  AttnArgs a;
  a.tune = tuning;
  a.Q = Q; a.ldq = ldq; a.K = K; a.V = V; a.ldkv = ldkv; a.O = O; a.ldo = ldo; a.B = B; a.Tq = Tq; a.S = S; a.H = H;
  a.hd = hd; a.scale = scale; a.key_len = key_len;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (family == 1) return generic_attention(dtype, a, s);
  if (family == 2) {
    const AttnPlan plan = plan_attention(dtype, a);
    D3PM_REQUIRE(plan.mfma(), D3PM_E_SHAPE, "%s: shape not supported by the MFMA kernel", who);
    return mfma_attention(dtype, a, plan, s);
  }
  return run_attention(cx, dtype, a, 0, s);
}

int d3pm_op_attention(int dtype, int family, const void* Q, int ldq, const void* K, const void* V, int ldkv, void* O,
                      int ldo, int B, int Tq, int S, int H, int hd, float scale, const d3pm_tuning* tuning, void* stream) {
  return op_attention_impl("d3pm_op_attention", dtype, family, Q, ldq, K, V, ldkv, O, ldo, B, Tq, S, H, hd, scale, nullptr, tuning, stream);
}

// key_len (device, [B]) is read by the kernels only: a value outside 1 .. S cannot be refused here without a copy to the host
int d3pm_op_attention_keylen(int dtype, int family, const void* Q, int ldq, const void* K, const void* V, int ldkv, void* O,
                             int ldo, int B, int Tq, int S, int H, int hd, float scale, const int32_t* key_len,
                             const d3pm_tuning* tuning, void* stream) {
  return op_attention_impl("d3pm_op_attention_keylen", dtype, family, Q, ldq, K, V, ldkv, O, ldo, B, Tq, S, H, hd, scale, key_len, tuning,
                           stream);
}

// the gathered attn32p_hd64 whatever the grid size: the planner is asked with attn_query_groups = 32 (always the 32 x 32 x 16 walk)
int d3pm_op_attention_gather(int dtype, const void* Q, int ldq, const void* K, const void* V, int ldkv, int kv_rows, const int32_t* key_row,
                             const int32_t* seg_start, const int32_t* seg_len, void* O, int ldo, int B, int Tq, int S, int H, int hd, float scale,
                             const int32_t* key_len, const d3pm_tuning* tuning, void* stream) {
  D3PM_REQUIRE(Q && K && V && O && key_row && seg_start && seg_len && kv_rows > 0 && B > 0 && Tq > 0 && S > 0 && H > 0 && hd > 0, D3PM_E_ARG,
               "d3pm_op_attention_gather: bad arguments");
  d3pm_tuning tn = tune_of(tuning);
  tn.attn_query_groups = 32;
  AttnArgs a;
  a.tune = &tn;
  a.Q = Q; a.ldq = ldq; a.K = K; a.V = V; a.ldkv = ldkv; a.O = O; a.ldo = ldo; a.B = B; a.Tq = Tq; a.S = S; a.H = H;
  a.hd = hd; a.scale = scale; a.key_len = key_len; a.seg_start = seg_start; a.seg_len = seg_len; a.key_row = key_row; a.kv_rows = kv_rows;
  const AttnPlan plan = plan_attention(dtype, a);
  D3PM_REQUIRE(plan.kernel == ATTN_32P, D3PM_E_SHAPE,
               "d3pm_op_attention_gather: needs a 16-bit dtype, head width 64, Tq a multiple of 128, S of 64 and 16-byte aligned rows");
  return mfma_attention(dtype, a, plan, static_cast<hipStream_t>(stream));
}

// the pooled attn32p_hd64 with the pool and the grid the caller names; an utterance beyond the pool takes the gathered walk in the same launch
int d3pm_op_attention_gather_pool(int dtype, const void* Q, int ldq, const void* K, const void* V, int ldkv, int kv_rows, const int32_t* key_row,
                                  const int32_t* seg_start, const int32_t* seg_len, void* O, int ldo, int B, int Tq, int S, int H, int hd, float scale,
                                  const int32_t* key_len, const int32_t* seg_key, const int32_t* pool_src, int pool_rows, int qblocks_grid,
                                  const d3pm_tuning* tuning, void* stream) {
  D3PM_REQUIRE(Q && K && V && O && key_row && seg_start && seg_len && seg_key && kv_rows > 0 && B > 0 && Tq > 0 && S > 0 && H > 0 && hd > 0 &&
                   pool_rows > 0 && qblocks_grid > 0,
               D3PM_E_ARG, "d3pm_op_attention_gather_pool: bad arguments");
  d3pm_tuning tn = tune_of(tuning);
  tn.attn_query_groups = 32;
  AttnArgs a;
  a.tune = &tn;
  a.Q = Q; a.ldq = ldq; a.K = K; a.V = V; a.ldkv = ldkv; a.O = O; a.ldo = ldo; a.B = B; a.Tq = Tq; a.S = S; a.H = H;
  a.hd = hd; a.scale = scale; a.key_len = key_len; a.seg_start = seg_start; a.seg_len = seg_len; a.key_row = key_row; a.kv_rows = kv_rows;
  a.seg_key = seg_key; a.pool_src = pool_src; a.pool_rows = pool_rows; a.qblocks_grid = qblocks_grid;
  const AttnPlan plan = plan_attention(dtype, a);
  D3PM_REQUIRE(plan.kernel == ATTN_32P_POOL, D3PM_E_SHAPE,
               "d3pm_op_attention_gather_pool: needs what d3pm_op_attention_gather needs, qblocks_grid <= Tq / 128, and the tiles, the index "
               "(4 S bytes) and the pool (256 bytes per row) within 160 KiB of LDS");
  return mfma_attention(dtype, a, plan, static_cast<hipStream_t>(stream));
}

// key_len1 / key_len2 (device, [B]) are read by the kernels only: see d3pm_op_attention_keylen
int d3pm_op_attention_pair_keylen(int dtype, const void* Q1, const void* K1, const void* V1, void* O1, int S1, const void* Q2, const void* K2,
                                  const void* V2, void* O2, int S2, int ldq, int ldkv, int ldo, int B, int Tq, int H, int hd, float scale,
                                  const int32_t* key_len1, const int32_t* key_len2, const d3pm_tuning* tuning, void* stream) {
  D3PM_REQUIRE(Q1 && K1 && V1 && O1 && Q2 && K2 && V2 && O2 && B > 0 && Tq > 0 && S1 > 0 && S2 > 0 && H > 0 && hd > 0, D3PM_E_ARG,
               "d3pm_op_attention_pair: bad arguments");
  const Ctx cx(tuning);
  AttnArgs a;
  a.tune = tuning;
  a.Q = Q1; a.ldq = ldq; a.K = K1; a.V = V1; a.ldkv = ldkv; a.O = O1; a.ldo = ldo; a.B = B; a.Tq = Tq; a.S = S1; a.H = H;
  a.hd = hd; a.scale = scale;
  a.Q2 = Q2; a.K2 = K2; a.V2 = V2; a.O2 = O2; a.S2 = S2;
  a.key_len = key_len1; a.key_len2 = key_len2;
  return run_attention(cx, dtype, a, 0, static_cast<hipStream_t>(stream));
}

int d3pm_op_attention_pair(int dtype, const void* Q1, const void* K1, const void* V1, void* O1, int S1, const void* Q2, const void* K2,
                           const void* V2, void* O2, int S2, int ldq, int ldkv, int ldo, int B, int Tq, int H, int hd, float scale,
                           const d3pm_tuning* tuning, void* stream) {
  return d3pm_op_attention_pair_keylen(dtype, Q1, K1, V1, O1, S1, Q2, K2, V2, O2, S2, ldq, ldkv, ldo, B, Tq, H, hd, scale, nullptr, nullptr,
                                       tuning, stream);
}

// the cross pair of the deduplicated loop (tests): query segments through the planner and the launcher like any other call -- a plan
// other than the resident 32 x 32 x 16 pair is refused by run_attention, which knows which kernels take segments
int d3pm_op_attention_pair_segments(int dtype, const void* Q1, const void* K1, const void* V1, void* O1, int S1, const void* Q2,
                                    const void* K2, const void* V2, void* O2, int S2, int ldq, int ldkv, int ldo, int B, int Tq, int H,
                                    int hd, float scale, const int32_t* seg_start, const int32_t* seg_len, const int32_t* key_len1,
                                    const int32_t* key_len2, const d3pm_tuning* tuning, void* stream) {
  D3PM_REQUIRE(Q1 && K1 && V1 && O1 && Q2 && K2 && V2 && O2 && seg_start && seg_len && B > 0 && Tq > 0 && S1 > 0 && S2 > 0 && H > 0 && hd > 0,
               D3PM_E_ARG, "d3pm_op_attention_pair_segments: bad arguments");
  const Ctx cx(tuning);
  AttnArgs a;
  a.tune = tuning;
  a.Q = Q1; a.ldq = ldq; a.K = K1; a.V = V1; a.ldkv = ldkv; a.O = O1; a.ldo = ldo; a.B = B; a.Tq = Tq; a.S = S1; a.H = H;
  a.hd = hd; a.scale = scale;
  a.Q2 = Q2; a.K2 = K2; a.V2 = V2; a.O2 = O2; a.S2 = S2;
  a.key_len = key_len1; a.key_len2 = key_len2; a.seg_start = seg_start; a.seg_len = seg_len;
  return run_attention(cx, dtype, a, 0, static_cast<hipStream_t>(stream));
}

int d3pm_op_layernorm(int dtype, const void* X, void* Y, const void* w, const void* b, const void* film, int M, int d,
                      float eps, void* stream) {
  D3PM_REQUIRE(X && Y && w && b && M > 0 && d > 0, D3PM_E_ARG, "d3pm_op_layernorm: bad arguments");
  LayerNormArgs ln;
  ln.X = X; ln.Y = Y; ln.w = w; ln.b = b; ln.film = film; ln.M = M; ln.d = d; ln.eps = eps;
  const Ctx cx(nullptr);
  return run_layernorm(cx, dtype, ln, 0, static_cast<hipStream_t>(stream));
}

int d3pm_op_linear_rowpanel(int dtype, const void* X, const void* X2, int ldx, const void* W, const void* bias, void* Y, const void* R1,
                            const uint8_t* row_mask, int mask_period, int M, int K, const void* ln_w, const void* ln_b, void* ln_y,
                            const void* ln2_w, const void* ln2_b, void* ln2_y, const void* film, float eps, void* ln_sx, void* ln2_sx,
                            void* stream) {
  D3PM_REQUIRE(X && W && bias && Y && R1 && ln_w && ln_b && ln_y && M > 0 && K > 0, D3PM_E_ARG, "d3pm_op_linear_rowpanel: bad arguments");
  LinearArgs g;
  g.X = X; g.ldx = ldx; g.W = W; g.bias = bias; g.Y = Y; g.ldy = 512; g.R1 = R1; g.ldr = 512; g.row_mask = row_mask;
  g.mask_period = mask_period > 0 ? mask_period : 1; g.M = M; g.N = 512; g.K = K;
  RowPanelFuse f;
  f.X2 = X2; f.lnw = ln_w; f.lnb = ln_b; f.lny = ln_y; f.lnw2 = ln2_w; f.lnb2 = ln2_b; f.lny2 = ln2_y; f.film = film; f.eps = eps;
  f.sx = ln_sx; f.sx2 = ln2_sx;
  D3PM_REQUIRE(row_panel_supported(dtype, g, f), D3PM_E_SHAPE,
               "d3pm_op_linear_rowpanel: needs a 16-bit dtype, M a multiple of 96, K a multiple of 128 (>= 256), 16-byte aligned "
               "operands and one of the three fused forms (include/d3pm_hip.h)");
  return row_panel_linear(dtype, g, f, static_cast<hipStream_t>(stream));
}

int d3pm_op_cond_embed(int dtype, int which, const int32_t* tokens, int n_levels, const void* tables, const void* pe, void* y, int rows,
                       int s_prompt, int d, int n_classes, void* stream) {
  D3PM_REQUIRE(tokens && tables && pe && y && rows > 0 && d > 0 && n_classes > 0, D3PM_E_ARG, "d3pm_op_cond_embed: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (which == 0) return cond_embed_text(dtype, tokens, tables, pe, y, rows, rows, d, n_classes, nullptr, s);
  D3PM_REQUIRE(n_levels > 0 && s_prompt > 0, D3PM_E_ARG, "d3pm_op_cond_embed: bad prompt arguments");
  return cond_embed_prompt(dtype, tokens, n_levels, tables, pe, y, rows, s_prompt, d, n_classes, nullptr, s);
}

void d3pm_tuning_default(d3pm_tuning* t) {
  if (t) *t = tune_of(nullptr);
}

int d3pm_prof_create(int kclass, int max_events, d3pm_prof** out) {
  D3PM_REQUIRE(out && kclass >= 0 && kclass <= D3PM_K_COUNT && max_events > 0, D3PM_E_ARG, "d3pm_prof_create: bad arguments");
  d3pm_prof* p = new (std::nothrow) d3pm_prof();
  D3PM_REQUIRE(p, D3PM_E_ARG, "d3pm_prof_create: out of host memory");
  p->ev.resize(static_cast<size_t>(max_events) * 2);
  p->cls.assign(static_cast<size_t>(max_events), -1);
  for (size_t i = 0; i < p->ev.size(); ++i) {
    if (hipEventCreate(&p->ev[i]) != hipSuccess) {
      set_error("d3pm_prof_create: hipEventCreate failed");
      for (size_t j = 0; j < i; ++j) (void)hipEventDestroy(p->ev[j]);     // the events created so far
      delete p;
      return D3PM_E_HIP;
    }
  }
  p->kclass = kclass;
  *out = p;
  return D3PM_OK;
}

int d3pm_prof_read_class(d3pm_prof* p, int kclass, int* launches, double* total_ms, double* flops, double* bytes) {
  D3PM_REQUIRE(p && kclass >= 0 && kclass < D3PM_K_COUNT, D3PM_E_ARG, "d3pm_prof_read_class: bad arguments");
  double ms = 0;
  int n = 0;
  for (int i = 0; i + 1 < p->used; i += 2) {
    if (p->cls[i / 2] != kclass) continue;
    D3PM_CHECK_HIP(hipEventSynchronize(p->ev[i + 1]));
    float m = 0;
    D3PM_CHECK_HIP(hipEventElapsedTime(&m, p->ev[i], p->ev[i + 1]));
    ms += m;
    ++n;
  }
  if (launches) *launches = n;
  if (total_ms) *total_ms = ms;
  if (flops) *flops = p->flops[kclass];
  if (bytes) *bytes = p->bytes[kclass];
  return D3PM_OK;
}

int d3pm_prof_read(d3pm_prof* p, int* launches, double* total_ms, double* flops, double* bytes) {
  D3PM_REQUIRE(p, D3PM_E_ARG, "d3pm_prof_read: null handle");
  int n = 0;
  double ms = 0, fl = 0, by = 0;
  for (int c = 0; c < D3PM_K_COUNT; ++c) {
    int nc = 0;
    double mc = 0, fc = 0, bc = 0;
    D3PM_TRY(d3pm_prof_read_class(p, c, &nc, &mc, &fc, &bc));
    n += nc; ms += mc; fl += fc; by += bc;
  }
  if (launches) *launches = n;
  if (total_ms) *total_ms = ms;
  if (flops) *flops = fl;
  if (bytes) *bytes = by;
  p->used = 0;
  for (int c = 0; c < D3PM_K_COUNT; ++c) p->flops[c] = p->bytes[c] = 0;
  return D3PM_OK;
}

int d3pm_prof_destroy(d3pm_prof* p) {
  if (!p) return D3PM_OK;
  for (auto& e : p->ev) (void)hipEventDestroy(e);
  delete p;
  return D3PM_OK;
}

}  // extern "C"
