// d3pm_sequence.cpp -- the workspace carve-up and the once-per-call plans of d3pm_sequence.h, and the library's error message.
// Host code only: no kernel, no launch, no HIP runtime call.
#include "d3pm_sequence.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>

namespace d3pm {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

Workspace carve(const d3pm_shape& sh, int batch, char* base) {
  const size_t es = dtype_size(sh.dtype), n = static_cast<size_t>(batch) * sh.canvas, d = sh.d_model;
  Workspace w{};
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
  w.x = take(n * d * es);
  w.h = take(n * d * es);
  w.h2 = take(n * d * es);           // adjacent to h: norm2 | norm22 outputs feed ONE [2n, d] query projection
  // Regions that are never live together share memory (D3PM_TUNE_WORKSPACE_ALIAS): 350 -> 200 MB per 32 utterances beside a
  // 256-MB Infinity Cache, +1.6 % tokens/s measured for the first pair alone (profiles/round2_c_ab_throughput.txt):
  //   packed qkv rows -> cross-attention queries -> MLP hidden rows -> logits of the iteration;
  //   norm22 output (dead once the query projection ran) -> prompt cross-attention output
  if (tune_of(sh.tuning).workspace_alias) {
    const size_t big = n * 4 * d * es, lg = n * levels(sh) * logits_ld(sh) * es;
    w.mlp = take(big > lg ? big : lg);
    w.qkv = w.mlp;
    w.logits = w.mlp;
    w.att = take(n * d * es);
    w.att2 = w.h2;
  } else {
    w.qkv = take(n * 3 * d * es);
    w.att = take(n * d * es);
    w.att2 = take(n * d * es);
    w.mlp = take(n * 4 * d * es);
    w.logits = take(n * levels(sh) * logits_ld(sh) * es);
  }
  w.stats = reinterpret_cast<float*>(take(((n + 15) & ~static_cast<size_t>(15)) * ((d + 31) / 32) * 2 * sizeof(float)));
  w.mxs = reinterpret_cast<uint8_t*>(take(2 * n * ((d + 31) / 32)));
  if (base && 17 * n + 12 * static_cast<size_t>(batch) + 16 <= 2 * n * ((d + 31) / 32)) {
    int32_t* ip = reinterpret_cast<int32_t*>(w.mxs);
    w.dd.row_of = ip; w.dd.rep_pos = ip + n; w.dd.cid = ip + 2 * n; w.dd.key_cls = ip + 3 * n; w.dd.cnt = ip + 4 * n; w.dd.seg_start = w.dd.cnt + batch;
    w.dd.seg_len = w.dd.seg_start + batch; w.dd.m_live = w.dd.seg_len + batch; w.dd.cmask = reinterpret_cast<uint8_t*>(w.dd.m_live + 4);
  }
  if (fold_shape_ok(sh.dtype, sh.d_model)) {
    const size_t L = sh.n_layers;
    w.fc1f = take(L * 4 * d * d * es);
    w.fc1f_s = reinterpret_cast<float*>(take(L * 4 * d * sizeof(float)));
    w.fc1f_b = reinterpret_cast<float*>(take(L * 4 * d * sizeof(float)));
    if (levels(sh) == 1) {      // whatever d3pm_tuning.ln_fold says: a caller never has to know
      const size_t mt = qkv_table_rows(sh.n_classes);
      w.tab_x = take(mt * d * es);
      w.tab_stats = reinterpret_cast<float*>(take(mt * (d / 32) * 2 * sizeof(float)));
      w.tab_qkv = take(mt * 3 * d * es);
      // The sampler launch writes these rows while it reads the logits, which alias ws.qkv: q takes a region of its own, k | v
      // the adjacent h | h2 -- the folded sequence writes no LayerNorm output, so nothing lives there between the last block of
      // an evaluation and the first out-projection of the next (h: o_text of the two-launch cross-attention output; h2 = att2 under
      // workspace_alias: the prompt cross-attention output, both dead behind their block)
      w.q0 = take(n * d * es);
      w.kv0 = w.h;
    }
  }
  w.total = off;
  return w;
}

int fold_plan(const DenoiserArgs& q, uint32_t flags, bool fp8) {
  const d3pm_shape& sh = q.sh;
  if (fp8 || !q.w.fold || !fold_features(tune_of(sh.tuning)).fold || (flags & D3PM_FLAG_FORCE_GENERIC) || !fold_shape_ok(sh.dtype, sh.d_model)) return FOLD_NONE;
  FoldPlanner plan{sh.dtype, sh.tuning, sh.d_model == 512};
  for (int l = 0; l < sh.n_layers; ++l)
    if (folded_block(q, l, false, plan) != D3PM_OK) return FOLD_NONE;
  return plan.big ? FOLD_QUADS : FOLD_PARTS;
}

LoopPlan loop_plan(const DenoiserArgs& q0, uint32_t flags, const LoopCall& call) {
  const d3pm_shape& sh = q0.sh;
  const Workspace& ws = q0.ws;
  const FoldFeatures on = fold_features(tune_of(sh.tuning));
  LoopPlan p;
  p.batch = q0.batch; p.canvas = sh.canvas; p.t_stop = call.t_stop;
  p.fold = fold_plan(q0, flags, call.fp8);
  // Block-0 QKV from the per-id table (build_qkv_table): every unguided loop -- plain, canvas / known frames, keys, sampling / nucleus,
  // trace -- once it runs two iterations.  The GUIDED loop keeps the projection: its first evaluation embeds through embed_twins and
  // its sampler launch (posterior_sample_prep_guided) does not gather.
  p.table = p.fold != FOLD_NONE && on.table && levels(sh) == 1 && !call.guided && call.t_start - call.t_stop >= 2 && ws.tab_qkv;
  DenoiserArgs q = q0;
  if (p.table) q.qkv_table = ws.tab_qkv;
  // Row deduplication (d3pm_dedup.hip): the unguided 16-bit n_q = 1 loop with the table, moments as quads, and every launch of the
  // sequence on a kernel that reads the live count / the query segments from device memory.  Otherwise the launch list runs untouched.
  const int n_rows = q.batch * sh.canvas;
  if (p.table && p.fold == FOLD_QUADS && on.dedup && !call.fp8 && !call.guided && ws.dd.row_of && n_rows % 384 == 0 && sh.n_layers <= 16 &&
      sh.n_classes <= kDedupMaxClasses && q.batch <= kDedupMaxBatch && ws.h2 == at(ws.h, static_cast<size_t>(n_rows) * sh.d_model, dtype_size(sh.dtype))) {
    DedupPlanner dp{sh.dtype, sh.tuning, true};
    for (int l = 0; l < sh.n_layers; ++l) (void)folded_block(q, l, true, dp, l == 0);
    LinearArgs fin = projection(ws.x, q.w.final_w, q.w.final_b, ws.logits, n_rows, sh.n_classes, sh.d_model);
    fin.ldy = logits_ld(sh); fin.tune = sh.tuning;
    const LinearPlan fp = plan_linear(sh.dtype, fin);
    // the self-attention walks its keys through an index (attn32p_hd64 GATHER): the staged index beside the tiles, and 32-bit byte
    // offsets into the rows it reads -- the compact QKV rows [n_rows][3d] or the block-0 QKV table
    const unsigned long long kv_rows = std::max<unsigned long long>(n_rows, qkv_table_rows(sh.n_classes));
    const bool gather_ok = static_cast<size_t>(sh.canvas) * 4 <= kGatherIndexBytes && kv_rows * 3 * sh.d_model * dtype_size(sh.dtype) < (1ull << 32);
    p.dedup = dp.ok && gather_ok && (fp.big() || fp.kernel == LIN_128_GLDS);
  }
  // The regime of an iteration of the deduplicated loop, decided with no read-back (the loop is graph-captured): iteration t
  // evaluates x_t, which the sampler launch of iteration t + 1 drew with cbar_prev = cbar[t] (make_posterior_consts), so a frame of it is
  // still masked with probability float(cbar[t]) -- the index of the iteration itself, also for t_start, whose canvas the caller
  // brings (all mask in a full reverse process).  An estimate within live_latency_rows() takes the latency launch list when every
  // projection of a block plans onto gemm_mfma_panel64 for it (the final projection keeps its kernel).  The estimate chooses speed
  // only: every kernel reads the live count from the device.  Known frames are the caller's and cannot be counted here: such a loop
  // keeps the big-tile list.
  // The iterations that stay on big tiles get an estimate of their own (LoopPlan::rows_est), by the same reasoning and under the same
  // condition on known frames; it moves the tile geometry of the projections onto the residual stream and nothing else.
  p.live_tiles = p.dedup && !call.known;
  p.n_classes = sh.n_classes;
  if (p.dedup && on.latency && !call.known) {
    q.dd = &ws.dd;
    q.m_est = live_latency_rows();
    DedupPlanner lp{sh.dtype, sh.tuning, true, LIN_PANEL64};
    for (int l = 0; l < sh.n_layers; ++l) (void)folded_block(q, l, false, lp, l == 0);
    p.latency = lp.ok;
  }
  return p;
}

}  // namespace d3pm

extern "C" const char* d3pm_last_error(void) { return d3pm::g_err; }
