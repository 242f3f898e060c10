// live_tiles_plan_table.cpp -- prints what the big-tile planner does with the second estimate of the deduplicated loop
// (csrc/d3pm_plan.cpp: plan_distinct_rows, live_short96_rows / live_short128_rows, big_tile with LinearArgs::rows_est; csrc/d3pm_sequence.h: LoopPlan::rows_est)
// for tests/test_live_tiles_plan_api.py.  Host only, linked like tests/launch_plan_table.cpp; defines no function of the library.
#include <sys/mman.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "d3pm_sequence.h"

using namespace d3pm;

static char g_buf[256] __attribute__((aligned(64)));      // every pointer of a case: aligned, never dereferenced

static const char* linear_name(int k) {
  return k == LIN_BIG ? "big" : k == LIN_PANEL64 ? "panel64" : k == LIN_128_GLDS ? "128glds" : k == LIN_GENERIC ? "generic" : "other";
}

// a projection onto the residual stream of width 512 with the epilogue `epi`, as the loop's producer lambda builds it
static LinearArgs producer_args(int M, int K, int epi) {
  LinearArgs a;
  a.X = a.W = a.bias = g_buf; a.Y = g_buf; a.R1 = g_buf;
  a.M = M; a.N = 512; a.K = K; a.ldx = K; a.ldy = 512; a.ldr = 512;
  if (epi & EPI_MASK) { a.row_mask = reinterpret_cast<const uint8_t*>(g_buf); a.mask_period = M; }
  a.stats_out = reinterpret_cast<float*>(g_buf);
  a.moment_quads = (epi & EPI_QUADS) != 0;
  a.m_live = reinterpret_cast<const int*>(g_buf);
  return a;
}
static void print_plan(const char* what, int B, const char* est, const LinearPlan& p, int form) {
  std::printf("linear case=%s B=%d est=%s kernel=%s geom=%d tm=%d tn=%d grid=%u lds=%zu n_tiles=%d tiles_total=%d epi=%d form=%d\n", what, B, est,
              linear_name(p.kernel), p.geom, p.tm, p.tn, p.grid, p.lds, p.n_tiles, p.tiles_total, p.epi, form);
}
// the three producers and the dual at B utterances of 768 frames: a call that never touches the field, and the estimates `ests`
static void producer_cases(int B, const std::vector<int>& ests) {
  const int n = B * 768;
  const int quads = EPI_R1 | EPI_STATS | EPI_QUADS;
  char est[32];
  for (int i = -1; i < static_cast<int>(ests.size()); ++i) {
    if (i < 0) std::snprintf(est, sizeof est, "none");
    else std::snprintf(est, sizeof est, "%d", ests[i]);
    auto with = [&](LinearArgs a) {
      if (i >= 0) a.rows_est = ests[i];
      return a;
    };
    print_plan("out", B, est, plan_linear(D3PM_BF16, with(producer_args(n, 512, quads))), -1);
    print_plan("fc2", B, est, plan_linear(D3PM_BF16, with(producer_args(n, 2048, quads | EPI_MASK))), -1);
    const CrossOutPlan c = plan_cross_out(D3PM_BF16, with(producer_args(n, 512, quads)), g_buf, false, true);
    print_plan("cross", B, est, c.dual, c.form);
    // a launch without a device-side row count walks the capacity: the estimate must not move it
    LinearArgs nl = with(producer_args(n, 512, quads));
    nl.m_live = nullptr;
    print_plan("out_no_live", B, est, plan_linear(D3PM_BF16, nl), -1);
  }
}

// ---- the 32-utterance loop, walked as the library walks it (the model of tests/launch_plan_table.cpp) ----
static char* reserve(size_t bytes) {
  void* p = mmap(nullptr, bytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (p == MAP_FAILED) { std::perror("mmap"); std::exit(1); }
  return static_cast<char*>(p);
}
static const void* fake_weight() {
  static char* pool = reserve(1 << 20);
  static size_t used = 0;
  used += 256;
  return pool + used;
}
struct Model {
  d3pm_tuning tn = tune_of(nullptr);
  d3pm_shape sh{};
  d3pm_block_weights blocks[6];
  d3pm_fold_block fold[6];
  d3pm_weights w{};
  Workspace ws{};
  int batch;
  const void *kv_text, *kv_prompt;
  const uint8_t* mask;
  Model(int batch_, int ln_fold) : batch(batch_) {
    tn.ln_fold = ln_fold;
    sh.d_model = 512; sh.n_heads = 8; sh.n_layers = 6; sh.canvas = 768; sh.s_text = 50; sh.s_prompt = 225; sh.n_classes = 1025; sh.mask_id = 1024;
    sh.timesteps = 100; sh.dtype = D3PM_BF16; sh.n_q = 1; sh.tuning = &tn;
    for (auto& b : blocks) {
      const void** p = reinterpret_cast<const void**>(&b);
      for (size_t i = 0; i < sizeof b / sizeof *p; ++i) p[i] = fake_weight();
    }
    for (auto& f : fold) {
      f.qkv_w = fake_weight(); f.q2_w = fake_weight();
      f.qkv_s = static_cast<const float*>(fake_weight()); f.qkv_b = static_cast<const float*>(fake_weight());
      f.q2_s = static_cast<const float*>(fake_weight()); f.q2_b = static_cast<const float*>(fake_weight());
    }
    w.resps_emb = fake_weight(); w.time_emb = fake_weight(); w.final_w = fake_weight(); w.final_b = fake_weight(); w.blocks = blocks; w.fold = fold;
    ws = carve(sh, batch, reserve(carve(sh, batch, nullptr).total));
    const size_t kv = static_cast<size_t>(sh.n_layers) * batch * 2 * sh.d_model * 2;
    kv_text = reserve(kv * sh.s_text); kv_prompt = reserve(kv * sh.s_prompt);
    mask = reinterpret_cast<const uint8_t*>(reserve(sh.canvas));
  }
  DenoiserArgs args() const { return DenoiserArgs{sh, w, batch, mask, sh.canvas, kv_text, kv_prompt, ws, KeyCounts{}, 0}; }
};
struct Schedule {
  uint16_t betas[101], d[100], c[100], dbar[100], cbar[100];
  d3pm_schedule s{100, d, c, dbar, cbar};
  Schedule() { if (d3pm_schedule_build(100, betas, d, c, dbar, cbar) != D3PM_OK) std::exit(1); }
};
// prints every projection of block 1 of iteration t as the library's launcher would plan it
struct Printer {
  const Model& m; const char* name; int t;
  void line(const char* kind, const LinearArgs& g, const LinearPlan& p, int form) {
    const char* what = g.fold_s ? (g.act == ACT_GELU ? "fc1" : g.N == 3 * g.K ? "qkv" : "q2") : g.X == m.ws.mlp ? "fc2" : kind[0] == 'd' ? "cross" : "out";
    std::printf("step case=%s t=%d name=%s kind=%s kernel=%s geom=%d tm=%d tn=%d grid=%u lds=%zu epi=%d form=%d rows_est=%d\n", name, t, what, kind,
                linear_name(p.kernel), p.geom, p.tm, p.tn, p.grid, p.lds, p.epi, form, g.rows_est);
  }
  int linear(LinearArgs g) {
    g.tune = m.sh.tuning;
    line("linear", g, plan_linear(m.sh.dtype, g), -1);
    return D3PM_OK;
  }
  int attention(const AttnArgs&) { return D3PM_OK; }
  int dual(const CrossOutPlan& c, const LinearArgs& g, const void*) {
    line("dual", g, c.dual, c.form);
    return D3PM_OK;
  }
};
static void loop_case(const char* name, int B, int ln_fold, bool known) {
  const Schedule sched;
  const Model m(B, ln_fold);
  DenoiserArgs q = m.args();
  LoopCall call;
  call.t_start = 99; call.t_stop = 0; call.known = known;
  const LoopPlan p = loop_plan(q, 0, call);
  std::printf("plan case=%s fold=%d dedup=%d latency=%d live_tiles=%d\n", name, p.fold, p.dedup ? 1 : 0, p.latency ? 1 : 0, p.live_tiles ? 1 : 0);
  if (p.table) q.qkv_table = m.ws.tab_qkv;
  if (p.dedup) q.dd = &m.ws.dd;
  for (int t = 99; t > 0; --t) {
    const float cbar = host_h2f(sched.cbar[t]);
    q.m_est = p.m_est(&sched.s, t); q.seg_est = p.seg_est(&sched.s, t); q.rows_est = p.rows_est(&sched.s, t);
    std::printf("iter case=%s t=%d live_rows=%d distinct=%d m_est=%d rows_est=%d\n", name, t, plan_live_rows(B, 768, cbar),
                plan_distinct_rows(B, 768, m.sh.n_classes, cbar), q.m_est, q.rows_est);
    Printer pr{m, name, t};
    if (folded_block(q, 1, p.fold == FOLD_QUADS && !q.m_est, pr, false) != D3PM_OK) std::exit(1);
  }
}

int main() {
  const int S96 = live_short96_rows(), S128 = live_short128_rows();
  std::printf("const S96=%d S128=%d R=%d cus=%d\n", S96, S128, live_latency_rows(), kCUs);
  for (int B : {1, 2, 3, 8, 10, 11, 16, 32}) {
    const int n = B * 768;
    producer_cases(B, {0, 1, 96, 3841, S96 - 1, S96, S96 + 1, S128 - 1, S128, S128 + 1, 6144, n - 1, n, n + 5});
  }
  // the tuning codes that force the short tiles: the producers take them, everything else the automatic choice
  for (int variant : {9, 10}) {
    d3pm_tuning tn = tune_of(nullptr);
    tn.gemm_variant = variant;
    char name[32];
    for (int B : {1, 16, 32}) {
      const int n = B * 768, quads = EPI_R1 | EPI_STATS | EPI_QUADS;
      auto forced = [&](LinearArgs a) { a.tune = &tn; return a; };
      std::snprintf(name, sizeof name, "v%d_out", variant);
      print_plan(name, B, "none", plan_linear(D3PM_BF16, forced(producer_args(n, 512, quads))), -1);
      std::snprintf(name, sizeof name, "v%d_fc2", variant);
      print_plan(name, B, "none", plan_linear(D3PM_BF16, forced(producer_args(n, 2048, quads | EPI_MASK))), -1);
      std::snprintf(name, sizeof name, "v%d_cross", variant);
      const CrossOutPlan c = plan_cross_out(D3PM_BF16, forced(producer_args(n, 512, quads)), g_buf, false, true);
      print_plan(name, B, "none", c.dual, c.form);
      LinearArgs parts = forced(producer_args(n, 512, EPI_R1 | EPI_STATS));      // moments as parts: no short tile
      std::snprintf(name, sizeof name, "v%d_out_parts", variant);
      print_plan(name, B, "none", plan_linear(D3PM_BF16, parts), -1);
      LinearArgs r2 = forced(producer_args(n, 512, quads));                       // R1 + R2: the second of two launches, no short tile
      r2.R2 = g_buf;
      std::snprintf(name, sizeof name, "v%d_out_r2", variant);
      print_plan(name, B, "none", plan_linear(D3PM_BF16, r2), -1);
    }
  }
  loop_case("b32", 32, 1, false);
  loop_case("b32_fold4", 32, 4, false);
  loop_case("b32_known", 32, 1, true);
  loop_case("b16", 16, 1, false);
  // the estimate by itself: edges of its arguments
  for (float cbar : {1.0f, 0.999f, 0.5f, 0.0f})
    for (int classes : {1, 2, 1025, 1 << 20})
      std::printf("distinct batch=32 canvas=768 classes=%d cbar=%.3f rows=%d live_rows=%d\n", classes, cbar, plan_distinct_rows(32, 768, classes, cbar),
                  plan_live_rows(32, 768, cbar));
  return 0;
}
