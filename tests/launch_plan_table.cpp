// launch_plan_table.cpp -- prints the launch planner's choices (csrc/d3pm_plan.cpp), the launches of a folded block and the plan of a
// sampler loop (csrc/d3pm_sequence.{h,cpp}) for tests/test_launch_plan_api.py.
// Host only: compiled with `hipcc -x hip --cuda-host-only` and linked with d3pm_plan.cpp, d3pm_sequence.cpp and d3pm_schedule.cpp, it
// needs no device and no HIP runtime, and defines no function of the library itself.
// One `key=value ...` line per case; the sweep at the end checks properties of every plan itself and prints what it saw.
#include <sys/mman.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "d3pm_sequence.h"

using namespace d3pm;

static char g_buf[256] __attribute__((aligned(64)));      // every pointer of a case: aligned, never dereferenced

static const char* linear_name(int k) {
  switch (k) {
    case LIN_GENERIC: return "generic";
    case LIN_QUADS_REFUSED: return "quads_refused";
    case LIN_BIG: return "big";
    case LIN_PANEL64: return "panel64";
    case LIN_128_PF: return "128pf";
    case LIN_128_PERSIST: return "128persist";
    case LIN_128_GLDS: return "128glds";
  }
  return "?";
}
static const char* attn_name(int k) {
  switch (k) {
    case ATTN_GENERIC: return "generic";
    case ATTN_32P: return "attn32p_hd64";
    case ATTN_32: return "attn32_hd64";
    case ATTN_32_CROSS: return "attn32_cross_hd64";
    case ATTN_CROSS: return "attn_cross_hd64";
    case ATTN_SPLIT: return "attn_split_hd64";
    case ATTN_TILES: return "attn_mfma_hd64";
  }
  return "?";
}

// a projection with the epilogue `epi` (EPI_* bits), ldx = K, ldy = N rounded up to 8
static LinearArgs linear_args(int M, int N, int K, int epi, const d3pm_tuning* tune) {
  LinearArgs a;
  a.X = a.W = a.bias = g_buf; a.Y = g_buf;
  a.M = M; a.N = N; a.K = K; a.ldx = K; a.ldy = (N + 7) / 8 * 8; a.ldr = a.ldy; a.tune = tune;
  a.act = (epi & EPI_GELU) ? ACT_GELU : (epi & EPI_RELU) ? ACT_RELU : (epi & EPI_SILU) ? ACT_SILU : ACT_NONE;
  if (epi & (EPI_R1 | EPI_R2)) a.R1 = g_buf;
  if (epi & EPI_R2) a.R2 = g_buf;
  if (epi & EPI_MASK) { a.row_mask = reinterpret_cast<const uint8_t*>(g_buf); a.mask_period = M; }
  if (epi & EPI_LNF) { a.fold_s = a.fold_b = a.stats_in = reinterpret_cast<const float*>(g_buf); a.bias = nullptr; }
  if (epi & EPI_STATS) a.stats_out = reinterpret_cast<float*>(g_buf);
  a.moment_quads = (epi & EPI_QUADS) != 0;
  return a;
}

static void print_linear(const char* name, const LinearArgs& a, const LinearPlan& p) {
  std::printf("linear case=%s M=%d N=%d K=%d kernel=%s geom=%d tile=%dx%d grid=%u lds=%zu epi=%d\n", name, a.M, a.N, a.K, linear_name(p.kernel),
              p.geom, p.tm, p.tn, p.grid, p.lds, p.epi);
}
static void linear_case(const char* name, int M, int N, int K, int epi = 0, const d3pm_tuning* tune = nullptr) {
  const LinearArgs a = linear_args(M, N, K, epi, tune);
  print_linear(name, a, plan_linear(D3PM_BF16, a));
}

static d3pm_tuning default_tuning() { return tune_of(nullptr); }

// ---- the launch sequence and the loop plan (csrc/d3pm_sequence.h), walked as the library walks them ----
// address space that is never touched: the workspace carve() is run over, and 256-byte aligned stand-ins for the weights
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

// the d = 512, 8-head, 6-layer, 768-frame, 50 + 225-key, 1025-class bf16 model with `batch` utterances per evaluation
struct Model {
  d3pm_tuning tn = default_tuning();
  d3pm_shape sh{};
  d3pm_block_weights blocks[6];
  d3pm_fold_block fold[6];
  d3pm_weights w{};
  Workspace ws{};
  int batch;
  const void *kv_text, *kv_prompt;
  const uint8_t* mask;
  Model(int batch_, int n_q = 1, int ln_fold = 1, int regime_batch = 0) : batch(batch_) {
    tn.ln_fold = ln_fold; tn.regime_batch = regime_batch;
    sh.d_model = 512; sh.n_heads = 8; sh.n_layers = 6; sh.canvas = 768; sh.s_text = 50; sh.s_prompt = 225; sh.n_classes = 1025; sh.mask_id = 1024;
    sh.timesteps = 100; sh.dtype = D3PM_BF16; sh.n_q = n_q; sh.tuning = &tn;
    for (auto& b : blocks) {      // (a struct of pointers and nothing else)
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
  DenoiserArgs args(int token_rows = 0) const { return DenoiserArgs{sh, w, batch, mask, sh.canvas, kv_text, kv_prompt, ws, KeyCounts{}, token_rows}; }
};

// a visitor of folded_block that plans each launch as the library's launcher does (the caller's tuning, no forced family) and keeps it
struct Step {
  char kind;      // 'L' projection, 'D' dual out-projection, 'A' attention
  LinearArgs g; LinearPlan lp; int form;
  AttnArgs a; AttnPlan ap;
};
struct Recorder {
  int dt; const d3pm_tuning* tune;
  std::vector<Step> steps;
  int linear(LinearArgs g) {
    g.tune = tune;
    steps.push_back(Step{'L', g, plan_linear(dt, g), 0, AttnArgs{}, AttnPlan{}});
    return D3PM_OK;
  }
  int attention(AttnArgs a) {
    a.tune = tune;
    steps.push_back(Step{'A', LinearArgs{}, LinearPlan{}, 0, a, plan_attention(dt, a)});
    return D3PM_OK;
  }
  int dual(const CrossOutPlan& c, const LinearArgs& g, const void*) {
    steps.push_back(Step{'D', g, c.dual, c.form, AttnArgs{}, AttnPlan{}});
    return D3PM_OK;
  }
};
// a recorded launch by the workspace regions it reads and writes
static const char* step_name(const Step& s, const Workspace& ws) {
  if (s.kind == 'A') return s.a.Q2 ? "cross_attn" : "self_attn";
  if (s.kind == 'D') return "cross";
  if (s.g.Y == ws.h) return "cross_text";                            // o_text of the two-launch form: no moments
  if (s.g.fold_s) return s.g.act == ACT_GELU ? "fc1" : s.g.N == 3 * s.g.K ? "qkv" : "q2";
  return s.g.X == ws.mlp ? "fc2" : s.g.X == ws.att2 ? "cross" : "out";
}
static std::vector<Step> walk_block(const Model& m, const DenoiserArgs& q, int l, bool quads, bool qkv_ready) {
  Recorder r{m.sh.dtype, m.sh.tuning, {}};
  if (folded_block(q, l, quads, r, qkv_ready) != D3PM_OK) std::exit(1);
  return r.steps;
}

// the moment-touching launches of block 1 as fold_plan asks them (parts format, every row), under the names they have always had here
static void fold_cases(int B) {
  const Model m(B);
  char name[64];
  for (const Step& s : walk_block(m, m.args(), 1, false, false)) {
    if (s.kind == 'A' || (!s.g.fold_s && !s.g.stats_out)) continue;
    const char* what = step_name(s, m.ws);
    std::snprintf(name, sizeof name, "fold_%s/%d", what, B);
    print_linear(name, s.g, s.lp);
    if (!std::strcmp(what, "cross")) std::printf("cross case=%d form=%d\n", B, s.form);      // (of two launches, the one that writes the moments)
  }
}

// every launch of blocks 0 and 1, and the launch count of every block, of an evaluation whose DenoiserArgs are `q`
static void block_cases(const char* name, const Model& m, const DenoiserArgs& q, bool quads) {
  for (int l = 0; l < m.sh.n_layers; ++l) {
    const std::vector<Step> steps = walk_block(m, q, l, quads, q.qkv_table != nullptr);
    std::printf("block case=%s l=%d launches=%zu\n", name, l, steps.size());
    for (size_t i = 0; l < 2 && i < steps.size(); ++i) {
      const Step& s = steps[i];
      if (s.kind == 'A')
        std::printf("step case=%s l=%d i=%zu name=%s kind=attn kernel=%s segments=%d gather=%d\n", name, l, i, step_name(s, m.ws), attn_name(s.ap.kernel),
                    s.a.seg_len ? 1 : 0, s.a.key_row ? 1 : 0);
      else
        std::printf("step case=%s l=%d i=%zu name=%s kind=%s kernel=%s tile=%dx%d epi=%d form=%d live=%d\n", name, l, i, step_name(s, m.ws),
                    s.kind == 'D' ? "dual" : "linear", linear_name(s.lp.kernel), s.lp.tm, s.lp.tn, s.lp.epi, s.form, s.g.m_live ? 1 : 0);
    }
  }
}

struct Schedule {
  uint16_t betas[101], d[100], c[100], dbar[100], cbar[100];
  d3pm_schedule s{100, d, c, dbar, cbar};
  Schedule() { if (d3pm_schedule_build(100, betas, d, c, dbar, cbar) != D3PM_OK) std::exit(1); }
};

static LoopCall full_loop() {
  LoopCall c;
  c.t_start = 99; c.t_stop = 0;
  return c;
}
// the plan of a call, and its latency iterations
static LoopPlan plan_case(const char* name, const DenoiserArgs& q, uint32_t flags, const LoopCall& call, const Schedule& sched) {
  const LoopPlan p = loop_plan(q, flags, call);
  int first = -1, last = -1, count = 0;
  for (int t = call.t_start; t > call.t_stop; --t)
    if (p.m_est(&sched.s, t)) { if (first < 0) first = t; last = t; ++count; }
  std::printf("plan case=%s fold=%d table=%d dedup=%d latency=%d first=%d last=%d count=%d\n", name, p.fold, p.table ? 1 : 0, p.dedup ? 1 : 0,
              p.latency ? 1 : 0, first, last, count);
  return p;
}
static void sequence_cases() {
  const Schedule sched;
  char name[64];
  for (int B : {2, 8, 16, 32}) {
    const Model m(B);
    DenoiserArgs q = m.args();
    std::snprintf(name, sizeof name, "b%d", B);
    const LoopPlan p = plan_case(name, q, 0, full_loop(), sched);
    if (p.table) q.qkv_table = m.ws.tab_qkv;
    if (p.dedup) q.dd = &m.ws.dd;
    block_cases(name, m, q, p.fold == FOLD_QUADS);
    if (!p.dedup) continue;
    q.m_est = 64;      // a latency iteration: moments as parts
    std::snprintf(name, sizeof name, "lat%d", B);
    block_cases(name, m, q, false);
  }
  for (int ln_fold : {4, 3, 2, 0}) {
    const Model m(32, 1, ln_fold);
    std::snprintf(name, sizeof name, "ln_fold%d", ln_fold);
    plan_case(name, m.args(), 0, full_loop(), sched);
  }
  const Model m(32);
  const LoopPlan p32 = loop_plan(m.args(), 0, full_loop());
  for (int t : {74, 73})
    std::printf("est case=b32 t=%d rows=%d m_est=%d\n", t, plan_live_rows(32, 768, host_h2f(sched.cbar[t])), p32.m_est(&sched.s, t));
  LoopCall call = full_loop();
  call.fp8 = true;
  plan_case("fp8", m.args(), 0, call, sched);
  plan_case("force_generic", m.args(), D3PM_FLAG_FORCE_GENERIC, full_loop(), sched);
  call = full_loop();
  call.known = true;
  plan_case("known", m.args(), 0, call, sched);
  call = full_loop();
  call.t_stop = 98;
  plan_case("one_iteration", m.args(), 0, call, sched);
  // guided: the evaluation of 2 x 32 utterances under regime_batch = 64, x_t with a row per pair
  const Model g(64, 1, 1, 64);
  call = full_loop();
  call.guided = true;
  plan_case("guided", g.args(32 * 768), 0, call, sched);
  const Model q8(32, 8);
  plan_case("n_q8", q8.args(), 0, full_loop(), sched);
}

static void attn_case(const char* name, int B, bool cross, const d3pm_tuning& tn, bool key_len = false, bool keeps = false) {
  AttnArgs a;
  a.Q = a.K = a.V = g_buf; a.O = g_buf;
  a.B = B; a.H = 8; a.hd = 64; a.Tq = 768; a.tune = &tn;
  if (cross) {
    a.S = 50; a.S2 = 225; a.ldq = 1024; a.ldkv = 1024; a.ldo = 512;
    a.Q2 = a.K2 = a.V2 = g_buf; a.O2 = g_buf;
  } else {
    a.S = 768; a.ldq = a.ldkv = 1536; a.ldo = 512;
  }
  if (key_len) a.key_len = reinterpret_cast<const int32_t*>(g_buf);
  a.masked_keeps_schedule = keeps;
  const AttnPlan p = plan_attention(D3PM_BF16, a);
  std::printf("attn case=%s B=%d kernel=%s masked=%d qg=%d pair=%d n_qsplit=%d n_qblocks=%d n_first=%d grid=%u lds=%zu\n", name, B,
              attn_name(p.kernel), p.masked ? 1 : 0, p.qg, p.pair_seq ? 1 : 0, p.n_qsplit, p.n_qblocks, p.n_first, p.grid, p.lds);
}

// ---- the sweep: no expected table, properties of each plan alone ----
static long g_cases = 0, g_planned = 0, g_violations = 0;
static std::set<std::tuple<int, int, int>> g_seen;      // (family: 0 = 128, 1 = big, 2 = panel64, 3 = big dual, 4 = panel64 dual; epi; geom)

static void violation(const char* what, const LinearArgs& a, const LinearPlan& p, const d3pm_tuning& tn) {
  ++g_violations;
  std::printf("violation what=%s M=%d N=%d K=%d kernel=%s geom=%d grid=%u lds=%zu epi=%d gemm_variant=%d lat_tile=%d row_panel=%d\n", what, a.M, a.N, a.K,
              linear_name(p.kernel), p.geom, p.grid, p.lds, p.epi, tn.gemm_variant, tn.lat_tile, tn.row_panel);
}
static void check_plan(const LinearArgs& a, const LinearPlan& p, const d3pm_tuning& tn, bool dual) {
  ++g_cases;
  if (p.kernel == LIN_GENERIC || p.kernel == LIN_QUADS_REFUSED) return;
  ++g_planned;
  const bool big = p.kernel == LIN_BIG, panel = p.kernel == LIN_PANEL64;
  const int* table = dual ? (big ? kEpiBigDual : kEpiPanel64Dual) : big ? kEpiBig : panel ? kEpiPanel64 : kEpi128;
  if (!epi_listed(table, p.epi)) violation("epilogue_not_in_family_table", a, p, tn);
  if (p.grid == 0) violation("empty_grid", a, p, tn);
  if (p.lds > 160 * 1024) violation("lds_over_160KiB", a, p, tn);
  if ((p.epi & EPI_QUADS) && !big) violation("quads_off_big_tiles", a, p, tn);
  // (the panel64 dual has always been chosen without a look at moment_quads: fold_plan asks in the parts format and then keeps it)
  if (a.moment_quads && !big && !dual) violation("quad_arguments_off_big_tiles", a, p, tn);
  if (dual && big && p.geom < 2) violation("dual_on_geometry_1", a, p, tn);
  if (dual && !big && !panel) violation("dual_on_128_family", a, p, tn);
  if (big && (p.geom < 1 || p.geom > 3 || a.M % p.tm || a.N % p.tn)) violation("big_tiles_not_whole", a, p, tn);
  if (panel && (p.geom < 0 || p.geom > 2)) violation("panel64_geometry", a, p, tn);
  if (static_cast<long long>(p.grid) > static_cast<long long>(p.tiles_total)) {
    // persistent grids round up to the 8 XCDs: at most 7 idle workgroups
    if (static_cast<long long>(p.grid) > ((static_cast<long long>(p.tiles_total) + 7) & ~7ll)) violation("grid_over_tiles", a, p, tn);
  }
  g_seen.insert({dual ? (big ? 3 : 4) : big ? 1 : panel ? 2 : 0, p.epi, (big || panel) ? p.geom : 0});
}

static void sweep() {
  static const int Ms[] = {16, 96, 192, 768, 1152, 1536, 1728, 6144, 24576}, Ns[] = {64, 512, 1025, 1536, 2048}, Ks[] = {64, 256, 512, 2048};
  // every epilogue the three families list (d3pm_plan.cpp), and four that none does
  static const int epis[] = {0, EPI_GELU, EPI_R1, EPI_R2, EPI_R1 | EPI_MASK, EPI_LNF, EPI_LNF | EPI_GELU, EPI_R1 | EPI_STATS, EPI_R2 | EPI_STATS,
                             EPI_R1 | EPI_MASK | EPI_STATS, EPI_RELU, EPI_SILU, EPI_LNF | EPI_QUADS, EPI_LNF | EPI_GELU | EPI_QUADS,
                             EPI_R1 | EPI_STATS | EPI_QUADS, EPI_R2 | EPI_STATS | EPI_QUADS, EPI_R1 | EPI_MASK | EPI_STATS | EPI_QUADS,
                             EPI_GELU | EPI_R1, EPI_MASK, EPI_R2 | EPI_MASK, EPI_RELU | EPI_R1};
  static const int variants[] = {0, 2, 3, 4, 5, 6, 7, 8}, lat_tiles[] = {0, 1, 2, 3};
  for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int variant : variants) {
    d3pm_tuning tn = default_tuning();
    tn.gemm_variant = variant;
    for (int lat_tile : lat_tiles) {
      tn.lat_tile = lat_tile;
      for (int epi : epis) {
        const LinearArgs a = linear_args(M, N, K, epi, &tn);
        check_plan(a, plan_linear(D3PM_BF16, a), tn, false);
        check_plan(a, plan_linear(D3PM_F16, a), tn, false);
        if (plan_linear(D3PM_F32, a).mfma() || plan_linear(D3PM_BF16, a, true).mfma()) violation("fp32_or_forced_generic_on_mfma", a, plan_linear(D3PM_F32, a), tn);
      }
    }
    tn.lat_tile = 0;
    for (int row_panel = 0; row_panel < 16; ++row_panel) for (int epi : {EPI_R1, EPI_R1 | EPI_STATS, EPI_R1 | EPI_STATS | EPI_QUADS}) for (int allowed = 0; allowed < 2; ++allowed) {
      tn.row_panel = row_panel;
      const LinearArgs g = linear_args(M, N, K, epi, &tn);
      const CrossOutPlan c = plan_cross_out(D3PM_BF16, g, g_buf, false, allowed != 0);
      if (c.form == CROSS_OUT_TWO_LAUNCHES) { ++g_cases; continue; }
      check_plan(g, c.dual, tn, true);
      if ((c.form == CROSS_OUT_BIG_DUAL) != c.dual.big()) violation("dual_form_and_family_disagree", g, c.dual, tn);
      if (c.form == CROSS_OUT_BIG_DUAL && !allowed) violation("big_dual_where_not_allowed", g, c.dual, tn);
      if (plan_cross_out(D3PM_BF16, g, g_buf, true, allowed != 0).form != CROSS_OUT_TWO_LAUNCHES) violation("forced_generic_dual", g, c.dual, tn);
    }
  }
  // attention: every documented code of the three fields, self and cross, masked and not
  long attn_cases = 0;
  for (int q : {0, 1, 2, 4, 32, 33}) for (int r : {0, 1, 2, 3, 4, 5}) for (int ps : {0, 1, 2}) for (int B : {1, 2, 3, 10, 11, 32}) for (int regime : {0, 32})
    for (int cross = 0; cross < 2; ++cross) for (int masked = 0; masked < 3; ++masked) {
      d3pm_tuning tn = default_tuning();
      tn.attn_query_groups = q; tn.attn_cross_resident = r; tn.attn_pair_sequential = ps; tn.regime_batch = regime;
      AttnArgs a;
      a.Q = a.K = a.V = g_buf; a.O = g_buf; a.B = B; a.H = 8; a.hd = 64; a.Tq = 768; a.tune = &tn;
      a.S = cross ? 50 : 768; a.ldq = a.ldkv = 1536; a.ldo = 512;
      if (cross) { a.Q2 = a.K2 = a.V2 = g_buf; a.O2 = g_buf; a.S2 = 225; }
      if (masked) a.key_len = reinterpret_cast<const int32_t*>(g_buf);
      a.masked_keeps_schedule = masked == 2;
      const AttnPlan p = plan_attention(D3PM_BF16, a);
      ++attn_cases;
      const bool resident = p.kernel == ATTN_32_CROSS || p.kernel == ATTN_CROSS;
      const bool bad = !p.mfma() || p.grid == 0 || p.lds > 160 * 1024 || (resident && (!cross || p.n_qsplit < 1 || p.n_qsplit > p.n_qblocks)) ||
                       ((p.kernel == ATTN_32 || p.kernel == ATTN_32P) && cross) || (p.kernel == ATTN_SPLIT && (masked || q != 4)) ||
                       (p.kernel == ATTN_TILES && (p.qg < 1 || p.qg > 2 || (p.pair_seq && !cross))) || (masked && !p.masked) ||
                       plan_attention(D3PM_BF16, a, true).mfma() || plan_attention(D3PM_F32, a).mfma();
      if (bad) {
        ++g_violations;
        std::printf("violation what=attention q=%d r=%d ps=%d B=%d regime=%d cross=%d masked=%d kernel=%s grid=%u lds=%zu\n", q, r, ps, B, regime, cross, masked,
                    attn_name(p.kernel), p.grid, p.lds);
      }
    }
  for (const auto& t : g_seen) std::printf("seen family=%d epi=%d geom=%d\n", std::get<0>(t), std::get<1>(t), std::get<2>(t));
  std::printf("sweep cases=%ld planned=%ld attention=%ld violations=%ld\n", g_cases, g_planned, attn_cases, g_violations);
}

int main() {
  char name[64];
  for (int B : {1, 2, 3, 8, 10, 11, 16, 32}) {
    const int n = B * 768;
    auto one = [&](const char* what, int N, int K) {
      std::snprintf(name, sizeof name, "%s/%d", what, B);
      linear_case(name, n, N, K);
    };
    one("qkv", 1536, 512); one("out", 512, 512); one("q2", 1024, 512); one("fc1", 2048, 512); one("fc2", 512, 2048); one("final", 1025, 512);
  }
  linear_case("qkv_table", 1152, 1536, 512);
  linear_case("out_rows16", 16, 512, 512);
  linear_case("out_rows31", 31, 512, 512);
  linear_case("out_rows32", 32, 512, 512);
  linear_case("native_qkv", 448, 96, 32);
  for (int B : {8, 10, 11, 16, 32}) fold_cases(B);
  sequence_cases();

  d3pm_tuning tn = default_tuning();
  for (int B : {10, 11, 32}) attn_case("self", B, false, tn);
  attn_case("self_keylen_keeps", 32, false, tn, true, true);
  attn_case("self_keylen", 32, false, tn, true, false);
  for (int B : {1, 10, 11, 32}) attn_case("cross", B, true, tn);
  d3pm_tuning t33 = tn; t33.attn_query_groups = 33;
  attn_case("self_plain_walk", 32, false, t33);
  d3pm_tuning tr = tn; tr.regime_batch = 32;
  attn_case("self_regime32", 4, false, tr);
  d3pm_tuning t4 = tn; t4.attn_cross_resident = 4;
  attn_case("cross_resident16", 32, true, t4);
  d3pm_tuning ts = tn; ts.attn_query_groups = 4;
  attn_case("cross_split", 1, true, ts);

  sweep();
  return 0;
}
