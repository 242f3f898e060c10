// live_rows_plan_table.cpp -- prints the host-side live-row estimate and the launch planner's choices under it (csrc/d3pm_plan.cpp) for
// tests/test_live_rows_plan_api.py.  Host only, like launch_plan_table.cpp.
//   live_rows_plan_table BATCH CANVAS CBAR_0 CBAR_1 ...      one `est` line per cbar value, then the projections of a block
#include <cstdio>
#include <cstdlib>

#include "d3pm_plan.h"

using namespace d3pm;

static char g_buf[256] __attribute__((aligned(64)));      // every pointer of a case: aligned, never dereferenced

static const char* linear_name(int k) { return k == LIN_BIG ? "big" : k == LIN_PANEL64 ? "panel64" : k == LIN_128_GLDS ? "128glds" : "other"; }

static LinearArgs linear_args(int M, int N, int K, int epi, int m_est) {
  LinearArgs a;
  a.X = a.W = a.bias = g_buf; a.Y = g_buf;
  a.M = M; a.N = N; a.K = K; a.ldx = K; a.ldy = N; a.ldr = N;
  a.act = (epi & EPI_GELU) ? ACT_GELU : ACT_NONE;
  if (epi & (EPI_R1 | EPI_R2)) a.R1 = g_buf;
  if (epi & EPI_MASK) { a.row_mask = reinterpret_cast<const uint8_t*>(g_buf); a.mask_period = M; }
  if (epi & EPI_LNF) { a.fold_s = a.fold_b = a.stats_in = reinterpret_cast<const float*>(g_buf); a.bias = nullptr; }
  if (epi & EPI_STATS) a.stats_out = reinterpret_cast<float*>(g_buf);
  a.m_live = reinterpret_cast<const int*>(g_buf);
  a.m_est = m_est;
  return a;
}

static void print_plan(const char* what, int B, int m_est, bool quads, const LinearArgs& a, const LinearPlan& p, const int* table, int form) {
  std::printf("linear case=%s B=%d m_est=%d quads=%d M=%d N=%d kernel=%s geom=%d tm=%d tn=%d grid=%u n_tiles=%d tiles_total=%d epi=%d listed=%d form=%d\n", what, B,
              m_est, quads ? 1 : 0, a.M, a.N, linear_name(p.kernel), p.geom, p.tm, p.tn, p.grid, p.n_tiles, p.tiles_total, p.epi,
              epi_listed(table, p.epi) ? 1 : 0, form);
}

// the launches of folded_block (d3pm_api.hip) over B utterances of 768 frames at d = 512 with the estimate m_est; quads as the loop
// passes them (the big-tile iterations) or parts (the latency iterations)
static void block_cases(int B, int m_est, bool quads) {
  const int n = B * 768, d = 512;
  auto one = [&](const char* what, int N, int K, int epi) {
    LinearArgs a = linear_args(n, N, K, epi, m_est);
    a.moment_quads = quads;
    const LinearPlan p = plan_linear(D3PM_BF16, a);
    print_plan(what, B, m_est, quads, a, p, p.kernel == LIN_PANEL64 ? kEpiPanel64 : p.kernel == LIN_BIG ? kEpiBig : kEpi128, -1);
  };
  one("qkv", 3 * d, d, EPI_LNF);
  one("out", d, d, EPI_R1 | EPI_STATS);
  one("q2", 2 * d, d, EPI_LNF);
  LinearArgs g = linear_args(n, d, d, EPI_R1 | EPI_STATS, m_est);
  g.moment_quads = quads;
  const CrossOutPlan c = plan_cross_out(D3PM_BF16, g, g_buf, false, true);
  print_plan("cross", B, m_est, quads, g, c.dual, c.form == CROSS_OUT_PANEL64_DUAL ? kEpiPanel64Dual : kEpiBigDual, c.form);
  one("fc1", 4 * d, d, EPI_LNF | EPI_GELU);
  one("fc2", d, 4 * d, EPI_R1 | EPI_MASK | EPI_STATS);
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int batch = std::atoi(argv[1]), canvas = std::atoi(argv[2]);
  const int R = live_latency_rows();
  std::printf("bound R=%d\n", R);
  for (int i = 3; i < argc; ++i) {
    const int est = plan_live_rows(batch, canvas, static_cast<float>(std::atof(argv[i])));
    std::printf("est t=%d rows=%d latency=%d\n", i - 3, est, live_latency(est) ? 1 : 0);
  }
  for (int B : {11, 16, 32}) {
    block_cases(B, 0, true);
    for (int m_est : {1, 64, 385, R / 2, R}) block_cases(B, m_est, false);
    block_cases(B, R + 1, true);
    block_cases(B, B * 768 + 5, true);
  }
  return 0;
}
