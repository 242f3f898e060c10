// few_rows_plan_table.cpp -- prints the self-attention plans of the deduplicated loop under the host's per-utterance row estimate
// (csrc/d3pm_plan.cpp: plan_attention with AttnArgs::seg_est, attn_pool_rows) for tests/test_few_rows_plan_api.py and
// tests/test_gpu_few_rows_loop.py.  Host only, like launch_plan_table.cpp.
//   few_rows_plan_table BATCH CANVAS CBAR_0 CBAR_1 ...      one `iter` line per cbar value, then `attn` cases
#include <cstdio>
#include <cstdlib>

#include "d3pm_plan.h"

using namespace d3pm;

static char g_buf[256] __attribute__((aligned(64)));      // every pointer of a case: aligned, never dereferenced

// the self-attention of folded_block (d3pm_sequence.h) over B utterances of `canvas` frames, 8 heads of 64, k | v in [rows][3 d]
static AttnArgs self_args(int B, int canvas, int seg_est, bool gather, bool seg_key, bool masked) {
  const int d = 512;
  const int32_t* ip = reinterpret_cast<const int32_t*>(g_buf);
  AttnArgs a;
  a.Q = a.K = a.V = g_buf; a.O = g_buf;
  a.ldq = a.ldkv = 3 * d; a.ldo = d;
  a.B = B; a.Tq = canvas; a.S = canvas; a.H = 8; a.hd = 64; a.scale = 0.125f;
  a.seg_start = a.seg_len = ip;
  if (gather) { a.key_row = ip; a.kv_rows = B * canvas; }
  if (seg_key) a.seg_key = ip;
  if (masked) { a.key_len = ip; a.masked_keeps_schedule = true; }
  a.seg_est = seg_est;
  return a;
}

static void print_attn(const char* what, int B, int canvas, int seg_est, const AttnPlan& p) {
  std::printf("attn case=%s B=%d canvas=%d seg_est=%d kernel=%d masked=%d n_qblocks=%d pool_rows=%d grid=%u lds=%zu total_lds=%zu\n", what, B, canvas,
              seg_est, p.kernel, p.masked ? 1 : 0, p.n_qblocks, p.pool_rows, p.grid, p.lds, p.lds + 3 * 2 * static_cast<size_t>(TILE));
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int batch = std::atoi(argv[1]), canvas = std::atoi(argv[2]);
  const int P = attn_pool_rows();
  std::printf("bound P=%d R=%d ATTN_32P=%d ATTN_32P_POOL=%d\n", P, live_latency_rows(), static_cast<int>(ATTN_32P), static_cast<int>(ATTN_32P_POOL));
  for (int i = 3; i < argc; ++i) {      // what the loop asks in iteration t = i - 3 (LoopPlan::m_est / seg_est)
    const int est = plan_live_rows(batch, canvas, static_cast<float>(std::atof(argv[i])));
    const int seg_est = (est + batch - 1) / batch;
    const AttnPlan p = plan_attention(D3PM_BF16, self_args(batch, canvas, seg_est, true, true, false));
    std::printf("iter t=%d rows=%d seg_est=%d latency=%d kernel=%d grid=%u\n", i - 3, est, seg_est, live_latency(est) ? 1 : 0, p.kernel, p.grid);
  }
  for (int B : {16, 32}) {
    for (int seg_est : {0, 1, 2, 127, P, P + 1, 2 * P, 768, 100000}) {
      print_attn("loop", B, 768, seg_est, plan_attention(D3PM_BF16, self_args(B, 768, seg_est, true, true, false)));
      print_attn("masked", B, 768, seg_est, plan_attention(D3PM_F16, self_args(B, 768, seg_est, true, true, true)));
      print_attn("no_seg_key", B, 768, seg_est, plan_attention(D3PM_BF16, self_args(B, 768, seg_est, true, false, false)));
      print_attn("no_gather", B, 768, seg_est, plan_attention(D3PM_BF16, self_args(B, 768, seg_est, false, true, false)));
    }
  }
  // the longest canvas whose index the gathered kernel stages: pool and index still inside a workgroup's LDS
  print_attn("long", 32, 4096, P, plan_attention(D3PM_BF16, self_args(32, 4096, P, true, true, false)));
  {   // a pool named by the caller (d3pm_op_attention_gather_pool): 384 rows fit, 512 do not and keep the gathered kernel
    for (int rows : {384, 512}) {
      AttnArgs a = self_args(2, 512, 0, true, true, false);
      d3pm_tuning tn = tune_of(nullptr);
      tn.attn_query_groups = 32;
      a.tune = &tn; a.pool_rows = rows; a.qblocks_grid = 1;
      print_attn(rows == 384 ? "named384" : "named512", 2, 512, 0, plan_attention(D3PM_BF16, a));
    }
  }
  return 0;
}
