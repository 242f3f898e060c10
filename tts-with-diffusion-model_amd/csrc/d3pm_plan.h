// d3pm_plan.h -- which kernel a projection or an attention call runs on, with which grid and how much LDS: decided here, once,
// by pure host functions of (dtype, arguments, tuning).  d3pm_plan.cpp holds no kernel and makes no HIP runtime call, so a test
// on a machine without a GPU can link it and read every choice (tests/test_launch_plan_api.py).  The launchers in
// d3pm_mfma_*.hip take a plan and only translate it into a template instantiation and a <<<>>>; d3pm_api.hip asks the planner
// for every launch it enqueues, and d3pm_sequence.{h,cpp} -- host-only by the same rule -- for the launches of a whole block when a
// call plans its loop.
#pragma once
#include "d3pm_kernels.h"

namespace d3pm {

constexpr int kCUs = 256;                                // compute units of the MI355X: every "fills the chip" rule counts in these

// ---- geometry shared by the planner and the kernels it plans for ----
constexpr int BK = 64;                                  // GEMM k-step: one 128-byte LDS row per tile row
constexpr int ROW_BYTES = BK * 2;
constexpr int BM = 128, BN = 128;                       // the 128 x 128 GEMM family (d3pm_mfma_gemm.hip)
constexpr int KC = 256;                                 // k per round of the panel64 family (d3pm_mfma_gemm_lat.hip)
constexpr int HD = 64, BKV = 64, ROWB = 128;            // attention: head width, keys per tile, bytes per K / V row
constexpr int TILE = BKV * ROWB;                        // 8 KiB per K or V tile
// gathered keys (AttnArgs::key_row, attn32p_hd64): the staged index, 4 bytes per key, shares a workgroup's 64 KiB with 48 KiB of tiles
constexpr size_t kGatherIndexBytes = 16 * 1024;
// the key pool (AttnArgs::seg_est, attn32p_hd64 POOL): tiles, staged index and 256 bytes per pool row within a workgroup's 160 KiB
constexpr size_t kAttnPoolLdsBytes = 160 * 1024;

// epilogue bits = the EPI template argument of every GEMM kernel (d3pm_mfma_tile.h epilogue_store)
constexpr int EPI_GELU = 1, EPI_R1 = 2, EPI_R2 = 4, EPI_MASK = 8, EPI_RELU = 16, EPI_SILU = 32, EPI_LNF = 64, EPI_STATS = 128;
constexpr int EPI_QUADS = 256;

// ---- projections ----
// LIN_GENERIC: the MFMA family does not take these arguments.  LIN_QUADS_REFUSED: it would, but not on big tiles, and the quad format
// of the row moments exists in the big-tile epilogues only (mfma_linear fails with D3PM_E_SHAPE).
enum LinearKernel { LIN_GENERIC = 0, LIN_QUADS_REFUSED, LIN_BIG, LIN_PANEL64, LIN_128_PF, LIN_128_PERSIST, LIN_128_GLDS };
struct LinearPlan {
  int kernel = LIN_GENERIC;
  int geom = 0;                  // LIN_BIG: 1 = 96 x 512, 2 = 192 x 256, 3 = 192 x 128, 4 = 96 x 128, 5 = 128 x 128;  LIN_PANEL64: 0 = 64 x 64, 1 = 96 x 64, 2 = 32 x 64
  int tm = 0, tn = 0;            // rows x columns of a tile
  int epi = 0;                   // EPI_* bits: an entry of the family's table below
  unsigned grid = 0;
  size_t lds = 0;                // dynamic LDS bytes
  int n_tiles = 0, tiles_total = 0;      // tiles along N, tiles in all
  bool mfma() const { return kernel != LIN_GENERIC; }
  bool big() const { return kernel == LIN_BIG; }
};
LinearPlan plan_linear(int dtype, const LinearArgs& a, bool force_generic = false);

// ---- the live rows of an iteration of the deduplicated loop, bounded on the host (the loop is graph-captured: no read-back) ----
// batch * min(canvas, 2 + ceil(canvas * (1 - cbar_t))): the revealed frames of an utterance in expectation (each at most one class of
// its own) plus the mask class and the padded one.  cbar_t = float(cbar[t]) of the schedule for the iteration that evaluates x_t.
int plan_live_rows(int batch, int canvas, float cbar_t);
// the regime rule: an iteration whose estimate is at most live_latency_rows() takes the latency launch list (every projection of a block
// on gemm_mfma_panel64, moments as parts); LinearArgs::m_est carries the estimate to plan_linear / plan_cross_out.  0 = no estimate.
int live_latency_rows();
inline bool live_latency(int m_est) { return m_est > 0 && m_est <= live_latency_rows(); }
// The second estimate, for the iterations that stay on big tiles (LinearArgs::rows_est): the DISTINCT classes among the revealed frames.
// batch * min(canvas, 2 + ceil(n_classes * (1 - exp(-r / n_classes)))) with r = canvas * (1 - cbar_t): r uniform draws from n_classes
// ids hit that many different ones in expectation, and a uniform draw maximises the count, so a trained model lies below it.  Never
// above plan_live_rows of the same arguments (n (1 - exp(-r / n)) <= r).  Erring high is the cheap side: a tile sized for more rows.
int plan_distinct_rows(int batch, int canvas, int n_classes, float cbar_t);
// the rule of big_tile for a producer with quads and 0 < rows_est < M whose capacity takes 192 x 128 tiles: 96 x 128 tiles up to
// live_short96_rows() estimated rows, 128 x 128 up to live_short128_rows(), each while its tiles fit the 2 * kCUs slots in one round
int live_short96_rows();
int live_short128_rows();

// ---- what d3pm_tuning.ln_fold switches on, by name: nothing outside fold_features compares the field with a number ----
// fold: the LayerNorms folded into the projections.  On top of it, each a condition among others of loop_plan (d3pm_sequence.h):
// table: block-0 QKV from the per-id table; dedup: one row per distinct token of an utterance; latency: the per-iteration switch of
// the deduplicated loop to the latency launch list.
struct FoldFeatures { bool fold, table, dedup, latency; };
FoldFeatures fold_features(const d3pm_tuning& tn);

// the instantiated epilogues of each family (the switch of its launcher has exactly these cases), 0-terminated after the first entry
extern const int kEpi128[], kEpiBig[], kEpiPanel64[], kEpiBigDual[], kEpiPanel64Dual[];
bool epi_listed(const int* table, int epi);

// do `tiles` fill >= 80 % of the slots and >= 85 % of their whole rounds over `slots` resident workgroups?
inline bool fills_rounds(long long tiles, long long slots) {
  const long long rounds = (tiles + slots - 1) / slots;
  return tiles * 5 >= slots * 4 && tiles * 100 >= rounds * slots * 85;
}

// ---- the cross-attention out-projection pair: x = (x + o_text) + o_prompt through the same weights ----
// Three forms with the same bits.  `g` is the o_text projection onto the residual stream (R1 = Y = x, tune set), X2 the o_prompt rows.
enum { CROSS_OUT_TWO_LAUNCHES = 0, CROSS_OUT_PANEL64_DUAL, CROSS_OUT_BIG_DUAL };
struct CrossOutPlan {
  int form = CROSS_OUT_TWO_LAUNCHES;
  LinearPlan dual;               // the one launch of the two dual forms: LIN_PANEL64 (32 x 64) or LIN_BIG (geometry 2 .. 5)
};
CrossOutPlan plan_cross_out(int dtype, const LinearArgs& g, const void* X2, bool force_generic, bool big_dual_allowed);

// ---- attention ----
enum AttnKernel {
  ATTN_GENERIC = 0,
  ATTN_32P,            // attn32p_hd64: self-attention on the 32 x 32 x 16 instruction, software-pipelined walk
  ATTN_32,             // attn32_hd64: the same, plain walk
  ATTN_32_CROSS,       // attn32_cross_hd64: the cross pair with K / V resident, 32 x 32 x 16
  ATTN_CROSS,          // attn_cross_hd64: the cross pair with K / V resident, 16 x 16 x 32
  ATTN_SPLIT,          // attn_split_hd64: key tiles split over the four waves
  ATTN_TILES,          // attn_mfma_hd64<qg, pair_seq>: tile by tile
  ATTN_32P_POOL        // attn32p_hd64 POOL: the gathered walk of ATTN_32P with the distinct K | V rows of an utterance pooled in LDS
};
struct AttnPlan {
  int kernel = ATTN_GENERIC;
  bool masked = false;           // the key-length arm (a template argument of the 32 x 32 x 16 and the resident kernels)
  int qg = 0;                    // ATTN_TILES: 16-query groups per wave (1 or 2)
  bool pair_seq = false;         // ATTN_TILES: a workgroup runs both problems of a pair one after the other
  int n_qsplit = 0;              // resident cross kernels: workgroups per (utterance, head)
  int n_qblocks = 0;             // ATTN_32P_POOL: the query blocks per (utterance, head) in the grid; a workgroup strides over the rest
  int pool_rows = 0;             // ATTN_32P_POOL: rows of the K | V pool
  int n_first = 0;               // paired grids: workgroups of the first problem (-1: sequential pair)
  unsigned grid = 0;
  size_t lds = 0;                // dynamic LDS bytes
  bool mfma() const { return kernel != ATTN_GENERIC; }
};
AttnPlan plan_attention(int dtype, const AttnArgs& a, bool force_generic = false);
// the largest AttnArgs::seg_est that takes the pooled self-attention, and the rows of its pool
int attn_pool_rows();

// the batch the automatic attention choices are made for (a shard of a split batch takes the kernels of the whole batch)
inline int logical_batch(const d3pm_tuning& tn, int B) { return tn.regime_batch > 0 ? tn.regime_batch : B; }

}  // namespace d3pm
