// d3pm_plan.cpp -- the kernel choices of d3pm_plan.h.  Host code only: no kernel, no launch, no HIP runtime call.
// All GEMM schedules accumulate in the same order, so a choice made here never changes a bit of a projection's result; the
// attention instruction shape (16 x 16 x 32 or 32 x 32 x 16) does, which is why it follows the LOGICAL batch.
#include "d3pm_plan.h"

#include <cmath>
#include <cstdint>

namespace d3pm {
namespace {

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) % 16) == 0; }
inline bool is16(int dtype) { return dtype == D3PM_F16 || dtype == D3PM_BF16; }

// operand and stride alignment every MFMA GEMM family asks for (16-byte rows, 16-byte epilogue loads and stores)
bool operands_ok(const LinearArgs& a) {
  if (a.ldx % 8 != 0 || a.ldy % 8 != 0 || !al16(a.X) || !al16(a.W) || !al16(a.Y)) return false;
  if (a.R1 && (a.ldr % 8 != 0 || a.N % 8 != 0 || !al16(a.R1))) return false;
  if (a.R2 && !al16(a.R2)) return false;
  return true;
}

// the EPI bits of `a`; the quad format is a bit of the big-tile family alone
int epi_of(const LinearArgs& a) {
  return (a.act == ACT_GELU ? EPI_GELU : a.act == ACT_RELU ? EPI_RELU : a.act == ACT_SILU ? EPI_SILU : 0) |
         (a.R1 ? (a.R2 ? EPI_R2 : EPI_R1) : 0) | (a.row_mask ? EPI_MASK : 0) | (a.fold_s ? EPI_LNF : 0) | (a.stats_out ? EPI_STATS : 0);
}

// Is the epilogue `a` asks for one of the family's instantiated ones?  R2 without R1 is none (epi_of would read it as plain) -- except
// under ReLU / SiLU, where the 128 x 128 family has always let a stray R2 through unread; carried over as it was.
bool epi_ok(const int* table, const LinearArgs& a) {
  if (a.R2 && !a.R1 && a.act != ACT_RELU && a.act != ACT_SILU) return false;
  return epi_listed(table, epi_of(a));
}

// ---- 128 x 128 family (d3pm_mfma_gemm.hip): the precondition of every MFMA projection ----
bool k128_ok(int dtype, const LinearArgs& a) {
  if (!is16(dtype)) return false;
  if (a.M < 1 || a.N < 1 || a.K < BK || a.K % BK != 0) return false;
  if (!operands_ok(a)) return false;
  if (static_cast<long long>(a.M) * a.N < 128 * 128) return false;     // not worth a 128^2 tile
  return fold_args_ok(a) && epi_ok(kEpi128, a);
}

// ---- big tiles (d3pm_mfma_gemm_big.hip) ----
// Tile geometries: id 1 = 96 x 512 (1 x 8 waves), 2 = 192 x 256 (2 x 4 waves), 3 = 192 x 128 (2 x 2 waves, two workgroups per CU);
// the short tiles of the deduplicated loop's producers: 4 = 96 x 128, 5 = 128 x 128 (2 x 2 waves of three / four 16-row blocks)
void big_geometry(int id, int& tm, int& tn, int& waves) {
  tm = id == 1 || id == 4 ? 96 : id == 5 ? 128 : 192;
  tn = id == 1 ? 512 : id == 2 ? 256 : 128;
  waves = id >= 3 ? 4 : 8;
}

// The short tiles are instantiated for what the loop launches on them and nothing else: the projections onto the residual stream with
// quads -- R1 [+ mask] + moments, and the dual out-projection, whose first launch argument looks the same (plan_cross_out)
bool short_tile_epilogue(const LinearArgs& a) {
  return a.stats_out && a.moment_quads && a.R1 && !a.R2 && a.act == ACT_NONE && !a.fold_s;
}

// today's automatic choice among the geometries 1 .. 3 for the capacity a.M (0: none)
int big_tile_capacity(const LinearArgs& a) {
  auto fits = [&](int id) {
    int tm, tn, waves;
    big_geometry(id, tm, tn, waves);
    if (a.M % tm != 0 || a.N % tn != 0) return false;
    return fills_rounds(static_cast<long long>(a.M / tm) * (a.N / tn), kCUs * (8 / waves));   // >= 85 % of the slot-rounds do work
  };
  // Under the GELU epilogue 192 x 128 tiles win clearly: its VALU work only overlaps with MFMAs when a second workgroup shares the
  // CU (two 4-wave workgroups per CU).  For the other K = 512 projections the microbenchmark cannot tell 192 x 128 from 192 x 256
  // (qkv 43.3 vs 44.5 us, merged q 30.5 vs 31.4: profiles/round3_v_ab_gemm_geometries.txt) but the sampler's loop can, where the
  // operands arrive cold from the previous launch and two independent workgroups per CU hide that better than one: GEMM class
  // 1317 -> 1241 us per iteration, 97.8 k -> 101.2 k tokens/s with 192 x 128 everywhere (interleaved arms of bench.py --tune
  // gemm_variant=8, profiles/round3_v_ab_tune_geom.txt)
  // -- and fc2 (K = 2048) likewise: with 192 x 128 for the K = 512 projections only the class is at 1294 us, with fc2 too at 1249
  // (profiles/round3_w_ab_tune_geom.txt).  So: two 4-wave workgroups per CU wherever that geometry fills its rounds.
  if (fits(3)) return 3;
  if (fits(2)) return 2;
  if (fits(1)) return 1;
  // Mid-size batches (the VCTK config: 32 x 384 rows; 8 .. 16 utterances of the libritts shape) leave the chip partly idle with
  // every big tile, yet 192 x 128 tiles of four waves still beat the 128 x 128 kernels there once at least half (long K) or all
  // of the CUs get one: measured at M = 12288 / 6144 (tests/ab_gemm_shapes.py, profiles/round3_f_ab_gemm_shapes.txt): qkv 24.1 vs
  // 26.6 / 15.6 vs 17.2 us, out-projection 12.8 vs 15.8 us, fc2 31.8 vs 39.0 / 29.5 vs 35.4 us
  if (a.M % 192 == 0 && a.N % 128 == 0) {
    const long long tiles = static_cast<long long>(a.M / 192) * (a.N / 128);
    if (tiles >= (a.K >= 1024 ? kCUs / 2 : kCUs)) return 3;
  }
  return 0;
}

// 0 = not applicable, else the geometry id.  `want` (tuning knob): 0 auto, 1 .. 5 forced (4 / 5 where they are instantiated, else auto).
int big_tile(int dtype, const LinearArgs& a, int want) {
  if (!is16(dtype)) return 0;
  if (a.K < 4 * BK || a.K % (2 * BK) != 0 || a.M < 96 || a.N < 128) return 0;
  if (!operands_ok(a)) return 0;
  if (!fold_args_ok(a) || (a.fold_s && a.K != 512)) return 0;      // the big tile prefetches the 16 moment parts of a 512-wide row
  if (!epi_ok(kEpiBig, a)) return 0;
  if (a.ldx >= (1 << 24) || a.K >= (1 << 24)) return 0;       // 32-bit per-lane DMA offsets
  auto whole = [&](int id) {                                   // tuning knob / kernel tests: any shape of whole tiles
    int tm, tn, waves;
    big_geometry(id, tm, tn, waves);
    return a.M % tm == 0 && a.N % tn == 0;
  };
  if (want >= 1 && want <= 3) return whole(want) ? want : 0;
  if ((want == 4 || want == 5) && short_tile_epilogue(a) && whole(want)) return want;
  const int id = big_tile_capacity(a);
  // A producer of the deduplicated loop with an estimate of its live rows below the capacity (LinearArgs::rows_est): the kernel walks
  // the live tiles alone, so what counts is how THEY lie on the chip.  A shorter tile spreads the same rows over more workgroups, each
  // of which stages (96 | 128) + 128 operand rows per k-step instead of 320 through its CU's L2 -> LDS path.  Measured along the
  // 32 x 750-frame loop with each tile forced in every iteration (profiles/round26_live_tiles_ab_interleaved.txt), fc2 / dual / self
  // out-projection in us per launch: at t = 73 (3 180 live rows) 192 x 128 takes 32.7 / 21.0 / 15.3, 128 x 128 27.3 / 17.1 / 12.1,
  // 96 x 128 25.0 / 15.4 / 10.8; at t = 35 (about 11 500) 36.4 / 22.8 / 15.9, 34.8 / 22.7 / 14.5 and 34.3 / 19.8 / 13.1; at t = 1
  // (14 997) 42.7 / 28.7 / 18.2, 39.1 / 24.0 / 15.3 and 55.4 / 31.8 / 19.5.  The 96-row tile wins while its tiles fit the 512 workgroup slots (two
  // four-wave workgroups per CU) and loses a whole round beyond (12 288 rows at N = 512); the 128-row tile wins from there to its own
  // last whole round (16 384 rows).  So: the shortest tile whose tiles of the ESTIMATE fit the slots in one round, bounded by
  // live_short96_rows() / live_short128_rows().  The estimate errs high (plan_distinct_rows), which here costs a few us; erring low
  // would cost a round.  192 x 256 tiles (one eight-wave workgroup per CU) were measured for the late iterations and lost everywhere.
  // Correctness never depends on the estimate: every geometry accumulates in the same order.
  if (id == 3 && want == 0 && a.m_live && a.rows_est > 0 && a.rows_est < a.M && short_tile_epilogue(a)) {
    const long long n_tiles = a.N / 128, slots = 2 * kCUs;
    if (a.rows_est <= live_short96_rows() && whole(4) && (a.rows_est + 95) / 96 * n_tiles <= slots) return 4;
    if (a.rows_est <= live_short128_rows() && whole(5) && (a.rows_est + 127) / 128 * n_tiles <= slots) return 5;
  }
  return id;
}

// a persistent launch of geometry `id` over the whole tiles of M x N: at most one workgroup per slot, a multiple of the 8 XCDs
LinearPlan big_plan(const LinearArgs& a, int id, int epi) {
  LinearPlan p;
  int waves;
  big_geometry(id, p.tm, p.tn, waves);
  p.kernel = LIN_BIG; p.geom = id; p.epi = epi;
  p.n_tiles = a.N / p.tn; p.tiles_total = (a.M / p.tm) * p.n_tiles;
  const int slots = kCUs * (8 / waves), want = (p.tiles_total + 7) & ~7;
  p.grid = static_cast<unsigned>(want < slots ? want : slots);
  p.lds = 2 * static_cast<size_t>(p.tm + p.tn) * ROW_BYTES;
  return p;
}

// ---- panel64 (d3pm_mfma_gemm_lat.hip): TM x 64 tiles, whole-K panels ----
constexpr int kPanelTm[3] = {64, 96, 32};
inline size_t panel64_xoper(int tm) { return static_cast<size_t>(KC / BK) * tm * ROW_BYTES; }      // the X panel of a round
inline size_t panel64_buf(int tm) { return panel64_xoper(tm) + panel64_xoper(64); }                // X + W of a round

bool panel64_ok(int dtype, const LinearArgs& a) {
  if (!is16(dtype)) return false;
  if (a.M < 1 || a.N < 16 || a.K < KC || a.K % KC != 0) return false;
  if (!operands_ok(a)) return false;
  return epi_ok(kEpiPanel64, a) && fold_args_ok(a);
}

// d3pm_tuning.lat_tile: 0 auto, 1 / 2 / 3 = always 64 x 64 / 96 x 64 / 32 x 64.  Auto: the geometry with the fewest rounds over the
// CUs (one workgroup per CU), then the one with the most workgroups (the time of a launch here is the latency of one
// workgroup's chain -- DMA flight, k-steps, epilogue -- so a round less or a shorter chain is what pays; flops do not matter)
// the rows a panel64 launch is sized for: the capacity, or the estimate of the live rows below it (LinearArgs::m_est)
inline int panel64_rows(const LinearArgs& a) { return a.m_est > 0 && a.m_est < a.M ? a.m_est : a.M; }

int panel64_geometry(const LinearArgs& a) {
  const int lat_tile = tune_of(a.tune).lat_tile;
  if (lat_tile >= 1 && lat_tile <= 3) return lat_tile - 1;
  const int rows = panel64_rows(a);
  int best = 0;
  long long best_rounds = 0, best_tiles = 0;
  for (int g = 0; g < 3; ++g) {
    const long long tiles = static_cast<long long>((rows + kPanelTm[g] - 1) / kPanelTm[g]) * ((a.N + 63) / 64), rounds = (tiles + kCUs - 1) / kCUs;
    if (g == 0 || rounds < best_rounds || (rounds == best_rounds && tiles > best_tiles)) { best = g; best_rounds = rounds; best_tiles = tiles; }
  }
  return best;
}

LinearPlan panel64_plan(const LinearArgs& a, int geom, int epi, bool dual) {
  LinearPlan p;
  p.kernel = LIN_PANEL64; p.geom = geom; p.tm = kPanelTm[geom]; p.tn = 64; p.epi = epi;
  p.n_tiles = (a.N + 63) / 64; p.tiles_total = ((a.M + p.tm - 1) / p.tm) * p.n_tiles;
  // the grid covers the estimated live rows; the kernel walks tile, tile + grid, .. over the live tiles it reads from the device
  p.grid = static_cast<unsigned>(((panel64_rows(a) + p.tm - 1) / p.tm) * p.n_tiles);
  p.lds = 2 * panel64_buf(p.tm) + (dual ? 2 * panel64_xoper(p.tm) : 0);      // dual: the second operand's panel rides in beside
  return p;
}

// d3pm_tuning.gemm_variant -> the big-tile geometry it forces (0: the automatic choice).  6 / 7 / 8 = 192 x 256 / 96 x 512 / 192 x 128;
// 9 / 10 = 96 x 128 / 128 x 128 for the producers they are instantiated for, the automatic choice for everything else.
inline int big_want(int gemm_variant) {
  return gemm_variant == 6 ? 2 : gemm_variant == 7 ? 1 : gemm_variant == 8 ? 3 : gemm_variant == 9 ? 4 : gemm_variant == 10 ? 5 : 0;
}
// The dual reads 6 and 8 only: 7 (96 x 512) means "auto" to it, because the dual needs geometry >= 2.  Carried over as it was on
// purpose: whether 7 should rather switch the dual off is a behaviour question of its own.
inline int big_want_dual(int gemm_variant) { return gemm_variant == 6 ? 2 : gemm_variant == 8 ? 3 : gemm_variant == 9 ? 4 : gemm_variant == 10 ? 5 : 0; }

}  // namespace

// instantiated epilogues: plain, GELU, R1, R1+R2, R1+mask; LNF, LNF+GELU; R1 / R2 / R1+mask + STATS
#define D3PM_EPI_COMMON                                                                                                             \
  0, EPI_GELU, EPI_R1, EPI_R2, EPI_R1 | EPI_MASK, EPI_LNF, EPI_LNF | EPI_GELU, EPI_R1 | EPI_STATS, EPI_R2 | EPI_STATS,           \
      EPI_R1 | EPI_MASK | EPI_STATS
// ... + the condition-encoder FFN epilogues.  ReLU and SiLU always take gemm_mfma_128_glds, and only without residual, mask, fold or
// moments (deliberate: the encoders run once per call, nothing else was ever measured for them)
const int kEpi128[] = {D3PM_EPI_COMMON, EPI_RELU, EPI_SILU, 0};
// ... + the quad format of the row moments on everything that reads or writes them
const int kEpiBig[] = {D3PM_EPI_COMMON, EPI_LNF | EPI_QUADS, EPI_LNF | EPI_GELU | EPI_QUADS, EPI_R1 | EPI_STATS | EPI_QUADS,
                       EPI_R2 | EPI_STATS | EPI_QUADS, EPI_R1 | EPI_MASK | EPI_STATS | EPI_QUADS, 0};
const int kEpiPanel64[] = {D3PM_EPI_COMMON, 0};
#undef D3PM_EPI_COMMON
// two products through one tile: x' = rn(rn(R1 + h) + y2), i.e. the R1 + R2 epilogue with R2 from registers (big) / R1 + h (panel64)
const int kEpiBigDual[] = {EPI_R2, EPI_R2 | EPI_STATS, EPI_R2 | EPI_STATS | EPI_QUADS, 0};
const int kEpiPanel64Dual[] = {EPI_R1, EPI_R1 | EPI_STATS, 0};

bool epi_listed(const int* table, int epi) {
  if (table[0] == epi) return true;
  for (int i = 1; table[i] != 0; ++i)
    if (table[i] == epi) return true;
  return false;
}

// d3pm_tuning.gemm_variant: 0 auto, 2 throughput (128 x 128 persistent over whole tiles), 3 the round-1 latency schedule
// (128 x 128, two stages), 4 the latency schedule (64 x 64 tiles, whole-K panels), 5 throughput with one 128 x 128 tile per
// workgroup, 6 / 7 / 8 big tiles (192 x 256 / 96 x 512 / 192 x 128, d3pm_mfma_gemm_big.hip) wherever they apply, else as auto
// without big tiles, 9 / 10 the short tiles (96 x 128 / 128 x 128) for the producers with quads, auto for everything else.  gemm_persist_slots: resident workgroups of the persistent schedule (4 per CU).
LinearPlan plan_linear(int dtype, const LinearArgs& a, bool force_generic) {
  LinearPlan p;
  if (force_generic || !k128_ok(dtype, a)) return p;
  const d3pm_tuning& tn = tune_of(a.tune);
  const int variant = tn.gemm_variant;
  // below 8 the slot count means the default (deliberate: 0 in a zero-initialised d3pm_tuning); otherwise whole groups of the 8 XCDs
  const int persist_slots = tn.gemm_persist_slots >= 8 ? (tn.gemm_persist_slots & ~7) : 4 * kCUs;
  const bool autosel = variant == 0 || (variant >= 6 && variant <= 10);
  const int epi = epi_of(a);
  // an iteration of the deduplicated loop with few live rows: the latency family whatever the capacity (moments as parts: the loop
  // chooses the format per iteration, LoopPlan::m_est in d3pm_sequence.h)
  if (variant == 0 && live_latency(a.m_est) && !a.moment_quads && panel64_ok(dtype, a)) return panel64_plan(a, panel64_geometry(a), epi, false);
  if (autosel)
    if (const int id = big_tile(dtype, a, big_want(variant))) return big_plan(a, id, epi | (a.moment_quads ? EPI_QUADS : 0));
  if (a.moment_quads) {            // the quad format of the row moments exists in the big-tile epilogues only
    p.kernel = LIN_QUADS_REFUSED;
    return p;
  }
  const bool few_rows = autosel && a.M <= 1536;       // one or two utterances: the latency families
  // 64 x 64 tiles with whole-K panels in flight (d3pm_mfma_gemm_lat.hip); 4 forces it for any M
  if ((variant == 4 || few_rows) && panel64_ok(dtype, a)) return panel64_plan(a, panel64_geometry(a), epi, false);
  const bool ffn_act = a.act == ACT_RELU || a.act == ACT_SILU;
  const bool latency = !ffn_act && (variant == 3 || few_rows);
  p.tm = BM; p.tn = BN; p.epi = epi;
  p.n_tiles = (a.N + BN - 1) / BN;
  const int m_tiles = (a.M + BM - 1) / BM;
  p.tiles_total = p.n_tiles * m_tiles;
  // shapes made of whole tiles go through the persistent kernel once there are enough tiles to fill the chip twice
  // over (a ragged edge would need a second launch that costs more than persistence gains: measured on N = 1025)
  const bool persist = !latency && !ffn_act && (autosel || variant == 2) && a.M % BM == 0 && a.N % BN == 0 &&
                       static_cast<long long>(p.n_tiles) * m_tiles >= 2 * kCUs &&
                       static_cast<long long>(BM) * a.ldx * 2 < (1ll << 31) && static_cast<long long>(BN) * a.K * 2 < (1ll << 31);
  p.kernel = latency ? LIN_128_PF : persist ? LIN_128_PERSIST : LIN_128_GLDS;
  p.lds = static_cast<size_t>(latency ? 4 : 2) * BM * ROW_BYTES;   // 64 KiB: two workgroups per CU; 32 KiB: four
  const int want = (p.tiles_total + 7) & ~7;
  p.grid = static_cast<unsigned>(persist ? (want < persist_slots ? want : persist_slots) : p.tiles_total);
  return p;
}

CrossOutPlan plan_cross_out(int dtype, const LinearArgs& g, const void* X2, bool force_generic, bool big_dual_allowed) {
  CrossOutPlan c;
  if (force_generic) return c;
  const d3pm_tuning& tn = tune_of(g.tune);
  const bool dual_args = X2 && al16(X2) && g.R1 && !g.R2 && !g.row_mask && g.act == ACT_NONE && g.bias && !g.fold_s;
  if (!dual_args) return c;
  // one or two utterances: both products through one resident weight panel of the latency GEMM (o_text stays in registers):
  // whole 32 x 64 tiles, K = 512 (both operand panels and the weight panel resident: 128 KiB)
  // (g.moment_quads is not looked at, as it never was: this form writes parts, and fold_plan, which asks in the parts format, answers
  // FOLD_PARTS whenever it is chosen -- d3pm_sequence.h FoldPlanner::dual)
  if ((tn.row_panel & 8) && tn.gemm_variant == 0 && panel64_ok(dtype, g) && g.K == 2 * KC && g.M % 32 == 0 && g.N % 64 == 0 &&
      (g.M <= 2048 || live_latency(g.m_est))) {
    c.form = CROSS_OUT_PANEL64_DUAL;
    c.dual = panel64_plan(g, 2, EPI_R1 | (g.stats_out ? EPI_STATS : 0), true);
    return c;
  }
  // throughput batches: the same two products through one tile of the ordinary big-tile launch (the first result kept packed in 48
  // registers); with stats_out, the row moments of x' for the folded norm3 of fc1
  if (big_dual_allowed && (tn.row_panel & 2)) {
    const int id = big_tile(dtype, g, big_want_dual(tn.gemm_variant));
    if (id >= 2) {
      c.form = CROSS_OUT_BIG_DUAL;
      c.dual = big_plan(g, id, EPI_R2 | (g.stats_out ? EPI_STATS | (g.moment_quads ? EPI_QUADS : 0) : 0));
    }
  }
  return c;      // two launches: o_text -> ws.h, then o_prompt with R1 = x, R2 = h
}

// ---- the live rows of a deduplicated iteration ----
int plan_live_rows(int batch, int canvas, float cbar_t) {
  const float revealed = static_cast<float>(canvas) * (1.0f - cbar_t);
  long long per_utt = 2 + static_cast<long long>(std::ceil(revealed > 0.f ? revealed : 0.f));
  if (per_utt > canvas) per_utt = canvas;
  const long long rows = static_cast<long long>(batch) * per_utt;
  return rows > INT32_MAX ? INT32_MAX : static_cast<int>(rows);
}

int plan_distinct_rows(int batch, int canvas, int n_classes, float cbar_t) {
  const double revealed = static_cast<float>(canvas) * (1.0f - cbar_t);      // plan_live_rows' float product, so that ceil never exceeds its
  const double n = n_classes > 0 ? static_cast<double>(n_classes) : 1.0;
  const double distinct = revealed > 0.0 ? n * (1.0 - std::exp(-revealed / n)) : 0.0;      // <= revealed
  long long per_utt = 2 + static_cast<long long>(std::ceil(distinct));
  if (per_utt > canvas) per_utt = canvas;
  const long long rows = static_cast<long long>(batch) * per_utt;
  return rows > INT32_MAX ? INT32_MAX : static_cast<int>(rows);
}

// The largest estimates that take the 96-row and the 128-row tile (big_tile, where the measurements are).  Compile-time constants
// like R below so that A/B builds can move them; big_tile also asks that the tiles fit the 512 slots in one round, which at N = 512
// is the same 12 288 and 16 384 rows.
#ifndef D3PM_LIVE_SHORT96_ROWS
#define D3PM_LIVE_SHORT96_ROWS 12288
#endif
#ifndef D3PM_LIVE_SHORT128_ROWS
#define D3PM_LIVE_SHORT128_ROWS 16384
#endif
int live_short96_rows() { return D3PM_LIVE_SHORT96_ROWS; }
int live_short128_rows() { return D3PM_LIVE_SHORT128_ROWS; }

// R, the largest estimate that takes the latency launch list: measured, not derived (profiles/round19_live_regime_ab_interleaved.txt).
// Interleaved arms of the 32 x 750-frame bf16 loop over library builds that differ in this constant alone (tools/build_variant.py), ms
// per step: R = 1536 (the planner's few_rows bound) 120.1, 3072 118.8, 4608 118.3, 6144 118.4 against the parent's 125.9 on one box;
// 4608 116.4, 6144 116.6, 7680 118.0, 9216 119.0, 12288 122.6 against 124.0 on another.  The step time is flat from 3072 to 6144,
// so the bound comes from the kernel trace of the R = 4608 build: an iteration's kernels take 890 us against the parent's 956 at
// t = 75 (estimate 3520), 995 against 983 at t = 73 (4064: break-even) and 1040 against 979 at t = 72 (4352: a loss; fc1 on 96 x 64
// tiles 29.6 us against 18.8 on big tiles, QKV 20.9 against 12.3, while fc2 still wins with 25.4 against 31.9).  3840 lies between
// the estimates of t = 74 (3776), the last iteration that gains, and of t = 73.  The estimate runs a quarter or more above the live rows of that loop (duplicates among
// the revealed frames: 3520 estimated, about 2794 live at t = 75), so in live rows the crossover lies near 3000: below it an
// iteration is the latency of its launches, which one flight of whole-K panels cuts; above it 64-column tiles re-read the weight
// panel once per 32 .. 96 rows and lose to the 192-row tiles.  A bound on the low side of the flat stretch also costs a caller whose
// canvas holds more distinct ids than a reverse process would (further rounds in every launch) the least.  (A compile-time constant so
// that A/B builds can move it; it is no tuning field.)
#ifndef D3PM_LIVE_LATENCY_ROWS
#define D3PM_LIVE_LATENCY_ROWS 3840
#endif
int live_latency_rows() { return D3PM_LIVE_LATENCY_ROWS; }

// The rows of the self-attention's K | V pool, and the largest per-utterance estimate that takes it (a compile-time constant for the same
// reason).  The gathered walk costs 20.6 us per launch (sd 0.25) from 2 to about 120 rows per utterance -- one workgroup alone on
// its CU waits out the L2 round trip of every 32-key block -- so the bound is not a crossover but the LDS a pool row costs: 256 bytes,
// 83 KiB in all at 128 rows with the 768-key index, one workgroup per CU, which is what these iterations launch anyway.  Measurements:
// profiles/round25_few_rows_ab_interleaved.txt.
#ifndef D3PM_ATTN_POOL_ROWS
#define D3PM_ATTN_POOL_ROWS 128
#endif
int attn_pool_rows() { return D3PM_ATTN_POOL_ROWS; }

// ---- d3pm_tuning.ln_fold (include/d3pm_hip.h): 0 the LayerNorm launches, 1 everything (default), 2 the fold alone, 3 fold + table,
// 4 fold + table + deduplication without the latency list.  The only place that reads the codes.
FoldFeatures fold_features(const d3pm_tuning& tn) {
  FoldFeatures f;
  f.fold = tn.ln_fold != 0;
  f.table = tn.ln_fold != 2;
  f.dedup = tn.ln_fold == 1 || tn.ln_fold == 4;
  f.latency = tn.ln_fold == 1;
  return f;
}

// ---- attention ----
namespace {

// what every MFMA attention kernel asks for: 16-bit, head width 64, 16-byte rows and operands (16-byte output stores)
bool attn_operands_ok(int dtype, const AttnArgs& a) {
  if (!is16(dtype) || a.hd != HD || a.S < 1 || a.Tq < 1) return false;
  if (a.ldq % 8 || a.ldkv % 8 || a.ldo % 8) return false;
  if (a.Q2 && !(a.S2 >= 1 && al16(a.Q2) && al16(a.K2) && al16(a.V2) && al16(a.O2))) return false;
  return al16(a.Q) && al16(a.K) && al16(a.V) && al16(a.O);
}

}  // namespace

AttnPlan plan_attention(int dtype, const AttnArgs& a, bool force_generic) {
  AttnPlan p;
  if (force_generic || !attn_operands_ok(dtype, a)) return p;
  const d3pm_tuning& tn = tune_of(a.tune);
  // ---- the tuning fields' integer codes, translated here and nowhere else ----
  // attn_query_groups: 0 auto, 1 / 2 that many 16-query groups per wave of the tile-by-tile kernel (and never the 32 x 32 x 16 one),
  // 4 the key-split kernel, 32 always the 32 x 32 x 16 self-attention, 33 the same with the plain walk (A/B against the pipelined one)
  const int q = tn.attn_query_groups;
  const bool qg_auto = q == 0, force32 = q == 32 || q == 33, plain_walk32 = q == 33, want_split = q == 4;
  const int forced_qg = (q == 1 || q == 2) ? q : 0;
  // attn_pair_sequential: 0 never, 1 auto (when the paired grid still has >= 2 workgroups per CU), 2 always
  const bool seq_auto = tn.attn_pair_sequential == 1, seq_always = tn.attn_pair_sequential == 2;
  // attn_cross_resident: the cross pair with every K / V tile resident in LDS: 0 never, 1 auto, 2 always, 3 always with one query
  // block per workgroup (the first form), 4 always on the 16 x 16 x 32 instruction (attn_cross_hd64, bit-identical to the
  // tile-by-tile kernel), 5 always on the 32 x 32 x 16 one
  const int r = tn.attn_cross_resident;
  const bool resident_auto = r == 1, resident_always = r >= 2, one_block_per_wg = r == 3, resident16 = r == 4;
  const long long batch = logical_batch(tn, a.B);
  p.masked = a.key_len != nullptr || a.key_len2 != nullptr;

  // The 32 x 32 x 16 kernel of d3pm_mfma_attn32.hip wherever it applies (whole 128-query blocks and 64-key tiles of a single
  // problem: the self-attention of a DiT block; with key lengths S is the padded count, the tiles are staged whole) once its grid has
  // two workgroups per CU (measured: 55.3 vs 65.3 us at 32 utterances x 768 frames, 19.5 vs 20.3 at 32 x 384, 28.8 vs 30.8 at
  // 16 x 768; tests/ab_attn32.py); below that the 64-query workgroups of the tile-by-tile kernel finish sooner.
  // Key lengths: the masked instantiations on an explicit 32 / 33, or where the denoiser plan asks for the unmasked choice
  // (AttnArgs::masked_keeps_schedule); any other masked call keeps the tile-by-tile kernel, as it always has (deliberate: the stock
  // NAR stage keeps its bits).
  const bool auto32 = qg_auto && static_cast<long long>(a.Tq / 128) * a.H * batch >= 2 * kCUs && (a.key_len == nullptr || a.masked_keeps_schedule);
  if ((force32 || auto32) && a.Q2 == nullptr && a.Tq >= 128 && a.Tq % 128 == 0 && a.S >= BKV && a.S % BKV == 0) {
    p.kernel = plain_walk32 ? ATTN_32 : ATTN_32P;
    p.masked = a.key_len != nullptr;
    p.n_qblocks = a.Tq / 128;
    p.grid = static_cast<unsigned>(p.n_qblocks * a.H * a.B);
    if (a.key_row && !plain_walk32) p.lds = static_cast<size_t>(a.S) * 4;      // the staged key index behind the static tiles
    // Few distinct rows per utterance (AttnArgs::seg_est): one workgroup per CU, which nothing covers while it waits for the staged
    // halves of each 32-key block, so the utterance's K | V rows of the head go to LDS once and the walk stages from there.  The grid
    // covers the estimated query blocks; a longer segment is walked all the same (stride), one beyond the pool through key_row.
    const bool pool_named = a.pool_rows > 0 && a.qblocks_grid > 0;
    if (a.key_row && a.seg_len && a.seg_key && p.kernel == ATTN_32P && (pool_named || (a.seg_est > 0 && a.seg_est <= attn_pool_rows()))) {
      const int rows = pool_named ? a.pool_rows : attn_pool_rows(), qblocks = pool_named ? a.qblocks_grid : (a.seg_est + 127) / 128;
      const size_t lds = p.lds + 2 * static_cast<size_t>(rows) * ROWB;
      if (3 * 2 * TILE + lds <= kAttnPoolLdsBytes && qblocks <= p.n_qblocks) {
        p.kernel = ATTN_32P_POOL;
        p.pool_rows = rows; p.n_qblocks = qblocks; p.lds = lds;
        p.grid = static_cast<unsigned>(qblocks * a.H * a.B);
      }
    }
    return p;
  }
  // The resident cross pair (<= 64 text keys, <= 256 prompt keys; key lengths do not change the choice: S / S2 are the padded
  // counts, which size the LDS image).  Auto = when its grid (256 queries per workgroup) has at least one workgroup per CU: at one
  // utterance it is 24 workgroups of eight waves and the tile-by-tile kernel's 192 small ones finish sooner (p50 latency
  // 46.7 -> 42.2 ms, profiles/round2_d_latency_ab.txt)
  const long long cross_wgs = static_cast<long long>((a.Tq + 255) / 256) * a.H * batch;
  if ((resident_always || (resident_auto && cross_wgs >= kCUs)) && a.Q2 != nullptr && a.S <= BKV && a.S2 <= 4 * BKV) {
    p.n_qblocks = (a.Tq + 255) / 256;
    p.n_qsplit = (kCUs + a.H * a.B - 1) / (a.H * a.B);            // workgroups per (utterance, head): enough to cover the CUs
    p.n_qsplit = p.n_qsplit < 1 ? 1 : p.n_qsplit > p.n_qblocks ? p.n_qblocks : p.n_qsplit;
    if (one_block_per_wg) p.n_qsplit = p.n_qblocks;
    // the same residency on the 32 x 32 x 16 instruction with the software-pipelined block of d3pm_mfma_attn32.hip is the shipped
    // form (34.9 vs 35.8 us per pair in the microbenchmark, 43.1 vs 44.1 us per attention launch in the loop, tests/ab_cross32.py,
    // profiles/round3_r_ab_cross32.txt; it takes over at the batch size where the self-attention changes instruction shape too):
    // every code but 4 takes it when resident is chosen (deliberate).  (Its S / S2 / Q2 conditions are the ones just tested.)
    p.kernel = resident16 ? ATTN_CROSS : ATTN_32_CROSS;
    p.grid = static_cast<unsigned>(p.n_qsplit * a.H * a.B);
    p.lds = static_cast<size_t>(1 + (a.S2 + BKV - 1) / BKV) * 2 * TILE;
    return p;
  }
  // Opt-in only (attn_query_groups = 4, deliberate): the key-split kernel of d3pm_mfma_attn_lat.hip -- four waves share 32 queries and
  // take every fourth key tile; one problem or a pair, no key lengths.  Measured at one utterance 0.8 ms of 38.8 faster (p50), at two
  // utterances 2 ms slower (tests/ab_latency.py, profiles/round3_o_ab_latency.txt): the launch is bound by the K / V bytes each
  // workgroup streams through its CU (196 KB per (head, query group) at 768 keys), not by the length of the tile chain, so it is not
  // an automatic choice -- one utterance keeps the schedule, and therefore the bits, of the batches up to ten.
  if (want_split && !p.masked) {
    p.kernel = ATTN_SPLIT;
    p.n_qblocks = (a.Tq + 31) / 32;
    p.n_first = p.n_qblocks * a.H * a.B;
    p.grid = static_cast<unsigned>(p.n_first) * (a.Q2 ? 2 : 1);
    return p;
  }
  // Tile by tile.  Two 16-query groups per wave (each K / V fragment read from LDS feeds two MFMAs; 63.8 vs 65.8 us on the
  // 768 x 768 x 256-head self-attention, 27.7 vs 30.1 us on the 225-key prompt attention) once that still leaves >= 4 workgroups per
  // CU, one group otherwise (a single utterance is 48 workgroups of two groups: latency regime).
  const long long wgs2 = static_cast<long long>((a.Tq + 127) / 128) * a.H * a.B * (a.Q2 ? 2 : 1);
  p.kernel = ATTN_TILES;
  p.qg = forced_qg == 0 ? (wgs2 >= 4 * kCUs ? 2 : 1) : forced_qg;
  const int per_block = 64 * p.qg;
  p.n_qblocks = (a.Tq + per_block - 1) / per_block;
  const int n_blocks1 = p.n_qblocks * a.H * a.B;
  p.pair_seq = a.Q2 != nullptr && (seq_always || (seq_auto && n_blocks1 >= 2 * kCUs));
  p.n_first = p.pair_seq ? -1 : n_blocks1;
  p.grid = static_cast<unsigned>(n_blocks1) * ((a.Q2 && !p.pair_seq) ? 2 : 1);
  return p;
}

}  // namespace d3pm
