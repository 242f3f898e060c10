// d3pm_mfma_gemm_lat.hip -- latency GEMM for one or two utterances (M <= 1536 rows) and for the iterations of the deduplicated loop
// that have as few live rows (LinearArgs::m_live / m_est): 64 x 64 tiles, whole-K panels.
//
//   Y[M][N] = epilogue(X[M][K] . W[N][K]^T + bias)      same contract and epilogue as d3pm_mfma_gemm.hip
//
// replaces the nn.Linear / MultiheadAttention projections of DiTBlock.forward
// (/root/reference/vall_e/vall_e/ar_discrete.py:132,138,142,159,776) when ONE utterance is sampled (the p50-latency
// half of the BASELINE.json metric).  At M = 768 every 128 x 128 launch costs ~10 us whatever its size
// (profiles/round1_i_microbench.txt): 24 .. 72 workgroups on 256 CUs, each walking its eight k-steps one DMA round
// trip after the other.  The time is latency, so this kernel removes the chain instead of shortening its links:
//   * 64 x 64 output tiles: 96 .. 384 workgroups for the block's projections at M = 768;
//   * the operand panels of a tile for 256 k (X [64][256] + W [64][256] = 64 KiB) fit one LDS buffer, and there are two:
//     for K = 512 EVERY DMA piece of the tile is issued before the first wait (32 per wave, all in flight together),
//     so the kernel pays one memory round trip, not eight; longer K (fc2: 2048) streams 256-k rounds through the
//     two buffers;
//   * within a round the four k-steps run back to back, no barriers (the whole round has landed);
//   * same swizzled 128-byte-row LDS image per 64-k sub-tile, same D = W_frag . X_frag^T orientation, same k order
//     and the same epilogue code as the other schedules: bit-identical results.
//   * a LayerNorm prologue (the tile's 64 whole rows normalised in LDS before the MFMAs, for the projections fed by a LayerNorm)
//     was built, measured and not shipped: 78 vs 53 ms p50 against the folded LayerNorm (source up to commit d54b189).
//   * two products through one weight panel (DUAL, K = d_model = 512, 32 x 64 tiles): the text and prompt cross-attention outputs
//     both go through cross_attn.out_proj (ar_discrete.py:138,142).  The tile's W panel is in LDS for the whole kernel anyway, so
//     the second operand's panel (X2, 32 KiB) rides in beside it and a second pass of the same k-steps gives
//     x' = rn(rn(R1 + rn(X W^T + b)) + rn(X2 W^T + b)) -- the R1 + R2 epilogue of the two-launch form with R2 taken from
//     registers: same bits, one launch (and one round trip of the intermediate through HBM) less per DiT block.
#include "d3pm_kernels.h"
#include "d3pm_mfma_tile.h"

namespace d3pm {
namespace {

// Tile geometries (TM x TN, four waves as 2 x 2): 64 x 64 is the base; 96 x 64 turns the 288 / 384 tiles of the qkv / fc1
// projections of one utterance (two rounds over 256 CUs at one workgroup per CU) into 192 / 256 (one round, one DMA flight);
// 32 x 64 gives the N = 512 projections (out-proj, fc2: 96 tiles of 64 x 64) 192 workgroups with half the X panel each.
template <int TM, int TN> struct LatGeom {
  static constexpr int XSUB = TM * ROW_BYTES, WSUB = TN * ROW_BYTES;     // one [rows][64 k] sub-tile of each operand
  static constexpr int XOPER = (KC / BK) * XSUB, WOPER = (KC / BK) * WSUB;
  static constexpr int BUF = XOPER + WOPER;                              // X + W of a round
};

__device__ __forceinline__ int xcd_remap_lat(int bid, int nblocks) {
  const int q = nblocks >> 3, r = nblocks & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// one output tile (tile index `bid`: row tile bid / n_tiles, column tile bid % n_tiles) by the whole workgroup
template <typename T, int EPI, int TM, int TN, bool DUAL>
__device__ __forceinline__ void panel64_tile(const T* __restrict__ X, int ldx, const T* __restrict__ W, const T* __restrict__ bias, T* Y,
                                             int ldy, const T* R1, const T* R2, int ldr, const uint8_t* __restrict__ row_mask,
                                             int mask_period, int M, int N, int K, int n_tiles, const EpiFold& ef,
                                             const T* __restrict__ X2, int bid) {
  using G = LatGeom<TM, TN>;
  static_assert(!DUAL || ((EPI & ~EPI_STATS) == EPI_R1 && TN == 64), "two products: whole tiles, K = 2 rounds, x' = (R1 + h) + y2");
  static_assert(TM % 32 == 0 && TN % 64 == 0, "four waves as 2 x 2, column blocks regrouped in pairs");
  constexpr int XP = TM / 32, WP = TN / 32;       // DMA pieces (8 rows) per wave and sub-tile = MFMA row / column blocks per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = (bid / n_tiles) * TM, n0 = (bid % n_tiles) * TN;
  const uint32_t lds_base = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)smem));
  // DMA piece (sub-tile s, rows 8j .. 8j+7): a wave takes the pieces j = wave + 4 i of every sub-tile of both operands
  // (swizzle key (row >> 1) & 7: one per-lane offset per piece)
  const int lrow = lane >> 3;
  const T* gx[XP];
  const T* gw[WP];
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int row = 8 * (wave + 4 * i) + lrow;
    int mr = m0 + row;
    mr = mr < M ? mr : M - 1;                // ragged edges: clamped loads, predicated stores
    gx[i] = X + static_cast<size_t>(mr) * ldx + ((lane & 7) ^ ((row >> 1) & 7)) * 8;
  }
#pragma unroll
  for (int i = 0; i < WP; ++i) {
    const int row = 8 * (wave + 4 * i) + lrow;
    int nr = n0 + row;
    nr = nr < N ? nr : N - 1;
    gw[i] = W + static_cast<size_t>(nr) * K + ((lane & 7) ^ ((row >> 1) & 7)) * 8;
  }
  // the epilogue's operands (bias, residuals, frame mask) are requested FIRST: they are older than every DMA piece, so the
  // counted waits below cover them, and they have landed long before the last MFMA instead of starting a new round trip there
  EpiPre<T, WP, XP> pre;
  if constexpr (!DUAL) epilogue_prefetch<T, EPI, WP, XP>(pre, bias, R1, R2, ldr, row_mask, mask_period, M, N, m0 + wm * (TM / 2), n0 + wn * (TN / 2), lane, &ef);
  [[maybe_unused]] Pack8<T> dual_r1;
  [[maybe_unused]] EpiPre<T, WP, XP> dual_pre;
  if constexpr (DUAL) {
    epilogue_prefetch<T, 0, WP, XP>(dual_pre, bias, nullptr, nullptr, ldr, nullptr, 1, M, N, m0 + wm * (TM / 2), n0 + wn * (TN / 2), lane);
    dual_r1 = *reinterpret_cast<const Pack8<T>*>(R1 + static_cast<size_t>(m0 + wm * (TM / 2) + (lane & 15)) * ldr + n0 + wn * (TN / 2) + epilogue_nq(lane));
  }
  constexpr int PIECES = (KC / BK) * (XP + WP);       // per wave and round
  constexpr int PIECES2 = DUAL ? 2 * (KC / BK) * XP : 0;   // the second operand's panel (both rounds), issued last
  auto issue_round = [&](int r, int buf) {
    const uint32_t base = lds_base + buf * G::BUF;
#pragma unroll
    for (int s = 0; s < KC / BK; ++s) {
#pragma unroll
      for (int i = 0; i < XP; ++i) glds16_asm(gx[i] + r * KC + s * BK, base + s * G::XSUB + (wave + 4 * i) * 1024);
#pragma unroll
      for (int i = 0; i < WP; ++i) glds16_asm(gw[i] + r * KC + s * BK, base + G::XOPER + s * G::WSUB + (wave + 4 * i) * 1024);
    }
  };
  floatx4 acc[WP][XP];
#pragma unroll
  for (int a = 0; a < WP; ++a)
#pragma unroll
    for (int b = 0; b < XP; ++b) acc[a][b] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, fch = lane >> 4;
  const int rounds = K / KC;                 // K is a multiple of 256 (launcher)
  issue_round(0, 0);
  if (rounds > 1) issue_round(1, 1);
  if constexpr (DUAL) {                      // K = 2 rounds (launcher): X2's whole-K panel behind the two buffers
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int s = 0; s < KC / BK; ++s)
#pragma unroll
        for (int i = 0; i < XP; ++i) {
          const int row = 8 * (wave + 4 * i) + lrow;       // whole tiles (launcher): no clamp
          glds16_asm(X2 + static_cast<size_t>(m0 + row) * ldx + ((lane & 7) ^ ((row >> 1) & 7)) * 8 + r * KC + s * BK,
                     lds_base + 2 * G::BUF + r * G::XOPER + s * G::XSUB + (wave + 4 * i) * 1024);
        }
  }
  // the four k-steps of one round: X sub-tiles at bx, W sub-tiles at bw
  auto round_product = [&](const char* bx, const char* bw) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < KC / BK; ++s)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        uint4 fx[XP], fw[WP];
#pragma unroll
        for (int q = 0; q < XP; ++q) fx[q] = *reinterpret_cast<const uint4*>(bx + s * G::XSUB + lds_off(wm * (TM / 2) + q * 16 + frow, ks * 4 + fch));
#pragma unroll
        for (int q = 0; q < WP; ++q) fw[q] = *reinterpret_cast<const uint4*>(bw + s * G::WSUB + lds_off(wn * (TN / 2) + q * 16 + frow, ks * 4 + fch));
#pragma unroll
        for (int nt = 0; nt < WP; ++nt)
#pragma unroll
          for (int mt = 0; mt < XP; ++mt) acc[nt][mt] = mma<T>(fw[nt], fx[mt], acc[nt][mt]);
      }
  };
  for (int r = 0; r < rounds; ++r) {
    const int buf = r & 1;
    if (r + 1 < rounds) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES + PIECES2) : "memory");   // the next round's pieces may stay in flight
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES2) : "memory");
    __builtin_amdgcn_s_barrier();            // every wave's pieces of round r have landed
    __builtin_amdgcn_sched_barrier(0);
    const char* bx = smem + buf * G::BUF;
    round_product(bx, bx + G::XOPER);
    __builtin_amdgcn_sched_barrier(0);
    if (r + 2 < rounds) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();          // every wave has finished reading this buffer
      issue_round(r + 2, buf);
    }
  }
  if constexpr (DUAL) {
    // h = rn(X W^T + b) packed in registers, then the second product over the same W panel (both rounds are still in LDS)
    static_assert(XP == 1 && WP == 2, "32 x 64 tiles: one 16-byte group per lane");
    uintx4 h1p[1], y2p[1];
    epilogue_store<T, 0, WP, XP, true, true, false, true>(acc, bias, Y, ldy, nullptr, nullptr, ldr, nullptr, 1, M, N, m0 + wm * (TM / 2), n0 + wn * (TN / 2), lane, h1p, &dual_pre);
#pragma unroll
    for (int a = 0; a < WP; ++a)
#pragma unroll
      for (int b = 0; b < XP; ++b) acc[a][b] = floatx4{0.f, 0.f, 0.f, 0.f};
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();            // every wave's X2 pieces have landed
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < 2; ++r) round_product(smem + 2 * G::BUF + r * G::XOPER, smem + r * G::BUF + G::XOPER);
    __builtin_amdgcn_sched_barrier(0);
    epilogue_store<T, 0, WP, XP, true, true, false, true>(acc, bias, Y, ldy, nullptr, nullptr, ldr, nullptr, 1, M, N, m0 + wm * (TM / 2), n0 + wn * (TN / 2), lane, y2p, &dual_pre);
    // x' = rn(rn(R1 + h) + y2): the R1 + R2 epilogue of the two-launch form with R2 = h from registers
    const Pack8<T> r1 = dual_r1;
    const Pack8<T> hh = __builtin_bit_cast(Pack8<T>, h1p[0]), yy = __builtin_bit_cast(Pack8<T>, y2p[0]);
    Pack8<T> o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o.v[i] = static_cast<T>(rn<T>(static_cast<float>(r1.v[i]) + static_cast<float>(hh.v[i])) + static_cast<float>(yy.v[i]));
    *reinterpret_cast<Pack8<T>*>(Y + static_cast<size_t>(m0 + wm * (TM / 2) + (lane & 15)) * ldy + n0 + wn * (TN / 2) + epilogue_nq(lane)) = o;
    if constexpr ((EPI & EPI_STATS) != 0) {      // the moments of the new rows, in the order every epilogue uses (d3pm_mfma_tile.h: emit_stats)
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = static_cast<float>(o.v[i]);
      part_stats_store(v, ef.stats_out, static_cast<size_t>(m0 + wm * (TM / 2) + (lane & 15)), N, n0 + wn * (TN / 2), lane >> 4, true);
    }
    return;
  }
  epilogue_store<T, EPI, WP, XP, false, false, false, true>(acc, bias, Y, ldy, R1, R2, ldr, row_mask, mask_period, M, N, m0 + wm * (TM / 2),
                                                            n0 + wn * (TN / 2), lane, nullptr, &pre, &ef);
}

// Live row count from device memory (LinearArgs::m_live, or null): only the row tiles that hold a row below it run, never more than the
// capacity's (M sizes every operand; rows behind the count inside the last live tile are computed like any row).  The grid is the
// planner's ESTIMATE of the live tiles (LinearArgs::m_est; the capacity's without one), so a workgroup walks tile, tile + grid, ..:
// more live rows than estimated cost further rounds, never a row.  A workgroup without a tile leaves in front of its first barrier.
// The XCD ranges are those of the live total, as in the big-tile kernel.  Without a count the grid is the tile count and the walk
// is one tile long.
template <typename T, int EPI, int TM = 64, int TN = 64, bool DUAL = false>
__global__ __launch_bounds__(256, 1) void gemm_mfma_panel64(const T* __restrict__ X, int ldx, const T* __restrict__ W,
                                                            const T* __restrict__ bias, T* Y, int ldy, const T* R1,
                                                            const T* R2, int ldr, const uint8_t* __restrict__ row_mask,
                                                            int mask_period, int M, int N, int K, int n_tiles,
                                                            EpiFold ef, const T* __restrict__ X2 = nullptr,
                                                            const int* __restrict__ m_live = nullptr) {
  const int m_tiles = (M + TM - 1) / TM;
  const int live_tiles = (m_live ? max(min((*m_live + TM - 1) / TM, m_tiles), 0) : m_tiles) * n_tiles;
  const int step = static_cast<int>(gridDim.x);
  for (int vt = blockIdx.x; vt < live_tiles; vt += step) {      // block-uniform
    panel64_tile<T, EPI, TM, TN, DUAL>(X, ldx, W, bias, Y, ldy, R1, R2, ldr, row_mask, mask_period, M, N, K, n_tiles, ef, X2,
                                       xcd_remap_lat(vt, live_tiles));
    if (vt + step < live_tiles) {      // a further round: the panels are reused
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();      // every wave has read its last fragments and its stores have left
    }
  }
}

}  // namespace

// Which projections come here, with which of the three geometries: d3pm_plan.cpp (panel64_ok, panel64_geometry).
template <typename U, int E, int TM, int TN>
static int panel64_launch(const LinearArgs& a, const LinearPlan& p, hipStream_t s) {
  using G = LatGeom<TM, TN>;
  D3PM_LDS_ATTR((&gemm_mfma_panel64<U, E, TM, TN>), 2 * G::BUF);
  gemm_mfma_panel64<U, E, TM, TN><<<dim3(p.grid), dim3(256), p.lds, s>>>(
      static_cast<const U*>(a.X), a.ldx, static_cast<const U*>(a.W), static_cast<const U*>(a.bias), static_cast<U*>(a.Y), a.ldy,
      static_cast<const U*>(a.R1), static_cast<const U*>(a.R2), a.ldr, a.row_mask, a.mask_period, a.M, a.N, a.K, p.n_tiles,
      epi_fold_of(a), nullptr, a.m_live);
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

template <typename U, int E> static int panel64_geometry(const LinearArgs& a, const LinearPlan& p, hipStream_t s) {
  switch (p.geom) {
    case 1: return panel64_launch<U, E, 96, 64>(a, p, s);
    case 2: return panel64_launch<U, E, 32, 64>(a, p, s);
    default: return panel64_launch<U, E, 64, 64>(a, p, s);
  }
}

// x' = rn(rn(R1 + rn(X W^T + b)) + rn(X2 W^T + b)) in one launch (the two cross-attention out-projections of a DiT block at one or
// two utterances): whole 32 x 64 tiles, K = 512 (both operand panels and the weight panel resident: 128 KiB)
template <typename U, int E>
static int panel64_dual_launch(const LinearArgs& a, const void* X2, const LinearPlan& p, const EpiFold& ef, hipStream_t s) {
  using G = LatGeom<32, 64>;
  D3PM_LDS_ATTR((&gemm_mfma_panel64<U, E, 32, 64, true>), 2 * G::BUF + 2 * G::XOPER);
  gemm_mfma_panel64<U, E, 32, 64, true><<<dim3(p.grid), dim3(256), p.lds, s>>>(
      static_cast<const U*>(a.X), a.ldx, static_cast<const U*>(a.W), static_cast<const U*>(a.bias), static_cast<U*>(a.Y), a.ldy,
      static_cast<const U*>(a.R1), nullptr, a.ldr, nullptr, 1, a.M, a.N, a.K, p.n_tiles, ef, static_cast<const U*>(X2), a.m_live);
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

int panel64_dual(int dtype, const LinearArgs& a, const void* X2, const LinearPlan& p, hipStream_t s) {
  auto go = [&](auto* tag) -> int {
    using U = std::remove_pointer_t<decltype(tag)>;
    switch (p.epi) {      // kEpiPanel64Dual (d3pm_plan.cpp)
      case EPI_R1 | EPI_STATS: return panel64_dual_launch<U, EPI_R1 | EPI_STATS>(a, X2, p, epi_fold_of(a), s);
      case EPI_R1: return panel64_dual_launch<U, EPI_R1>(a, X2, p, EpiFold{}, s);
      default: break;      // no plan names another one (tests/test_launch_plan_api.py)
    }
    return D3PM_E_SHAPE;
  };
  return dtype == D3PM_F16 ? go(static_cast<f16*>(nullptr)) : go(static_cast<bf16*>(nullptr));
}

int panel64_linear(int dtype, const LinearArgs& a, const LinearPlan& p, hipStream_t s) {
  auto go = [&](auto* tag) -> int {
    using U = std::remove_pointer_t<decltype(tag)>;
    switch (p.epi) {      // kEpiPanel64 (d3pm_plan.cpp)
      case 0: return panel64_geometry<U, 0>(a, p, s);
      case EPI_GELU: return panel64_geometry<U, EPI_GELU>(a, p, s);
      case EPI_R1: return panel64_geometry<U, EPI_R1>(a, p, s);
      case EPI_R2: return panel64_geometry<U, EPI_R2>(a, p, s);
      case EPI_R1 | EPI_MASK: return panel64_geometry<U, EPI_R1 | EPI_MASK>(a, p, s);
      case EPI_LNF: return panel64_geometry<U, EPI_LNF>(a, p, s);
      case EPI_LNF | EPI_GELU: return panel64_geometry<U, EPI_LNF | EPI_GELU>(a, p, s);
      case EPI_R1 | EPI_STATS: return panel64_geometry<U, EPI_R1 | EPI_STATS>(a, p, s);
      case EPI_R2 | EPI_STATS: return panel64_geometry<U, EPI_R2 | EPI_STATS>(a, p, s);
      case EPI_R1 | EPI_MASK | EPI_STATS: return panel64_geometry<U, EPI_R1 | EPI_MASK | EPI_STATS>(a, p, s);
      default: break;      // no plan names another one (tests/test_launch_plan_api.py)
    }
    return D3PM_E_SHAPE;
  };
  return dtype == D3PM_F16 ? go(static_cast<f16*>(nullptr)) : go(static_cast<bf16*>(nullptr));
}

}  // namespace d3pm
