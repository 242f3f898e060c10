// d3pm_mfma_gemm_big.hip -- big-tile persistent MFMA GEMM for the DiT projections at throughput batch sizes.
//
//   Y[M][N] = epilogue(X[M][K] . W[N][K]^T + bias)      same contract and epilogue as d3pm_mfma_gemm.hip
//
// replaces the nn.Linear / MultiheadAttention projections of DiTBlock.forward
// (/root/reference/vall_e/vall_e/ar_discrete.py:132,138,142,159) when the batch is large enough to fill the chip.
//
// Why a second structure.  With K = d_model = 512 the 128 x 128 kernels of d3pm_mfma_gemm.hip move one byte from L2
// into LDS per 64 flop; the measured L2 -> LDS rate of a CU (~32 B/clk) then caps them at half the MFMA rate
// (profiles/round1_*: 577 .. 853 TFLOP/s by shape, 0.30 of peak over the loop).  The lever is bytes per flop:
//   * a wave owns a 96 x 64 sub-tile (6 x 4 MFMA tiles of 16 x 16, 96 accumulator registers); a workgroup is 2 x 2 of them (192 x 128,
//     77 flop per staged byte, TWO workgroups per CU: the default since round 3 -- in the sampler's loop two independent
//     workgroups hide cold operands and each other's epilogue better than one, big_tile in d3pm_plan.cpp) or eight (192 x 256 / 96 x 512,
//     110 / 81 flop per staged byte, one workgroup per CU);
//   * the tile shapes divide the bench workload exactly: M = 32 utterances x 768 canvas rows = 128 x 192 rows, N = 512 / 1024 /
//     1536 / 2048 = 4 / 8 / 12 / 16 x 128 columns, i.e. 512 / 1024 / 1536 / 2048 tiles = 1 / 2 / 3 / 4 whole rounds over the 512
//     resident workgroups -- the 128 x 128 / 256 x 256 grids left a quarter of the chip idle in the last round (DESIGN_HISTORY.md
//     section 3);
//   * two LDS stages of (TM + TN) x 128 B; the next k-step's 1-KiB DMA pieces (global_load_lds_dwordx4 from inline
//     asm, invisible to hipcc's wait counters) are issued one per four MFMAs inside the current k-step, so the
//     memory pipeline's issue back-pressure hides under the partner wave's MFMAs; one s_barrier per k-step with a
//     counted vmcnt; the stream of k-steps runs across tile boundaries (the next tile's first k-step is in flight
//     under the epilogue) and the epilogue's 16-byte stores stay in flight into the next tile;
//   * same swizzled 128-byte-row LDS image, same D = W_frag . X_frag^T orientation and the same epilogue code as the
//     128 x 128 kernels (d3pm_mfma_tile.h): the accumulation order over k is identical, results are bit-identical.
#include "d3pm_kernels.h"
#include "d3pm_mfma_tile.h"
#include "d3pm_mx.h"

namespace d3pm {
namespace {

// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N - 1>{})
template <class F, int... I> __device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F> __device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// one 16-byte fragment read whose completion is waited for by hand (lds_wait): hipcc would otherwise sink each read
// down to the instruction before its first use (it minimises registers), which exposes the LDS latency in every group
__device__ __forceinline__ void lds_read16(uintx4& dst, uint32_t addr, int off) {   // off: a constant after inlining
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off));
}
// wait until at most N of this wave's LDS reads are outstanding; the "+v" operands are the fragments this makes valid,
// so that no MFMA that consumes them can be scheduled above the wait
template <int N> __device__ __forceinline__ void lds_wait(uintx4& a) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(N)); }
template <int N> __device__ __forceinline__ void lds_wait(uintx4& a, uintx4& b, uintx4& c, uintx4& d, uintx4& e) {
  asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e) : "n"(N));
}
// DMA piece without the M0 save / restore of glds16_asm_s.  M0 is a reserved register that hipcc only writes right in
// front of its own M0-reading instructions (LDS-DMA builtins, s_movrel, GWS), and gemm_mfma_big contains none of those
// (checked in the .s: no m0 outside these statements), so the value left behind is never observed.
__device__ __forceinline__ void glds16_m0(const void* sbase, uint32_t voff, uint32_t lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

// The schedule is the hand-placed one (fragment reads from asm with counted lgkmcnt, one DMA piece per MFMA group).  Built, measured,
// not shipped (source up to commit d54b189, figures in DESIGN.md section 3): compiler-placed reads, deferred stores (a tile's 12 output
// stores issued inside the next tile's first k-steps) and every DMA piece of the next k-step in front of the first MFMA group.

// Row-panel fusion (FUSE != 0; 96 x 512 tiles, d_model = 512 only: a workgroup then owns whole rows of the residual stream):
//   bit 0  a SECOND product with the same weights runs through the same tile before the epilogue -- the text and prompt
//          cross-attention outputs both go through cross_attn.out_proj (ar_discrete.py:138,142): h = rn(X W^T + b) stays
//          packed in registers, then x' = rn(rn(R1 + h) + rn(X2 W^T + b)): one launch, no h round trip through HBM;
//   bit 1  LayerNorm of the finished rows (the NEXT op of the block, ar_discrete.py:131,136,153) in the epilogue: the row
//          moments are reduced in registers, across lanes and across the eight waves (LDS) in the exact order of
//          layernorm_vec (wave_sum_up), so the output is bit-identical to the stand-alone LayerNorm launch it replaces;
//   bit 2  a second LayerNorm of the same rows (norm2 | norm22);   bit 3  FiLM on the first (norm3, :145-156);
//   bit 5  (fp8 fast path) the LayerNorm outputs leave in the block-scaled fp8 format of d3pm_mx.hip instead of 16 bit: lny / lny2
//          are then code buffers [M][512] bytes and sx / sx2 their block scales [M][4][4]; the value that is quantised is the 16-bit
//          LayerNorm result bit for bit (the four lanes that own 32 consecutive columns of a row own one MX block).
template <typename T> struct RowPanelArgs {
  const T* X2; const T* lnw; const T* lnb; const T* lnw2; const T* lnb2; const T* film; T* lny; T* lny2; float eps;
  uint8_t* sx; uint8_t* sx2;
};
constexpr int FUSE_DUAL = 1, FUSE_LN = 2, FUSE_LN2 = 4, FUSE_FILM = 8, FUSE_MX = 32;

// MT: 16-row blocks per wave.  6 everywhere but on the short tiles of the deduplicated loop's producers (3 / 4 with 2 x 2 waves: 96 x 128
// and 128 x 128 tiles, d3pm_plan.cpp big_tile); whatever carries an MT below was a 6, or a 12 = 2 x 6, before them.
template <typename T, int EPI, int WM, int WN, int FUSE = 0, int MT = 6>
__global__ __launch_bounds__(WM * WN * 64, 2) void gemm_mfma_big(const T* __restrict__ X, int ldx, const T* __restrict__ W,
                                                        const T* __restrict__ bias, T* Y, int ldy, const T* R1,
                                                        const T* R2, int ldr, const uint8_t* __restrict__ row_mask,
                                                        int mask_period, int M, int N, int K, int n_tiles,
                                                        int tiles_total, RowPanelArgs<T> rp, EpiFold ef,
                                                        const int* __restrict__ m_live = nullptr) {
  constexpr int NW = WM * WN, WR = 16 * MT, TM = WR * WM, TN = 64 * WN;   // 8 waves: one workgroup per CU; 4 waves: two
  static_assert(MT == 6 || ((MT == 3 || MT == 4) && WM == 2 && WN == 2 && (FUSE == 0 || FUSE == 1)), "short tiles: 2 x 2 waves, plain or dual");
  // live row count from device memory (LinearArgs::m_live): the tiles that hold a row below it, walked over the XCD ranges of THAT total
  // (never more than the plan's: M is the capacity of every operand)
  if (m_live) tiles_total = min(((*m_live + TM - 1) / TM) * n_tiles, tiles_total);
  constexpr int XD = TM / 8, WD = TN / 8;              // 1-KiB DMA pieces (8 rows x 128 B) per k-step and operand
  constexpr int XPW = (XD + NW - 1) / NW, WPW = WD / NW;   // pieces per wave
  constexpr int NDMA = XPW + WPW;                      // 7 (192 x 256), 10 (96 x 512: waves 4..7 repeat an X piece), 10 (192 x 128)
  static_assert(NW % 2 == 0 && WD % NW == 0 && (XD % NW == 0 || (XD % NW) % 2 == 0), "piece distribution keeps the parity of the wave");
  constexpr int X_BYTES = TM * ROW_BYTES, STAGE = (TM + TN) * ROW_BYTES;
  static_assert(NDMA <= 4 * MT, "one DMA piece per group of four MFMAs (MT = 3: seven pieces for six groups, the first group issues two)");
  // EPI_LNF (K = 512: the launcher): the row moments a lane needs for its six row blocks are 24 x 8 bytes per tile -- 48 KB per
  // workgroup tile beside its 320 KB of operands, through the same CU <-> L2 path (EPI_QUADS: 6 x 8 bytes, 12 KB) -- and a round trip
  // the epilogue would start with.  Loaded where the epilogue needs them they cost qkv 36.7 -> 45.1 us and fc1 69.7 -> 84.8 us in the loop; requested at
  // the top of the tile they stalled the second k-step instead (every k-step waits with vmcnt(0), vector-memory operations
  // retire in order).  The one place such a load can hide is ACROSS an epilogue: the moments of the NEXT row panel are requested
  // at the start of the epilogue of the last tile of this one, from inline asm (NMOM = 24 loads, 6 with quads) behind the tile's own
  // per-column vectors (8 asm loads), the epilogue waits with vmcnt(NMOM) -- its vectors have landed, the moments may stay in
  // flight -- and the next tile's first k-step, which waits for everything older than the 12 output stores anyway, finds them
  // landed; they are reduced to the two scalars per row right behind that k-step.
  constexpr bool kLnfPre = (EPI & EPI_LNF) != 0;
  constexpr bool kQuads = (EPI & EPI_QUADS) != 0;
  static_assert(!kQuads || ((EPI & (EPI_LNF | EPI_STATS)) != 0 && WN % 2 == 0), "a quad = the 128 columns of two neighbouring waves");
  constexpr int MPR = kQuads ? 1 : 4;                   // moment loads per row block and lane: one quad, or parts 4 g .. 4 g + 3
  constexpr int NMOM = MT * MPR;                        // the moment loads of a tile: what the epilogue's counted wait leaves in flight
  static_assert(NMOM == (kQuads ? MT : 4 * MT) && NMOM < 64, "vmcnt operand");
  constexpr bool kDual = (FUSE & FUSE_DUAL) != 0, kLn = (FUSE & FUSE_LN) != 0, kLn2 = (FUSE & FUSE_LN2) != 0, kFilm = (FUSE & FUSE_FILM) != 0;
  constexpr bool kMx = (FUSE & FUSE_MX) != 0;
  static_assert(!kMx || kLn, "the MX output is the LayerNorm output");
  static_assert(FUSE == 0 || FUSE == FUSE_DUAL || (WM == 1 && WN == 8), "row-panel fusion: 96 x 512 tiles");
  static_assert((EPI & (EPI_LNF | EPI_STATS)) == 0 || FUSE == 0 || (FUSE == FUSE_DUAL && (EPI & EPI_LNF) == 0),
                "the folded-LayerNorm epilogues ride in the plain launches (and the row moments in the dual out-projection)");
  static_assert(!kLn2 || kLn, "the second LayerNorm shares the moments of the first");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  // XCD x = blockIdx & 7 owns a contiguous range of tiles (the n-tiles of one X panel then share an L2)
  const int xcd = blockIdx.x & 7, per_xcd = gridDim.x >> 3;
  const int tq = tiles_total >> 3, tr = tiles_total & 7;
  const int lo = xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq, cnt = tq + (xcd < tr ? 1 : 0);
  int t = blockIdx.x >> 3;
  // Tile walk: workgroup slot s of an XCD takes tiles s, s + per_xcd, .. of the XCD's range, so the n-tiles of one row panel run at
  // the same time on neighbouring CUs and share the panel's X rows in L2 (fetched from the fabric once).  A walk over CONSECUTIVE
  // tiles (one workgroup = 3-4 n-tiles of one panel, its row scalars fetched once) was measured for the folded launches: +1.2 %
  // while the output rows still went through L2, nothing once they left as `sc1` stores (106.8 k vs 106.7 k tokens/s) -- and it
  // re-fetched each panel 2-3 times from the fabric (PMC 93.6 MB per launch against 49 / 30 algorithmic), so it is not kept.
  const int t_end = cnt, t_step = per_xcd;
  if (t >= t_end) return;                                            // block-uniform
  const uint32_t lds_base = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) char*)smem));
  // DMA piece j of an operand tile = rows 8j .. 8j+7; a wave takes pieces j = wave + NW p, so the swizzle key
  // (row >> 1) & 7 = (4 (j & 1) + (lane >> 4)) & 7 is the same for all of its pieces: one per-lane offset per operand
  const int lrow = lane >> 3, logical = (lane & 7) ^ ((4 * (wave & 1) + (lane >> 4)) & 7);
  const uint32_t ox = static_cast<uint32_t>(lrow * ldx + logical * 8) * 2u;
  const uint32_t ow = static_cast<uint32_t>(lrow * K + logical * 8) * 2u;
  auto dma = [&](int p, const T* px, const T* pw, uint32_t stage) __attribute__((always_inline)) {   // p: unrolled constant
    if (p < XPW) {
      int j = wave + NW * p;
      if (XD % NW != 0 && j >= XD) j = (XD / NW) * NW + wave % (XD % NW);   // same parity as `wave`: a harmless repeat
      glds16_m0(px + static_cast<size_t>(8 * j) * ldx, ox, stage + j * 1024);
    } else {
      const int j = wave + NW * (p - XPW);
      glds16_m0(pw + static_cast<size_t>(8 * j) * K, ow, stage + X_BYTES + j * 1024);
    }
  };
  // fragment addresses: row = base + 16 q + (lane & 15); the swizzle key (row >> 1) & 7 = (lane & 15) >> 1 because
  // every base is a multiple of 16
  const int frow = lane & 15, fch = lane >> 4, fkey = (frow >> 1) & 7;
  const int fo0 = frow * ROW_BYTES + ((fch ^ fkey) << 4), fo1 = frow * ROW_BYTES + (((4 + fch) ^ fkey) << 4);
  // PINS, not code: no instruction comes from fx_base / fw_base here, from `pend` below or from their uses in the k-step lambda.  hipcc's
  // early passes run before that lambda is inlined and see what it captures; with the operand bases and the twelve registers of the
  // retired deferred-store schedule captured, the instantiations keep the instruction streams they were measured with (all but two
  // unfolded bf16 GELU ones, which the epilogue's lost table arm moved) -- without them scalar code of every prologue moves
  // (profiles/round12_experiment_library_retired_same_code.txt).  Drop them only with a new measurement.
  const char* const fx_base = smem + wm * WR * ROW_BYTES;
  const char* const fw_base = smem + X_BYTES + wn * 64 * ROW_BYTES;

  const int nk = K / BK;                                             // even (checked by the launcher)
  int tile = lo + t;
  const T* sx = X + static_cast<size_t>((tile / n_tiles) * TM) * ldx;
  const T* sw = W + static_cast<size_t>((tile % n_tiles) * TN) * K;
#pragma unroll
  for (int p = 0; p < NDMA; ++p) dma(p, sx, sw, lds_base);          // first k-step of the first tile
  typedef float float2v __attribute__((ext_vector_type(2)));
  [[maybe_unused]] float2v lst[MT][MPR];                              // EPI_LNF: the moments of the tile about to start, in flight
  auto moments_request = [&](int mrow0) __attribute__((always_inline)) {
    // entries MPR g .. MPR g + MPR - 1 of row (lane & 15) of each of the six 16-row blocks: [row block][entry][row][2] (stats_index,
    // 16 parts or 4 quads per row; one entry of a row block = one 128-byte line), NMOM loads
    constexpr int P = 4 * MPR;
    const float* sp = ef.stats_in + stats_index(static_cast<size_t>(mrow0 + wm * WR + (lane & 15)), (lane >> 4) * MPR, P);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(lst[mt][0]) : "v"(sp + mt * P * 32) : "memory");
      if constexpr (MPR == 4) {
        asm volatile("global_load_dwordx2 %0, %1, off offset:128" : "=v"(lst[mt][MPR - 3]) : "v"(sp + mt * P * 32) : "memory");
        asm volatile("global_load_dwordx2 %0, %1, off offset:256" : "=v"(lst[mt][MPR - 2]) : "v"(sp + mt * P * 32) : "memory");
        asm volatile("global_load_dwordx2 %0, %1, off offset:384" : "=v"(lst[mt][MPR - 1]) : "v"(sp + mt * P * 32) : "memory");
      }
    }
  };
  if constexpr (kLnfPre) moments_request((tile / n_tiles) * TM);     // the first tile's: covered by the wait below
  [[maybe_unused]] RowScalars<MT> rows;
  [[maybe_unused]] bool fresh = true;                                // lst holds moments that have not been reduced yet
  // the first step of a tile waits with vmcnt(12): behind an epilogue the DMA pieces are older than its 12 stores; the very
  // first tile has no stores behind its pieces, so they are waited for here
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  uintx4 pend[12];                // pin (above)
#pragma unroll
  for (int j = 0; j < 12; ++j) pend[j] = uintx4{0u, 0u, 0u, 0u};
  T* pend_y = Y;
  bool pending = false;
  // EPI_STATS | EPI_QUADS: the quads of the tile's rows from the part moments z[mt * 2 + np] (part_stats_reduce) of this wave's 64
  // columns.  Waves 2 j and 2 j + 1 own the 128 columns of quad j: the even one adds its two parts from 0.f, hands that over through
  // stage 1 (its last reads were the k-step that has just ended; the next DMA into it is issued behind the next tile's first barrier,
  // after the odd wave has consumed the hand-over), the odd one adds its own two parts and stores the quad
  [[maybe_unused]] auto quads_out = [&](const float (&z)[2 * MT], int m0, int n0) __attribute__((always_inline)) {
    float* xch = reinterpret_cast<float*>(smem + STAGE) + (wm * (WN / 2) + (wn >> 1)) * MT * 64 + lane;
    static_assert(WM * (WN / 2) * MT * 64 * 4 <= STAGE, "hand-over fits in one stage");
    asm volatile("s_barrier" ::: "memory");             // every wave has retired its fragment reads of stage 1
    if ((wn & 1) == 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) xch[mt * 64] = (0.f + z[mt * 2]) + z[mt * 2 + 1];
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the hand-over is in LDS
    if ((wn & 1) != 0) {
      const int g = lane >> 4;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const float qv = (xch[mt * 64] + z[mt * 2]) + z[mt * 2 + 1];
        if (g < 2) ef.stats_out[stats_index(static_cast<size_t>(m0 + wm * WR + mt * 16 + (lane & 15)), (n0 + wn * 64) >> 7, N >> 7) + g] = qv;
      }
    }
  };
  for (;;) {
    floatx4 acc[4][MT];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < MT; ++b) acc[a][b] = floatx4{0.f, 0.f, 0.f, 0.f};
    const int m0 = (tile / n_tiles) * TM, n0 = (tile % n_tiles) * TN;
    [[maybe_unused]] EpiPre<T, 4, MT> pre;
    // what follows this tile (block-uniform); the last tile re-reads its own first k-step: valid memory, never used
    const int t_next = t + t_step;
    const bool more = t_next < t_end;
    const int tile_next = more ? lo + t_next : tile;
    const T* sx_next = X + static_cast<size_t>((tile_next / n_tiles) * TM) * ldx;
    const T* sw_next = W + static_cast<size_t>((tile_next % n_tiles) * TN) * K;

    // one k-step on stage S while the DMA pieces of the following k-step (px, pw) go to stage S ^ 1.  WAITN: what the wait at
    // the top may leave in flight (the previous tile's output stores, which are younger than this k-step's pieces)
    auto step = [&](auto S_, auto WAITN_, const T* px, const T* pw) __attribute__((always_inline)) {
      constexpr int S = decltype(S_)::value, WAITN = decltype(WAITN_)::value;
      [[maybe_unused]] const char* bx = fx_base + S * STAGE;      // pins (top of the kernel)
      [[maybe_unused]] const char* bw = fw_base + S * STAGE;
      const uint32_t nxt = lds_base + (S ^ 1) * STAGE;
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (WAITN > 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAITN) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();      // every wave's pieces of this k-step have landed; stage S ^ 1 is no longer read
      __builtin_amdgcn_sched_barrier(0);
      {
        // issue order of the 20 fragment reads of a k-step: W0..3 X0 X1 | g0: X2 | g1: X3 | g2: X4 W'0 | g3: X5 W'1 | g4: X6 W'2 |
        // g5: X7 W'3 | g6: X8 | g7: X9 | g8: X10 | g9: X11 (X six row blocks per k-half, W' = the second k-half's W fragments);
        // group g consumes X_g (and W at g = 0, W' at g = 6): the counts below are the reads younger than what it needs
        // MT = 4 (eight groups): W0..3 X0 X1 | g0: X2 W'0 | g1: X3 W'1 | g2: X4 W'2 | g3: X5 W'3 | g4: X6 | g5: X7.
        // MT = 3 (six groups):   W0..3 X0 X1 | g0: X2 W'0 W'1 | g1: X3 W'2 | g2: X4 W'3 | g3: X5: the same rule -- X two groups ahead
        // through a ring of three registers, W' spread over the groups of the first k-half -- with its own counts.
        const uint32_t ax0 = lds_base + S * STAGE + wm * WR * ROW_BYTES + fo0, ax1 = ax0 - fo0 + fo1;
        const uint32_t aw0 = lds_base + S * STAGE + X_BYTES + wn * 64 * ROW_BYTES + fo0, aw1 = aw0 - fo0 + fo1;
        uintx4 fw0[4], fw1[4], fx[3];
        static_for<4>([&](auto NT) { lds_read16(fw0[NT.value], aw0, NT.value * 16 * ROW_BYTES); });
        lds_read16(fx[0], ax0, 0);
        lds_read16(fx[1], ax0, 16 * ROW_BYTES);
        static_for<2 * MT>([&](auto G) {
          constexpr int g = G.value, ks = g / MT, mt = g % MT;
          if constexpr (g + 2 < 2 * MT) lds_read16(fx[(g + 2) % 3], (g + 2) / MT ? ax1 : ax0, ((g + 2) % MT) * 16 * ROW_BYTES);
          if constexpr (MT == 6) {
            if constexpr (ks == 0 && mt >= 2) lds_read16(fw1[mt - 2], aw1, (mt - 2) * 16 * ROW_BYTES);
          } else if constexpr (MT == 4) {
            if constexpr (ks == 0) lds_read16(fw1[mt], aw1, mt * 16 * ROW_BYTES);
          } else {
            if constexpr (g == 0) lds_read16(fw1[0], aw1, 0);
            if constexpr (ks == 0) lds_read16(fw1[mt + 1], aw1, (mt + 1) * 16 * ROW_BYTES);
          }
          if constexpr (g < NDMA) dma(g, px, pw, nxt);
          if constexpr (2 * MT + g < NDMA) dma(2 * MT + g, px, pw, nxt);
          constexpr int kWait6[12] = {2, 2, 3, 4, 5, 5, 1, 2, 2, 2, 1, 0}, kWait4[12] = {3, 4, 5, 5, 1, 2, 1, 0}, kWait3[12] = {4, 5, 6, 1, 1, 0};
          constexpr int kWait = MT == 6 ? kWait6[g] : MT == 4 ? kWait4[g] : kWait3[g];
          if constexpr (g == 0) lds_wait<kWait>(fw0[0], fw0[1], fw0[2], fw0[3], fx[0]);
          else if constexpr (g == MT) lds_wait<kWait>(fw1[0], fw1[1], fw1[2], fw1[3], fx[g % 3]);
          else lds_wait<kWait>(fx[g % 3]);
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) acc[nt][mt] = mma<T>(__builtin_bit_cast(uint4, ks ? fw1[nt] : fw0[nt]), __builtin_bit_cast(uint4, fx[g % 3]), acc[nt][mt]);
          if constexpr (WAITN < 0 && g < 0) { if (pending) *reinterpret_cast<uintx4*>(pend_y + ldy) = pend[g]; }      // pin: never instantiated
        });
      }
      __builtin_amdgcn_sched_barrier(0);
    };

    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    uintx4 h1p[kDual ? 2 * MT : 1];
    // the nk k-steps of one product: operand rows `ax`, weights `sw`; (nx, nw) = the first k-step of whatever follows
    auto run_k = [&](const T* ax, const T* nx, const T* nw, auto FIRSTW) __attribute__((always_inline)) {
      step(I0{}, FIRSTW, ax + BK, sw + BK);
      if constexpr (kLnfPre) {
        // the first k-step waited for everything older than the previous tile's stores: this tile's moments, requested in front of
        // those stores, have landed (the "+v" operands keep every use behind that wait)
        if (fresh)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
          for (int i = 0; i < MPR; ++i) asm volatile("" : "+v"(lst[mt][i]));
          float a = 0.f, q = 0.f;                        // fold_row_moments' order: a quad is these four adds done by the producer
#pragma unroll
          for (int i = 0; i < MPR; ++i) { a += lst[mt][i][0]; q += lst[mt][i][1]; }
          a = add_xor16(a); q = add_xor16(q);
          fold_row_scalars(add_xor32(a), add_xor32(q), 512, ef.eps, rows.ra[mt], rows.rc[mt]);
        }
      }
      step(I1{}, I0{}, ax + 2 * BK, sw + 2 * BK);
      for (int kt = 2; kt < nk; kt += 2) {                  // nk is even and >= 4
        step(I0{}, I0{}, ax + (kt + 1) * BK, sw + (kt + 1) * BK);
        const bool last = kt + 2 >= nk;
        step(I1{}, I0{}, last ? nx : ax + (kt + 2) * BK, last ? nw : sw + (kt + 2) * BK);
      }
    };
    if constexpr (kDual) {
      // two products through the same weights, one loop so that the k-step code exists once: phase 0 ends with its result
      // packed in registers (h1p), phase 1 runs into the common epilogue below
      const T* sx2 = rp.X2 + static_cast<size_t>(m0) * ldx;
      const T* ax = sx;
#pragma unroll 1
      for (int ph = 0; ph < 2; ++ph) {
        const bool mid = ph == 0;
        run_k(ax, mid ? sx2 : sx_next, mid ? sw : sw_next, std::integral_constant<int, 2 * MT>{});
        if (mid) {
          epilogue_store<T, 0, 4, MT, true, true>(acc, bias, Y, ldy, nullptr, nullptr, ldr, nullptr, 1, M, N, m0 + wm * WR, n0 + wn * 64, lane, h1p);
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < MT; ++b) acc[a][b] = floatx4{0.f, 0.f, 0.f, 0.f};
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // nothing but the bias loads follows these DMA pieces: wait for all
          ax = sx2;
        }
      }
    } else {
      run_k(sx, sx_next, sw_next, std::integral_constant<int, 2 * MT>{});
    }
    if constexpr (FUSE != 0) {
      uintx4 xp[2 * MT];
      if constexpr (kDual) {
        // x' = rn(rn(R1 + h) + rn(X2 W^T + b)): the R1 + R2 epilogue of the two-launch form with R2 = h taken from registers
        epilogue_store<T, 0, 4, MT, true, true>(acc, bias, Y, ldy, nullptr, nullptr, ldr, nullptr, 1, M, N, m0 + wm * WR, n0 + wn * 64, lane, xp);
        const T* r1row = R1 + static_cast<size_t>(m0 + wm * WR + (lane & 15)) * ldr + n0 + wn * 64 + epilogue_nq(lane);
        Pack8<T> r1p[2 * MT];
#pragma unroll
        for (int j = 0; j < 2 * MT; ++j) r1p[j] = *reinterpret_cast<const Pack8<T>*>(r1row + static_cast<size_t>((j / 2) * 16) * ldr + (j % 2) * 32);
#pragma unroll
        for (int j = 0; j < 2 * MT; ++j) {
          const Pack8<T> hh = __builtin_bit_cast(Pack8<T>, h1p[j]), yy = __builtin_bit_cast(Pack8<T>, xp[j]);
          Pack8<T> o;
#pragma unroll
          for (int i = 0; i < 8; ++i)
            o.v[i] = static_cast<T>(rn<T>(static_cast<float>(r1p[j].v[i]) + static_cast<float>(hh.v[i])) + static_cast<float>(yy.v[i]));
          xp[j] = __builtin_bit_cast(uintx4, o);
        }
      } else {
        epilogue_store<T, EPI, 4, MT, true, true>(acc, bias, Y, ldy, R1, R2, ldr, row_mask, mask_period, M, N, m0, n0 + wn * 64, lane, xp);
      }
      // ---- the finished rows: store x', then LayerNorm them in place (layernorm_vec's arithmetic, bit for bit)
      const int g = lane >> 4, nq = epilogue_nq(lane);
      T* yrow = Y + static_cast<size_t>(m0 + wm * WR + (lane & 15)) * ldy + n0 + wn * 64 + nq;
#pragma unroll
      for (int j = 0; j < 2 * MT; ++j) {
        T* yp = yrow + static_cast<size_t>((j / 2) * 16) * ldy + (j % 2) * 32;
        if constexpr (FUSE == FUSE_DUAL) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(yp), "v"(xp[j]) : "memory");   // as the plain epilogue (kNts)
        else *reinterpret_cast<uintx4*>(yp) = xp[j];
      }
      if constexpr ((EPI & EPI_STATS) != 0) {        // the row moments of the new rows for the folded LayerNorm that reads them next
        [[maybe_unused]] float z[2 * MT];
#pragma unroll
        for (int j = 0; j < 2 * MT; ++j) {
          const Pack8<T> p = __builtin_bit_cast(Pack8<T>, xp[j]);
          float v[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] = static_cast<float>(p.v[i]);
          if constexpr (kQuads) z[j] = part_stats_reduce(v);
          else part_stats_store(v, ef.stats_out, static_cast<size_t>(m0 + wm * WR + (j / 2) * 16 + (lane & 15)), N, n0 + wn * 64 + (j % 2) * 32, g, true);
        }
        if constexpr (kQuads) quads_out(z, m0, n0);
      }
      if constexpr (kLn) {
        static_assert(!kLn || MT == 6, "row-panel LayerNorm: 96 x 512 tiles");
        float* red = reinterpret_cast<float*>(smem + 2 * STAGE);              // [2][96 rows][8 waves] partial sums
        auto unpack = [&](int j, float (&v)[8]) __attribute__((always_inline)) {
          const Pack8<T> p = __builtin_bit_cast(Pack8<T>, xp[j]);
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] = static_cast<float>(p.v[i]);
        };
        // a row's 512 columns = 64 chunks of 8; this lane holds chunks c = 8 wave + 4 np + 2 (g & 1) + (g >> 1) of rows
        // (lane & 15) + 16 mt.  wave_sum_up's tree over the chunk index: bit 0 = lane ^ 32, bit 1 = lane ^ 16, bit 2 = np,
        // bits 3..5 = the wave (through LDS), each level adding the two halves exactly as the 64-lane butterfly does
        auto row_total = [&](float (&part)[6][2], int which, float (&tot)[6]) __attribute__((always_inline)) {
#pragma unroll
          for (int mt = 0; mt < 6; ++mt) {
            float a0 = part[mt][0], a1 = part[mt][1];
            a0 = add_xor32(a0); a1 = add_xor32(a1);         // v[l] + v[l ^ 32], then ^ 16 (d3pm_common.h: same bits as __shfl_xor)
            a0 = add_xor16(a0); a1 = add_xor16(a1);
            const float w8 = a0 + a1;
            if (g == 0) red[(which * 96 + mt * 16 + (lane & 15)) * 8 + wave] = w8;
          }
          __syncthreads();
#pragma unroll
          for (int mt = 0; mt < 6; ++mt) {
            const floatx4 lo4 = *reinterpret_cast<const floatx4*>(red + (which * 96 + mt * 16 + (lane & 15)) * 8);
            const floatx4 hi4 = *reinterpret_cast<const floatx4*>(red + (which * 96 + mt * 16 + (lane & 15)) * 8 + 4);
            tot[mt] = ((lo4[0] + lo4[1]) + (lo4[2] + lo4[3])) + ((hi4[0] + hi4[1]) + (hi4[2] + hi4[3]));
          }
        };
        float part[6][2], mean[6], rstd[6];
#pragma unroll
        for (int mt = 0; mt < 6; ++mt)
#pragma unroll
          for (int np = 0; np < 2; ++np) {
            float v[8], s1 = 0.f;
            unpack(mt * 2 + np, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) s1 += v[i];
            part[mt][np] = s1;
          }
        row_total(part, 0, mean);
#pragma unroll
        for (int mt = 0; mt < 6; ++mt) mean[mt] = mean[mt] / 512.0f;
#pragma unroll
        for (int mt = 0; mt < 6; ++mt)
#pragma unroll
          for (int np = 0; np < 2; ++np) {
            float v[8], q = 0.f;
            unpack(mt * 2 + np, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) { const float tt = v[i] - mean[mt]; q += tt * tt; }
            part[mt][np] = q;
          }
        row_total(part, 1, rstd);
#pragma unroll
        for (int mt = 0; mt < 6; ++mt) rstd[mt] = rsqrtf(rstd[mt] / 512.0f + rp.eps);
        if constexpr (kMx) {
          // the LayerNorm result(s) as MX rows: per row block both 32-column halves are finished, quantised and stored together
          Pack8<T> wv[2], bv[2], sc[2], sh[2], w2v[2], b2v[2];
#pragma unroll
          for (int np = 0; np < 2; ++np) {
            const int col = n0 + wn * 64 + np * 32 + nq;
            wv[np] = *reinterpret_cast<const Pack8<T>*>(rp.lnw + col); bv[np] = *reinterpret_cast<const Pack8<T>*>(rp.lnb + col);
            if constexpr (kFilm) { sc[np] = *reinterpret_cast<const Pack8<T>*>(rp.film + col); sh[np] = *reinterpret_cast<const Pack8<T>*>(rp.film + 512 + col); }
            if constexpr (kLn2) { w2v[np] = *reinterpret_cast<const Pack8<T>*>(rp.lnw2 + col); b2v[np] = *reinterpret_cast<const Pack8<T>*>(rp.lnb2 + col); }
          }
          uint8_t* const y8 = reinterpret_cast<uint8_t*>(rp.lny);
          uint8_t* const y8b = reinterpret_cast<uint8_t*>(rp.lny2);
          const int col0 = n0 + wn * 64, blk = (col0 >> 5) + (lane >> 4);          // the block whose scale byte lanes g = 0 / 1 write
#pragma unroll
          for (int mt = 0; mt < 6; ++mt) {
            uint2 cd[2], cd2[2];
            uint32_t sb[2], sb2[2];
#pragma unroll
            for (int np = 0; np < 2; ++np) {
              float v[8], o[8], o2[8];
              unpack(mt * 2 + np, v);
#pragma unroll
              for (int i = 0; i < 8; ++i) {
                const float nrm = (v[i] - mean[mt]) * rstd[mt];
                o[i] = rn<T>(nrm * static_cast<float>(wv[np].v[i]) + static_cast<float>(bv[np].v[i]));
                if constexpr (kFilm) {
                  const float gg = rn<T>(1.0f + static_cast<float>(sc[np].v[i]));
                  o[i] = rn<T>(rn<T>(o[i] * gg) + static_cast<float>(sh[np].v[i]));
                }
                if constexpr (kLn2) o2[i] = rn<T>(nrm * static_cast<float>(w2v[np].v[i]) + static_cast<float>(b2v[np].v[i]));
              }
              cd[np] = mx_block_quantise(o, sb[np]);
              if constexpr (kLn2) cd2[np] = mx_block_quantise(o2, sb2[np]);
            }
            const size_t row = static_cast<size_t>(m0 + mt * 16 + (lane & 15));
            mx_store_row64(cd[0], cd[1], y8 + row * 512 + col0, lane);
            if constexpr (kLn2) mx_store_row64(cd2[0], cd2[1], y8b + row * 512 + col0, lane);
            if (lane < 32) {
              rp.sx[row * 16 + (blk & 3) * 4 + (blk >> 2)] = static_cast<uint8_t>(lane < 16 ? sb[0] : sb[1]);
              if constexpr (kLn2) rp.sx2[row * 16 + (blk & 3) * 4 + (blk >> 2)] = static_cast<uint8_t>(lane < 16 ? sb2[0] : sb2[1]);
            }
          }
        } else {
#pragma unroll
        for (int np = 0; np < 2; ++np) {
          const int col = n0 + wn * 64 + np * 32 + nq;
          const Pack8<T> wv = *reinterpret_cast<const Pack8<T>*>(rp.lnw + col), bv = *reinterpret_cast<const Pack8<T>*>(rp.lnb + col);
          Pack8<T> sc, sh, w2v, b2v;
          if constexpr (kFilm) { sc = *reinterpret_cast<const Pack8<T>*>(rp.film + col); sh = *reinterpret_cast<const Pack8<T>*>(rp.film + 512 + col); }
          if constexpr (kLn2) { w2v = *reinterpret_cast<const Pack8<T>*>(rp.lnw2 + col); b2v = *reinterpret_cast<const Pack8<T>*>(rp.lnb2 + col); }
#pragma unroll
          for (int mt = 0; mt < 6; ++mt) {
            float v[8], nrm[8];
            unpack(mt * 2 + np, v);
            Pack8<T> o;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              nrm[i] = (v[i] - mean[mt]) * rstd[mt];
              o.v[i] = static_cast<T>(nrm[i] * static_cast<float>(wv.v[i]) + static_cast<float>(bv.v[i]));
            }
            if constexpr (kFilm) {
#pragma unroll
              for (int i = 0; i < 8; ++i) {
                const float gg = rn<T>(1.0f + static_cast<float>(sc.v[i]));
                o.v[i] = static_cast<T>(rn<T>(static_cast<float>(o.v[i]) * gg) + static_cast<float>(sh.v[i]));
              }
            }
            const size_t off = static_cast<size_t>(m0 + mt * 16 + (lane & 15)) * 512 + col;
            *reinterpret_cast<Pack8<T>*>(rp.lny + off) = o;
            if constexpr (kLn2) {
              Pack8<T> o2;
#pragma unroll
              for (int i = 0; i < 8; ++i) o2.v[i] = static_cast<T>(nrm[i] * static_cast<float>(w2v.v[i]) + static_cast<float>(b2v.v[i]));
              *reinterpret_cast<Pack8<T>*>(rp.lny2 + off) = o2;
            }
          }
        }
        }   // 16-bit LayerNorm outputs
      }
    } else {
      if constexpr (kLnfPre) {
        floatx4 bq[4], sq[4];
        const int ncol = n0 + wn * 64 + (lane >> 4) * 4;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(bq[nt]) : "v"(ef.b + ncol + nt * 16) : "memory");
          asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(sq[nt]) : "v"(ef.s + ncol + nt * 16) : "memory");
        }
        fresh = more && (tile_next / n_tiles) != (tile / n_tiles);      // the next tile reads other rows
        if (fresh) {
          moments_request((tile_next / n_tiles) * TM);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NMOM) : "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          asm volatile("" : "+v"(bq[nt]), "+v"(sq[nt]));
#pragma unroll
          for (int r = 0; r < 4; ++r) { pre.bv[nt][r] = bq[nt][r]; pre.sv[nt][r] = sq[nt][r]; }
        }
        epilogue_store<T, EPI, 4, MT, true, false, true, true>(acc, bias, Y, ldy, R1, R2, ldr, row_mask, mask_period, M, N, m0 + wm * WR,
                                                              n0 + wn * 64, lane, nullptr, &pre, &ef, &rows);
      } else {
        // output rows leave as `sc1` stores (kNts): they are not read again by this launch, and left in the XCD's L2 they displace the
        // operand panels the other tiles of the launch still stream (in the loop: 103.8 k -> 106.2 k tokens/s with the stand-alone
        // LayerNorms, 104.5 k -> 110.5 k with them folded; `nt`, which keeps the line in L2, was tried and lost)
        [[maybe_unused]] float z[2 * MT];
        epilogue_store<T, EPI, 4, MT, true, false, true>(acc, bias, Y, ldy, R1, R2, ldr, row_mask, mask_period, M, N, m0 + wm * WR,
                                                          n0 + wn * 64, lane, nullptr, &pre, &ef, nullptr, z);
        if constexpr (kQuads && (EPI & EPI_STATS) != 0) quads_out(z, m0, n0);
      }
    }
    if (!more) break;
    t = t_next;
    tile = tile_next;
    sx = sx_next;
    sw = sw_next;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the unused look-ahead pieces must not outlive the workgroup's LDS
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) % 16) == 0; }

}  // namespace

// Which shapes take which geometry (1 = 96 x 512, 1 x 8 waves; 2 = 192 x 256, 2 x 4; 3 = 192 x 128, 2 x 2, two workgroups per CU;
// 4 = 96 x 128 and 5 = 128 x 128, 2 x 2 waves of three / four row blocks), with which grid and LDS: d3pm_plan.cpp (big_tile, big_plan).
// The launchers below instantiate what a plan names.
template <typename U, int E, int WM, int WN, int MT = 6>
static int big_launch(const LinearArgs& a, const LinearPlan& p, hipStream_t s) {
  D3PM_LDS_ATTR((&gemm_mfma_big<U, E, WM, WN, 0, MT>), 160 * 1024);
  gemm_mfma_big<U, E, WM, WN, 0, MT><<<dim3(p.grid), dim3(WM * WN * 64), p.lds, s>>>(
      static_cast<const U*>(a.X), a.ldx, static_cast<const U*>(a.W), static_cast<const U*>(a.bias), static_cast<U*>(a.Y), a.ldy,
      static_cast<const U*>(a.R1), static_cast<const U*>(a.R2), a.ldr, a.row_mask, a.mask_period, a.M, a.N, a.K, p.n_tiles,
      p.tiles_total, RowPanelArgs<U>{}, epi_fold_of(a), a.m_live);
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

template <typename U, int E>
static int big_launch_geometry(const LinearArgs& a, const LinearPlan& p, hipStream_t s) {
  if (p.geom == 1) return big_launch<U, E, 1, 8>(a, p, s);
  if (p.geom == 2) return big_launch<U, E, 2, 4>(a, p, s);
  // the short tiles: the producers of the deduplicated loop and nothing else (d3pm_plan.cpp short_tile_epilogue)
  if constexpr (E == (EPI_R1 | EPI_STATS | EPI_QUADS) || E == (EPI_R1 | EPI_MASK | EPI_STATS | EPI_QUADS)) {
    if (p.geom == 4) return big_launch<U, E, 2, 2, 3>(a, p, s);
    if (p.geom == 5) return big_launch<U, E, 2, 2, 4>(a, p, s);
  }
  if (p.geom != 3) return D3PM_E_SHAPE;
  return big_launch<U, E, 2, 2>(a, p, s);
}

// Both cross-attention out-projections (ar_discrete.py:138,142: the SAME weights) in one launch of the ordinary big-tile geometry:
// a second product through the tile, the first result kept packed in 48 registers, x' = rn(rn(R1 + rn(X W^T + b)) + rn(X2 W^T + b))
// -- the bits of the two launches it replaces -- and, with stats_out, the row moments of x' for the folded norm3 of fc1.
template <typename U, int E, int WM, int WN, int MT = 6>
static int big_dual_launch(const LinearArgs& a, const void* X2, const LinearPlan& p, hipStream_t s) {
  D3PM_LDS_ATTR((&gemm_mfma_big<U, E, WM, WN, FUSE_DUAL, MT>), 160 * 1024);
  RowPanelArgs<U> rp{};
  rp.X2 = static_cast<const U*>(X2);
  gemm_mfma_big<U, E, WM, WN, FUSE_DUAL, MT><<<dim3(p.grid), dim3(WM * WN * 64), p.lds, s>>>(
      static_cast<const U*>(a.X), a.ldx, static_cast<const U*>(a.W), static_cast<const U*>(a.bias), static_cast<U*>(a.Y), a.ldy,
      static_cast<const U*>(a.R1), nullptr, a.ldr, nullptr, 1, a.M, a.N, a.K, p.n_tiles, p.tiles_total, rp, epi_fold_of(a), a.m_live);
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

int big_dual(int dtype, const LinearArgs& a, const void* X2, const LinearPlan& p, hipStream_t s) {
  auto go = [&](auto* tag) -> int {
    using U = std::remove_pointer_t<decltype(tag)>;
    if (p.geom < 2 || p.geom > 5 || (p.geom > 3 && p.epi != (EPI_R2 | EPI_STATS | EPI_QUADS))) return D3PM_E_SHAPE;
    switch (p.epi) {      // kEpiBigDual (d3pm_plan.cpp); geometry 2 or 3, with quads also the short tiles 4 and 5
      case EPI_R2 | EPI_STATS | EPI_QUADS:
        if (p.geom == 4) return big_dual_launch<U, EPI_R2 | EPI_STATS | EPI_QUADS, 2, 2, 3>(a, X2, p, s);
        if (p.geom == 5) return big_dual_launch<U, EPI_R2 | EPI_STATS | EPI_QUADS, 2, 2, 4>(a, X2, p, s);
        return p.geom == 2 ? big_dual_launch<U, EPI_R2 | EPI_STATS | EPI_QUADS, 2, 4>(a, X2, p, s)
                           : big_dual_launch<U, EPI_R2 | EPI_STATS | EPI_QUADS, 2, 2>(a, X2, p, s);
      case EPI_R2 | EPI_STATS:
        return p.geom == 2 ? big_dual_launch<U, EPI_R2 | EPI_STATS, 2, 4>(a, X2, p, s) : big_dual_launch<U, EPI_R2 | EPI_STATS, 2, 2>(a, X2, p, s);
      case EPI_R2: return p.geom == 2 ? big_dual_launch<U, EPI_R2, 2, 4>(a, X2, p, s) : big_dual_launch<U, EPI_R2, 2, 2>(a, X2, p, s);
      default: break;      // no plan names another one (tests/test_launch_plan_api.py)
    }
    return D3PM_E_SHAPE;
  };
  return dtype == D3PM_F16 ? go(static_cast<f16*>(nullptr)) : go(static_cast<bf16*>(nullptr));
}

int big_linear(int dtype, const LinearArgs& a, const LinearPlan& p, hipStream_t s) {
  auto go = [&](auto* tag) -> int {
    using U = std::remove_pointer_t<decltype(tag)>;
    switch (p.epi) {      // kEpiBig (d3pm_plan.cpp)
      case EPI_LNF: return big_launch_geometry<U, EPI_LNF>(a, p, s);
      case EPI_LNF | EPI_GELU: return big_launch_geometry<U, EPI_LNF | EPI_GELU>(a, p, s);
      case EPI_R1 | EPI_STATS: return big_launch_geometry<U, EPI_R1 | EPI_STATS>(a, p, s);
      case EPI_R2 | EPI_STATS: return big_launch_geometry<U, EPI_R2 | EPI_STATS>(a, p, s);
      case EPI_R1 | EPI_MASK | EPI_STATS: return big_launch_geometry<U, EPI_R1 | EPI_MASK | EPI_STATS>(a, p, s);
      case EPI_LNF | EPI_QUADS: return big_launch_geometry<U, EPI_LNF | EPI_QUADS>(a, p, s);
      case EPI_LNF | EPI_GELU | EPI_QUADS: return big_launch_geometry<U, EPI_LNF | EPI_GELU | EPI_QUADS>(a, p, s);
      case EPI_R1 | EPI_STATS | EPI_QUADS: return big_launch_geometry<U, EPI_R1 | EPI_STATS | EPI_QUADS>(a, p, s);
      case EPI_R2 | EPI_STATS | EPI_QUADS: return big_launch_geometry<U, EPI_R2 | EPI_STATS | EPI_QUADS>(a, p, s);
      case EPI_R1 | EPI_MASK | EPI_STATS | EPI_QUADS: return big_launch_geometry<U, EPI_R1 | EPI_MASK | EPI_STATS | EPI_QUADS>(a, p, s);
      case 0: return big_launch_geometry<U, 0>(a, p, s);
      case EPI_GELU: return big_launch_geometry<U, EPI_GELU>(a, p, s);
      case EPI_R1: return big_launch_geometry<U, EPI_R1>(a, p, s);
      case EPI_R2: return big_launch_geometry<U, EPI_R2>(a, p, s);
      case EPI_R1 | EPI_MASK: return big_launch_geometry<U, EPI_R1 | EPI_MASK>(a, p, s);
      default: break;      // no plan names another one (tests/test_launch_plan_api.py)
    }
    return D3PM_E_SHAPE;
  };
  return dtype == D3PM_F16 ? go(static_cast<f16*>(nullptr)) : go(static_cast<bf16*>(nullptr));
}

// ---- row-panel fusion: projection onto the residual stream + the LayerNorm(s) that read it next, one launch ----------
// Instantiated: out-proj + x -> norm2 | norm22 (EPI_R1, two LayerNorms); both cross-attention out-projections + x -> norm3 with
// FiLM (EPI_R2 from registers); fc2 + x, frame mask -> the next block's norm1 (EPI_R1 | EPI_MASK).
static int row_panel_kind(const LinearArgs& a, const RowPanelFuse& f) {
  const bool r1 = a.R1 != nullptr, mk = a.row_mask != nullptr, dual = f.X2 != nullptr, ln2 = f.lnw2 != nullptr, film = f.film != nullptr;
  if (!r1 || a.R2 || !f.lnw || !f.lnb || !f.lny || a.act != ACT_NONE) return 0;
  if (ln2 != (f.lnb2 != nullptr) || ln2 != (f.lny2 != nullptr)) return 0;
  if (!dual && !mk && ln2 && !film) return 1;
  if (dual && !mk && !ln2 && film) return 2;
  if (!dual && mk && !ln2 && !film) return 3;
  return 0;
}

bool row_panel_supported(int dtype, const LinearArgs& a, const RowPanelFuse& f) {
  if (dtype != D3PM_F16 && dtype != D3PM_BF16) return false;
  if (a.N != 512 || a.ldy != 512 || a.ldr != 512 || a.M < 96 || a.M % 96 != 0 || a.K < 4 * BK || a.K % (2 * BK) != 0) return false;
  if (a.ldx % 8 != 0 || a.ldx >= (1 << 24) || a.K >= (1 << 24) || !a.bias) return false;
  for (const void* p : {a.X, a.W, static_cast<const void*>(a.Y), a.R1, a.bias, f.X2, f.lnw, f.lnb, f.lnw2, f.lnb2, f.film,
                        static_cast<const void*>(f.lny), static_cast<const void*>(f.lny2)})
    if (!aligned16(p)) return false;
  if ((f.sx != nullptr) != (f.sx2 != nullptr) && f.lnw2) return false;     // both LayerNorm outputs in the same format
  if (f.sx && row_panel_kind(a, f) == 3) return false;                       // MX outputs: the two forms the fp8 fast path uses
  return row_panel_kind(a, f) != 0;
}

template <typename U, int E, int FUSE>
static int row_panel_launch(const LinearArgs& a, const RowPanelFuse& f, hipStream_t s) {
  static_assert((FUSE & FUSE_MX) == 0 || (FUSE & FUSE_LN) != 0, "MX output = LayerNorm output");
  const int tiles_total = a.M / 96, want = (tiles_total + 7) & ~7;
  const dim3 grid(static_cast<unsigned>(want < 256 ? want : 256));
  const size_t lds = 2 * static_cast<size_t>(96 + 512) * ROW_BYTES + 2 * 96 * 8 * sizeof(float);
  D3PM_LDS_ATTR((&gemm_mfma_big<U, E, 1, 8, FUSE>), 160 * 1024);
  RowPanelArgs<U> rp{static_cast<const U*>(f.X2), static_cast<const U*>(f.lnw), static_cast<const U*>(f.lnb),
                     static_cast<const U*>(f.lnw2), static_cast<const U*>(f.lnb2), static_cast<const U*>(f.film),
                     static_cast<U*>(f.lny), static_cast<U*>(f.lny2), f.eps, static_cast<uint8_t*>(f.sx), static_cast<uint8_t*>(f.sx2)};
  gemm_mfma_big<U, E, 1, 8, FUSE><<<grid, dim3(512), lds, s>>>(
      static_cast<const U*>(a.X), a.ldx, static_cast<const U*>(a.W), static_cast<const U*>(a.bias), static_cast<U*>(a.Y), a.ldy,
      static_cast<const U*>(a.R1), nullptr, a.ldr, a.row_mask, a.mask_period, a.M, a.N, a.K, 1, tiles_total, rp, EpiFold{});
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

int row_panel_linear(int dtype, const LinearArgs& a, const RowPanelFuse& f, hipStream_t s) {
  const int kind = row_panel_kind(a, f);
  auto go = [&](auto* tag) -> int {
    using U = std::remove_pointer_t<decltype(tag)>;
    switch (kind) {
      case 1:
        if (f.sx) return row_panel_launch<U, EPI_R1, FUSE_LN | FUSE_LN2 | FUSE_MX>(a, f, s);
        return row_panel_launch<U, EPI_R1, FUSE_LN | FUSE_LN2>(a, f, s);
      case 2: return f.sx ? row_panel_launch<U, EPI_R2, FUSE_DUAL | FUSE_LN | FUSE_FILM | FUSE_MX>(a, f, s)
                          : row_panel_launch<U, EPI_R2, FUSE_DUAL | FUSE_LN | FUSE_FILM>(a, f, s);
      case 3: return row_panel_launch<U, EPI_R1 | EPI_MASK, FUSE_LN>(a, f, s);
      default: break;
    }
    set_error("row-panel projection: unsupported epilogue combination");
    return D3PM_E_SHAPE;
  };
  return dtype == D3PM_F16 ? go(static_cast<f16*>(nullptr)) : go(static_cast<bf16*>(nullptr));
}

}  // namespace d3pm
