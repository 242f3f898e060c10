// d3pm_mfma_attn.hip -- flash-style attention on MFMA for head_dim 64 (f16 / bf16), gfx950.
//
// Replaces the need_weights branch of torch's multi_head_attention_forward as called by
// DiTBlock.forward (/root/reference/vall_e/vall_e/ar_discrete.py:132 self, :138 text, :142 prompt):
// q*sqrt(1/hd) -> bmm -> softmax -> bmm.  The [T,S] score matrix and the head-averaged weights the
// reference materialises (and throws away) never exist here.
//
// Workgroup = 4 wave64 = 64 (QG=1) or 128 (QG=2) queries of one (utterance, head); each wave owns 16*QG queries and walks
// the keys in tiles of 64 with an online softmax.
//   * S^T = K.Q^T by v_mfma_f32_16x16x32 (K fragment = A operand from LDS, Q fragment = B operand
//     held in registers for the whole kernel): a lane holds 4 consecutive keys x 4 key tiles of ONE
//     query, so max / sum run in-lane plus two xor-shuffles (lanes l, l^16, l^32, l^48 share a query);
//   * the exponentiated scores of two key tiles, converted to 16 bit, ARE the B operand of the
//     P.V product (contraction index permuted consistently on both operands): no LDS round trip;
//   * V stays row-major in LDS and is read column-major with ds_read_b64_tr_b16 (4 keys x 16
//     columns per 16-lane group) as the A operand, giving O^T: a lane owns 4 consecutive output
//     columns of its own query, so the softmax rescale needs no cross-lane traffic;
//   * K and V tiles are staged global -> registers -> LDS (16 B per lane) one tile ahead, one
//     barrier per tile; 128-B LDS rows, 16-B chunks XOR-swizzled (K: (row>>1)&7 for the b128
//     fragment reads, V: ((row>>1)&3)<<1 for the transposed reads) -- conflict-free by construction.
// Numerics (flash-style, NOT the eager rounding points -- the generic attention_rows keeps those): scores stay
// fp32 in the log2 domain, the probabilities enter the second MFMA un-normalised (2^(s-m) <= 1, rounded to
// the storage dtype), the row sum is accumulated in fp32 and divided out at the end.  Differs from the eager
// round(bmm) -> softmax -> round -> bmm chain by rounding noise only (precision modes).
// The softmax is VALU-bound at head_dim 64 (256 flop of MFMA per score), so it is kept to ~6 VALU issue
// slots per score: max, sub, v_exp_f32, add, half a cvt_pk; the O rescale is skipped when no maximum moved
// and the key-padding compare/select only runs on a ragged last tile.
#include "d3pm_plan.h"      // HD, BKV, ROWB, TILE and the AttnPlan the launchers take

namespace d3pm {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((ext_vector_type(4)));


template <typename T> __device__ __forceinline__ floatx4 mma(uint4 a, uint4 b, floatx4 c);
template <> __device__ __forceinline__ floatx4 mma<f16>(uint4 a, uint4 b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ floatx4 mma<bf16>(uint4 a, uint4 b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ int k_off(int row, int chunk) { return row * ROWB + ((chunk ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int v_off(int row, int chunk) { return row * ROWB + ((chunk ^ (((row >> 1) & 3) << 1)) << 4); }

constexpr float kDefer = 8.0f;   // log2 of the largest un-normalised probability tolerated before m_ref is raised

// max over the four lanes l, l^16, l^32, l^48 on the VALU (no LDS round trip): after v_permlane16_swap of two copies
// one holds the even 16-lane rows twice and the other the odd rows twice; v_permlane32_swap does the same for halves.
// Inline asm: see the note on the two-result builtin in d3pm_mfma_gemm.hip; s_nop 1 = the VALU-write hazard.
__device__ __forceinline__ float max_over_query_lanes(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  x = fmaxf(a, b);
  a = x;
  b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return fmaxf(a, b);
}

// two floats -> one packed 16-bit pair; the vector conversion lowers to a single v_cvt_pk_{bf16,f16}_f32
template <typename T> __device__ __forceinline__ uint32_t pack2(float a, float b) {
  typedef float float2v __attribute__((ext_vector_type(2)));
  typedef T pair __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((float2v){a, b}, pair));
}

// Output rows of the 16 x 16 kernels.  A lane holds, per 16-column block dt of its query's 64 output columns, columns
// 16 dt + 4 g .. + 3 (g = lane >> 4): four 8-byte stores per query group, a tail bound by the number of store INSTRUCTIONS
// (MI355X_MICROARCH.md, 'attention epilogue store tail').  v_permlane16_swap between the packed registers of blocks dt and dt + 1
// (odd 16-lane rows of the first trade places with the even rows of the second -- the regrouping of the GEMM epilogue,
// d3pm_mfma_tile.h) leaves a lane with 8 consecutive columns (dt + (g & 1)) 16 + (g >> 1) 8 .. + 7: two 16-byte stores, same
// bytes, same addresses.  Every lane takes part in the swaps; only the store is predicated.
template <typename T>
__device__ __forceinline__ void store_rows16(T* row_base /* O + row * ldo + h * 64, 16-byte aligned */, const floatx4 (&acc)[4], float inv, int g,
                                             bool live) {
#pragma unroll
  for (int dt = 0; dt < 4; dt += 2) {
    uint32_t ax = pack2<T>(acc[dt][0] * inv, acc[dt][1] * inv), ay = pack2<T>(acc[dt][2] * inv, acc[dt][3] * inv);
    uint32_t bx = pack2<T>(acc[dt + 1][0] * inv, acc[dt + 1][1] * inv), by = pack2<T>(acc[dt + 1][2] * inv, acc[dt + 1][3] * inv);
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(ax), "+v"(bx));
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(ay), "+v"(by));
    if (live) *reinterpret_cast<uint4*>(row_base + (dt + (g & 1)) * 16 + (g >> 1) * 8) = uint4{ax, ay, bx, by};
  }
}

template <typename T, int QG, bool PAIR>   // QG groups of 16 queries per wave (K/V fragments are read once per wave and reused)
__global__ __launch_bounds__(256, QG == 1 ? 4 : 2) void attn_mfma_hd64(const T* __restrict__ Q, int ldq, const T* __restrict__ Kp,
                                                      const T* __restrict__ Vp, int ldkv, T* __restrict__ O, int ldo,
                                                      int Tq, int S, float scale, int H, int n_qblocks,
                                                      const T* __restrict__ Q2, const T* __restrict__ K2,
                                                      const T* __restrict__ V2, T* __restrict__ O2, int S2, int n_first,
                                                      const int32_t* __restrict__ key_len, const int32_t* __restrict__ key_len2) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILE];   // [buffer][K tile | V tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // 1-D grid, XCD-aware order: workgroups are dealt round-robin over the 8 XCDs, so give each XCD a contiguous
  // range of (utterance, head, query-block) ids -- the query blocks that share one K/V then share one L2
  // (PMC: L2 hit rate of the plain 3-D grid was 42 %).
  int bid;
  {
    const int nblocks = gridDim.x, q = nblocks >> 3, r = nblocks & 7, xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  // Paired launch (the text and prompt cross-attentions of a block: same queries' rows, different Q / K / V): n_first
  // < 0 -> every workgroup runs problem 1 and then problem 2 for its query block, sharing its fixed costs (half the
  // workgroups; the 50-key text problem alone is a single tile per workgroup); n_first >= 0 -> the second half of the
  // grid takes problem 2.
  const bool sequential = PAIR && n_first < 0;
  if (!sequential && bid >= n_first) {   // block-uniform
    bid -= n_first;
    Q = Q2; Kp = K2; Vp = V2; O = O2; S = S2; key_len = key_len2;
  }
  const int qb = bid % n_qblocks, h = (bid / n_qblocks) % H, b = bid / (n_qblocks * H);
  for (int prob = 0; prob < (PAIR ? 2 : 1); ++prob) {
  if (prob == 1) { Q = Q2; Kp = K2; Vp = V2; O = O2; S = S2; key_len = key_len2; }
  const int S_pad = S;                                 // row stride of the K/V batches
  if (key_len) S = min(key_len[b], S_pad);             // valid keys of this utterance (>= 1)
  const int q0 = (qb * 4 + wave) * (16 * QG);
  const int qi = lane & 15, g = lane >> 4;
  const T* Kb = Kp + static_cast<size_t>(b) * S_pad * ldkv + h * HD;
  const T* Vb = Vp + static_cast<size_t>(b) * S_pad * ldkv + h * HD;

  // Q fragments (B operand of S^T = K.Q^T): lane holds q[query][32*ks + 8g .. +7], pre-scaled by
  // sqrt(1/hd) * log2(e) so that the scores come out of the MFMA in the log2 domain (softmax via v_exp_f32)
  const float qscale = scale * 1.4426950408889634f;
  uint4 qf[QG][2];
#pragma unroll
  for (int qg = 0; qg < QG; ++qg) {
    int qrow = q0 + qg * 16 + qi;
    qrow = qrow < Tq ? qrow : Tq - 1;
    const T* qp = Q + (static_cast<size_t>(b) * Tq + qrow) * ldq + h * HD;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      typedef T tvec8 __attribute__((ext_vector_type(8)));
      const tvec8 e = __builtin_bit_cast(tvec8, *reinterpret_cast<const uint4*>(qp + ks * 32 + g * 8));
      qf[qg][ks] = uint4{pack2<T>(static_cast<float>(e[0]) * qscale, static_cast<float>(e[1]) * qscale),
                         pack2<T>(static_cast<float>(e[2]) * qscale, static_cast<float>(e[3]) * qscale),
                         pack2<T>(static_cast<float>(e[4]) * qscale, static_cast<float>(e[5]) * qscale),
                         pack2<T>(static_cast<float>(e[6]) * qscale, static_cast<float>(e[7]) * qscale)};
    }
  }

  // staging: thread -> 2 x 16 B of the K tile and 2 x 16 B of the V tile (rows r0s and r0s+32, chunk chs);
  // plain scalars / by-value struct so that the in-flight tile lives in VGPRs, not in scratch
  const int r0s = tid >> 3, chs = tid & 7;
  const int ko0 = k_off(r0s, chs), ko1 = k_off(r0s + 32, chs), vo0 = v_off(r0s, chs), vo1 = v_off(r0s + 32, chs);
  struct Staged { uint4 k0, k1, v0, v1; };
  // whole tiles: a wave-uniform tile base (scalar registers) + two per-lane byte offsets that never change, so a tile costs
  // no vector address arithmetic; only a ragged last tile clamps its rows
  const uint32_t lo0 = static_cast<uint32_t>(r0s * ldkv + chs * 8) * 2u, lo1 = lo0 + static_cast<uint32_t>(32 * ldkv) * 2u;
  auto load_tile = [=](int tile) -> Staged {
    Staged st;
    const char* kt = reinterpret_cast<const char*>(Kb + static_cast<size_t>(tile) * BKV * ldkv);
    const char* vt = reinterpret_cast<const char*>(Vb + static_cast<size_t>(tile) * BKV * ldkv);
    if ((tile + 1) * BKV <= S) {
      st.k0 = *reinterpret_cast<const uint4*>(kt + lo0);
      st.k1 = *reinterpret_cast<const uint4*>(kt + lo1);
      st.v0 = *reinterpret_cast<const uint4*>(vt + lo0);
      st.v1 = *reinterpret_cast<const uint4*>(vt + lo1);
    } else {
      int a = tile * BKV + r0s, c = a + 32;
      a = a < S ? a : S - 1;
      c = c < S ? c : S - 1;
      st.k0 = *reinterpret_cast<const uint4*>(Kb + static_cast<size_t>(a) * ldkv + chs * 8);
      st.k1 = *reinterpret_cast<const uint4*>(Kb + static_cast<size_t>(c) * ldkv + chs * 8);
      st.v0 = *reinterpret_cast<const uint4*>(Vb + static_cast<size_t>(a) * ldkv + chs * 8);
      st.v1 = *reinterpret_cast<const uint4*>(Vb + static_cast<size_t>(c) * ldkv + chs * 8);
    }
    return st;
  };
  auto store_tile = [=](char* base, const Staged& st) {
    *reinterpret_cast<uint4*>(base + ko0) = st.k0;
    *reinterpret_cast<uint4*>(base + ko1) = st.k1;
    *reinterpret_cast<uint4*>(base + TILE + vo0) = st.v0;
    *reinterpret_cast<uint4*>(base + TILE + vo1) = st.v1;
  };

  const int n_tiles = (S + BKV - 1) / BKV;
  Staged st = load_tile(0);
  store_tile(smem, st);
  __syncthreads();

  float m_ref[QG];
  floatx4 negm[QG], acc_o[QG][4], acc_l[QG];
  const uint32_t one2 = pack2<T>(1.0f, 1.0f);
  const uint4 ones = uint4{one2, one2, one2, one2};
#pragma unroll
  for (int qg = 0; qg < QG; ++qg) {
    m_ref[qg] = 0.f;
    negm[qg] = floatx4{0.f, 0.f, 0.f, 0.f};
    acc_l[qg] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc_o[qg][dt] = floatx4{0.f, 0.f, 0.f, 0.f};
  }

  // per-lane LDS offsets of the fragment reads, computed once: the XOR swizzle only touches address bits that the tile-local
  // row / column-block constants do not, so every read of a tile is one of these plus an instruction immediate
  //   K (b128): row 16 kt + qi, chunk 4 ks + g          -> ok[ks] + kt * 2048
  //   V (tr b64): row 32 kb2 + 16 half + 4 g + (qi >> 2), columns 16 dt + 4 (qi & 3) -> ov[dt] + kb2 * 4096 + half * 2048
  int ok[2], ov[4];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) ok[ks] = k_off(qi, ks * 4 + g);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const int col = dt * 16 + 4 * (qi & 3);
    ov[dt] = v_off(4 * g + (qi >> 2), col >> 3) + (col & 7) * 2;
  }
  // two tiles per trip so that the buffer a tile reads (and the one it fills) is a compile-time constant
  auto do_tile = [&](int tile, auto BUF_) __attribute__((always_inline)) {
    constexpr int BUF = decltype(BUF_)::value;
    const char* kb = smem + BUF * 2 * TILE;
    const char* vb = kb + TILE;
    const bool more = tile + 1 < n_tiles;
    if (more) st = load_tile(tile + 1);

    // ---- S^T tile: 64 keys x (16 QG) queries per wave; each K fragment feeds QG MFMAs ----
    // The accumulator starts at -m_ref (one register quad per query group, shared by the four key tiles as the C
    // operand), so the scores leave the matrix pipe already relative to the running reference: no subtraction.
    floatx4 s[QG][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        uint4 kf = *reinterpret_cast<const uint4*>(kb + ok[ks] + kt * 16 * ROWB);
#pragma unroll
        for (int qg = 0; qg < QG; ++qg) s[qg][kt] = mma<T>(kf, qf[qg][ks], ks == 0 ? negm[qg] : s[qg][kt]);
      }
    // lane holds scores (log2 domain, minus m_ref) of its query for keys tile*64 + kt*16 + 4g + r
    const bool ragged = (tile == n_tiles - 1) && (S & (BKV - 1));   // wave-uniform: only the last tile can be partial
    uint4 pf[QG][2];
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
      if (ragged) {
        const int lim = S - tile * BKV - 4 * g;              // keys of this lane's column that exist: compare with constants
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[qg][kt][r] = (kt * 16 + r < lim) ? s[qg][kt][r] : -INFINITY;
      }
      float mx = fmaxf(s[qg][0][0], s[qg][0][1]);          // linear chain: hipcc folds pairs into v_max3_f32
      mx = fmaxf(fmaxf(mx, s[qg][0][2]), s[qg][0][3]);
#pragma unroll
      for (int kt = 1; kt < 4; ++kt) {
        mx = fmaxf(fmaxf(mx, s[qg][kt][0]), s[qg][kt][1]);
        mx = fmaxf(fmaxf(mx, s[qg][kt][2]), s[qg][kt][3]);
      }
      // Deferred maximum: m_ref only moves when some score of the wave exceeds it by more than 2^kDefer (or on the
      // first tile), so the common tile does neither the cross-lane maximum nor the rescale of O; probabilities are
      // then at most 2^kDefer instead of 1, which neither fp32 sums nor 16-bit P notice (normalised by the same sum).
      if (tile == 0 || __any(mx > kDefer)) {               // wave-uniform
        mx = max_over_query_lanes(mx);                     // lanes l, l^16, l^32, l^48 share a query
        const float delta = tile == 0 ? mx : fmaxf(mx, 0.f);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[qg][kt][r] -= delta;
        if (tile != 0) {                                   // on the first tile O and l are still zero
          const float alpha = __builtin_amdgcn_exp2f(-delta);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc_l[qg][r] *= alpha;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc_o[qg][dt][r] *= alpha;
        }
        m_ref[qg] += delta;
        negm[qg] = floatx4{-m_ref[qg], -m_ref[qg], -m_ref[qg], -m_ref[qg]};
      }
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[qg][kt][r] = __builtin_amdgcn_exp2f(s[qg][kt][r]);
      // contraction index j<4 -> key tile 2kb, j>=4 -> key tile 2kb+1 (same permutation as the V reads)
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2) {
        const floatx4 pa = s[qg][2 * kb2], pb = s[qg][2 * kb2 + 1];
        pf[qg][kb2] = uint4{pack2<T>(pa[0], pa[1]), pack2<T>(pa[2], pa[3]), pack2<T>(pb[0], pb[1]), pack2<T>(pb[2], pb[3])};
      }
    }

    // ---- O^T += V^T . P^T ; each transposed V fragment feeds QG MFMAs ----
#pragma unroll
    for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        // 16-lane group g, lane qi: address of row (key0 + qi>>2), columns 16dt + 4(qi&3) .. +3
        typedef short4v __attribute__((address_space(3))) * lds_ptr;
        short4v va = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(vb + ov[dt] + (2 * kb2) * 16 * ROWB));
        short4v vc = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(vb + ov[dt] + (2 * kb2 + 1) * 16 * ROWB));
        uint2 lo = __builtin_bit_cast(uint2, va), hi = __builtin_bit_cast(uint2, vc);
        const uint4 vf = uint4{lo.x, lo.y, hi.x, hi.y};
#pragma unroll
        for (int qg = 0; qg < QG; ++qg) acc_o[qg][dt] = mma<T>(vf, pf[qg][kb2], acc_o[qg][dt]);
      }
    // row sums on the matrix pipe: ones^T . P^T adds the (rounded) probabilities of all 64 keys of the tile for
    // the lane's query into every register of acc_l -- 2 MFMAs instead of 16 v_add + the final shuffles
#pragma unroll
    for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
      for (int qg = 0; qg < QG; ++qg) acc_l[qg] = mma<T>(ones, pf[qg][kb2], acc_l[qg]);
    if (more) store_tile(smem + (BUF ^ 1) * 2 * TILE, st);
    __syncthreads();
  };
  for (int tile = 0; tile < n_tiles; tile += 2) {
    do_tile(tile, std::integral_constant<int, 0>{});
    if (tile + 1 < n_tiles) do_tile(tile + 1, std::integral_constant<int, 1>{});
  }

#pragma unroll
  for (int qg = 0; qg < QG; ++qg) {
    const float inv = 1.0f / acc_l[qg][0];
    const int qrow = q0 + qg * 16 + qi;
    store_rows16<T>(O + (static_cast<size_t>(b) * Tq + (qrow < Tq ? qrow : Tq - 1)) * ldo + h * HD, acc_o[qg], inv, g, qrow < Tq);
  }
  }   // problems of a sequential pair
}

// ---- cross-attention pair with short key sequences: attn_cross_hd64 ---------------------------------------------------
// The text (<= 64 keys) and prompt (<= 256 keys) cross-attentions of a DiT block (ar_discrete.py:138,142) are two tiny
// problems per query block: at B = 32 the tile-by-tile kernel above spends 49 us on 13.8 GFLOP (measured in situ) -- five
// dependent load -> LDS -> barrier rounds per workgroup at two workgroups per CU, i.e. pure latency.  Here EVERY K / V tile of
// both problems (<= 80 KiB) is fetched into LDS by direct-to-LDS DMA at kernel entry, all pieces in flight at once, the
// workgroup waits once and then runs the five tiles back to back with no further barrier.  Eight waves x 32 queries share
// the tiles (256 queries per workgroup).  Arithmetic per tile is the code of attn_mfma_hd64 (same rounding, same order).
typedef const __attribute__((address_space(1))) void* glb_ptr_t;
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// A software-pipelined walk (the products of tile i + 1 issued before the softmax of tile i) was built, measured and not shipped
// (source up to commit d54b189).
// MASK: key_len1 / key_len2 (device int32 [B], either may be null) = the valid keys of utterance b among the S1 / S2 padded ones.
// S1 / S2 stay the row strides of the batches; behind them the kernel is the unmasked one on the valid counts (only their tiles
// are fetched, the ragged last tile is masked as ever).
template <typename T, bool MASK = false>
__global__ __launch_bounds__(512, 2) void attn_cross_hd64(const T* __restrict__ Q1, const T* __restrict__ K1, const T* __restrict__ V1,
                                                          T* __restrict__ O1, int S1, const T* __restrict__ Q2,
                                                          const T* __restrict__ K2, const T* __restrict__ V2, T* __restrict__ O2,
                                                          int S2, int ldq, int ldkv, int ldo, int Tq, float scale, int H,
                                                          int n_qblocks, int n_qsplit, const int32_t* __restrict__ key_len1,
                                                          const int32_t* __restrict__ key_len2) {
  constexpr int QG = 2, MAXT = 5;                            // 1 text tile + up to 4 prompt tiles
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [tile][K | V], 16 KiB per tile
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bid;
  {
    const int nblocks = gridDim.x, q = nblocks >> 3, r = nblocks & 7, xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  // a workgroup keeps the K / V image of its (utterance, head) and walks the query blocks qs, qs + n_qsplit, ..: at the
  // throughput batch n_qsplit = 1 -- one workgroup per CU, one DMA flight per (utterance, head) instead of one per query block
  const int qs = bid % n_qsplit, h = (bid / n_qsplit) % H, b = bid / (n_qsplit * H);
  const int S1_pad = S1, S2_pad = S2;                        // row strides of the K / V batches
  if constexpr (MASK) {
    if (key_len1) S1 = min(key_len1[b], S1_pad);
    if (key_len2) S2 = min(key_len2[b], S2_pad);
  }
  const int nt2 = (S2 + BKV - 1) / BKV, n_tiles = 1 + nt2;
  // ---- every K / V piece of both problems: 16 pieces (1 KiB = 8 rows x 128 B) per tile, dealt over the 8 waves
  {
    const int lrow = lane >> 3, cpos = lane & 7;
    const int total = n_tiles * 16;
    for (int p = wave; p < total; p += 8) {                 // wave-uniform trip count
      const int tile = p >> 4, which = (p >> 3) & 1, j = p & 7;   // which: 0 = K, 1 = V
      const int row = 8 * j + lrow;
      const int logical = which == 0 ? (cpos ^ ((row >> 1) & 7)) : (cpos ^ (((row >> 1) & 3) << 1));
      const T* base = tile == 0 ? (which == 0 ? K1 : V1) : (which == 0 ? K2 : V2);
      const int S = tile == 0 ? S1 : S2, S_pad = tile == 0 ? S1_pad : S2_pad;
      int key = (tile == 0 ? 0 : (tile - 1) * BKV) + row;
      key = key < S ? key : S - 1;
      const T* src = base + (static_cast<size_t>(b) * S_pad + key) * ldkv + h * HD + logical * 8;
      __builtin_amdgcn_global_load_lds((glb_ptr_t)src, (lds_ptr_t)(smem + tile * 2 * TILE + which * TILE + j * 1024), 16, 0, 0);
    }
  }
  const int qi = lane & 15, g = lane >> 4;
  const float qscale = scale * 1.4426950408889634f;
  const uint32_t one2 = pack2<T>(1.0f, 1.0f);
  const uint4 ones = uint4{one2, one2, one2, one2};
  bool landed = false;
  // the queries of a (query block, problem) phase are fetched one phase ahead: raw rows in registers while the previous phase
  // computes, scaled and packed at the top of their own phase
  uint4 qraw[QG][2];
  auto fetch_q = [&](int qb, int prob) __attribute__((always_inline)) {
    const T* Q = prob == 0 ? Q1 : Q2;
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
      int qrow = (qb * 8 + wave) * (16 * QG) + qg * 16 + qi;
      qrow = qrow < Tq ? qrow : Tq - 1;
      const T* qp = Q + (static_cast<size_t>(b) * Tq + qrow) * ldq + h * HD;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) qraw[qg][ks] = *reinterpret_cast<const uint4*>(qp + ks * 32 + g * 8);
    }
  };
  fetch_q(qs, 0);
  for (int qb = qs; qb < n_qblocks; qb += n_qsplit) {
  const int q0 = (qb * 8 + wave) * (16 * QG);
  for (int prob = 0; prob < 2; ++prob) {
    T* O = prob == 0 ? O1 : O2;
    const int S = prob == 0 ? S1 : S2, t0 = prob == 0 ? 0 : 1, nt = prob == 0 ? 1 : nt2;
    uint4 qf[QG][2];
#pragma unroll
    for (int qg = 0; qg < QG; ++qg)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        typedef T tvec8 __attribute__((ext_vector_type(8)));
        const tvec8 e = __builtin_bit_cast(tvec8, qraw[qg][ks]);
        qf[qg][ks] = uint4{pack2<T>(static_cast<float>(e[0]) * qscale, static_cast<float>(e[1]) * qscale),
                           pack2<T>(static_cast<float>(e[2]) * qscale, static_cast<float>(e[3]) * qscale),
                           pack2<T>(static_cast<float>(e[4]) * qscale, static_cast<float>(e[5]) * qscale),
                           pack2<T>(static_cast<float>(e[6]) * qscale, static_cast<float>(e[7]) * qscale)};
      }
    if (prob == 0) fetch_q(qb, 1);
    else if (qb + n_qsplit < n_qblocks) fetch_q(qb + n_qsplit, 0);
    if (!landed) {                                           // one wait for the whole workgroup's K / V image
      __syncthreads();                                       // (drains this wave's DMA pieces, then the barrier)
      landed = true;
    }
    float m_ref[QG];
    floatx4 negm[QG], acc_o[QG][4], acc_l[QG];
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
      m_ref[qg] = 0.f;
      negm[qg] = floatx4{0.f, 0.f, 0.f, 0.f};
      acc_l[qg] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) acc_o[qg][dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    // S^T of one tile from the current -m_ref
    auto qk_tile = [&](int tile, floatx4 (&s)[QG][4]) __attribute__((always_inline)) {
      const char* kb = smem + (t0 + tile) * 2 * TILE;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          uint4 kf = *reinterpret_cast<const uint4*>(kb + k_off(kt * 16 + qi, ks * 4 + g));
#pragma unroll
          for (int qg = 0; qg < QG; ++qg) s[qg][kt] = mma<T>(kf, qf[qg][ks], ks == 0 ? negm[qg] : s[qg][kt]);
        }
    };
    // softmax of one tile's scores -> the 16-bit probabilities as PV operands
    auto softmax_tile = [&](int tile, floatx4 (&s)[QG][4], uint4 (&pf)[QG][2]) __attribute__((always_inline)) {
      const bool ragged = (tile == nt - 1) && (S & (BKV - 1));
      const int key_base = tile * BKV + 4 * g;
#pragma unroll
      for (int qg = 0; qg < QG; ++qg) {
        if (ragged) {
#pragma unroll
          for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[qg][kt][r] = (key_base + kt * 16 + r < S) ? s[qg][kt][r] : -INFINITY;
        }
        float mx = fmaxf(s[qg][0][0], s[qg][0][1]);
        mx = fmaxf(fmaxf(mx, s[qg][0][2]), s[qg][0][3]);
#pragma unroll
        for (int kt = 1; kt < 4; ++kt) {
          mx = fmaxf(fmaxf(mx, s[qg][kt][0]), s[qg][kt][1]);
          mx = fmaxf(fmaxf(mx, s[qg][kt][2]), s[qg][kt][3]);
        }
        if (tile == 0 || __any(mx > kDefer)) {
          mx = max_over_query_lanes(mx);
          const float delta = tile == 0 ? mx : fmaxf(mx, 0.f);
#pragma unroll
          for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[qg][kt][r] -= delta;
          if (tile != 0) {
            const float alpha = __builtin_amdgcn_exp2f(-delta);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc_l[qg][r] *= alpha;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
              for (int r = 0; r < 4; ++r) acc_o[qg][dt][r] *= alpha;
          }
          m_ref[qg] += delta;
          negm[qg] = floatx4{-m_ref[qg], -m_ref[qg], -m_ref[qg], -m_ref[qg]};
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[qg][kt][r] = __builtin_amdgcn_exp2f(s[qg][kt][r]);
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2) {
          const floatx4 pa = s[qg][2 * kb2], pb = s[qg][2 * kb2 + 1];
          pf[qg][kb2] = uint4{pack2<T>(pa[0], pa[1]), pack2<T>(pa[2], pa[3]), pack2<T>(pb[0], pb[1]), pack2<T>(pb[2], pb[3])};
        }
      }
    };
    auto pv_tile = [&](int tile, const uint4 (&pf)[QG][2]) __attribute__((always_inline)) {
      const char* vb = smem + (t0 + tile) * 2 * TILE + TILE;
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const int col = dt * 16 + 4 * (qi & 3);
          const int r0 = (2 * kb2) * 16 + 4 * g + (qi >> 2), r1 = r0 + 16;
          typedef short4v __attribute__((address_space(3))) * lds_ptr;
          short4v va = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(vb + v_off(r0, col >> 3) + (col & 7) * 2));
          short4v vc = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(vb + v_off(r1, col >> 3) + (col & 7) * 2));
          uint2 lo = __builtin_bit_cast(uint2, va), hi = __builtin_bit_cast(uint2, vc);
          const uint4 vf = uint4{lo.x, lo.y, hi.x, hi.y};
#pragma unroll
          for (int qg = 0; qg < QG; ++qg) acc_o[qg][dt] = mma<T>(vf, pf[qg][kb2], acc_o[qg][dt]);
        }
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int qg = 0; qg < QG; ++qg) acc_l[qg] = mma<T>(ones, pf[qg][kb2], acc_l[qg]);
    };
    for (int tile = 0; tile < nt; ++tile) {
      floatx4 s[QG][4];
      uint4 pf[QG][2];
      qk_tile(tile, s);
      softmax_tile(tile, s, pf);
      pv_tile(tile, pf);
    }
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
      const float inv = 1.0f / acc_l[qg][0];
      const int qrow = q0 + qg * 16 + qi;
      store_rows16<T>(O + (static_cast<size_t>(b) * Tq + (qrow < Tq ? qrow : Tq - 1)) * ldo + h * HD, acc_o[qg], inv, g, qrow < Tq);
    }
  }
  }   // query blocks
  (void)MAXT;
}

}  // namespace

// Which kernel, which grid, how much LDS: plan_attention (d3pm_plan.cpp), where the tuning fields and the measurements behind the
// automatic choices are described.  What is left here is the plan -> instantiation table.
int mfma_attention(int dtype, const AttnArgs& a, const AttnPlan& p, hipStream_t s) {
  switch (p.kernel) {
    case ATTN_32P: case ATTN_32: case ATTN_32P_POOL: return mfma_attention32(dtype, a, p, s);
    case ATTN_32_CROSS: return mfma_attention32_cross(dtype, a, p, s);
    case ATTN_SPLIT: return mfma_attention_split(dtype, a, p, s);
    case ATTN_CROSS: case ATTN_TILES: break;
    default:
      set_error("attention: not planned for the MFMA family");
      return D3PM_E_SHAPE;
  }
  const int n_qblocks = p.n_qblocks, n_qsplit = p.n_qsplit, n_first = p.n_first;
  if (p.kernel == ATTN_CROSS) {
    const dim3 grid(p.grid), block(512);
#define D3PM_CROSS(T, MASK)                                                                                                  \
    do {                                                                                                                     \
      D3PM_LDS_ATTR((&attn_cross_hd64<T, MASK>), 5 * 2 * TILE);                                                              \
      attn_cross_hd64<T, MASK><<<grid, block, p.lds, s>>>(static_cast<const T*>(a.Q), static_cast<const T*>(a.K),             \
          static_cast<const T*>(a.V), static_cast<T*>(a.O), a.S, static_cast<const T*>(a.Q2), static_cast<const T*>(a.K2),    \
          static_cast<const T*>(a.V2), static_cast<T*>(a.O2), a.S2, a.ldq, a.ldkv, a.ldo, a.Tq, a.scale, a.H, n_qblocks, n_qsplit, \
          a.key_len, a.key_len2);                                                                                            \
    } while (0)
    if (p.masked) {
      if (dtype == D3PM_F16) D3PM_CROSS(f16, true); else D3PM_CROSS(bf16, true);
    } else if (dtype == D3PM_F16) D3PM_CROSS(f16, false); else D3PM_CROSS(bf16, false);
#undef D3PM_CROSS
    D3PM_LAUNCH_CHECK();
    return D3PM_OK;
  }
  const int qg = p.qg;
  const bool seq = p.pair_seq;
  const dim3 grid(p.grid), block(256);
#define D3PM_ATTN(T, QG, PAIR)                                                                                       \
  attn_mfma_hd64<T, QG, PAIR><<<grid, block, 0, s>>>(static_cast<const T*>(a.Q), a.ldq, static_cast<const T*>(a.K),  \
                                                     static_cast<const T*>(a.V), a.ldkv, static_cast<T*>(a.O), a.ldo, a.Tq, \
                                                     a.S, a.scale, a.H, n_qblocks, static_cast<const T*>(a.Q2),           \
                                                     static_cast<const T*>(a.K2), static_cast<const T*>(a.V2),           \
                                                     static_cast<T*>(a.O2), a.S2, n_first, a.key_len, a.key_len2)
#define D3PM_ATTN_QG(T)                                                                    \
  do {                                                                                     \
    if (seq) { if (qg == 1) D3PM_ATTN(T, 1, true); else D3PM_ATTN(T, 2, true); }           \
    else { if (qg == 1) D3PM_ATTN(T, 1, false); else D3PM_ATTN(T, 2, false); }             \
  } while (0)
  if (dtype == D3PM_F16) D3PM_ATTN_QG(f16); else D3PM_ATTN_QG(bf16);
#undef D3PM_ATTN_QG
#undef D3PM_ATTN
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

}  // namespace d3pm
