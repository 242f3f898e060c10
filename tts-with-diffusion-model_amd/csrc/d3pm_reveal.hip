// d3pm_reveal.hip -- confidence-ordered reveal (d3pm_reveal, include/d3pm_hip.h; MaskGIT / SoundStorm decoding on the absorbing
// canvas): one step is two launches behind the final projection,
//   reveal_candidate_rows     one wave per masked free row: the row's candidate id and its score (d3pm_sample_row.h reveal_from_z)
//   reveal_commit_rows        one wave per utterance: the quota of the step, the rows that come first in the order, their ids
//   reveal_commit_prep_rows   the loop's form of the second launch (NextIterPrep, d3pm_kernels.h): one wave per row, which runs its
//                             utterance's selection itself, commits its own row and gathers that row's embedding with its moments;
//                             the workgroups behind the row workgroups rebuild fc1 o norm3 o FiLM of the NEXT timestep.
// No LDS, no atomics, no barrier anywhere in this file.
#include <cmath>

#include "d3pm_kernels.h"
#include "d3pm_fold_rows.h"
#include "d3pm_sample_row.h"

namespace d3pm {
namespace {

constexpr int kRevealSlots = 16;      // lane l holds frames l + 64 i, i < 16: canvases up to 1024

// wave-uniform loads of one row's state: scalar branches on them
__device__ __forceinline__ int uniform_byte(const uint8_t* p, size_t i) { return __builtin_amdgcn_readfirstlane(static_cast<int>(p[i])); }

template <typename T, bool kKnown, int kFilter>
__global__ __launch_bounds__(256) void reveal_candidate_rows(
    const T* __restrict__ logits, int ldl, const int32_t* __restrict__ x_t, const uint8_t* __restrict__ frame_mask, int mask_period,
    const uint8_t* __restrict__ known, int32_t* __restrict__ cand_out, float* __restrict__ score_out, int rows, int K, int mask_id, uint64_t seed,
    uint32_t row0, int t, int greedy, float lambda, RowFilter flt, float top_p) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  // a row that is padded, known or already revealed leaves here: nothing read but its byte(s) and its id, nothing written
  if (uniform_byte(frame_mask, static_cast<size_t>(row) % mask_period) == 0) return;
  if constexpr (kKnown) {
    if (uniform_byte(known, row) != 0) return;
  }
  if (__builtin_amdgcn_readfirstlane(x_t[row]) != mask_id) return;
  const T* lr = logits + static_cast<size_t>(row) * ldl;
  const uint32_t grow = row0 + static_cast<uint32_t>(row);
  const RevealRow r = (K == 1025 && mask_id < 1024)      // kernel-uniform
      ? reveal_row_1025<T, kFilter>(lr, mask_id, seed, grow, static_cast<uint32_t>(t), greedy, lambda, lane, flt, top_p)
      : reveal_row<T, kFilter>(lr, K, mask_id, seed, grow, static_cast<uint32_t>(t), greedy, lambda, lane, flt, top_p);
  if (lane == 0) {
    cand_out[row] = r.cand;
    score_out[row] = r.score;
  }
}

// fp32 bits -> key whose unsigned order is the order of the values (negative values reverse, the others move above them)
__device__ __forceinline__ uint32_t f32_order_key(float v) {
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The selection of one utterance by one wave.  x / fm / kn / score point at the utterance's `canvas` (<= 1024) entries; kn may be
// null.  Returns, per lane, bit i set <=> frame lane + 64 i is revealed by this step.  keep_frac = float(cbar[t_next]) (0 on the last
// step): F free rows, `masked` of them masked, keep = min(masked, floor((double) F * (double) keep_frac)), the masked - keep rows that
// come first in the order (score key descending, frame index ascending) are revealed.  The threshold key is the largest c with
// #{key >= c} >= masked - keep, built bit by bit from the top as filter_row builds theta: every count is a popcount of a wave-wide
// compare mask on the scalar unit, wave-uniform by construction.  Ties at the threshold go out in ascending slot, and within a
// slot by the lane prefix count of the ballot.
__device__ __forceinline__ uint32_t reveal_select(const int32_t* __restrict__ x, const uint8_t* __restrict__ fm, const uint8_t* __restrict__ kn,
                                                  const float* __restrict__ score, int canvas, int mask_id, float keep_frac, int lane) {
  uint32_t key[kRevealSlots];      // 0 for a frame that is not a masked free row: below every candidate (>= 1), never counted
  int n_free = 0, n_masked = 0;
#pragma unroll
  for (int i = 0; i < kRevealSlots; ++i) {
    const int f = lane + i * kWave;
    const bool in = f < canvas;
    const bool free_row = in && fm[f] != 0 && !(kn && kn[f] != 0);
    const bool masked = free_row && x[f] == mask_id;
    key[i] = masked ? f32_order_key(score[f]) : 0u;
    n_free += __popcll(__ballot(free_row));
    n_masked += __popcll(__ballot(masked));
  }
  const int quota = static_cast<int>(floor(static_cast<double>(n_free) * static_cast<double>(keep_frac)));
  const int n_reveal = n_masked - (quota < n_masked ? quota : n_masked);
  if (n_reveal <= 0) return 0u;      // wave-uniform
  uint32_t c = 0u;
#pragma unroll 1
  for (uint32_t bit = 0x80000000u; bit; bit >>= 1) {
    const uint32_t cand = c | bit;
    int n = 0;
#pragma unroll
    for (int i = 0; i < kRevealSlots; ++i) n += __popcll(__ballot(key[i] >= cand));
    c = n >= n_reveal ? cand : c;
  }
  int above = 0;
#pragma unroll
  for (int i = 0; i < kRevealSlots; ++i) above += __popcll(__ballot(key[i] > c));
  int ties = n_reveal - above;      // how many of the rows AT the threshold are revealed: the first ones in frame order
  uint32_t sel = 0u;
#pragma unroll
  for (int i = 0; i < kRevealSlots; ++i) {
    const bool tie = key[i] == c && c != 0u;
    const uint64_t bal = __ballot(tie);
    const int before = static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(bal >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(bal), 0u)));
    if (key[i] > c || (tie && before < ties)) sel |= 1u << i;
    ties -= __popcll(bal);      // (negative once the ties are used up: `before < ties` then fails for every lane)
  }
  return sel;
}

// the step form of the commit: one wave per utterance writes the whole utterance.  A revealed row takes its candidate; every other
// row keeps x_t (when x_next is x_t itself nothing is stored for it: known and padded rows are never written).  x_next2: the
// optional trace slot, which receives every row.
__global__ __launch_bounds__(64) void reveal_commit_rows(const int32_t* x_t, int32_t* x_next, int32_t* __restrict__ x_next2,
                                                         const uint8_t* __restrict__ frame_mask, int mask_period, const uint8_t* __restrict__ known,
                                                         const int32_t* __restrict__ cand, const float* __restrict__ score, int canvas, int mask_id,
                                                         float keep_frac) {
  const int lane = threadIdx.x & 63;
  const size_t base = static_cast<size_t>(blockIdx.x) * canvas;
  const uint32_t sel = reveal_select(x_t + base, frame_mask + base % mask_period, known ? known + base : nullptr, score + base, canvas, mask_id, keep_frac,
                                     lane);
  const bool in_place = x_next == x_t;      // kernel-uniform
#pragma unroll
  for (int i = 0; i < kRevealSlots; ++i) {
    const int f = lane + i * kWave;
    if (f >= canvas) continue;
    const bool mine = (sel >> i) & 1u;
    const int id = mine ? cand[base + f] : x_t[base + f];
    if (mine || !in_place) x_next[base + f] = id;
    if (x_next2) x_next2[base + f] = id;
  }
}

// The loop's second launch.  x_next must NOT be x_t: every row wave reads its whole utterance's x_t while the others store their rows.
template <typename T, bool kKnown>
__global__ __launch_bounds__(256) void reveal_commit_prep_rows(
    const int32_t* __restrict__ x_t, int32_t* __restrict__ x_next, int32_t* __restrict__ x_next2, const uint8_t* __restrict__ frame_mask, int mask_period,
    const uint8_t* __restrict__ known, const int32_t* __restrict__ cand, const float* __restrict__ score, int rows, int canvas, int K, int mask_id,
    float keep_frac, int sample_blocks, const T* __restrict__ table, T* __restrict__ xres, float* __restrict__ stats, int d, bool quads, FoldStepPtrs fp,
    const T* __restrict__ film_t, int n_layers, T* __restrict__ Wf, float* __restrict__ s_out, float* __restrict__ b_out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (static_cast<int>(blockIdx.x) >= sample_blocks) {
    const int r = (blockIdx.x - sample_blocks) * 4 + wave;
    if (r < 4 * d * n_layers) fold_layer_row<T>(fp, film_t, 4 * d, d, r, lane, Wf, s_out, b_out);
    return;
  }
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const int b = row / canvas, f = row - b * canvas;
  const size_t base = static_cast<size_t>(b) * canvas;
  const uint8_t* fm = frame_mask + base % mask_period;
  const uint8_t* kn = nullptr;
  if constexpr (kKnown) kn = known + base;
  const uint32_t sel = reveal_select(x_t + base, fm, kn, score + base, canvas, mask_id, keep_frac, lane);
  const uint32_t owner_sel = static_cast<uint32_t>(__shfl(static_cast<int>(sel), f & (kWave - 1), kWave));
  const bool mine = (owner_sel >> (f >> 6)) & 1u;      // wave-uniform: one wave per row
  const int id = __builtin_amdgcn_readfirstlane(mine ? cand[row] : x_t[row]);
  if (lane == 0) {
    x_next[row] = id;
    if (x_next2) x_next2[row] = id;
  }
  embed_row_stats<T>(table, id, fm[f] != 0, xres, row, d, K, stats, quads, lane);
}

}  // namespace

int reveal_candidates(const RevealArgs& a, hipStream_t s) {
  D3PM_REQUIRE(a.n_classes <= kWave * kMaxGroupsPerLane * 4, D3PM_E_SHAPE, "the reveal sampler supports up to %d classes", kWave * kMaxGroupsPerLane * 4);
  const dim3 grid((a.rows + 3) / 4), block(256);
  const RowFilter flt{a.temperature, a.top_k};
#define D3PM_RC_ARGS(T)                                                                                                                          \
  static_cast<const T*>(a.logits), a.ldl, a.x_t, a.frame_mask, a.mask_period, a.known, a.cand, a.score, a.rows, a.n_classes, a.mask_id, a.seed, \
      a.row0, a.t, a.greedy, a.lambda, flt, a.top_p
#define D3PM_RC_ARM(T, kKnown)                                                                                 \
  do {                                                                                                         \
    if (a.filtered()) reveal_candidate_rows<T, kKnown, kNucleusArm><<<grid, block, 0, s>>>(D3PM_RC_ARGS(T));  \
    else reveal_candidate_rows<T, kKnown, 0><<<grid, block, 0, s>>>(D3PM_RC_ARGS(T));                         \
  } while (0)
#define D3PM_RC(T)                    \
  do {                                \
    if (a.known) D3PM_RC_ARM(T, true); \
    else D3PM_RC_ARM(T, false);       \
  } while (0)
  switch (a.logits_dtype) {
    case D3PM_F32: D3PM_RC(float); break;
    case D3PM_F16: D3PM_RC(f16); break;
    case D3PM_BF16: D3PM_RC(bf16); break;
    default: set_error("unknown logits dtype %d", a.logits_dtype); return D3PM_E_ARG;
  }
#undef D3PM_RC
#undef D3PM_RC_ARM
#undef D3PM_RC_ARGS
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

int reveal_commit(const RevealArgs& a, hipStream_t s) {
  D3PM_REQUIRE(a.canvas <= kRevealSlots * kWave, D3PM_E_SHAPE, "the reveal selection supports canvases up to %d frames", kRevealSlots * kWave);
  reveal_commit_rows<<<dim3(a.rows / a.canvas), dim3(kWave), 0, s>>>(a.x_t, a.x_next, a.x_next2, a.frame_mask, a.mask_period, a.known, a.cand, a.score,
                                                                    a.canvas, a.mask_id, a.keep_frac);
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

bool reveal_commit_prep_supported(const RevealArgs& a, const NextIterPrep& n) {
  return a.x_next != a.x_t && a.canvas <= kRevealSlots * kWave && a.logits_dtype == n.dtype && (n.dtype == D3PM_F16 || n.dtype == D3PM_BF16) &&
         n.n_layers <= 16 && n.d % 256 == 0 && (!n.quads || n.d == 512) && n.table && n.x && n.stats && n.blocks && n.film_t && n.Wf;
}

int reveal_commit_prep(const RevealArgs& a, const NextIterPrep& n, hipStream_t s) {
  FoldStepPtrs p{};
  for (int l = 0; l < n.n_layers; ++l) {
    p.W[l] = n.blocks[l].fc1_w; p.bias[l] = n.blocks[l].fc1_b; p.gamma[l] = n.blocks[l].norm3_w; p.beta[l] = n.blocks[l].norm3_b;
  }
  const int sample_blocks = (a.rows + 3) / 4, fold_blocks = (4 * n.d * n.n_layers + 3) / 4;
  const dim3 grid(static_cast<unsigned>(sample_blocks + fold_blocks)), block(256);
#define D3PM_RCP_ARGS(T)                                                                                                                     \
  a.x_t, a.x_next, a.x_next2, a.frame_mask, a.mask_period, a.known, a.cand, a.score, a.rows, a.canvas, a.n_classes, a.mask_id, a.keep_frac, \
      sample_blocks, static_cast<const T*>(n.table), static_cast<T*>(n.x), n.stats, n.d, n.quads, p, static_cast<const T*>(n.film_t), n.n_layers,   \
      static_cast<T*>(n.Wf), n.s_out, n.b_out
#define D3PM_RCP(T)                                                                                \
  do {                                                                                             \
    if (a.known) reveal_commit_prep_rows<T, true><<<grid, block, 0, s>>>(D3PM_RCP_ARGS(T));        \
    else reveal_commit_prep_rows<T, false><<<grid, block, 0, s>>>(D3PM_RCP_ARGS(T));               \
  } while (0)
  if (n.dtype == D3PM_F16) D3PM_RCP(f16); else D3PM_RCP(bf16);
#undef D3PM_RCP
#undef D3PM_RCP_ARGS
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

}  // namespace d3pm
