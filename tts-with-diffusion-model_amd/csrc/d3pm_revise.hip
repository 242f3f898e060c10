// d3pm_revise.hip -- the reveal step whose held rows compete again for their place (d3pm_revise, include/d3pm_hip.h; the Token-Critic /
// remasking family of decoders on the absorbing canvas).  Kernels of their own: a call without d3pm_revise runs none of this file, and
// d3pm_reveal.hip knows nothing of it.  One step is two launches behind the final projection,
//   revise_candidate_rows     one wave per FREE row.  A masked row goes through reveal_row[_1025] with the arguments and the noise of
//                             reveal_candidate_rows; a held row (it holds an id j) through logprob_row[_1025] at j, the bonus and the
//                             order noise.  The branch is wave-uniform.
//   revise_commit_rows        one wave per utterance: hold = F - floor(F cbar[t_next]) free rows hold an id after the step, the ones
//                             that come first in the order among ALL free rows; an unselected held row takes mask_id.
//   revise_commit_prep_rows   the loop's form of the second launch (NextIterPrep): one wave per row, which runs its utterance's
//                             selection itself, commits its own row and gathers that row's embedding with its moments; the workgroups
//                             behind the row workgroups rebuild fc1 o norm3 o FiLM of the NEXT timestep.
// Both commits optionally reset the two grids of d3pm_frame_scores on the rows they re-mask (step = 0, logprob = 0), so that the
// launch behind them (d3pm_logprob.hip, unchanged) records the row's next reveal.
// No LDS, no atomics, no barrier anywhere in this file.
#include <cmath>

#include "d3pm_kernels.h"
#include "d3pm_fold_rows.h"
#include "d3pm_sample_row.h"
#include "d3pm_logprob_row.h"

namespace d3pm {
namespace {

constexpr int kReviseSlots = 16;      // lane l holds frames l + 64 i, i < 16: canvases up to 1024

// wave-uniform load of one row's byte: scalar branches on it
__device__ __forceinline__ int row_byte(const uint8_t* p, size_t i) { return __builtin_amdgcn_readfirstlane(static_cast<int>(p[i])); }

template <typename T, bool kKnown, int kFilter>
__global__ __launch_bounds__(256) void revise_candidate_rows(
    const T* __restrict__ logits, int ldl, const int32_t* __restrict__ x_t, const uint8_t* __restrict__ frame_mask, int mask_period,
    const uint8_t* __restrict__ known, int32_t* __restrict__ cand_out, float* __restrict__ score_out, int rows, int K, int mask_id, uint64_t seed,
    uint32_t row0, int t, int greedy, float lambda, RowFilter flt, float top_p, float hold_bonus) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  // a row that is padded or known leaves here: nothing read but its byte(s), nothing written
  if (row_byte(frame_mask, static_cast<size_t>(row) % mask_period) == 0) return;
  if constexpr (kKnown) {
    if (row_byte(known, row) != 0) return;
  }
  const int j = __builtin_amdgcn_readfirstlane(x_t[row]);
  const T* lr = logits + static_cast<size_t>(row) * ldl;
  const uint32_t grow = row0 + static_cast<uint32_t>(row);
  const bool k1025 = K == 1025 && mask_id < 1024;      // kernel-uniform
  RevealRow r;
  if (j == mask_id) {      // wave-uniform: the masked row of d3pm_reveal, same routine, arguments and noise
    r = k1025 ? reveal_row_1025<T, kFilter>(lr, mask_id, seed, grow, static_cast<uint32_t>(t), greedy, lambda, lane, flt, top_p)
              : reveal_row<T, kFilter>(lr, K, mask_id, seed, grow, static_cast<uint32_t>(t), greedy, lambda, lane, flt, top_p);
  } else {                 // a held row: the model's own log-probability of its id on this evaluation, no filter
    const float lp = k1025 ? logprob_row_1025<T>(lr, mask_id, j, lane) : logprob_row<T>(lr, K, mask_id, j, lane);
    r.cand = j;
    r.score = lp + hold_bonus;
    if (lambda != 0.f && !greedy) {      // kernel-uniform: the statement that turns a masked row's conf into its score
      float v[4];
      noise4(seed, 0u, grow, static_cast<uint32_t>(t), kStreamRevealChoice, v);
      r.score = r.score + lambda * gumbel(v[0]);
    }
  }
  if (lane == 0) {
    cand_out[row] = r.cand;
    score_out[row] = r.score;
  }
}

// fp32 bits -> key whose unsigned order is the order of the values (negative values reverse, the others move above them)
__device__ __forceinline__ uint32_t order_key(float v) {
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct ReviseSel { uint32_t sel, free; };      // per lane, bit i <=> frame lane + 64 i: holds an id after the step / is a free row

// The selection of one utterance by one wave.  x / fm / kn / score point at the utterance's `canvas` (<= 1024) entries; kn may be
// null.  keep_frac = float(cbar[t_next]) (0 on the last step): F free rows, hold = F - floor((double) F * (double) keep_frac) of them
// hold an id after the step -- the ones that come first in the order (score key descending, frame index ascending) among all free
// rows, masked and held alike.  The threshold key is the largest c with #{key >= c} >= hold, built bit by bit from the top; every
// count is a popcount of a wave-wide compare mask on the scalar unit, wave-uniform by construction.  Ties at the threshold go out in
// ascending slot, and within a slot by the lane prefix count of the ballot.
__device__ __forceinline__ ReviseSel revise_select(const uint8_t* __restrict__ fm, const uint8_t* __restrict__ kn, const float* __restrict__ score,
                                                   int canvas, float keep_frac, int lane) {
  uint32_t key[kReviseSlots];      // 0 for a frame that is not a free row: below every candidate (>= 1), never counted
  ReviseSel r{0u, 0u};
  int n_free = 0;
#pragma unroll
  for (int i = 0; i < kReviseSlots; ++i) {
    const int f = lane + i * kWave;
    const bool free_row = f < canvas && fm[f] != 0 && !(kn && kn[f] != 0);
    key[i] = free_row ? order_key(score[f]) : 0u;
    r.free |= free_row ? 1u << i : 0u;
    n_free += __popcll(__ballot(free_row));
  }
  const int n_hold = n_free - static_cast<int>(floor(static_cast<double>(n_free) * static_cast<double>(keep_frac)));
  if (n_hold <= 0) return r;      // wave-uniform
  uint32_t c = 0u;
#pragma unroll 1
  for (uint32_t bit = 0x80000000u; bit; bit >>= 1) {
    const uint32_t cand = c | bit;
    int n = 0;
#pragma unroll
    for (int i = 0; i < kReviseSlots; ++i) n += __popcll(__ballot(key[i] >= cand));
    c = n >= n_hold ? cand : c;
  }
  int above = 0;
#pragma unroll
  for (int i = 0; i < kReviseSlots; ++i) above += __popcll(__ballot(key[i] > c));
  int ties = n_hold - above;      // how many of the rows AT the threshold are selected: the first ones in frame order
#pragma unroll
  for (int i = 0; i < kReviseSlots; ++i) {
    const bool tie = key[i] == c && c != 0u;
    const uint64_t bal = __ballot(tie);
    const int before = static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(bal >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(bal), 0u)));
    if (key[i] > c || (tie && before < ties)) r.sel |= 1u << i;
    ties -= __popcll(bal);      // (negative once the ties are used up: `before < ties` then fails for every lane)
  }
  return r;
}

// the step form of the commit: one wave per utterance writes the whole utterance.  A free row takes its candidate (a held row's is its
// own id) when selected and mask_id when not; every other row keeps x_t.  When x_next is x_t itself only changed rows are stored:
// known and padded rows are never written.  x_next2: the optional trace slot, which receives every row.  logprob / step: the optional
// grids of d3pm_frame_scores, reset on the rows this launch re-masks.
__global__ __launch_bounds__(64) void revise_commit_rows(const int32_t* x_t, int32_t* x_next, int32_t* __restrict__ x_next2,
                                                         const uint8_t* __restrict__ frame_mask, int mask_period, const uint8_t* __restrict__ known,
                                                         const int32_t* __restrict__ cand, const float* __restrict__ score, int canvas, int mask_id,
                                                         float keep_frac, float* __restrict__ logprob, int32_t* __restrict__ step) {
  const int lane = threadIdx.x & 63;
  const size_t base = static_cast<size_t>(blockIdx.x) * canvas;
  const ReviseSel r = revise_select(frame_mask + base % mask_period, known ? known + base : nullptr, score + base, canvas, keep_frac, lane);
  const bool in_place = x_next == x_t;      // kernel-uniform
#pragma unroll
  for (int i = 0; i < kReviseSlots; ++i) {
    const int f = lane + i * kWave;
    if (f >= canvas) continue;
    const bool free_row = (r.free >> i) & 1u, mine = (r.sel >> i) & 1u;
    const int cur = x_t[base + f];
    const int id = free_row ? (mine ? cand[base + f] : mask_id) : cur;
    if (id != cur || !in_place) x_next[base + f] = id;
    if (x_next2) x_next2[base + f] = id;
    if (step && free_row && !mine && cur != mask_id) {
      step[base + f] = 0;
      logprob[base + f] = 0.0f;
    }
  }
}

// The loop's second launch.  x_next must NOT be x_t: every row wave reads its whole utterance's state while the others store their rows.
template <typename T, bool kKnown>
__global__ __launch_bounds__(256) void revise_commit_prep_rows(
    const int32_t* __restrict__ x_t, int32_t* __restrict__ x_next, int32_t* __restrict__ x_next2, const uint8_t* __restrict__ frame_mask, int mask_period,
    const uint8_t* __restrict__ known, const int32_t* __restrict__ cand, const float* __restrict__ score, int rows, int canvas, int K, int mask_id,
    float keep_frac, float* __restrict__ logprob, int32_t* __restrict__ step, int sample_blocks, const T* __restrict__ table, T* __restrict__ xres,
    float* __restrict__ stats, int d, bool quads, FoldStepPtrs fp, const T* __restrict__ film_t, int n_layers, T* __restrict__ Wf,
    float* __restrict__ s_out, float* __restrict__ b_out) {
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
  const ReviseSel r = revise_select(fm, kn, score + base, canvas, keep_frac, lane);
  const int owner = f & (kWave - 1), slot = f >> 6;
  const bool mine = (static_cast<uint32_t>(__shfl(static_cast<int>(r.sel), owner, kWave)) >> slot) & 1u;           // wave-uniform: one wave per row
  const bool free_row = (static_cast<uint32_t>(__shfl(static_cast<int>(r.free), owner, kWave)) >> slot) & 1u;
  const int cur = __builtin_amdgcn_readfirstlane(x_t[row]);
  const int id = free_row ? (mine ? __builtin_amdgcn_readfirstlane(cand[row]) : mask_id) : cur;
  if (lane == 0) {
    x_next[row] = id;
    if (x_next2) x_next2[row] = id;
    if (step && free_row && !mine && cur != mask_id) {
      step[row] = 0;
      logprob[row] = 0.0f;
    }
  }
  embed_row_stats<T>(table, id, fm[f] != 0, xres, row, d, K, stats, quads, lane);
}

}  // namespace

int revise_candidates(const ReviseArgs& v, hipStream_t s) {
  const RevealArgs& a = v.r;
  D3PM_REQUIRE(a.n_classes <= kWave * kMaxGroupsPerLane * 4, D3PM_E_SHAPE, "the revise step supports up to %d classes", kWave * kMaxGroupsPerLane * 4);
  const dim3 grid((a.rows + 3) / 4), block(256);
  const RowFilter flt{a.temperature, a.top_k};
#define D3PM_VC_ARGS(T)                                                                                                                          \
  static_cast<const T*>(a.logits), a.ldl, a.x_t, a.frame_mask, a.mask_period, a.known, a.cand, a.score, a.rows, a.n_classes, a.mask_id, a.seed, \
      a.row0, a.t, a.greedy, a.lambda, flt, a.top_p, v.hold_bonus
#define D3PM_VC_ARM(T, kKnown)                                                                                 \
  do {                                                                                                         \
    if (a.filtered()) revise_candidate_rows<T, kKnown, kNucleusArm><<<grid, block, 0, s>>>(D3PM_VC_ARGS(T));  \
    else revise_candidate_rows<T, kKnown, 0><<<grid, block, 0, s>>>(D3PM_VC_ARGS(T));                         \
  } while (0)
#define D3PM_VC(T)                     \
  do {                                 \
    if (a.known) D3PM_VC_ARM(T, true); \
    else D3PM_VC_ARM(T, false);        \
  } while (0)
  switch (a.logits_dtype) {
    case D3PM_F32: D3PM_VC(float); break;
    case D3PM_F16: D3PM_VC(f16); break;
    case D3PM_BF16: D3PM_VC(bf16); break;
    default: set_error("unknown logits dtype %d", a.logits_dtype); return D3PM_E_ARG;
  }
#undef D3PM_VC
#undef D3PM_VC_ARM
#undef D3PM_VC_ARGS
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

int revise_commit(const ReviseArgs& v, hipStream_t s) {
  const RevealArgs& a = v.r;
  D3PM_REQUIRE(a.canvas <= kReviseSlots * kWave, D3PM_E_SHAPE, "the revise selection supports canvases up to %d frames", kReviseSlots * kWave);
  revise_commit_rows<<<dim3(a.rows / a.canvas), dim3(kWave), 0, s>>>(a.x_t, a.x_next, a.x_next2, a.frame_mask, a.mask_period, a.known, a.cand, a.score,
                                                                    a.canvas, a.mask_id, a.keep_frac, v.logprob, v.step);
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

// applies wherever reveal_commit_prep_supported(v.r, n) holds
int revise_commit_prep(const ReviseArgs& v, const NextIterPrep& n, hipStream_t s) {
  const RevealArgs& a = v.r;
  FoldStepPtrs p{};
  for (int l = 0; l < n.n_layers; ++l) {
    p.W[l] = n.blocks[l].fc1_w; p.bias[l] = n.blocks[l].fc1_b; p.gamma[l] = n.blocks[l].norm3_w; p.beta[l] = n.blocks[l].norm3_b;
  }
  const int sample_blocks = (a.rows + 3) / 4, fold_blocks = (4 * n.d * n.n_layers + 3) / 4;
  const dim3 grid(static_cast<unsigned>(sample_blocks + fold_blocks)), block(256);
#define D3PM_VCP_ARGS(T)                                                                                                                     \
  a.x_t, a.x_next, a.x_next2, a.frame_mask, a.mask_period, a.known, a.cand, a.score, a.rows, a.canvas, a.n_classes, a.mask_id, a.keep_frac, \
      v.logprob, v.step, sample_blocks, static_cast<const T*>(n.table), static_cast<T*>(n.x), n.stats, n.d, n.quads, p,                     \
      static_cast<const T*>(n.film_t), n.n_layers, static_cast<T*>(n.Wf), n.s_out, n.b_out
#define D3PM_VCP(T)                                                                                \
  do {                                                                                             \
    if (a.known) revise_commit_prep_rows<T, true><<<grid, block, 0, s>>>(D3PM_VCP_ARGS(T));        \
    else revise_commit_prep_rows<T, false><<<grid, block, 0, s>>>(D3PM_VCP_ARGS(T));               \
  } while (0)
  if (n.dtype == D3PM_F16) D3PM_VCP(f16); else D3PM_VCP(bf16);
#undef D3PM_VCP
#undef D3PM_VCP_ARGS
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

}  // namespace d3pm
