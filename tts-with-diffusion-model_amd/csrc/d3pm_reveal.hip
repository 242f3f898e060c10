// d3pm_reveal.hip -- confidence-ordered reveal (d3pm_reveal, include/d3pm_hip.h; MaskGIT / SoundStorm decoding on the absorbing
// canvas) and its form under d3pm_revise, where the rows that hold an id compete again for their place (the Token-Critic / remasking
// family).  kRevise, the last template argument of every kernel, tells the two apart; a call without d3pm_revise launches only
// kRevise = false instantiations.  One step is two launches behind the final projection,
//   reveal_candidate_rows     one wave per masked free row: the row's candidate id and its score (d3pm_sample_row.h reveal_from_z).
//                             kRevise: also one wave per held free row (it holds an id j): cand = j, score = logprob_row[_1025] at j
//                             + the bonus + the order noise.  The branch is wave-uniform.
//   reveal_commit_rows        one wave per utterance: the quota of the step, the rows that come first in the order, their ids.
//                             kRevise: the order runs over ALL free rows, and an unselected free row takes mask_id.
//   reveal_commit_prep_rows   the loop's form of the second launch (NextIterPrep, d3pm_kernels.h): one wave per row, which runs its
//                             utterance's selection itself, commits its own row and gathers that row's embedding with its moments;
//                             the workgroups behind the row workgroups rebuild fc1 o norm3 o FiLM of the NEXT timestep.
// kRevise: both commits optionally reset the two grids of d3pm_frame_scores on the rows they re-mask (step = 0, logprob = 0), so that
// the launch behind them (d3pm_logprob.hip) records the row's next reveal.
// No LDS, no atomics, no barrier anywhere in this file.
#include <cmath>
#include <type_traits>

#include "d3pm_kernels.h"
#include "d3pm_fold_rows.h"
#include "d3pm_sample_row.h"
#include "d3pm_logprob_row.h"

namespace d3pm {
namespace {

constexpr int kRevealSlots = 16;      // lane l holds frames l + 64 i, i < 16: canvases up to 1024

// wave-uniform loads of one row's state: scalar branches on them
__device__ __forceinline__ int uniform_byte(const uint8_t* p, size_t i) { return __builtin_amdgcn_readfirstlane(static_cast<int>(p[i])); }

template <typename T, bool kKnown, int kFilter, bool kRevise>
__global__ __launch_bounds__(256) void reveal_candidate_rows(
    const T* __restrict__ logits, int ldl, const int32_t* __restrict__ x_t, const uint8_t* __restrict__ frame_mask, int mask_period,
    const uint8_t* __restrict__ known, int32_t* __restrict__ cand_out, float* __restrict__ score_out, int rows, int K, int mask_id, uint64_t seed,
    uint32_t row0, int t, int greedy, float lambda, RowFilter flt, float top_p, float hold_bonus) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  // a row that is padded, known or (!kRevise) already revealed leaves here: nothing read but its byte(s) and its id, nothing written
  if (uniform_byte(frame_mask, static_cast<size_t>(row) % mask_period) == 0) return;
  if constexpr (kKnown) {
    if (uniform_byte(known, row) != 0) return;
  }
  const int j = __builtin_amdgcn_readfirstlane(x_t[row]);
  if constexpr (!kRevise) {
    if (j != mask_id) return;
  }
  const T* lr = logits + static_cast<size_t>(row) * ldl;
  const uint32_t grow = row0 + static_cast<uint32_t>(row);
  const bool k1025 = K == 1025 && mask_id < 1024;      // kernel-uniform
  RevealRow r;
  if (!kRevise || j == mask_id) {      // wave-uniform: a masked row, the same routine, arguments and noise in both forms
    r = k1025 ? reveal_row_1025<T, kFilter>(lr, mask_id, seed, grow, static_cast<uint32_t>(t), greedy, lambda, lane, flt, top_p)
              : reveal_row<T, kFilter>(lr, K, mask_id, seed, grow, static_cast<uint32_t>(t), greedy, lambda, lane, flt, top_p);
  } else {                             // a held row: the model's own log-probability of its id on this evaluation, no filter
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

struct RevealSel { uint32_t sel, free; };      // per lane, bit i <=> frame lane + 64 i: takes its candidate by this step / is a free row

// The selection of one utterance by one wave.  x / fm / kn / score point at the utterance's `canvas` (<= 1024) entries; kn may be
// null.  keep_frac = float(cbar[t_next]) (0 on the last step); F free rows, quota = floor((double) F * (double) keep_frac).
//   !kRevise: the `masked` masked free rows compete, and masked - min(quota, masked) of them are revealed;
//   kRevise:  all F free rows compete, masked and held alike (x is not read), and F - quota of them hold an id after the step.
// The selected rows are the ones that come first in the order (score key descending -- the fp32 key of d3pm_order_key.h --, frame
// index ascending).  The threshold key is
// the largest c with #{key >= c} >= the number to select, built bit by bit from the top as filter_row builds theta: every count is a
// popcount of a wave-wide compare mask on the scalar unit, wave-uniform by construction.  Ties at the threshold go out in ascending
// slot, and within a slot by the lane prefix count of the ballot.
template <bool kRevise>
__device__ __forceinline__ RevealSel reveal_select(const int32_t* __restrict__ x, const uint8_t* __restrict__ fm, const uint8_t* __restrict__ kn,
                                                   const float* __restrict__ score, int canvas, int mask_id, float keep_frac, int lane) {
  uint32_t key[kRevealSlots];      // 0 for a frame that does not compete: below every candidate (>= 1), never counted
  RevealSel r{0u, 0u};
  int n_free = 0, n_masked = 0;
#pragma unroll
  for (int i = 0; i < kRevealSlots; ++i) {
    const int f = lane + i * kWave;
    const bool free_row = f < canvas && fm[f] != 0 && !(kn && kn[f] != 0);
    bool competes = free_row;
    if constexpr (!kRevise) competes = free_row && x[f] == mask_id;
    key[i] = competes ? order_key<float>(score[f]) : 0u;
    r.free |= free_row ? 1u << i : 0u;
    n_free += __popcll(__ballot(free_row));
    if constexpr (!kRevise) n_masked += __popcll(__ballot(competes));
  }
  const int quota = static_cast<int>(floor(static_cast<double>(n_free) * static_cast<double>(keep_frac)));
  const int n_pick = kRevise ? n_free - quota : n_masked - (quota < n_masked ? quota : n_masked);
  if (n_pick <= 0) return r;      // wave-uniform
  uint32_t c = 0u;
#pragma unroll 1
  for (uint32_t bit = 0x80000000u; bit; bit >>= 1) {
    const uint32_t cand = c | bit;
    int n = 0;
#pragma unroll
    for (int i = 0; i < kRevealSlots; ++i) n += __popcll(__ballot(key[i] >= cand));
    c = n >= n_pick ? cand : c;
  }
  int above = 0;
#pragma unroll
  for (int i = 0; i < kRevealSlots; ++i) above += __popcll(__ballot(key[i] > c));
  int ties = n_pick - above;      // how many of the rows AT the threshold are selected: the first ones in frame order
#pragma unroll
  for (int i = 0; i < kRevealSlots; ++i) {
    const bool tie = key[i] == c && c != 0u;
    const uint64_t bal = __ballot(tie);
    const int before = static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(bal >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(bal), 0u)));
    if (key[i] > c || (tie && before < ties)) r.sel |= 1u << i;
    ties -= __popcll(bal);      // (negative once the ties are used up: `before < ties` then fails for every lane)
  }
  return r;
}

// the step form of the commit: one wave per utterance writes the whole utterance.  A selected row takes its candidate (kRevise: a
// held row's is its own id), an unselected free row takes mask_id under kRevise, and every other row keeps x_t.  When x_next is x_t
// itself only revealed (kRevise: changed) rows are stored: known and padded rows are never written.  x_next2: the optional trace
// slot, which receives every row.  logprob / step (kRevise): the optional grids of d3pm_frame_scores, reset on the rows this launch
// re-masks.
template <bool kRevise>
__global__ __launch_bounds__(64) void reveal_commit_rows(const int32_t* x_t, int32_t* x_next, int32_t* __restrict__ x_next2,
                                                         const uint8_t* __restrict__ frame_mask, int mask_period, const uint8_t* __restrict__ known,
                                                         const int32_t* __restrict__ cand, const float* __restrict__ score, int canvas, int mask_id,
                                                         float keep_frac, float* __restrict__ logprob, int32_t* __restrict__ step) {
  const int lane = threadIdx.x & 63;
  const size_t base = static_cast<size_t>(blockIdx.x) * canvas;
  const RevealSel r = reveal_select<kRevise>(x_t + base, frame_mask + base % mask_period, known ? known + base : nullptr, score + base, canvas, mask_id,
                                             keep_frac, lane);
  const bool in_place = x_next == x_t;      // kernel-uniform
#pragma unroll
  for (int i = 0; i < kRevealSlots; ++i) {
    const int f = lane + i * kWave;
    if (f >= canvas) continue;
    const bool mine = (r.sel >> i) & 1u;
    if constexpr (kRevise) {
      const bool free_row = (r.free >> i) & 1u;
      const int cur = x_t[base + f];
      const int id = free_row ? (mine ? cand[base + f] : mask_id) : cur;
      if (id != cur || !in_place) x_next[base + f] = id;
      if (x_next2) x_next2[base + f] = id;
      if (step && free_row && !mine && cur != mask_id) {
        step[base + f] = 0;
        logprob[base + f] = 0.0f;
      }
    } else {
      const int id = mine ? cand[base + f] : x_t[base + f];
      if (mine || !in_place) x_next[base + f] = id;
      if (x_next2) x_next2[base + f] = id;
    }
  }
}

// The loop's second launch.  x_next must NOT be x_t: every row wave reads its whole utterance's state while the others store their rows.
template <typename T, bool kKnown, bool kRevise>
__global__ __launch_bounds__(256) void reveal_commit_prep_rows(
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
  const RevealSel r = reveal_select<kRevise>(x_t + base, fm, kn, score + base, canvas, mask_id, keep_frac, lane);
  const int owner = f & (kWave - 1), slot = f >> 6;
  const bool mine = (static_cast<uint32_t>(__shfl(static_cast<int>(r.sel), owner, kWave)) >> slot) & 1u;      // wave-uniform: one wave per row
  int id;
  if constexpr (kRevise) {
    const bool free_row = (static_cast<uint32_t>(__shfl(static_cast<int>(r.free), owner, kWave)) >> slot) & 1u;
    const int cur = __builtin_amdgcn_readfirstlane(x_t[row]);
    id = free_row ? (mine ? __builtin_amdgcn_readfirstlane(cand[row]) : mask_id) : cur;
    if (lane == 0 && step && free_row && !mine && cur != mask_id) {
      step[row] = 0;
      logprob[row] = 0.0f;
    }
  } else {
    id = __builtin_amdgcn_readfirstlane(mine ? cand[row] : x_t[row]);
  }
  if (lane == 0) {
    x_next[row] = id;
    if (x_next2) x_next2[row] = id;
  }
  embed_row_stats<T>(table, id, fm[f] != 0, xres, row, d, K, stats, quads, lane);
}

// f(std::bool_constant<b>{}): a run-time flag becomes a template argument, each instantiation named once where f launches
template <typename F>
void with_flag(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

template <typename T>
void launch_candidates(const RevealArgs& a, hipStream_t s) {
  const dim3 grid((a.rows + 3) / 4), block(256);
  const RowFilter flt{a.temperature, a.top_k};
  with_flag(a.known != nullptr, [&](auto kn) {
    with_flag(a.filtered(), [&](auto fl) {
      with_flag(a.revise, [&](auto rv) {
        reveal_candidate_rows<T, decltype(kn)::value, decltype(fl)::value ? kNucleusArm : 0, decltype(rv)::value><<<grid, block, 0, s>>>(
            static_cast<const T*>(a.logits), a.ldl, a.x_t, a.frame_mask, a.mask_period, a.known, a.cand, a.score, a.rows, a.n_classes, a.mask_id, a.seed,
            a.row0, a.t, a.greedy, a.lambda, flt, a.top_p, a.hold_bonus);
      });
    });
  });
}

template <typename T>
void launch_commit_prep(const RevealArgs& a, const NextIterPrep& n, hipStream_t s) {
  FoldStepPtrs p{};
  for (int l = 0; l < n.n_layers; ++l) {
    p.W[l] = n.blocks[l].fc1_w; p.bias[l] = n.blocks[l].fc1_b; p.gamma[l] = n.blocks[l].norm3_w; p.beta[l] = n.blocks[l].norm3_b;
  }
  const int sample_blocks = (a.rows + 3) / 4, fold_blocks = (4 * n.d * n.n_layers + 3) / 4;
  const dim3 grid(static_cast<unsigned>(sample_blocks + fold_blocks)), block(256);
  with_flag(a.known != nullptr, [&](auto kn) {
    with_flag(a.revise, [&](auto rv) {
      reveal_commit_prep_rows<T, decltype(kn)::value, decltype(rv)::value><<<grid, block, 0, s>>>(
          a.x_t, a.x_next, a.x_next2, a.frame_mask, a.mask_period, a.known, a.cand, a.score, a.rows, a.canvas, a.n_classes, a.mask_id, a.keep_frac,
          a.logprob, a.step, sample_blocks, static_cast<const T*>(n.table), static_cast<T*>(n.x), n.stats, n.d, n.quads, p,
          static_cast<const T*>(n.film_t), n.n_layers, static_cast<T*>(n.Wf), n.s_out, n.b_out);
    });
  });
}

}  // namespace

int reveal_candidates(const RevealArgs& a, hipStream_t s) {
  D3PM_REQUIRE(a.n_classes <= kWave * kMaxGroupsPerLane * 4, D3PM_E_SHAPE, "the %s supports up to %d classes", a.revise ? "revise step" : "reveal sampler",
               kWave * kMaxGroupsPerLane * 4);
  switch (a.logits_dtype) {
    case D3PM_F32: launch_candidates<float>(a, s); break;
    case D3PM_F16: launch_candidates<f16>(a, s); break;
    case D3PM_BF16: launch_candidates<bf16>(a, s); break;
    default: set_error("unknown logits dtype %d", a.logits_dtype); return D3PM_E_ARG;
  }
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

int reveal_commit(const RevealArgs& a, hipStream_t s) {
  D3PM_REQUIRE(a.canvas <= kRevealSlots * kWave, D3PM_E_SHAPE, "the %s selection supports canvases up to %d frames", a.revise ? "revise" : "reveal",
               kRevealSlots * kWave);
  with_flag(a.revise, [&](auto rv) {
    reveal_commit_rows<decltype(rv)::value><<<dim3(a.rows / a.canvas), dim3(kWave), 0, s>>>(
        a.x_t, a.x_next, a.x_next2, a.frame_mask, a.mask_period, a.known, a.cand, a.score, a.canvas, a.mask_id, a.keep_frac, a.logprob, a.step);
  });
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

bool reveal_commit_prep_supported(const RevealArgs& a, const NextIterPrep& n) {
  return a.x_next != a.x_t && a.canvas <= kRevealSlots * kWave && a.logits_dtype == n.dtype && (n.dtype == D3PM_F16 || n.dtype == D3PM_BF16) &&
         n.n_layers <= 16 && n.d % 256 == 0 && (!n.quads || n.d == 512) && n.table && n.x && n.stats && n.blocks && n.film_t && n.Wf;
}

int reveal_commit_prep(const RevealArgs& a, const NextIterPrep& n, hipStream_t s) {
  if (n.dtype == D3PM_F16) launch_commit_prep<f16>(a, n, s);
  else launch_commit_prep<bf16>(a, n, s);
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

}  // namespace d3pm
