// d3pm_sample.hip -- D3PM absorbing-state transition / posterior / categorical sampling kernels.
//
// Replaces (paths under /root/reference/vall_e/vall_e/):
//   posterior_sample_rows  AR.p_sample + q_posterior_logits + _at + _at_onehot (ar_discrete.py:337-420)
//   q_sample_rows          AR.q_sample + q_probs                               (ar_discrete.py:467-502)
//   uniform_rows           the torch.rand draws at ar_discrete.py:402,480 (Philox stream instead)
//
// The reference multiplies one-hot / softmax rows into dense [1025,1025] fp16 tables; every table
// is d*I + c*1 e_M^T with row M = e_M (proven on the reference's tables in
// tests/golden/make_golden.py), so per row the work is O(K):
//     fact1_j = d_t [j==x] (x != M)      |  c_t (j != M), 1 (j == M)        (x == M)
//     fact2_j = rn16(p_j * dbar_{t-1}) (j != M),  rn16(cbar_{t-1} * sum_{k!=M} p_k + p_M) (j == M)
//     out_j   = rn16(log16(rn16(fact1_j+eps)) + log16(rn16(fact2_j+eps)))
//     x_{t-1} = argmax_j fp32(out_j) + gumbel(u_j)
// with p = rn16(softmax_fp32(rn16 logits)).  All fp16 rounding points of the eager fp16 model are
// kept; HBM traffic per row is the K logits in and one id out (plus 4 B of x_t).
//
// Mapping: one wave per row; lane l owns class groups g = l, l+64, .. (4 consecutive classes per
// Philox call), i.e. 5 groups x 4 classes = 20 registers of logits for K = 1025.
#include <cmath>

#include "d3pm_kernels.h"
#include "d3pm_fold_rows.h"
#include "d3pm_sample_row.h"

namespace d3pm {
namespace {

// Is this wave's frame row given by the caller (the known-frame map of d3pm_canvas, uint8 [batch][canvas])?  One byte load per wave,
// broadcast through readfirstlane so that the branch on it is a scalar one: a known row skips the whole draw.
__device__ __forceinline__ bool row_is_known(const uint8_t* __restrict__ known, int frow) {
  return __builtin_amdgcn_readfirstlane(static_cast<int>(known[frow])) != 0;
}

// kKnown (replacement conditioning): a row whose frame is marked in `known` keeps x_t[row] -- no logits read, no
// Philox draw (the noise of every other row is keyed by its own global row and does not move) -- and takes the same stores.
// kKnown = false is the kernel without the map: `known` is never read.
// kFilter (temperature / top-k, d3pm_sample_row.h): a compile-time arm like kKnown.  The kernels without it keep their names, their
// arguments and their code; the *_filtered kernels below carry the two numbers as one more argument.  kFilter == kNucleusArm
// (top-p behind them, d3pm_nucleus) is a third arm with kernels of its own (nucleus_sample_*), so that a call without top_p launches
// the kernels it launched before there was one; `theta_out` [rows] is that arm's optional output (a known row: NaN).
template <typename T, bool kKnown, int kFilter>
__device__ __forceinline__ void posterior_sample_rows_body(
    const T* __restrict__ logits, int ldl, const int32_t* x_t, int32_t* x_next,
    int32_t* x_next2, uint16_t* __restrict__ post_out, int rows, int K, int mask_id,
    uint64_t seed, const uint64_t* __restrict__ seed_hbm, uint32_t row0, int greedy, const PosteriorConsts& pc, int n_q,
    const uint8_t* __restrict__ known, const RowFilter& flt, const RowNucleus& nuc = RowNucleus{}) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + wave;
  if (row >= rows) return;
  if constexpr (kKnown) {
    if (row_is_known(known, n_q > 1 ? row / n_q : row)) {      // wave-uniform: one wave per row
      if (lane == 0) {
        const int keep = x_t[row];
        x_next[row] = keep;
        if (x_next2) x_next2[row] = keep;
        if constexpr (kFilter == kNucleusArm)
          if (nuc.theta_out) nuc.theta_out[row] = __builtin_nanf("");
      }
      return;
    }
  }
  const RowNucleus row_nuc{nuc.top_p, nuc.theta_out ? nuc.theta_out + row : nullptr};      // (never read outside the nucleus arm)
  if (seed_hbm) seed = *seed_hbm;
  // n_q > 1 (d3pm_shape.n_q): row = frame row * n_q + level; the level-0 token of a frame draws the noise the level-0-only
  // path draws, level l > 0 draws from Philox stream 16 + l at the same (frame row, t)
  const int frow = n_q > 1 ? row / n_q : row, level = row - frow * (n_q > 1 ? n_q : 1);
  const uint32_t strm = level ? 16u + static_cast<uint32_t>(level) : 0u;
  int best_j;
  if (K == 1025 && mask_id < 1024 && !post_out)        // kernel-uniform: the predicate-free routine for the reference's class count (same bits)
    best_j = sample_row_1025<T, kFilter>(logits + static_cast<size_t>(row) * ldl, mask_id, x_t[row], seed, row0 + static_cast<uint32_t>(frow), greedy, pc, lane, strm,
                                         D3PM_SAMPLER_EARLY_OUT != 0, flt, row_nuc);
  else
    best_j = sample_row<T, kFilter>(logits + static_cast<size_t>(row) * ldl, K, mask_id, x_t[row], seed, row0 + static_cast<uint32_t>(frow), greedy, pc,
                                    post_out ? post_out + static_cast<size_t>(row) * K : nullptr, lane, strm, flt, row_nuc);
  if (lane == 0) {
    x_next[row] = best_j;
    if (x_next2) x_next2[row] = best_j;
  }
}

template <typename T, bool kKnown>
__global__ __launch_bounds__(256) void posterior_sample_rows(
    const T* __restrict__ logits, int ldl, const int32_t* x_t, int32_t* x_next,
    int32_t* x_next2, uint16_t* __restrict__ post_out, int rows, int K, int mask_id,
    uint64_t seed, const uint64_t* __restrict__ seed_hbm, uint32_t row0, int greedy, PosteriorConsts pc, int n_q,
    const uint8_t* __restrict__ known) {
  posterior_sample_rows_body<T, kKnown, 0>(logits, ldl, x_t, x_next, x_next2, post_out, rows, K, mask_id, seed, seed_hbm, row0, greedy, pc, n_q,
                                               known, RowFilter{});
}

template <typename T, bool kKnown>
__global__ __launch_bounds__(256) void posterior_sample_rows_filtered(
    const T* __restrict__ logits, int ldl, const int32_t* x_t, int32_t* x_next,
    int32_t* x_next2, uint16_t* __restrict__ post_out, int rows, int K, int mask_id,
    uint64_t seed, const uint64_t* __restrict__ seed_hbm, uint32_t row0, int greedy, PosteriorConsts pc, int n_q,
    const uint8_t* __restrict__ known, RowFilter flt) {
  posterior_sample_rows_body<T, kKnown, kFilterArm>(logits, ldl, x_t, x_next, x_next2, post_out, rows, K, mask_id, seed, seed_hbm, row0, greedy, pc,
                                                    n_q, known, flt);
}

template <typename T, bool kKnown>
__global__ __launch_bounds__(256) void nucleus_sample_rows(
    const T* __restrict__ logits, int ldl, const int32_t* x_t, int32_t* x_next,
    int32_t* x_next2, uint16_t* __restrict__ post_out, int rows, int K, int mask_id,
    uint64_t seed, const uint64_t* __restrict__ seed_hbm, uint32_t row0, int greedy, PosteriorConsts pc, int n_q,
    const uint8_t* __restrict__ known, RowFilter flt, RowNucleus nuc) {
  posterior_sample_rows_body<T, kKnown, kNucleusArm>(logits, ldl, x_t, x_next, x_next2, post_out, rows, K, mask_id, seed, seed_hbm, row0, greedy, pc,
                                                     n_q, known, flt, nuc);
}

// The sampler of iteration t and the preparation of iteration t - 1 in one launch (NextIterPrep, d3pm_kernels.h): workgroups
// [0, sample_blocks) draw x_{t-1} for four rows each and at once gather those rows' embeddings into the residual stream with
// their moments (the id is in every lane after the wave argmax); the workgroups behind them rebuild fc1 o norm3 o FiLM(t - 1) of
// every block.  The two halves are independent (one VALU-bound, one a 24-MB stream), so the launch costs the longer of them: at one
// utterance 12.4 + 8.7 + 5.0 us of launches become ~13, at 32 utterances 94 + 10.8 + 10.5 become ~97.
// kKnown as in posterior_sample_rows: a known row takes best_j = x_t[row] and goes through the same stores and the same gather, so
// the next iteration's residual row and moments are written exactly as for a drawn id.
template <typename T, bool kKnown, int kFilter>
__device__ __forceinline__ void posterior_sample_prep_rows_body(
    const T* __restrict__ logits, int ldl, const int32_t* x_t, int32_t* x_next, int32_t* x_next2, int rows, int K, int mask_id,
    uint64_t seed, const uint64_t* __restrict__ seed_hbm, uint32_t row0, int greedy, const PosteriorConsts& pc, int mask_period, int sample_blocks,
    const T* __restrict__ table, T* __restrict__ xres, float* __restrict__ stats, const uint8_t* __restrict__ frame_mask, int d,
    bool quads, const FoldStepPtrs& fp, const T* __restrict__ film_t, int n_layers, T* __restrict__ Wf, float* __restrict__ s_out, float* __restrict__ b_out,
    const uint8_t* __restrict__ known, const T* __restrict__ qkv_table, T* __restrict__ q0, T* __restrict__ kv0, const RowFilter& flt,
    const RowNucleus& nuc = RowNucleus{}) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (static_cast<int>(blockIdx.x) >= sample_blocks) {
    const int r = (blockIdx.x - sample_blocks) * 4 + wave;
    if (r < 4 * d * n_layers) fold_layer_row<T>(fp, film_t, 4 * d, d, r, lane, Wf, s_out, b_out);
    return;
  }
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  if (seed_hbm) seed = *seed_hbm;
  int best_j;
  bool keep = false;
  if constexpr (kKnown) keep = row_is_known(known, row);      // wave-uniform: one wave per row
  if (keep)
    best_j = x_t[row];
  else
    best_j = (K == 1025 && mask_id < 1024)
        ? sample_row_1025<T, kFilter>(logits + static_cast<size_t>(row) * ldl, mask_id, x_t[row], seed, row0 + static_cast<uint32_t>(row), greedy, pc, lane, 0u,
                                      D3PM_SAMPLER_EARLY_OUT != 0, flt, nuc)
        : sample_row<T, kFilter>(logits + static_cast<size_t>(row) * ldl, K, mask_id, x_t[row], seed, row0 + static_cast<uint32_t>(row), greedy, pc, nullptr, lane, 0u, flt,
                                 nuc);
  if (lane == 0) {
    x_next[row] = best_j;
    if (x_next2) x_next2[row] = best_j;
  }
  embed_row_stats<T>(table, best_j, frame_mask[row % mask_period] != 0, xres, row, d, K, stats, quads, lane, qkv_table, q0, kv0);
}

template <typename T, bool kKnown>
__global__ __launch_bounds__(256) void posterior_sample_prep_rows(
    const T* __restrict__ logits, int ldl, const int32_t* x_t, int32_t* x_next, int32_t* x_next2, int rows, int K, int mask_id,
    uint64_t seed, const uint64_t* __restrict__ seed_hbm, uint32_t row0, int greedy, PosteriorConsts pc, int mask_period, int sample_blocks,
    const T* __restrict__ table, T* __restrict__ xres, float* __restrict__ stats, const uint8_t* __restrict__ frame_mask, int d,
    bool quads, FoldStepPtrs fp, const T* __restrict__ film_t, int n_layers, T* __restrict__ Wf, float* __restrict__ s_out, float* __restrict__ b_out,
    const uint8_t* __restrict__ known, const T* __restrict__ qkv_table, T* __restrict__ q0, T* __restrict__ kv0) {
  posterior_sample_prep_rows_body<T, kKnown, 0>(logits, ldl, x_t, x_next, x_next2, rows, K, mask_id, seed, seed_hbm, row0, greedy, pc, mask_period,
                                                    sample_blocks, table, xres, stats, frame_mask, d, quads, fp, film_t, n_layers, Wf, s_out, b_out, known,
                                                    qkv_table, q0, kv0, RowFilter{});
}

template <typename T, bool kKnown>
__global__ __launch_bounds__(256) void posterior_sample_prep_rows_filtered(
    const T* __restrict__ logits, int ldl, const int32_t* x_t, int32_t* x_next, int32_t* x_next2, int rows, int K, int mask_id,
    uint64_t seed, const uint64_t* __restrict__ seed_hbm, uint32_t row0, int greedy, PosteriorConsts pc, int mask_period, int sample_blocks,
    const T* __restrict__ table, T* __restrict__ xres, float* __restrict__ stats, const uint8_t* __restrict__ frame_mask, int d,
    bool quads, FoldStepPtrs fp, const T* __restrict__ film_t, int n_layers, T* __restrict__ Wf, float* __restrict__ s_out, float* __restrict__ b_out,
    const uint8_t* __restrict__ known, const T* __restrict__ qkv_table, T* __restrict__ q0, T* __restrict__ kv0, RowFilter flt) {
  posterior_sample_prep_rows_body<T, kKnown, kFilterArm>(logits, ldl, x_t, x_next, x_next2, rows, K, mask_id, seed, seed_hbm, row0, greedy, pc, mask_period,
                                                         sample_blocks, table, xres, stats, frame_mask, d, quads, fp, film_t, n_layers, Wf, s_out, b_out,
                                                         known, qkv_table, q0, kv0, flt);
}

// the loop's launch with top_p: no theta output (the loop has none), so `top_p` travels alone
template <typename T, bool kKnown>
__global__ __launch_bounds__(256) void nucleus_sample_prep_rows(
    const T* __restrict__ logits, int ldl, const int32_t* x_t, int32_t* x_next, int32_t* x_next2, int rows, int K, int mask_id,
    uint64_t seed, const uint64_t* __restrict__ seed_hbm, uint32_t row0, int greedy, PosteriorConsts pc, int mask_period, int sample_blocks,
    const T* __restrict__ table, T* __restrict__ xres, float* __restrict__ stats, const uint8_t* __restrict__ frame_mask, int d,
    bool quads, FoldStepPtrs fp, const T* __restrict__ film_t, int n_layers, T* __restrict__ Wf, float* __restrict__ s_out, float* __restrict__ b_out,
    const uint8_t* __restrict__ known, const T* __restrict__ qkv_table, T* __restrict__ q0, T* __restrict__ kv0, RowFilter flt, float top_p) {
  posterior_sample_prep_rows_body<T, kKnown, kNucleusArm>(logits, ldl, x_t, x_next, x_next2, rows, K, mask_id, seed, seed_hbm, row0, greedy, pc, mask_period,
                                                          sample_blocks, table, xres, stats, frame_mask, d, quads, fp, film_t, n_layers, Wf, s_out, b_out,
                                                          known, qkv_table, q0, kv0, flt, RowNucleus{top_p, nullptr});
}

// The sampler launch of the deduplicated loop (d3pm_dedup.hip): canvas row `row` reads the logits of compact row row_of[row] -- the same
// bits its own row would hold -- and everything per position stays per position: the Philox row, the known frames, x_next, the trace.
// Nothing is embedded here (the index of the next iteration comes first); the workgroups behind the sampler's fold fc1 as in
// posterior_sample_prep_rows (sample_blocks = the whole grid when there is no next iteration).
template <typename T, bool kKnown, int kFilter>
__device__ __forceinline__ void dedup_sample_rows_body(
    const T* __restrict__ logits, int ldl, const int32_t* __restrict__ row_of, const int32_t* x_t, int32_t* x_next, int32_t* x_next2, int rows, int K,
    int mask_id, uint64_t seed, const uint64_t* __restrict__ seed_hbm, uint32_t row0, int greedy, const PosteriorConsts& pc, int sample_blocks, int d,
    const FoldStepPtrs& fp, const T* __restrict__ film_t, int n_layers, T* __restrict__ Wf, float* __restrict__ s_out, float* __restrict__ b_out,
    const uint8_t* __restrict__ known, const RowFilter& flt, const RowNucleus& nuc = RowNucleus{}) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (static_cast<int>(blockIdx.x) >= sample_blocks) {
    const int r = (blockIdx.x - sample_blocks) * 4 + wave;
    if (r < 4 * d * n_layers) fold_layer_row<T>(fp, film_t, 4 * d, d, r, lane, Wf, s_out, b_out);
    return;
  }
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  if (seed_hbm) seed = *seed_hbm;
  int best_j;
  bool keep = false;
  if constexpr (kKnown) keep = row_is_known(known, row);      // wave-uniform: one wave per row
  if (keep) {
    best_j = x_t[row];
  } else {
    int src = __builtin_amdgcn_readfirstlane(row_of[row]);
    src = src < 0 ? 0 : (src >= rows ? rows - 1 : src);
    const T* lr = logits + static_cast<size_t>(src) * ldl;
    best_j = (K == 1025 && mask_id < 1024)
        ? sample_row_1025<T, kFilter>(lr, mask_id, x_t[row], seed, row0 + static_cast<uint32_t>(row), greedy, pc, lane, 0u, D3PM_SAMPLER_EARLY_OUT != 0, flt, nuc)
        : sample_row<T, kFilter>(lr, K, mask_id, x_t[row], seed, row0 + static_cast<uint32_t>(row), greedy, pc, nullptr, lane, 0u, flt, nuc);
  }
  if (lane == 0) {
    x_next[row] = best_j;
    if (x_next2) x_next2[row] = best_j;
  }
}

#define D3PM_DEDUP_SAMPLE_PARAMS                                                                                                                  \
  const T *__restrict__ logits, int ldl, const int32_t *__restrict__ row_of, const int32_t *x_t, int32_t *x_next, int32_t *x_next2, int rows, int K, \
      int mask_id, uint64_t seed, const uint64_t *__restrict__ seed_hbm, uint32_t row0, int greedy, PosteriorConsts pc, int sample_blocks, int d,     \
      FoldStepPtrs fp, const T *__restrict__ film_t, int n_layers, T *__restrict__ Wf, float *__restrict__ s_out, float *__restrict__ b_out,          \
      const uint8_t *__restrict__ known
#define D3PM_DEDUP_SAMPLE_PASS \
  logits, ldl, row_of, x_t, x_next, x_next2, rows, K, mask_id, seed, seed_hbm, row0, greedy, pc, sample_blocks, d, fp, film_t, n_layers, Wf, s_out, b_out, known
template <typename T, bool kKnown>
__global__ __launch_bounds__(256) void dedup_sample_rows(D3PM_DEDUP_SAMPLE_PARAMS) {
  dedup_sample_rows_body<T, kKnown, 0>(D3PM_DEDUP_SAMPLE_PASS, RowFilter{});
}
template <typename T, bool kKnown>
__global__ __launch_bounds__(256) void dedup_sample_rows_filtered(D3PM_DEDUP_SAMPLE_PARAMS, RowFilter flt) {
  dedup_sample_rows_body<T, kKnown, kFilterArm>(D3PM_DEDUP_SAMPLE_PASS, flt);
}
template <typename T, bool kKnown>
__global__ __launch_bounds__(256) void dedup_sample_rows_top_p(D3PM_DEDUP_SAMPLE_PARAMS, RowFilter flt, float top_p) {
  dedup_sample_rows_body<T, kKnown, kNucleusArm>(D3PM_DEDUP_SAMPLE_PASS, flt, RowNucleus{top_p, nullptr});
}
#undef D3PM_DEDUP_SAMPLE_PARAMS
#undef D3PM_DEDUP_SAMPLE_PASS

// ---- classifier-free guidance (d3pm_guidance) -------------------------------------------------------------------
// The logits buffer holds 2 * rows rows: row r is utterance row r under its condition (c), row rows + r the same frame under the
// null condition (u).  The accessor hands the row routines  fmaf(w, float(c_j) - float(u_j), float(c_j))  -- an fp32 subtraction and
// an explicit fma, no contraction left to the compiler -- and the routines round it to fp16 as their first act, where they round a
// plain logit today: one rounding, z_j = rn16(...).  Everything behind the load is the routine as it is.
template <typename T>
struct GuidedRow {
  const T* c; const T* u; float w;
  __device__ __forceinline__ GuidedRow(const T* c_, const T* u_, float w_) : c(c_), u(u_), w(w_) {}
  __device__ __forceinline__ float operator[](int j) const {
    const float cj = static_cast<float>(c[j]);
    return __builtin_fmaf(w, cj - static_cast<float>(u[j]), cj);
  }
};

// The guided kernels always carry the nucleus arm: with the neutral triple (1, 0, 1) filter_row and nucleus_row change no value (both
// tests are kernel-uniform and skip; the maximum is taken again over the same numbers), so the ids are those of the unfiltered
// routine -- tests/test_gpu_guidance.py compares exactly that pair.  n_q = 1, seed by value (the entries refuse anything else).
// k1025: the reference's class count takes kernels with the predicate-free routine alone, any other K kernels with the general routine
// alone.  (One kernel with both behind a kernel-uniform branch, as the unguided kernels have it, runs out of scalar registers here:
// the lane masks of the general routine's per-class guards stay alive across two loads and an fma each.)
template <typename T, bool k1025>
__device__ __forceinline__ int guided_row_draw(const T* __restrict__ logits, int ldl, int row, int rows, int K, int mask_id, int x, uint64_t seed,
                                               uint32_t grow, int greedy, const PosteriorConsts& pc, int lane, const RowFilter& flt, float top_p, float w) {
  const GuidedRow<T> lr(logits + static_cast<size_t>(row) * ldl, logits + (static_cast<size_t>(rows) + row) * ldl, w);
  const RowNucleus nuc{top_p, nullptr};
  if constexpr (k1025)
    return sample_row_1025<T, kNucleusArm>(lr, mask_id, x, seed, grow, greedy, pc, lane, 0u, D3PM_SAMPLER_EARLY_OUT != 0, flt, nuc);
  else
    return sample_row<T, kNucleusArm>(lr, K, mask_id, x, seed, grow, greedy, pc, nullptr, lane, 0u, flt, nuc);
}

template <typename T, bool kKnown, bool k1025>
__global__ __launch_bounds__(256) void guided_sample_rows(
    const T* __restrict__ logits, int ldl, const int32_t* x_t, int32_t* x_next, int32_t* x_next2, int rows, int K, int mask_id,
    uint64_t seed, uint32_t row0, int greedy, PosteriorConsts pc, const uint8_t* __restrict__ known, RowFilter flt, float top_p, float w) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  int best_j;
  bool keep = false;
  if constexpr (kKnown) keep = row_is_known(known, row);      // wave-uniform: one wave per row
  if (keep)
    best_j = x_t[row];
  else
    best_j = guided_row_draw<T, k1025>(logits, ldl, row, rows, K, mask_id, x_t[row], seed, row0 + static_cast<uint32_t>(row), greedy, pc, lane, flt, top_p, w);
  if (lane == 0) {
    x_next[row] = best_j;
    if (x_next2) x_next2[row] = best_j;
  }
}

// posterior_sample_prep_rows under guidance: the wave that draws row r writes the next iteration's embedding row and moments of rows
// r AND rows + r (the null twin sees the same x); the fc1-fold workgroups are those of the unguided launch.
// (The body repeats posterior_sample_prep_rows_body statement for statement instead of sharing it through a functor: with the shared
// form the compiler allocates the registers of the UNGUIDED fused kernels differently, and those are to stay the code they were.
// A change to either body belongs in both.)
template <typename T, bool kKnown, bool k1025>
__global__ __launch_bounds__(256) void guided_sample_prep_rows(
    const T* __restrict__ logits, int ldl, const int32_t* x_t, int32_t* x_next, int32_t* x_next2, int rows, int K, int mask_id,
    uint64_t seed, uint32_t row0, int greedy, PosteriorConsts pc, int mask_period, int sample_blocks,
    const T* __restrict__ table, T* __restrict__ xres, float* __restrict__ stats, const uint8_t* __restrict__ frame_mask, int d,
    bool quads, FoldStepPtrs fp, const T* __restrict__ film_t, int n_layers, T* __restrict__ Wf, float* __restrict__ s_out, float* __restrict__ b_out,
    const uint8_t* __restrict__ known, RowFilter flt, float top_p, float w) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (static_cast<int>(blockIdx.x) >= sample_blocks) {
    const int r = (blockIdx.x - sample_blocks) * 4 + wave;
    if (r < 4 * d * n_layers) fold_layer_row<T>(fp, film_t, 4 * d, d, r, lane, Wf, s_out, b_out);
    return;
  }
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  int best_j;
  bool keep = false;
  if constexpr (kKnown) keep = row_is_known(known, row);      // wave-uniform: one wave per row
  if (keep)
    best_j = x_t[row];
  else
    best_j = guided_row_draw<T, k1025>(logits, ldl, row, rows, K, mask_id, x_t[row], seed, row0 + static_cast<uint32_t>(row), greedy, pc, lane, flt, top_p, w);
  if (lane == 0) {
    x_next[row] = best_j;
    if (x_next2) x_next2[row] = best_j;
  }
  const bool live = frame_mask[row % mask_period] != 0;
  embed_row_stats<T>(table, best_j, live, xres, row, d, K, stats, quads, lane);
  embed_row_stats<T>(table, best_j, live, xres, rows + row, d, K, stats, quads, lane);
}

// forward noising: logits are log16(rn16(row_of_Qbar_t + eps)) with at most three distinct values
__global__ __launch_bounds__(256) void q_sample_rows(const int32_t* __restrict__ x0, int32_t* __restrict__ out,
                                                     const uint8_t* __restrict__ frame_mask, int mask_period,
                                                     int rows, int K, int mask_id, uint64_t seed,
                                                     uint32_t row0, int t, float log_dbar, float log_cbar,
                                                     float log_zero, float log_one) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + wave;
  if (row >= rows) return;
  const int x = x0[row];
  const int groups = (K + 3) >> 2;
  int best_j = 0;
  float best_v = -INFINITY;
  for (int g = lane; g < groups; g += kWave) {
    float u[4];
    noise4(seed, static_cast<uint32_t>(g), row0 + static_cast<uint32_t>(row), static_cast<uint32_t>(t), 1u, u);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      int j = g * 4 + w;
      if (j >= K) continue;
      float l;
      if (x == mask_id) l = (j == mask_id) ? log_one : log_zero;
      else l = (j == x) ? log_dbar : (j == mask_id ? log_cbar : log_zero);
      float v = l + gumbel(u[w]);
      if (v > best_v) { best_v = v; best_j = j; }
    }
  }
  wave_argmax(best_v, best_j);
  if (lane == 0) out[row] = frame_mask[row % mask_period] ? best_j : 0;
}

__global__ void uniform_rows(uint64_t seed, int t, uint32_t row0, int rows, int K, int stream_id,
                             float* __restrict__ out) {
  const int groups = (K + 3) >> 2;
  size_t idx = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<size_t>(rows) * groups) return;
  int r = static_cast<int>(idx / groups), g = static_cast<int>(idx % groups);
  float u[4];
  noise4(seed, static_cast<uint32_t>(g), row0 + static_cast<uint32_t>(r), static_cast<uint32_t>(t),
         static_cast<uint32_t>(stream_id), u);
  for (int w = 0; w < 4; ++w)
    if (g * 4 + w < K) out[static_cast<size_t>(r) * K + g * 4 + w] = u[w];
}

}  // namespace

float host_h2f(uint16_t h);
float host_log16(float fact);

int posterior_sample(const SampleArgs& a, hipStream_t s) {
  D3PM_REQUIRE(a.n_classes <= kWave * kMaxGroupsPerLane * 4, D3PM_E_SHAPE,
               "posterior_sample supports up to %d classes", kWave * kMaxGroupsPerLane * 4);
  const int rpb = 4;
  dim3 grid((a.rows + rpb - 1) / rpb), block(rpb * kWave);
  const RowFilter flt{a.temperature, a.top_k};
  const RowNucleus nuc{a.top_p, a.theta_out};
  // no map: the kernel without the known-row arm; neutral sampling options: the kernel without the filter arm; top_p (or a theta
  // output): the nucleus arm
#define D3PM_PS_ARGS(T)                                                                                                          \
  static_cast<const T*>(a.logits), a.ldl, a.x_t, a.x_next, a.x_next2, a.posterior_out, a.rows, a.n_classes, a.mask_id, a.seed, \
      a.seed_hbm, a.row0, a.greedy, a.pc, a.n_q, a.known
#define D3PM_PS_ARM(T, kKnown)                                                                            \
  do {                                                                                                    \
    if (a.nucleus()) nucleus_sample_rows<T, kKnown><<<grid, block, 0, s>>>(D3PM_PS_ARGS(T), flt, nuc);         \
    else if (a.filtered()) posterior_sample_rows_filtered<T, kKnown><<<grid, block, 0, s>>>(D3PM_PS_ARGS(T), flt); \
    else posterior_sample_rows<T, kKnown><<<grid, block, 0, s>>>(D3PM_PS_ARGS(T));                           \
  } while (0)
#define D3PM_PS(T)                    \
  do {                                \
    if (a.known) D3PM_PS_ARM(T, true); \
    else D3PM_PS_ARM(T, false);       \
  } while (0)
  switch (a.logits_dtype) {
    case D3PM_F32: D3PM_PS(float); break;
    case D3PM_F16: D3PM_PS(f16); break;
    case D3PM_BF16: D3PM_PS(bf16); break;
    default: set_error("unknown logits dtype %d", a.logits_dtype); return D3PM_E_ARG;
  }
#undef D3PM_PS
#undef D3PM_PS_ARM
#undef D3PM_PS_ARGS
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

bool posterior_sample_prep_supported(const SampleArgs& a, const NextIterPrep& n) {
  return a.n_q == 1 && !a.posterior_out && !a.theta_out && a.logits_dtype == n.dtype && (n.dtype == D3PM_F16 || n.dtype == D3PM_BF16) && n.n_layers <= 16 &&
         n.d % 256 == 0 && (!n.quads || n.d == 512) && a.n_classes <= kWave * kMaxGroupsPerLane * 4 && n.table && n.x && n.stats && n.frame_mask && n.mask_period > 0 && n.blocks && n.film_t && n.Wf &&
         (n.qkv_table != nullptr) == (n.q0 != nullptr) && (n.q0 != nullptr) == (n.kv0 != nullptr);
}

int posterior_sample_prep(const SampleArgs& a, const NextIterPrep& n, hipStream_t s) {
  FoldStepPtrs p{};
  for (int l = 0; l < n.n_layers; ++l) {
    p.W[l] = n.blocks[l].fc1_w; p.bias[l] = n.blocks[l].fc1_b; p.gamma[l] = n.blocks[l].norm3_w; p.beta[l] = n.blocks[l].norm3_b;
  }
  const int sample_blocks = (a.rows + 3) / 4, fold_blocks = (4 * n.d * n.n_layers + 3) / 4;
  const dim3 grid(static_cast<unsigned>(sample_blocks + fold_blocks)), block(256);
  const RowFilter flt{a.temperature, a.top_k};
#define D3PM_PSP_ARGS(T)                                                                                                                            \
  static_cast<const T*>(a.logits), a.ldl, a.x_t, a.x_next, a.x_next2, a.rows, a.n_classes, a.mask_id, a.seed, a.seed_hbm, a.row0, a.greedy, a.pc, \
      n.mask_period, sample_blocks, static_cast<const T*>(n.table), static_cast<T*>(n.x), n.stats, n.frame_mask, n.d, n.quads, p,                 \
      static_cast<const T*>(n.film_t), n.n_layers, static_cast<T*>(n.Wf), n.s_out, n.b_out, a.known, static_cast<const T*>(n.qkv_table),         \
      static_cast<T*>(n.q0), static_cast<T*>(n.kv0)
#define D3PM_PSP_ARM(T, kKnown)                                                                                  \
  do {                                                                                                           \
    if (a.nucleus()) nucleus_sample_prep_rows<T, kKnown><<<grid, block, 0, s>>>(D3PM_PSP_ARGS(T), flt, a.top_p);    \
    else if (a.filtered()) posterior_sample_prep_rows_filtered<T, kKnown><<<grid, block, 0, s>>>(D3PM_PSP_ARGS(T), flt); \
    else posterior_sample_prep_rows<T, kKnown><<<grid, block, 0, s>>>(D3PM_PSP_ARGS(T));                            \
  } while (0)
#define D3PM_PSP(T)                     \
  do {                                  \
    if (a.known) D3PM_PSP_ARM(T, true);  \
    else D3PM_PSP_ARM(T, false);        \
  } while (0)
  if (n.dtype == D3PM_F16) D3PM_PSP(f16); else D3PM_PSP(bf16);
#undef D3PM_PSP
#undef D3PM_PSP_ARM
#undef D3PM_PSP_ARGS
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

int posterior_sample_dedup(const SampleArgs& a, const int32_t* row_of, const NextIterPrep& n, hipStream_t s) {
  D3PM_REQUIRE(row_of && a.n_q == 1 && !a.posterior_out && !a.theta_out && !a.guided && (a.logits_dtype == D3PM_F16 || a.logits_dtype == D3PM_BF16) &&
                   a.n_classes <= kWave * kMaxGroupsPerLane * 4 && n.n_layers <= 16,
               D3PM_E_ARG, "deduplicated sampler: one level, 16-bit logits, ids only");
  const bool folds = n.Wf != nullptr;
  D3PM_REQUIRE(!folds || (n.blocks && n.film_t && n.s_out && n.b_out && n.d % 256 == 0 && n.dtype == a.logits_dtype), D3PM_E_ARG,
               "deduplicated sampler: bad fc1 fold arguments");
  FoldStepPtrs p{};
  if (folds)
    for (int l = 0; l < n.n_layers; ++l) {
      p.W[l] = n.blocks[l].fc1_w; p.bias[l] = n.blocks[l].fc1_b; p.gamma[l] = n.blocks[l].norm3_w; p.beta[l] = n.blocks[l].norm3_b;
    }
  const int sample_blocks = (a.rows + 3) / 4, fold_blocks = folds ? (4 * n.d * n.n_layers + 3) / 4 : 0;
  const dim3 grid(static_cast<unsigned>(sample_blocks + fold_blocks)), block(256);
  const RowFilter flt{a.temperature, a.top_k};
#define D3PM_DS_ARGS(T)                                                                                                                          \
  static_cast<const T*>(a.logits), a.ldl, row_of, a.x_t, a.x_next, a.x_next2, a.rows, a.n_classes, a.mask_id, a.seed, a.seed_hbm, a.row0, a.greedy, \
      a.pc, sample_blocks, n.d, p, static_cast<const T*>(n.film_t), folds ? n.n_layers : 0, static_cast<T*>(n.Wf), n.s_out, n.b_out, a.known
#define D3PM_DS_ARM(T, kKnown)                                                                                   \
  do {                                                                                                           \
    if (a.nucleus()) dedup_sample_rows_top_p<T, kKnown><<<grid, block, 0, s>>>(D3PM_DS_ARGS(T), flt, a.top_p);    \
    else if (a.filtered()) dedup_sample_rows_filtered<T, kKnown><<<grid, block, 0, s>>>(D3PM_DS_ARGS(T), flt);      \
    else dedup_sample_rows<T, kKnown><<<grid, block, 0, s>>>(D3PM_DS_ARGS(T));                                      \
  } while (0)
#define D3PM_DS(T)                     \
  do {                                 \
    if (a.known) D3PM_DS_ARM(T, true);  \
    else D3PM_DS_ARM(T, false);        \
  } while (0)
  if (a.logits_dtype == D3PM_F16) D3PM_DS(f16); else D3PM_DS(bf16);
#undef D3PM_DS
#undef D3PM_DS_ARM
#undef D3PM_DS_ARGS
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

// a.guided: a.logits holds 2 * a.rows rows (the null twins behind the conditioned rows), x_t / x_next / known a.rows
int posterior_sample_guided(const SampleArgs& a, hipStream_t s) {
  D3PM_REQUIRE(a.guided && a.n_q == 1 && !a.seed_hbm && !a.posterior_out && !a.theta_out, D3PM_E_ARG, "guided sampler: one level, seed by value, ids only");
  D3PM_REQUIRE(a.n_classes <= kWave * kMaxGroupsPerLane * 4, D3PM_E_SHAPE, "posterior_sample supports up to %d classes",
               kWave * kMaxGroupsPerLane * 4);
  const dim3 grid((a.rows + 3) / 4), block(256);
  const RowFilter flt{a.temperature, a.top_k};
  // the reference's class count takes kernels with the predicate-free routine alone, any other K kernels with the general one alone
  const bool k1025 = a.n_classes == 1025 && a.mask_id < 1024;
#define D3PM_GS_ARM(T, kKnown, kRef)                                                                                                          \
  guided_sample_rows<T, kKnown, kRef><<<grid, block, 0, s>>>(static_cast<const T*>(a.logits), a.ldl, a.x_t, a.x_next, a.x_next2, a.rows, a.n_classes, \
                                                             a.mask_id, a.seed, a.row0, a.greedy, a.pc, a.known, flt, a.top_p, a.guidance)
#define D3PM_GS(T)                                  \
  do {                                              \
    if (a.known && k1025) D3PM_GS_ARM(T, true, true);  \
    else if (a.known) D3PM_GS_ARM(T, true, false);     \
    else if (k1025) D3PM_GS_ARM(T, false, true);       \
    else D3PM_GS_ARM(T, false, false);                 \
  } while (0)
  switch (a.logits_dtype) {
    case D3PM_F32: D3PM_GS(float); break;
    case D3PM_F16: D3PM_GS(f16); break;
    case D3PM_BF16: D3PM_GS(bf16); break;
    default: set_error("unknown logits dtype %d", a.logits_dtype); return D3PM_E_ARG;
  }
#undef D3PM_GS
#undef D3PM_GS_ARM
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

// n.x / n.stats hold 2 * a.rows rows; supported where posterior_sample_prep_supported(a, n) holds
int posterior_sample_prep_guided(const SampleArgs& a, const NextIterPrep& n, hipStream_t s) {
  D3PM_REQUIRE(a.guided && !a.seed_hbm, D3PM_E_ARG, "guided sampler: seed by value");
  FoldStepPtrs p{};
  for (int l = 0; l < n.n_layers; ++l) {
    p.W[l] = n.blocks[l].fc1_w; p.bias[l] = n.blocks[l].fc1_b; p.gamma[l] = n.blocks[l].norm3_w; p.beta[l] = n.blocks[l].norm3_b;
  }
  const int sample_blocks = (a.rows + 3) / 4, fold_blocks = (4 * n.d * n.n_layers + 3) / 4;
  const dim3 grid(static_cast<unsigned>(sample_blocks + fold_blocks)), block(256);
  const RowFilter flt{a.temperature, a.top_k};
  const bool k1025 = a.n_classes == 1025 && a.mask_id < 1024;
#define D3PM_GSP(T, kKnown, kRef)                                                                                                                \
  guided_sample_prep_rows<T, kKnown, kRef><<<grid, block, 0, s>>>(                                                                                   \
      static_cast<const T*>(a.logits), a.ldl, a.x_t, a.x_next, a.x_next2, a.rows, a.n_classes, a.mask_id, a.seed, a.row0, a.greedy, a.pc,       \
      n.mask_period, sample_blocks, static_cast<const T*>(n.table), static_cast<T*>(n.x), n.stats, n.frame_mask, n.d, n.quads, p,                \
      static_cast<const T*>(n.film_t), n.n_layers, static_cast<T*>(n.Wf), n.s_out, n.b_out, a.known, flt, a.top_p, a.guidance)
#define D3PM_GSP_T(T)                                  \
  do {                                                 \
    if (a.known && k1025) D3PM_GSP(T, true, true);      \
    else if (a.known) D3PM_GSP(T, true, false);         \
    else if (k1025) D3PM_GSP(T, false, true);           \
    else D3PM_GSP(T, false, false);                     \
  } while (0)
  if (n.dtype == D3PM_F16) D3PM_GSP_T(f16); else D3PM_GSP_T(bf16);
#undef D3PM_GSP_T
#undef D3PM_GSP
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

int q_sample_launch(const d3pm_shape* sh, int batch, const int32_t* x0, int32_t* out, const uint8_t* frame_mask,
                    int t, const d3pm_schedule* sched, uint64_t seed, uint32_t utt0, hipStream_t s) {
  const int rows = batch * sh->canvas, rpb = 4;
  float ld = host_log16(host_h2f(sched->dbar[t])), lc = host_log16(host_h2f(sched->cbar[t]));
  q_sample_rows<<<(rows + rpb - 1) / rpb, rpb * kWave, 0, s>>>(x0, out, frame_mask, sh->canvas, rows, sh->n_classes,
                                                               sh->mask_id, seed, utt0 * sh->canvas, t, ld, lc,
                                                               host_log16(0.f), host_log16(1.f));
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

// Training-side loss rows (ar_discrete.py:683-690): x = logits * mask (a padded frame becomes an all-zero row, i.e. a
// uniform prediction), target = x0 * mask, row loss = logsumexp(x) - x[target]; the caller takes the mean over the
// canvas.  One wave per row, fp32 arithmetic on the logits as stored.
template <typename T>
__global__ __launch_bounds__(256) void ce_loss_rows(const T* __restrict__ logits, int ldl, const int32_t* __restrict__ targets,
                                                    const uint8_t* __restrict__ frame_mask, int mask_period, int rows, int K,
                                                    float* __restrict__ row_loss) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + wave;
  if (row >= rows) return;
  if (!frame_mask[row % mask_period]) {
    if (lane == 0) row_loss[row] = logf(static_cast<float>(K));
    return;
  }
  const T* lr = logits + static_cast<size_t>(row) * ldl;
  float mx = -INFINITY;
  for (int j = lane; j < K; j += kWave) mx = fmaxf(mx, static_cast<float>(lr[j]));
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < K; j += kWave) sum += expf(static_cast<float>(lr[j]) - mx);
  sum = wave_sum(sum);
  int tg = targets[row];
  tg = tg < 0 ? 0 : (tg >= K ? K - 1 : tg);
  if (lane == 0) row_loss[row] = mx + logf(sum) - static_cast<float>(lr[tg]);
}

int ce_loss_launch(int dtype, const void* logits, int ldl, const int32_t* targets, const uint8_t* frame_mask, int mask_period,
                   int rows, int K, float* row_loss, hipStream_t s) {
  const dim3 grid((rows + 3) / 4), block(256);
  switch (dtype) {
    case D3PM_F32: ce_loss_rows<float><<<grid, block, 0, s>>>(static_cast<const float*>(logits), ldl, targets, frame_mask, mask_period, rows, K, row_loss); break;
    case D3PM_F16: ce_loss_rows<f16><<<grid, block, 0, s>>>(static_cast<const f16*>(logits), ldl, targets, frame_mask, mask_period, rows, K, row_loss); break;
    case D3PM_BF16: ce_loss_rows<bf16><<<grid, block, 0, s>>>(static_cast<const bf16*>(logits), ldl, targets, frame_mask, mask_period, rows, K, row_loss); break;
    default: set_error("unknown logits dtype %d", dtype); return D3PM_E_ARG;
  }
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

int uniform_launch(uint64_t seed, int t, uint32_t row0, int rows, int K, int stream_id, float* out, hipStream_t s) {
  size_t n = static_cast<size_t>(rows) * ((K + 3) / 4);
  uniform_rows<<<static_cast<unsigned>((n + 255) / 256), 256, 0, s>>>(seed, t, row0, rows, K, stream_id, out);
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

}  // namespace d3pm
