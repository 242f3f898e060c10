// d3pm_logprob.hip -- per-frame log-probability of the revealed id (d3pm_frame_scores, include/d3pm_hip.h): one launch behind the
// sampler launch of an iteration, issued only by the *_scored loops and by d3pm_frame_scores_step,
//   frame_scores_init_rows   one thread per canvas row: step = (live && !known && x == mask_id) ? 0 : -1, logprob = 0
//   frame_logprob_rows       one wave per canvas row, four rows per workgroup like the samplers.  A wave leaves after two words unless
//                            the row is free, still marked masked (step 0) and has just left the mask (x_next != mask_id); a wave that
//                            stays reads the row's logits once, writes logprob, then step = t.  On average rows / (T - 1) rows per
//                            iteration do that.
// Three sources of the logits row: plain (row r), guided (rows r and rows + r through rn16(fmaf(w, c - u, c)), d3pm_guidance) and
// indexed (row row_of[r] of the deduplicated loop's compact logits, clamped like dedup_sample_rows).
// No LDS, no atomics, no barrier anywhere in this file.
#include <cmath>

#include "d3pm_kernels.h"
#include "d3pm_logprob_row.h"

namespace d3pm {
namespace {

constexpr int kSrcPlain = 0, kSrcGuided = 1, kSrcIndexed = 2;

// GuidedRow of d3pm_sample.hip (a copy: that one lives in its file's unnamed namespace): an fp32 subtraction and an explicit fma, which
// the row routine rounds to fp16 as its first act
template <typename T>
struct ScoredGuidedRow {
  const T* c; const T* u; float w;
  __device__ __forceinline__ ScoredGuidedRow(const T* c_, const T* u_, float w_) : c(c_), u(u_), w(w_) {}
  __device__ __forceinline__ float operator[](int j) const {
    const float cj = static_cast<float>(c[j]);
    return __builtin_fmaf(w, cj - static_cast<float>(u[j]), cj);
  }
};

__global__ __launch_bounds__(256) void frame_scores_init_rows(const int32_t* __restrict__ x, const uint8_t* __restrict__ frame_mask, int mask_period,
                                                              const uint8_t* __restrict__ known, float* __restrict__ logprob,
                                                              int32_t* __restrict__ step, int rows, int mask_id) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const bool free_masked = frame_mask[static_cast<size_t>(row) % mask_period] != 0 && !(known && known[row] != 0) && x[row] == mask_id;
  step[row] = free_masked ? 0 : -1;
  logprob[row] = 0.0f;
}

// k1025: the reference's class count takes kernels with the predicate-free routine alone, any other K kernels with the general one alone
// (as the guided samplers are split, d3pm_sample.hip guided_row_draw)
template <typename T, int kSrc, bool k1025>
__global__ __launch_bounds__(256) void frame_logprob_rows(const T* __restrict__ logits, int ldl, const int32_t* __restrict__ row_of,
                                                          const int32_t* __restrict__ x_next, float* __restrict__ logprob, int32_t* step, int rows,
                                                          int K, int mask_id, int t, float w) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  // wave-uniform loads of the row's state, scalar branches on them: a row that is not free, already scored or still masked leaves here
  if (__builtin_amdgcn_readfirstlane(step[row]) != 0) return;
  const int j = __builtin_amdgcn_readfirstlane(x_next[row]);
  if (j == mask_id) return;
  float lp;
  if constexpr (kSrc == kSrcGuided) {
    const ScoredGuidedRow<T> lr(logits + static_cast<size_t>(row) * ldl, logits + (static_cast<size_t>(rows) + row) * ldl, w);
    if constexpr (k1025) lp = logprob_row_1025<T>(lr, mask_id, j, lane);
    else lp = logprob_row<T>(lr, K, mask_id, j, lane);
  } else {
    int src = row;
    if constexpr (kSrc == kSrcIndexed) {
      src = __builtin_amdgcn_readfirstlane(row_of[row]);
      src = src < 0 ? 0 : (src >= rows ? rows - 1 : src);
    }
    const T* lr = logits + static_cast<size_t>(src) * ldl;
    if constexpr (k1025) lp = logprob_row_1025<T>(lr, mask_id, j, lane);
    else lp = logprob_row<T>(lr, K, mask_id, j, lane);
  }
  if (lane == 0) {
    logprob[row] = lp;
    step[row] = t;
  }
}

}  // namespace

int frame_scores_init(const int32_t* x, const uint8_t* frame_mask, int mask_period, const uint8_t* known, float* logprob, int32_t* step, int rows,
                      int mask_id, hipStream_t s) {
  frame_scores_init_rows<<<dim3((rows + 255) / 256), dim3(256), 0, s>>>(x, frame_mask, mask_period, known, logprob, step, rows, mask_id);
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

int frame_logprob(const LogprobArgs& a, hipStream_t s) {
  D3PM_REQUIRE(a.n_classes <= kWave * kMaxGroupsPerLane * 4, D3PM_E_SHAPE, "the frame scores support up to %d classes", kWave * kMaxGroupsPerLane * 4);
  D3PM_REQUIRE(!(a.row_of && (a.guided || a.logits_dtype == D3PM_F32)), D3PM_E_ARG, "frame scores: indexed logits are 16-bit and unguided");
  const dim3 grid((a.rows + 3) / 4), block(256);
  const bool k1025 = a.n_classes == 1025 && a.mask_id < 1024;
#define D3PM_LP_ARM(T, kSrc, kRef)                                                                                                       \
  frame_logprob_rows<T, kSrc, kRef><<<grid, block, 0, s>>>(static_cast<const T*>(a.logits), a.ldl, a.row_of, a.x_next, a.logprob, a.step, \
                                                           a.rows, a.n_classes, a.mask_id, a.t, a.guidance)
#define D3PM_LP_SRC(T, kSrc)                \
  do {                                      \
    if (k1025) D3PM_LP_ARM(T, kSrc, true);  \
    else D3PM_LP_ARM(T, kSrc, false);       \
  } while (0)
#define D3PM_LP(T)                                  \
  do {                                              \
    if (a.guided) D3PM_LP_SRC(T, kSrcGuided);       \
    else if (a.row_of) D3PM_LP_SRC(T, kSrcIndexed); \
    else D3PM_LP_SRC(T, kSrcPlain);                 \
  } while (0)
  switch (a.logits_dtype) {
    case D3PM_F32:      // (never indexed: refused above)
      if (a.guided) D3PM_LP_SRC(float, kSrcGuided);
      else D3PM_LP_SRC(float, kSrcPlain);
      break;
    case D3PM_F16: D3PM_LP(f16); break;
    case D3PM_BF16: D3PM_LP(bf16); break;
    default: set_error("unknown logits dtype %d", a.logits_dtype); return D3PM_E_ARG;
  }
#undef D3PM_LP
#undef D3PM_LP_SRC
#undef D3PM_LP_ARM
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

}  // namespace d3pm
