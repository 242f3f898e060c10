// d3pm_nar_draw.hip -- the NAR stage's level draw with options (d3pm_nar_draw, include/d3pm_hip.h): known frames,
// top-k / top-p on the row's v = rn<T>(logit / temperature), and the log-probability of the id that stands in the frame afterwards.
//   nar_draw_rows   one wave per response frame on the grid of nar_sample_rows (d3pm_nar.hip), four frames per workgroup, the same row
//                   addressing; the row sits in registers in the z[R][4] layout of d3pm_sample_row.h (group g = lane + 64 i, classes
//                   4g .. 4g+3), so the Philox words of (g, (utt0 + b) * 65536 + f, level, stream 2) land on the classes they land on there.
// The cuts are filter_row / nucleus_row (d3pm_sample_row.h) with the key of a value in ITS OWN storage type -- 16 bits of the f16 /
// bf16 pattern (16 rounds), 32 bits of an fp32 (32 rounds) -- where the D3PM kernels key every value as fp16; the log-probability is
// logprob_from_z (d3pm_logprob_row.h).  A launch without options never comes here: d3pm_api.hip sends it to nar_sample_rows.
// Under classifier-free guidance (d3pm_nar_level_guided, d3pm_op_nar_draw_guided) the same kernel takes its guided arm: the grid holds
// 2 * batch utterances, utterance batch + b the null twin of b, and a frame's row is z = rn<T>(fmaf(w, float(c) - float(u), float(c)))
// of its two rows, formed where a plain row is loaded -- for the draw and once more for the log-probability.
// No LDS, no atomics, no barrier anywhere in this file.
#include <cmath>

#include "d3pm_kernels.h"
#include "d3pm_sample_row.h"
#include "d3pm_logprob_row.h"

namespace d3pm {
namespace {

constexpr int kR = kMaxGroupsPerLane;

__device__ __forceinline__ float guide_weight(float w) { return w; }

// kFilter: 0 = no cut (known frames and / or the log-probability alone), kFilterArm = top-k, kNucleusArm = top-k and top-p
// W: empty = the plain draw, whose kernels take no further argument; one float = the guided arm and its weight w (lens / logits /
// resp then hold 2 * batch utterances and `batch` counts the logical ones)
template <typename T, int kFilter, typename... W>
__global__ __launch_bounds__(256) void nar_draw_rows(const T* __restrict__ logits, int ldl, const int32_t* __restrict__ lens,
                                                     int32_t* __restrict__ resp, int tr_max, int resp_stride, int t_max, int n_tokens,
                                                     int level, float temperature, uint64_t seed, uint32_t utt0, int greedy, int batch,
                                                     int top_k, float top_p, const uint8_t* __restrict__ known,
                                                     float* __restrict__ logprob_out, float* __restrict__ theta_out, W... weight) {
  static_assert(sizeof...(W) <= 1, "at most the guidance weight");
  constexpr bool kGuided = sizeof...(W) == 1;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int idx = blockIdx.x * (blockDim.x >> 6) + wave;
  if (idx >= batch * tr_max) return;
  const int b = idx / tr_max, f = idx % tr_max;
  const int tt = lens[b * 3], tp = lens[b * 3 + 1], tr = lens[b * 3 + 2];
  if (f >= tr || tt + tp + 2 + f >= t_max) return;   // outside the utterance or the grid: nothing is read, nothing is written
  const T* ur = nullptr;      // the twin's row of the same frame
  float gw = 0.0f;
  if constexpr (kGuided) {
    const int un = lens[(batch + b) * 3] + lens[(batch + b) * 3 + 1] + 2 + f;
    if (un >= t_max) return;
    ur = logits + (static_cast<size_t>(batch + b) * t_max + un) * ldl;
    gw = guide_weight(weight...);
  }
  int32_t* out = resp + (static_cast<size_t>(b) * tr_max + f) * resp_stride + level + 1;
  const bool held = known != nullptr && __builtin_amdgcn_readfirstlane(static_cast<int>(known[idx])) != 0;      // wave-uniform
  if (held) {
    if (theta_out && lane == 0) theta_out[idx] = __builtin_nanf("");
    if (!logprob_out) return;
  }
  const T* lr = logits + (static_cast<size_t>(b) * t_max + (tt + tp + 2 + f)) * ldl;
  // float(l_j); -inf in a slot without a class.  Read once for the draw and once more for the log-probability (the row is in cache):
  // the logits do not stay in registers across the cuts.  Every slot reads an address inside the row (n_tokens >= 1) and the slots
  // without a class drop what they read: twenty loads in flight, no branch and no wait around each
  auto load_row = [&](float (&z)[kR][4]) {
#pragma unroll
    for (int i = 0; i < kR; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int j = (lane + i * kWave) * 4 + w;
        const int at = j < n_tokens ? j : n_tokens - 1;
        float l = ldf(lr + at);
        if constexpr (kGuided) l = rn<T>(__builtin_fmaf(gw, l - ldf(ur + at), l));      // the subtraction in fp32, one rounding to T
        z[i][w] = j < n_tokens ? l : -INFINITY;
      }
  };
  int id;
  if (held) {
    id = __builtin_amdgcn_readfirstlane(*out);
  } else {
    float v[kR][4];    // what nar_sample_rows compares
    load_row(v);
#pragma unroll
    for (int i = 0; i < kR; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) v[i][w] = rn<T>(v[i][w] / temperature);      // -inf stays -inf
    if constexpr (kFilter != 0) {      // the D3PM row cuts (d3pm_sample_row.h), keyed in T, on a row without a tail class
      float none = -INFINITY;
      auto valid = [&](int i, int w) { return (lane + i * kWave) * 4 + w < n_tokens; };
      filter_row<T>(v, none, false, valid, RowFilter{1.0f, top_k});      // the temperature has been applied above
      if constexpr (kFilter == kNucleusArm) {
        const float theta = nucleus_row<T>(v, none, false, valid, top_p);
        if (theta_out && lane == 0) theta_out[idx] = theta;
      }
    }
    // the statements of nar_sample_rows on v'': a cut class still draws its uniform, adds it to -inf and never wins
    int best_j = 0;
    float best_v = -INFINITY;
#pragma unroll
    for (int i = 0; i < kR; ++i) {
      const int g = lane + i * kWave;
      if (g * 4 >= n_tokens) continue;
      float u[4];
      if (!greedy) noise4(seed, static_cast<uint32_t>(g), (utt0 + static_cast<uint32_t>(b)) * 65536u + static_cast<uint32_t>(f),
                          static_cast<uint32_t>(level), 2u, u);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int j = g * 4 + w;
        if (j >= n_tokens) continue;
        float x = v[i][w];
        if (!greedy) x += gumbel(u[w]);
        if (x > best_v) { best_v = x; best_j = j; }
      }
    }
    wave_argmax(best_v, best_j);
    id = best_j;
    if (lane == 0) {
      *out = id;
      if constexpr (kGuided) out[static_cast<size_t>(batch) * tr_max * resp_stride] = id;      // the twin's half takes the same id
    }
  }
  if (logprob_out) {      // of the row's own logits: no mask class, no tail (an id outside the row selects no register: -inf)
    float z[kR][4];
    load_row(z);
    const float lp = logprob_from_z<kR, false>(z, -INFINITY, 0, /*mask_id*/ -1, id, lane);
    if (lane == 0) logprob_out[static_cast<size_t>(idx) * (resp_stride - 1) + level] = lp;
  }
}

}  // namespace

int nar_draw(int dtype, const void* logits, int ldl, const int32_t* lens, int32_t* resp, int tr_max, int resp_stride, int t_max,
             int n_tokens, int level, float temperature, uint64_t seed, uint32_t utt0, int greedy, int batch, const NarDrawArgs& d,
             hipStream_t s, const float* guidance) {
  D3PM_REQUIRE(n_tokens >= 1 && n_tokens <= kWave * kMaxGroupsPerLane * 4, D3PM_E_SHAPE, "the NAR draw with options supports up to %d tokens",
               kWave * kMaxGroupsPerLane * 4);
  const dim3 grid((batch * tr_max + 3) / 4), block(256);
  const int arm = (d.theta_out || d.top_p < 1.0f) ? kNucleusArm : (d.top_k > 0 ? kFilterArm : 0);
#define D3PM_DRAW_ARGS(T) \
  static_cast<const T*>(logits), ldl, lens, resp, tr_max, resp_stride, t_max, n_tokens, level, temperature, seed, utt0, greedy, batch, d.top_k, \
      d.top_p, d.known, d.logprob_out, d.theta_out
#define D3PM_DRAW_ARM(T, kArm)                                                                          \
  do {                                                                                                  \
    if (guidance) nar_draw_rows<T, kArm, float><<<grid, block, 0, s>>>(D3PM_DRAW_ARGS(T), *guidance);   \
    else nar_draw_rows<T, kArm><<<grid, block, 0, s>>>(D3PM_DRAW_ARGS(T));                              \
  } while (0)
#define D3PM_DRAW(T)                                        \
  do {                                                      \
    if (arm == kNucleusArm) D3PM_DRAW_ARM(T, kNucleusArm);  \
    else if (arm == kFilterArm) D3PM_DRAW_ARM(T, kFilterArm); \
    else D3PM_DRAW_ARM(T, 0);                               \
  } while (0)
  switch (dtype) {
    case D3PM_F32: D3PM_DRAW(float); break;
    case D3PM_F16: D3PM_DRAW(f16); break;
    case D3PM_BF16: D3PM_DRAW(bf16); break;
    default: set_error("unknown dtype %d", dtype); return D3PM_E_ARG;
  }
#undef D3PM_DRAW
#undef D3PM_DRAW_ARM
#undef D3PM_DRAW_ARGS
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

}  // namespace d3pm
