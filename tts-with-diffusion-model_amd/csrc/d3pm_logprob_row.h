// d3pm_logprob_row.h -- the model's own log-probability of one id among the codec ids of a row (d3pm_frame_scores).
// One wave, one row.  The statements are those of reveal_from_z / reveal_row_1025 / reveal_row (d3pm_sample_row.h) under the neutral
// triple, repeated here instead of shared with them (d3pm_sample.hip on guided_sample_prep_rows says why): the row's z = rn16(logit)
// lose the mask class (-inf), then
//     m = max z,  S = sum_k expf(z_k - m)  (per-lane partial sums in ascending class, the tail last, then wave_sum),
//     logprob = z_j - m - logf(S)
// for the id j the caller names (wave-uniform, not the mask id).  No temperature, no top-k, no top-p: for the greedy candidate of
// d3pm_reveal under the neutral triple this is that row's conf, bit for bit.  The NAR draw (d3pm_nar_draw.hip) calls logprob_from_z
// on a row's own float(logit) with mask_id = -1 (no class is the mask) and no tail.
#pragma once
#include <cmath>

#include "d3pm_sample_row.h"

namespace d3pm {
namespace {

// z, zt, tail_j, kTail as for reveal_from_z; j wave-uniform.  A j outside the row's classes selects no register: -inf (general
// layout) or the tail's z (1025 layout, where pass 4 is the tail) -- registers only, nothing is read from memory through j.
template <int R, bool kTail>
__device__ __forceinline__ float logprob_from_z(float (&z)[R][4], float zt, int tail_j, int mask_id, int j, int lane) {
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) z[i][w] = (lane + i * kWave) * 4 + w == mask_id ? -INFINITY : z[i][w];
  if (kTail && tail_j == mask_id) zt = -INFINITY;
  float mx = zt;
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) mx = fmaxf(mx, z[i][w]);
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) sum += expf(z[i][w] - mx);      // exp(-inf) = 0: the mask class, slots without a class
  if constexpr (kTail) sum += expf(zt - mx);
  sum = wave_sum(sum);
  // z_j: pass / word picked by wave-uniform selects, then the owner lane's copy (the tail: no pass hits, lane 0 holds zt)
  const int g = j >> 2, pass = g >> 6, word = j & 3, owner = g & (kWave - 1);
  float zv = kTail ? zt : -INFINITY;
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) zv = (pass == i && word == w) ? z[i][w] : zv;
  const float zj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, zv), owner));
  return zj - mx - logf(sum);
}

template <typename T, typename P>
__device__ __forceinline__ float logprob_row_1025(P lr, int mask_id, int j, int lane) {
  constexpr int K = 1025;
  float z[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) z[i][w] = rn16(static_cast<float>(lr[(lane + i * kWave) * 4 + w]));
  const float zt = lane == 0 ? rn16(static_cast<float>(lr[K - 1])) : -INFINITY;
  return logprob_from_z<4, true>(z, zt, K - 1, mask_id, j, lane);
}

template <typename T, typename P>
__device__ __forceinline__ float logprob_row(P lr, int K, int mask_id, int j, int lane) {
  const int groups = (K + 3) >> 2;
  float z[kMaxGroupsPerLane][4];
#pragma unroll
  for (int i = 0; i < kMaxGroupsPerLane; ++i) {
    const int g = lane + i * kWave;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = g * 4 + w;
      z[i][w] = (g < groups && c < K) ? rn16(static_cast<float>(lr[c])) : -INFINITY;
    }
  }
  return logprob_from_z<kMaxGroupsPerLane, false>(z, -INFINITY, 0, mask_id, j, lane);
}

}  // namespace
}  // namespace d3pm
