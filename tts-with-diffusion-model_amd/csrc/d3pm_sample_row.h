// d3pm_sample_row.h -- the per-row D3PM posterior + Gumbel-max draw, shared by the stand-alone sampler
// (d3pm_sample.hip: logits from HBM) and the fused final-projection + sampler (d3pm_final_sample.hip: logits from LDS).
// Arithmetic and rounding points: see the header of d3pm_sample.hip (/root/reference/vall_e/vall_e/ar_discrete.py:337-420).
#pragma once
#include <cmath>

#include "d3pm_kernels.h"
#include "d3pm_order_key.h"

namespace d3pm {
namespace {

constexpr int kMaxGroupsPerLane = 5;   // supports n_classes <= 64*5*4 = 1280
constexpr float kEps = 1.0e-6f;        // self.eps (ar_discrete.py:276), added in fp32 opmath then rounded

// ---- temperature / top-k on the x0-logits (d3pm_sampling) ----------------------------------------------
// kFilter arm of the two routines below: right after the load, the row's z = rn16(logit) become
//     z'  = rn16(z / temperature)                         (fp32 division, one rounding)
//     z'' = z' >= theta ? z' : -inf,  theta = the top_k-th largest z' counted with multiplicity (top_k = 0: no cut)
// and everything behind the load runs on z'' as it is.  theta is found without LDS and without a sort: every fp16 value maps to a
// 16-bit key whose unsigned order is the order of the values (d3pm_order_key.h), and the key of theta is the largest c with
// #{key >= c} >= top_k, built bit by bit from the top.  One round counts each of the lane's values with one vector compare
// whose wave-wide mask is popcounted on the scalar unit, so the count is wave-uniform by construction: no shuffle, no barrier,
// no divergence.  The final cut compares VALUES (z' >= theta), so that -0 and +0 (two keys, one value) are kept or cut together.
struct RowFilter {
  float temperature = 1.0f;
  int top_k = 0;
};

// z[R][4]: the lane's classes (valid(i, w) says which slots hold a class of the row; the others hold -inf and stay -inf);
// zt: one more class in the lanes where has_tail is set (sample_row_1025's class 1024), -inf elsewhere.
// TKey: the storage type whose rounding the temperature division takes and whose bit pattern is the key (d3pm_order_key.h): as
// many rounds per search as the key has bits.  The D3PM kernels key every value as fp16; the NAR draw (d3pm_nar_draw.hip) keys a
// row in the model's own dtype.
template <typename TKey = f16, int R, typename V>
__device__ __forceinline__ void filter_row(float (&z)[R][4], float& zt, bool has_tail, V valid, const RowFilter& f) {
  if (f.temperature != 1.0f) {      // kernel-uniform
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) z[i][w] = rn<TKey>(z[i][w] / f.temperature);      // -inf stays -inf
    zt = rn<TKey>(zt / f.temperature);
  }
  if (f.top_k > 0) {                // kernel-uniform
    uint32_t key[R][4];             // 0 for a slot without a class: below every candidate (>= 1), never counted
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) key[i][w] = valid(i, w) ? order_key<TKey>(z[i][w]) : 0u;
    const uint32_t kt = has_tail ? order_key<TKey>(zt) : 0u;
    uint32_t c = 0u;
#pragma unroll
    for (uint32_t bit = kKeyTop<TKey>; bit; bit >>= 1) {
      const uint32_t cand = c | bit;
      int n = __popcll(__ballot(kt >= cand));
#pragma unroll
      for (int i = 0; i < R; ++i)
#pragma unroll
        for (int w = 0; w < 4; ++w) n += __popcll(__ballot(key[i][w] >= cand));
      c = n >= f.top_k ? cand : c;
    }
    const float theta = order_value<TKey>(c);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) z[i][w] = z[i][w] >= theta ? z[i][w] : -INFINITY;
    zt = zt >= theta ? zt : -INFINITY;
  }
}

// ---- nucleus (top-p) on z'' (d3pm_nucleus) ---------------------------------------------------------------
// kFilter == kNucleusArm of the two routines below: behind filter_row, the row's z'' lose everything below the nucleus threshold,
//     e_j = expf(z''_j - max z''),  q_j = (uint32)(e_j * 2^20) truncated,  Q = sum_j q_j,  mass(c) = sum_{key_j >= c} q_j,
//     theta = value of the LARGEST key c with (double) mass(c) >= (double) top_p * (double) Q,   z'''_j = z''_j >= theta ? z''_j : -inf.
// The selection is the top-k one with weights instead of counts: mass is monotone in c, so the key is built bit by bit from the
// top; one round adds, per lane, the q of the lane's keys that are >= the candidate and sums the 64 integers over the wave (DPP and
// permlane-swap adds: no LDS, no barrier, no atomics).  Integers: Q and every mass are the same whatever order lanes add in, so theta
// is a function of the q_j alone.  A mass is an integer and the right-hand side one rounded fp64 product <= Q < 2^31, so
// mass >= rhs <=> mass >= ceil(rhs): the fp64 comparison is made once per row, as an integer target.  The maximum has q = 2^20 and
// is always kept: max z''' = max z'', and the exponentials of the kept classes are those the routine computes again behind this.
constexpr int kFilterArm = 1, kNucleusArm = 2;      // values of the routines' kFilter (0: no filter)
struct RowNucleus {
  float top_p = 1.0f;            // 1 = no cut (theta = -inf)
  float* theta_out = nullptr;    // optional: where lane 0 of the wave that filtered this row writes the row's theta
};

// wave_sum_up (d3pm_common.h) on integers: every step is v[l] + v[l ^ off], here exact in any order
template <int CTRL> __device__ __forceinline__ uint32_t add_dpp_u32(uint32_t v) {
  return v + static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
  v = add_dpp_u32<0xB1>(v);    // quad_perm [1, 0, 3, 2]: l ^ 1
  v = add_dpp_u32<0x4E>(v);    // quad_perm [2, 3, 0, 1]: l ^ 2
  v = add_dpp_u32<0x141>(v);   // row_half_mirror
  v = add_dpp_u32<0x140>(v);   // row_mirror
  uint32_t a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  v = a + b;
  a = v; b = v;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return a + b;
}

// z, zt, has_tail, valid: as for filter_row (which has run).  Returns theta in every lane.
template <typename TKey = f16, int R, typename V>
__device__ __forceinline__ float nucleus_row(float (&z)[R][4], float& zt, bool has_tail, V valid, float top_p) {
  if (!(top_p < 1.0f)) return -INFINITY;      // kernel-uniform
  float mx = zt;
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) mx = fmaxf(mx, z[i][w]);
  mx = wave_max(mx);
  uint32_t key[R][4], q[R][4];      // 0 / 0 for a slot without a class (its z is -inf: expf gives 0)
  uint32_t part = 0u;
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      key[i][w] = valid(i, w) ? order_key<TKey>(z[i][w]) : 0u;
      q[i][w] = static_cast<uint32_t>(expf(z[i][w] - mx) * 1048576.0f);
      part += q[i][w];
    }
  const uint32_t kt = has_tail ? order_key<TKey>(zt) : 0u;
  const uint32_t qt = static_cast<uint32_t>(expf(zt - mx) * 1048576.0f);
  const uint32_t Q = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(wave_sum_u32(part + qt))));
  const uint32_t target = static_cast<uint32_t>(ceil(static_cast<double>(top_p) * static_cast<double>(Q)));
  uint32_t c = 0u;
#pragma unroll
  for (uint32_t bit = kKeyTop<TKey>; bit; bit >>= 1) {
    const uint32_t cand = c | bit;
    uint32_t m = kt >= cand ? qt : 0u;
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) m += key[i][w] >= cand ? q[i][w] : 0u;
    m = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(wave_sum_u32(m))));      // every lane holds the sum
    c = m >= target ? cand : c;
  }
  const float theta = order_value<TKey>(c);
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) z[i][w] = z[i][w] >= theta ? z[i][w] : -INFINITY;
  zt = zt >= theta ? zt : -INFINITY;
  return theta;
}

// One wave draws x_{t-1} of one row.  `lr[j]` are the row's K logits in the model dtype (any address space);
// returns the sampled id in every lane.  `post_row` (optional) receives the fp16 posterior logits of the row.
// kFilter: kFilterArm = the row's logits pass through filter_row first (`flt`), kNucleusArm = through nucleus_row behind it as well
// (`nuc`); 0 = the routine without either, `flt` and `nuc` are never read.
template <typename T, int kFilter = 0, typename P>
__device__ __forceinline__ int sample_row(P lr, int K, int mask_id, int x, uint64_t seed, uint32_t grow, int greedy,
                                          const PosteriorConsts& pc, uint16_t* post_row, int lane, uint32_t stream = 0u,
                                          const RowFilter& flt = RowFilter{}, const RowNucleus& nuc = RowNucleus{}) {
  const int groups = (K + 3) >> 2;
  float z[kMaxGroupsPerLane][4];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < kMaxGroupsPerLane; ++i) {
    int g = lane + i * kWave;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      int j = g * 4 + w;
      float v = (g < groups && j < K) ? rn16(static_cast<float>(lr[j])) : -INFINITY;
      z[i][w] = v;
      mx = fmaxf(mx, v);
    }
  }
  if constexpr (kFilter != 0) {
    float none = -INFINITY;
    auto valid = [&](int i, int w) { const int g = lane + i * kWave; return g < groups && g * 4 + w < K; };
    filter_row(z, none, false, valid, flt);
    if constexpr (kFilter == kNucleusArm) {
      const float theta = nucleus_row(z, none, false, valid, nuc.top_p);
      if (nuc.theta_out && lane == 0) *nuc.theta_out = theta;
    }
    mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < kMaxGroupsPerLane; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) mx = fmaxf(mx, z[i][w]);
  }
  int best_j = 0;
  float best_v = -INFINITY;
  if (pc.t == 0) {
    // t == 0: model logits are used as they are and no noise is added (ar_discrete.py:407,413)
#pragma unroll
    for (int i = 0; i < kMaxGroupsPerLane; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        int j = (lane + i * kWave) * 4 + w;
        if (j < K && z[i][w] > best_v) { best_v = z[i][w]; best_j = j; }
      }
  } else {
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxGroupsPerLane; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        float e = expf(z[i][w] - mx);   // exp(-inf) = 0 for the padding classes
        z[i][w] = e;
        sum += e;
      }
    sum = wave_sum(sum);
    float s_other = 0.f, p_mask = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxGroupsPerLane; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        int j = (lane + i * kWave) * 4 + w;
        float p = rn16(z[i][w] / sum);
        z[i][w] = p;
        if (j == mask_id) p_mask = p; else s_other += p;
      }
    s_other = wave_sum(s_other);
    p_mask = wave_sum(p_mask);
    const float f2_mask = rn16(fmaf(s_other, pc.cbar_prev, p_mask));
    const bool x_is_mask = (x == mask_id);
#pragma unroll
    for (int i = 0; i < kMaxGroupsPerLane; ++i) {
      int g = lane + i * kWave;
      if (g >= groups) continue;
      float u[4];
      if (!greedy) noise4(seed, static_cast<uint32_t>(g), grow, static_cast<uint32_t>(pc.t), stream, u);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        int j = g * 4 + w;
        if (j >= K) continue;
        float lf1 = x_is_mask ? (j == mask_id ? pc.log_f1_one : pc.log_f1_c)
                              : (j == x ? pc.log_f1_d : pc.log_f1_zero);
        float f2 = (j == mask_id) ? f2_mask : rn16(z[i][w] * pc.dbar_prev);
        float lf2 = rn16(logf(rn16(f2 + kEps)));
        float out = rn16(lf1 + lf2);
        if (post_row) post_row[j] = __builtin_bit_cast(uint16_t, static_cast<f16>(out));
        float v = greedy ? out : out + gumbel(u[w]);
        if (v > best_v) { best_v = v; best_j = j; }   // ascending j per lane keeps the first maximum
      }
    }
  }
  wave_argmax(best_v, best_j);
  return best_j;
}

// The same routine for n_classes = 1025 = 4 x 256 + 1 (1024 codec ids + the mask id: every model of the reference, ar_discrete.py:255)
// without a predicate in it.  The general routine above walks five passes of 64 groups x 4 classes and tests every group and every
// class against K -- 121 exec-mask branches in the compiled kernel, and a fifth pass that exists for ONE class (1024, lane 0).
// Here passes 0..3 cover classes 0..1023 unconditionally and class 1024 is a tail element of lane 0 (the other lanes carry a -inf
// logit, whose exp is 0: what they added in the general routine as well).  Every operation on a class, the order in which a lane
// accumulates its partial sums (ascending class, the tail last) and the first-index argmax are those of sample_row: same bits.
#ifndef D3PM_SAMPLER_EARLY_OUT
#define D3PM_SAMPLER_EARLY_OUT 1      // A/B builds (tools/build_variant.py NAME -DD3PM_SAMPLER_EARLY_OUT=0): the full routine for every row
#endif
// kFilter as in sample_row.  The revealed-row early-out below stays exact under it: its bounds are statements about the routine's
// inputs, and the routine's inputs are then z'' -- `sum` is the sum over the kept classes, the kept token's score is computed from
// its own z'' (probability 0 when the filter cut it: the test then fails or holds exactly as the full routine decides).
template <typename T, int kFilter = 0, typename P>
__device__ __forceinline__ int sample_row_1025(P lr, int mask_id, int x, uint64_t seed, uint32_t grow, int greedy,
                                               const PosteriorConsts& pc, int lane, uint32_t stream = 0u, bool early_out = D3PM_SAMPLER_EARLY_OUT != 0,
                                               const RowFilter& flt = RowFilter{}, const RowNucleus& nuc = RowNucleus{}) {
  constexpr int K = 1025;
  float z[4][4], zt;
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      z[i][w] = rn16(static_cast<float>(lr[(lane + i * kWave) * 4 + w]));
      mx = fmaxf(mx, z[i][w]);
    }
  zt = lane == 0 ? rn16(static_cast<float>(lr[K - 1])) : -INFINITY;
  mx = fmaxf(mx, zt);
  if constexpr (kFilter != 0) {
    filter_row(z, zt, lane == 0, [](int, int) { return true; }, flt);
    if constexpr (kFilter == kNucleusArm) {      // paid before the early-out test below, whose `sum` is then the sum over z'''
      const float theta = nucleus_row(z, zt, lane == 0, [](int, int) { return true; }, nuc.top_p);
      if (nuc.theta_out && lane == 0) *nuc.theta_out = theta;
    }
    mx = zt;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) mx = fmaxf(mx, z[i][w]);
  }
  int best_j = 0;
  float best_v = -INFINITY;
  if (pc.t == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if (z[i][w] > best_v) { best_v = z[i][w]; best_j = (lane + i * kWave) * 4 + w; }
    if (zt > best_v) { best_v = zt; best_j = K - 1; }
  } else {
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        z[i][w] = expf(z[i][w] - mx);
        sum += z[i][w];
      }
    zt = expf(zt - mx);
    sum += zt;
    sum = wave_sum(sum);
    const bool x_is_mask = (x == mask_id);
    // score of class j from its probability: the reference's out_j (+ Gumbel noise); f2m = fact2 of the mask class
    auto one = [&](int j, float p, float u, float f2m) __attribute__((always_inline)) {
      const float lf1 = x_is_mask ? (j == mask_id ? pc.log_f1_one : pc.log_f1_c) : (j == x ? pc.log_f1_d : pc.log_f1_zero);
      const float f2 = (j == mask_id) ? f2m : rn16(p * pc.dbar_prev);
      const float lf2 = rn16(logf(rn16(f2 + kEps)));
      const float out = rn16(lf1 + lf2);
      return greedy ? out : out + gumbel(u);
    };
    // the uniforms of the row's 1025 classes: groups lane + 64 i (words 0..3) and word 0 of group 256
    float u[4][4], ut[4] = {0.5f, 0.5f, 0.5f, 0.5f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int w = 0; w < 4; ++w) u[i][w] = 0.5f;
      if (!greedy) noise4(seed, static_cast<uint32_t>(lane + i * kWave), grow, static_cast<uint32_t>(pc.t), stream, u[i]);
    }
    if (!greedy) noise4(seed, 256u, grow, static_cast<uint32_t>(pc.t), stream, ut);      // group 256 = classes 1024..1027: word 0
    if (!x_is_mask && !greedy && early_out) {
      // A REVEALED row (x_t != mask) keeps its token unless another class wins the Gumbel race, and every other class starts
      // log(eps) = -13.8 behind (fact1 = 0 off the diagonal: ar_discrete.py:337-420).  Instead of the posterior of all
      // 1025 classes (a division, three logs and six roundings each) the kept token's exact score is compared with an UPPER bound
      // of every other class's, built from the same monotone operations on upper bounds of their inputs:
      //   p_j <= rn16(1 / sum)  (the largest exponential is exp(0) = 1);   gumbel(u_j) <= gumbel(max_j u_j);   and for the mask class
      //   fact2_M <= rn16(1.001 cbar + rn16(1 / sum))  (sum_{k != M} p_k <= 1.001: 1025 roundings to fp16) with its own uniform.
      // If the kept token clears both bounds by 2^-5 (four fp16 quanta at this magnitude; whatever logf does in its last bit is four
      // orders below that) it is the argmax the full routine returns, whatever the other scores are; otherwise the full routine
      // runs on the values already in registers.  Same ids as without the test, by construction; what is skipped is ~55 % of the
      // row's vector work (the uniforms themselves, ~40 %, are still drawn: the stream is part of the contract).
      float um = fmaxf(fmaxf(fmaxf(u[0][0], u[0][1]), fmaxf(u[0][2], u[0][3])), fmaxf(fmaxf(u[1][0], u[1][1]), fmaxf(u[1][2], u[1][3])));
      um = fmaxf(um, fmaxf(fmaxf(fmaxf(u[2][0], u[2][1]), fmaxf(u[2][2], u[2][3])), fmaxf(fmaxf(u[3][0], u[3][1]), fmaxf(u[3][2], u[3][3]))));
      um = wave_max(lane == 0 ? fmaxf(um, ut[0]) : um);
      // (exponential, uniform) of a class id that is the same in every lane: pass / word picked by wave-uniform selects, then the owner
      // lane's copy (class 1024: group 256 = lane 0's tail)
      auto at = [&](int j, float& ej, float& uj) __attribute__((always_inline)) {
        const int g = j >> 2, pass = g >> 6, word = j & 3, owner = g & 63;
        float ev = zt, uv = ut[0];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const bool hit = pass == i && word == w;   // wave-uniform
            ev = hit ? z[i][w] : ev;
            uv = hit ? u[i][w] : uv;
          }
        ej = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ev), owner));
        uj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, uv), owner));
      };
      const int xu = __builtin_amdgcn_readfirstlane(x), mu = __builtin_amdgcn_readfirstlane(mask_id);
      float e_x, u_x, e_m, u_m;
      at(xu, e_x, u_x);
      at(mu, e_m, u_m);
      (void)e_m;
      const float v_x = one(xu, rn16(e_x / sum), u_x, 0.f);      // the kept token's score exactly as the full routine computes it (x != M)
      const float p_ub = rn16(1.0f / sum);
      const float lf2_ub = rn16(logf(rn16(rn16(p_ub * pc.dbar_prev) + kEps)));
      const float others_ub = rn16(pc.log_f1_zero + lf2_ub) + gumbel(um);
      const float lf2m_ub = rn16(logf(rn16(rn16(fmaf(1.001f, pc.cbar_prev, p_ub)) + kEps)));
      const float mask_ub = rn16(pc.log_f1_zero + lf2m_ub) + gumbel(u_m);
      if (fmaxf(others_ub, mask_ub) + 0.03125f < v_x) return xu;      // wave-uniform: every operand is
    }
    float s_other = 0.f, p_mask = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float p = rn16(z[i][w] / sum);
        z[i][w] = p;
        const bool is_mask = (lane + i * kWave) * 4 + w == mask_id;
        p_mask = is_mask ? p : p_mask;
        s_other += is_mask ? 0.f : p;           // (+ 0 leaves the partial sum as it is: the general routine skips the add)
      }
    zt = rn16(zt / sum);
    s_other += zt;                              // class 1024 is never the mask id (512)
    s_other = wave_sum(s_other);
    p_mask = wave_sum(p_mask);
    const float f2_mask = rn16(fmaf(s_other, pc.cbar_prev, p_mask));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int g = lane + i * kWave;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float v = one(g * 4 + w, z[i][w], u[i][w], f2_mask);
        if (v > best_v) { best_v = v; best_j = g * 4 + w; }   // ascending j per lane keeps the first maximum
      }
    }
    {
      const float v = one(K - 1, zt, ut[0], f2_mask);
      if (lane == 0 && v > best_v) { best_v = v; best_j = K - 1; }
    }
  }
  wave_argmax(best_v, best_j);
  return best_j;
}

// ---- confidence-ordered reveal (d3pm_reveal): candidate and score of one masked row ------------------------
// One wave, one row.  z, zt, has_tail, valid as for filter_row; kTail says whether the routine carries a tail class at all (class
// tail_j, held by the lanes with has_tail).  The row's z lose the mask class (-inf: the mask is not a token to reveal), pass through
// filter_row / nucleus_row as they are (kFilter != 0), and then
//     m = max z''',  S = sum_j expf(z'''_j - m),  cand = first-index argmax of z'''_j + gumbel(u_j)   (greedy: of z'''_j)
//     conf = z'''_cand - m - logf(S),  score = conf + lambda * gumbel(v)                              (lambda 0 or greedy: conf)
// u_j is the uniform the posterior draw of this row would take at this t (stream 0), v word 0 of (0, row, t, stream 4).
constexpr uint32_t kStreamRevealChoice = 4;
struct RevealRow { int cand; float score; };

template <int R, bool kTail, int kFilter, typename V>
__device__ __forceinline__ RevealRow reveal_from_z(float (&z)[R][4], float zt, bool has_tail, int tail_j, V valid, int mask_id, uint64_t seed,
                                                   uint32_t grow, uint32_t t, int greedy, float lambda, int lane, const RowFilter& flt, float top_p) {
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) z[i][w] = (lane + i * kWave) * 4 + w == mask_id ? -INFINITY : z[i][w];
  if (kTail && tail_j == mask_id) zt = -INFINITY;
  if constexpr (kFilter != 0) {
    filter_row(z, zt, has_tail, valid, flt);
    (void)nucleus_row(z, zt, has_tail, valid, top_p);
  }
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
    for (int w = 0; w < 4; ++w) sum += expf(z[i][w] - mx);      // exp(-inf) = 0: cut classes, the mask class, slots without a class
  if constexpr (kTail) sum += expf(zt - mx);
  sum = wave_sum(sum);
  int best_j = 0;
  float best_v = -INFINITY, best_z = -INFINITY;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int g = lane + i * kWave;
    float u[4] = {0.5f, 0.5f, 0.5f, 0.5f};
    if (!greedy) noise4(seed, static_cast<uint32_t>(g), grow, t, 0u, u);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float v = greedy ? z[i][w] : z[i][w] + gumbel(u[w]);      // -inf stays -inf and never wins
      if (v > best_v) { best_v = v; best_j = g * 4 + w; best_z = z[i][w]; }      // ascending j per lane keeps the first maximum
    }
  }
  if constexpr (kTail) {
    float ut[4] = {0.5f, 0.5f, 0.5f, 0.5f};
    if (!greedy) noise4(seed, static_cast<uint32_t>(tail_j >> 2), grow, t, 0u, ut);
    const float uw = (tail_j & 2) ? ((tail_j & 1) ? ut[3] : ut[2]) : ((tail_j & 1) ? ut[1] : ut[0]);
    const float v = greedy ? zt : zt + gumbel(uw);
    if (has_tail && v > best_v) { best_v = v; best_j = tail_j; best_z = zt; }
  }
  wave_argmax(best_v, best_j);
  // the lane that owns class best_j holds it as its own best (it carries the wave's maximum, first index): its z is z'''_cand
  const float zc = __shfl(best_z, (best_j >> 2) & (kWave - 1), kWave);
  RevealRow r;
  r.cand = best_j;
  r.score = zc - mx - logf(sum);
  if (lambda != 0.f && !greedy) {      // kernel-uniform
    float v[4];
    noise4(seed, 0u, grow, t, kStreamRevealChoice, v);
    r.score = r.score + lambda * gumbel(v[0]);
  }
  return r;
}

// the K = 1025 layout of sample_row_1025 (17 values per lane, no predicate) and the general one (K <= 1280) of sample_row
template <typename T, int kFilter, typename P>
__device__ __forceinline__ RevealRow reveal_row_1025(P lr, int mask_id, uint64_t seed, uint32_t grow, uint32_t t, int greedy, float lambda, int lane,
                                                     const RowFilter& flt, float top_p) {
  constexpr int K = 1025;
  float z[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) z[i][w] = rn16(static_cast<float>(lr[(lane + i * kWave) * 4 + w]));
  const float zt = lane == 0 ? rn16(static_cast<float>(lr[K - 1])) : -INFINITY;
  return reveal_from_z<4, true, kFilter>(z, zt, lane == 0, K - 1, [](int, int) { return true; }, mask_id, seed, grow, t, greedy, lambda, lane, flt,
                                         top_p);
}

template <typename T, int kFilter, typename P>
__device__ __forceinline__ RevealRow reveal_row(P lr, int K, int mask_id, uint64_t seed, uint32_t grow, uint32_t t, int greedy, float lambda, int lane,
                                                const RowFilter& flt, float top_p) {
  const int groups = (K + 3) >> 2;
  float z[kMaxGroupsPerLane][4];
#pragma unroll
  for (int i = 0; i < kMaxGroupsPerLane; ++i) {
    const int g = lane + i * kWave;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int j = g * 4 + w;
      z[i][w] = (g < groups && j < K) ? rn16(static_cast<float>(lr[j])) : -INFINITY;
    }
  }
  auto valid = [&](int i, int w) { const int g = lane + i * kWave; return g < groups && g * 4 + w < K; };
  return reveal_from_z<kMaxGroupsPerLane, false, kFilter>(z, -INFINITY, false, 0, valid, mask_id, seed, grow, t, greedy, lambda, lane, flt, top_p);
}

}  // namespace
}  // namespace d3pm
