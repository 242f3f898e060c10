// d3pm_nar_draw.hip -- the NAR stage's level draw with options (d3pm_nar_draw, include/d3pm_hip.h): known frames,
// top-k / top-p on the row's v = rn<T>(logit / temperature), and the log-probability of the id that stands in the frame afterwards.
//   nar_draw_rows   one wave per response frame on the grid of nar_sample_rows (d3pm_nar.hip), four frames per workgroup, the same row
//                   addressing; the row sits in registers in the z[R][4] layout of d3pm_sample_row.h (group g = lane + 64 i, classes
//                   4g .. 4g+3), so the Philox words of (g, (utt0 + b) * 65536 + f, level, stream 2) land on the classes they land on there.
// The cuts are the NAR's twins of filter_row / nucleus_row (d3pm_sample_row.h): the same selection, bit by bit from the top of an order
// key, but the key is that of the value in ITS OWN storage type -- 16 bits of the f16 / bf16 pattern (16 rounds), 32 bits of an fp32
// (32 rounds) -- where the D3PM routines key every value as fp16.  Those routines are left as they are, so the D3PM kernels compile to
// what they compiled to.  A launch without options never comes here: d3pm_api.hip sends it to nar_sample_rows.
// No LDS, no atomics, no barrier anywhere in this file.
#include <cmath>

#include "d3pm_kernels.h"
#include "d3pm_sample_row.h"

namespace d3pm {
namespace {

constexpr int kR = kMaxGroupsPerLane;

// value <-> key in the storage type T: negative values reverse (all bits flipped), the others move above them (sign bit set) -- the
// rule of f16_order_key on T's own bit pattern
template <typename T> struct KeyBits { using U = uint16_t; };
template <> struct KeyBits<float> { using U = uint32_t; };

template <typename T>
__device__ __forceinline__ uint32_t order_key(float v) {      // v is exact in T
  using U = typename KeyBits<T>::U;
  constexpr uint32_t top = 1u << (8 * sizeof(U) - 1), all = static_cast<uint32_t>(static_cast<U>(~static_cast<U>(0)));
  const uint32_t u = __builtin_bit_cast(U, static_cast<T>(v));
  return (u & top) ? (~u & all) : (u | top);
}
template <typename T>
__device__ __forceinline__ float order_value(uint32_t key) {
  using U = typename KeyBits<T>::U;
  constexpr uint32_t top = 1u << (8 * sizeof(U) - 1), all = static_cast<uint32_t>(static_cast<U>(~static_cast<U>(0)));
  const U u = static_cast<U>((key & top) ? (key & (top - 1u)) : (~key & all));
  return static_cast<float>(__builtin_bit_cast(T, u));
}

// theta1 = the top_k-th largest v counted with multiplicity; v' = v >= theta1 ? v : -inf.  key: 0 in a slot without a class (below
// every candidate, never counted).  The counts are popcounts of wave-wide compare masks: wave-uniform by construction.
template <typename T>
__device__ __forceinline__ void draw_top_k(float (&v)[kR][4], const uint32_t (&key)[kR][4], int top_k) {
  constexpr uint32_t top = 1u << (8 * sizeof(typename KeyBits<T>::U) - 1);
  uint32_t c = 0u;
#pragma unroll
  for (uint32_t bit = top; bit; bit >>= 1) {
    const uint32_t cand = c | bit;
    int n = 0;
#pragma unroll
    for (int i = 0; i < kR; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) n += __popcll(__ballot(key[i][w] >= cand));
    c = n >= top_k ? cand : c;
  }
  const float theta = order_value<T>(c);
#pragma unroll
  for (int i = 0; i < kR; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) v[i][w] = v[i][w] >= theta ? v[i][w] : -INFINITY;
}

// theta = value of the largest key c with mass(c) >= top_p * Q on the integer masses q = (uint32)(expf(v' - max v') * 2^20); returns
// it in every lane and cuts the row at it.  The keys of the classes top-k has cut are still those of their v: their q is 0 (v' is
// -inf), so they add nothing to any mass.  A row that is -inf throughout has Q = 0 (NaN converts to 0): every round holds, theta is
// the NaN of the all-ones key and the row stays -inf.
template <typename T>
__device__ __forceinline__ float draw_nucleus(float (&v)[kR][4], const uint32_t (&key)[kR][4], float top_p) {
  if (!(top_p < 1.0f)) return -INFINITY;      // kernel-uniform
  constexpr uint32_t top = 1u << (8 * sizeof(typename KeyBits<T>::U) - 1);
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < kR; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) mx = fmaxf(mx, v[i][w]);
  mx = wave_max(mx);
  uint32_t q[kR][4], part = 0u;
#pragma unroll
  for (int i = 0; i < kR; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      q[i][w] = static_cast<uint32_t>(expf(v[i][w] - mx) * 1048576.0f);
      part += q[i][w];
    }
  const uint32_t Q = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(wave_sum_u32(part))));
  const uint32_t target = static_cast<uint32_t>(ceil(static_cast<double>(top_p) * static_cast<double>(Q)));
  uint32_t c = 0u;
#pragma unroll
  for (uint32_t bit = top; bit; bit >>= 1) {
    const uint32_t cand = c | bit;
    uint32_t m = 0u;
#pragma unroll
    for (int i = 0; i < kR; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) m += key[i][w] >= cand ? q[i][w] : 0u;
    m = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(wave_sum_u32(m))));
    c = m >= target ? cand : c;
  }
  const float theta = order_value<T>(c);
#pragma unroll
  for (int i = 0; i < kR; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) v[i][w] = v[i][w] >= theta ? v[i][w] : -INFINITY;
  return theta;
}

// kFilter: 0 = no cut (known frames and / or the log-probability alone), kFilterArm = top-k, kNucleusArm = top-k and top-p
template <typename T, int kFilter>
__global__ __launch_bounds__(256) void nar_draw_rows(const T* __restrict__ logits, int ldl, const int32_t* __restrict__ lens,
                                                     int32_t* __restrict__ resp, int tr_max, int resp_stride, int t_max, int n_tokens,
                                                     int level, float temperature, uint64_t seed, uint32_t utt0, int greedy, int batch,
                                                     int top_k, float top_p, const uint8_t* __restrict__ known,
                                                     float* __restrict__ logprob_out, float* __restrict__ theta_out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int idx = blockIdx.x * (blockDim.x >> 6) + wave;
  if (idx >= batch * tr_max) return;
  const int b = idx / tr_max, f = idx % tr_max;
  const int tt = lens[b * 3], tp = lens[b * 3 + 1], tr = lens[b * 3 + 2];
  if (f >= tr || tt + tp + 2 + f >= t_max) return;   // outside the utterance or the grid: nothing is read, nothing is written
  int32_t* out = resp + (static_cast<size_t>(b) * tr_max + f) * resp_stride + level + 1;
  const bool held = known != nullptr && __builtin_amdgcn_readfirstlane(static_cast<int>(known[idx])) != 0;      // wave-uniform
  if (held) {
    if (theta_out && lane == 0) theta_out[idx] = __builtin_nanf("");
    if (!logprob_out) return;
  }
  const T* lr = logits + (static_cast<size_t>(b) * t_max + (tt + tp + 2 + f)) * ldl;
  float z[kR][4];      // float(l_j); -inf in a slot without a class
#pragma unroll
  for (int i = 0; i < kR; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int j = (lane + i * kWave) * 4 + w;
      z[i][w] = j < n_tokens ? ldf(lr + j) : -INFINITY;
    }
  int id;
  if (held) {
    id = __builtin_amdgcn_readfirstlane(*out);
  } else {
    float v[kR][4];    // what nar_sample_rows compares
#pragma unroll
    for (int i = 0; i < kR; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) v[i][w] = rn<T>(z[i][w] / temperature);      // -inf stays -inf
    if constexpr (kFilter != 0) {
      uint32_t key[kR][4];
#pragma unroll
      for (int i = 0; i < kR; ++i)
#pragma unroll
        for (int w = 0; w < 4; ++w) key[i][w] = (lane + i * kWave) * 4 + w < n_tokens ? order_key<T>(v[i][w]) : 0u;
      if (top_k > 0) draw_top_k<T>(v, key, top_k);      // kernel-uniform
      if constexpr (kFilter == kNucleusArm) {
        const float theta = draw_nucleus<T>(v, key, top_p);
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
    if (lane == 0) *out = id;
  }
  if (logprob_out) {
    // d3pm_logprob_row.h's order on the row's own logits: per-lane partial sums in ascending class, then wave_sum; z_j by
    // wave-uniform selects and the owner lane's copy (an id outside the row selects no register: -inf)
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < kR; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) mx = fmaxf(mx, z[i][w]);
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < kR; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) sum += expf(z[i][w] - mx);
    sum = wave_sum(sum);
    const int g = id >> 2, pass = g >> 6, word = id & 3, owner = g & (kWave - 1);
    float zv = -INFINITY;
#pragma unroll
    for (int i = 0; i < kR; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) zv = (pass == i && word == w) ? z[i][w] : zv;
    const float zj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, zv), owner));
    if (lane == 0) logprob_out[static_cast<size_t>(idx) * (resp_stride - 1) + level] = zj - mx - logf(sum);
  }
}

}  // namespace

int nar_draw(int dtype, const void* logits, int ldl, const int32_t* lens, int32_t* resp, int tr_max, int resp_stride, int t_max,
             int n_tokens, int level, float temperature, uint64_t seed, uint32_t utt0, int greedy, int batch, const NarDrawArgs& d,
             hipStream_t s) {
  D3PM_REQUIRE(n_tokens <= kWave * kMaxGroupsPerLane * 4, D3PM_E_SHAPE, "the NAR draw with options supports up to %d tokens",
               kWave * kMaxGroupsPerLane * 4);
  const dim3 grid((batch * tr_max + 3) / 4), block(256);
  const int arm = (d.theta_out || d.top_p < 1.0f) ? kNucleusArm : (d.top_k > 0 ? kFilterArm : 0);
#define D3PM_DRAW_ARM(T, kArm)                                                                                                          \
  nar_draw_rows<T, kArm><<<grid, block, 0, s>>>(static_cast<const T*>(logits), ldl, lens, resp, tr_max, resp_stride, t_max, n_tokens, level, \
                                                temperature, seed, utt0, greedy, batch, d.top_k, d.top_p, d.known, d.logprob_out, d.theta_out)
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
  D3PM_LAUNCH_CHECK();
  return D3PM_OK;
}

}  // namespace d3pm
