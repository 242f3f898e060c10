// order_key_table.cpp -- walks the order-key map of csrc/d3pm_order_key.h on the host (tests/test_order_key_api.py builds and runs it).
// One line per storage type:  f16 / bf16 over all 65 536 keys, fp32 over its edge patterns and a fixed-seed sample of 2^20 patterns.
#include <cmath>
#include <cstdio>
#include <limits>

#include "d3pm_order_key.h"

using namespace d3pm;

// every key of a 16-bit type, ascending
template <typename T>
static void walk16(const char* name) {
  long nan = 0, roundtrip_bad = 0, decreasing = 0, equal_pairs = 0, zero_pairs = 0, below_one = 0;
  bool have_prev = false;
  float prev = 0.f;
  uint32_t prev_key = 0u;
  for (uint32_t k = 0; k < 65536u; ++k) {
    const float v = order_value<T>(k);
    if (std::isnan(v)) { ++nan; continue; }
    roundtrip_bad += order_key<T>(v) != k;
    below_one += k < 1u;
    if (have_prev) {
      decreasing += v < prev;
      if (v == prev) {      // consecutive non-NaN keys: with no decreasing pair, the only way two distinct keys share a value
        ++equal_pairs;
        zero_pairs += v == 0.f && std::signbit(prev) && !std::signbit(v) && k == prev_key + 1u;
      }
    }
    have_prev = true; prev = v; prev_key = k;
  }
  std::printf("%s keys=65536 nan=%ld roundtrip_bad=%ld decreasing=%ld equal_pairs=%ld zero_pairs=%ld below_one=%ld key0_nan=%d top_nan=%d "
              "key_neg_inf=%u key_neg_zero=%u key_pos_zero=%u key_pos_inf=%u\n",
              name, nan, roundtrip_bad, decreasing, equal_pairs, zero_pairs, below_one, std::isnan(order_value<T>(0u)) ? 1 : 0,
              std::isnan(order_value<T>(0xFFFFu)) ? 1 : 0, order_key<T>(-INFINITY), order_key<T>(-0.0f), order_key<T>(0.0f), order_key<T>(INFINITY));
}

static uint32_t bits_of(float v) { return __builtin_bit_cast(uint32_t, v); }

// one fp32 pattern: key -> value gives the pattern back bit for bit, value -> key the key
static bool roundtrip32(uint32_t u, long& nan) {
  const float v = __builtin_bit_cast(float, u);
  if (std::isnan(v)) { ++nan; return true; }
  const uint32_t k = order_key<float>(v);
  return k >= 1u && bits_of(order_value<float>(k)) == u && order_key<float>(order_value<float>(k)) == k;
}

int main() {
  walk16<f16>("f16");
  walk16<bf16>("bf16");
  const float fmax = std::numeric_limits<float>::max(), dmin = std::numeric_limits<float>::denorm_min();
  const float edge[] = {-INFINITY, -fmax, -1.0f, -dmin, -0.0f, 0.0f, dmin, 1.0f, fmax, INFINITY};      // ascending
  const int n_edge = static_cast<int>(sizeof(edge) / sizeof(edge[0]));
  long nan = 0, edge_bad = 0, edge_order_bad = 0, sample_bad = 0, sample_order_bad = 0;
  for (int i = 0; i < n_edge; ++i) {
    edge_bad += !roundtrip32(bits_of(edge[i]), nan);
    if (i > 0) edge_order_bad += !(order_key<float>(edge[i - 1]) < order_key<float>(edge[i]));      // -0 < +0 as keys
  }
  uint64_t s = 0x9E3779B97F4A7C15ull;      // splitmix64, fixed seed
  auto next = [&]() {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<uint32_t>((z ^ (z >> 31)) >> 16);
  };
  const long n_sample = 1l << 20;
  for (long i = 0; i < n_sample; ++i) {
    const uint32_t ua = next(), ub = next();
    sample_bad += !roundtrip32(ua, nan);
    const float a = __builtin_bit_cast(float, ua), b = __builtin_bit_cast(float, ub);
    if (std::isnan(a) || std::isnan(b)) continue;
    // the keys order as the values do; equal values with different keys are the two zeros
    const uint32_t ka = order_key<float>(a), kb = order_key<float>(b);
    sample_order_bad += (a < b) != (ka < kb) && !(a == b && a == 0.f);
  }
  std::printf("f32 edge=%d edge_bad=%ld edge_order_bad=%ld sample=%ld sample_bad=%ld sample_order_bad=%ld nan=%ld key0_nan=%d top_nan=%d "
              "key_neg_zero=%u key_pos_zero=%u\n",
              n_edge, edge_bad, edge_order_bad, n_sample, sample_bad, sample_order_bad, nan, std::isnan(order_value<float>(0u)) ? 1 : 0,
              std::isnan(order_value<float>(0xFFFFFFFFu)) ? 1 : 0, order_key<float>(-0.0f), order_key<float>(0.0f));
  return 0;
}
