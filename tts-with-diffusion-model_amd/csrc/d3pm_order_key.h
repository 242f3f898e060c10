// d3pm_order_key.h -- value <-> key in a storage type T (f16, bf16, float): a key of T's width whose unsigned order is the order of
// the values.  Negative values reverse (all bits flipped), the others move above them (sign bit set).  -0 and +0 are two adjacent
// keys of one value, every non-NaN value has a key >= 1 (key 0 is a NaN: free for a slot that holds nothing), the all-ones key is a
// NaN.  The row cuts (d3pm_sample_row.h) and the reveal order (d3pm_reveal.hip) search a threshold key bit by bit from the top.
// Host and device: tests/order_key_table.cpp walks the map without a GPU.
#pragma once
#include "d3pm_common.h"

namespace d3pm {

template <typename T> struct KeyBits { using U = uint16_t; };
template <> struct KeyBits<float> { using U = uint32_t; };
template <typename T> constexpr uint32_t kKeyTop = 1u << (8 * sizeof(typename KeyBits<T>::U) - 1);      // where a bit-by-bit search starts

template <typename T>
__host__ __device__ __forceinline__ uint32_t order_key(float v) {      // v is exact in T
  using U = typename KeyBits<T>::U;
  constexpr uint32_t top = kKeyTop<T>, all = top | (top - 1u);
  const uint32_t u = __builtin_bit_cast(U, static_cast<T>(v));
  // (a 32-bit key is written without the mask that does nothing there: with it the compiler picks other instructions for
  // reveal_select, and tools/kernel_bodies.py compares the D3PM kernels with what they were)
  return (u & top) ? (sizeof(U) == 4 ? ~u : ~u & all) : (u | top);
}
template <typename T>
__host__ __device__ __forceinline__ float order_value(uint32_t key) {
  using U = typename KeyBits<T>::U;
  constexpr uint32_t top = kKeyTop<T>, all = top | (top - 1u);
  const U u = static_cast<U>((key & top) ? (key & (top - 1u)) : (~key & all));
  return static_cast<float>(__builtin_bit_cast(T, u));
}

}  // namespace d3pm
