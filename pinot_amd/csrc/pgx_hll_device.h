// libpgx: device helpers shared by the kernels that run over the query kernels' selection bits (pgx_hll.hip,
// pgx_distinct.hip): reading rows of a packed big-endian fixed-bit forward index, one at a time or a whole mask word's
// 32 rows at once, and folding group columns' global ids into a dense slot.
#pragma once
#include <hip/hip_runtime.h>

#include "pgx_internal.h"

namespace pgx {

__device__ __forceinline__ uint32_t hll_value(const uint32_t* __restrict__ fwd, int32_t row, int bits) {
  const int64_t o = static_cast<int64_t>(row) * bits;
  const uint32_t* w = fwd + (o >> 5);
  const int s = static_cast<int>(o & 31);
  const uint32_t mask = bits == 32 ? 0xFFFFFFFFu : ((1u << bits) - 1u);
  const uint32_t hi = __builtin_bswap32(w[0]);
  if (s + bits <= 32) return (hi >> (32 - s - bits)) & mask;  // (the next word may lie past the index: never read)
  const uint64_t x = (static_cast<uint64_t>(hi) << 32) | __builtin_bswap32(w[1]);
  return static_cast<uint32_t>(x >> (64 - s - bits)) & mask;
}

// The same without a branch: both dwords are always read.  For rows inside the padded index only (whole tiles plus 64
// bytes: the second dword of the last row is still inside).
__device__ __forceinline__ uint32_t hll_value2(const uint32_t* __restrict__ fwd, int32_t row, int bits) {
  const int64_t o = static_cast<int64_t>(row) * bits;
  const uint32_t* w = fwd + (o >> 5);
  const int s = static_cast<int>(o & 31);
  const uint64_t x = (static_cast<uint64_t>(__builtin_bswap32(w[0])) << 32) | __builtin_bswap32(w[1]);
  return static_cast<uint32_t>((x << s) >> (64 - bits));
}

// The 32 dictIds of one mask word's rows of a B-bit forward index: B dwords, every one read once (streaming), then
// constant-shift extraction (the layout of pgx_select.hip sel_decode32).
template <int B>
__device__ __forceinline__ void hll_decode32(const uint32_t* __restrict__ p, uint32_t (&v)[32]) {
  uint32_t w[B + 1];
#pragma unroll
  for (int i = 0; i < B; ++i) w[i] = __builtin_bswap32(__builtin_nontemporal_load(p + i));
  w[B] = 0;
  constexpr uint32_t MASK = (B == 32) ? 0xFFFFFFFFu : ((1u << (B & 31)) - 1u);
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int o = j * B, k = o >> 5, sh = o & 31;
    if (sh + B <= 32) {
      v[j] = (w[k] >> (32 - sh - B)) & MASK;
    } else {
      const uint64_t win = (static_cast<uint64_t>(w[k]) << 32) | w[k + 1];
      v[j] = static_cast<uint32_t>(win >> (64 - sh - B)) & MASK;
    }
  }
}

#define PGX_HLL_CASES(X) \
  X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) \
  X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)

__device__ __forceinline__ void hll_decode_word(int bits, const uint32_t* __restrict__ fwd, int64_t word,
                                                uint32_t (&v)[32]) {
  const uint32_t* p = fwd + word * bits;
  switch (bits) {
#define PGX_HLL_CASE(b)    \
  case b:                  \
    hll_decode32<b>(p, v); \
    break;
    PGX_HLL_CASES(PGX_HLL_CASE)
#undef PGX_HLL_CASE
    default:
#pragma unroll
      for (int j = 0; j < 32; ++j) v[j] = 0;
  }
}

constexpr int kHllDenseRows = 8;  // selected rows of a mask word from which the whole word's column is decoded

constexpr uint32_t kHllNoSlot = 0x20000u;  // above every slot (kHllMaxGroupSlots = 0x10000)

// One group column's global id folded into a doc's slot so far.  32-bit throughout: a slot inside the key space and
// each of its terms are below 0x10000, so both are clamped there before they are added; an id of 65536 or more (a
// remap entry of -1 among them) is outside every key space.  A result of 0x10000 or more stays there.
__device__ __forceinline__ uint32_t hll_mv_fold(uint32_t prev, uint32_t gid, uint32_t mul) {
  const uint32_t hi = gid >> 16;
  const uint32_t bad = static_cast<uint32_t>(static_cast<int32_t>(hi | (0u - hi)) >> 31);
  const uint32_t term = __builtin_elementwise_min((gid & 0xFFFFu) * mul, 0x10000u);  // mul <= 0x10000 (launcher)
  return (__builtin_elementwise_min(prev, 0x10000u) + term) | (bad & kHllNoSlot);
}

}  // namespace pgx
