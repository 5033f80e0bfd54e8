// libpgx: device code shared by the kernels that run over the query kernels' selection bits (pgx_hll.hip,
// pgx_distinct.hip), on top of the forward-index readers of pgx_device.h (one row at a time or a whole mask word's 32
// rows at once): folding group columns' global ids into a dense slot; and the walk itself -- an item's 32-doc mask
// words strided over a workgroup, zero words skipped, dense words decoded whole and sparse ones row by row, multi-value
// columns as runs of docs that own ranges of the value stream, under GROUP BY with the docs' slots parked in LDS.  The
// walk is a template over the item type; what happens to a word, a row or a batch of value rows is the caller's
// callable, so nothing here knows whether it maxes a register or ORs a presence bit.  The launchers' argument checks
// are at the end.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pgx_device.h"
#include "pgx_internal.h"

namespace pgx {

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

// the slot of one row, or kHllNoSlot or more: a remap of -1, or a key outside the planned space
__device__ __forceinline__ uint32_t sel_row_slot(const HllGCol* gc, const HllGroupKey& K, int32_t row) {
  uint32_t s = 0u;
  for (int g = 0; g < K.ngcols; ++g) {
    const uint32_t id = pgx_fwd_value(gc[g].fwd, row, gc[g].bits);
    const uint32_t gid = gc[g].remap ? static_cast<uint32_t>(gc[g].remap[id]) : id;  // a negative id: >= 2^31
    s = hll_mv_fold(s, gid, static_cast<uint32_t>(K.gmul[g]));
  }
  return s;
}

// The same through the directory of a sparse run: the row's global ids packed into the directory's key and looked up
// over the whole table.  The group's index, or kHllNoSlot for a key the directory does not hold (an id that does not
// fit its field, a remap of -1 among them, is in no key); every such row is counted in *K.miss.
__device__ __forceinline__ uint32_t sel_row_slot_sparse(const HllGCol* gc, const SelSparseKey& K, int32_t row) {
  u64 k0 = 0ull, k1 = 0ull;
  uint32_t bad = 0u;
  for (int g = 0; g < K.ngcols; ++g) {
    const uint32_t id = pgx_fwd_value(gc[g].fwd, row, gc[g].bits);
    const uint32_t gid = gc[g].remap ? static_cast<uint32_t>(gc[g].remap[id]) : id;  // a negative id: >= 2^31
    const uint32_t sh = K.shift[g];
    bad |= static_cast<uint32_t>(static_cast<u64>(gid) >> K.bits[g]);  // (bits <= 31: a card is an int32)
    const u64 lo = static_cast<u64>(gid) << sh;
    const u64 hi = sh > 32u ? static_cast<u64>(gid) >> (64u - sh) : 0ull;  // the part past bit 64 (0 unless it straddles)
    const u64 w1 = 0ull - static_cast<u64>(K.word[g]);                     // all ones: the field starts in word 1
    k0 |= lo & ~w1;
    k1 |= (lo & w1) | (hi & ~w1);
  }
  i64 h = -1;
  if (bad == 0u)
    h = K.W == 1 ? pgx_find<1>(K.keys, K.state, K.cap, {k0}, K.cap) : pgx_find<2>(K.keys, K.state, K.cap, {k0, k1}, K.cap);
  if (h < 0) {
    atomicAdd(K.miss, 1ull);
    return kHllNoSlot;
  }
  return K.index[h];
}

// rows of the key's tables: a slot at or past it is never written
__device__ __forceinline__ uint32_t sel_key_rows(const HllGroupKey& K) { return static_cast<uint32_t>(K.slots); }
__device__ __forceinline__ uint32_t sel_key_rows(const SelSparseKey& K) { return K.groups; }
__device__ __forceinline__ uint32_t sel_row_slot(const HllGCol* gc, const SelSparseKey& K, int32_t row) {
  return sel_row_slot_sparse(gc, K, row);
}

// s[j]: the slot of row J0 + j of the mask word that starts at doc d0, j < 16, through a sparse run's directory: the
// selected rows' lookups one after the other; a row that is not selected is not looked up (it would count as a miss)
// and gets kHllNoSlot.  (The dense keys' 16 independent id loads per group column stand in the kernels themselves,
// under `if constexpr`: moved into a function of their own they compiled into other code (pgx_percentile_count_group
// into 106 VGPRs instead of 120, four kernels with one more SGPR), and the dense instantiations are to stay,
// instruction for instruction, what they were.)
template <int J0>
__device__ __forceinline__ void sel_word_slots(const HllGCol* gc, const SelSparseKey& K, uint32_t sel, int32_t d0,
                                               uint32_t (&s)[16]) {
#pragma unroll
  for (int j = 0; j < 16; ++j)
    s[j] = ((sel >> (J0 + j)) & 1u) != 0u ? sel_row_slot_sparse(gc, K, d0 + J0 + j) : kHllNoSlot;
}

template <class Key>
__device__ __forceinline__ bool sel_gcols_ok(const HllGCol* gc, const Key& K) {
  bool ok = true;
  for (int g = 0; g < K.ngcols; ++g) ok = ok && gc[g].bits >= 1 && gc[g].bits <= 32;
  return ok;
}

// ---- the walk over an item's selection bits --------------------------------------------------------------------------
// On every callable handed to a walk: inlined before anything is optimised, as the loops written out by hand were.
// (Left to the inliner's judgement, pgx_distinct_mark_mv kept its item in scratch memory.)
#define PGX_SEL_OP __attribute__((always_inline))

// the item's limit: dictIds at or past it take no part
__host__ __device__ __forceinline__ int32_t sel_limit(const HllItem& A) { return A.ncodes; }
__host__ __device__ __forceinline__ int32_t sel_limit(const DistinctItem& A) { return A.card; }
__host__ __device__ __forceinline__ int32_t sel_limit(const PercentileItem& A) { return A.card; }

// mask words of an item; an item with a count or width out of range, or an empty code table or dictionary, has no rows
template <class Item>
__device__ __forceinline__ int sel_words(const Item& A) {
  return A.num_docs > 0 && A.bits >= 1 && A.bits <= 32 && sel_limit(A) >= 1 ? (A.num_docs + 31) >> 5 : 0;
}
template <class Item>
__device__ __forceinline__ int sel_mv_words(const Item& A, const int32_t* start, int32_t total) {
  return start && total > 0 ? sel_words(A) : 0;
}

// mask word w of the item without the bits at and past num_docs (the spare word is never read: w < words)
template <class Item>
__device__ __forceinline__ uint32_t sel_mask_word(const Item& A, int64_t w) {
  uint32_t sel = A.sel[w];
  const int32_t left = A.num_docs - static_cast<int32_t>(w * 32);
  if (left < 32) sel &= (1u << left) - 1u;
  return sel;
}

// The workgroup's share of the item's mask words, one word per thread and step.  A word with kHllDenseRows or more
// selected rows goes to dense(w, sel) whole, the rows of any other non-zero word one by one to row(doc).
template <class Item, class Dense, class Row>
__device__ __forceinline__ void sel_walk(const Item& A, int words, Dense dense, Row row) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kHllBlock;
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * kHllBlock + threadIdx.x; w < words; w += stride) {
    const uint32_t sel = sel_mask_word(A, w);
    if (sel == 0u) continue;
    if (__builtin_popcount(sel) >= kHllDenseRows) {
      dense(w, sel);
    } else {
      const int32_t d0 = static_cast<int32_t>(w * 32);
      for (uint32_t m = sel; m;) {
        const int k = __builtin_ctz(m);
        m &= m - 1u;
        row(d0 + k);
      }
    }
  }
}

template <int N>
using sel_rows = std::integral_constant<int, N>;  // a batch's size, handed to the callable as a type: its loops unroll
constexpr int kSelMvBatch = 16;  // value rows per pass of a long range
constexpr int kSelMvShort = 4;   // ... of a range's last rows (a sparse word's doc has a few values only)

// value rows [lo, hi) clamped to the stream (start[] is device data nobody validated), handed on as
// batch(sel_rows<N>, a, b): rows a .. a + N - 1 of which those below b count, a < b <= total
template <class Batch>
__device__ __forceinline__ void sel_mv_range(int32_t total, int32_t lo, int32_t hi, Batch batch) {
  uint32_t a = static_cast<uint32_t>(lo < 0 ? 0 : lo);
  const uint32_t b = static_cast<uint32_t>(hi < 0 ? 0 : hi < total ? hi : total);  // total > 0 (sel_mv_words)
  while (a < b && b - a > static_cast<uint32_t>(kSelMvShort)) {
    batch(sel_rows<kSelMvBatch>{}, a, b);
    a += kSelMvBatch;
  }
  if (a < b) batch(sel_rows<kSelMvShort>{}, a, b);
}

// A maximal run of selected docs a .. a + len - 1 of a mask word owns one contiguous value range: ranges are walked,
// not docs, and a fully selected word is one range.  One lane walks a range alone (long ranges are not shared across
// the wave), so a doc with hundreds of values keeps its lane busy while the wave's other lanes wait.
template <class Item, class Batch>
__device__ __forceinline__ void sel_mv_walk(const Item& A, int words, const int32_t* start, int32_t total,
                                            Batch batch) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kHllBlock;
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * kHllBlock + threadIdx.x; w < words; w += stride) {
    const int32_t d0 = static_cast<int32_t>(w * 32);
    for (uint32_t m = sel_mask_word(A, w); m;) {  // (bits at and past num_docs are off: d0 + a + len <= num_docs)
      const int a = __builtin_ctz(m);
      const uint32_t rest = ~(m >> a);
      const int len = rest ? __builtin_ctz(rest) : 32;
      m &= ~((len == 32 ? 0xFFFFFFFFu : ((1u << len) - 1u)) << a);
      sel_mv_range(total, start[d0 + a], start[d0 + a + len], batch);
    }
  }
}

// The same under GROUP BY.  A doc's slot comes from its single-value group columns gc; every value of the doc goes to
// that slot, so ranges are walked per doc: batch(slot, sel_rows<N>, a, b).  A word's slots are computed first, for a
// dense word in passes of independent loads over its 32 docs (all inside the group columns' padded indexes; a doc that
// is not selected takes remap entry 0), and parked in LDS (slot_of: 32 * kHllBlock words): one column of 32 per thread,
// which only that thread touches.
template <class Item, class Key, class Batch>
__device__ __forceinline__ void sel_mv_group_walk(const Item& A, const HllGCol* gc, const Key& K,
                                                  const int32_t* __restrict__ start, int32_t total, uint32_t* slot_of,
                                                  Batch batch) {
  const int tid = static_cast<int>(threadIdx.x);
  uint32_t* const mine = slot_of + tid;  // doc j of the word: mine[j * kHllBlock]
  const int words = sel_gcols_ok(gc, K) ? sel_mv_words(A, start, total) : 0;
  const uint32_t slots32 = sel_key_rows(K);  // <= kHllMaxGroupSlots, sparse: <= kSelMaxSparseGroups (launcher)
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kHllBlock;
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * kHllBlock + tid; w < words; w += stride) {
    const uint32_t sel = sel_mask_word(A, w);
    if (sel == 0u) continue;
    const int32_t d0 = static_cast<int32_t>(w * 32);
    if constexpr (std::is_same<Key, HllGroupKey>::value) {
      const bool dense = __builtin_popcount(sel) >= kHllDenseRows;
      for (int g = 0; g < K.ngcols; ++g) {
        const uint32_t* __restrict__ gf = gc[g].fwd;
        const int32_t* __restrict__ rm = gc[g].remap;
        const int gb = gc[g].bits;
        const uint32_t mul = static_cast<uint32_t>(K.gmul[g]);  // 1..slots (launcher)
        if (dense) {
#pragma unroll 8
          for (int j = 0; j < 32; ++j) {
            const uint32_t on = 0u - ((sel >> j) & 1u);
            const uint32_t id = pgx_fwd_value2(gf, d0 + j, gb) & on;
            const uint32_t gid = rm ? static_cast<uint32_t>(rm[id]) : id;  // a negative id: >= 2^31
            mine[j * kHllBlock] = hll_mv_fold(g == 0 ? 0u : mine[j * kHllBlock], gid, mul);
          }
        } else {
          for (uint32_t m = sel; m;) {
            const int j = __builtin_ctz(m);
            m &= m - 1u;
            const uint32_t id = pgx_fwd_value(gf, d0 + j, gb);
            const uint32_t gid = rm ? static_cast<uint32_t>(rm[id]) : id;
            mine[j * kHllBlock] = hll_mv_fold(g == 0 ? 0u : mine[j * kHllBlock], gid, mul);
          }
        }
      }
    } else {  // a sparse run: one directory lookup per selected doc
      for (uint32_t m = sel; m;) {
        const int j = __builtin_ctz(m);
        m &= m - 1u;
        mine[j * kHllBlock] = sel_row_slot_sparse(gc, K, d0 + j);
      }
    }
    for (uint32_t m = sel; m;) {
      const int j = __builtin_ctz(m);
      m &= m - 1u;
      const uint32_t s = mine[j * kHllBlock];
      if (s >= slots32) continue;  // (a key outside the planned space: the doc takes no part)
      sel_mv_range(total, start[d0 + j], start[d0 + j + 1],
                   [&](auto n, uint32_t a, uint32_t b) PGX_SEL_OP { batch(s, n, a, b); });
    }
  }
}

// ---- the launchers' checks, on the caller's host copy of the items ----------------------------------------------------
inline bool sel_grid_ok(int nitems, int wgs_per_item) {
  return nitems >= 0 && nitems <= 65535 && wgs_per_item >= 1 && wgs_per_item <= 1024;
}
inline bool sel_key_ok(int ngcols, const uint64_t* gmul, int64_t slots) {
  if (!gmul || ngcols < 1 || ngcols > kMaxGroupCols || slots < 1 || slots > kHllMaxGroupSlots) return false;
  for (int g = 0; g < ngcols; ++g)
    if (gmul[g] < 1 || gmul[g] > static_cast<uint64_t>(slots)) return false;  // a mixed-radix layout
  return true;
}
// the sparse forms' key, a host struct: the directory is there and sized, every field lies inside the key's W words
inline bool sel_sparse_key_ok(const SelSparseKey* K) {
  if (!K || !K->keys || !K->index || !K->miss || (K->W != 1 && K->W != 2) || (K->W == 2 && !K->state)) return false;
  if (K->groups < 1u || K->groups > static_cast<uint32_t>(kSelMaxSparseGroups)) return false;
  if (K->cap == 0 || (K->cap & (K->cap - 1)) != 0 || K->cap < K->groups) return false;
  if (K->ngcols < 1 || K->ngcols > kMaxGroupCols) return false;
  for (int g = 0; g < K->ngcols; ++g) {
    const int first = 64 * K->word[g] + K->shift[g];
    if (K->bits[g] < 1 || K->bits[g] > 32 || K->shift[g] > 63 || K->word[g] > 1 || first + K->bits[g] > 64 * K->W)
      return false;
  }
  return true;
}
inline bool sel_gcols_host_ok(const HllGCol* gc, int ngcols) {
  for (int c = 0; c < ngcols; ++c)
    if (!gc[c].fwd || gc[c].bits < 1 || gc[c].bits > 32) return false;
  return true;
}
template <class Item>
bool sel_item_ok(const Item& a, int32_t least_limit) {
  return a.num_docs >= 0 && a.bits >= 1 && a.bits <= 32 && sel_limit(a) >= least_limit && a.sel && a.fwd && a.out;
}
inline bool sel_mv_ok(const int32_t* start, int32_t total) { return start && total >= 0; }
inline HllGroupKey sel_key(int ngcols, const uint64_t* gmul, int64_t slots) {  // (after sel_key_ok)
  HllGroupKey K{};
  for (int g = 0; g < ngcols; ++g) K.gmul[g] = gmul[g];
  K.slots = static_cast<uint64_t>(slots);
  K.ngcols = ngcols;
  return K;
}

// One launch over nitems items, grid (workgroups per item, items): refused unless the grid is in range, both copies of
// the items are there and ok(check[i]) holds for every item; no items, no launch.  extra: the group forms' key.
template <class Item, class Ok, class... Extra>
hipError_t sel_launch(void (*kernel)(const Item*, int, Extra...), const Item* items, const Item* check, int nitems,
                      int wgs_per_item, hipStream_t stream, Ok ok, Extra... extra) {
  if (!sel_grid_ok(nitems, wgs_per_item) || !items || !check) return hipErrorInvalidValue;
  for (int i = 0; i < nitems; ++i)
    if (!ok(check[i])) return hipErrorInvalidValue;
  if (nitems == 0) return hipSuccess;
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(wgs_per_item), static_cast<unsigned>(nitems)), dim3(kHllBlock),
                     0, stream, items, nitems, extra...);
  return hipGetLastError();
}

}  // namespace pgx
