// libpgx: DISTINCTCOUNT / DISTINCTCOUNTMV presence bitmaps -- DistinctCountAggregationFunction (operator/aggregation/
// function/DistinctCountAggregationFunction.java: the set of (int) hashCode over the selected docs' values;
// DistinctCountMVAggregationFunction.java: over every value of every selected doc) over the selection bits the query
// kernels wrote.  Reference paths are relative to pinot-core/src/main/java/com/linkedin/pinot/core/.
//
// The hash depends on the dictionary value alone, so the set of a dictionary's selected values is one presence bit per
// dictId: (card + 31) / 32 u32 words, under GROUP BY one such row per slot.  Bits are only ever ORed in: the words are
// exact whatever the grid size or scheduling, and segments that share a dictionary combine by marking the same bitmap.
// Every mark reads its word first and issues the atomic only when it adds a bit: after warm-up almost none does.
//
//   pgx_distinct_mark           grid (workgroups per item, items), one item per (segment, function).  A workgroup
//                               strides over its item's 32-row mask words as pgx_hll_offer does (zero words skipped,
//                               words with 8 or more selected rows decoded whole, the others row by row).  A bitmap of
//                               up to kDistinctLdsWords words is marked in LDS and its non-zero words are ORed into HBM
//                               at the end; a larger one is marked in HBM directly.
//   pgx_distinct_mark_group     the same into table[slot * words + (id >> 5)]: slot = sum of the group columns' global
//                               ids x gmul (column 0 least significant), as in pgx_hll_offer_group.
//   pgx_distinct_mark_mv        the column is multi-value: a run of consecutive selected docs of a mask word owns one
//                               contiguous range of the value stream, clamped to the stream's row count.
//   pgx_distinct_mark_mv_group  the same per doc, into the doc's slot's row.
//   pgx_distinct_count          popcount of each listed row of a table.
//   pgx_distinct_emit           hash[dictId] of every set bit of each listed row in ascending dictId order, from the
//                               caller's offset for that row on; positions come from a prefix over the word popcounts.
//                               Grid (workgroups per row, rows): a workgroup takes one stretch of the row's words and
//                               counts the bits of the words before it itself.
// The walk over the selection bits is shared with pgx_hll.hip and lives in pgx_hll_device.h; here are the marks it is
// handed, the result kernels and the launchers.
// No workgroup waits on another; all stores are plain vector stores and vector atomics.
#include <hip/hip_runtime.h>

#include "pgx_device.h"
#include "pgx_hll_device.h"
#include "pgx_internal.h"

namespace pgx {

constexpr uint32_t kDistinctNone = 0xFFFFFFFFu;  // no dictId: card <= INT32_MAX

__device__ __host__ __forceinline__ uint32_t dist_bitmap_words(int32_t card) {
  return (static_cast<uint32_t>(card) + 31u) >> 5;  // card >= 1
}

// bit `id` of the bitmap bm (LDS or HBM), id < card
__device__ __forceinline__ void dist_mark(uint32_t* bm, uint32_t id) {
  uint32_t* w = bm + (id >> 5);
  const uint32_t b = 1u << (id & 31u);
  if ((*w & b) == 0u) atomicOr(w, b);
}

// v[j]: the dictId of row j of a mask word.  Two passes of 32 independent accesses: the rows' bitmap words (a row that
// is not selected or whose dictId lies at or past card reads word 0, so no load is conditional), then the few atomics.
__device__ __forceinline__ void dist_mark_word(uint32_t* bm, const DistinctItem& A, uint32_t sel, uint32_t (&v)[32]) {
#pragma unroll
  for (int j = 0; j < 32; ++j) sel &= ~(static_cast<uint32_t>(v[j] >= static_cast<uint32_t>(A.card)) << j);
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const uint32_t on = 0u - ((sel >> j) & 1u);  // all ones or 0
    const uint32_t id = v[j] & on;
    const uint32_t have = 0u - ((bm[id >> 5] >> (id & 31u)) & 1u);
    v[j] = id | ~on | have;  // kDistinctNone: nothing to add
  }
#pragma unroll
  for (int j = 0; j < 32; ++j)
    if (v[j] != kDistinctNone) atomicOr(&bm[v[j] >> 5], 1u << (v[j] & 31u));
}

__device__ __forceinline__ void dist_scan(uint32_t* bm, const DistinctItem& A, int words) {
  sel_walk(
      A, words,
      [&](int64_t w, uint32_t sel) PGX_SEL_OP {
        uint32_t v[32];
        pgx_fwd_decode_word(A.bits, A.fwd, w, v);
        dist_mark_word(bm, A, sel, v);
      },
      [&](int32_t row) PGX_SEL_OP {
        const uint32_t id = pgx_fwd_value(A.fwd, row, A.bits);
        if (id < static_cast<uint32_t>(A.card)) dist_mark(bm, id);
      });
}

// the workgroup's LDS bitmap into the item's: only words that hold a bit, and an atomic only where one is new
__device__ __forceinline__ void dist_flush(const uint32_t* lbits, uint32_t* out, uint32_t bw) {
  for (uint32_t i = threadIdx.x; i < bw; i += kHllBlock) {
    const uint32_t b = lbits[i];
    if (b != 0u && (b & ~out[i]) != 0u) atomicOr(&out[i], b);
  }
}

__global__ void __launch_bounds__(kHllBlock) pgx_distinct_mark(const DistinctItem* __restrict__ items, int nitems) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  __shared__ uint32_t lbits[kDistinctLdsWords];
  const DistinctItem A = items[item];
  const int words = sel_words(A);
  if (words == 0) return;  // (the whole workgroup)
  const uint32_t bw = dist_bitmap_words(A.card);
  if (bw <= static_cast<uint32_t>(kDistinctLdsWords)) {
    for (uint32_t i = threadIdx.x; i < bw; i += kHllBlock) lbits[i] = 0u;
    __syncthreads();
    dist_scan(lbits, A, words);
    __syncthreads();
    dist_flush(lbits, A.out, bw);
  } else {
    dist_scan(A.out, A, words);
  }
}

// ---- GROUP BY: single-value group columns -> a dense slot ----------------------------------------------------------
// Rows J0 .. J0 + 15 of a mask word whose dictIds are decoded (v): slots, bitmap words, atomics.  Half a word at a
// time: 16 loads in flight per lane and pass.  The word's rows all lie inside the group columns' padded indexes, so the
// id loads are unconditional; a row that marks nothing takes remap entry 0 and reads word 0 of the table.
template <int J0, class Key>
__device__ __forceinline__ void dist_group_rows(const DistinctGroupItem& G, const Key& K, uint32_t sel, int32_t d0,
                                                uint32_t (&v)[32]) {
  const uint32_t slots32 = sel_key_rows(K);  // <= kHllMaxGroupSlots, sparse: <= kSelMaxSparseGroups (launcher)
  const uint32_t bw = dist_bitmap_words(G.d.card);
  uint32_t s[16];
  if constexpr (std::is_same<Key, HllGroupKey>::value) {
    for (int g = 0; g < K.ngcols; ++g) {
      const uint32_t* __restrict__ gf = G.g[g].fwd;
      const int32_t* __restrict__ rm = G.g[g].remap;
      const int gb = G.g[g].bits;
      const uint32_t mul = static_cast<uint32_t>(K.gmul[g]);  // 1..slots (launcher)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t on = 0u - ((sel >> (J0 + j)) & 1u);
        const uint32_t id = pgx_fwd_value2(gf, d0 + J0 + j, gb) & on;
        const uint32_t gid = rm ? static_cast<uint32_t>(rm[id]) : id;
        s[j] = hll_mv_fold(g == 0 ? 0u : s[j], gid, mul);
      }
    }
  } else {
    sel_word_slots<J0>(G.g, K, sel, d0, s);
  }
  uint32_t* const table = G.d.out;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t ok = static_cast<uint32_t>(static_cast<int32_t>(s[j] - slots32) >> 31);  // s < slots (< 2^18)
    const uint32_t on = (0u - ((sel >> (J0 + j)) & 1u)) & ok;
    const uint32_t id = v[J0 + j] & on;
    s[j] &= on;
    const uint32_t cur = table[static_cast<size_t>(s[j]) * bw + (id >> 5)];
    v[J0 + j] = id | ~on | (0u - ((cur >> (id & 31u)) & 1u));
  }
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (v[J0 + j] != kDistinctNone)
      atomicOr(&table[static_cast<size_t>(s[j]) * bw + (v[J0 + j] >> 5)], 1u << (v[J0 + j] & 31u));
}

// Key: HllGroupKey or SelSparseKey (pgx_hll_offer_group); only the slot computation differs.
template <class Key>
__global__ void __launch_bounds__(kHllBlock) pgx_distinct_mark_group(const DistinctGroupItem* __restrict__ items,
                                                                     int nitems, const Key K) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  const DistinctGroupItem& G = items[item];
  const DistinctItem A = G.d;
  const uint32_t slots32 = sel_key_rows(K);
  const uint32_t bw = dist_bitmap_words(A.card);
  sel_walk(
      A, sel_gcols_ok(G.g, K) ? sel_words(A) : 0,
      [&](int64_t w, uint32_t sel) PGX_SEL_OP {
        uint32_t v[32];
        pgx_fwd_decode_word(A.bits, A.fwd, w, v);
#pragma unroll
        for (int j = 0; j < 32; ++j) sel &= ~(static_cast<uint32_t>(v[j] >= static_cast<uint32_t>(A.card)) << j);
        dist_group_rows<0>(G, K, sel, static_cast<int32_t>(w * 32), v);
        dist_group_rows<16>(G, K, sel, static_cast<int32_t>(w * 32), v);
      },
      [&](int32_t row) PGX_SEL_OP {
        const uint32_t id = pgx_fwd_value(A.fwd, row, A.bits);
        const uint32_t s = sel_row_slot(G.g, K, row);
        if (id < static_cast<uint32_t>(A.card) && s < slots32) dist_mark(A.out + static_cast<size_t>(s) * bw, id);
      });
}

// ---- DISTINCTCOUNTMV: every value of every selected doc --------------------------------------------------------------
// Value rows lo .. lo + N - 1 of an item's value stream marked in bm, in passes of N independent accesses: the dictIds,
// the bitmap words, then the few atomics.  lo < hi <= total: rows at or past hi take row hi - 1's address and mark
// nothing, so no load is conditional.  pgx_fwd_value2 reads the row's dword and the next: for a row below `total` both
// lie inside the stream's allocation (whole tiles of rows and 64 bytes more).
template <int N>
__device__ __forceinline__ void dist_mv_batch(uint32_t* bm, const DistinctItem& A, uint32_t lo, uint32_t hi) {
  uint32_t v[N];
  const uint32_t card = static_cast<uint32_t>(A.card);  // >= 1 (sel_words)
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint32_t r = lo + static_cast<uint32_t>(i);
    const uint32_t on = static_cast<uint32_t>(static_cast<int32_t>(r - hi) >> 31);  // r < hi (both below 2^31 + N)
    const uint32_t id = pgx_fwd_value2(A.fwd, static_cast<int32_t>(__builtin_elementwise_min(r, hi - 1u)), A.bits);
    const uint32_t t = __builtin_elementwise_min(id, card), d = t - card;  // d == 0: a dictId at or past card
    const uint32_t m = static_cast<uint32_t>(static_cast<int32_t>(d | (0u - d)) >> 31) & on;
    v[i] = (t & m) | ~m;
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint32_t on = v[i] != kDistinctNone ? 0xFFFFFFFFu : 0u;
    const uint32_t id = v[i] & on;
    v[i] = id | ~on | (0u - ((bm[id >> 5] >> (id & 31u)) & 1u));
  }
#pragma unroll
  for (int i = 0; i < N; ++i)
    if (v[i] != kDistinctNone) atomicOr(&bm[v[i] >> 5], 1u << (v[i] & 31u));
}

// A run of consecutive selected docs owns one contiguous range of the value stream (sel_mv_walk).
__global__ void __launch_bounds__(kHllBlock) pgx_distinct_mark_mv(const DistinctMvItem* __restrict__ items,
                                                                  int nitems) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  __shared__ uint32_t lbits[kDistinctLdsWords];
  const DistinctMvItem M = items[item];
  const int words = sel_mv_words(M.d, M.start, M.total);
  if (words == 0) return;  // (the whole workgroup)
  const uint32_t bw = dist_bitmap_words(M.d.card);
  const auto scan = [&](uint32_t* bm) PGX_SEL_OP {
    sel_mv_walk(M.d, words, M.start, M.total, [&](auto n, uint32_t lo, uint32_t hi) PGX_SEL_OP {
      dist_mv_batch<decltype(n)::value>(bm, M.d, lo, hi);
    });
  };
  if (bw <= static_cast<uint32_t>(kDistinctLdsWords)) {
    for (uint32_t i = threadIdx.x; i < bw; i += kHllBlock) lbits[i] = 0u;
    __syncthreads();
    scan(lbits);
    __syncthreads();
    dist_flush(lbits, M.d.out, bw);
  } else {
    scan(M.d.out);
  }
}

// The same into the slots' rows in HBM: every value of a doc into the row of the doc's slot (sel_mv_group_walk).
template <class Key>
__global__ void __launch_bounds__(kHllBlock) pgx_distinct_mark_mv_group(const DistinctMvGroupItem* __restrict__ items,
                                                                        int nitems, const Key K) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  __shared__ uint32_t slot_of[32 * kHllBlock];
  const DistinctMvGroupItem& M = items[item];
  const DistinctItem A = M.g.d;
  const uint32_t bw = dist_bitmap_words(A.card);
  sel_mv_group_walk(A, M.g.g, K, M.start, M.total, slot_of,
                    [&](uint32_t s, auto n, uint32_t lo, uint32_t hi) PGX_SEL_OP {
                      dist_mv_batch<decltype(n)::value>(A.out + static_cast<size_t>(s) * bw, A, lo, hi);
                    });
}

// ---- the result's rows: sizes, then hash codes in dictId order -------------------------------------------------------
// word i of a row without the bits at and past card (the mark kernels never set them; a caller's table may)
__device__ __forceinline__ uint32_t dist_row_word(const uint32_t* __restrict__ row, uint32_t i, uint32_t bw,
                                                  uint32_t card) {
  const uint32_t b = row[i];
  const uint32_t left = card - i * 32u;  // >= 1 for i < bw
  return (i + 1u == bw && left < 32u) ? (b & ((1u << left) - 1u)) : b;
}

// x summed over the workgroup (every thread gets the sum); part: 4 words of LDS
__device__ __forceinline__ uint32_t dist_block_sum(uint32_t x, uint32_t* part) {
  for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d);
  __syncthreads();  // (the previous sum's readers are done with part)
  if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = x;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

// out[r] = set bits of table row rows[r] (a row outside 0 .. slots - 1: 0)
__global__ void __launch_bounds__(kHllBlock) pgx_distinct_count(const uint32_t* __restrict__ table, uint32_t card,
                                                                const int64_t* __restrict__ rows, int64_t nrows,
                                                                uint64_t slots, uint32_t* __restrict__ out) {
  __shared__ uint32_t part[4];
  const uint32_t bw = dist_bitmap_words(static_cast<int32_t>(card));
  for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    const int64_t s = rows[r];
    uint32_t n = 0u;
    if (s >= 0 && static_cast<uint64_t>(s) < slots) {
      const uint32_t* row = table + static_cast<size_t>(s) * bw;
      for (uint32_t i = threadIdx.x; i < bw; i += kHllBlock) n += __builtin_popcount(dist_row_word(row, i, bw, card));
    }
    n = dist_block_sum(n, part);
    if (threadIdx.x == 0) out[r] = n;
  }
}

// out[off[r] + k] = hash[the k-th set dictId of table row rows[r]], k ascending; nothing at or past index cap.  The
// gridDim.x workgroups of a row take one stretch of its words each (a multiple of 256 words); a workgroup first sums
// the popcounts of the words before its stretch, then takes the stretch 256 words at a time: an exclusive prefix of
// the words' popcounts (a scan inside each wave, then the waves' totals) gives every word its position.  The positions
// are a function of the row alone, so the order does not depend on the grid or the scheduling.
__global__ void __launch_bounds__(kHllBlock) pgx_distinct_emit(const uint32_t* __restrict__ table, uint32_t card,
                                                               const int64_t* __restrict__ rows,
                                                               const int64_t* __restrict__ off, int64_t nrows,
                                                               uint64_t slots, const int32_t* __restrict__ hash,
                                                               int32_t* __restrict__ out, int64_t cap) {
  __shared__ uint32_t wsum[4];
  const uint32_t bw = dist_bitmap_words(static_cast<int32_t>(card));
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t stretch = ((bw + gridDim.x - 1u) / gridDim.x + kHllBlock - 1u) / kHllBlock * kHllBlock;
  const uint64_t first64 = static_cast<uint64_t>(blockIdx.x) * stretch;
  if (first64 >= bw) return;  // (the whole workgroup)
  const uint32_t first = static_cast<uint32_t>(first64);
  const uint32_t last = bw - first < stretch ? bw : first + stretch;
  for (int64_t r = blockIdx.y; r < nrows; r += gridDim.y) {
    const int64_t s = rows[r];
    if (s < 0 || static_cast<uint64_t>(s) >= slots) continue;  // (the whole workgroup)
    const uint32_t* row = table + static_cast<size_t>(s) * bw;
    uint32_t before_stretch = 0u;
    for (uint32_t i = threadIdx.x; i < first; i += kHllBlock)
      before_stretch += __builtin_popcount(row[i]);  // (not the last word: no bits at or past card to drop)
    int64_t base = off[r] + dist_block_sum(before_stretch, wsum);
    for (uint32_t i0 = first; i0 < last; i0 += kHllBlock) {
      const uint32_t i = i0 + threadIdx.x;
      uint32_t b = i < bw ? dist_row_word(row, i, bw, card) : 0u;
      const uint32_t c = __builtin_popcount(b);
      uint32_t inc = c;
      for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
      }
      __syncthreads();  // (the previous step's readers are done with wsum)
      if (lane == 63u) wsum[wave] = inc;
      __syncthreads();
      uint32_t before = inc - c;
      for (uint32_t k = 0; k < wave; ++k) before += wsum[k];
      int64_t pos = base + before;
      while (b) {
        const uint32_t id = i * 32u + static_cast<uint32_t>(__builtin_ctz(b));
        b &= b - 1u;
        if (pos >= 0 && pos < cap) out[pos] = hash[id];
        ++pos;
      }
      base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
  }
}

}  // namespace pgx

static bool dist_item_ok(const pgx::DistinctItem& d) { return pgx::sel_item_ok(d, 1); }

// items: nitems descriptors in device memory; check: the caller's host copy of them, which is what gets validated.
// Every item's `out` holds (card + 31) / 32 words (the group forms: slots rows of them), zeroed or holding earlier marks.
extern "C" hipError_t pgx_launch_distinct_mark(const pgx::DistinctItem* items, const pgx::DistinctItem* check,
                                               int nitems, int wgs_per_item, hipStream_t stream) {
  return pgx::sel_launch(pgx::pgx_distinct_mark, items, check, nitems, wgs_per_item, stream, dist_item_ok);
}

extern "C" hipError_t pgx_launch_distinct_mark_group(const pgx::DistinctGroupItem* items,
                                                     const pgx::DistinctGroupItem* check, int nitems, int ngcols,
                                                     const uint64_t* gmul, int64_t slots, int wgs_per_item,
                                                     hipStream_t stream) {
  if (!pgx::sel_key_ok(ngcols, gmul, slots)) return hipErrorInvalidValue;
  return pgx::sel_launch(
      pgx::pgx_distinct_mark_group<pgx::HllGroupKey>, items, check, nitems, wgs_per_item, stream,
      [&](const pgx::DistinctGroupItem& g) { return dist_item_ok(g.d) && pgx::sel_gcols_host_ok(g.g, ngcols); },
      pgx::sel_key(ngcols, gmul, slots));
}

// The sparse forms: every item's `out` holds key->groups rows; key: the caller's host struct (pgx_hll.hip).
extern "C" hipError_t pgx_launch_distinct_mark_group_sparse(const pgx::DistinctGroupItem* items,
                                                            const pgx::DistinctGroupItem* check, int nitems,
                                                            const pgx::SelSparseKey* key, int wgs_per_item,
                                                            hipStream_t stream) {
  if (!pgx::sel_sparse_key_ok(key)) return hipErrorInvalidValue;
  const int ngcols = key->ngcols;
  return pgx::sel_launch(
      pgx::pgx_distinct_mark_group<pgx::SelSparseKey>, items, check, nitems, wgs_per_item, stream,
      [&](const pgx::DistinctGroupItem& g) { return dist_item_ok(g.d) && pgx::sel_gcols_host_ok(g.g, ngcols); }, *key);
}

// The start arrays are device data, so the kernels clamp every value range to `total`.
extern "C" hipError_t pgx_launch_distinct_mark_mv(const pgx::DistinctMvItem* items, const pgx::DistinctMvItem* check,
                                                  int nitems, int wgs_per_item, hipStream_t stream) {
  return pgx::sel_launch(
      pgx::pgx_distinct_mark_mv, items, check, nitems, wgs_per_item, stream,
      [](const pgx::DistinctMvItem& m) { return dist_item_ok(m.d) && pgx::sel_mv_ok(m.start, m.total); });
}

extern "C" hipError_t pgx_launch_distinct_mark_mv_group(const pgx::DistinctMvGroupItem* items,
                                                        const pgx::DistinctMvGroupItem* check, int nitems, int ngcols,
                                                        const uint64_t* gmul, int64_t slots, int wgs_per_item,
                                                        hipStream_t stream) {
  if (!pgx::sel_key_ok(ngcols, gmul, slots)) return hipErrorInvalidValue;
  return pgx::sel_launch(
      pgx::pgx_distinct_mark_mv_group<pgx::HllGroupKey>, items, check, nitems, wgs_per_item, stream,
      [&](const pgx::DistinctMvGroupItem& m) {
        return dist_item_ok(m.g.d) && pgx::sel_gcols_host_ok(m.g.g, ngcols) && pgx::sel_mv_ok(m.start, m.total);
      },
      pgx::sel_key(ngcols, gmul, slots));
}

extern "C" hipError_t pgx_launch_distinct_mark_mv_group_sparse(const pgx::DistinctMvGroupItem* items,
                                                               const pgx::DistinctMvGroupItem* check, int nitems,
                                                               const pgx::SelSparseKey* key, int wgs_per_item,
                                                               hipStream_t stream) {
  if (!pgx::sel_sparse_key_ok(key)) return hipErrorInvalidValue;
  const int ngcols = key->ngcols;
  return pgx::sel_launch(
      pgx::pgx_distinct_mark_mv_group<pgx::SelSparseKey>, items, check, nitems, wgs_per_item, stream,
      [&](const pgx::DistinctMvGroupItem& m) {
        return dist_item_ok(m.g.d) && pgx::sel_gcols_host_ok(m.g.g, ngcols) && pgx::sel_mv_ok(m.start, m.total);
      },
      *key);
}

// table: slots rows of (card + 31) / 32 words; rows: nrows row indexes (int64, device); counts: nrows u32 (device).
extern "C" hipError_t pgx_launch_distinct_count(const uint32_t* table, int32_t card, const int64_t* rows,
                                                int64_t nrows, int64_t slots, uint32_t* counts, int wgs,
                                                hipStream_t stream) {
  if (!table || !rows || !counts || card < 1 || nrows < 0 || nrows > pgx::kHllMaxGroupSlots || slots < 1 ||
      slots > pgx::kHllMaxGroupSlots || wgs < 1 || wgs > 65535)
    return hipErrorInvalidValue;
  if (nrows == 0) return hipSuccess;
  hipLaunchKernelGGL(pgx::pgx_distinct_count, dim3(static_cast<unsigned>(wgs)), dim3(pgx::kHllBlock), 0, stream, table,
                     static_cast<uint32_t>(card), rows, nrows, static_cast<uint64_t>(slots), counts);
  return hipGetLastError();
}

// off: nrows positions in `out` (int64, device), row r's codes go to out[off[r]] onwards; hash: card i32 per dictId;
// out: capacity i32, never written at or past it.  Grid: wgs_per_row x wgs.
extern "C" hipError_t pgx_launch_distinct_emit(const uint32_t* table, int32_t card, const int64_t* rows,
                                               const int64_t* off, int64_t nrows, int64_t slots, const int32_t* hash,
                                               int32_t* out, int64_t capacity, int wgs_per_row, int wgs,
                                               hipStream_t stream) {
  if (!table || !rows || !off || !hash || !out || card < 1 || nrows < 0 || nrows > pgx::kHllMaxGroupSlots ||
      slots < 1 || slots > pgx::kHllMaxGroupSlots || capacity < 0 || wgs < 1 || wgs > 65535 || wgs_per_row < 1 ||
      wgs_per_row > 1024)
    return hipErrorInvalidValue;
  if (nrows == 0 || capacity == 0) return hipSuccess;
  hipLaunchKernelGGL(pgx::pgx_distinct_emit, dim3(static_cast<unsigned>(wgs_per_row), static_cast<unsigned>(wgs)),
                     dim3(pgx::kHllBlock), 0, stream, table,
                     static_cast<uint32_t>(card), rows, off, nrows, static_cast<uint64_t>(slots), hash, out, capacity);
  return hipGetLastError();
}
