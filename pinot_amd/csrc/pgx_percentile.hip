// libpgx: PERCENTILE / PERCENTILEMV value histograms -- PercentileAggregationFunction (operator/aggregation/function/
// PercentileAggregationFunction.java: the selected docs' values collected into a DoubleArrayList;
// PercentileMVAggregationFunction.java: every value of every selected doc) over the selection bits the query kernels
// wrote.  Reference paths are relative to pinot-core/src/main/java/com/linkedin/pinot/core/.
//
// The list's order is lost at the reduce (query/aggregation/function/quantile/PercentileUtil.java:40-52 sorts it), so
// the intermediate is "how many selected rows hold each dictionary value": one u64 counter per dictId, under GROUP BY
// one row of `card` counters per slot.  Counters are only ever added to, with integer adds: every counter is exact
// whatever the grid size or the scheduling, and segments that share a dictionary add into the same table.  Unlike a
// presence mark an add cannot be skipped after a plain read, so small tables are summed on chip first.
//
//   pgx_percentile_count           grid (workgroups per item, items), one item per (segment, function).  A workgroup
//                                  strides over its item's 32-row mask words as pgx_distinct_mark does (zero words
//                                  skipped, words with 8 or more selected rows decoded whole, the others row by row).
//                                  A table of up to kPercentileLdsCounters counters is counted in LDS (u32: a workgroup
//                                  sees one item, an item has at most INT32_MAX rows or values) and its non-zero
//                                  counters are added into HBM at the end, one atomic each; for a larger one every
//                                  selected row is one 64-bit atomic add without return into HBM.
//   pgx_percentile_count_group     the same into table[slot * card + id]: slot = sum of the group columns' global ids
//                                  x gmul (column 0 least significant); LDS when slots x card fits.
//   pgx_percentile_count_mv        the column is multi-value: a run of consecutive selected docs of a mask word owns
//                                  one contiguous range of the value stream, clamped to the stream's row count.
//   pgx_percentile_count_mv_group  the same per doc, into the doc's slot's row.
//   pgx_percentile_sizes           non-zero counters of each listed row of a table.
//   pgx_percentile_emit            (dictId, count) of every non-zero counter of each listed row in ascending dictId
//                                  order, from the caller's offset for that row on.  Grid (workgroups per row, rows): a
//                                  workgroup takes one stretch of the row and counts the non-zero counters before it
//                                  itself, so positions are a function of the row alone.
// The walk over the selection bits is pgx_hll_device.h's; here are the adds it is handed, the result kernels and the
// launchers.  No workgroup waits on another; all stores are plain vector stores and vector atomics.
#include <hip/hip_runtime.h>

#include "pgx_device.h"
#include "pgx_hll_device.h"
#include "pgx_internal.h"

namespace pgx {

// one more in counter i: an LDS u32 (ds_add_u32) or an HBM u64 (global_atomic_add_x2), neither returns
__device__ __forceinline__ void pct_add(uint32_t* c, size_t i) { atomicAdd(c + i, 1u); }
__device__ __forceinline__ void pct_add_u64(uint64_t* c, size_t i, unsigned long long n) {
  __hip_atomic_fetch_add((PGX_G unsigned long long*)c + i, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void pct_add(uint64_t* c, size_t i) { pct_add_u64(c, i, 1ull); }

// the workgroup's LDS counters into the item's table: only those that counted something
__device__ __forceinline__ void pct_flush(const uint32_t* lc, uint64_t* out, uint32_t n) {
  for (uint32_t i = threadIdx.x; i < n; i += kHllBlock) {
    const uint32_t c = lc[i];
    if (c != 0u) pct_add_u64(out, i, c);
  }
}

__device__ __forceinline__ void pct_zero(uint32_t* lc, uint32_t n) {
  for (uint32_t i = threadIdx.x; i < n; i += kHllBlock) lc[i] = 0u;
  __syncthreads();
}

template <class C>
__device__ __forceinline__ void pct_scan(C* ctr, const PercentileItem& A, int words) {
  const uint32_t card = static_cast<uint32_t>(A.card);
  sel_walk(
      A, words,
      [&](int64_t w, uint32_t sel) PGX_SEL_OP {
        uint32_t v[32];
        pgx_fwd_decode_word(A.bits, A.fwd, w, v);  // the word's loads, issued together
#pragma unroll
        for (int j = 0; j < 32; ++j)
          if (((sel >> j) & 1u) != 0u && v[j] < card) pct_add(ctr, v[j]);
      },
      [&](int32_t row) PGX_SEL_OP {
        const uint32_t id = pgx_fwd_value(A.fwd, row, A.bits);
        if (id < card) pct_add(ctr, id);
      });
}

__global__ void __launch_bounds__(kHllBlock) pgx_percentile_count(const PercentileItem* __restrict__ items,
                                                                  int nitems) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  __shared__ uint32_t lc[kPercentileLdsCounters];
  const PercentileItem A = items[item];
  const int words = sel_words(A);
  if (words == 0) return;  // (the whole workgroup)
  const uint32_t card = static_cast<uint32_t>(A.card);
  if (card <= static_cast<uint32_t>(kPercentileLdsCounters)) {
    pct_zero(lc, card);
    pct_scan(lc, A, words);
    __syncthreads();
    pct_flush(lc, A.out, card);
  } else {
    pct_scan(A.out, A, words);
  }
}

// ---- GROUP BY: single-value group columns -> a dense slot ----------------------------------------------------------
// Rows J0 .. J0 + 15 of a mask word whose dictIds are decoded (v): slots, then the adds.  Half a word at a time, as in
// pgx_distinct_mark_group: 16 loads in flight per lane and pass.  The word's rows all lie inside the group columns'
// padded indexes, so the id loads are unconditional; a row that counts nothing takes remap entry 0.
template <int J0, class C, class Key>
__device__ __forceinline__ void pct_group_rows(C* ctr, const PercentileGroupItem& G, const Key& K, uint32_t sel,
                                               int32_t d0, const uint32_t (&v)[32]) {
  const uint32_t slots32 = sel_key_rows(K);  // <= kHllMaxGroupSlots, sparse: <= kSelMaxSparseGroups (launcher)
  const uint32_t card = static_cast<uint32_t>(G.d.card);
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
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (((sel >> (J0 + j)) & 1u) != 0u && s[j] < slots32 && v[J0 + j] < card)
      pct_add(ctr, static_cast<size_t>(s[j]) * card + v[J0 + j]);
}

template <class C, class Key>
__device__ __forceinline__ void pct_group_scan(C* ctr, const PercentileGroupItem& G, const Key& K, int words) {
  const PercentileItem& A = G.d;
  const uint32_t slots32 = sel_key_rows(K);
  const uint32_t card = static_cast<uint32_t>(A.card);
  sel_walk(
      A, words,
      [&](int64_t w, uint32_t sel) PGX_SEL_OP {
        uint32_t v[32];
        pgx_fwd_decode_word(A.bits, A.fwd, w, v);
        pct_group_rows<0>(ctr, G, K, sel, static_cast<int32_t>(w * 32), v);
        pct_group_rows<16>(ctr, G, K, sel, static_cast<int32_t>(w * 32), v);
      },
      [&](int32_t row) PGX_SEL_OP {
        const uint32_t id = pgx_fwd_value(A.fwd, row, A.bits);
        const uint32_t s = sel_row_slot(G.g, K, row);
        if (id < card && s < slots32) pct_add(ctr, static_cast<size_t>(s) * card + id);
      });
}

// counters of a group table when it is counted in LDS, else 0: rows <= 131072 and card < 2^31, so no overflow
__device__ __forceinline__ uint64_t pct_key_rows64(const HllGroupKey& K) { return K.slots; }
__device__ __forceinline__ uint64_t pct_key_rows64(const SelSparseKey& K) { return K.groups; }
template <class Key>
__device__ __forceinline__ uint32_t pct_lds_counters(const Key& K, int32_t card) {
  const uint64_t n = pct_key_rows64(K) * static_cast<uint64_t>(card > 0 ? card : 0);
  return n <= static_cast<uint64_t>(kPercentileLdsCounters) ? static_cast<uint32_t>(n) : 0u;
}

// Key: HllGroupKey or SelSparseKey (pgx_hll_offer_group); only the slot computation differs.
template <class Key>
__global__ void __launch_bounds__(kHllBlock) pgx_percentile_count_group(const PercentileGroupItem* __restrict__ items,
                                                                        int nitems, const Key K) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  __shared__ uint32_t lc[kPercentileLdsCounters];
  const PercentileGroupItem& G = items[item];
  const int words = sel_gcols_ok(G.g, K) ? sel_words(G.d) : 0;
  if (words == 0) return;  // (the whole workgroup)
  const uint32_t n = pct_lds_counters(K, G.d.card);
  if (n != 0u) {
    pct_zero(lc, n);
    pct_group_scan(lc, G, K, words);
    __syncthreads();
    pct_flush(lc, G.d.out, n);
  } else {
    pct_group_scan(G.d.out, G, K, words);
  }
}

// ---- PERCENTILEMV: every value of every selected doc -----------------------------------------------------------------
// Value rows lo .. lo + N - 1 of an item's value stream counted in ctr: N independent loads, then the adds.  lo < hi <=
// total: rows at or past hi take row hi - 1's address and count nothing, so no load is conditional.  pgx_fwd_value2
// reads the row's dword and the next: for a row below `total` both lie inside the stream's allocation.
template <int N, class C>
__device__ __forceinline__ void pct_mv_batch(C* ctr, const PercentileItem& A, uint32_t lo, uint32_t hi) {
  uint32_t v[N];
  const uint32_t card = static_cast<uint32_t>(A.card);  // >= 1 (sel_words)
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint32_t r = lo + static_cast<uint32_t>(i);
    v[i] = pgx_fwd_value2(A.fwd, static_cast<int32_t>(__builtin_elementwise_min(r, hi - 1u)), A.bits);
  }
#pragma unroll
  for (int i = 0; i < N; ++i)
    if (lo + static_cast<uint32_t>(i) < hi && v[i] < card) pct_add(ctr, v[i]);
}

__global__ void __launch_bounds__(kHllBlock) pgx_percentile_count_mv(const PercentileMvItem* __restrict__ items,
                                                                     int nitems) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  __shared__ uint32_t lc[kPercentileLdsCounters];
  const PercentileMvItem M = items[item];
  const int words = sel_mv_words(M.d, M.start, M.total);
  if (words == 0) return;  // (the whole workgroup)
  const uint32_t card = static_cast<uint32_t>(M.d.card);
  const auto scan = [&](auto* ctr) PGX_SEL_OP {
    sel_mv_walk(M.d, words, M.start, M.total, [&](auto n, uint32_t lo, uint32_t hi) PGX_SEL_OP {
      pct_mv_batch<decltype(n)::value>(ctr, M.d, lo, hi);
    });
  };
  if (card <= static_cast<uint32_t>(kPercentileLdsCounters)) {
    pct_zero(lc, card);
    scan(lc);
    __syncthreads();
    pct_flush(lc, M.d.out, card);
  } else {
    scan(M.d.out);
  }
}

// The same into the slots' rows: every value of a doc into the row of the doc's slot (sel_mv_group_walk).
template <class Key>
__global__ void __launch_bounds__(kHllBlock) pgx_percentile_count_mv_group(
    const PercentileMvGroupItem* __restrict__ items, int nitems, const Key K) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  __shared__ uint32_t slot_of[32 * kHllBlock];
  __shared__ uint32_t lc[kPercentileLdsCounters];
  const PercentileMvGroupItem& M = items[item];
  const PercentileItem A = M.g.d;
  const uint32_t card = static_cast<uint32_t>(A.card > 0 ? A.card : 0);
  const auto scan = [&](auto* ctr) PGX_SEL_OP {
    sel_mv_group_walk(A, M.g.g, K, M.start, M.total, slot_of,
                      [&](uint32_t s, auto n, uint32_t lo, uint32_t hi) PGX_SEL_OP {
                        pct_mv_batch<decltype(n)::value>(ctr + static_cast<size_t>(s) * card, A, lo, hi);
                      });
  };
  const uint32_t n = pct_lds_counters(K, A.card);
  if (n != 0u) {
    pct_zero(lc, n);
    scan(lc);
    __syncthreads();
    pct_flush(lc, A.out, n);
  } else {
    scan(A.out);
  }
}

// ---- the result's rows: sizes, then (dictId, count) pairs in dictId order ----------------------------------------------
// x summed over the workgroup (every thread gets the sum); part: 4 words of LDS
__device__ __forceinline__ uint32_t pct_block_sum(uint32_t x, uint32_t* part) {
  for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d);
  __syncthreads();  // (the previous sum's readers are done with part)
  if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = x;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

// out[r] = non-zero counters of table row rows[r] (a row outside 0 .. slots - 1: 0)
__global__ void __launch_bounds__(kHllBlock) pgx_percentile_sizes(const uint64_t* __restrict__ table, uint32_t card,
                                                                  const int64_t* __restrict__ rows, int64_t nrows,
                                                                  uint64_t slots, uint32_t* __restrict__ out) {
  __shared__ uint32_t part[4];
  for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    const int64_t s = rows[r];
    uint32_t n = 0u;
    if (s >= 0 && static_cast<uint64_t>(s) < slots) {
      const uint64_t* row = table + static_cast<size_t>(s) * card;
#pragma unroll 8  // (a long row is read by one workgroup: eight independent loads in flight per thread)
      for (uint32_t i = threadIdx.x; i < card; i += kHllBlock) n += row[i] != 0u ? 1u : 0u;
    }
    n = pct_block_sum(n, part);
    if (threadIdx.x == 0) out[r] = n;
  }
}

// ids[off[r] + k], counts[off[r] + k] = the k-th non-zero counter of table row rows[r] and its dictId, k ascending;
// nothing at or past index cap.  The gridDim.x workgroups of a row take one stretch of its counters each (a multiple of
// 256); a workgroup first counts the non-zero counters before its stretch, then takes the stretch 256 counters at a
// time: a ballot inside each wave and the waves' totals give every counter its position.
__global__ void __launch_bounds__(kHllBlock) pgx_percentile_emit(const uint64_t* __restrict__ table, uint32_t card,
                                                                 const int64_t* __restrict__ rows,
                                                                 const int64_t* __restrict__ off, int64_t nrows,
                                                                 uint64_t slots, int32_t* __restrict__ ids,
                                                                 uint64_t* __restrict__ counts, int64_t cap) {
  __shared__ uint32_t wsum[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t per = (static_cast<uint64_t>(card) + gridDim.x - 1u) / gridDim.x;
  const uint64_t stretch = (per + kHllBlock - 1u) / kHllBlock * kHllBlock;
  const uint64_t first64 = static_cast<uint64_t>(blockIdx.x) * stretch;
  if (first64 >= card) return;  // (the whole workgroup)
  const uint32_t first = static_cast<uint32_t>(first64);
  const uint32_t last = card - first < stretch ? card : first + static_cast<uint32_t>(stretch);
  for (int64_t r = blockIdx.y; r < nrows; r += gridDim.y) {
    const int64_t s = rows[r];
    if (s < 0 || static_cast<uint64_t>(s) >= slots) continue;  // (the whole workgroup)
    const uint64_t* row = table + static_cast<size_t>(s) * card;
    uint32_t before_stretch = 0u;
#pragma unroll 8  // (first is a multiple of 256: eight independent loads in flight per thread)
    for (uint32_t i = threadIdx.x; i < first; i += kHllBlock) before_stretch += row[i] != 0u ? 1u : 0u;
    int64_t base = off[r] + pct_block_sum(before_stretch, wsum);
    for (uint32_t i0 = first; i0 < last; i0 += kHllBlock) {
      const uint32_t i = i0 + threadIdx.x;  // (i0 < card <= INT32_MAX: no wrap)
      const uint64_t c = i < last ? row[i] : 0u;
      const unsigned long long b = __ballot(c != 0u);
      __syncthreads();  // (the previous step's readers are done with wsum)
      if (lane == 0u) wsum[wave] = static_cast<uint32_t>(__popcll(b));
      __syncthreads();
      uint32_t before = static_cast<uint32_t>(__popcll(b & ((1ull << lane) - 1ull)));
      for (uint32_t k = 0; k < wave; ++k) before += wsum[k];
      const int64_t pos = base + before;
      if (c != 0u && pos >= 0 && pos < cap) {
        ids[pos] = static_cast<int32_t>(i);
        counts[pos] = c;
      }
      base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
  }
}

}  // namespace pgx

static bool pct_item_ok(const pgx::PercentileItem& d) { return pgx::sel_item_ok(d, 1); }

// items: nitems descriptors in device memory; check: the caller's host copy of them, which is what gets validated.
// Every item's `out` holds card u64 counters (the group forms: slots rows of them), zeroed or holding earlier counts.
extern "C" hipError_t pgx_launch_percentile_count(const pgx::PercentileItem* items, const pgx::PercentileItem* check,
                                                  int nitems, int wgs_per_item, hipStream_t stream) {
  return pgx::sel_launch(pgx::pgx_percentile_count, items, check, nitems, wgs_per_item, stream, pct_item_ok);
}

extern "C" hipError_t pgx_launch_percentile_count_group(const pgx::PercentileGroupItem* items,
                                                        const pgx::PercentileGroupItem* check, int nitems, int ngcols,
                                                        const uint64_t* gmul, int64_t slots, int wgs_per_item,
                                                        hipStream_t stream) {
  if (!pgx::sel_key_ok(ngcols, gmul, slots)) return hipErrorInvalidValue;
  return pgx::sel_launch(
      pgx::pgx_percentile_count_group<pgx::HllGroupKey>, items, check, nitems, wgs_per_item, stream,
      [&](const pgx::PercentileGroupItem& g) { return pct_item_ok(g.d) && pgx::sel_gcols_host_ok(g.g, ngcols); },
      pgx::sel_key(ngcols, gmul, slots));
}

// The sparse forms: every item's `out` holds key->groups rows; key: the caller's host struct (pgx_hll.hip).
extern "C" hipError_t pgx_launch_percentile_count_group_sparse(const pgx::PercentileGroupItem* items,
                                                               const pgx::PercentileGroupItem* check, int nitems,
                                                               const pgx::SelSparseKey* key, int wgs_per_item,
                                                               hipStream_t stream) {
  if (!pgx::sel_sparse_key_ok(key)) return hipErrorInvalidValue;
  const int ngcols = key->ngcols;
  return pgx::sel_launch(
      pgx::pgx_percentile_count_group<pgx::SelSparseKey>, items, check, nitems, wgs_per_item, stream,
      [&](const pgx::PercentileGroupItem& g) { return pct_item_ok(g.d) && pgx::sel_gcols_host_ok(g.g, ngcols); },
      *key);
}

// The start arrays are device data, so the kernels clamp every value range to `total`.
extern "C" hipError_t pgx_launch_percentile_count_mv(const pgx::PercentileMvItem* items,
                                                     const pgx::PercentileMvItem* check, int nitems, int wgs_per_item,
                                                     hipStream_t stream) {
  return pgx::sel_launch(
      pgx::pgx_percentile_count_mv, items, check, nitems, wgs_per_item, stream,
      [](const pgx::PercentileMvItem& m) { return pct_item_ok(m.d) && pgx::sel_mv_ok(m.start, m.total); });
}

extern "C" hipError_t pgx_launch_percentile_count_mv_group(const pgx::PercentileMvGroupItem* items,
                                                           const pgx::PercentileMvGroupItem* check, int nitems,
                                                           int ngcols, const uint64_t* gmul, int64_t slots,
                                                           int wgs_per_item, hipStream_t stream) {
  if (!pgx::sel_key_ok(ngcols, gmul, slots)) return hipErrorInvalidValue;
  return pgx::sel_launch(
      pgx::pgx_percentile_count_mv_group<pgx::HllGroupKey>, items, check, nitems, wgs_per_item, stream,
      [&](const pgx::PercentileMvGroupItem& m) {
        return pct_item_ok(m.g.d) && pgx::sel_gcols_host_ok(m.g.g, ngcols) && pgx::sel_mv_ok(m.start, m.total);
      },
      pgx::sel_key(ngcols, gmul, slots));
}

extern "C" hipError_t pgx_launch_percentile_count_mv_group_sparse(const pgx::PercentileMvGroupItem* items,
                                                                  const pgx::PercentileMvGroupItem* check,
                                                                  int nitems, const pgx::SelSparseKey* key,
                                                                  int wgs_per_item, hipStream_t stream) {
  if (!pgx::sel_sparse_key_ok(key)) return hipErrorInvalidValue;
  const int ngcols = key->ngcols;
  return pgx::sel_launch(
      pgx::pgx_percentile_count_mv_group<pgx::SelSparseKey>, items, check, nitems, wgs_per_item, stream,
      [&](const pgx::PercentileMvGroupItem& m) {
        return pct_item_ok(m.g.d) && pgx::sel_gcols_host_ok(m.g.g, ngcols) && pgx::sel_mv_ok(m.start, m.total);
      },
      *key);
}

// table: slots rows of card u64 counters; rows: nrows row indexes (int64, device); sizes: nrows u32 (device).
extern "C" hipError_t pgx_launch_percentile_sizes(const uint64_t* table, int32_t card, const int64_t* rows,
                                                  int64_t nrows, int64_t slots, uint32_t* sizes, int wgs,
                                                  hipStream_t stream) {
  if (!table || !rows || !sizes || card < 1 || nrows < 0 || nrows > pgx::kHllMaxGroupSlots || slots < 1 ||
      slots > pgx::kHllMaxGroupSlots || wgs < 1 || wgs > 65535)
    return hipErrorInvalidValue;
  if (nrows == 0) return hipSuccess;
  hipLaunchKernelGGL(pgx::pgx_percentile_sizes, dim3(static_cast<unsigned>(wgs)), dim3(pgx::kHllBlock), 0, stream,
                     table, static_cast<uint32_t>(card), rows, nrows, static_cast<uint64_t>(slots), sizes);
  return hipGetLastError();
}

// off: nrows positions (int64, device), row r's pairs go to ids[off[r]], counts[off[r]] onwards; ids: capacity i32,
// counts: capacity u64, neither ever written at or past it.  Grid: wgs_per_row x wgs.
extern "C" hipError_t pgx_launch_percentile_emit(const uint64_t* table, int32_t card, const int64_t* rows,
                                                 const int64_t* off, int64_t nrows, int64_t slots, int32_t* ids,
                                                 uint64_t* counts, int64_t capacity, int wgs_per_row, int wgs,
                                                 hipStream_t stream) {
  if (!table || !rows || !off || !ids || !counts || card < 1 || nrows < 0 || nrows > pgx::kHllMaxGroupSlots ||
      slots < 1 || slots > pgx::kHllMaxGroupSlots || capacity < 0 || wgs < 1 || wgs > 65535 || wgs_per_row < 1 ||
      wgs_per_row > 1024)
    return hipErrorInvalidValue;
  if (nrows == 0 || capacity == 0) return hipSuccess;
  hipLaunchKernelGGL(pgx::pgx_percentile_emit, dim3(static_cast<unsigned>(wgs_per_row), static_cast<unsigned>(wgs)),
                     dim3(pgx::kHllBlock), 0, stream, table, static_cast<uint32_t>(card), rows, off, nrows,
                     static_cast<uint64_t>(slots), ids, counts, capacity);
  return hipGetLastError();
}
