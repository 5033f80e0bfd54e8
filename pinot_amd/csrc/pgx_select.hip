// libpgx: selection with ORDER BY -- the per-segment top-K of MSelectionOrderByOperator (operator/MSelectionOrderByOperator
// .java, query/selection/SelectionOperatorService.java: a PriorityQueue of offset + size docs under
// CompositeDocIdValComparator) over the selection bits the query kernels wrote.  Reference paths are relative to
// pinot-core/src/main/java/com/linkedin/pinot/core/.
//
// A row's key is its order columns' dictIds (v1 dictionaries are sorted: dictId order is value order inside a segment;
// DESC columns take card - 1 - id), concatenated most-significant first into one u64.  Rows rank by (key, docId)
// ascending, smaller is better: a total order, so the K best rows are one set whatever the grid size or scheduling.
//
//   pgx_select_topk    grid (workgroups per item, items).  A workgroup strides over its item's 32-row mask words, one
//                      word per thread and step.  It keeps candidates in LDS (C = max(2 * pow2(K), 512) entries of
//                      u64 key + u32 doc) and a threshold, the K-th best entry so far.  Rows are first tested in
//                      registers, on the first order column alone where that decides; only survivors take part in the
//                      appends.  When fewer than 256 free entries are left the buffer is bitonic-sorted, cut to K and
//                      the threshold lowered.  Each workgroup writes its <= K candidates, best first, and their count
//                      to its own slot of a global scratch.
//   pgx_select_merge   one workgroup per item: the same buffer over the item's candidate lists; writes the final <= K
//                      docIds best first and their count.
//   pgx_select_gather  one thread per (schema column, item, rank): the selected doc's dictId.
//
// Multi-value schema columns (SelectionFetcher's *ArraySelectionColumnIterator: every value of the doc, in the doc's
// own order) take three more launches after the merge, over the pairs (multi-value column m, item i) = m * nitems + i:
//   pgx_select_mv_offsets  one workgroup per pair: the value counts start[d + 1] - start[d] of the item's <= K docs,
//                          scanned exclusively into K + 1 offsets relative to the pair, and the pair's total.
//   pgx_select_mv_bases    one workgroup: the exclusive scan of the pairs' totals into int64 bases and the grand total.
//   pgx_select_mv_gather   one or several workgroups per pair, the pair's offsets in LDS: one output value per thread
//                          and step -- the thread finds the value's rank by binary search, reads the value from the
//                          doc's range of the stream and stores it at base + j (consecutive threads, consecutive j).
// No workgroup waits on another; all stores are plain vector stores.
//
// Selection without ORDER BY (MSelectionOnlyOperator) replaces the top-K and the merge by pgx_select_first_count /
// pgx_select_first, described where they are defined; the gather and the multi-value launches run unchanged after them.
#include <hip/hip_runtime.h>

#include "pgx_device.h"
#include "pgx_internal.h"

namespace pgx {

__device__ __forceinline__ uint64_t sel_key(const SelItem& A, int32_t doc) {
  uint64_t key = 0;
  for (int c = 0; c < A.ncols; ++c) {
    const SelCol& col = A.c[c];
    uint32_t v = pgx_fwd_value(col.fwd, doc, col.bits);
    if (col.desc) v = col.card - 1u - v;
    key = (key << col.kbits) | v;
  }
  return key;
}

__device__ __forceinline__ bool sel_less(uint64_t ka, uint32_t da, uint64_t kb, uint32_t db) {
  return ka < kb || (ka == kb && da < db);
}

constexpr int kSelDenseRows = 8;  // selected rows of a mask word from which the whole word's column is decoded

// Candidate buffer of one workgroup.  An empty entry is (~0, ~0): worse than every row (docIds are below 2^31).
struct SelBuf {
  uint64_t* keys;
  uint32_t* docs;
  int* count;       // entries held (LDS)
  uint64_t* thrk;   // threshold (LDS): a row must be better than (thrk, thrd) to enter
  uint32_t* thrd;
  int C, K;
};

// Sort the n held entries, keep the best K, lower the threshold.  Called by every thread with the same n, after a
// barrier that follows the last append.
__device__ void sel_sort_cut(const SelBuf& B, int n) {
  const int tid = static_cast<int>(threadIdx.x);
  int P = 2;  // the power of two that holds the n entries (<= C): the bitonic network's size
  while (P < n) P <<= 1;
  for (int i = n + tid; i < P; i += kSelBlock) {
    B.keys[i] = ~0ull;
    B.docs[i] = ~0u;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += kSelBlock) {
        const int x = i ^ j;
        if (x > i) {
          const uint64_t ka = B.keys[i], kb = B.keys[x];
          const uint32_t da = B.docs[i], db = B.docs[x];
          const bool up = (i & k) == 0;
          if (sel_less(kb, db, ka, da) == up) {
            B.keys[i] = kb;
            B.docs[i] = db;
            B.keys[x] = ka;
            B.docs[x] = da;
          }
        }
      }
      __syncthreads();
    }
  if (tid == 0) {
    const int m = n < B.K ? n : B.K;
    *B.count = m;
    if (m == B.K) {
      *B.thrk = B.keys[B.K - 1];
      *B.thrd = B.docs[B.K - 1];
    }
  }
  __syncthreads();
}

// One append round: every thread offers at most one row.  Called by every thread, after a barrier that follows the
// last append; (thrk, thrd) is the thread's register copy of the threshold.
__device__ __forceinline__ void sel_offer(const SelBuf& B, bool has, uint64_t key, uint32_t doc, uint64_t& thrk,
                                          uint32_t& thrd) {
  const int n = *B.count;
  __syncthreads();  // every thread has read the count before any append changes it
  if (n + kSelBlock > B.C) {
    sel_sort_cut(B, n);
    thrk = *B.thrk;
    thrd = *B.thrd;
  }
  if (has && sel_less(key, doc, thrk, thrd)) {
    const int slot = atomicAdd(B.count, 1);  // < C: at most 256 appends per round
    B.keys[slot] = key;
    B.docs[slot] = doc;
  }
}

#define PGX_SEL_BUF(B, C_, K_)                                   \
  extern __shared__ uint64_t sel_smem[];                         \
  __shared__ int sel_count;                                      \
  __shared__ uint64_t sel_thrk;                                  \
  __shared__ uint32_t sel_thrd;                                  \
  SelBuf B;                                                      \
  B.keys = sel_smem;                                             \
  B.docs = reinterpret_cast<uint32_t*>(sel_smem + (C_));         \
  B.count = &sel_count;                                          \
  B.thrk = &sel_thrk;                                            \
  B.thrd = &sel_thrd;                                            \
  B.C = (C_);                                                    \
  B.K = (K_);                                                    \
  if (threadIdx.x == 0) {                                        \
    sel_count = 0;                                               \
    sel_thrk = ~0ull;                                            \
    sel_thrd = ~0u;                                              \
  }                                                              \
  __syncthreads();

__global__ void __launch_bounds__(kSelBlock) pgx_select_topk(const SelItem* __restrict__ items, int nitems, int K, int C,
                                                             uint64_t* __restrict__ cand_key,
                                                             uint32_t* __restrict__ cand_doc,
                                                             int32_t* __restrict__ cand_cnt) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  PGX_SEL_BUF(B, C, K)
  __shared__ uint32_t sel_mins[kSelBlock];
  __shared__ uint32_t sel_seed;
  const SelItem& A = items[item];
  const int tid = static_cast<int>(threadIdx.x);
  const int G = static_cast<int>(gridDim.x), wg = static_cast<int>(blockIdx.x);
  const int num_docs = A.num_docs;
  // the mask's spare word and the bits past num_docs are never used; an item without a valid column list has no rows
  const int words = A.ncols >= 1 && A.ncols <= kSelMaxOrderCols ? (num_docs + 31) >> 5 : 0;
  uint64_t thrk = ~0ull;
  uint32_t thrd = ~0u;
  // the first order column, and where its field sits in the key
  const uint32_t* __restrict__ c0fwd = A.c[0].fwd;
  const int c0bits = A.c[0].bits;
  const uint32_t c0card = A.c[0].card;
  const bool c0desc = A.c[0].desc != 0;
  int sh0 = 0;
  for (int c = 1; c < A.ncols; ++c) sh0 += A.c[c].kbits;
  const int64_t stride = static_cast<int64_t>(G) * kSelBlock;
  const int64_t w_first = static_cast<int64_t>(wg) * kSelBlock + tid;
  uint32_t sel_ahead = w_first < words ? A.sel[w_first] : 0u;  // each step loads the next step's mask word
  for (int64_t base = static_cast<int64_t>(wg) * kSelBlock; base < words; base += stride) {
    const int64_t w = base + tid;
    uint32_t sel = sel_ahead;
    sel_ahead = w + stride < words ? A.sel[w + stride] : 0u;
    int32_t d0 = 0;
    if (w < words) {
      d0 = static_cast<int32_t>(w * 32);
      if (num_docs - d0 < 32) sel &= (1u << (num_docs - d0)) - 1u;
    }
    // Rows that beat the threshold as this thread knows it (no barrier once the threshold is set: after the first
    // steps nearly every row ends here).  The first order column decides for most rows: its value x (card - 1 - id
    // for DESC) against the threshold key's leading field t0 -- x < t0 beats it, x > t0 does not, and only x == t0
    // needs the whole key.  Words with many selected rows decode the column's 32 values at once; sparse words read
    // their rows one by one.
    const bool dense = __builtin_popcount(sel) >= kSelDenseRows;
    uint32_t v[32];
    if (dense) {
      pgx_fwd_decode_word(c0bits, c0fwd, w, v);
#pragma unroll
      for (int j = 0; j < 32; ++j) v[j] = c0desc ? c0card - 1u - v[j] : v[j];
    }
    const uint64_t t0w = thrk >> sh0;
    uint32_t t0 = t0w > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(t0w);
    // No threshold yet (the buffer never held K rows): without one, every selected row of the step would go through
    // the append rounds.  A bound from this step's rows alone: the K-th smallest of the threads' minima of x -- K
    // rows are at or below it, so no row above it is among the best K.  (K <= 256 threads; ~0 = no bound.)
    const bool seed = thrk == ~0ull && thrd == ~0u && K <= kSelBlock;  // the same in every thread
    if (seed) {
      uint32_t mn = ~0u;
      if (dense) {
#pragma unroll
        for (int j = 0; j < 32; ++j) mn = ((sel >> j) & 1u) && v[j] < mn ? v[j] : mn;
      } else {
        for (uint32_t m = sel; m;) {
          const int k = __builtin_ctz(m);
          m &= m - 1u;
          uint32_t x = pgx_fwd_value(c0fwd, d0 + k, c0bits);
          if (c0desc) x = c0card - 1u - x;
          mn = x < mn ? x : mn;
        }
      }
      sel_mins[tid] = mn;
      __syncthreads();
      int rank = 0;  // of this thread's minimum among the 256, ties by thread: ranks are distinct
      for (int j = 0; j < kSelBlock; ++j) {
        const uint32_t o = sel_mins[j];
        rank += static_cast<int>(o < mn || (o == mn && j < tid));
      }
      if (rank == K - 1) sel_seed = mn;
      __syncthreads();  // (the next write of sel_mins follows the barriers of the append rounds below)
      t0 = sel_seed;
    }
    uint32_t surv = 0u, eq = 0u;
    if (dense) {
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        surv |= static_cast<uint32_t>(v[j] < t0) << j;
        eq |= static_cast<uint32_t>(v[j] == t0) << j;
      }
      surv &= sel;
      eq &= sel;
    } else {
      for (uint32_t m = sel; m;) {
        const int k = __builtin_ctz(m);
        m &= m - 1u;
        uint32_t x = pgx_fwd_value(c0fwd, d0 + k, c0bits);
        if (c0desc) x = c0card - 1u - x;
        surv |= static_cast<uint32_t>(x < t0) << k;
        eq |= static_cast<uint32_t>(x == t0) << k;
      }
    }
    if (seed) {
      surv |= eq;  // no threshold to compare whole keys with
    } else {
      for (uint32_t m = eq; m;) {
        const int k = __builtin_ctz(m);
        m &= m - 1u;
        if (sel_less(sel_key(A, d0 + k), static_cast<uint32_t>(d0 + k), thrk, thrd)) surv |= 1u << k;
      }
    }
    while (__syncthreads_or(surv != 0u)) {
      const bool has = surv != 0u;
      uint64_t key = 0;
      uint32_t doc = 0;
      if (has) {
        const int k = __builtin_ctz(surv);
        surv &= surv - 1u;
        doc = static_cast<uint32_t>(d0 + k);
        key = sel_key(A, d0 + k);
      }
      sel_offer(B, has, key, doc, thrk, thrd);
    }
    if (thrk == ~0ull && thrd == ~0u) {  // still no threshold: set one as soon as K rows are held
      const int held = *B.count;
      __syncthreads();
      if (held >= K) {
        sel_sort_cut(B, held);
        thrk = *B.thrk;
        thrd = *B.thrd;
      }
    }
  }
  __syncthreads();
  const int n = *B.count;
  __syncthreads();
  sel_sort_cut(B, n);
  const int m = *B.count;
  const int64_t slot = static_cast<int64_t>(item) * G + wg;
  for (int i = tid; i < m; i += kSelBlock) {
    cand_key[slot * K + i] = B.keys[i];
    cand_doc[slot * K + i] = B.docs[i];
  }
  if (tid == 0) cand_cnt[slot] = m;
}

__global__ void __launch_bounds__(kSelBlock) pgx_select_merge(int nitems, int K, int C, int G,
                                                              const uint64_t* __restrict__ cand_key,
                                                              const uint32_t* __restrict__ cand_doc,
                                                              const int32_t* __restrict__ cand_cnt,
                                                              int32_t* __restrict__ out_doc,
                                                              int32_t* __restrict__ out_cnt) {
  const int item = static_cast<int>(blockIdx.x);
  if (item >= nitems) return;
  PGX_SEL_BUF(B, C, K)
  const int tid = static_cast<int>(threadIdx.x);
  uint64_t thrk = ~0ull;
  uint32_t thrd = ~0u;
  // the item's G lists as one array of G * K slots, 256 per step; slot p of list g holds a row when p < cand_cnt[g]
  const int64_t first = static_cast<int64_t>(item) * G;
  const int total = G * K;
  for (int i0 = 0; i0 < total; i0 += kSelBlock) {
    const int i = i0 + tid;
    bool has = false;
    uint64_t key = 0;
    uint32_t doc = 0;
    if (i < total) {
      const int g = i / K, p = i - g * K;
      if (p < cand_cnt[first + g]) {
        has = true;
        key = cand_key[first * K + i];
        doc = cand_doc[first * K + i];
      }
    }
    if (__syncthreads_or(has && sel_less(key, doc, thrk, thrd))) sel_offer(B, has, key, doc, thrk, thrd);
  }
  __syncthreads();
  const int n = *B.count;
  __syncthreads();
  sel_sort_cut(B, n);
  const int m = *B.count;
  for (int i = tid; i < m; i += kSelBlock) out_doc[static_cast<int64_t>(item) * K + i] = static_cast<int32_t>(B.docs[i]);
  if (tid == 0) out_cnt[item] = m;
}

__global__ void __launch_bounds__(kSelBlock) pgx_select_gather(const SelGatherCol* __restrict__ cols, int nitems,
                                                               int ncols, int K, const int32_t* __restrict__ out_doc,
                                                               const int32_t* __restrict__ out_cnt,
                                                               int32_t* __restrict__ out_ids) {
  const int64_t rows = static_cast<int64_t>(nitems) * K;
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kSelBlock + threadIdx.x;
  if (idx >= rows * ncols) return;
  const int64_t row = idx % rows;
  const int c = static_cast<int>(idx / rows);
  const int item = static_cast<int>(row / K), rank = static_cast<int>(row % K);
  if (rank >= out_cnt[item]) return;  // ranks past the count keep what the caller put there
  const SelGatherCol col = cols[static_cast<int64_t>(item) * ncols + c];
  out_ids[idx] = static_cast<int32_t>(pgx_fwd_value(col.fwd, out_doc[row], col.bits));
}

// ---- multi-value schema columns ---------------------------------------------------------------------------------------
// Exclusive prefix sum of one value per thread over the workgroup (scan: kSelBlock entries of LDS, free again on
// return); total: the sum of all.  Called by every thread.
template <class T>
__device__ __forceinline__ T sel_block_scan(T v, T* scan, T& total) {
  const int tid = static_cast<int>(threadIdx.x);
  scan[tid] = v;
  __syncthreads();
  for (int d = 1; d < kSelBlock; d <<= 1) {
    const T add = tid >= d ? scan[tid - d] : T(0);
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  total = scan[kSelBlock - 1];
  const T incl = scan[tid];
  __syncthreads();
  return incl - v;
}

constexpr int kSelMvRanks = 8;  // ranks per thread of pgx_select_mv_offsets: K <= 2048 = 8 * kSelBlock

// The item's row count as the merge wrote it, kept inside [0, K]: no rank past it is ever read as a doc.
__device__ __forceinline__ int sel_mv_count(const int32_t* __restrict__ out_cnt, int item, int K) {
  const int c = out_cnt[item];
  return c < 0 ? 0 : (c > K ? K : c);
}

__global__ void __launch_bounds__(kSelBlock) pgx_select_mv_offsets(const SelMvCol* __restrict__ cols, int nitems, int nmv,
                                                                   int K, const int32_t* __restrict__ out_doc,
                                                                   const int32_t* __restrict__ out_cnt,
                                                                   int32_t* __restrict__ rel_off,
                                                                   int32_t* __restrict__ totals) {
  const int64_t pair = static_cast<int64_t>(blockIdx.x);
  if (pair >= static_cast<int64_t>(nitems) * nmv) return;
  __shared__ int32_t scan[kSelBlock];
  const int tid = static_cast<int>(threadIdx.x);
  const int item = static_cast<int>(pair % nitems);
  const int32_t* __restrict__ start = cols[pair].start;
  const int cnt = sel_mv_count(out_cnt, item, K);
  // thread t owns the ranks t * E ... t * E + E - 1: one scan over the threads' sums serves all K ranks
  const int E = (K + kSelBlock - 1) / kSelBlock;
  int32_t len[kSelMvRanks];
  int32_t sum = 0;
#pragma unroll
  for (int i = 0; i < kSelMvRanks; ++i) {
    const int r = tid * E + i;
    len[i] = 0;
    if (i < E && r < cnt) {
      const int32_t d = out_doc[static_cast<int64_t>(item) * K + r];
      len[i] = start[d + 1] - start[d];
    }
    sum += len[i];
  }
  int32_t total;
  int32_t at = sel_block_scan<int32_t>(sum, scan, total);
  int32_t* __restrict__ off = rel_off + pair * (K + 1);
#pragma unroll
  for (int i = 0; i < kSelMvRanks; ++i) {
    const int r = tid * E + i;
    if (i < E && r < K) off[r] = at;  // ranks at or past the count hold the total: they own no value
    at += len[i];
  }
  if (tid == 0) {
    off[K] = total;
    totals[pair] = total;
  }
}

__global__ void __launch_bounds__(kSelBlock) pgx_select_mv_bases(const int32_t* __restrict__ totals, int64_t npairs,
                                                                 int64_t* __restrict__ bases) {
  if (blockIdx.x != 0) return;
  __shared__ int64_t scan[kSelBlock];
  const int tid = static_cast<int>(threadIdx.x);
  int64_t carry = 0;
  for (int64_t i0 = 0; i0 < npairs; i0 += kSelBlock) {
    const int64_t i = i0 + tid;
    const int64_t v = i < npairs ? totals[i] : 0;
    int64_t step;
    const int64_t at = sel_block_scan<int64_t>(v, scan, step);
    if (i < npairs) bases[i] = carry + at;
    carry += step;
  }
  if (tid == 0) bases[npairs] = carry;
}

__global__ void __launch_bounds__(kSelBlock) pgx_select_mv_gather(const SelMvCol* __restrict__ cols, int nitems, int nmv,
                                                                  int K, int G, const int32_t* __restrict__ out_doc,
                                                                  const int32_t* __restrict__ out_cnt,
                                                                  const int32_t* __restrict__ rel_off,
                                                                  const int64_t* __restrict__ bases,
                                                                  int32_t* __restrict__ values, int64_t capacity) {
  extern __shared__ int32_t sel_mv_smem[];  // off[K + 1], then per rank start[doc] - off[rank]
  const int64_t pair = static_cast<int64_t>(blockIdx.x) / G;
  const int wg = static_cast<int>(static_cast<int64_t>(blockIdx.x) % G);
  if (pair >= static_cast<int64_t>(nitems) * nmv) return;
  const int tid = static_cast<int>(threadIdx.x);
  const int32_t* __restrict__ goff = rel_off + pair * (K + 1);
  const int32_t total = goff[K];
  if (static_cast<int64_t>(wg) * kSelBlock >= total) return;  // the whole workgroup: nothing of the pair is left for it
  const int item = static_cast<int>(pair % nitems);
  const SelMvCol col = cols[pair];
  const int cnt = sel_mv_count(out_cnt, item, K);
  int32_t* off = sel_mv_smem;
  int32_t* delta = sel_mv_smem + K + 1;
  for (int r = tid; r <= K; r += kSelBlock) {
    const int32_t o = goff[r];
    off[r] = o;
    if (r < K) delta[r] = r < cnt ? col.start[out_doc[static_cast<int64_t>(item) * K + r]] - o : 0;
  }
  __syncthreads();
  const int64_t base = bases[pair];
  for (int64_t j = static_cast<int64_t>(wg) * kSelBlock + tid; j < total; j += static_cast<int64_t>(G) * kSelBlock) {
    // the rank that owns value j: the last r with off[r] <= j (off[0] = 0 <= j < total = off[K]; a doc without
    // values shares its offset with the next rank and is passed over)
    int lo = 0, hi = K;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (off[mid] <= j) lo = mid; else hi = mid;
    }
    if (base + j < capacity)
      values[base + j] = static_cast<int32_t>(pgx_fwd_value2(col.values, static_cast<int64_t>(delta[lo]) + j, col.bits));
  }
}

// ---- selection without ORDER BY ---------------------------------------------------------------------------------------
// MSelectionOnlyOperator (operator/query/MSelectionOnlyOperator.java:58-110) takes the first docs the filter yields, in
// docId order, and stops: per item the first K set bits of its selection mask.
//   pgx_select_first_count  grid (G, items), G > 1 only.  Workgroup g owns a contiguous stripe of the item's mask: the
//                           16-byte chunks (four 32-row words, 128 rows) [g * S, (g + 1) * S), S = ceil(chunks / G).
//                           It writes the stripe's popcount saturated at K to stripe_cnt[item * G + g], and leaves its
//                           loop as soon as the running count reaches K.
//   pgx_select_first        the same grid.  The workgroup's base is the sum of the stripes before its own (one lane per
//                           stripe, G <= 64); a workgroup whose base is at or past K returns.  Per step every thread
//                           loads one chunk (one 16-byte load where the mask is 16-byte aligned, else word by word),
//                           popcounts it, and an exclusive scan inside the wave64 and across the four waves through LDS
//                           gives it its rank; a thread whose rank is below K writes its set bits' docIds at
//                           out_doc[item * K + rank ...] while that stays below K.  The loop ends, for the whole
//                           workgroup, once base + the rows seen reaches K: a dense mask costs one or two steps.
// The ranks depend on the mask alone, so the rows are the same for every G.  An item whose `sel` is null selects every
// doc: docIds 0 .. min(K, num_docs) - 1, no mask read.  No workgroup waits on another; all stores are plain vector stores.
constexpr int kSelFirstWords = 4;  // mask words per thread and step

struct SelFirstStripe {
  int64_t c_begin, c_end;  // chunks of kSelFirstWords words
  int words;
};

__device__ __forceinline__ SelFirstStripe sel_first_stripe(int num_docs, int G, int wg) {
  SelFirstStripe s;
  s.words = num_docs > 0 ? (num_docs + 31) >> 5 : 0;  // the spare word and the bits past num_docs are never used
  const int64_t chunks = (static_cast<int64_t>(s.words) + kSelFirstWords - 1) / kSelFirstWords;
  const int64_t per = (chunks + G - 1) / G;
  s.c_begin = per * wg < chunks ? per * wg : chunks;
  s.c_end = s.c_begin + per < chunks ? s.c_begin + per : chunks;
  return s;
}

// Chunk c of the mask, rows at or past num_docs cleared; all zero at or past c_end.  The 16-byte load is taken only
// where it ends inside the mask's words + 1 spare word.
__device__ __forceinline__ uint4 sel_first_chunk(const uint32_t* __restrict__ sel, bool aligned, int64_t c, int64_t c_end,
                                                 int words, int num_docs) {
  uint4 m = make_uint4(0u, 0u, 0u, 0u);
  if (c >= c_end) return m;
  const int64_t w0 = c * kSelFirstWords;
  if (aligned && w0 + kSelFirstWords <= static_cast<int64_t>(words) + 1) {
    m = *reinterpret_cast<const uint4*>(sel + w0);
  } else {
    m.x = sel[w0];
    if (w0 + 1 < words) m.y = sel[w0 + 1];
    if (w0 + 2 < words) m.z = sel[w0 + 2];
    if (w0 + 3 < words) m.w = sel[w0 + 3];
  }
  const int64_t rem = static_cast<int64_t>(num_docs) - w0 * 32;  // rows of the mask from this chunk on: >= 1
  if (rem < 32 * kSelFirstWords) {
    const int r = static_cast<int>(rem);
    m.x &= r >= 32 ? ~0u : (1u << r) - 1u;
    m.y &= r >= 64 ? ~0u : (r > 32 ? (1u << (r - 32)) - 1u : 0u);
    m.z &= r >= 96 ? ~0u : (r > 64 ? (1u << (r - 64)) - 1u : 0u);
    m.w &= r > 96 ? (1u << (r - 96)) - 1u : 0u;
  }
  return m;
}

__device__ __forceinline__ void sel_first_emit(uint32_t m, int32_t d0, int& rank, int K, int32_t* __restrict__ out) {
  while (m && rank < K) {
    out[rank++] = d0 + __builtin_ctz(m);
    m &= m - 1u;
  }
}

// The walk over one stripe, from rank `base` on: returns base + the stripe's selected rows, or some count >= K once
// that many are known (the same value in every thread).  EMIT: write the docIds of the ranks below K.
template <bool EMIT>
__device__ __forceinline__ int sel_first_walk(const uint32_t* __restrict__ sel, const SelFirstStripe& S, int num_docs,
                                              int base, int K, int32_t* __restrict__ out) {
  __shared__ int wave_rows[2][kSelBlock / 64];
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const bool aligned = (reinterpret_cast<uintptr_t>(sel) & 15u) == 0;
  int run = base;
  int buf = 0;
  uint4 ahead = sel_first_chunk(sel, aligned, S.c_begin + tid, S.c_end, S.words, num_docs);
  for (int64_t c0 = S.c_begin; c0 < S.c_end && run < K; c0 += kSelBlock, buf ^= 1) {
    const int64_t c = c0 + tid;
    const uint4 m = ahead;
    ahead = sel_first_chunk(sel, aligned, c + kSelBlock, S.c_end, S.words, num_docs);  // each step loads the next one's
    const int rows = __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
    int incl = rows;  // inclusive scan over the wave64
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_rows[buf][wave] = incl;
    __syncthreads();  // (the buffers alternate: the next step's writes go to the other one)
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSelBlock / 64; ++w) {
      const int r = wave_rows[buf][w];
      before += w < wave ? r : 0;
      total += r;
    }
    if (EMIT) {
      int rank = run + before + incl - rows;
      if (rows && rank < K) {
        const int32_t d0 = static_cast<int32_t>(c * (32 * kSelFirstWords));
        sel_first_emit(m.x, d0, rank, K, out);
        sel_first_emit(m.y, d0 + 32, rank, K, out);
        sel_first_emit(m.z, d0 + 64, rank, K, out);
        sel_first_emit(m.w, d0 + 96, rank, K, out);
      }
    }
    run += total;
  }
  return run;
}

__global__ void __launch_bounds__(kSelBlock) pgx_select_first_count(const SelItem* __restrict__ items, int nitems, int K,
                                                                    int32_t* __restrict__ stripe_cnt) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  const int G = static_cast<int>(gridDim.x), wg = static_cast<int>(blockIdx.x);
  const uint32_t* __restrict__ sel = items[item].sel;
  const int num_docs = items[item].num_docs;
  const SelFirstStripe S = sel_first_stripe(num_docs, G, wg);
  int64_t rows;
  if (!sel) {  // every doc selected: the stripe's rows
    const int64_t nd = num_docs > 0 ? num_docs : 0;
    const int64_t d0 = S.c_begin * (32 * kSelFirstWords), d1 = S.c_end * (32 * kSelFirstWords);
    rows = (d1 < nd ? d1 : nd) - (d0 < nd ? d0 : nd);
  } else {
    rows = sel_first_walk<false>(sel, S, num_docs, 0, K, nullptr);
  }
  if (threadIdx.x == 0) stripe_cnt[static_cast<int64_t>(item) * G + wg] = static_cast<int32_t>(rows < K ? rows : K);
}

// out_lim (may be null): out_lim[item] = min(out_cnt[item], limit), the count the gathers after it run over.
__global__ void __launch_bounds__(kSelBlock) pgx_select_first(const SelItem* __restrict__ items, int nitems, int K,
                                                              const int32_t* __restrict__ stripe_cnt,
                                                              int32_t* __restrict__ out_doc, int32_t* __restrict__ out_cnt,
                                                              int limit, int32_t* __restrict__ out_lim) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  __shared__ int first_base, first_total;
  const int G = static_cast<int>(gridDim.x), wg = static_cast<int>(blockIdx.x);
  const int tid = static_cast<int>(threadIdx.x);
  const uint32_t* __restrict__ sel = items[item].sel;
  const int num_docs = items[item].num_docs;
  int32_t* __restrict__ out = out_doc + static_cast<int64_t>(item) * K;
  if (!sel) {  // every doc selected
    if (wg != 0) return;
    const int n = num_docs < K ? (num_docs > 0 ? num_docs : 0) : K;
    for (int r = tid; r < n; r += kSelBlock) out[r] = r;
    if (tid == 0) {
      out_cnt[item] = n;
      if (out_lim) out_lim[item] = n < limit ? n : limit;
    }
    return;
  }
  int base = 0, total = -1;  // total: the item's rows (saturated) when the stripes' counts say it, else from the walk
  if (G > 1) {
    if (tid < 64) {  // one lane per stripe: the rows before this workgroup's stripe, and the item's
      const int v = tid < G ? stripe_cnt[static_cast<int64_t>(item) * G + tid] : 0;
      int b = tid < wg ? v : 0, t = v;
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        b += __shfl_xor(b, d, 64);
        t += __shfl_xor(t, d, 64);
      }
      if (tid == 0) {
        first_base = b;
        first_total = t;
      }
    }
    __syncthreads();
    base = first_base;
    total = first_total;
    if (base >= K) return;  // the whole workgroup: the K rows lie in earlier stripes (never workgroup 0)
  }
  const SelFirstStripe S = sel_first_stripe(num_docs, G, wg);
  const int run = sel_first_walk<true>(sel, S, num_docs, base, K, out);
  if (G == 1) total = run;
  if (wg == 0 && tid == 0) {
    const int n = total < K ? total : K;
    out_cnt[item] = n;
    if (out_lim) out_lim[item] = n < limit ? n : limit;
  }
}

}  // namespace pgx

// LDS entries of the candidate buffer for K rows: a power of two (bitonic sort) with room for K kept entries plus one
// round of 256 appends.
static int sel_buffer_entries(int K) {
  int p = 1;
  while (p < K) p <<= 1;
  return 2 * p < 512 ? 512 : 2 * p;
}

static bool sel_args_ok(int nitems, int K, int wgs) {
  return nitems >= 0 && nitems <= 65535 && K >= 1 && K <= 2048 /* PGX_SEL_MAX_ROWS */ && wgs >= 1 && wgs <= 1024;
}

// Scratch: cand_key / cand_doc hold nitems x wgs_per_item x K entries, cand_cnt nitems x wgs_per_item.
extern "C" hipError_t pgx_launch_select_topk(const pgx::SelItem* items, int nitems, int K, int wgs_per_item,
                                             uint64_t* cand_key, uint32_t* cand_doc, int32_t* cand_cnt,
                                             hipStream_t stream) {
  if (!sel_args_ok(nitems, K, wgs_per_item) || !items || !cand_key || !cand_doc || !cand_cnt)
    return hipErrorInvalidValue;
  if (nitems == 0) return hipSuccess;
  const int C = sel_buffer_entries(K);
  hipLaunchKernelGGL(pgx::pgx_select_topk, dim3(static_cast<unsigned>(wgs_per_item), static_cast<unsigned>(nitems)),
                     dim3(pgx::kSelBlock), size_t(C) * 12, stream, items, nitems, K, C, cand_key, cand_doc, cand_cnt);
  return hipGetLastError();
}

// out_doc holds nitems x K docIds (item i's rank r at [i * K + r]), out_cnt nitems counts.
extern "C" hipError_t pgx_launch_select_merge(int nitems, int K, int wgs_per_item, const uint64_t* cand_key,
                                              const uint32_t* cand_doc, const int32_t* cand_cnt, int32_t* out_doc,
                                              int32_t* out_cnt, hipStream_t stream) {
  if (!sel_args_ok(nitems, K, wgs_per_item) || !cand_key || !cand_doc || !cand_cnt || !out_doc || !out_cnt)
    return hipErrorInvalidValue;
  if (nitems == 0) return hipSuccess;
  const int C = sel_buffer_entries(K);
  hipLaunchKernelGGL(pgx::pgx_select_merge, dim3(static_cast<unsigned>(nitems)), dim3(pgx::kSelBlock), size_t(C) * 12,
                     stream, nitems, K, C, wgs_per_item, cand_key, cand_doc, cand_cnt, out_doc, out_cnt);
  return hipGetLastError();
}

// cols holds nitems x ncols descriptors; out_ids ncols x nitems x K dictIds (column c, item i, rank r at
// [(c * nitems + i) * K + r]).
extern "C" hipError_t pgx_launch_select_gather(const pgx::SelGatherCol* cols, int nitems, int ncols, int K,
                                               const int32_t* out_doc, const int32_t* out_cnt, int32_t* out_ids,
                                               hipStream_t stream) {
  if (!sel_args_ok(nitems, K, 1) || ncols < 0 || !cols || !out_doc || !out_cnt || !out_ids) return hipErrorInvalidValue;
  const int64_t total = static_cast<int64_t>(nitems) * K * ncols;
  if (total == 0) return hipSuccess;
  const int64_t blocks = (total + pgx::kSelBlock - 1) / pgx::kSelBlock;
  if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pgx::pgx_select_gather, dim3(static_cast<unsigned>(blocks)), dim3(pgx::kSelBlock), 0, stream, cols,
                     nitems, ncols, K, out_doc, out_cnt, out_ids);
  return hipGetLastError();
}

// Selection without ORDER BY.  stripe_cnt holds nitems x wgs_per_item counts (item i's stripe g at [i * wgs_per_item +
// g]); with wgs_per_item > 1 pgx_launch_select_first reads what pgx_launch_select_first_count wrote there on the same
// stream, with one workgroup per item it reads none (stripe_cnt may be null).  out_doc / out_cnt as the merge writes
// them: item i's rank r at [i * K + r], ascending docIds, out_cnt[i] = min(matches, K); ranks past the count keep
// what the caller put there.  out_lim (may be null): nitems counts min(out_cnt[i], limit), 1 <= limit <= K.
static bool sel_first_args_ok(int nitems, int K, int wgs) {
  return nitems >= 0 && nitems <= 65535 && K >= 1 && K <= 2048 /* PGX_SEL_MAX_ROWS */ && wgs >= 1 && wgs <= 64;
}

extern "C" hipError_t pgx_launch_select_first_count(const pgx::SelItem* items, int nitems, int K, int wgs_per_item,
                                                    int32_t* stripe_cnt, hipStream_t stream) {
  if (!sel_first_args_ok(nitems, K, wgs_per_item) || !items || !stripe_cnt) return hipErrorInvalidValue;
  if (nitems == 0) return hipSuccess;
  hipLaunchKernelGGL(pgx::pgx_select_first_count,
                     dim3(static_cast<unsigned>(wgs_per_item), static_cast<unsigned>(nitems)), dim3(pgx::kSelBlock), 0,
                     stream, items, nitems, K, stripe_cnt);
  return hipGetLastError();
}

extern "C" hipError_t pgx_launch_select_first(const pgx::SelItem* items, int nitems, int K, int wgs_per_item,
                                              const int32_t* stripe_cnt, int32_t* out_doc, int32_t* out_cnt, int limit,
                                              int32_t* out_lim, hipStream_t stream) {
  if (!sel_first_args_ok(nitems, K, wgs_per_item) || !items || !out_doc || !out_cnt ||
      (wgs_per_item > 1 && !stripe_cnt) || (out_lim && (limit < 1 || limit > K)))
    return hipErrorInvalidValue;
  if (nitems == 0) return hipSuccess;
  hipLaunchKernelGGL(pgx::pgx_select_first, dim3(static_cast<unsigned>(wgs_per_item), static_cast<unsigned>(nitems)),
                     dim3(pgx::kSelBlock), 0, stream, items, nitems, K, stripe_cnt, out_doc, out_cnt, limit, out_lim);
  return hipGetLastError();
}

// The multi-value launches run after pgx_launch_select_merge on its stream, over out_doc / out_cnt as it wrote them.
// cols holds nmv x nitems descriptors, pair (multi-value column m, item i) at [m * nitems + i].
static bool sel_mv_args_ok(int nitems, int nmv, int K) {
  return sel_args_ok(nitems, K, 1) && nmv >= 0 && static_cast<int64_t>(nitems) * nmv <= 0x7FFFFFFF / 64;
}

// rel_off holds (K + 1) int32 per pair: rank r of the pair owns values [rel_off[r], rel_off[r + 1]) of the pair's
// values, ranks at or past the item's count none; totals one int32 per pair (= its rel_off[K]).
extern "C" hipError_t pgx_launch_select_mv_offsets(const pgx::SelMvCol* cols, int nitems, int nmv, int K,
                                                   const int32_t* out_doc, const int32_t* out_cnt, int32_t* rel_off,
                                                   int32_t* totals, hipStream_t stream) {
  if (!sel_mv_args_ok(nitems, nmv, K) || !cols || !out_doc || !out_cnt || !rel_off || !totals)
    return hipErrorInvalidValue;
  const int64_t pairs = static_cast<int64_t>(nitems) * nmv;
  if (pairs == 0) return hipSuccess;
  hipLaunchKernelGGL(pgx::pgx_select_mv_offsets, dim3(static_cast<unsigned>(pairs)), dim3(pgx::kSelBlock), 0, stream,
                     cols, nitems, nmv, K, out_doc, out_cnt, rel_off, totals);
  return hipGetLastError();
}

// bases holds npairs + 1 int64: where each pair's values start in the value buffer, and the grand total.
extern "C" hipError_t pgx_launch_select_mv_bases(const int32_t* totals, int64_t npairs, int64_t* bases,
                                                 hipStream_t stream) {
  if (npairs < 0 || npairs > 0x7FFFFFFF / 64 || (npairs > 0 && !totals) || !bases) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pgx::pgx_select_mv_bases, dim3(1), dim3(pgx::kSelBlock), 0, stream, totals, npairs, bases);
  return hipGetLastError();
}

// values holds `capacity` dictIds (the grand total of pgx_launch_select_mv_bases, or more): pair p's value j at
// [bases[p] + j]; nothing is stored at or past capacity.  wgs_per_pair workgroups share a pair's values.
extern "C" hipError_t pgx_launch_select_mv_gather(const pgx::SelMvCol* cols, int nitems, int nmv, int K,
                                                  int wgs_per_pair, const int32_t* out_doc, const int32_t* out_cnt,
                                                  const int32_t* rel_off, const int64_t* bases, int32_t* values,
                                                  int64_t capacity, hipStream_t stream) {
  if (!sel_mv_args_ok(nitems, nmv, K) || wgs_per_pair < 1 || wgs_per_pair > 64 || capacity < 0 || !cols || !out_doc ||
      !out_cnt || !rel_off || !bases || (capacity > 0 && !values))
    return hipErrorInvalidValue;
  const int64_t pairs = static_cast<int64_t>(nitems) * nmv;
  if (pairs == 0 || capacity == 0) return hipSuccess;
  hipLaunchKernelGGL(pgx::pgx_select_mv_gather, dim3(static_cast<unsigned>(pairs * wgs_per_pair)), dim3(pgx::kSelBlock),
                     size_t(2 * K + 1) * 4, stream, cols, nitems, nmv, K, wgs_per_pair, out_doc, out_cnt, rel_off, bases,
                     values, capacity);
  return hipGetLastError();
}
