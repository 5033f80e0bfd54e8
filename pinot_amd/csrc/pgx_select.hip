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
// No workgroup waits on another; all stores are plain vector stores.
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
