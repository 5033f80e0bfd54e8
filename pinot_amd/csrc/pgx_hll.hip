// libpgx: DISTINCTCOUNTHLL registers -- DistinctCountHLLAggregationFunction (operator/aggregation/function/
// DistinctCountHLLAggregationFunction.java:51-92: hll.offer((int) hashCode) per selected doc) over the selection bits
// the query kernels wrote.  Reference paths are relative to pinot-core/src/main/java/com/linkedin/pinot/core/.
//
// The hash depends on the dictionary value alone, so the host builds one u16 code per dictId (pgx_hll.cpp:
// register << 8 | rank) and an offer is one gather and one register max.  Max is idempotent and order-free: the
// registers are exact whatever the grid size or scheduling, and segments combine by maxing into the same registers.
//
//   pgx_hll_offer        grid (workgroups per item, items), one item per (segment, function).  A workgroup strides over
//                        its item's 32-row mask words, one word per thread and step, skipping zero words.  Words with
//                        many selected rows decode the column's 32 dictIds at once, sparse words read their rows one
//                        by one.  Ranks are maxed into 256 u32 registers in LDS (read first, atomic only when greater:
//                        after warm-up almost no offer changes a register); at the end thread t maxes a non-zero
//                        register t into out[t].  A dense word goes in passes of independent accesses -- 32 code
//                        gathers, 32 register reads, then the few atomics -- so that a wave has 32 loads in flight
//                        instead of one chain of gather, read and compare per row.
//   pgx_hll_offer_group  the same over (group slot, register) pairs: slot = sum of the group columns' global ids x
//                        gmul (column 0 least significant), registers u32 in one table of slots x 256 in HBM, zeroed by
//                        the caller.  u32 and not bytes: the hardware's 32-bit atomic max updates a register in one
//                        instruction, where a byte register needs a compare-and-swap loop on its dword that retries
//                        whenever any of the four neighbours changed; the price is 4 bytes per register to zero and a
//                        narrowing pass (pgx_hll_narrow) over the groups the result holds.
//   pgx_hll_narrow       one thread per (group, four registers): the listed slots' registers as bytes.
//   pgx_hll_offer_mv     DISTINCTCOUNTHLLMV (DistinctCountHLLMVAggregationFunction.java): the column is multi-value and
//                        every value of every selected doc is offered.  The same grid and LDS registers; a run of
//                        consecutive selected docs of a mask word owns one contiguous range of the value stream
//                        (start[first] .. start[last + 1]), walked in passes of independent accesses.
//   pgx_hll_offer_mv_group  the same into the slots x 256 table: the slot of a doc from its single-value group columns
//                        as in pgx_hll_offer_group, every value of the doc into that slot.
// The walk over the selection bits (mask words, dense and sparse words, runs of docs, the slots of a word's docs) is
// shared with pgx_distinct.hip and lives in pgx_hll_device.h; here are the offers it is handed, and the launchers.
// No workgroup waits on another; all stores are plain vector stores and vector atomics.
#include <hip/hip_runtime.h>

#include "pgx_device.h"
#include "pgx_hll_device.h"
#include "pgx_internal.h"

namespace pgx {

// regs: 256 u32 registers (LDS or HBM)
__device__ __forceinline__ void hll_offer(uint32_t* regs, const HllItem& A, uint32_t id) {
  if (id >= static_cast<uint32_t>(A.ncodes)) return;
  const uint32_t c = A.codes[id];
  const uint32_t j = c >> 8, r = c & 0xFFu;
  if (regs[j] < r) atomicMax(&regs[j], r);
}

// v[j]: the dictId of row j of a mask word -> its code, 0 for a row that is not selected or whose dictId lies at or
// past the table (rank >= 1: a code is never 0).  ncodes >= 1 here: an empty table's item has no selected rows to offer.
// The row's "on" state lives in its bit of sel and is applied as a mask on both sides of the load: a compare held
// across the 32 loads in flight would take a pair of scalar registers per row.
__device__ __forceinline__ void hll_gather_codes(const HllItem& A, uint32_t sel, uint32_t (&v)[32]) {
#pragma unroll
  for (int j = 0; j < 32; ++j) sel &= ~(static_cast<uint32_t>(v[j] >= static_cast<uint32_t>(A.ncodes)) << j);
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const uint32_t on = 0u - ((sel >> j) & 1u);  // all ones or 0
    v[j] = A.codes[v[j] & on] & on;
  }
}

__global__ void __launch_bounds__(kHllBlock) pgx_hll_offer(const HllItem* __restrict__ items, int nitems) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  __shared__ uint32_t regs[kHllRegs];
  const int tid = static_cast<int>(threadIdx.x);
  regs[tid] = 0u;
  __syncthreads();
  const HllItem A = items[item];
  // v: a word's rows.  Out here on purpose: declared inside the callable, where its lifetime ends with every word, the
  // compiler schedules the passes into 114 VGPRs (4 waves per SIMD) instead of 79 (6).
  uint32_t v[32];
  sel_walk(
      A, sel_words(A),
      [&](int64_t w, uint32_t sel) PGX_SEL_OP {
        // three passes over the word, each of 32 independent accesses the hardware keeps in flight together (a chain
        // of gather, register read and compare per row leaves one access in flight per wave): the codes (entry 0
        // stands in for rows that offer nothing, so no load is conditional; a code is never 0), the registers, the few
        // atomics
        pgx_fwd_decode_word(A.bits, A.fwd, w, v);
        hll_gather_codes(A, sel, v);
#pragma unroll
        for (int j = 0; j < 32; ++j) v[j] = regs[v[j] >> 8] < (v[j] & 0xFFu) ? v[j] : 0u;
#pragma unroll
        for (int j = 0; j < 32; ++j)
          if (v[j] != 0u) atomicMax(&regs[v[j] >> 8], v[j] & 0xFFu);
      },
      [&](int32_t row) PGX_SEL_OP { hll_offer(regs, A, pgx_fwd_value(A.fwd, row, A.bits)); });
  __syncthreads();
  const uint32_t r = regs[tid];
  if (r != 0u && A.out[tid] < r) atomicMax(&A.out[tid], r);
}

// Rows J0 .. J0 + 15 of a mask word whose codes are gathered (v): slots, registers, atomics.  Half a word at a time:
// 16 loads in flight per lane and pass, and half the addresses live at once.
template <int J0>
__device__ __forceinline__ void hll_group_rows(const HllGroupItem& G, const HllGroupKey& K, int32_t d0,
                                               uint32_t (&v)[32]) {
  const uint32_t slots32 = static_cast<uint32_t>(K.slots);  // <= kHllMaxGroupSlots (launcher)
  for (int g = 0; g < K.ngcols; ++g) {
    const uint32_t* __restrict__ gf = G.g[g].fwd;
    const int32_t* __restrict__ rm = G.g[g].remap;
    const int gb = G.g[g].bits;
    const uint32_t mul = static_cast<uint32_t>(K.gmul[g]);  // 1..slots (launcher)
#pragma unroll
    for (int j = J0; j < J0 + 16; ++j) {
      // Masks, not compares: 32 compares hoisted above the loads would each hold a pair of scalar registers.
      // on: the row still offers (its code field is not 0); a row that does not reads remap entry 0.
      const uint32_t c16 = v[j] & 0xFFFFu;
      const uint32_t on = static_cast<uint32_t>(static_cast<int32_t>(c16 | (0u - c16)) >> 31);
      const uint32_t id = pgx_fwd_value2(gf, d0 + j, gb) & on;
      const uint32_t gid = rm ? static_cast<uint32_t>(rm[id]) : id;  // a negative id: >= 2^31
      // 32-bit arithmetic throughout (a 64-bit multiply-add carries out into scalar registers too): an id of
      // 65536 or more is outside every key space (bad); below that, slot so far + id * mul < 2^32, saturated to
      // 2^17, and ok = it is below slots
      const uint32_t hi = gid >> 16;
      const uint32_t bad = static_cast<uint32_t>(static_cast<int32_t>(hi | (0u - hi)) >> 31);
      const uint32_t s = __builtin_elementwise_min((v[j] >> 16) + (gid & 0xFFFFu) * mul, 0x20000u);
      const uint32_t ok = ~static_cast<uint32_t>(static_cast<int32_t>(slots32 - 1u - s) >> 31) & ~bad;
      v[j] = (c16 | (s << 16)) & ok & on;  // (a key outside the planned space: the row offers nothing)
    }
  }
  uint32_t* const table = G.h.out;
#pragma unroll
  for (int j = J0; j < J0 + 16; ++j) {
    const uint32_t cur = table[static_cast<size_t>(v[j] >> 16) * kHllRegs + ((v[j] >> 8) & 0xFFu)];
    v[j] = cur < (v[j] & 0xFFu) ? v[j] : 0u;
  }
#pragma unroll
  for (int j = J0; j < J0 + 16; ++j)
    if (v[j] != 0u) atomicMax(&table[static_cast<size_t>(v[j] >> 16) * kHllRegs + ((v[j] >> 8) & 0xFFu)], v[j] & 0xFFu);
}

// The same through a sparse run's directory.  A group's index takes 17 bits, so it does not share the word with the
// code: the 16 rows' indexes are looked up first (sel_word_slots: only rows that still offer), then the registers and
// the few atomics as above.  A row whose key the directory does not hold offers nothing.
template <int J0>
__device__ __forceinline__ void hll_group_rows(const HllGroupItem& G, const SelSparseKey& K, int32_t d0,
                                               uint32_t (&v)[32]) {
  uint32_t on16 = 0u;
#pragma unroll
  for (int j = 0; j < 16; ++j) on16 |= static_cast<uint32_t>((v[J0 + j] & 0xFFFFu) != 0u) << (J0 + j);
  uint32_t s[16];
  sel_word_slots<J0>(G.g, K, on16, d0, s);
  uint32_t* const table = G.h.out;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const bool ok = s[j] < K.groups;
    s[j] = ok ? s[j] : 0u;
    const uint32_t c = ok ? v[J0 + j] & 0xFFFFu : 0u;
    const uint32_t cur = table[static_cast<size_t>(s[j]) * kHllRegs + (c >> 8)];
    v[J0 + j] = cur < (c & 0xFFu) ? c : 0u;
  }
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (v[J0 + j] != 0u)
      atomicMax(&table[static_cast<size_t>(s[j]) * kHllRegs + (v[J0 + j] >> 8)], v[J0 + j] & 0xFFu);
}

// Key: HllGroupKey (a dense key space: the slot is a multiply-add) or SelSparseKey (the result's groups: the slot is a
// directory lookup); only the slot computation differs.
template <class Key>
__global__ void __launch_bounds__(kHllBlock) pgx_hll_offer_group(const HllGroupItem* __restrict__ items, int nitems,
                                                                 const Key K) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  const HllGroupItem& G = items[item];
  const HllItem A = G.h;
  const uint32_t slots32 = sel_key_rows(K);  // <= kHllMaxGroupSlots, sparse: <= kSelMaxSparseGroups (launcher)
  sel_walk(
      A, sel_gcols_ok(G.g, K) ? sel_words(A) : 0,
      [&](int64_t w, uint32_t sel) PGX_SEL_OP {
        // passes of 32 independent accesses, as in pgx_hll_offer: the codes; per group column the rows' ids (the word's
        // rows all lie inside the padded index, so the id loads are unconditional; a row that offers nothing takes
        // remap entry 0) folded into the slot, which shares the word with the code (both fit 16 bits); the registers;
        // the few atomics
        uint32_t v[32];
        pgx_fwd_decode_word(A.bits, A.fwd, w, v);
        hll_gather_codes(A, sel, v);
        hll_group_rows<0>(G, K, static_cast<int32_t>(w * 32), v);
        hll_group_rows<16>(G, K, static_cast<int32_t>(w * 32), v);
      },
      [&](int32_t row) PGX_SEL_OP {
        const uint32_t s = sel_row_slot(G.g, K, row);
        if (s < slots32)  // (a key outside the planned space: never written)
          hll_offer(A.out + static_cast<size_t>(s) * kHllRegs, A, pgx_fwd_value(A.fwd, row, A.bits));
      });
}

// ---- DISTINCTCOUNTHLLMV: every value of every selected doc ----------------------------------------------------------
// Value rows lo .. lo + N - 1 of an item's value stream offered into regs (256 u32, LDS or HBM), in passes of N
// independent accesses: the dictIds, the codes, the registers, then the few atomics.  lo < hi <= A.h.total: rows at or
// past hi take row hi - 1's address and offer nothing (their mask is 0), so no load is conditional.  Masks, not
// compares, across the loads (hll_gather_codes).  pgx_fwd_value2 reads the row's dword and the next: for a row below
// `total` both lie inside the stream's allocation, because padded_fwd_bytes(total, bits) covers whole tiles of rows
// and 64 bytes more (the second dword of the last row ends at most 8 bytes past total * bits / 8).
template <int N>
__device__ __forceinline__ void hll_mv_batch(uint32_t* regs, const HllItem& A, uint32_t lo, uint32_t hi) {
  uint32_t v[N], m[N];
  const uint32_t nc = static_cast<uint32_t>(A.ncodes);  // >= 1 (sel_words)
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint32_t r = lo + static_cast<uint32_t>(i);
    const uint32_t on = static_cast<uint32_t>(static_cast<int32_t>(r - hi) >> 31);  // r < hi (both below 2^31 + N)
    const uint32_t id = pgx_fwd_value2(A.fwd, static_cast<int32_t>(__builtin_elementwise_min(r, hi - 1u)), A.bits);
    const uint32_t t = __builtin_elementwise_min(id, nc), d = t - nc;  // d == 0: a dictId at or past the table
    m[i] = static_cast<uint32_t>(static_cast<int32_t>(d | (0u - d)) >> 31) & on;
    v[i] = t & m[i];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = A.codes[v[i]] & m[i];  // (a code is never 0)
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = regs[v[i] >> 8] < (v[i] & 0xFFu) ? v[i] : 0u;
#pragma unroll
  for (int i = 0; i < N; ++i)
    if (v[i] != 0u) atomicMax(&regs[v[i] >> 8], v[i] & 0xFFu);
}

// A run of consecutive selected docs owns one contiguous range of the value stream (sel_mv_walk).
__global__ void __launch_bounds__(kHllBlock) pgx_hll_offer_mv(const HllMvItem* __restrict__ items, int nitems) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  __shared__ uint32_t regs[kHllRegs];
  const int tid = static_cast<int>(threadIdx.x);
  regs[tid] = 0u;
  __syncthreads();
  const HllMvItem M = items[item];
  const HllItem A = M.h;
  sel_mv_walk(A, sel_mv_words(A, M.start, M.total), M.start, M.total, [&](auto n, uint32_t lo, uint32_t hi) PGX_SEL_OP {
    hll_mv_batch<decltype(n)::value>(regs, A, lo, hi);
  });
  __syncthreads();
  const uint32_t r = regs[tid];
  if (r != 0u && A.out[tid] < r) atomicMax(&A.out[tid], r);
}

// The same over a table of slots x 256 registers in HBM: every value of a doc into the doc's slot (sel_mv_group_walk).
template <class Key>
__global__ void __launch_bounds__(kHllBlock) pgx_hll_offer_mv_group(const HllMvGroupItem* __restrict__ items,
                                                                    int nitems, const Key K) {
  const int item = static_cast<int>(blockIdx.y);
  if (item >= nitems) return;
  __shared__ uint32_t slot_of[32 * kHllBlock];
  const HllMvGroupItem& M = items[item];
  const HllItem A = M.g.h;
  sel_mv_group_walk(A, M.g.g, K, M.start, M.total, slot_of,
                    [&](uint32_t s, auto n, uint32_t lo, uint32_t hi) PGX_SEL_OP {
                      hll_mv_batch<decltype(n)::value>(A.out + static_cast<size_t>(s) * kHllRegs, A, lo, hi);
                    });
}

__global__ void __launch_bounds__(kHllBlock) pgx_hll_narrow(const uint32_t* __restrict__ table,
                                                            const int64_t* __restrict__ slot, int64_t ngroups,
                                                            uint64_t slots, uint32_t* __restrict__ out) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kHllBlock + threadIdx.x;  // (group, register quad)
  if (idx >= ngroups * (kHllRegs / 4)) return;
  const int64_t g = idx / (kHllRegs / 4);
  const int q = static_cast<int>(idx % (kHllRegs / 4));
  const int64_t s = slot[g];
  uint32_t packed = 0u;
  if (s >= 0 && static_cast<uint64_t>(s) < slots) {
    const uint32_t* r = table + s * kHllRegs + 4 * q;
    packed = (r[0] & 0xFFu) | ((r[1] & 0xFFu) << 8) | ((r[2] & 0xFFu) << 16) | ((r[3] & 0xFFu) << 24);
  }
  out[idx] = packed;
}

// ---- the group directory of a sparse run (SelSparseKey, pgx_internal.h) -----------------------------------------------
// Thread i puts key i (W words) into the open-addressing table with value i, on the pattern of pgx_join_build
// (pgx_merge.hip): pgx_insert over the whole table -- the keys are distinct and cap >= n, so a free slot always exists.
__global__ void __launch_bounds__(kHllBlock) pgx_sel_dir_build(const unsigned long long* __restrict__ keys, int64_t n,
                                                               int W, unsigned long long* __restrict__ tkey,
                                                               unsigned int* __restrict__ tstate,
                                                               uint32_t* __restrict__ tidx, uint64_t cap) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kHllBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t h = W == 1 ? pgx_insert<1>(tkey, tstate, cap, {keys[i]}, cap)
                           : pgx_insert<2>(tkey, tstate, cap, {keys[2 * i], keys[2 * i + 1]}, cap);
  if (h >= 0) tidx[h] = static_cast<uint32_t>(i);
}

// out[i] = the group of key i (W words), or kHllNoSlot (counted in *K.miss): the lookup every sparse group kernel does
// per row, on its own for the tests and the benchmarks.
__global__ void __launch_bounds__(kHllBlock) pgx_sel_dir_find(const unsigned long long* __restrict__ keys, int64_t n,
                                                              const SelSparseKey K, uint32_t* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kHllBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t h = K.W == 1 ? pgx_find<1>(K.keys, K.state, K.cap, {keys[i]}, K.cap)
                             : pgx_find<2>(K.keys, K.state, K.cap, {keys[2 * i], keys[2 * i + 1]}, K.cap);
  if (h < 0) atomicAdd(K.miss, 1ull);
  out[i] = h < 0 ? kHllNoSlot : K.index[h];
}

}  // namespace pgx

// keys: n keys of W words in device memory, distinct; check: the caller's host copy of them.  Of the table, tkey (cap x
// W words) and, when W == 2, tstate (cap words) are cleared here, on the stream, before the build; tidx (cap words) is
// not: only the entries of slots that hold a key are written, and only those are ever read.  Refused without launching
// anything: a null pointer, a negative count or one over kSelMaxSparseGroups, a W other than 1 or 2, a capacity that
// is not a power of two, is below the count or is above 2^20 (eight times the largest count: nothing needs more), and
// a one-word key of ~0 (the empty slot).
extern "C" hipError_t pgx_launch_sel_dir_build(const unsigned long long* keys, const unsigned long long* check,
                                               int64_t n, int W, unsigned long long* tkey, unsigned int* tstate,
                                               uint32_t* tidx, uint64_t cap, hipStream_t stream) {
  if (!keys || !check || !tkey || !tidx || n < 0 || n > pgx::kSelMaxSparseGroups || (W != 1 && W != 2) ||
      (W == 2 && !tstate) || cap == 0 || (cap & (cap - 1)) != 0 || cap < static_cast<uint64_t>(n) ||
      cap > (1ull << 20))
    return hipErrorInvalidValue;
  if (W == 1)
    for (int64_t i = 0; i < n; ++i)
      if (check[i] == ~0ull) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(tkey, 0xFF, cap * static_cast<uint64_t>(W) * 8, stream);
  if (e == hipSuccess && W == 2) e = hipMemsetAsync(tstate, 0, cap * 4, stream);
  if (e != hipSuccess || n == 0) return e;
  const int64_t blocks = (n + pgx::kHllBlock - 1) / pgx::kHllBlock;
  hipLaunchKernelGGL(pgx::pgx_sel_dir_build, dim3(static_cast<unsigned>(blocks)), dim3(pgx::kHllBlock), 0, stream, keys,
                     n, W, tkey, tstate, tidx, cap);
  return hipGetLastError();
}

// out: n u32 (device).  key: the caller's host struct, checked as the sparse group launchers check it.
extern "C" hipError_t pgx_launch_sel_dir_find(const unsigned long long* keys, int64_t n, const pgx::SelSparseKey* key,
                                              uint32_t* out, hipStream_t stream) {
  if (!keys || !out || n < 0 || n > (1ll << 24) || !pgx::sel_sparse_key_ok(key)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const int64_t blocks = (n + pgx::kHllBlock - 1) / pgx::kHllBlock;
  hipLaunchKernelGGL(pgx::pgx_sel_dir_find, dim3(static_cast<unsigned>(blocks)), dim3(pgx::kHllBlock), 0, stream, keys,
                     n, *key, out);
  return hipGetLastError();
}

static bool hll_item_ok(const pgx::HllItem& h) { return pgx::sel_item_ok(h, 0) && h.codes; }

// items: nitems descriptors in device memory; check: the caller's host copy of them, which is what gets validated.
extern "C" hipError_t pgx_launch_hll_offer(const pgx::HllItem* items, const pgx::HllItem* check, int nitems,
                                           int wgs_per_item, hipStream_t stream) {
  return pgx::sel_launch(pgx::pgx_hll_offer, items, check, nitems, wgs_per_item, stream, hll_item_ok);
}

// Every item's `h.out` is a table of slots x 256 u32 registers, zeroed by the caller.  gmul: ngcols host values.
extern "C" hipError_t pgx_launch_hll_offer_group(const pgx::HllGroupItem* items, const pgx::HllGroupItem* check,
                                                 int nitems, int ngcols, const uint64_t* gmul, int64_t slots,
                                                 int wgs_per_item, hipStream_t stream) {
  if (!pgx::sel_key_ok(ngcols, gmul, slots)) return hipErrorInvalidValue;
  return pgx::sel_launch(
      pgx::pgx_hll_offer_group<pgx::HllGroupKey>, items, check, nitems, wgs_per_item, stream,
      [&](const pgx::HllGroupItem& g) { return hll_item_ok(g.h) && pgx::sel_gcols_host_ok(g.g, ngcols); },
      pgx::sel_key(ngcols, gmul, slots));
}

// The sparse form: every item's `h.out` is a table of key->groups x 256 u32 registers, zeroed by the caller; key: the
// caller's host struct (its directory built by pgx_launch_sel_dir_build on the same stream).
extern "C" hipError_t pgx_launch_hll_offer_group_sparse(const pgx::HllGroupItem* items,
                                                        const pgx::HllGroupItem* check, int nitems,
                                                        const pgx::SelSparseKey* key, int wgs_per_item,
                                                        hipStream_t stream) {
  if (!pgx::sel_sparse_key_ok(key)) return hipErrorInvalidValue;
  const int ngcols = key->ngcols;
  return pgx::sel_launch(
      pgx::pgx_hll_offer_group<pgx::SelSparseKey>, items, check, nitems, wgs_per_item, stream,
      [&](const pgx::HllGroupItem& g) { return hll_item_ok(g.h) && pgx::sel_gcols_host_ok(g.g, ngcols); }, *key);
}

// out: ngroups x 256 bytes (as ngroups x 64 dwords); group i's registers are those of table slot slot[i].
extern "C" hipError_t pgx_launch_hll_narrow(const uint32_t* table, const int64_t* slot, int64_t ngroups, int64_t slots,
                                            uint32_t* out, hipStream_t stream) {
  if (ngroups < 0 || slots < 1 || slots > pgx::kHllMaxGroupSlots || ngroups > slots || !table || !slot || !out)
    return hipErrorInvalidValue;
  if (ngroups == 0) return hipSuccess;
  const int64_t blocks = (ngroups * (pgx::kHllRegs / 4) + pgx::kHllBlock - 1) / pgx::kHllBlock;
  hipLaunchKernelGGL(pgx::pgx_hll_narrow, dim3(static_cast<unsigned>(blocks)), dim3(pgx::kHllBlock), 0, stream, table,
                     slot, ngroups, static_cast<uint64_t>(slots), out);
  return hipGetLastError();
}

// DISTINCTCOUNTHLLMV.  Validated like the launchers above, on the caller's host copy of the items; the start array
// itself is device data, so the kernels clamp every value range to `total`.
extern "C" hipError_t pgx_launch_hll_offer_mv(const pgx::HllMvItem* items, const pgx::HllMvItem* check, int nitems,
                                              int wgs_per_item, hipStream_t stream) {
  return pgx::sel_launch(
      pgx::pgx_hll_offer_mv, items, check, nitems, wgs_per_item, stream,
      [](const pgx::HllMvItem& m) { return hll_item_ok(m.h) && pgx::sel_mv_ok(m.start, m.total); });
}

// Every item's `g.h.out` is a table of slots x 256 u32 registers, zeroed by the caller.  gmul: ngcols host values.
extern "C" hipError_t pgx_launch_hll_offer_mv_group(const pgx::HllMvGroupItem* items,
                                                    const pgx::HllMvGroupItem* check, int nitems, int ngcols,
                                                    const uint64_t* gmul, int64_t slots, int wgs_per_item,
                                                    hipStream_t stream) {
  if (!pgx::sel_key_ok(ngcols, gmul, slots)) return hipErrorInvalidValue;
  return pgx::sel_launch(
      pgx::pgx_hll_offer_mv_group<pgx::HllGroupKey>, items, check, nitems, wgs_per_item, stream,
      [&](const pgx::HllMvGroupItem& m) {
        return hll_item_ok(m.g.h) && pgx::sel_gcols_host_ok(m.g.g, ngcols) && pgx::sel_mv_ok(m.start, m.total);
      },
      pgx::sel_key(ngcols, gmul, slots));
}

extern "C" hipError_t pgx_launch_hll_offer_mv_group_sparse(const pgx::HllMvGroupItem* items,
                                                           const pgx::HllMvGroupItem* check, int nitems,
                                                           const pgx::SelSparseKey* key, int wgs_per_item,
                                                           hipStream_t stream) {
  if (!pgx::sel_sparse_key_ok(key)) return hipErrorInvalidValue;
  const int ngcols = key->ngcols;
  return pgx::sel_launch(
      pgx::pgx_hll_offer_mv_group<pgx::SelSparseKey>, items, check, nitems, wgs_per_item, stream,
      [&](const pgx::HllMvGroupItem& m) {
        return hll_item_ok(m.g.h) && pgx::sel_gcols_host_ok(m.g.g, ngcols) && pgx::sel_mv_ok(m.start, m.total);
      },
      *key);
}
