// libpgx: FASTHLL -- FastHllAggregationFunction (operator/aggregation/function/FastHllAggregationFunction.java: addAll
// of every selected doc's deserialized HyperLogLog into one of log2m 8) over the presence bitmaps the DISTINCTCOUNT
// mark kernels wrote (pgx_distinct.hip).  Reference paths are relative to pinot-core/src/main/java/com/linkedin/pinot/core/.
//
// addAll is a register-wise maximum and so idempotent: a group's registers are a function of the SET of dictIds
// selected in it.  The dictionary's estimators lie decoded in HBM, 256 bytes per dictId (64 dwords, registers <= 31:
// pgx_fasthll.cpp), and
//
//   pgx_fasthll_fold   folds the image rows of a bitmap row's set bits into that result row's u32 registers.  Grid
//                      (workgroups per row, rows): a workgroup takes one stretch of the row's words, a multiple of 64,
//                      in steps of 256 words, every fourth word to a wave (so a short stretch still busies all four); a
//                      step whose words are all zero is skipped.  A wave lists the set bits of its 64 words in LDS
//                      (positions from a prefix over the popcounts) and then folds them kFoldBatch image rows at a
//                      time: each a coalesced dword per lane, lane l holding registers 4l .. 4l + 3, all loads of a
//                      batch independent and in flight together.  The maximum is taken byte-wise inside the dword
//                      (registers are below 128).  The four waves combine through LDS, and
//                      thread t raises register t of the output: a plain load, then atomicMax only when greater, as
//                      pgx_hll_offer_group does.  Other workgroups of the row and other dictionaries of the column do
//                      the same to the same registers, so the union over dictionaries is taken here, on the device;
//                      pgx_hll_narrow then writes the bytes.
// Bits at or past card in the last word are masked, so no image row at or past card is read.
// No workgroup waits on another; all stores are plain vector stores and vector atomics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pgx_device.h"
#include "pgx_internal.h"

namespace pgx {

constexpr int kFoldWaves = kHllBlock / 64;
constexpr int kFoldBatch = 8;               // image rows in flight per wave
constexpr uint32_t kFoldSplitWords = 64u;  // a row of more words is shared: a workgroup per 64 words, up to 64

__device__ __host__ __forceinline__ uint32_t fold_bitmap_words(int32_t card) {
  return (static_cast<uint32_t>(card) + 31u) >> 5;  // card >= 1
}

// byte-wise maximum of four bytes below 128 each: bit 7 of (x | 0x80) - y says x >= y, and no byte borrows
__device__ __forceinline__ uint32_t fold_max4(uint32_t x, uint32_t y) {
  const uint32_t ge = (((x | 0x80808080u) - y) >> 7) & 0x01010101u;
  const uint32_t m = ge * 0xFFu;
  return (x & m) | (y & ~m);
}

// out[r * 256 + j] = max(itself, register j of image row d) over the set bits d < card of table row rows[r]; a row
// outside 0 .. slots - 1 folds nothing.
__global__ void __launch_bounds__(kHllBlock) pgx_fasthll_fold(const uint32_t* __restrict__ table, uint32_t card,
                                                              const uint32_t* __restrict__ image,
                                                              const int64_t* __restrict__ rows, int64_t nrows,
                                                              uint64_t slots, uint32_t* __restrict__ out) {
  __shared__ uint16_t ids[kFoldWaves][64 * 32];  // per wave: the set bits of its 64 words, as lane * 32 + bit
  __shared__ uint32_t part[kFoldWaves][64];
  const uint32_t bw = fold_bitmap_words(static_cast<int32_t>(card));
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t stretch =
      ((bw + gridDim.x - 1u) / gridDim.x + kFoldSplitWords - 1u) / kFoldSplitWords * kFoldSplitWords;
  const uint64_t first64 = static_cast<uint64_t>(blockIdx.x) * stretch;
  if (first64 >= bw) return;  // (the whole workgroup)
  const uint32_t first = static_cast<uint32_t>(first64);
  const uint32_t last = bw - first < stretch ? bw : first + stretch;
  for (int64_t r = blockIdx.y; r < nrows; r += gridDim.y) {
    const int64_t s = rows[r];
    if (s < 0 || static_cast<uint64_t>(s) >= slots) continue;  // (the whole workgroup)
    const uint32_t* row = table + static_cast<size_t>(s) * bw;
    uint32_t acc = 0u;
    for (uint32_t i0 = first; i0 < last; i0 += kHllBlock) {
      const uint32_t i = i0 + lane * kFoldWaves + wave;  // the step's words dealt round to the waves
      uint32_t b = 0u;
      if (i < last) {
        b = row[i];
        const uint32_t left = card - i * 32u;  // >= 1 for i < bw
        if (i + 1u == bw && left < 32u) b &= (1u << left) - 1u;
      }
      // (also: the previous step's readers are done with ids, the previous row's with part)
      if (!__syncthreads_or(b != 0u)) continue;
      const uint32_t c = __builtin_popcount(b);
      uint32_t inc = c;
      for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
      }
      const uint32_t total = __shfl(inc, 63);  // <= 2,048
      uint32_t pos = inc - c;
      while (b) {
        ids[wave][pos++] = static_cast<uint16_t>(lane * 32u + static_cast<uint32_t>(__builtin_ctz(b)));
        b &= b - 1u;
      }
      __syncthreads();
      const uint32_t w0 = i0 + wave;  // the wave's first word; entry e: word w0 + 4 * (e >> 5), bit e & 31
      for (uint32_t k = 0; k < total; k += kFoldBatch) {
        uint32_t v[kFoldBatch];
#pragma unroll
        for (int u = 0; u < kFoldBatch; ++u) {  // past the list's end: its last entry again
          const uint32_t j = __builtin_elementwise_min(k + static_cast<uint32_t>(u), total - 1u);
          const uint32_t e = ids[wave][j];
          const size_t id = static_cast<size_t>(w0 + (e >> 5) * kFoldWaves) * 32u + (e & 31u);
          v[u] = image[id * (kHllRegs / 4) + lane];
        }
#pragma unroll
        for (int u = 0; u < kFoldBatch; ++u) acc = fold_max4(acc, v[u]);
      }
    }
    part[wave][lane] = acc;
    __syncthreads();
    uint32_t m = 0u;
#pragma unroll
    for (int w = 0; w < kFoldWaves; ++w)
      m = __builtin_elementwise_max(m, (part[w][threadIdx.x >> 2] >> (8u * (threadIdx.x & 3u))) & 0xFFu);
    uint32_t* o = out + static_cast<size_t>(r) * kHllRegs + threadIdx.x;
    if (m != 0u && *o < m) atomicMax(o, m);
  }
}

}  // namespace pgx

// Workgroups a row of a dictionary of `card` values is shared by: one per kFoldSplitWords bitmap words, up to 64.
extern "C" int pgx_fasthll_fold_split(int32_t card) {
  if (card < 1) return 0;
  const uint32_t bw = pgx::fold_bitmap_words(card);
  return static_cast<int>(std::min<uint32_t>(64u, (bw + pgx::kFoldSplitWords - 1u) / pgx::kFoldSplitWords));
}

// table: slots rows of (card + 31) / 32 words; image: card x 64 dwords, four registers below 128 to a dword; rows:
// nrows row indexes (int64, device) and check, the caller's host copy of them, which is what gets validated; out:
// nrows x 256 u32 registers (device), zeroed or holding what earlier launches folded.  Grid:
// pgx_fasthll_fold_split(card) x wgs.
extern "C" hipError_t pgx_launch_fasthll_fold(const uint32_t* table, int32_t card, const uint32_t* image,
                                              const int64_t* rows, const int64_t* check, int64_t nrows, int64_t slots,
                                              uint32_t* out, int wgs, hipStream_t stream) {
  if (!table || !image || !rows || !check || !out || card < 1 || nrows < 0 || nrows > pgx::kHllMaxGroupSlots ||
      slots < 1 || slots > pgx::kHllMaxGroupSlots || wgs < 1 || wgs > 65535)
    return hipErrorInvalidValue;
  for (int64_t i = 0; i < nrows; ++i)
    if (check[i] < 0 || check[i] >= slots) return hipErrorInvalidValue;
  if (nrows == 0) return hipSuccess;
  const int per_row = pgx_fasthll_fold_split(card);
  hipLaunchKernelGGL(pgx::pgx_fasthll_fold, dim3(static_cast<unsigned>(per_row), static_cast<unsigned>(wgs)),
                     dim3(pgx::kHllBlock), 0, stream, table, static_cast<uint32_t>(card), image, rows, nrows,
                     static_cast<uint64_t>(slots), out);
  return hipGetLastError();
}
