// libpgx: the bitmap inverted-index kernels and their launchers (the a-7 stage of the query hot path, pgx_kernels.hip).
// Reference paths are relative to pinot-core/src/main/java/com/linkedin/pinot/core/.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "pgx_device.h"
#include "pgx_internal.h"
#include "pgx_roaring_device.h"

namespace pgx {

// ---------------------------------------------------------------------------------------------
// a-7: bitmap inverted-index leaves (the format, the field reads, the container search and cursor, the element spread
// and the workgroup expander pgx_rexpand are pgx_roaring_device.h, shared with the generated query kernels).  One
// workgroup expands one 65536-doc chunk of one (segment, leaf): each lane searches one bitmap's container keys for the
// chunk, then the workgroup ORs the found containers into an 8 KiB LDS mask and writes the 2048 mask words to HBM with
// coalesced stores.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ const PGX_G JRDesc* gdescs(const RDesc* descs) { return (const PGX_G JRDesc*)descs; }

// Leaf table of one leaf: descriptor a (-1: the empty leaf, no bitmaps).
__device__ __forceinline__ PgxRLeavesReg<1> one_leaf(const RDesc* descs, int a) {
  PgxRLeavesReg<1> L;
  L.desc[0] = a;
  L.b0[0] = 0;
  L.total = a >= 0 ? descs[a].nb : 0;
  return L;
}

__global__ void __launch_bounds__(256) pgx_roaring_expand(const RDesc* __restrict__ descs, int npairs, int maxchunks) {
  const int pair = static_cast<int>(blockIdx.x / maxchunks);
  const int chunk = static_cast<int>(blockIdx.x - static_cast<unsigned>(pair) * maxchunks);
  if (pair >= npairs) return;
  const RDesc& D = descs[pair];
  if (chunk >= D.nchunks) return;
  __shared__ uint32_t m[2048];
  __shared__ PgxRScratch S;
  const int tid = threadIdx.x;
  pgx_rexpand<256>(one_leaf(descs, pair), gdescs(descs), chunk, m, S);
  uint32_t* out = D.mask + static_cast<size_t>(chunk) * 2048;
  for (int i = tid; i < 2048; i += 256) out[i] = m[i];
}

// AND / OR / NOT over bitmap leaves for one 65536-doc chunk (AndBlockDocIdSet.fastIterator's bitmap AND,
// OrBlockDocIdSet's bitmap OR, BitmapDocIdSet's exclusion flip): a stack of LDS masks, each leaf expanded on its own
// into the top of the stack, the result written once.  One workgroup per (program, chunk).  The fallback for programs
// of more than kRProgMaxLeaves leaves.
constexpr int kRProgStack = 4;
__global__ void __launch_bounds__(256) pgx_roaring_program(const RProg* __restrict__ progs, const RDesc* __restrict__ descs,
                                                           int nprogs, int maxchunks) {
  const int pi = static_cast<int>(blockIdx.x / maxchunks);
  const int chunk = static_cast<int>(blockIdx.x - static_cast<unsigned>(pi) * maxchunks);
  if (pi >= nprogs) return;
  const RProg& P = progs[pi];
  if (chunk >= P.nchunks) return;
  __shared__ uint32_t stk[kRProgStack][2048];
  __shared__ PgxRScratch S;
  const int tid = threadIdx.x;
  const int64_t doc0 = static_cast<int64_t>(chunk) << 16;
  int sp = 0;
  for (int i = 0; i < P.nops; ++i) {
    const int op = P.op[i];
    if (op == RP_LEAF) {
      pgx_rexpand<256>(one_leaf(descs, P.arg[i]), gdescs(descs), chunk, stk[sp], S);
      ++sp;
    } else if (op == RP_NOT) {
      uint32_t* m = stk[sp - 1];
      for (int w = tid; w < 2048; w += 256) m[w] = ~m[w] & pgx_rkeep(doc0 + 32 * w, P.num_docs);
    } else {
      uint32_t* a = stk[sp - 2];
      const uint32_t* b = stk[sp - 1];
      for (int w = tid; w < 2048; w += 256) a[w] = op == RP_AND ? (a[w] & b[w]) : (a[w] | b[w]);
      --sp;
    }
    __syncthreads();
  }
  uint32_t* out = P.mask + static_cast<size_t>(chunk) * 2048;
  for (int w = tid; w < 2048; w += 256) out[w] = stk[0][w];
}

// The AND / OR / NOT program for mask word w of `chunk` in registers, over the leaf masks lm[leaf * 2048 + w] (leaves
// in program order).
constexpr int kRProgMaxLeaves = PGX_J_MAX_RLEAVES;
__device__ __forceinline__ uint32_t rprog_word(const RProg& P, const uint32_t* lm, int chunk, int w) {
  uint32_t st[kRProgMaxLeaves];
  int sp = 0, leaf = 0;
  const uint32_t keep = pgx_rkeep((static_cast<int64_t>(chunk) << 16) + 32 * w, P.num_docs);
  for (int i = 0; i < P.nops; ++i) {
    const int op = P.op[i];
    if (op == RP_LEAF) {
      st[sp++] = lm[leaf * 2048 + w];
      ++leaf;
    } else if (op == RP_NOT) {
      st[sp - 1] = ~st[sp - 1] & keep;
    } else {
      st[sp - 2] = op == RP_AND ? (st[sp - 2] & st[sp - 1]) : (st[sp - 2] | st[sp - 1]);
      --sp;
    }
  }
  return st[0];
}

// The same program with every leaf expanded at once (pgx_rexpand over all its leaves), then the AND / OR / NOT program
// evaluated per mask word in registers and written straight out.  The dependent global-load chain is that of ONE leaf,
// not one per leaf (C5: 3 leaves, 34 bitmaps), and the LDS holds exactly the program's leaf masks (dynamic LDS,
// nleaves x 8 KiB).
__global__ void __launch_bounds__(256) pgx_roaring_program_wide(const RProg* __restrict__ progs,
                                                                const RDesc* __restrict__ descs, int nprogs,
                                                                int maxchunks) {
  const int pi = static_cast<int>(blockIdx.x / maxchunks);
  const int chunk = static_cast<int>(blockIdx.x - static_cast<unsigned>(pi) * maxchunks);
  if (pi >= nprogs) return;
  const RProg& P = progs[pi];
  if (chunk >= P.nchunks) return;
  extern __shared__ uint32_t lmask[];  // [leaf][2048]
  __shared__ PgxRScratch S;
  __shared__ int leaf_desc[kRProgMaxLeaves], leaf_b0[kRProgMaxLeaves + 1], nleaves;
  const int tid = threadIdx.x;
  if (tid == 0) {
    int nl = 0, tot = 0;
    for (int i = 0; i < P.nops; ++i)
      if (P.op[i] == RP_LEAF) {
        const int a = P.arg[i];
        leaf_desc[nl] = a;
        leaf_b0[nl] = tot;
        tot += a >= 0 ? descs[a].nb : 0;
        ++nl;
      }
    leaf_b0[nl] = tot;
    nleaves = nl;
  }
  __syncthreads();
  const PgxRLeavesLds L{leaf_desc, leaf_b0, nleaves, leaf_b0[nleaves]};
  pgx_rexpand<256>(L, gdescs(descs), chunk, lmask, S);
  __syncthreads();
  uint32_t* out = P.mask + static_cast<size_t>(chunk) * 2048;
  for (int w = tid; w < 2048; w += 256) out[w] = rprog_word(P, lmask, chunk, w);
}

// One workgroup per (segment, program), walking the segment's 65536-doc chunks in order.  Every bitmap of the program
// (<= kSegRBitmaps, one lane each) keeps a cursor into its sorted container keys, and the key / cardinality / offset of
// its NEXT container are loaded while the current chunk is expanded, so a chunk costs the element and bitmap-word loads
// only (the per-chunk kernels above pay a container search of four dependent loads per chunk).  Array elements spread
// over all lanes (4 loads in flight each), bitmap-container words too; the AND / OR / NOT program is evaluated per mask
// word in registers and the chunk's mask written out.  Its barriers order LDS only (pgx_lds_barrier): the
// container-field prefetches and the previous chunk's mask stores stay in flight across every phase of the chunk loop.
constexpr int kSegRThreads = 512;
constexpr int kSegRBitmaps = 512;
__global__ void __launch_bounds__(kSegRThreads, 8) pgx_roaring_program_seg(const RProg* __restrict__ progs,
                                                                        const RDesc* __restrict__ descs, int nprogs,
                                                                        int parts) {
  // `parts` workgroups per segment, each walking a contiguous range of its chunks: short segment lists (a batch of a
  // long query) still put enough workgroups on the chip
  const int pi = static_cast<int>(blockIdx.x) / parts;
  if (pi >= nprogs) return;
  const RProg& P = progs[pi];
  const int per = (P.nchunks + parts - 1) / parts;
  const int c0 = (static_cast<int>(blockIdx.x) % parts) * per;
  const int c1 = min(P.nchunks, c0 + per);
  if (c0 >= c1) return;
  extern __shared__ uint32_t lmask[];  // [leaf][2048]
  __shared__ const uint8_t* cptr[kSegRBitmaps];
  __shared__ int ccard[kSegRBitmaps], cpre[kSegRBitmaps + 1], cleaf[kSegRBitmaps];
  __shared__ int ncont;
  __shared__ int bidx[kSegRBitmaps], nbm;
  const int tid = threadIdx.x;
  // leaves in program order (uniform loads); lane tid < total bitmaps owns bitmap (tid - first) of leaf `leaf`
  int nl = 0, tot = 0, leaf = 0, my_desc = -1, my_first = 0;
  for (int i = 0; i < P.nops; ++i)
    if (P.op[i] == RP_LEAF && nl < kRProgMaxLeaves) {
      const int a = P.arg[i];
      const int nb = a >= 0 ? descs[a].nb : 0;
      if (tid >= tot && tid < tot + nb) {
        leaf = nl;
        my_desc = a;
        my_first = tot;
      }
      tot += nb;
      ++nl;
    }
  // this lane's bitmap and the fields of its first container at or after c0 (the host launches this kernel only when
  // the program's bitmaps number <= kSegRBitmaps)
  PgxRCursor cu;
  if (my_desc >= 0) cu.seek(pgx_rbitmap(gdescs(descs) + my_desc, tid - my_first), c0);
  constexpr int kPer = 4;  // array elements in flight per lane (8 costs a quarter of the workgroups per CU)
  for (int chunk = c0; chunk < c1; ++chunk) {
    for (int i = tid; i < nl * 2048; i += kSegRThreads) lmask[i] = 0u;
    if (tid == 0) ncont = 0;
    pgx_lds_barrier();
    if (cu.key() == chunk) {
      const int slot = atomicAdd(&ncont, 1);
      cptr[slot] = cu.ptr();
      ccard[slot] = cu.card();
      cleaf[slot] = leaf;
      cu.advance();  // prefetches the next container's fields (consumed at a later chunk)
    }
    pgx_lds_barrier();
    const int nc = ncont;
    if (tid < 64) pgx_rcard_prefix<kSegRBitmaps / 64, true>(tid, nc, ccard, cpre, &cpre[kSegRBitmaps], bidx, &nbm);
    pgx_lds_barrier();
    const int ne = cpre[kSegRBitmaps];
    const int nbc = nbm;
    // the first bitmap container's words are requested before the array elements, so both round trips overlap
    uint32_t bw[2048 / kSegRThreads];
    if (nbc > 0) pgx_rwords_load<kSegRThreads>(cptr[bidx[0]], tid, bw);
    pgx_rspread<kSegRThreads, kPer>(tid, nc, ne, cptr, cpre, cleaf, lmask);
    for (int i = 0; i < nbc; ++i) {  // bitmap containers: all words in flight, then the ORs
      const int k = bidx[i];
      if (i > 0) pgx_rwords_load<kSegRThreads>(cptr[k], tid, bw);
      pgx_rwords_or<kSegRThreads>(lmask + cleaf[k] * 2048, tid, bw);
    }
    pgx_lds_barrier();
    uint32_t* out = P.mask + static_cast<size_t>(chunk) * 2048;
    for (int w = tid; w < 2048; w += kSegRThreads) out[w] = rprog_word(P, lmask, chunk, w);
    pgx_lds_barrier();  // lmask is zeroed for the next chunk
  }
}

// Wave-per-chunk form of the bitmap programs: every wavefront walks its own range of one segment's chunks with its own
// LDS masks, and the workgroup never synchronises (the workgroup kernel above spends most of a chunk waiting at five
// barriers for its slowest wave).  Lane b owns bitmap b of the program (<= 64 bitmaps) and its container cursor.
// Leaves share mask slots by the plan of pgx_internal.h RPlan (the host sizes the launch by the same walker): phase 0
// ORs containers into their leaf's slot, phase 1 clears the AND-NOT leaves' containers out of theirs.  The rest of the
// postfix program is evaluated over the slots and the chunk's mask written.
//
// The wide reader (WIDE, the default).  The phases order the LDS updates, not the loads: a chunk starts by requesting a
// round of phase 0 array granules and the first half of its first bitmap container, of either phase (C5: everything but
// the second half of its one bitmap container), before the first update.  Array containers are read as naturally
// aligned 16-byte granules, the granules of all containers of the chunk spread over the lanes by a prefix over granule
// counts (phase 0 containers first, then phase 1's: each phase is a range of granules).  A granule's halves before the
// container's first element or after its last belong to a neighbouring container (the next chunk's) or to a header,
// and are masked off.  Bitmap containers are read as 16 bytes per lane from the dword at or below their first byte and,
// at 2 modulo 4, shifted together with the next lane's first dword.  The read contract (pgx_jit_abi.h JRDesc::inv): a
// load touches only naturally aligned granules of at most 16 bytes that overlap the container's own bytes.  A lane owns
// mask words 4t .. 4t + 3 (t = 64 j + lane), so bitmap containers, the program over the slots, the mask store and the
// clearing all move 16 bytes per lane.  Held per lane: 7 granules, their 7 marks and half a bitmap container (4 x 16
// bytes): 8 granules spill at the 128 VGPRs of four waves per SIMD, and so does a whole bitmap container beside them.
// WIDE = false (PGX_DEBUG=rnarrow) is the reader this one replaced, kept for the A/B and the tests: a prefix over
// element counts, two-byte loads, one phase after the other, mask word j * 64 + lane.
constexpr int kWaveGranules = 7;  // granules per lane of one round of array containers: 448 (C5: ~370 per chunk)
constexpr int kWaveNarrowElems = 16;  // WIDE = false: array elements per lane in flight
typedef u32 pgx_u32x4_dw __attribute__((ext_vector_type(4), aligned(4)));  // 16 bytes at any dword

// Granules base + 64 q + lane (below `end`) of the chunk's array containers: container k holds granules pre[k] ..
// pre[k + 1] - 1, starts at byte ptrs[k] and has meta[k] & 0xFFFF elements; its mask slot starts at word meta[k] >> 16.
// am[q]: bits 0-7 the granule's halves that are elements of the container, bits 8.. the slot's first word.  Lanes past
// the last granule load it again with no half valid: no branch around the load (pgx_rspread says why).
template <int B>
__device__ __forceinline__ void wave_granules_load(int base, int end, int lane, const int* pre,
                                                   const uint8_t* const* ptrs, const int* meta, pgx_u32x4 (&A)[B],
                                                   u32 (&am)[B]) {
#pragma unroll
  for (int q = 0; q < B; ++q) {
    const int gi = base + 64 * q + lane, g = min(gi, end - 1);
    int k = 0;
#pragma unroll
    for (int step = 32; step > 0; step >>= 1)
      if (pre[k + step] <= g) k += step;  // largest k <= 63 with pre[k] <= g (pre[k] is the total past the last)
    const uintptr_t s = reinterpret_cast<uintptr_t>(ptrs[k]);
    const int m = meta[k];
    const uintptr_t ga = (s & ~static_cast<uintptr_t>(15)) + 16 * static_cast<uintptr_t>(g - pre[k]);
    A[q] = *(const PGX_G pgx_u32x4*)ga;
    const int first = max(static_cast<int>(s - ga), 0) >> 1;
    const int last = min(static_cast<int>(s + 2 * (m & 0xFFFF) - ga), 16) >> 1;  // 1 .. 8: the granule overlaps
    const u32 vm = gi < end ? (0xFFu >> (8 - last)) & (0xFFu << first) & 0xFFu : 0u;
    am[q] = vm | static_cast<u32>(m >> 16) << 8;
  }
}
// The LDS updates of one round's granules: OR the elements in (PH 0) or clear them out (PH 1).
template <int PH, int B>
__device__ __forceinline__ void wave_granules_apply(u32* sm, const pgx_u32x4 (&A)[B], const u32 (&am)[B]) {
#pragma unroll
  for (int q = 0; q < B; ++q) {
    u32* d = sm + (am[q] >> 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const u32 w = A[q][i >> 1];
      const u32 v = (i & 1) ? w >> 16 : w & 0xFFFFu;
      if ((am[q] >> i) & 1u) {
        if (PH == 0) atomicOr(&d[v >> 5], 1u << (v & 31u));
        else atomicAnd(&d[v >> 5], ~(1u << (v & 31u)));
      }
    }
  }
}
// Bitmap container at byte c (any 2-byte alignment; wave-uniform), its 16-byte groups 64 j + lane for j = J0 .. J0 + H
// - 1, counted from the dword at or below c.  At 2 modulo 4 a group's last two bytes lie in the next lane's first
// dword; `tail` is the dword after the H groups (lane 0), which at J0 + H = 8 holds the container's last two bytes.
template <int J0, int H>
__device__ __forceinline__ void wave_words_load(uintptr_t c, int lane, pgx_u32x4 (&W)[H], u32& tail) {
  const PGX_G unsigned char* cb = (const PGX_G unsigned char*)(c & ~static_cast<uintptr_t>(3));
#pragma unroll
  for (int j = 0; j < H; ++j) W[j] = *(const PGX_G pgx_u32x4_dw*)(cb + static_cast<u32>(16 * (64 * (J0 + j) + lane)));
  tail = 0u;
  if ((c & 2) && lane == 0) tail = *(const PGX_G u32*)(cb + 1024u * (J0 + H));
}
// ORs those groups into (PH 0) or clears them out of (PH 1) the slot m, words 4t .. 4t + 3 of t = 64 j + lane.  No
// other lane touches these words here and a wave's LDS operations complete in order, so the update is a plain one.
template <int PH, int J0, int H>
__device__ __forceinline__ void wave_words_apply(u32* m, uintptr_t c, int lane, const pgx_u32x4 (&W)[H], u32 tail) {
  const u32 sh = (c & 2) ? 16u : 0u;
  pgx_u32x4* m4 = reinterpret_cast<pgx_u32x4*>(m) + 64 * J0 + lane;
#pragma unroll
  for (int j = 0; j < H; ++j) {
    // the dword after this lane's 16 bytes: the next lane's first, for lane 63 lane 0's of the next group
    const u32 wrap = __builtin_amdgcn_readfirstlane(j < H - 1 ? W[(j + 1) % H].x : tail);
    const u32 up = __shfl(W[j].x, (lane + 1) & 63, 64);
    const u32 next = lane == 63 ? wrap : up;
    pgx_u32x4 o;
    o.x = __builtin_amdgcn_alignbit(W[j].y, W[j].x, sh);
    o.y = __builtin_amdgcn_alignbit(W[j].z, W[j].y, sh);
    o.z = __builtin_amdgcn_alignbit(W[j].w, W[j].z, sh);
    o.w = __builtin_amdgcn_alignbit(next, W[j].w, sh);
    const pgx_u32x4 cur = m4[64 * j];
    m4[64 * j] = PH == 0 ? (cur | o) : (cur & ~o);
  }
}
// Inclusive prefix sum over the wave's lanes in registers: shifts inside each row of 16 lanes, then each row's total
// broadcast into the rows after it (lanes without a source add 0).
__device__ __forceinline__ int wave_prefix_sum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);  // row_bcast:15 into rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);  // row_bcast:31 into rows 2 and 3
  return v;
}
__device__ __forceinline__ int wave_bits_below(uint64_t m) {  // set bits of m below this lane
  return static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<u32>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<u32>(m), 0u)));
}
__device__ __forceinline__ uintptr_t wave_lane_ptr(uintptr_t v, int src) {  // lane src's v (src wave-uniform)
  const u32 lo = __builtin_amdgcn_readlane(static_cast<u32>(v), src);
  const u32 hi = __builtin_amdgcn_readlane(static_cast<u32>(v >> 32), src);
  return (static_cast<uintptr_t>(hi) << 32) | lo;
}

template <int NS, int WPB, int MINW, bool WIDE>
__global__ void __launch_bounds__(64 * WPB, MINW) pgx_roaring_program_wave(const RProg* __restrict__ progs,
                                                                          const RDesc* __restrict__ descs, int nprogs,
                                                                          int parts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t wmask[];  // [wave][NS][2048]
  __shared__ int wpre[WPB][65];
  __shared__ const uint8_t* wptr[WPB][64];
  __shared__ int wslot[WPB][64];
  const int lane = static_cast<int>(threadIdx.x) & 63, wv = static_cast<int>(threadIdx.x) >> 6;
  // (the wave's number through readfirstlane: the compiler then knows that the program is wave-uniform and reads it,
  // every chunk's walk over its ops included, with scalar loads)
  const int gw = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * WPB + wv);
  const int pi = gw / parts;
  if (pi >= nprogs) return;  // per wave: nothing below synchronises the workgroup
  const RProg& P = progs[pi];
  const int per = (P.nchunks + parts - 1) / parts;
  const int c0 = (gw % parts) * per;
  const int c1 = min(P.nchunks, c0 + per);
  if (c0 >= c1) return;
  uint32_t* sm = wmask + wv * NS * 2048;
  pgx_u32x4* sm4 = reinterpret_cast<pgx_u32x4*>(sm);
  int* pre = wpre[wv];
  const uint8_t** ptrs = wptr[wv];
  int* slots = wslot[wv];
  // slot plan: this lane's bitmap, its leaf's slot and phase
  int my_desc = -1, my_first = 0, my_slot = 0, my_phase = 0;
  bool any_andnot = false, rest = false;  // rest: ops are left for after the expansion (C5: none, all fused)
  int top_slot = 0;
  {
    RPlan plan;
    int tot = 0;
    for (int i = 0; i < P.nops;) {
      const bool is_leaf = P.op[i] == RP_LEAF;
      const int a = P.arg[i];
      i += plan.step(P, i);  // a fused OR / NOT, AND is done by the expansion itself
      top_slot = plan.top();
      rest |= !is_leaf;
      if (!is_leaf) continue;
      const int nb = a >= 0 ? descs[a].nb : 0;
      if (lane >= tot && lane < tot + nb) {
        my_desc = a;
        my_first = tot;
        my_slot = plan.slot;
        my_phase = plan.phase;
      }
      tot += nb;
      any_andnot |= plan.phase != 0;
    }
  }
  PgxRCursor cu;
  if (my_desc >= 0) cu.seek(pgx_rbitmap(gdescs(descs) + my_desc, lane - my_first), c0);
#pragma unroll
  for (int s = 0; s < NS; ++s)
    for (int j = 0; j < 32; ++j) sm[s * 2048 + j * 64 + lane] = 0u;
  // the mask is written 16 bytes per lane where it is 16-byte aligned (chunks are 8 KiB apart)
  const bool out16 = (reinterpret_cast<uintptr_t>(P.mask) & 15u) == 0;
  for (int chunk = c0; chunk < c1; ++chunk) {
    const bool act = cu.key() == chunk;
    const uint8_t* cptr = cu.ptr();
    const int ccard = cu.card();
    if (act) cu.advance();  // now: the next container's fields are consumed at a later chunk
    if constexpr (WIDE) {
      constexpr int B = kWaveGranules;
      const uintptr_t cs = reinterpret_cast<uintptr_t>(cptr);
      const bool arr = act && ccard <= 4096, p1 = my_phase != 0;
      // granules of this lane's array container, phase 0 counted in the low half and phase 1 in the high half of one
      // prefix (<= 64 x 513 each)
      const int ng = arr ? static_cast<int>(((cs + 2 * ccard - 1) >> 4) - (cs >> 4)) + 1 : 0;
      const u32 v = p1 ? static_cast<u32>(ng) << 16 : static_cast<u32>(ng);
      const u32 incl = static_cast<u32>(wave_prefix_sum(static_cast<int>(v)));
      const u32 tot = __builtin_amdgcn_readlane(incl, 63);
      const int t0 = static_cast<int>(tot & 0xFFFFu), t = t0 + static_cast<int>(tot >> 16);
      // container records in phase order: the phase 0 containers by lane, then the phase 1 containers by lane
      const uint64_t a0 = __ballot(arr && !p1), a1 = __ballot(arr && p1);
      const int n0 = __popcll(a0), na = n0 + __popcll(a1);
      if (arr) {
        const int rank = p1 ? n0 + wave_bits_below(a1) : wave_bits_below(a0);
        pre[rank] = p1 ? t0 + static_cast<int>((incl - v) >> 16) : static_cast<int>((incl - v) & 0xFFFFu);
        ptrs[rank] = cptr;
        slots[rank] = ccard | (my_slot * 2048) << 16;
      }
      if (lane >= na) pre[lane] = t;
      if (lane == 63) pre[64] = t;
      uint64_t b0 = __ballot(act && !arr && !p1), b1 = __ballot(act && !arr && p1);
      pgx_wave_lds_sync();
      // requests first: a round of phase 0 granules and half of the first bitmap container, of either phase.  Then the
      // updates in phase order; within a phase they commute, so phase 1 takes its bitmap containers first (the held
      // half is theirs when phase 0 has none) and loads its own array granules after them.
      pgx_u32x4 A[B], W0[4];
      u32 am[B], tail0 = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) W0[j] = pgx_u32x4{0u, 0u, 0u, 0u};  // (defined on every path: not kept across chunks)
      const int held = b0 ? __builtin_ctzll(b0) : (b1 ? __builtin_ctzll(b1) : -1);
      if (t0 > 0) {  // (one block, every load of A followed by its updates on every path: no wait for A outside it)
        wave_granules_load<B>(0, t0, lane, pre, ptrs, slots, A, am);
        if (held >= 0) wave_words_load<0, 4>(wave_lane_ptr(cs, held), lane, W0, tail0);
        for (int base = 0;;) {
          wave_granules_apply<0, B>(sm, A, am);
          base += 64 * B;
          if (base >= t0) break;
          wave_granules_load<B>(base, t0, lane, pre, ptrs, slots, A, am);
        }
      } else if (held >= 0) {
        wave_words_load<0, 4>(wave_lane_ptr(cs, held), lane, W0, tail0);
      }
      while (b0) {
        const int src = __builtin_ctzll(b0);
        b0 &= b0 - 1;
        const uintptr_t c = wave_lane_ptr(cs, src);
        u32* m = sm + __builtin_amdgcn_readlane(my_slot, src) * 2048;
        pgx_u32x4 W1[4];
        u32 tail1;
        if (src != held) wave_words_load<0, 4>(c, lane, W0, tail0);
        wave_words_load<4, 4>(c, lane, W1, tail1);
        wave_words_apply<0, 0, 4>(m, c, lane, W0, tail0);
        wave_words_apply<0, 4, 4>(m, c, lane, W1, tail1);
      }
      if (t > t0 || b1) {
        pgx_wave_lds_sync();
        while (b1) {
          const int src = __builtin_ctzll(b1);
          b1 &= b1 - 1;
          const uintptr_t c = wave_lane_ptr(cs, src);
          u32* m = sm + __builtin_amdgcn_readlane(my_slot, src) * 2048;
          pgx_u32x4 W1[4];
          u32 tail1;
          if (src != held) wave_words_load<0, 4>(c, lane, W0, tail0);
          wave_words_load<4, 4>(c, lane, W1, tail1);
          wave_words_apply<1, 0, 4>(m, c, lane, W0, tail0);
          wave_words_apply<1, 4, 4>(m, c, lane, W1, tail1);
        }
        for (int base = t0; base < t; base += 64 * B) {
          wave_granules_load<B>(base, t, lane, pre, ptrs, slots, A, am);
          wave_granules_apply<1, B>(sm, A, am);
        }
      }
      pgx_wave_lds_sync();
      // the rest of the program over the slots (the plan's walk again), words 4t .. 4t + 3 of t = 64 j + lane; result
      // written, slots cleared
      const int64_t doc0 = static_cast<int64_t>(chunk) << 16;
      RPlan plan;
      for (int i = 0; rest && i < P.nops;) {
        const int op = P.op[i];
        i += plan.step(P, i);
        if (op == RP_LEAF) continue;
        pgx_u32x4* a = sm4 + plan.slot * 512;
        if (op == RP_NOT) {
#pragma unroll 2
          for (int j = 0; j < 8; ++j) {
            const int w = 4 * (64 * j + lane);
            pgx_u32x4 x = a[64 * j + lane];
            x.x = ~x.x & pgx_rkeep(doc0 + 32 * w, P.num_docs);
            x.y = ~x.y & pgx_rkeep(doc0 + 32 * (w + 1), P.num_docs);
            x.z = ~x.z & pgx_rkeep(doc0 + 32 * (w + 2), P.num_docs);
            x.w = ~x.w & pgx_rkeep(doc0 + 32 * (w + 3), P.num_docs);
            a[64 * j + lane] = x;
          }
        } else {
          const pgx_u32x4* b = sm4 + plan.rhs * 512;
          if (op == RP_AND) {
#pragma unroll
            for (int j = 0; j < 8; ++j) a[64 * j + lane] &= b[64 * j + lane];
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) a[64 * j + lane] |= b[64 * j + lane];
          }
        }
      }
      const pgx_u32x4* r = sm4 + top_slot * 512;
      PGX_G uint32_t* out = (PGX_G uint32_t*)P.mask + static_cast<size_t>(chunk) * 2048;
      if (out16) {
#pragma unroll
        for (int j = 0; j < 8; ++j) ((PGX_G pgx_u32x4*)out)[64 * j + lane] = r[64 * j + lane];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) ((PGX_G pgx_u32x4_dw*)out)[64 * j + lane] = r[64 * j + lane];
      }
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) sm4[s * 512 + 64 * j + lane] = pgx_u32x4{0u, 0u, 0u, 0u};
      pgx_wave_lds_sync();
      continue;
    }
    // WIDE = false from here to the end of the chunk
    for (int ph = 0; ph < (any_andnot ? 2 : 1); ++ph) {
      const bool mine = act && my_phase == ph;
      const bool arr = mine && ccard <= 4096;
      const int v = arr ? ccard : 0;
      int incl = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
      }
      const int total = __shfl(incl, 63, 64);
      pre[lane] = incl - v;
      if (lane == 63) pre[64] = incl;
      ptrs[lane] = mine ? cptr : nullptr;
      slots[lane] = my_slot;
      uint64_t bm = __ballot(mine && ccard > 4096);
      pgx_wave_lds_sync();
      // array containers: element e of the chunk's concatenated containers, container k with pre[k] <= e < pre[k + 1];
      // the lane's first element by one search, later ones (64 apart) by stepping forward (about one step each)
      if (total > 0) {
        int k = 0;
#pragma unroll
        for (int step = 32; step > 0; step >>= 1)
          if (pre[k + step] <= lane) k += step;  // largest k <= 63 with pre[k] <= lane
        int kend = pre[k + 1], kbeg = pre[k];
        const uint8_t* kp = ptrs[k];
        int ks = slots[k];
        constexpr int B = kWaveNarrowElems;
        for (int e0 = lane; e0 < total; e0 += 64 * B) {
          uint32_t val[B];
          int dst[B];
#pragma unroll
          for (int q = 0; q < B; ++q) {
            const int e = e0 + 64 * q;
            dst[q] = -1;
            if (e < total) {
              while (kend <= e) {
                ++k;
                kbeg = kend;
                kend = pre[k + 1];
                kp = ptrs[k];
                ks = slots[k];
              }
              val[q] = pgx_rd16(kp + 2 * (e - kbeg));
              dst[q] = ks * 2048;
            }
          }
#pragma unroll
          for (int q = 0; q < B; ++q)
            if (dst[q] >= 0) {
              if (ph == 0) atomicOr(&sm[dst[q] + (val[q] >> 5)], 1u << (val[q] & 31u));
              else atomicAnd(&sm[dst[q] + (val[q] >> 5)], ~(1u << (val[q] & 31u)));
            }
        }
      }
      // bitmap containers: 16 words per lane in flight at a time, ORed into (or cleared out of) the leaf's slot
      while (bm) {
        const int src = __builtin_ctzll(bm);
        bm &= bm - 1;
        const uint8_t* c = ptrs[src];
        uint32_t* m = sm + slots[src] * 2048;
        const bool al = (reinterpret_cast<uintptr_t>(c) & 3u) == 0;
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
          uint32_t x[16];
          if (al) {
            const PGX_G uint32_t* c32 = (const PGX_G uint32_t*)(c);
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = c32[(h * 16 + j) * 64 + lane];
          } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = pgx_rd32(c + 4 * ((h * 16 + j) * 64 + lane));
          }
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (x[j]) {
              if (ph == 0) atomicOr(&m[(h * 16 + j) * 64 + lane], x[j]);
              else atomicAnd(&m[(h * 16 + j) * 64 + lane], ~x[j]);
            }
        }
      }
      pgx_wave_lds_sync();
    }
    // the rest of the program over the slots (the plan's walk again), word j * 64 + lane; result written, slots cleared
    const int64_t doc0 = static_cast<int64_t>(chunk) << 16;
    uint32_t* out = P.mask + static_cast<size_t>(chunk) * 2048;
    RPlan plan;
    for (int i = 0; i < P.nops;) {
      const int op = P.op[i];
      i += plan.step(P, i);
      if (op == RP_LEAF) continue;
      uint32_t* a = sm + plan.slot * 2048;
      if (op == RP_NOT) {
#pragma unroll 4
        for (int j = 0; j < 32; ++j) {
          const int w = j * 64 + lane;
          a[w] = ~a[w] & pgx_rkeep(doc0 + 32 * w, P.num_docs);
        }
      } else {
        const uint32_t* b = sm + plan.rhs * 2048;
        if (op == RP_AND) {
#pragma unroll 8
          for (int j = 0; j < 32; ++j) a[j * 64 + lane] &= b[j * 64 + lane];
        } else {
#pragma unroll 8
          for (int j = 0; j < 32; ++j) a[j * 64 + lane] |= b[j * 64 + lane];
        }
      }
    }
    const uint32_t* r = sm + plan.top() * 2048;
#pragma unroll 8
    for (int j = 0; j < 32; ++j) out[j * 64 + lane] = r[j * 64 + lane];
    for (int s = 0; s < NS; ++s)
#pragma unroll 8
      for (int j = 0; j < 32; ++j) sm[s * 2048 + j * 64 + lane] = 0u;
    pgx_wave_lds_sync();
  }
}

}  // namespace pgx

extern "C" hipError_t pgx_launch_roaring(const pgx::RDesc* descs, int npairs, int maxchunks, hipStream_t stream) {
  if (npairs <= 0 || maxchunks <= 0) return hipSuccess;
  const long long blocks = static_cast<long long>(npairs) * maxchunks;
  if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pgx::pgx_roaring_expand, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, descs, npairs,
                     maxchunks);
  return hipGetLastError();
}

// Wave-per-chunk bitmap programs (host: every program <= 64 bitmaps and <= 3 slots).  The launcher has no context to
// take knobs from (the tests call it directly), so it reads its two A/B switches from PGX_DEBUG itself: rnarrow (the
// two-byte reader) and rparts=N (waves per segment).
namespace {
struct WaveKnobs {
  bool narrow = false;
  int parts = 0;
};
WaveKnobs wave_knobs() {
  WaveKnobs k;
  const char* e = std::getenv("PGX_DEBUG");
  while (e && *e) {
    const char* end = std::strchr(e, ',');
    const size_t n = end ? static_cast<size_t>(end - e) : std::strlen(e);
    if (n == 7 && std::strncmp(e, "rnarrow", 7) == 0) k.narrow = true;
    else if (n > 7 && std::strncmp(e, "rparts=", 7) == 0) k.parts = std::atoi(e + 7);
    e = end ? end + 1 : nullptr;
  }
  return k;
}
int device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  return cus;
}
}  // namespace

extern "C" hipError_t pgx_launch_roaring_program_wave(const pgx::RProg* progs, const pgx::RDesc* descs, int nprogs,
                                                      int maxchunks, int nslots, hipStream_t stream) {
  if (nprogs <= 0 || maxchunks <= 0) return hipSuccess;
  const WaveKnobs kn = wave_knobs();
  // two rounds of the 16 waves a CU holds with one mask slot (four per SIMD; 8,192 waves on 256 CUs), at most one wave
  // per chunk
  const int target = 2 * 16 * device_cus();
  int parts = std::max(1, std::min(maxchunks, kn.parts > 0 ? kn.parts : (target + nprogs - 1) / nprogs));
  const long long waves = static_cast<long long>(nprogs) * parts;
  // waves per SIMD the LDS allows (NS x 8 KiB per wave) bound the registers: 1 slot -> 4, 2 -> 2, 3 -> 1
#define PGX_WAVE_LAUNCH(NS, WPB, MINW, WIDE)                                                                       \
  hipLaunchKernelGGL((pgx::pgx_roaring_program_wave<NS, WPB, MINW, WIDE>),                                        \
                     dim3(static_cast<unsigned>((waves + WPB - 1) / WPB)), dim3(64 * WPB),                        \
                     static_cast<size_t>(NS) * WPB * 2048 * 4, stream, progs, descs, nprogs, parts)
  if (kn.narrow) {
    if (nslots <= 1) PGX_WAVE_LAUNCH(1, 4, 4, false);
    else if (nslots == 2) PGX_WAVE_LAUNCH(2, 2, 2, false);
    else PGX_WAVE_LAUNCH(3, 2, 1, false);
  } else {
    if (nslots <= 1) PGX_WAVE_LAUNCH(1, 4, 4, true);
    else if (nslots == 2) PGX_WAVE_LAUNCH(2, 2, 2, true);
    else PGX_WAVE_LAUNCH(3, 2, 1, true);
  }
#undef PGX_WAVE_LAUNCH
  return hipGetLastError();
}

extern "C" hipError_t pgx_launch_roaring_program(const pgx::RProg* progs, const pgx::RDesc* descs, int nprogs,
                                                 int maxchunks, int maxleaves, hipStream_t stream) {
  if (nprogs <= 0 || maxchunks <= 0) return hipSuccess;
  const long long blocks = static_cast<long long>(nprogs) * maxchunks;
  if (maxleaves < 0 && -maxleaves <= pgx::kRProgMaxLeaves) {  // per-segment walk (host: every program <= 512 bitmaps)
    // at least ~2048 workgroups (two full rounds at 4 resident per CU on 256 CUs), at most 8 parts per segment
    int parts = std::max(1, std::min(std::min(maxchunks, 8), (2048 + nprogs - 1) / nprogs));
      hipLaunchKernelGGL(pgx::pgx_roaring_program_seg, dim3(static_cast<unsigned>(nprogs * parts)),
                       dim3(pgx::kSegRThreads), static_cast<size_t>(-maxleaves) * 2048 * 4, stream, progs, descs,
                       nprogs, parts);
    return hipGetLastError();
  }
  if (maxleaves >= 1 && maxleaves <= pgx::kRProgMaxLeaves) {
    hipLaunchKernelGGL(pgx::pgx_roaring_program_wide, dim3(static_cast<unsigned>(blocks)), dim3(256),
                       static_cast<size_t>(maxleaves) * 2048 * 4, stream, progs, descs, nprogs, maxchunks);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(pgx::pgx_roaring_program, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, progs, descs,
                     nprogs, maxchunks);
  return hipGetLastError();
}
