// Internal host/device structures of libpgx (not part of the ABI).
#pragma once
#include <stdint.h>

#include "pgx_jit_abi.h"

namespace pgx {

constexpr int kTileRows = 8192;        // rows per workgroup tile = 256 lanes x 32 rows
constexpr int kLaneRows = 32;          // rows owned by one lane: exactly one 32-bit mask word
constexpr int kBlock = 256;            // threads per workgroup
constexpr int kMaxQCols = 16;          // distinct columns a query touches
constexpr int kMaxLeaves = 64;         // filter leaves of one query
constexpr int kInlineLeaves = PGX_J_MAX_LEAVES;  // leaf slots held inside KSeg / JSeg; the rest behind their xleaf
constexpr int kMaxLeafSlots = PGX_J_MAX_SLOTS;   // query leaves + bitmap-program masks + star-tree range leaves (the
                                                 // programs' int8_t arguments index them)
constexpr int kStarMaxLeaves = 8;      // star-tree plans: query leaves (their range leaves fill slots up to 16)
constexpr int kMaxAggs = 8;
constexpr int kMaxGroupCols = 16;
constexpr int kMaxProg = 192;          // generic kernel's program: a tree of L leaves emits at most L leaf ops, L - 1
                                       // pairwise folds and L OP_STATs, 3 * kMaxLeaves - 1 in all
constexpr int kStackDepth = 8;
constexpr uint64_t kEmptyKey = ~0ull;

enum LeafMode : int8_t {
  LEAF_SCAN_INTERVAL = 0,  // decode + lo <= id <= hi
  LEAF_SCAN_BITSET = 1,    // decode + bitset lookup
  LEAF_RANGES = 2,         // sorted doc ranges
  LEAF_NONE = 3,           // always false (empty binding)
  LEAF_DOCMASK = 4,        // query kernels: bitmap inverted-index leaf expanded to a per-segment doc mask
  LEAF_DOCMASK_NOT = 5,    // ... NEQ / NOT_IN: OR of the non-matching bitmaps, flipped (BitmapBasedFilterOperator)
  LEAF_RCHUNK = 6,         // query kernels: a bitmap program evaluated per 65536-doc chunk into LDS by the kernel
};

// Bitmap inverted-index expansion (pgx_roaring.hip pgx_roaring_expand): one descriptor per (segment, leaf).  The
// layout is shared with the generated query kernels (pgx_jit_abi.h JRDesc), which evaluate bitmap programs per chunk
// themselves (LEAF_RCHUNK).
//   mask: nchunks x 2048 words: bit (doc & 31) of word (doc >> 5); inv: device copy of <col>.bitmap.inv;
//   offs: byte offsets (into inv) of the roaring bitmaps to OR; nb: their number; nchunks: ceil(total_docs / 65536)
using RDesc = ::JRDesc;

// A sub-tree of the filter whose leaves are all bitmap inverted-index leaves, evaluated per 65536-doc chunk into ONE
// doc mask: by pgx_roaring_program into HBM, or inside the query kernel into LDS (LEAF_RCHUNK).  pgx_jit_abi.h JRProg.
constexpr int kMaxRProg = PGX_J_MAX_RPROG;
enum RProgOp : int8_t { RP_LEAF = 0, RP_AND = 1, RP_OR = 2, RP_NOT = 3 };
using RProg = ::JRProg;

// Slot plan of the wave-per-chunk kernel (pgx_roaring_program_wave), the one statement of its rule: the kernel's lane
// assignment, its evaluation and the host's choice of the kernel (pgx_host.cpp rprog_wave_slots) all step this walker.
// Leaves share mask "slots" while the slot's operand is still "pure" (an OR of leaves, nothing applied to it yet):
//   * a leaf directly followed by OR is ORed into the pure top operand's slot (phase 0);
//   * a leaf directly followed by NOT, AND is cleared out of the pure top operand's slot (phase 1: AND-NOT, after
//     every phase-0 container of the chunk), which leaves the slot impure;
//   * every other leaf takes a new slot.
// C5's (f1 IN .. OR f2 = 7) AND NOT f3 = 3 thus needs ONE 8 KiB slot per wave.  The operand stack is one 64-bit word of
// 4-bit entries (slot in bits 0-2, "pure" in bit 3, top in bits 0-3) and shifts on every binary op unconditionally, so
// only programs that pass fits() may be walked on the device.  Everything here is wave-uniform (scalar registers), and
// what a caller does not read (the device never reads depth, max_depth or ok) is dropped by the compiler.
#ifdef __HIPCC__
#define PGX_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PGX_HD inline
#endif
struct RPlan {
  uint64_t stk = 0;
  int ns = 0;                    // slots handed out
  int depth = 0, max_depth = 0;  // operands on the stack
  bool ok = true;                // every op known and given its operands so far
  // of the last step(): a leaf's slot and phase; NOT's operand slot; AND / OR's left (= result) slot and right slot rhs
  int slot = 0, phase = 0, rhs = 0;
  // Applies op i and returns how many ops that consumed: a fused leaf takes its OR / its NOT, AND with it.
  PGX_HD int step(const RProg& P, int i) {
    const int op = P.op[i];
    if (op == RP_LEAF) {
      int f = 0;
      if (stk & 8u) {
        if (i + 1 < P.nops && P.op[i + 1] == RP_OR) f = 1;
        else if (i + 2 < P.nops && P.op[i + 1] == RP_NOT && P.op[i + 2] == RP_AND) f = 2;
      }
      if (!f) {
        stk = (stk << 4) | 8u | static_cast<uint64_t>(ns);
        ++ns;
        ++depth;
        max_depth = depth > max_depth ? depth : max_depth;
      }
      slot = top();
      phase = f == 2 ? 1 : 0;
      if (f == 2) stk &= ~uint64_t(8);
      return 1 + f;
    }
    if (op == RP_NOT) {
      ok &= depth >= 1;
      slot = top();
    } else if (op == RP_AND || op == RP_OR) {
      ok &= depth >= 2;
      --depth;
      rhs = top();
      stk >>= 4;  // drop the right operand; the left one holds the result
      slot = top();
    } else {
      ok = false;
    }
    stk &= ~uint64_t(8);  // no longer pure
    return 1;
  }
  PGX_HD int top() const { return static_cast<int>(stk & 7u); }
  // after the last op: well formed (one result left), at most 16 operands deep, slot ids below 8
  PGX_HD bool fits() const { return ok && depth == 1 && max_depth <= 16 && ns <= 7; }
};

enum ProgOp : int8_t { OP_LEAF = 0, OP_AND = 1, OP_OR = 2, OP_STAT = 3, OP_TRUE = 4 };

// Multi-value columns (pgx_kernels.hip).  Values are the .mv.fwd raw section (value i at bits [i*B, i*B+B), MSB-first
// big-endian, like a single-value forward index over value positions); doc d owns values [start[d], start[d+1]).
// MV scan leaf (MVScanDocIdIterator + the evaluators' apply(int[]), operator/filter/predicate/*PredicateEvaluator
// .java): a doc matches when ANY value is in the matching set (EQ / IN / RANGE), or, for NEQ / NOT_IN, when NO value is
// outside it; one output bit per doc.
struct MvLeaf {
  const uint32_t* vals;
  const int32_t* start;        // num_docs + 1
  const uint32_t* bitset;      // matching dictIds (null: lo <= id <= lo + span)
  uint32_t* mask;              // out: bit (d & 31) of word d >> 5
  int32_t bits;
  int32_t num_docs;
  uint32_t lo, span;
  int32_t neg;
  int32_t pad;
};
// MV aggregation (Count/Sum/Min/Max/AvgMVAggregationFunction): every value of every selected doc of one segment.
struct MvAgg {
  const uint32_t* vals;
  const int32_t* start;
  const uint32_t* sel;         // selected docs: bit (d & 31) of word d >> 5 (written by the query kernel)
  const void* dict;            // int64 or double per dictId
  unsigned long long* out;     // [count, sum (int64 or f64 bits), ordered min, ordered max]
  int32_t bits;
  int32_t num_docs;
  int32_t fp;
  int32_t pad;
};

// Group-by with multi-value group columns and/or multi-value functions (DefaultGroupKeyGenerator.java:475-608
// generateKeysForDocId*, DefaultGroupByExecutor.java:154-196 aggregateGroupByMV): per selected doc, one group key per
// combination of its group columns' values; every key receives the doc's contribution of every function.
struct MvGCol {                // one group-by or aggregated column of one segment
  const uint32_t* vals;        // single-value forward index, or the multi-value values section
  const int32_t* start;        // multi-value: doc starts (num_docs + 1); null for single-value
  const int32_t* remap;        // group column: segment dictId -> global id (null: identity)
  const void* dict;            // aggregated column: int64 / double per dictId
  int32_t bits;
  int32_t pad;
};
struct MvGroupSeg {
  const uint32_t* sel;         // selected docs (query kernel selection bits, bit d & 31 of word d >> 5)
  int32_t num_docs;
  int32_t pad;
  MvGCol g[kMaxGroupCols];
  MvGCol a[kMaxAggs];
};
enum MvFnKind : int8_t { MVF_COUNT = 0, MVF_SUM = 1, MVF_MIN = 2, MVF_MAX = 3, MVF_AVG = 4, MVF_COUNTMV = 5,
                         MVF_SUMMV = 6, MVF_MINMV = 7, MVF_MAXMV = 8, MVF_AVGMV = 9 };
struct MvGroupArgs {
  const MvGroupSeg* segs;
  int32_t nsegs;
  int32_t ngcols, naggs;
  int32_t group_mode;          // G_DENSE_GLOBAL, G_HASH64 or G_HASH128
  int8_t fn[kMaxAggs];         // MvFnKind
  int8_t fp[kMaxAggs];         // FLOAT / DOUBLE values
  int8_t cnt_plane[kMaxAggs];  // AVGMV: the plane of its value count (else -1)
  uint64_t gmul[kMaxGroupCols];
  int32_t gshift[kMaxGroupCols];
  int32_t ghi[kMaxGroupCols];
  uint64_t slots;              // dense slots or hash capacity (power of two)
  unsigned long long* table;   // planes x slots
  unsigned long long* keys;    // hash keys (64-bit, or lo / hi pairs)
  unsigned int* key_state;     // hash128 slot states
  unsigned long long* overflow;
  unsigned long long* ord;     // MINMV / MAXMV per-segment holders: [seg][agg][slot] (ordered encodings)
};

// Selection with ORDER BY (pgx_select.hip; MSelectionOrderByOperator / SelectionOperatorService): one item per segment.
// A row's order key is its order columns' dictIds (card - 1 - id for DESC), kbits each, concatenated most-significant
// first into one u64; rows are ranked by (key, docId) ascending.
constexpr int kSelMaxOrderCols = 8;
constexpr int kSelBlock = 256;
struct SelCol {
  const uint32_t* fwd;         // packed big-endian fixed-bit forward index
  int32_t bits;                // bits per stored dictId
  int32_t kbits;               // bits the column takes in the key: max(1, ceil(log2 card))
  uint32_t card;
  int32_t desc;
};
struct SelItem {
  const uint32_t* sel;         // selected docs: bit (d & 31) of word d >> 5 (written by the query kernel)
  int32_t num_docs;
  int32_t ncols;
  SelCol c[kSelMaxOrderCols];
};
struct SelGatherCol {          // one schema column of one item (pgx_select_gather)
  const uint32_t* fwd;
  int32_t bits;
  int32_t pad;
};
struct SelMvCol {              // one multi-value schema column of one item (pgx_select_mv_*): pair (column m, item i)
  const uint32_t* values;      // at [m * nitems + i].  The fixed-bit value stream, padded past its last value
  const int32_t* start;        // doc d owns values [start[d], start[d + 1]); num_docs + 1 entries
  int32_t bits;
  int32_t pad;
};

// DISTINCTCOUNTHLL (pgx_hll.hip; DistinctCountHLLAggregationFunction over stream-lib's HyperLogLog(log2m = 8)): one
// item per (segment, function).  codes[dictId] = register << 8 | rank of offer((int) hashCode(value)); the registers
// are u32 and only ever maxed into, so items that share `out` combine.
constexpr int kHllRegs = 256;
constexpr int kHllBlock = 256;
constexpr int kHllMaxGroupSlots = 65536;  // pgx.h PGX_HLL_MAX_GROUP_SLOTS
struct HllItem {
  const uint32_t* sel;         // selected docs: bit (d & 31) of word d >> 5 (written by the query kernel)
  const uint32_t* fwd;         // packed big-endian fixed-bit forward index, padded to whole tiles
  const uint16_t* codes;       // ncodes entries
  uint32_t* out;               // 256 registers; the group kernel: slots x 256
  int32_t bits;
  int32_t num_docs;
  int32_t ncodes;              // dictIds at or past it are never looked up
  int32_t pad;
};
struct HllGCol {               // one group column of one segment
  const uint32_t* fwd;
  const int32_t* remap;        // segment dictId -> global id (null: identity)
  int32_t bits;
  int32_t pad;
};
struct HllGroupItem {
  HllItem h;
  HllGCol g[kMaxGroupCols];
};
static_assert(sizeof(HllItem) == 48 && sizeof(HllGroupItem) == 48 + kMaxGroupCols * 24, "tests/hll_ref.py mirrors these");
// DISTINCTCOUNTHLLMV: the item's column is multi-value.  h.fwd is the value stream (`total` rows of h.bits bits,
// padded as a forward index of `total` rows), h.sel and h.num_docs count docs, and doc d owns the value rows
// start[d] .. start[d + 1] - 1.  The group columns of the group form are single-value (one row per doc).
struct HllMvItem {
  HllItem h;
  const int32_t* start;        // num_docs + 1 ascending entries; entries past index num_docs are never read
  int32_t total;               // value rows of the stream: rows at or past it are never read, whatever start[] holds
  int32_t pad;
};
struct HllMvGroupItem {
  HllGroupItem g;
  const int32_t* start;
  int32_t total;
  int32_t pad;
};
static_assert(sizeof(HllMvItem) == 64 && sizeof(HllMvGroupItem) == sizeof(HllGroupItem) + 16,
              "tests/hll_mv_ref.py mirrors these");
struct HllGroupKey {           // passed by value: slot = sum over the group columns of global id x gmul
  uint64_t gmul[kMaxGroupCols];
  uint64_t slots;
  int32_t ngcols;
  int32_t pad;
};
// The sparse counterpart (PGX_X_SPARSE_GROUP_SETS): the tables hold one row per group of the result, and a row's group
// is looked up in a directory -- an open-addressing table (pgx_insert / pgx_find, pgx_device.h) from the row's packed
// key to the group's index, built by pgx_sel_dir_build from the result's keys.  The key is the directory's own: field g
// is group column g's global id in bits[g] = ceil(log2(global cardinality)) bits (at least 1), the fields packed one
// after the other from bit 0 of a 128-bit word (field g starts at bit 64 * word[g] + shift[g]; one that straddles bit
// 64 continues in word 1).  W: key words per table slot, 1 (keys of up to 64 bits, none of them ~0: that is the empty
// slot) or 2.
constexpr int kSelMaxSparseGroups = 131072;  // pgx.h PGX_SET_MAX_SPARSE_GROUPS; every index is below kHllNoSlot
struct SelSparseKey {          // passed by value
  const unsigned long long* keys;   // cap x W words
  const unsigned int* state;        // cap (W == 2; not read when W == 1)
  const uint32_t* index;            // cap: the group of the key in that slot
  unsigned long long* miss;         // rows whose key the directory does not hold
  uint64_t cap;                     // a power of two, >= groups
  uint8_t shift[kMaxGroupCols];
  uint8_t word[kMaxGroupCols];
  uint8_t bits[kMaxGroupCols];
  uint32_t groups;                  // 1 .. kSelMaxSparseGroups
  int32_t W;
  int32_t ngcols;
  int32_t pad;
};
static_assert(sizeof(SelSparseKey) == 40 + 3 * kMaxGroupCols + 16, "tests/sel_dir_ref.py mirrors this");

// DISTINCTCOUNT / DISTINCTCOUNTMV (pgx_distinct.hip; DistinctCountAggregationFunction): one item per (segment,
// function), laid out like the HLL items.  The state is one presence bit per dictId, (card + 31) / 32 u32 words per
// dictionary (under GROUP BY one such row per slot); bits are only ever ORed in, so items that share `out` combine.
constexpr int kDistinctLdsWords = 8192;  // bitmaps of up to 32 KiB (card <= 262,144) are marked in LDS
struct DistinctItem {
  const uint32_t* sel;         // selected docs: bit (d & 31) of word d >> 5 (written by the query kernel)
  const uint32_t* fwd;         // packed big-endian fixed-bit forward index, padded to whole tiles
  uint32_t* out;               // (card + 31) / 32 words; the group kernels: slots rows of that many words
  int32_t bits;
  int32_t num_docs;
  int32_t card;                // dictIds at or past it mark nothing; bits at or past it are never set
  int32_t pad;
};
struct DistinctGroupItem {
  DistinctItem d;
  HllGCol g[kMaxGroupCols];
};
struct DistinctMvItem {        // d.fwd is the value stream, doc i owns the value rows start[i] .. start[i + 1] - 1
  DistinctItem d;
  const int32_t* start;        // num_docs + 1 ascending entries; entries past index num_docs are never read
  int32_t total;               // value rows of the stream: rows at or past it are never read, whatever start[] holds
  int32_t pad;
};
struct DistinctMvGroupItem {
  DistinctGroupItem g;
  const int32_t* start;
  int32_t total;
  int32_t pad;
};
static_assert(sizeof(DistinctItem) == 40 && sizeof(DistinctGroupItem) == 40 + kMaxGroupCols * 24 &&
                  sizeof(DistinctMvItem) == 56 && sizeof(DistinctMvGroupItem) == sizeof(DistinctGroupItem) + 16,
              "tests/distinct_ref.py mirrors these");

// PERCENTILE / PERCENTILEMV value histograms (pgx_percentile.hip; PercentileAggregationFunction): one item per
// (segment, function), laid out like the DISTINCTCOUNT items.  The state is one u64 counter per dictId, `card` of them
// per dictionary (under GROUP BY one such row per slot); counters are only ever added to, so items that share `out`
// combine.
constexpr int kPercentileLdsCounters = 8192;  // tables of up to 32 KiB of u32 (slots x card) are counted in LDS
struct PercentileItem {
  const uint32_t* sel;         // selected docs: bit (d & 31) of word d >> 5 (written by the query kernel)
  const uint32_t* fwd;         // packed big-endian fixed-bit forward index, padded to whole tiles
  uint64_t* out;               // card counters; the group kernels: slots rows of card counters
  int32_t bits;
  int32_t num_docs;
  int32_t card;                // dictIds at or past it count nothing
  int32_t pad;
};
struct PercentileGroupItem {
  PercentileItem d;
  HllGCol g[kMaxGroupCols];
};
struct PercentileMvItem {      // d.fwd is the value stream, doc i owns the value rows start[i] .. start[i + 1] - 1
  PercentileItem d;
  const int32_t* start;        // num_docs + 1 ascending entries; entries past index num_docs are never read
  int32_t total;               // value rows of the stream: rows at or past it are never read, whatever start[] holds
  int32_t pad;
};
struct PercentileMvGroupItem {
  PercentileGroupItem g;
  const int32_t* start;
  int32_t total;
  int32_t pad;
};
static_assert(sizeof(PercentileItem) == 40 && sizeof(PercentileGroupItem) == 40 + kMaxGroupCols * 24 &&
                  sizeof(PercentileMvItem) == 56 && sizeof(PercentileMvGroupItem) == sizeof(PercentileGroupItem) + 16,
              "tests/percentile_ref.py mirrors these");

// Statistics automaton over one segment's leaf masks (pgx_kernels.hip pgx_fsm_chunks / pgx_fsm_compose).
struct FsmSeg {
  const uint32_t* lmask;       // leaf l, row r: bit (r & 31) of word [l * words + (r >> 5)]
  int64_t words;               // words per leaf
  int32_t num_docs;
  int32_t nint;                // intervals of constant range position
  int64_t chunk0;              // first chunk of this segment in the launch
  int32_t ibeg[3 * 10 + 2];    // interval first rows (ascending, ibeg[0] = 0)
  int32_t itab[3 * 10 + 2];    // interval transition table
};

enum AggKind : int8_t { A_COUNT = 0, A_SUM = 1, A_MIN = 2, A_MAX = 3, A_AVG = 4 };

// Accumulator plane ops (pgx.h pgx_query_dense_plane_op)
enum PlaneOp : int8_t { P_ADD_I64 = 0, P_ADD_F64 = 1, P_MIN_ORD = 2, P_MAX_ORD = 3 };

enum GroupMode : int8_t { G_NONE = 0, G_DENSE_LDS = 1, G_DENSE_GLOBAL = 2, G_HASH64 = 3, G_HASH128 = 4,
                          G_EMIT = 5 /* query kernels: emit key|value records for the partitioned group-by */,
                          G_HASHW = 6 /* keys of 3-4 64-bit words (ARRAY_MAP keys over 126 bits): generic kernel */ };
constexpr int kMaxKeyWords = 4;
inline bool hash_mode(int gm) { return gm == G_HASH64 || gm == G_HASH128 || gm == G_HASHW; }

struct KLeaf {
  int32_t lo, hi;
  const uint32_t* bitset;      // device, ceil(card/32) words (LEAF_SCAN_BITSET)
  const int32_t* ranges;       // device, 2*nranges inclusive [a,b] pairs, sorted (LEAF_RANGES)
  int32_t nranges;
  int8_t mode;
  int8_t pad[3];
};

struct KSeg {
  int64_t tile_begin;          // global tile index of this segment's first tile
  int32_t num_docs;            // rows scanned: [0, num_docs)
  int32_t num_tiles;
  const uint32_t* fwd[kMaxQCols];     // packed big-endian fixed-bit forward index (padded)
  const void* dict[kMaxQCols];        // value columns: int64 (INT/LONG) or double (FLOAT/DOUBLE) per dictId
  const int32_t* remap[kMaxQCols];    // group columns: dictId -> global id (nullptr = identity)
  int8_t bits[kMaxQCols];
  KLeaf leaf[kInlineLeaves];          // leaves 0-15 (the rest: KQuery.xleaf)
  uint32_t* lmask;                    // statistics automaton input: leaf l, row r -> bit (r & 31) of
  int64_t lmask_words;                // word [l * lmask_words + (r >> 5)] (nullptr: not requested)
};

struct KQuery {
  const KSeg* segs;
  int32_t num_segs;
  int32_t num_qcols;
  int64_t total_tiles;
  // filter program (postfix, stack machine)
  int32_t prog_len;
  int8_t prog_op[kMaxProg];
  int8_t prog_arg[kMaxProg];
  int8_t leaf_col[kMaxLeaves];
  // value columns decoded for aggregation (distinct), and aggs
  int32_t num_aggs;
  int8_t agg_kind[kMaxAggs];
  int8_t agg_col[kMaxAggs];      // query-column slot (-1 for COUNT)
  int8_t agg_fp[kMaxAggs];       // value column is FLOAT/DOUBLE
  int8_t plane_op[kMaxAggs + 1]; // plane 0 = count
  int32_t num_planes;            // 1 + num_aggs
  // group-by
  int8_t group_mode;
  int32_t num_gcols;
  int8_t gcol[kMaxGroupCols];
  uint64_t gmul[kMaxGroupCols];  // dense: mixed-radix multiplier; hash: bit shift
  int32_t gshift[kMaxGroupCols];
  int32_t ghi[kMaxGroupCols];    // 128-bit / wide keys: the 64-bit word the field goes to (0 = low)
  int32_t key_words;             // hash keys: 64-bit words per key (1, 2, or up to kMaxKeyWords for G_HASHW)
  uint64_t dense_slots;          // dense key space
  uint64_t hash_cap;             // power of two
  // outputs
  unsigned long long* agg_out;   // aggregation-only: num_planes accumulators (plane encodings)
  unsigned long long* stats;     // [0] docs matched, [1] entries scanned in filter (kernel part)
  unsigned long long* table;     // dense: planes x dense_slots ; hash: planes x hash_cap
  unsigned long long* keys;      // hash: key_words * hash_cap (word w of slot s at keys[s * key_words + w])
  unsigned int* key_state;       // hash128 / wide: 0 empty, 1 busy, 2 ready
  unsigned long long* overflow;  // hash insert failures (table full) -> host retries bigger
  // leaves 16 and up: xn per segment, leaf l of segment s at xleaf[s * xn + l - kInlineLeaves] (nullptr: none)
  const KLeaf* xleaf;
  int32_t xn;
};

}  // namespace pgx

// =================================================================================================
// Query-specialised kernels (pgx_jit.cpp): the shape of one launch group, from which a kernel is generated and
// compiled by hiprtc once per distinct shape (cached per process and device).
// =================================================================================================
#include <string>
#include <vector>

namespace pgx {

// Value images staged in LDS for aggregated columns (built once per column at staging time, pgx_stage.cpp).
enum ImgKind : int8_t {
  IMG_NONE = 0,   // no image: values are gathered from the HBM value table (int64 / double per dictId)
  IMG_U32 = 1,    // u32 (value - vbase) per dictId
  IMG_FOR16 = 2,  // 64 x u32 block bases (relative to vbase) then u16 offset per dictId; block = 1 << sh dictIds
  IMG_F64 = 3,    // double per dictId
};
constexpr int kImgFor16Blocks = 64;
constexpr int kLdsBudget = 160 * 1024 - 256;  // static LDS of one workgroup, minus the per-plane accumulators

// Narrow partitioned group-by (pgx_part.cpp run_narrow): the packed K-bit group key is mixed by a bijection of
// [0, 2^K), h = ((key * c1) & M) ^ (that >> s) with s = ceil(K / 2) (so the xor-shift inverts itself), and the
// partitions are h's top bits (the multiply carries every key bit into them); the xor-shift folds those well-mixed top
// bits into the low bits that choose a record's slot in the aggregation tables.  h's remaining bits travel in the
// records and the aggregation rebuilds the key with the inverse.  c1 has 32 bits: the scan's multiply of a key of up
// to 64 bits is three 32-bit multiplies (round 4 used two full 64-bit multiplies, eight, for the same partitions).
// Shared by the generated scan (pgx_jit.cpp), the split / aggregation kernels and the host.
constexpr uint64_t kNarrowC1 = 0x9E3779B1ull;
constexpr int kNarrow1Bits = 8;      // first split (inside the scan): 256 buckets
constexpr int kNarrowRing = 64;      // scan: per-bucket LDS ring of records (two 32-record units; the largest ring)
constexpr int kNarrowMaxBits2 = 10;  // second split (pgx_narrow_split): up to 1024 sub-buckets per bucket
// Environment knobs (A/B switches and test hooks), read ONCE per query by pgx_query_compile and kept with the query:
// planning and execution read them from there, never from the environment (no per-query walk of environ, no race
// with a setenv on another thread).  The whole set:
//   PGX_JIT=0          the generic interpreter kernel instead of the generated (hiprtc) kernels, everywhere (A/B)
//   PGX_PART_NARROW=0  sparse group-by through the 8-byte radix path instead of the narrow records; =direct: narrow
//                      records carry value offsets wherever they fit (default: dictIds + LDS image when there is one);
//                      =gather: integer records carry the dictId's index in a global value table (IMG 5, tests)
//   PGX_RCHUNK=0|1     bitmap programs evaluated by the separate pass / inside the query kernels (default: planner;
//                      programs whose chunk masks do not fit the kernels' LDS budget take the separate pass either way)
//   PGX_RPROG=off|wave|seg|chunk|stack   bitmap-program kernel (off: no program fusion; default: planner)
//   PGX_BATCH_SEGS=N   segments per batch of a long segment list on its first execution (0: one launch)
//   PGX_DEBUG=opt,...  part_small (radix buckets start undersized), narrow_k2=N (coarser narrow partitions),
//                      narrow_log (which sparse path ran, hash-table regrowth; on stderr), host_profile (planning phases
//                      on stderr); A/B switches measured slower and kept off: nunit=16 (16-record narrow
//                      scan units), pf2 (narrow scans load two tiles ahead), noimg (no LDS value images in the query
//                      kernels), head=N (a lone replay's first part is 1/N of the segments); A/B switches of the sparse
//                      tile body: densebody (doc-mask filters run the dense row loop), sparsek=N (a wave
//                      walks set bits while no lane holds more than N selected rows of a sub-step; default kSparseK);
//                      of the selection without ORDER BY: firstg=N (N workgroups per segment in
//                      pgx_select_first, 1 .. 64; default: one).
//                      Two more are read by pgx_launch_roaring_program_wave itself at every launch, because the tests
//                      call that launcher without a context: rnarrow (the wave kernel's two-byte container
//                      reader instead of the wide one), rparts=N (N waves per segment)
// and, outside the query: PGX_PLAN_CACHE=0 (process-wide), PGX_JIT_CACHE=<dir> / PGX_JIT_DUMP=<dir> (the compiler).
enum RProgKind { RPROG_AUTO = -1, RPROG_OFF = 0, RPROG_WAVE = 1, RPROG_SEG = 2, RPROG_CHUNK = 3, RPROG_STACK = 4 };
struct Knobs {
  bool jit = true;
  bool narrow = true;
  bool narrow_direct = false;  // PGX_PART_NARROW=direct
  bool narrow_gather = false;  // PGX_PART_NARROW=gather (tests): value-table records (IMG 5) where they fit
  int rchunk = -1;          // -1: planner's choice
  int rprog = RPROG_AUTO;
  int batch_segs = -1;      // -1: default (512; 0 with PGX_X_THROUGHPUT)
  bool no_img = false;      // PGX_DEBUG noimg: query kernels gather values from the dictionaries, no LDS images (A/B)
  bool prefetch2 = false;   // PGX_DEBUG pf2: narrow scans load two tiles ahead (A/B)
  int narrow_unit = 32;     // PGX_DEBUG nunit=16: 16-record units (32-record rings: two scan workgroups per CU)
  int lone_head = 2;        // PGX_DEBUG head=N: a lone replay's first part is 1/N of the segments (A/B)
  bool part_small = false;  // PGX_DEBUG part_small
  int narrow_k2 = -1;       // PGX_DEBUG narrow_k2=N
  bool narrow_log = false;  // PGX_DEBUG narrow_log
  bool dense_body = false;  // PGX_DEBUG densebody: doc-mask filters run the dense row loop, no sparse tile body (A/B)
  int sparse_k = -1;        // PGX_DEBUG sparsek=N: the sparse body's per-lane row limit (-1: kSparseK) (A/B)
  int sel_first_g = 0;      // PGX_DEBUG firstg=N: workgroups per segment of pgx_select_first (0: run_select's choice)
  bool host_profile = false;
};
Knobs read_knobs();

struct NarrowMix {
  uint64_t mask = 0, c1 = kNarrowC1, ic1 = 0;
  int s = 0;
};
inline uint64_t narrow_inverse(uint64_t c) {  // c odd: c * inverse == 1 (mod 2^64), Newton iteration
  uint64_t x = c;
  for (int i = 0; i < 6; ++i) x *= 2 - c * x;
  return x;
}
inline NarrowMix narrow_mix(int keybits) {
  NarrowMix m;
  m.mask = keybits >= 64 ? ~0ull : (uint64_t(1) << keybits) - 1u;
  m.s = (keybits + 1) / 2;
  m.ic1 = narrow_inverse(m.c1);
  return m;
}

// Sparse tile body of the query kernels: most selected rows one lane may hold in a sub-step for the wave to walk set
// bits instead of running the dense row loop (exported as pgx_sparse_k for the tests; PGX_DEBUG sparsek=N overrides)
constexpr int kSparseK = 4;

struct JitCol {
  int bits = 0;
  bool decode = false;   // read by a scan leaf, an aggregation or a group key
  int img = IMG_NONE;    // value image kind (aggregated columns)
  int img_sh = 0;        // IMG_FOR16 block shift
  int img_words = 0;     // LDS dwords reserved for the image (max over the group's segments)
  bool acc32 = false;    // R rows of (value - vbase) always fit a u32 partial sum
  bool fp = false;       // FLOAT/DOUBLE values
  bool remap = false;    // group column with a local->global dictId remap table
  bool frac = false;     // R * bits is not a multiple of 32: a lane's rows start mid-dword (dword-aligned load of
                         // the covering words, then a funnel shift by (first row * bits) % 32)
};

struct JitShape {
  int T = 256;           // threads per workgroup
  int R = 8;             // rows per lane per sub-step (R * bits % 32 == 0 for every decoded column without frac)
  int TL = 32;           // rows per lane per tile (a multiple of R): the rows whose raw words are loaded one tile ahead
  std::vector<JitCol> cols;
  std::vector<int> leaf_col, leaf_mode;   // leaf_col -1: doc-range leaf with no column (star-tree node ranges)
  std::vector<int> prog_op, prog_arg;
  std::vector<int> agg_kind, agg_col, plane_op;
  int group_mode = G_NONE;
  std::vector<int> gcol;
  std::vector<uint64_t> gmul;
  uint64_t dense_slots = 0;
  int num_planes = 1;
  // G_EMIT: record = key (group ids at gshift) | value offset << keybits; emit_col = value column (-1: none)
  std::vector<int> gshift;
  int keybits = 0;
  int emit_col = -1;
  // G_HASH64 / G_HASH128: group ids at gshift of the low (ghi 0) or high (ghi 1) key word; hash_slots LDS slots
  std::vector<int> ghi;
  int hash_slots = 0;
  bool leafmask = false;  // write every leaf's per-row predicate bit (statistics automaton input, pgx_stats.cpp)
  // LEAF_RCHUNK leaves, in leaf order: the bitmap program's postfix ops (RP_*), identical for the group's segments
  std::vector<std::vector<int>> rprog_ops;
  // G_EMIT: records split 2^part_bits ways inside the kernel (first radix pass fused; 0 = row-order records), and the
  // record's value field is the value column's dictId (sorted dictionary) instead of its offset from vbase
  int part_bits = 0;
  bool emit_dictid = false;
  // with part_bits: each workgroup appends to its own region ("slab") per bucket through LDS cursors, no staging and no
  // global cursor per sub-step (slab (b, w) at table + (b * part_nwg + part_wg_base + w) * part_cap)
  bool part_slab = false;
  // dense LDS group-by of COUNT + one integer SUM / AVG with a value image: both planes in ONE 64-bit LDS add, the
  // row count above bit dense_pack (the value offset below), flushed per segment (0: two adds per row)
  int dense_pack = 0;
  bool compact = false;   // pack each sub-step's selected rows into consecutive lanes before aggregating (selective)
  bool selmask = false;   // write every row's selection bit (multi-value aggregations read it)
  // with part_slab: narrow records (run_narrow).  The key is mixed (NarrowMix), its top part_bits choose the bucket and
  // the record is the rest of the mix | value dictId << (keybits - part_bits), narrow_vbits wide; it leaves as a u32
  // (the record's low half) plus, when it is wider than 32 bits, a u16 (bits 32..47) in a second array
  bool part_narrow = false;
  int narrow_vbits = 0;
  int narrow_unit = 32;   // records per unit that leaves the scan's rings (ring: two units per bucket)
  bool prefetch2 = false; // raw words of tiles tt+1 AND tt+2 in flight (no gate leaf): twice the bytes in flight
  // Filters made of doc-mask leaves only (aggregation-only and dense group-by kernels): a sub-step decodes and
  // aggregates only the rows whose selection bit is set, unless some lane of the wave holds more than sparse_k of them
  // (then the wave runs the dense row loop for that sub-step).  dense_body: the dense row loop always (A/B, tests)
  bool dense_body = false;
  int sparse_k = kSparseK;
};

// ----- numEntriesScannedInFilter automaton (pgx_stats.cpp builds it, pgx_kernels.hip pgx_fsm_* runs it) -----
constexpr int kFsmMaxLeaves = 10;                // transition tables are indexed by every leaf's membership bit
constexpr int kFsmMaxStates = 4096;
constexpr uint64_t kFsmMaxTable = 1ull << 22;    // u32 entries over all tables
constexpr int kFsmChunkRows = 1024;              // rows one thread runs from every start state
constexpr int kFsmMaxIntervals = 3 * kFsmMaxLeaves + 2;

struct FsmTreeNode {             // the physical filter tree after FilterPlanNode.reorder
  int op = 0;                    // 0 leaf, 1 AND, 2 OR
  int leaf = -1;
  int phys = 3;                  // leaf: 0 sorted, 2 bitmap, 3 scan
  std::vector<FsmTreeNode> kids;
};
struct FsmSegInfo {
  int32_t num_docs = 0;
  std::vector<int64_t> sorted_first, sorted_last;  // per leaf: first / last doc of a sorted leaf's ranges (0, 0 empty)
  uint32_t always_false = 0;                       // scan leaves whose predicate evaluator is alwaysFalse
};
struct FsmPlan {
  int num_states = 0, num_leaves = 0, num_tables = 0;
  std::vector<uint32_t> table;   // [(t * S + q) << L | input] = next_state << 16 | entries counted
  std::vector<std::vector<std::pair<int32_t, int32_t>>> seg_intervals;  // per segment: (first row, table)
};
bool fsm_build(const FsmTreeNode& tree, int num_leaves, const std::vector<FsmSegInfo>& segs, FsmPlan& out,
               std::string* err);

std::string jit_source(const JitShape& s, int* lds_bytes);
// Compile (or fetch from the cache) the kernel for shape s on the current device.  Returns the hipFunction_t as void*.
void* jit_function(const JitShape& s, int device, int* lds_bytes, std::string* err);

}  // namespace pgx
