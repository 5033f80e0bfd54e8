// libpgx: DISTINCTCOUNTHLL -- the per-dictId tables (HLL codes, DISTINCTCOUNT hash codes: dict_table), the runner and
// the register accessor.  The runner's items for the offer kernels and pgx_distinct.cpp's for the mark kernels are both
// built, uploaded and launched by SelItems (pgx_host.h) over one SelScan.
// DistinctCountHLLAggregationFunction (operator/aggregation/function/DistinctCountHLLAggregationFunction.java:51-92)
// offers (int) hashCode of every selected doc's value to a stream-lib HyperLogLog(log2m = 8); the executor hands it
// DataFetcher.getSVHashCodeArray (common/DataFetcher.java:242-248: dictionary.get(dictId).hashCode()).  The kernels
// are in pgx_hll.hip.  Reference paths are relative to pinot-core/src/main/java/com/linkedin/pinot/core/.
#include "pgx_hash.h"
#include "pgx_host.h"
#include "pgx_sel_key.h"

namespace pgxh {

static_assert(kSelKeyMaxCols == pgx::kMaxGroupCols, "pgx_sel_key.h lays out one field per group column");

// MurmurHash.hashLong (stream-lib 2.7.0: MurmurHash2 over the low, then the high half), in Java int arithmetic.
static uint32_t murmur_hash_long(int64_t v) {
  const uint32_t m = 0x5BD1E995u;
  uint32_t k = uint32_t(uint64_t(v)) * m;
  k ^= k >> 24;
  uint32_t h = k * m;
  k = uint32_t(uint64_t(v) >> 32) * m;
  k ^= k >> 24;
  h *= m;
  h ^= k * m;
  h ^= h >> 13;
  h *= m;
  h ^= h >> 15;
  return h;
}

// HyperLogLog.offer(Integer) -> offerHashed: register x >>> 24, rank nlz((x << 8) | 0x81) + 1 (1..25).
static uint16_t hll_code(int32_t hash_code) {
  const uint32_t x = murmur_hash_long(int64_t(hash_code));
  const uint32_t w = (x << 8) | 0x81u;
  return uint16_t(((x >> 24) << 8) | uint32_t(__builtin_clz(w) + 1));
}

static int32_t dict_hash_code(const StagedColumn& c, int i) {
  switch (c.data_type) {
    case PGX_INT: return int32_t(c.ivals[size_t(i)]);
    case PGX_LONG: return hash_long(c.ivals[size_t(i)]);
    case PGX_FLOAT: return hash_float(float(c.dvals[size_t(i)]));
    case PGX_DOUBLE: return hash_double(c.dvals[size_t(i)]);
    default: return hash_utf8(reinterpret_cast<const uint8_t*>(c.svals[size_t(i)].data()), c.svals[size_t(i)].size());
  }
}

// A table with one entry per dictId in HBM (entry i: of(the hash code of value i)), built on the first query that
// needs it.  Numeric dictionaries share it through their SharedDict (keyed by type and content); a STRING column keeps
// its own: buf is the one or the other.  Both belong to one staged dictionary: a realtime snapshot stages its (grown)
// dictionaries afresh and so never sees an earlier table.
template <class T, class F>
static const T* dict_table(pgx_ctx* ctx, const StagedColumn& c, DevBuf& buf, const char* what, F of) {
  std::lock_guard<std::mutex> g(ctx->dict_mu);
  if (buf.p) return buf.as<T>();
  std::vector<T> t(size_t(std::max(c.card, 1)), 0);
  for (int i = 0; i < c.card; ++i) t[size_t(i)] = of(dict_hash_code(c, i));
  DevBuf b(ctx, t.size() * sizeof(T));
  hip_check(hipMemcpy(b.p, t.data(), t.size() * sizeof(T), hipMemcpyHostToDevice), what);
  buf = std::move(b);
  return buf.as<T>();
}

static const uint16_t* hll_code_table(pgx_ctx* ctx, const StagedColumn& c) {
  return dict_table<uint16_t>(ctx, c, c.shared ? c.shared->hll_codes : c.hll_codes, "HLL codes H2D", hll_code);
}

// DISTINCTCOUNT: the i32 hash code per dictId, kept beside the HLL codes.
const int32_t* distinct_hash_table(pgx_ctx* ctx, const StagedColumn& c) {
  return dict_table<int32_t>(ctx, c, c.shared ? c.shared->dist_hash : c.dist_hash, "DISTINCTCOUNT hash codes H2D",
                             [](int32_t h) { return h; });
}

// workgroups per item: at least 4 steps of 256 mask words each, and no more over all items than stay resident
static int hll_wgs(const pgx_ctx* ctx, int max_words, size_t nitems) {
  int G = std::max(1, (max_words + 4 * kHllBlock - 1) / (4 * kHllBlock));
  G = std::min(G, std::max(1, int(size_t(8 * ctx->num_cus) / std::max<size_t>(1, nitems))));
  return std::min(G, 64);
}

// The group columns of every segment, once for all the scan's items: forward index, width and, where the segment's
// dictionary is not the global one, its remap table (a table that segments share is uploaded once).
static void sel_group_columns(pgx_ctx* ctx, SelScan& S) {
  std::vector<int32_t> blob;
  std::map<const std::vector<int32_t>*, size_t> roff;
  for (int g = 0; g < S.ng; ++g)
    if (!S.P->gdicts[size_t(g)].identity)
      for (int s = 0; s < S.n; ++s) {
        const std::vector<int32_t>* rm = S.P->gdicts[size_t(g)].remap[size_t(s)].get();
        if (rm && !roff.count(rm)) {
          roff[rm] = blob.size();
          blob.insert(blob.end(), rm->begin(), rm->end());
        }
      }
  S.remaps = DevBuf(ctx, std::max<size_t>(1, blob.size()) * 4);
  if (!blob.empty())
    hip_check(hipMemcpyAsync(S.remaps.p, blob.data(), blob.size() * 4, hipMemcpyHostToDevice, S.st), "remap H2D");
  S.gcols.assign(S.ng > 0 ? size_t(S.n) : 0, SelGCols{});
  for (size_t s = 0; s < S.gcols.size(); ++s)
    for (int g = 0; g < S.ng; ++g) {
      const StagedColumn& gc = S.segs[s]->col(S.q->group_cols[size_t(g)]);
      HllGCol& c = S.gcols[s].g[g];
      c.fwd = gc.fwd;  // (a column without one: refused when the first item is built)
      c.bits = gc.bits;
      const GlobalDict& gd = S.P->gdicts[size_t(g)];
      if (!gd.identity && gd.remap[s]) c.remap = S.remaps.as<int32_t>() + roff[gd.remap[s].get()];
    }
}

// group i's global id in group column g, from the result's key (a segment and its dictId)
static int64_t group_global_id(const GlobalDict& gd, int n, int32_t seg, int32_t id) {
  if (seg < 0 || seg >= n) fail(PGX_ERR_INTERNAL, "group key without a segment");
  const std::vector<int32_t>* rm = gd.identity ? nullptr : gd.remap[size_t(seg)].get();
  return rm ? (*rm)[size_t(id)] : id;
}

// The directory of a sparse run: the result's groups' packed keys in an open-addressing table of at least twice as many
// slots (pgx_sel_dir_build), and the key the sparse group launches take.
struct SelDirectory {
  DevBuf keys, tkey, tstate, tidx, miss;
  std::vector<unsigned long long> host;  // the packed keys, W words each (alive until the stream was waited for)
  pgx::SelSparseKey key{};
};

// A query with DISTINCTCOUNTHLL / DISTINCTCOUNTHLLMV functions: the rest of it (its filter, its standard functions or
// COUNT(*) alone, its GROUP BY) runs through the query kernels, which also write every scanned row's selection bit;
// pgx_hll_offer[_group] then offers every selected row's code, pgx_hll_offer_mv[_group] the code of every value of
// every selected doc of a multi-value column (DistinctCountHLLMVAggregationFunction.java).  DISTINCTCOUNT and
// DISTINCTCOUNTMV functions (codes 12, 13) ride the same scan: pgx_distinct.cpp marks their presence bits on the same
// stream and collects the result's sets afterwards; PERCENTILE and PERCENTILEMV (codes 15, 14) are the third family:
// pgx_percentile.cpp counts the selected values per dictId and collects the groups' (value, count) pairs.  FASTHLL
// (code 16) is the fourth: presence bitmaps of its own, marked as DISTINCTCOUNT's, whose rows pgx_fasthll.cpp folds
// through the dictionaries' register images into register blocks that follow the HLL columns' in the result.  Planned
// afresh every time (no plan cache).
// With PGX_X_SPARSE_GROUP_SETS a GROUP BY whose key space is not dense or has more than PGX_HLL_MAX_GROUP_SLOTS slots
// takes the sparse route: the scan runs first (through the global hash table, never the partitioned record path: the
// selection bits must be those of one complete scan by kernels known to write them), the result's groups go into a
// directory (SelDirectory), and the three families' tables get one row per group, in the result's order.
void run_hll(pgx_ctx* ctx, const pgx_query& q, pgx_segment* const* segs, int n, const pgx_leaf_binding* bindings,
             const pgx_exec_opts* opts, pgx_result* R, hipStream_t st, const Domain* dom) {
  const uint32_t xflags = opts ? opts->flags : 0;
  if (dom) fail(PGX_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL across devices");
  if (opts && (opts->dense_out || (xflags & PGX_X_KEEP_DENSE_ON_DEVICE)))
    fail(PGX_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL into a caller's dense table");
  if (!q.kn.jit) fail(PGX_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL needs the query kernels");
  for (const auto& d : q.key_domain)
    if (d.set) fail(PGX_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL with a key domain");
  if (n < 1) fail(PGX_ERR_INVALID_ARG, "no segments");
  const int na = int(q.agg_fn.size()), ng = int(q.group_cols.size());
  pgx_query qs = q;
  qs.flags |= PGX_Q_NO_STAR_TREE;  // every raw row gets its selection bit
  qs.agg_fn.clear();
  qs.agg_col.clear();
  std::vector<int> sv_pos(size_t(na), -1), hll_pos(size_t(na), -1), dist_pos(size_t(na), -1), pct_pos(size_t(na), -1);
  std::vector<std::string> hcols;  // a column is single-value or multi-value, so the name identifies the block
  std::vector<char> hmv;           // per HLL column: multi-value (DISTINCTCOUNTHLLMV)
  DistinctRun D;                   // DISTINCTCOUNT / DISTINCTCOUNTMV: their columns, bitmaps and items (pgx_distinct.cpp)
  PercentileRun Q;                 // PERCENTILE / PERCENTILEMV: their columns, counter tables and items (pgx_percentile.cpp)
  DistinctRun F;                   // FASTHLL: bitmaps as DISTINCTCOUNT's, no hash tables (pgx_fasthll.cpp)
  F.hashes = false;
  F.fn = "FASTHLL";
  std::vector<int> fast_pos(size_t(na), -1);
  for (int a = 0; a < na; ++a) {
    const int f = q.agg_fn[size_t(a)];
    if (f == PGX_FASTHLL) {  // (its columns are checked with their dictionaries: fasthll_images)
      const std::string& c = q.agg_col[size_t(a)];
      auto it = std::find(F.cols.begin(), F.cols.end(), c);
      fast_pos[size_t(a)] = int(it - F.cols.begin());
      if (it == F.cols.end()) {
        F.cols.push_back(c);
        F.mv.push_back(0);
      }
    } else if (f >= PGX_DISTINCTCOUNTHLL && f <= PGX_PERCENTILE) {
      const std::string& c = q.agg_col[size_t(a)];
      const bool mv = f == PGX_DISTINCTCOUNTHLLMV || f == PGX_DISTINCTCOUNTMV || f == PGX_PERCENTILEMV;
      const bool exact = f == PGX_DISTINCTCOUNT || f == PGX_DISTINCTCOUNTMV;
      const bool pct = f == PGX_PERCENTILE || f == PGX_PERCENTILEMV;
      for (int s = 0; s < n; ++s) {
        const bool is_mv = segs[s]->col(c).is_mv;
        if (!mv && is_mv)
          fail(PGX_ERR_UNSUPPORTED,
               std::string(pct ? "PERCENTILE" : exact ? "DISTINCTCOUNT" : "DISTINCTCOUNTHLL") + " on multi-value column " + c);
        if (mv && !is_mv) fail(PGX_ERR_UNSUPPORTED, "multi-value function on single-value column " + c);
      }
      std::vector<std::string>& cols = pct ? Q.cols : exact ? D.cols : hcols;
      auto it = std::find(cols.begin(), cols.end(), c);
      (pct ? pct_pos : exact ? dist_pos : hll_pos)[size_t(a)] = int(it - cols.begin());
      if (it == cols.end()) {
        cols.push_back(c);
        (pct ? Q.mv : exact ? D.mv : hmv).push_back(mv);
      }
    } else {
      if (f < PGX_COUNT || f > PGX_AVGMV) fail(PGX_ERR_UNSUPPORTED, "aggregation function not on the GPU path");
      if (is_standard_mv_fn(f))
        fail(PGX_ERR_UNSUPPORTED, "standard multi-value functions together with DISTINCTCOUNTHLL");
      sv_pos[size_t(a)] = int(qs.agg_fn.size());
      qs.agg_fn.push_back(f);
      qs.agg_col.push_back(q.agg_col[size_t(a)]);
    }
  }
  for (const auto& g : q.group_cols)
    for (int s = 0; s < n; ++s)
      if (segs[s]->col(g).is_mv) fail(PGX_ERR_UNSUPPORTED, "multi-value group column together with DISTINCTCOUNTHLL");
  if (qs.agg_fn.empty()) {
    qs.agg_fn.push_back(PGX_COUNT);
    qs.agg_col.push_back("");
  }
  const size_t nh = hcols.size(), nf = F.cols.size();
  for (int a = 0; a < na; ++a)  // FASTHLL's register blocks follow the HLL columns'
    if (fast_pos[size_t(a)] >= 0) hll_pos[size_t(a)] = int(nh) + fast_pos[size_t(a)];
  std::vector<std::vector<const uint32_t*>> fimg;
  fasthll_images(ctx, segs, n, F, fimg);  // (refuses the columns and the images' bytes before anything runs)

  // 1. the rest of the query, with selection bits
  const bool may_sparse = ng > 0 && (xflags & PGX_X_SPARSE_GROUP_SETS) != 0;
  ExecPlan P;
  P.want_selmask = true;
  plan_query(ctx, qs, segs, n, bindings, may_sparse ? xflags | PGX_X_NO_PARTITION : xflags, P);
  const KQuery& K = P.kq;
  const bool dense = K.group_mode == G_DENSE_LDS || K.group_mode == G_DENSE_GLOBAL;
  const bool sparse = ng > 0 && (!dense || P.use_part || P.dense_slots > uint64_t(PGX_HLL_MAX_GROUP_SLOTS));
  if (sparse && (!may_sparse || P.use_part))
    fail(PGX_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL under GROUP BY: dense key spaces of up to PGX_HLL_MAX_GROUP_SLOTS only");
  uint64_t slots = ng > 0 && !sparse ? P.dense_slots : 1;  // (a sparse run: the result's groups, known after the scan)
  if (!sparse) {
    distinct_plan(ctx, segs, n, slots, D);  // (refuses tables over PGX_DISTINCT_MAX_TABLE_BYTES before anything runs)
    distinct_plan(ctx, segs, n, slots, F);  // (FASTHLL's bitmaps count on their own)
    percentile_plan(ctx, segs, n, slots, Q);  // (... over PGX_PERCENTILE_MAX_TABLE_BYTES, and STRING columns)
  } else {
    for (const auto& c : Q.cols)  // (the one refusal of percentile_plan that does not depend on the groups)
      for (int s = 0; s < n; ++s)
        if (segs[s]->col(c).data_type == PGX_STRING) fail(PGX_ERR_UNSUPPORTED, "PERCENTILE on STRING column " + c);
  }
  P.sel_off.assign(size_t(n), 0);
  int64_t words = 0;
  int max_words = 0;
  for (int s = 0; s < n; ++s) {
    P.sel_off[size_t(s)] = words;
    const int w = (P.ksegs[size_t(s)].num_docs + 31) / 32 + 1;
    words += w;
    max_words = std::max(max_words, w);
  }
  P.sel_buf = DevBuf(ctx, size_t(std::max<int64_t>(words, 1)) * 4);
  hip_check(hipMemsetAsync(P.sel_buf.p, 0, size_t(std::max<int64_t>(words, 1)) * 4, st), "selection masks");
  ExecBuffers B;
  upload_plan(ctx, P, B, st);
  plan_jit(ctx, qs, segs, n, P, B);
  bool scanned = !(P.jit.empty() || !P.jit[0].fn);
  if (!scanned)  // every segment empty: nothing scanned, registers stay zero
    for (int s = 0; s < n; ++s)
      if (P.ksegs[size_t(s)].num_docs != 0) fail(PGX_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL needs the query kernels");
  const bool hash = hash_mode(K.group_mode);  // (a sparse run only)
  uint64_t hash_est = 0;
  if (hash) {  // the table's first size and its growth: run_query's
    P.hash_cap = hash_est = initial_hash_cap(segs, n, P);
    if (scanned) P.hash_cap = std::min<uint64_t>(P.hash_cap, std::max<uint64_t>(uint64_t(1) << 20, q.hash_cap_hint.load()));
  }
  for (int attempt = 0; attempt < 6; ++attempt) {
    // A pass that overflowed the hash table is run again whole.  The generated kernels write the selection words with
    // plain stores, a word per lane of every tile they visit; the words are cleared again all the same, so that the
    // bits the functions read are those of the one complete pass whatever an abandoned one left behind.
    if (attempt)
      hip_check(hipMemsetAsync(P.sel_buf.p, 0, size_t(std::max<int64_t>(words, 1)) * 4, st), "selection masks");
    alloc_outputs(ctx, P, B, nullptr, 0);
    reset_outputs(P, B, st);
    launch_scan(P, st);
    if (!hash) break;
    unsigned long long* outs = reinterpret_cast<unsigned long long*>(B.host.bytes() + B.off_outs);
    hip_check(hipMemcpyAsync(outs, B.dev() + B.off_outs, kOutsBytes, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    if (outs[24] == 0) break;
    if (attempt == 5) fail(PGX_ERR_OOM, "group-by hash table overflow");
    P.hash_cap = std::max(P.hash_cap * 4, hash_est);  // table full: grow and rerun
  }
  if (hash && P.hash_cap > q.hash_cap_hint.load()) q.hash_cap_hint.store(P.hash_cap);

  // 2. the offers, on the same stream: one item per (HLL column, segment).  A sparse run needs the result's groups
  // first: finish_result waits for the stream and yields every group (a trim is a call of its own, on the result).
  pgx_result Rs;
  SelDirectory dir;
  bool offer = true;
  if (sparse) {
    finish_result(ctx, qs, P, B, segs, n, st, &Rs, nullptr);
    if (Rs.lazy) fail(PGX_ERR_INTERNAL, "device-resident groups on the sparse route");  // (never planned: NO_PARTITION)
    const int64_t groups = Rs.num_groups;
    if (groups > int64_t(PGX_SET_MAX_SPARSE_GROUPS))
      fail(PGX_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL under GROUP BY: more than PGX_SET_MAX_SPARSE_GROUPS groups");
    std::vector<int64_t> cards(size_t(ng), 0);
    for (int g = 0; g < ng; ++g) cards[size_t(g)] = P.gdicts[size_t(g)].card;
    SelKeyLayout L;
    if (!sel_key_layout(cards.data(), ng, L))
      fail(PGX_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL under GROUP BY: group keys of more than 128 bits");
    if (uint64_t(nh + nf) * uint64_t(groups) * kHllRegs * 4 > uint64_t(PGX_HLL_MAX_TABLE_BYTES))
      fail(PGX_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL: registers over PGX_HLL_MAX_TABLE_BYTES");
    offer = groups > 0;
    if (offer) {
      slots = uint64_t(groups);
      distinct_plan(ctx, segs, n, slots, D);    // (the byte limits, at one row per group)
      distinct_plan(ctx, segs, n, slots, F);
      percentile_plan(ctx, segs, n, slots, Q);
      // the groups' keys.  One-word keys claim their slot on the key itself and ~0 is the empty slot: a result that
      // holds that key (every field all ones, 64 bits in all) takes two words, where a state word claims the slot
      dir.host.assign(size_t(groups) * 2, 0);
      std::vector<int64_t> gids(size_t(ng), 0);
      bool all_ones = false;
      for (int64_t i = 0; i < groups; ++i) {
        for (int g = 0; g < ng; ++g)
          gids[size_t(g)] = group_global_id(P.gdicts[size_t(g)], n, Rs.key_seg[size_t(g)][size_t(i)],
                                            Rs.key_id[size_t(g)][size_t(i)]);
        uint64_t k[2];
        if (!sel_key_pack(L, gids.data(), k)) fail(PGX_ERR_INTERNAL, "group id outside its dictionary");
        dir.host[size_t(i) * 2] = k[0];
        dir.host[size_t(i) * 2 + 1] = k[1];
        all_ones = all_ones || k[0] == ~0ull;
      }
      const int W = L.W == 1 && !all_ones ? 1 : 2;
      if (W == 1) {
        for (int64_t i = 0; i < groups; ++i) dir.host[size_t(i)] = dir.host[size_t(i) * 2];
        dir.host.resize(size_t(groups));
      }
      uint64_t cap = 2;
      while (cap < 2 * uint64_t(groups)) cap *= 2;
      dir.keys = DevBuf(ctx, dir.host.size() * 8);
      dir.tkey = DevBuf(ctx, cap * uint64_t(W) * 8);
      dir.tstate = DevBuf(ctx, cap * 4);
      dir.tidx = DevBuf(ctx, cap * 4);
      dir.miss = DevBuf(ctx, 8);
      hip_check(hipMemcpyAsync(dir.keys.p, dir.host.data(), dir.host.size() * 8, hipMemcpyHostToDevice, st),
                "group directory keys H2D");
      hip_check(hipMemsetAsync(dir.miss.p, 0, 8, st), "group directory misses");
      PGX_LAUNCH(st, "pgx_sel_dir_build",
                 pgx_launch_sel_dir_build(dir.keys.as<unsigned long long>(), dir.host.data(), groups, W,
                                          dir.tkey.as<unsigned long long>(), dir.tstate.as<unsigned int>(),
                                          dir.tidx.as<uint32_t>(), cap, st),
                 "group directory build");
      pgx::SelSparseKey& SK = dir.key;
      SK.keys = dir.tkey.as<unsigned long long>();
      SK.state = dir.tstate.as<unsigned int>();
      SK.index = dir.tidx.as<uint32_t>();
      SK.miss = dir.miss.as<unsigned long long>();
      SK.cap = cap;
      for (int g = 0; g < ng; ++g) {
        SK.shift[g] = L.shift[g];
        SK.word[g] = L.word[g];
        SK.bits[g] = L.bits[g];
      }
      SK.groups = uint32_t(groups);
      SK.W = W;
      SK.ngcols = ng;
    }
  }
  DevBuf regs(ctx, std::max<size_t>(1, nh * slots * kHllRegs * 4));
  SelScan S;
  HllItems H;
  if (offer) {
    if (nh) hip_check(hipMemsetAsync(regs.p, 0, nh * slots * kHllRegs * 4, st), "HLL registers");
    S.q = &q;
    S.P = &P;
    S.segs = segs;
    S.n = n;
    S.ng = ng;
    S.slots = slots;
    S.sparse = sparse ? &dir.key : nullptr;
    S.wgs = hll_wgs(ctx, max_words, (nh + nf + D.cols.size() + Q.cols.size()) * size_t(n));
    S.scanned = scanned;
    S.st = st;
    sel_group_columns(ctx, S);
    for (size_t k = 0; k < nh; ++k)
      for (int s = 0; s < n; ++s) {
        const StagedColumn& col = segs[s]->col(hcols[k]);
        HllItem h{};
        h.codes = hll_code_table(ctx, col);
        h.out = regs.as<uint32_t>() + k * slots * kHllRegs;
        h.ncodes = col.card;
        H.add(S, s, col, hmv[k], "DISTINCTCOUNTHLL", h);
      }
    H.upload(ctx, st, "HLL items H2D", "HLL MV items H2D");
    // the multi-value and the single-value items: one launch each, on the same stream, into their own register blocks
    H.launch_mv(S, "pgx_hll_offer_mv", pgx_launch_hll_offer_mv, "HLL MV offers", "pgx_hll_offer_mv_group",
                pgx_launch_hll_offer_mv_group, "HLL MV group offers", "pgx_hll_offer_mv_group_sparse",
                pgx_launch_hll_offer_mv_group_sparse);
    H.launch_sv(S, "pgx_hll_offer", pgx_launch_hll_offer, "HLL offers", "pgx_hll_offer_group",
                pgx_launch_hll_offer_group, "HLL group offers", "pgx_hll_offer_group_sparse",
                pgx_launch_hll_offer_group_sparse);
    // the DISTINCTCOUNT[MV] marks, on the same stream
    if (!D.cols.empty()) distinct_mark(ctx, S, D);
    if (nf) distinct_mark(ctx, S, F);  // FASTHLL: the same marks into its own bitmaps
    // the PERCENTILE[MV] counts, likewise
    if (!Q.cols.empty()) percentile_count(ctx, S, Q);
  }
  if (!sparse) {
    finish_result(ctx, qs, P, B, segs, n, st, &Rs, nullptr);  // waits for the stream (the items' host copies included)
  } else if (offer) {
    // every selected row's group is in the result: a row the directory did not find is a fault of this library
    unsigned long long missed = 0;
    hip_check(hipMemcpyAsync(&missed, dir.miss.p, 8, hipMemcpyDeviceToHost, st), "group directory misses D2H");
    hip_check(hipStreamSynchronize(st), "sync");  // (the items' and the keys' host copies included)
    if (missed != 0) fail(PGX_ERR_INTERNAL, "selected rows whose group the result does not hold");
  }

  // 3. assemble in the request's order; numEntriesScannedPostFilter counts each HLL column among the projected ones
  int extra = 0;  // (a column that functions of several families name counts once)
  std::vector<std::string> special = hcols;
  for (const auto* cols : {&F.cols, &D.cols, &Q.cols})
    for (const auto& c : *cols)
      if (std::find(special.begin(), special.end(), c) == special.end()) special.push_back(c);
  for (const auto& c : special)
    if (std::find(qs.agg_col.begin(), qs.agg_col.end(), c) == qs.agg_col.end() &&
        std::find(q.group_cols.begin(), q.group_cols.end(), c) == q.group_cols.end())
      ++extra;
  for (int i = 0; i < 4; ++i) R->stats[i] = Rs.stats[i];
  R->stats[2] = Rs.stats[0] * (P.n_proj + extra);
  R->num_aggs = na;
  R->agg_fn = q.agg_fn;
  R->top_n = q.top_n;
  R->group_by = ng > 0;
  R->mode = Rs.mode;
  R->hll_pos = hll_pos;
  R->dist_pos = dist_pos;
  R->pct_pos = pct_pos;
  const int64_t groups = ng > 0 ? Rs.num_groups : 1;
  R->hll_groups = groups;
  R->hll_regs.assign((nh + nf) * size_t(groups) * kHllRegs, 0);
  uint8_t* const fregs = R->hll_regs.data() + nh * size_t(groups) * kHllRegs;  // FASTHLL's blocks
  if (ng == 0) {
    std::vector<uint32_t> h32(nh * kHllRegs);
    if (nh) hip_check(hipMemcpy(h32.data(), regs.p, h32.size() * 4, hipMemcpyDeviceToHost), "HLL registers D2H");
    for (size_t i = 0; i < h32.size(); ++i) R->hll_regs[i] = uint8_t(h32[i]);
    distinct_collect(ctx, D, std::vector<int64_t>(1, 0), slots, st, R);
    percentile_collect(ctx, Q, std::vector<int64_t>(1, 0), slots, st, R);
    fasthll_collect(ctx, F, fimg, std::vector<int64_t>(1, 0), slots, st, fregs);
    R->agg_value.assign(size_t(na), 0.0);
    R->agg_count.assign(size_t(na), 0);
    for (int a = 0; a < na; ++a)
      if (sv_pos[size_t(a)] >= 0) {
        R->agg_value[size_t(a)] = Rs.agg_value[size_t(sv_pos[size_t(a)])];
        R->agg_count[size_t(a)] = Rs.agg_count[size_t(sv_pos[size_t(a)])];
      }
    return;
  }
  R->num_groups = Rs.num_groups;
  R->key_seg = std::move(Rs.key_seg);
  R->key_id = std::move(Rs.key_id);
  R->g_value.assign(size_t(na), std::vector<double>());
  R->g_count.assign(size_t(na), std::vector<int64_t>());
  for (int a = 0; a < na; ++a) {
    if (sv_pos[size_t(a)] >= 0) {
      R->g_value[size_t(a)] = std::move(Rs.g_value[size_t(sv_pos[size_t(a)])]);
      R->g_count[size_t(a)] = std::move(Rs.g_count[size_t(sv_pos[size_t(a)])]);
      // (two requests for the same standard function share nothing: each had its own slot in qs)
    } else {
      R->g_value[size_t(a)].assign(size_t(groups), 0.0);
      R->g_count[size_t(a)].assign(size_t(groups), 0);
    }
  }
  if (groups == 0) {
    distinct_collect(ctx, D, std::vector<int64_t>(), slots, st, R);  // (no groups: the accessors' shapes)
    percentile_collect(ctx, Q, std::vector<int64_t>(), slots, st, R);
    return;
  }
  // registers of the groups the result holds: their slots from the keys (global id x gmul; a sparse run: the group's
  // index), narrowed on the device
  std::vector<int64_t> gslot(size_t(groups), 0);
  if (sparse) std::iota(gslot.begin(), gslot.end(), int64_t(0));
  for (int g = 0; g < ng && !sparse; ++g) {
    const GlobalDict& gd = P.gdicts[size_t(g)];
    for (int64_t i = 0; i < groups; ++i)
      gslot[size_t(i)] += group_global_id(gd, n, R->key_seg[size_t(g)][size_t(i)], R->key_id[size_t(g)][size_t(i)]) *
                          int64_t(K.gmul[g]);
  }
  for (int64_t i = 0; i < groups; ++i)
    if (gslot[size_t(i)] < 0 || uint64_t(gslot[size_t(i)]) >= slots) fail(PGX_ERR_INTERNAL, "group slot out of range");
  distinct_collect(ctx, D, gslot, slots, st, R);
  percentile_collect(ctx, Q, gslot, slots, st, R);
  fasthll_collect(ctx, F, fimg, gslot, slots, st, fregs);
  if (nh == 0) return;
  // (a sparse run of more than 65,536 groups goes through pgx_hll_narrow in stretches, each a table of its own read
  // with the first entries of sdev: that rests on gslot[i] == i, checked here as the other two collectors check it)
  sel_result_rows_ok(gslot, slots);
  DevBuf sdev(ctx, size_t(groups) * 8), odev(ctx, size_t(groups) * kHllRegs);
  hip_check(hipMemcpyAsync(sdev.p, gslot.data(), size_t(groups) * 8, hipMemcpyHostToDevice, st), "HLL slots H2D");
  for (size_t k = 0; k < nh; ++k) {
    sel_result_stretches(size_t(groups), slots, [&](size_t c0, size_t cn, uint64_t cs) {
      PGX_LAUNCH(st, "pgx_hll_narrow",
                 pgx_launch_hll_narrow(regs.as<uint32_t>() + (k * slots + c0) * kHllRegs, sdev.as<int64_t>(), int64_t(cn),
                                       int64_t(cs), odev.as<uint32_t>() + c0 * (kHllRegs / 4), st),
                 "HLL narrow");
    });
    hip_check(hipMemcpyAsync(R->hll_regs.data() + k * size_t(groups) * kHllRegs, odev.p, size_t(groups) * kHllRegs,
                             hipMemcpyDeviceToHost, st),
              "HLL registers D2H");
    hip_check(hipStreamSynchronize(st), "sync");
  }
}

}  // namespace pgxh

extern "C" {

pgx_status pgx_hll_codes(int32_t data_type, const void* values, const int32_t* string_offsets, int64_t n,
                         uint16_t* codes) {
  return guarded([&] {
    if (const char* err = hash_values(data_type, values, string_offsets, n, codes, hll_code))
      fail(PGX_ERR_INVALID_ARG, err);
  });
}

pgx_status pgx_java_hash_codes(int32_t data_type, const void* values, const int32_t* string_offsets, int64_t n,
                               int32_t* hash_codes) {
  return guarded([&] {
    if (const char* err = java_hash_codes(data_type, values, string_offsets, n, hash_codes))
      fail(PGX_ERR_INVALID_ARG, err);
  });
}

pgx_status pgx_result_hll(const pgx_result* r, int32_t agg_index, int64_t first_group, int64_t num_groups,
                          uint8_t* registers) {
  return guarded([&] {
    if (r) r->ready();
    if (!r) fail(PGX_ERR_INVALID_ARG, "NULL argument");
    if (r->select) fail(PGX_ERR_INVALID_ARG, "selection result");
    if (agg_index < 0 || agg_index >= r->num_aggs || size_t(agg_index) >= r->hll_pos.size() ||
        r->hll_pos[size_t(agg_index)] < 0)
      fail(PGX_ERR_INVALID_ARG, "not a DISTINCTCOUNTHLL function index");  // (a DISTINCTCOUNT index among them)
    if (first_group < 0 || num_groups < 0 || first_group > r->hll_groups || num_groups > r->hll_groups - first_group)
      fail(PGX_ERR_INVALID_ARG, "group range outside the result");
    if (num_groups == 0) return;
    if (!registers) fail(PGX_ERR_INVALID_ARG, "NULL argument");
    const size_t k = size_t(r->hll_pos[size_t(agg_index)]);
    std::memcpy(registers, r->hll_regs.data() + (k * size_t(r->hll_groups) + size_t(first_group)) * kHllRegs,
                size_t(num_groups) * kHllRegs);
  });
}

}  // extern "C"
