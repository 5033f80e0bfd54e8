// libpgx: DISTINCTCOUNT / DISTINCTCOUNTMV inside run_hll (pgx_hll.cpp) -- the presence bitmaps, the mark launches on
// the scan's stream, and the result: set sizes and hash codes per group, read with pgx_result_distinct_counts and
// pgx_result_distinct.  DistinctCountAggregationFunction (operator/aggregation/function/
// DistinctCountAggregationFunction.java): the intermediate is the set of (int) hashCode over the selected docs' values,
// combine is set union, reduce its size.  The kernels are in pgx_distinct.hip; the items are built and launched by the
// SelItems of pgx_host.h, as the HLL offers' are.
#include "pgx_hash.h"
#include "pgx_host.h"

namespace pgxh {

// The same dictionary: one SharedDict (numeric), or equal staged STRING dictionaries.
bool same_dictionary(const StagedColumn& a, const StagedColumn& b) {
  if (a.shared || b.shared) return a.shared == b.shared;
  return a.data_type == b.data_type && a.card == b.card && a.dict_hash == b.dict_hash && a.svals == b.svals &&
         a.ivals == b.ivals && a.dvals == b.dvals;
}

// The bitmaps of the query: per column one per distinct dictionary of the executed segments.  Sized, checked against
// PGX_DISTINCT_MAX_TABLE_BYTES and only then allocated.
void distinct_plan(pgx_ctx* ctx, pgx_segment* const* segs, int n, uint64_t slots, DistinctRun& D) {
  uint64_t bytes = 0;
  D.maps.clear();
  D.maps.resize(D.cols.size());
  D.map_of.assign(D.cols.size(), std::vector<int>(size_t(n), 0));
  for (size_t k = 0; k < D.cols.size(); ++k)
    for (int s = 0; s < n; ++s) {
      const StagedColumn& c = segs[s]->col(D.cols[k]);
      auto& maps = D.maps[k];
      size_t b = 0;
      while (b < maps.size() && !same_dictionary(*maps[b].col, c)) ++b;
      if (b == maps.size()) {
        DistinctBitmap m;
        m.col = &c;
        m.words = (uint32_t(c.card) + 31u) >> 5;
        bytes += slots * m.words * 4;
        maps.push_back(std::move(m));
      }
      D.map_of[k][size_t(s)] = int(b);
    }
  if (bytes > uint64_t(PGX_DISTINCT_MAX_TABLE_BYTES))
    fail(PGX_ERR_UNSUPPORTED, std::string(D.fn) + ": presence bitmaps over PGX_DISTINCT_MAX_TABLE_BYTES");
  for (auto& maps : D.maps)
    for (auto& m : maps) {
      m.table = DevBuf(ctx, size_t(slots) * m.words * 4);
      if (D.hashes) m.hash = distinct_hash_table(ctx, *m.col);
    }
}

// One item per (column, segment), one launch for the single-value and one for the multi-value columns.
void distinct_mark(pgx_ctx* ctx, const SelScan& S, DistinctRun& D) {
  for (auto& maps : D.maps)
    for (auto& m : maps)
      hip_check(hipMemsetAsync(m.table.p, 0, size_t(S.slots) * m.words * 4, S.st), "DISTINCTCOUNT bitmaps");
  for (size_t k = 0; k < D.cols.size(); ++k)
    for (int s = 0; s < S.n; ++s) {
      const StagedColumn& col = S.segs[s]->col(D.cols[k]);
      pgx::DistinctItem d{};
      d.out = D.maps[k][size_t(D.map_of[k][size_t(s)])].table.as<uint32_t>();
      d.card = col.card;
      D.items.add(S, s, col, D.mv[k], D.fn, d);
    }
  D.items.upload(ctx, S.st, "DISTINCTCOUNT items H2D", "DISTINCTCOUNTMV items H2D");
  D.items.launch_sv(S, "pgx_distinct_mark", pgx_launch_distinct_mark, "DISTINCTCOUNT marks",
                    "pgx_distinct_mark_group", pgx_launch_distinct_mark_group, "DISTINCTCOUNT group marks",
                    "pgx_distinct_mark_group_sparse", pgx_launch_distinct_mark_group_sparse);
  D.items.launch_mv(S, "pgx_distinct_mark_mv", pgx_launch_distinct_mark_mv, "DISTINCTCOUNTMV marks",
                    "pgx_distinct_mark_mv_group", pgx_launch_distinct_mark_mv_group, "DISTINCTCOUNTMV group marks",
                    "pgx_distinct_mark_mv_group_sparse", pgx_launch_distinct_mark_mv_group_sparse);
}

// The result's groups: per bitmap the rows' sizes (pgx_distinct_count), then exactly that many hash codes
// (pgx_distinct_emit); per group the lists of the column's dictionaries merged by sort + unique.  One dictionary needs
// the unique step too: hash codes collide.
void distinct_collect(pgx_ctx* ctx, DistinctRun& D, const std::vector<int64_t>& rows, uint64_t slots, hipStream_t st,
                      pgx_result* R) {
  const size_t nd = D.cols.size(), groups = rows.size();
  R->dist_groups = int64_t(groups);
  R->dist_start.assign(nd, std::vector<int64_t>(groups + 1, 0));
  R->dist_codes.assign(nd, {});
  if (nd == 0 || groups == 0) return;
  sel_result_rows_ok(rows, slots);
  const int budget = 8 * std::max(1, ctx->num_cus);
  const int wgs = int(std::min<size_t>(groups, size_t(budget)));
  DevBuf rdev(ctx, groups * 8);
  hip_check(hipMemcpyAsync(rdev.p, rows.data(), groups * 8, hipMemcpyHostToDevice, st), "DISTINCTCOUNT rows H2D");
  struct Part {  // one bitmap's share of the result
    const DistinctBitmap* m;
    DevBuf cdev, odev, out;
    std::vector<uint32_t> counts;
    std::vector<int64_t> off;
    std::vector<int32_t> codes;
  };
  std::vector<std::vector<Part>> parts(nd);
  for (size_t k = 0; k < nd; ++k)
    for (const DistinctBitmap& m : D.maps[k]) {
      Part p;
      p.m = &m;
      p.cdev = DevBuf(ctx, groups * 4);
      p.counts.assign(groups, 0);
      sel_result_stretches(groups, slots, [&](size_t c0, size_t cn, uint64_t cs) {
        PGX_LAUNCH(st, "pgx_distinct_count",
                   pgx_launch_distinct_count(m.table.as<uint32_t>() + c0 * m.words, m.col->card, rdev.as<int64_t>(),
                                             int64_t(cn), int64_t(cs), p.cdev.as<uint32_t>() + c0, wgs, st),
                   "DISTINCTCOUNT sizes");
      });
      hip_check(hipMemcpyAsync(p.counts.data(), p.cdev.p, groups * 4, hipMemcpyDeviceToHost, st),
                "DISTINCTCOUNT sizes D2H");
      parts[k].push_back(std::move(p));
    }
  hip_check(hipStreamSynchronize(st), "sync");
  for (auto& pk : parts)
    for (Part& p : pk) {
      p.off.assign(groups + 1, 0);
      for (size_t i = 0; i < groups; ++i) p.off[i + 1] = p.off[i] + int64_t(p.counts[i]);
      const int64_t total = p.off[groups];
      if (total == 0) continue;
      // a long row is shared: a workgroup per 1,024 words, as far as the rows leave workgroups to spare
      const int per_row = std::max(1, std::min(int(std::min<uint32_t>(64u, (p.m->words + 1023u) / 1024u)), budget / wgs));
      p.odev = DevBuf(ctx, groups * 8);
      p.out = DevBuf(ctx, size_t(total) * 4);
      p.codes.assign(size_t(total), 0);
      hip_check(hipMemcpyAsync(p.odev.p, p.off.data(), groups * 8, hipMemcpyHostToDevice, st),
                "DISTINCTCOUNT offsets H2D");
      sel_result_stretches(groups, slots, [&](size_t c0, size_t cn, uint64_t cs) {
        PGX_LAUNCH(st, "pgx_distinct_emit",
                   pgx_launch_distinct_emit(p.m->table.as<uint32_t>() + c0 * p.m->words, p.m->col->card,
                                            rdev.as<int64_t>(), p.odev.as<int64_t>() + c0, int64_t(cn), int64_t(cs),
                                            p.m->hash, p.out.as<int32_t>(), total, per_row, wgs, st),
                   "DISTINCTCOUNT hash codes");
      });
      hip_check(hipMemcpyAsync(p.codes.data(), p.out.p, size_t(total) * 4, hipMemcpyDeviceToHost, st),
                "DISTINCTCOUNT hash codes D2H");
    }
  hip_check(hipStreamSynchronize(st), "sync");
  std::vector<int32_t> one;
  for (size_t k = 0; k < nd; ++k) {
    auto& codes = R->dist_codes[k];
    auto& start = R->dist_start[k];
    for (size_t i = 0; i < groups; ++i) {
      one.clear();
      for (const Part& p : parts[k]) one.insert(one.end(), p.codes.begin() + p.off[i], p.codes.begin() + p.off[i + 1]);
      sort_unique(one);
      codes.insert(codes.end(), one.begin(), one.end());
      start[i + 1] = int64_t(codes.size());
    }
  }
}

}  // namespace pgxh

extern "C" {

static const pgx_result* distinct_result(const pgx_result* r, int32_t agg_index, int64_t first_group,
                                         int64_t num_groups) {
  using namespace pgxh;
  if (r) r->ready();
  if (!r) fail(PGX_ERR_INVALID_ARG, "NULL argument");
  if (r->select) fail(PGX_ERR_INVALID_ARG, "selection result");
  if (agg_index < 0 || agg_index >= r->num_aggs || !r->is_distinct(agg_index))
    fail(PGX_ERR_INVALID_ARG, "not a DISTINCTCOUNT function index");
  if (first_group < 0 || num_groups < 0 || first_group > r->dist_groups || num_groups > r->dist_groups - first_group)
    fail(PGX_ERR_INVALID_ARG, "group range outside the result");
  return r;
}

pgx_status pgx_result_distinct_counts(const pgx_result* r, int32_t agg_index, int64_t first_group, int64_t num_groups,
                                      int64_t* counts) {
  using namespace pgxh;
  return guarded([&] {
    distinct_result(r, agg_index, first_group, num_groups);
    if (num_groups == 0) return;
    if (!counts) fail(PGX_ERR_INVALID_ARG, "NULL argument");
    const auto& start = r->dist_start[size_t(r->dist_pos[size_t(agg_index)])];
    for (int64_t i = 0; i < num_groups; ++i)
      counts[i] = start[size_t(first_group + i) + 1] - start[size_t(first_group + i)];
  });
}

pgx_status pgx_result_distinct(const pgx_result* r, int32_t agg_index, int64_t first_group, int64_t num_groups,
                               int32_t* hash_codes, int64_t capacity) {
  using namespace pgxh;
  return guarded([&] {
    distinct_result(r, agg_index, first_group, num_groups);
    const size_t k = size_t(r->dist_pos[size_t(agg_index)]);
    const int64_t a = r->dist_start[k][size_t(first_group)], b = r->dist_start[k][size_t(first_group + num_groups)];
    if (capacity < b - a) fail(PGX_ERR_INVALID_ARG, "hash code capacity too small");
    if (b == a) return;
    if (!hash_codes) fail(PGX_ERR_INVALID_ARG, "NULL argument");
    std::memcpy(hash_codes, r->dist_codes[k].data() + a, size_t(b - a) * 4);
  });
}

}  // extern "C"
