// libpgx: PERCENTILE / PERCENTILEMV inside run_hll (pgx_hll.cpp) -- the counter tables, the count launches on the
// scan's stream, and the result: (value, count) pairs per group, read with pgx_result_percentile_counts and
// pgx_result_percentile.  PercentileAggregationFunction (operator/aggregation/function/
// PercentileAggregationFunction.java): the intermediate is the DoubleArrayList of the selected docs' values, combine is
// concatenation, reduce sorts it and takes element (int)(size * p / 100) (query/aggregation/function/quantile/
// PercentileUtil.java:40-52); PercentileMVAggregationFunction.java: the same over every value of every selected doc.
// Held as a histogram it is one counter per dictId.  The kernels are in pgx_percentile.hip; the items are built and
// launched by the SelItems of pgx_host.h, as the HLL offers' and the DISTINCTCOUNT marks' are.
#include "pgx_host.h"

namespace pgxh {

// The tables of the query: per column one per distinct dictionary of the executed segments.  Sized, checked against
// PGX_PERCENTILE_MAX_TABLE_BYTES and only then allocated.
void percentile_plan(pgx_ctx* ctx, pgx_segment* const* segs, int n, uint64_t slots, PercentileRun& Q) {
  uint64_t bytes = 0;
  Q.tabs.clear();
  Q.tabs.resize(Q.cols.size());
  Q.tab_of.assign(Q.cols.size(), std::vector<int>(size_t(n), 0));
  for (size_t k = 0; k < Q.cols.size(); ++k)
    for (int s = 0; s < n; ++s) {
      const StagedColumn& c = segs[s]->col(Q.cols[k]);
      if (c.data_type == PGX_STRING) fail(PGX_ERR_UNSUPPORTED, "PERCENTILE on STRING column " + c.name);
      auto& tabs = Q.tabs[k];
      size_t b = 0;
      while (b < tabs.size() && !same_dictionary(*tabs[b].col, c)) ++b;
      if (b == tabs.size()) {
        PercentileTable t;
        t.col = &c;
        bytes += slots * uint64_t(std::max(c.card, 1)) * 8;
        tabs.push_back(std::move(t));
      }
      Q.tab_of[k][size_t(s)] = int(b);
    }
  if (bytes > uint64_t(PGX_PERCENTILE_MAX_TABLE_BYTES))
    fail(PGX_ERR_UNSUPPORTED, "PERCENTILE: counter tables over PGX_PERCENTILE_MAX_TABLE_BYTES");
  for (auto& tabs : Q.tabs)
    for (auto& t : tabs) t.table = DevBuf(ctx, size_t(slots) * size_t(std::max(t.col->card, 1)) * 8);
}

// One item per (column, segment), one launch for the single-value and one for the multi-value columns.
void percentile_count(pgx_ctx* ctx, const SelScan& S, PercentileRun& Q) {
  for (auto& tabs : Q.tabs)
    for (auto& t : tabs)
      hip_check(hipMemsetAsync(t.table.p, 0, size_t(S.slots) * size_t(std::max(t.col->card, 1)) * 8, S.st),
                "PERCENTILE counters");
  for (size_t k = 0; k < Q.cols.size(); ++k)
    for (int s = 0; s < S.n; ++s) {
      const StagedColumn& col = S.segs[s]->col(Q.cols[k]);
      if (col.card < 1) continue;  // (an empty dictionary: no rows)
      pgx::PercentileItem d{};
      d.out = Q.tabs[k][size_t(Q.tab_of[k][size_t(s)])].table.as<uint64_t>();
      d.card = col.card;
      Q.items.add(S, s, col, Q.mv[k], "PERCENTILE", d);
    }
  Q.items.upload(ctx, S.st, "PERCENTILE items H2D", "PERCENTILEMV items H2D");
  Q.items.launch_sv(S, "pgx_percentile_count", pgx_launch_percentile_count, "PERCENTILE counts",
                    "pgx_percentile_count_group", pgx_launch_percentile_count_group, "PERCENTILE group counts",
                    "pgx_percentile_count_group_sparse", pgx_launch_percentile_count_group_sparse);
  Q.items.launch_mv(S, "pgx_percentile_count_mv", pgx_launch_percentile_count_mv, "PERCENTILEMV counts",
                    "pgx_percentile_count_mv_group", pgx_launch_percentile_count_mv_group,
                    "PERCENTILEMV group counts", "pgx_percentile_count_mv_group_sparse",
                    pgx_launch_percentile_count_mv_group_sparse);
}

// the double the reference's Dictionary.getDoubleValue gives for dictId i
static double dict_double(const StagedColumn& c, int32_t i) {
  return c.data_type == PGX_INT || c.data_type == PGX_LONG ? double(c.ivals[size_t(i)]) : c.dvals[size_t(i)];
}

// The result's groups: per table the rows' sizes (pgx_percentile_sizes), then exactly that many (dictId, count) pairs
// (pgx_percentile_emit); per group the parts of the column's dictionaries merged by value, equal values summed.
void percentile_collect(pgx_ctx* ctx, PercentileRun& Q, const std::vector<int64_t>& rows, uint64_t slots,
                        hipStream_t st, pgx_result* R) {
  const size_t nq = Q.cols.size(), groups = rows.size();
  R->pct_groups = int64_t(groups);
  R->pct_start.assign(nq, std::vector<int64_t>(groups + 1, 0));
  R->pct_values.assign(nq, {});
  R->pct_counts.assign(nq, {});
  if (nq == 0 || groups == 0) return;
  sel_result_rows_ok(rows, slots);
  const int budget = 8 * std::max(1, ctx->num_cus);
  const int wgs = int(std::min<size_t>(groups, size_t(budget)));
  DevBuf rdev(ctx, groups * 8);
  hip_check(hipMemcpyAsync(rdev.p, rows.data(), groups * 8, hipMemcpyHostToDevice, st), "PERCENTILE rows H2D");
  struct Part {  // one table's share of the result
    const PercentileTable* t;
    DevBuf sdev, odev, idev, cdev;
    std::vector<uint32_t> sizes;
    std::vector<int64_t> off;
    std::vector<int32_t> ids;
    std::vector<uint64_t> counts;
  };
  std::vector<std::vector<Part>> parts(nq);
  for (size_t k = 0; k < nq; ++k)
    for (const PercentileTable& t : Q.tabs[k]) {
      Part p;
      p.t = &t;
      p.sizes.assign(groups, 0);
      if (t.col->card >= 1) {
        p.sdev = DevBuf(ctx, groups * 4);
        sel_result_stretches(groups, slots, [&](size_t c0, size_t cn, uint64_t cs) {
          PGX_LAUNCH(st, "pgx_percentile_sizes",
                     pgx_launch_percentile_sizes(t.table.as<uint64_t>() + c0 * size_t(t.col->card), t.col->card,
                                                 rdev.as<int64_t>(), int64_t(cn), int64_t(cs),
                                                 p.sdev.as<uint32_t>() + c0, wgs, st),
                     "PERCENTILE sizes");
        });
        hip_check(hipMemcpyAsync(p.sizes.data(), p.sdev.p, groups * 4, hipMemcpyDeviceToHost, st),
                  "PERCENTILE sizes D2H");
      }
      parts[k].push_back(std::move(p));
    }
  hip_check(hipStreamSynchronize(st), "sync");
  for (auto& pk : parts)
    for (Part& p : pk) {
      p.off.assign(groups + 1, 0);
      for (size_t i = 0; i < groups; ++i) p.off[i + 1] = p.off[i] + int64_t(p.sizes[i]);
      const int64_t total = p.off[groups];
      if (total == 0) continue;
      // a long row is shared: a workgroup per 8,192 counters, as far as the rows leave workgroups to spare
      const uint32_t card = uint32_t(p.t->col->card);
      const int per_row = std::max(1, std::min(int(std::min<uint32_t>(64u, (card + 8191u) / 8192u)), budget / wgs));
      p.odev = DevBuf(ctx, groups * 8);
      p.idev = DevBuf(ctx, size_t(total) * 4);
      p.cdev = DevBuf(ctx, size_t(total) * 8);
      p.ids.assign(size_t(total), 0);
      p.counts.assign(size_t(total), 0);
      hip_check(hipMemcpyAsync(p.odev.p, p.off.data(), groups * 8, hipMemcpyHostToDevice, st),
                "PERCENTILE offsets H2D");
      sel_result_stretches(groups, slots, [&](size_t c0, size_t cn, uint64_t cs) {
        PGX_LAUNCH(st, "pgx_percentile_emit",
                   pgx_launch_percentile_emit(p.t->table.as<uint64_t>() + c0 * size_t(card), p.t->col->card,
                                              rdev.as<int64_t>(), p.odev.as<int64_t>() + c0, int64_t(cn), int64_t(cs),
                                              p.idev.as<int32_t>(), p.cdev.as<uint64_t>(), total, per_row, wgs, st),
                   "PERCENTILE pairs");
      });
      hip_check(hipMemcpyAsync(p.ids.data(), p.idev.p, size_t(total) * 4, hipMemcpyDeviceToHost, st),
                "PERCENTILE dictIds D2H");
      hip_check(hipMemcpyAsync(p.counts.data(), p.cdev.p, size_t(total) * 8, hipMemcpyDeviceToHost, st),
                "PERCENTILE counts D2H");
    }
  hip_check(hipStreamSynchronize(st), "sync");
  std::vector<std::pair<double, int64_t>> one;
  for (size_t k = 0; k < nq; ++k) {
    auto& values = R->pct_values[k];
    auto& counts = R->pct_counts[k];
    auto& start = R->pct_start[k];
    for (size_t i = 0; i < groups; ++i) {
      one.clear();
      for (const Part& p : parts[k])
        for (int64_t j = p.off[i]; j < p.off[i + 1]; ++j) {
          const int32_t id = p.ids[size_t(j)];
          if (id < 0 || id >= p.t->col->card) fail(PGX_ERR_INTERNAL, "PERCENTILE dictId out of range");
          one.emplace_back(dict_double(*p.t->col, id), int64_t(p.counts[size_t(j)]));
        }
      // one dictionary's pairs ascend already (a sorted dictionary read in dictId order); several need the sort
      if (parts[k].size() > 1)
        std::stable_sort(one.begin(), one.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
      for (const auto& vc : one) {
        if (int64_t(values.size()) > start[i] && values.back() == vc.first) counts.back() += vc.second;
        else {
          values.push_back(vc.first);
          counts.push_back(vc.second);
        }
      }
      start[i + 1] = int64_t(values.size());
    }
  }
}

}  // namespace pgxh

extern "C" {

static const pgx_result* percentile_result(const pgx_result* r, int32_t agg_index, int64_t first_group,
                                           int64_t num_groups) {
  using namespace pgxh;
  if (r) r->ready();
  if (!r) fail(PGX_ERR_INVALID_ARG, "NULL argument");
  if (r->select) fail(PGX_ERR_INVALID_ARG, "selection result");
  if (agg_index < 0 || agg_index >= r->num_aggs || !r->is_percentile(agg_index))
    fail(PGX_ERR_INVALID_ARG, "not a PERCENTILE function index");
  if (first_group < 0 || num_groups < 0 || first_group > r->pct_groups || num_groups > r->pct_groups - first_group)
    fail(PGX_ERR_INVALID_ARG, "group range outside the result");
  return r;
}

pgx_status pgx_result_percentile_counts(const pgx_result* r, int32_t agg_index, int64_t first_group,
                                        int64_t num_groups, int64_t* counts) {
  using namespace pgxh;
  return guarded([&] {
    percentile_result(r, agg_index, first_group, num_groups);
    if (num_groups == 0) return;
    if (!counts) fail(PGX_ERR_INVALID_ARG, "NULL argument");
    const auto& start = r->pct_start[size_t(r->pct_pos[size_t(agg_index)])];
    for (int64_t i = 0; i < num_groups; ++i)
      counts[i] = start[size_t(first_group + i) + 1] - start[size_t(first_group + i)];
  });
}

pgx_status pgx_result_percentile(const pgx_result* r, int32_t agg_index, int64_t first_group, int64_t num_groups,
                                 double* values, int64_t* value_counts, int64_t capacity) {
  using namespace pgxh;
  return guarded([&] {
    percentile_result(r, agg_index, first_group, num_groups);
    const size_t k = size_t(r->pct_pos[size_t(agg_index)]);
    const int64_t a = r->pct_start[k][size_t(first_group)], b = r->pct_start[k][size_t(first_group + num_groups)];
    if (capacity < b - a) fail(PGX_ERR_INVALID_ARG, "pair capacity too small");
    if (b == a) return;
    if (!values || !value_counts) fail(PGX_ERR_INVALID_ARG, "NULL argument");
    std::memcpy(values, r->pct_values[k].data() + a, size_t(b - a) * 8);
    std::memcpy(value_counts, r->pct_counts[k].data() + a, size_t(b - a) * 8);
  });
}

pgx_status pgx_histogram_percentile(const double* values, const int64_t* counts, int64_t n, int32_t percentile,
                                    double* out) {
  using namespace pgxh;
  return guarded([&] {
    if (!out || n < 0 || (n > 0 && (!values || !counts))) fail(PGX_ERR_INVALID_ARG, "NULL argument");
    if (percentile < 0 || percentile > 100) fail(PGX_ERR_INVALID_ARG, "percentile outside 0..100");
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
      if (counts[i] < 0) fail(PGX_ERR_INVALID_ARG, "negative count");
      if (i > 0 && !(values[i - 1] < values[i])) fail(PGX_ERR_INVALID_ARG, "values not ascending");
      if (counts[i] > INT64_MAX - total) fail(PGX_ERR_INVALID_ARG, "counts overflow");
      total += counts[i];
    }
    if (total == 0) fail(PGX_ERR_INVALID_ARG, "percentile of an empty value list");
    const double pos = double(total) * (double(percentile) / 100.0);  // PercentileUtil: (int)(size * (p / 100.0))
    int64_t idx = pos >= 9.2e18 ? INT64_MAX : int64_t(pos);
    if (idx >= total) fail(PGX_ERR_INVALID_ARG, "percentile index past the value list");
    for (int64_t i = 0; i < n; ++i) {
      if (idx < counts[i]) {
        *out = values[i];
        return;
      }
      idx -= counts[i];
    }
    fail(PGX_ERR_INTERNAL, "unreachable");
  });
}

}  // extern "C"
