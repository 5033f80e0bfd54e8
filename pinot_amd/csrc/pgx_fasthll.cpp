// libpgx: FASTHLL inside run_hll (pgx_hll.cpp) -- pgx_fasthll_registers (the host decode of serialized estimators:
// fasthll_decode of pgx_hash.h), the per-dictionary register image, and the result: the fold of the presence bitmaps' rows into the groups' registers.
// FastHllAggregationFunction (operator/aggregation/function/FastHllAggregationFunction.java) merges the pre-aggregated
// HyperLogLogs of a STRING column (startree/hll/HllUtil.java convertHllToString / convertStringToHll); the
// intermediate is the merged estimator's 256 registers.  The bitmaps are DISTINCTCOUNT's (pgx_distinct.cpp: a second
// DistinctRun without hash tables, marked by the same kernels); the fold kernel is in pgx_fasthll.hip.
#include "pgx_hash.h"
#include "pgx_host.h"

namespace pgxh {

static_assert(kFastHllRegs == kHllRegs, "pgx_hash.h decodes log2m-8 estimators");

// The register image of a STRING dictionary in HBM: card x 256 bytes, row i the decoded estimator of value i.  Built on
// the first query that needs it and kept on the staged column beside its HLL codes (a realtime snapshot stages its
// grown dictionary afresh).  A value that is no estimator refuses the query.
static const uint32_t* fasthll_image(pgx_ctx* ctx, const StagedColumn& c) {
  std::lock_guard<std::mutex> g(ctx->dict_mu);
  if (c.fasthll_img.p) return c.fasthll_img.as<uint32_t>();
  std::vector<uint8_t> img(size_t(std::max(c.card, 1)) * kHllRegs, 0);
  for (int i = 0; i < c.card; ++i) {
    const std::string& v = c.svals[size_t(i)];
    if (!fasthll_decode(reinterpret_cast<const uint8_t*>(v.data()), v.size(), img.data() + size_t(i) * kHllRegs))
      fail(PGX_ERR_UNSUPPORTED, "FASTHLL: a value of column " + c.name + " is not a serialized log2m-8 HyperLogLog");
  }
  DevBuf b(ctx, img.size());
  hip_check(hipMemcpy(b.p, img.data(), img.size(), hipMemcpyHostToDevice), "FASTHLL register image H2D");
  c.fasthll_img = std::move(b);
  return c.fasthll_img.as<uint32_t>();
}

// The columns are single-value STRING columns in every executed segment, and the images of their distinct dictionaries
// (found as distinct_plan finds them: a dictionary's first column keeps the image) stay within
// PGX_FASTHLL_MAX_IMAGE_BYTES; only then is an image built.
void fasthll_images(pgx_ctx* ctx, pgx_segment* const* segs, int n, const DistinctRun& F,
                    std::vector<std::vector<const uint32_t*>>& images) {
  std::vector<std::vector<const StagedColumn*>> dicts(F.cols.size());
  uint64_t bytes = 0;
  for (size_t k = 0; k < F.cols.size(); ++k)
    for (int s = 0; s < n; ++s) {
      const StagedColumn& c = segs[s]->col(F.cols[k]);
      if (c.is_mv) fail(PGX_ERR_UNSUPPORTED, "FASTHLL on multi-value column " + c.name);
      if (c.data_type != PGX_STRING) fail(PGX_ERR_UNSUPPORTED, "FASTHLL on non-STRING column " + c.name);
      auto& d = dicts[k];
      if (std::none_of(d.begin(), d.end(), [&](const StagedColumn* o) { return same_dictionary(*o, c); })) {
        d.push_back(&c);
        bytes += uint64_t(std::max(c.card, 1)) * kHllRegs;
      }
    }
  if (bytes > uint64_t(PGX_FASTHLL_MAX_IMAGE_BYTES))
    fail(PGX_ERR_UNSUPPORTED, "FASTHLL: register images over PGX_FASTHLL_MAX_IMAGE_BYTES");
  images.assign(F.cols.size(), {});
  for (size_t k = 0; k < F.cols.size(); ++k)
    for (const StagedColumn* c : dicts[k]) images[k].push_back(fasthll_image(ctx, *c));
}

// regs: per column the result's groups x 256 bytes, in the result's order.  Per column one u32 register table of a row
// per group; every bitmap (dictionary) of the column folds into it, then pgx_hll_narrow writes the bytes.
void fasthll_collect(pgx_ctx* ctx, const DistinctRun& F, const std::vector<std::vector<const uint32_t*>>& images,
                     const std::vector<int64_t>& rows, uint64_t slots, hipStream_t st, uint8_t* regs) {
  const size_t nf = F.cols.size(), groups = rows.size();
  if (nf == 0 || groups == 0) return;
  sel_result_rows_ok(rows, slots);
  const size_t chunk = std::min(groups, size_t(pgx::kHllMaxGroupSlots));
  std::vector<int64_t> iota(chunk);
  std::iota(iota.begin(), iota.end(), int64_t(0));
  DevBuf rdev(ctx, groups * 8), idev(ctx, chunk * 8), wide(ctx, groups * kHllRegs * 4), odev(ctx, groups * kHllRegs);
  hip_check(hipMemcpyAsync(rdev.p, rows.data(), groups * 8, hipMemcpyHostToDevice, st), "FASTHLL rows H2D");
  hip_check(hipMemcpyAsync(idev.p, iota.data(), chunk * 8, hipMemcpyHostToDevice, st), "FASTHLL rows H2D");
  const int budget = 8 * std::max(1, ctx->num_cus);
  for (size_t k = 0; k < nf; ++k) {
    hip_check(hipMemsetAsync(wide.p, 0, groups * kHllRegs * 4, st), "FASTHLL registers");
    for (size_t b = 0; b < F.maps[k].size(); ++b) {
      const DistinctBitmap& m = F.maps[k][b];
      const int wgs = int(std::min<size_t>(groups, size_t(std::max(1, budget / pgx_fasthll_fold_split(m.col->card)))));
      sel_result_stretches(groups, slots, [&](size_t c0, size_t cn, uint64_t cs) {
        // (a stretch is a table of its own whose rows are 0, 1, ...: the first entries of rdev and of rows)
        PGX_LAUNCH(st, "pgx_fasthll_fold",
                   pgx_launch_fasthll_fold(m.table.as<uint32_t>() + c0 * m.words, m.col->card, images[k][b],
                                           rdev.as<int64_t>(), rows.data(), int64_t(cn), int64_t(cs),
                                           wide.as<uint32_t>() + c0 * kHllRegs, std::min(wgs, int(cn)), st),
                   "FASTHLL fold");
      });
    }
    sel_result_stretches(groups, uint64_t(groups), [&](size_t c0, size_t cn, uint64_t cs) {
      PGX_LAUNCH(st, "pgx_hll_narrow",
                 pgx_launch_hll_narrow(wide.as<uint32_t>() + c0 * kHllRegs, idev.as<int64_t>(), int64_t(cn), int64_t(cs),
                                       odev.as<uint32_t>() + c0 * (kHllRegs / 4), st),
                 "FASTHLL narrow");
    });
    hip_check(hipMemcpyAsync(regs + k * groups * kHllRegs, odev.p, groups * kHllRegs, hipMemcpyDeviceToHost, st),
              "FASTHLL registers D2H");
    hip_check(hipStreamSynchronize(st), "sync");
  }
}

}  // namespace pgxh

extern "C" {

pgx_status pgx_fasthll_registers(const void* values_utf8, const int32_t* string_offsets, int64_t n, uint8_t* registers,
                                 int64_t* bad_index) {
  using namespace pgxh;
  return guarded([&] {
    if (bad_index) *bad_index = -1;
    if (n < 0 || (n > 0 && (!values_utf8 || !string_offsets || !registers))) fail(PGX_ERR_INVALID_ARG, "bad argument");
    for (int64_t i = 0; i < n; ++i) {
      const int32_t a = string_offsets[i], b = string_offsets[i + 1];
      if (a < 0 || b < a) fail(PGX_ERR_INVALID_ARG, "string offsets not ascending");
      if (!fasthll_decode(static_cast<const uint8_t*>(values_utf8) + a, size_t(b - a), registers + i * kHllRegs)) {
        if (bad_index) *bad_index = i;
        fail(PGX_ERR_UNSUPPORTED, "not a serialized log2m-8 HyperLogLog");
      }
    }
  });
}

}  // extern "C"
