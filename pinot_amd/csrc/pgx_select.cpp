// libpgx: selection queries with ORDER BY -- SELECT cols | * FROM t [WHERE ...] ORDER BY c1 [ASC|DESC], ... LIMIT.
// Replaces operator/MSelectionOrderByOperator.java over query/selection/SelectionOperatorService.java (a PriorityQueue of
// offset + size docs per segment under CompositeDocIdValComparator).  The library returns every segment's best rows as
// (docId, dictIds); the caller merges the segments' lists by value, where MCombineOperator / SelectionOperatorService
// .mergeWithOrdering sit in the reference: dictIds of different segments do not compare.  With PGX_Q_SELECT_MV a
// multi-value schema column returns per row the dictIds of all the doc's values (pgx_select_mv_*, pgx_select.hip).
// Without ORDER BY (PGX_Q_SELECT_ONLY; operator/query/MSelectionOnlyOperator.java:58-110) a segment's rows are its first
// docs in docId order (pgx_select_first), the caller appends the segments' lists in call order, and the operator's early
// stop changes all four statistics: run_select's `only` branch.
// Reference paths are relative to pinot-core/src/main/java/com/linkedin/pinot/core/.
#include "pgx_host.h"

namespace pgxh {

// Data schema of a selection (SelectionOperatorUtils.extractDataSchema:223-253): the order columns in ORDER BY order,
// then the selected columns sorted by name, minus those already present; "*" is the segment's columns, sorted
// (getSelectionColumns:152-161).
static std::vector<std::string> select_schema(const pgx_query& q, const pgx_segment* seg0) {
  std::vector<std::string> cols = q.order_cols;
  std::vector<std::string> sel = q.sel_cols;
  if (sel.size() == 1 && sel[0] == "*") {
    sel.clear();
    if (seg0) sel = seg0->names;
  }
  std::sort(sel.begin(), sel.end());
  for (const auto& c : sel)
    if (std::find(cols.begin(), cols.end(), c) == cols.end()) cols.push_back(c);
  return cols;
}

// numEntriesScannedInFilter when MSelectionOnlyOperator stops pulling after P = offset + size docs
// (BReusableFilteredDocIdSetOperator.java:68-93 calls next() on the root P times, or until its end): what the filter's
// iterators had counted by then.  Closed forms exist for three classes of the physical tree:
//   'a'  no scan leaf: 0;
//   'b'  the whole filter is one scan leaf on a single-value column (SVScanDocIdIterator.next counts every row up to
//        and including each match): docId of the P-th match + 1, or the segment's raw docs when the scan reached its end;
//   'd'  a root AND whose children are all leaves, at least one of them sorted / bitmap (AndBlockDocIdSet.fastIterator
//        builds the answer, every scan child's applyAnd included, before the first next()): the full run's number.
// Any other tree (0) leaves scan iterators in a state that depends on where the pulling stopped: an AND of scans has
// counted the rows up to the last doc only, an OR's scan children each stand at their own next match.
static char select_only_class(const PNode& root, const pgx_query& q, const pgx_segment& seg) {
  if (!has_scan_leaf(root)) return 'a';
  if (root.op == PGX_F_LEAF) return seg.col(q.leaf_col[size_t(root.leaf)]).is_mv ? 0 : 'b';
  if (root.op != PGX_F_AND) return 0;
  bool index = false;
  for (const PNode& k : root.kids) {
    if (k.op != PGX_F_LEAF) return 0;
    index |= k.phys == PH_SORTED || k.phys == PH_BITMAP;
  }
  return index ? 'd' : 0;
}

static void leaf_kinds(const PNode& n, std::vector<int>& phys) {
  if (n.op == PGX_F_LEAF) phys[size_t(n.leaf)] = n.phys;
  for (const PNode& k : n.kids) leaf_kinds(k, phys);
}

// The class of a selection without ORDER BY over all segments of the call; refuses what has no closed form.  plan_query
// plans the filter with the first segment's index kinds: for class 'd', whose number is the full run's, every segment
// must agree with it leaf by leaf.
static char select_only_classify(const pgx_query& q, pgx_segment* const* segs, int n) {
  if (q.filter.empty()) return 'a';
  char cls = 0;
  std::vector<int> phys0;
  for (int s = 0; s < n; ++s) {
    const PNode root = build_tree(q, *segs[s]);
    const char c = select_only_class(root, q, *segs[s]);
    std::vector<int> phys(q.leaf_col.size(), PH_SCAN);
    leaf_kinds(root, phys);
    if (c == 0)
      fail(PGX_ERR_UNSUPPORTED,
           "selection without ORDER BY: numEntriesScannedInFilter of this filter depends on where the operator stops "
           "(closed forms: no scan leaf, one scan leaf, a root AND of leaves with a sorted / bitmap leaf)");
    if (s == 0) {
      cls = c;
      phys0 = phys;
    } else if (c != cls || (c == 'd' && phys != phys0)) {
      fail(PGX_ERR_UNSUPPORTED,
           "selection without ORDER BY: the segments' indexes put numEntriesScannedInFilter into different classes");
    }
  }
  return cls;
}

void run_select(pgx_ctx* ctx, const pgx_query& q, pgx_segment* const* segs, int n, const pgx_leaf_binding* bindings,
                const pgx_exec_opts* opts, pgx_result* R, hipStream_t st) {
  const uint32_t xflags = opts ? opts->flags : 0;
  if (opts && (opts->dense_out || (xflags & PGX_X_KEEP_DENSE_ON_DEVICE)))
    fail(PGX_ERR_UNSUPPORTED, "selection queries have no dense output");
  if (!q.kn.jit) fail(PGX_ERR_UNSUPPORTED, "selection queries need the query kernels");
  if (n < 0 || n > 65535) fail(PGX_ERR_UNSUPPORTED, "selection over more than 65535 segments");
  const int K = q.sel_offset + q.sel_size;
  const int no = int(q.order_cols.size());
  const bool only = no == 0;  // MSelectionOnlyOperator (pgx_select_compile took it with PGX_Q_SELECT_ONLY)
  const std::vector<std::string> schema = select_schema(q, n > 0 ? segs[0] : nullptr);
  const int nc = int(schema.size());

  // Multi-value columns only for a caller that reads them through pgx_result_select_mv_* (PGX_Q_SELECT_MV).  Among the
  // order columns one is a schema column like any other but no part of the key (CompositeDocIdValComparator.java:
  // 40-44 and SelectionOperatorService.getComparator skip it).
  const bool mv_ok = (q.flags & PGX_Q_SELECT_MV) != 0;

  // per-segment key layout; which schema columns are multi-value (every segment must agree)
  std::vector<SelItem> items(size_t(std::max(n, 0)));
  std::vector<int32_t> kinds(size_t(nc), 0);
  for (int s = 0; s < n; ++s) {
    SelItem& it = items[size_t(s)];
    it = SelItem{};
    it.num_docs = segs[s]->total_docs;
    int total_bits = 0, nk = 0;
    for (int c = 0; c < no; ++c) {
      const StagedColumn& col = segs[s]->col(q.order_cols[size_t(c)]);
      if (col.is_mv) {
        if (!mv_ok) fail(PGX_ERR_UNSUPPORTED, "ORDER BY multi-value column " + col.name);
        continue;
      }
      if (nk == kSelMaxOrderCols) fail(PGX_ERR_UNSUPPORTED, "more than 8 ORDER BY columns");
      SelCol& k = it.c[nk++];
      k.fwd = col.fwd;
      k.bits = col.bits;
      k.kbits = bits_for(col.card);
      k.card = uint32_t(std::max(col.card, 1));
      k.desc = q.order_asc[size_t(c)] ? 0 : 1;
      total_bits += k.kbits;
    }
    if (nk == 0 && !only) fail(PGX_ERR_UNSUPPORTED, "ORDER BY multi-value columns only");
    it.ncols = nk;
    if (total_bits > 64) fail(PGX_ERR_UNSUPPORTED, "selection order key wider than 64 bits");
    for (int c = 0; c < nc; ++c) {
      const StagedColumn& col = segs[s]->col(schema[size_t(c)]);
      if (col.is_mv && !mv_ok) fail(PGX_ERR_UNSUPPORTED, "selection of multi-value column " + col.name);
      if (s == 0) kinds[size_t(c)] = col.is_mv ? 1 : 0;
      else if (kinds[size_t(c)] != (col.is_mv ? 1 : 0))
        fail(PGX_ERR_UNSUPPORTED, "column " + col.name + " is multi-value in one segment and single-value in another");
    }
  }
  // column views: the single-value schema columns for pgx_select_gather (a multi-value column's fwd is a value stream,
  // not one entry per doc: it never goes there), the multi-value ones for pgx_select_mv_*
  std::vector<int> svi, mvi;
  for (int c = 0; c < nc; ++c) (kinds[size_t(c)] ? mvi : svi).push_back(c);
  const int nsv = int(svi.size()), nmv = int(mvi.size());
  std::vector<SelGatherCol> gcols(size_t(std::max(n, 0)) * size_t(nsv));
  std::vector<SelMvCol> mcols(size_t(std::max(n, 0)) * size_t(nmv));
  for (int s = 0; s < n; ++s) {
    for (int k = 0; k < nsv; ++k) {
      const StagedColumn& col = segs[s]->col(schema[size_t(svi[size_t(k)])]);
      gcols[size_t(s) * nsv + k] = SelGatherCol{col.fwd, col.bits, 0};
    }
    for (int m = 0; m < nmv; ++m) {
      const StagedColumn& col = segs[s]->col(schema[size_t(mvi[size_t(m)])]);
      mcols[size_t(m) * n + s] = SelMvCol{col.fwd, col.mv_start.as<const int32_t>(), col.bits, 0};
    }
  }

  R->select = true;
  R->group_by = false;
  R->num_aggs = 0;
  R->sel_schema = schema;
  R->sel_counts.assign(size_t(std::max(n, 0)), 0);
  R->sel_seg.clear();
  R->sel_doc.clear();
  R->sel_ids.clear();
  R->sel_kinds = kinds;
  R->sel_mv_off.assign(size_t(nc), {});
  R->sel_mv_val.assign(size_t(nc), {});
  for (int c : mvi) R->sel_mv_off[size_t(c)].assign(1, 0);
  if (n == 0) return;
  // without ORDER BY: which closed form the filter statistic takes, refused before anything is allocated; a request
  // without a filter selects every doc (a null mask), launches no query kernel and allocates no mask
  const char only_class = only ? select_only_classify(q, segs, n) : 0;
  const bool scan = !only || !q.filter.empty();

  // 1. the filter as COUNT(*): statistics and one selection bit per scanned row
  pgx_query qs = q;
  qs.select = false;
  qs.flags = (qs.flags & ~(PGX_Q_SELECT_MV | PGX_Q_SELECT_ONLY)) | PGX_Q_NO_STAR_TREE;  // every raw row gets its bit
  qs.agg_fn.assign(1, PGX_COUNT);
  qs.agg_col.assign(1, "");
  qs.group_cols.clear();
  qs.key_domain.clear();
  ExecPlan P;
  ExecBuffers B;
  int max_words = 0;
  if (scan) {
    P.want_selmask = true;
    plan_query(ctx, qs, segs, n, bindings, xflags, P);
    P.sel_off.assign(size_t(n), 0);
    int64_t words = 0;
    for (int s = 0; s < n; ++s) {
      P.sel_off[size_t(s)] = words;
      int w = (P.ksegs[size_t(s)].num_docs + 31) / 32 + 1;
      if (only) w = (w + 3) & ~3;  // pgx_select_first reads 16 bytes per thread: every segment's mask starts aligned
      words += w;
      max_words = std::max(max_words, w);
    }
    P.sel_buf = DevBuf(ctx, size_t(std::max<int64_t>(words, 1)) * 4);
    hip_check(hipMemsetAsync(P.sel_buf.p, 0, size_t(std::max<int64_t>(words, 1)) * 4, st), "selection masks");
    upload_plan(ctx, P, B, st);
    plan_jit(ctx, qs, segs, n, P, B);
    if (P.jit.empty()) {
      for (int s = 0; s < n; ++s)
        if (P.ksegs[size_t(s)].num_docs != 0) fail(PGX_ERR_UNSUPPORTED, "selection queries need the query kernels");
      R->stats[3] = P.total_raw;  // every segment empty: nothing scanned, no rows
      return;
    }
    alloc_outputs(ctx, P, B, nullptr, 0);
    reset_outputs(P, B, st);
    launch_scan(P, st);
  }

  // 2. per-segment top K and merge (without ORDER BY: the first K selected docs), gather -- on the same stream
  for (int s = 0; s < n; ++s) {
    items[size_t(s)].sel = scan ? P.sel_buf.as<uint32_t>() + P.sel_off[size_t(s)] : nullptr;
    items[size_t(s)].num_docs = scan ? P.ksegs[size_t(s)].num_docs : segs[s]->total_raw_docs;
  }
  // workgroups per segment: at least 4 steps of 256 mask words each, and no more over all segments than stay resident
  // (8 of 256 threads per CU, fewer when the candidate buffers fill the LDS): the scan hides its load latency with
  // resident waves, while every further workgroup adds a candidate list of K rows to the merge
  int cbuf = 1;
  while (cbuf < K) cbuf <<= 1;
  cbuf = std::max(512, 2 * cbuf) * 12;
  const int resident = std::max(1, std::min(8, (160 * 1024) / (cbuf + 512)));
  int G = std::max(1, (max_words + 4 * kSelBlock - 1) / (4 * kSelBlock));
  G = std::min(G, std::max(1, resident * ctx->num_cus / n));
  G = std::min(G, 64);
  if (only) {
    // workgroups per segment of pgx_select_first: at least 4 steps of 256 chunks of 4 mask words each, and no more
    // over all segments than stay resident (8 of 256 threads per CU).  PGX_DEBUG firstg=N sets the number (A/B runs).
    G = std::max(1, max_words / (4 * 4 * kSelBlock));
    G = std::min(G, std::max(1, 8 * ctx->num_cus / n));
    G = std::min(G, 64);
    if (q.kn.sel_first_g > 0) G = q.kn.sel_first_g;
  }
  const size_t slots = size_t(n) * size_t(G);
  const size_t rows = size_t(n) * size_t(K);
  const size_t nseg = size_t(n);
  DevBuf idev(ctx, items.size() * sizeof(SelItem)), gdev(ctx, std::max<size_t>(1, gcols.size()) * sizeof(SelGatherCol));
  DevBuf ckey, cdoc, ccnt(ctx, slots * 4);
  DevBuf odoc(ctx, rows * 4), ocnt(ctx, nseg * 4), oids(ctx, std::max<size_t>(1, rows * nsv) * 4);
  hip_check(hipMemcpyAsync(idev.p, items.data(), items.size() * sizeof(SelItem), hipMemcpyHostToDevice, st),
            "selection items H2D");
  if (!gcols.empty())
    hip_check(hipMemcpyAsync(gdev.p, gcols.data(), gcols.size() * sizeof(SelGatherCol), hipMemcpyHostToDevice, st),
              "selection columns H2D");
  // hfound: without ORDER BY, the docs found per segment among the first K = offset + size (the statistics read them);
  // the rows returned, and everything gathered for them, are the first `size` of those (olim)
  std::vector<int32_t> hfound;
  DevBuf olim;
  const int32_t* rcnt = ocnt.as<int32_t>();  // the row counts the gathers run over
  if (!only) {
    ckey = DevBuf(ctx, slots * K * 8);
    cdoc = DevBuf(ctx, slots * K * 4);
    PGX_LAUNCH(st, "pgx_select_topk",
               pgx_launch_select_topk(idev.as<SelItem>(), n, K, G, ckey.as<uint64_t>(), cdoc.as<uint32_t>(),
                                      ccnt.as<int32_t>(), st),
               "selection top-K");
    PGX_LAUNCH(st, "pgx_select_merge",
               pgx_launch_select_merge(n, K, G, ckey.as<uint64_t>(), cdoc.as<uint32_t>(), ccnt.as<int32_t>(),
                                       odoc.as<int32_t>(), ocnt.as<int32_t>(), st),
               "selection merge");
  } else {
    if (G > 1)
      PGX_LAUNCH(st, "pgx_select_first_count",
                 pgx_launch_select_first_count(idev.as<SelItem>(), n, K, G, ccnt.as<int32_t>(), st),
                 "selection first-K count");
    if (q.sel_offset > 0) {
      olim = DevBuf(ctx, nseg * 4);
      rcnt = olim.as<int32_t>();
    }
    PGX_LAUNCH(st, "pgx_select_first",
               pgx_launch_select_first(idev.as<SelItem>(), n, K, G, ccnt.as<int32_t>(), odoc.as<int32_t>(),
                                       ocnt.as<int32_t>(), q.sel_size, olim.as<int32_t>(), st),
               "selection first-K");
    hfound.assign(nseg, 0);
    hip_check(hipMemcpyAsync(hfound.data(), ocnt.p, nseg * 4, hipMemcpyDeviceToHost, st), "selection D2H");
  }
  PGX_LAUNCH(st, "pgx_select_gather",
             pgx_launch_select_gather(gdev.as<SelGatherCol>(), n, nsv, K, odoc.as<int32_t>(), rcnt, oids.as<int32_t>(),
                                      st),
             "selection gather");
  std::vector<int32_t> hdoc(rows), hcnt(nseg), hids(rows * nsv);
  hip_check(hipMemcpyAsync(hcnt.data(), rcnt, hcnt.size() * 4, hipMemcpyDeviceToHost, st), "selection D2H");
  hip_check(hipMemcpyAsync(hdoc.data(), odoc.p, hdoc.size() * 4, hipMemcpyDeviceToHost, st), "selection D2H");
  if (!hids.empty())
    hip_check(hipMemcpyAsync(hids.data(), oids.p, hids.size() * 4, hipMemcpyDeviceToHost, st), "selection D2H");

  // 2b. multi-value schema columns: per pair (column, segment) the rows' value offsets, the pairs' bases, the values.
  // The value buffer has the grand total's size, read back (8 bytes) between the second and the third launch: the
  // bound known beforehand, sum over pairs of min(K * max_mv, total_entries), is K times one long doc's length per
  // pair, and the total is needed on the host anyway before the values are copied.
  const size_t pairs = nseg * size_t(nmv);
  std::vector<int32_t> hrel(pairs * size_t(K + 1)), hval;
  std::vector<int64_t> hbase(pairs + 1, 0);
  DevBuf mdev, mrel, mtot, mbase, mval;
  if (nmv > 0) {
    mdev = DevBuf(ctx, pairs * sizeof(SelMvCol));
    mrel = DevBuf(ctx, hrel.size() * 4);
    mtot = DevBuf(ctx, pairs * 4);
    mbase = DevBuf(ctx, hbase.size() * 8);
    hip_check(hipMemcpyAsync(mdev.p, mcols.data(), pairs * sizeof(SelMvCol), hipMemcpyHostToDevice, st),
              "selection multi-value columns H2D");
    PGX_LAUNCH(st, "pgx_select_mv_offsets",
               pgx_launch_select_mv_offsets(mdev.as<SelMvCol>(), n, nmv, K, odoc.as<int32_t>(), rcnt,
                                            mrel.as<int32_t>(), mtot.as<int32_t>(), st),
               "selection multi-value offsets");
    PGX_LAUNCH(st, "pgx_select_mv_bases",
               pgx_launch_select_mv_bases(mtot.as<int32_t>(), int64_t(pairs), mbase.as<int64_t>(), st),
               "selection multi-value bases");
    hip_check(hipMemcpyAsync(hbase.data(), mbase.p, hbase.size() * 8, hipMemcpyDeviceToHost, st), "selection D2H");
    hip_check(hipMemcpyAsync(hrel.data(), mrel.p, hrel.size() * 4, hipMemcpyDeviceToHost, st), "selection D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    const int64_t grand = hbase[pairs];
    if (grand < 0) fail(PGX_ERR_INTERNAL, "selection value count out of range");
    if (grand > 0) {
      hval.assign(size_t(grand), 0);
      mval = DevBuf(ctx, size_t(grand) * 4);
      // workgroups per pair: one per 2048 values of an average pair (each loads the pair's K + 1 offsets first)
      const int wgs = int(std::min<int64_t>(64, std::max<int64_t>(1, (grand / int64_t(pairs) + 2047) / 2048)));
      PGX_LAUNCH(st, "pgx_select_mv_gather",
                 pgx_launch_select_mv_gather(mdev.as<SelMvCol>(), n, nmv, K, wgs, odoc.as<int32_t>(), rcnt,
                                             mrel.as<int32_t>(), mbase.as<int64_t>(), mval.as<int32_t>(), grand, st),
                 "selection multi-value gather");
      hip_check(hipMemcpyAsync(hval.data(), mval.p, hval.size() * 4, hipMemcpyDeviceToHost, st), "selection D2H");
    }
  }
  pgx_result Rs;
  if (scan) finish_result(ctx, qs, P, B, segs, n, st, &Rs, nullptr);  // waits for the stream
  else hip_check(hipStreamSynchronize(st), "sync");

  // 3. statistics as MSelectionOrderByOperator.getNextBlock reports them; rows compacted segment by segment
  int64_t total = 0;
  for (int s = 0; s < n; ++s) {
    if (hcnt[size_t(s)] < 0 || hcnt[size_t(s)] > K) fail(PGX_ERR_INTERNAL, "selection row count out of range");
    total += hcnt[size_t(s)];
  }
  if (!only) {
    R->stats[0] = Rs.stats[0];
    R->stats[1] = Rs.stats[1];
    R->stats[2] = Rs.stats[0] * nc;
    R->stats[3] = Rs.stats[3];
  } else {
    // MSelectionOnlyOperator.java:92-110: the docs it took, times the schema size, and the segment's raw docs; the
    // filter's entries by the class of select_only_class (a segment with fewer than K matches was pulled to its end:
    // the full run's number, which for a root scan leaf is the segment's raw docs)
    int64_t entries = 0, raw = 0;
    for (int s = 0; s < n; ++s) {
      const int32_t found = hfound[size_t(s)];
      if (found < hcnt[size_t(s)] || found > K) fail(PGX_ERR_INTERNAL, "selection row count out of range");
      const int64_t docs = items[size_t(s)].num_docs;
      raw += docs;
      if (only_class == 'b') entries += found == K ? int64_t(hdoc[size_t(s) * K + size_t(K) - 1]) + 1 : docs;
    }
    if (only_class == 'd') entries = Rs.stats[1];
    R->stats[0] = total;
    R->stats[1] = entries;
    R->stats[2] = total * nc;
    R->stats[3] = raw;
  }
  R->sel_counts = hcnt;
  R->sel_seg.reserve(size_t(total));
  R->sel_doc.reserve(size_t(total));
  R->sel_ids.assign(size_t(total) * nc, 0);
  int64_t at = 0;
  for (int s = 0; s < n; ++s)
    for (int r = 0; r < hcnt[size_t(s)]; ++r, ++at) {
      R->sel_seg.push_back(s);
      R->sel_doc.push_back(hdoc[size_t(s) * K + r]);
      for (int k = 0; k < nsv; ++k)
        R->sel_ids[size_t(svi[size_t(k)]) * size_t(total) + size_t(at)] = hids[(size_t(k) * n + s) * K + r];
    }
  // a multi-value column's pairs lie back to back in segment order, as its rows do: its values are one stretch of the
  // value buffer, and a row's offsets are its pair's shifted by the pair's base inside the column
  for (int m = 0; m < nmv; ++m) {
    const size_t c = size_t(mvi[size_t(m)]), p0 = size_t(m) * nseg;
    std::vector<int64_t>& off = R->sel_mv_off[c];
    off.assign(size_t(total) + 1, 0);
    const int64_t first = hbase[p0], last = hbase[p0 + nseg];
    if (first < 0 || last < first || last > int64_t(hval.size()))
      fail(PGX_ERR_INTERNAL, "selection value offsets out of range");
    at = 0;
    for (int s = 0; s < n; ++s) {
      const int32_t* rel = &hrel[(p0 + size_t(s)) * size_t(K + 1)];
      const int64_t base = hbase[p0 + size_t(s)] - first;
      for (int r = 0; r < hcnt[size_t(s)]; ++r, ++at) {
        off[size_t(at)] = base + rel[r];
        R->sel_ids[c * size_t(total) + size_t(at)] = rel[r + 1] - rel[r];
      }
    }
    off[size_t(total)] = last - first;
    R->sel_mv_val[c].assign(hval.begin() + first, hval.begin() + last);
  }
}

}  // namespace pgxh

extern "C" {

pgx_status pgx_select_compile(pgx_ctx* ctx, const pgx_select_desc* d, pgx_query** out) {
  return guarded([&] {
    if (!ctx || !d || !out) fail(PGX_ERR_INVALID_ARG, "NULL argument");
    if (d->num_columns < 1 || !d->columns) fail(PGX_ERR_INVALID_ARG, "selection without columns");
    if (d->num_order_by < 0 || d->offset < 0 || d->size < 0) fail(PGX_ERR_INVALID_ARG, "negative count");
    const bool only = d->num_order_by == 0 && (d->flags & PGX_Q_SELECT_ONLY);
    if (d->num_order_by == 0 && !only) fail(PGX_ERR_UNSUPPORTED, "selection without ORDER BY (MSelectionOnlyOperator)");
    // (with PGX_Q_SELECT_MV the limit counts the single-value order columns only: run_select knows which they are)
    if (d->num_order_by > kSelMaxOrderCols && !(d->flags & PGX_Q_SELECT_MV))
      fail(PGX_ERR_UNSUPPORTED, "more than 8 ORDER BY columns");
    if (!d->order_by && !only) fail(PGX_ERR_INVALID_ARG, "NULL argument");
    const int64_t rows = int64_t(d->offset) + d->size;
    if (rows == 0) fail(PGX_ERR_UNSUPPORTED, "selection of 0 rows (LIMIT 0)");
    // (without ORDER BY the offset plays no part in what is returned: MSelectionOnlyOperator's _limitDocs = size)
    if (only && d->size == 0) fail(PGX_ERR_UNSUPPORTED, "selection of 0 rows (LIMIT 0)");
    if (rows > PGX_SEL_MAX_ROWS) fail(PGX_ERR_UNSUPPORTED, "selection of more than PGX_SEL_MAX_ROWS rows");
    auto q = std::make_unique<pgx_query>();
    q->select = true;
    for (int c = 0; c < d->num_columns; ++c) {
      if (!d->columns[c] || !*d->columns[c]) fail(PGX_ERR_INVALID_ARG, "empty column name");
      q->sel_cols.push_back(d->columns[c]);
    }
    for (int c = 0; c < d->num_order_by; ++c) {
      if (!d->order_by[c].column || !*d->order_by[c].column) fail(PGX_ERR_INVALID_ARG, "empty column name");
      q->order_cols.push_back(d->order_by[c].column);
      q->order_asc.push_back(d->order_by[c].ascending != 0);
    }
    q->sel_offset = d->offset;
    q->sel_size = d->size;
    q->filter.assign(d->filter, d->filter + d->num_filter_nodes);
    for (int l = 0; l < d->num_leaves; ++l) {
      q->leaf_col.push_back(d->leaves[l].column);
      q->leaf_kind.push_back(d->leaves[l].kind);
    }
    q->agg_fn.assign(1, PGX_COUNT);  // what the filter runs as (run_select); never reported
    q->agg_col.assign(1, "");
    q->flags = d->flags | PGX_Q_NO_STAR_TREE;
    q->kn = read_knobs();
    *out = q.release();
  });
}

static const pgx_result& select_result(const pgx_result* r) {
  if (r) r->ready();
  if (!r || !r->select) fail(PGX_ERR_INVALID_ARG, "not a selection result");
  return *r;
}

pgx_status pgx_result_select_schema(const pgx_result* r, int32_t* num_columns, const char** names) {
  return guarded([&] {
    const pgx_result& S = select_result(r);
    if (num_columns) *num_columns = int32_t(S.sel_schema.size());
    if (names)
      for (size_t c = 0; c < S.sel_schema.size(); ++c) names[c] = S.sel_schema[c].c_str();  // owned by the result
  });
}

pgx_status pgx_result_select_counts(const pgx_result* r, int32_t* rows_per_segment) {
  return guarded([&] {
    const pgx_result& S = select_result(r);
    if (!rows_per_segment) fail(PGX_ERR_INVALID_ARG, "NULL argument");
    std::copy(S.sel_counts.begin(), S.sel_counts.end(), rows_per_segment);
  });
}

pgx_status pgx_result_select_rows(const pgx_result* r, int32_t* seg_index, int32_t* doc_id, int32_t* dict_ids) {
  return guarded([&] {
    const pgx_result& S = select_result(r);
    if (seg_index) std::copy(S.sel_seg.begin(), S.sel_seg.end(), seg_index);
    if (doc_id) std::copy(S.sel_doc.begin(), S.sel_doc.end(), doc_id);
    if (dict_ids) std::copy(S.sel_ids.begin(), S.sel_ids.end(), dict_ids);
  });
}

pgx_status pgx_result_select_kinds(const pgx_result* r, int32_t* is_mv) {
  return guarded([&] {
    const pgx_result& S = select_result(r);
    if (!is_mv) fail(PGX_ERR_INVALID_ARG, "NULL argument");
    std::copy(S.sel_kinds.begin(), S.sel_kinds.end(), is_mv);
  });
}

static size_t select_mv_column(const pgx_result& S, int32_t column) {
  if (column < 0 || size_t(column) >= S.sel_kinds.size() || !S.sel_kinds[size_t(column)])
    fail(PGX_ERR_INVALID_ARG, "not a multi-value schema column");
  return size_t(column);
}

pgx_status pgx_result_select_mv_offsets(const pgx_result* r, int32_t column, int64_t* offsets) {
  return guarded([&] {
    const pgx_result& S = select_result(r);
    const auto& off = S.sel_mv_off[select_mv_column(S, column)];
    if (!offsets) fail(PGX_ERR_INVALID_ARG, "NULL argument");
    std::copy(off.begin(), off.end(), offsets);
  });
}

pgx_status pgx_result_select_mv_values(const pgx_result* r, int32_t column, int32_t* dict_ids) {
  return guarded([&] {
    const pgx_result& S = select_result(r);
    const auto& val = S.sel_mv_val[select_mv_column(S, column)];
    if (dict_ids) std::copy(val.begin(), val.end(), dict_ids);
  });
}

}  // extern "C"
