/*
 * pgx.h -- C ABI of the MI355X-native pinot-core segment query path (libpgx.so).
 *
 * This is the drop-in boundary a JNI shim binds.  It replaces, for immutable
 * v1 segments and COUNT/SUM/MIN/MAX/AVG aggregation or group-by queries, the per-segment operator
 * tree the reference builds behind its plan-maker API and the in-JVM combine of the per-segment
 * results.  Reference interfaces replaced (pinot-core/src/main/java/com/linkedin/pinot/core/...):
 *
 *   pgx_segment_stage   <- segment/index/loader/Loaders.java:44-118 (Loaders.IndexSegment.load) +
 *                          segment/index/column/ColumnIndexContainer.java:45-139 (reader per column kind)
 *   pgx_execute         <- plan/maker/InstancePlanMakerImplV2.java:72-109 (makeInnerSegmentPlan /
 *                          makeInterSegmentPlan) -> plan/CombinePlanNode.java:66-124 ->
 *                          operator/MCombineOperator.java:84-199, operator/MCombineGroupByOperator.java:139-233
 *                          over per-segment operator/aggregation/AggregationOperator.java:77-104 and
 *                          operator/aggregation/groupby/AggregationGroupByOperator.java:81-106
 *   pgx_result_*        <- operator/blocks/IntermediateResultsBlock.java:65-233 (aggregation result list,
 *                          AggregationGroupByResult.getResultForKey, ExecutionStatistics)
 *   pgx_leaf_binding    <- operator/filter/predicate/PredicateEvaluator.getMatchingDictionaryIds (the caller's
 *                          PredicateEvaluatorProvider resolves each predicate to dictId space per segment)
 *   pgx_select_compile, <- plan/SelectionPlanNode.java -> operator/MSelectionOrderByOperator.java:59-124 over
 *   pgx_result_select_*    query/selection/SelectionOperatorService.java (the per-segment PriorityQueue of offset + size
 *                          docs under CompositeDocIdValComparator, iterator/DocIdIntValComparator) and
 *                          query/selection/SelectionOperatorUtils.java:223-253 (extractDataSchema)
 *
 * Conventions: every call returns pgx_status (0 = OK); no C++ exception crosses the ABI; on error
 * pgx_last_error() returns a thread-local message.  Plain pointers and sizes only.  A pgx_ctx is
 * bound to one device and is thread-safe; staged segments are immutable and may be shared by
 * concurrent queries.  Host buffers passed in are only read during the call.
 */
#ifndef PGX_H_
#define PGX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGX_ABI_VERSION 8  /* 7: pgx_mutable_* (realtime segments in place); 8: pgx_result_record_words, records of
                              * every device-resident layout (several value columns, f64 sums); pgx_select_compile and
                              * pgx_result_select_* were added under 8: new entry points only, no existing struct or
                              * call changed; likewise PGX_DISTINCTCOUNTHLL[MV], pgx_result_hll and pgx_hll_codes, and
                              * PGX_DISTINCTCOUNT[MV], pgx_result_distinct[_counts] and pgx_java_hash_codes, and
                              * PGX_PERCENTILE[MV], pgx_result_percentile[_counts] and pgx_histogram_percentile, and
                              * PGX_FASTHLL and pgx_fasthll_registers */

typedef enum {
  PGX_OK = 0,
  PGX_ERR_INVALID_ARG = 1,
  PGX_ERR_UNSUPPORTED = 2, /* caller falls back to the Java operators */
  PGX_ERR_OOM = 3,
  PGX_ERR_DEVICE = 4,
  PGX_ERR_TIMEOUT = 5,
  PGX_ERR_INTERNAL = 6
} pgx_status;

typedef enum { PGX_INT = 0, PGX_LONG = 1, PGX_FLOAT = 2, PGX_DOUBLE = 3, PGX_STRING = 4 } pgx_data_type;

/* The *MV functions aggregate every value of a multi-value column in the selected docs
 * (operator/aggregation/function/{Count,Sum,Min,Max,Avg}MVAggregationFunction.java); aggregation-only queries. */
/* PGX_DISTINCTCOUNTHLL (operator/aggregation/function/DistinctCountHLLAggregationFunction.java): a single-value
 * column of any of the five data types; its intermediate is 256 HyperLogLog registers per result (per group), read
 * with pgx_result_hll (below, "DISTINCTCOUNTHLL").  PGX_DISTINCTCOUNTHLLMV (DistinctCountHLLMVAggregationFunction.java)
 * is the same over every value of a multi-value column in the selected docs.
 * PGX_DISTINCTCOUNT (DistinctCountAggregationFunction.java) and PGX_DISTINCTCOUNTMV (DistinctCountMVAggregationFunction
 * .java) are the exact forms: the intermediate is the set of those hash codes, read with pgx_result_distinct_counts and
 * pgx_result_distinct (below, "DISTINCTCOUNT").
 * PGX_PERCENTILE (PercentileAggregationFunction.java) and PGX_PERCENTILEMV (PercentileMVAggregationFunction.java): the
 * intermediate is the multiset of the selected values, held as (value, count) pairs and read with
 * pgx_result_percentile_counts and pgx_result_percentile (below, "PERCENTILE").  The multi-value form has the lower
 * code on purpose: code 14 on a single-value column is refused at compile time.
 * PGX_FASTHLL (FastHllAggregationFunction.java): a single-value STRING column of serialized HyperLogLogs; the
 * intermediate is the 256 registers of their union, read with pgx_result_hll (below, "FASTHLL"). */
typedef enum { PGX_COUNT = 0, PGX_SUM = 1, PGX_MIN = 2, PGX_MAX = 3, PGX_AVG = 4,
               PGX_COUNTMV = 5, PGX_SUMMV = 6, PGX_MINMV = 7, PGX_MAXMV = 8, PGX_AVGMV = 9,
               PGX_DISTINCTCOUNTHLL = 10, PGX_DISTINCTCOUNTHLLMV = 11,
               PGX_DISTINCTCOUNT = 12, PGX_DISTINCTCOUNTMV = 13,
               PGX_PERCENTILEMV = 14, PGX_PERCENTILE = 15, PGX_FASTHLL = 16 } pgx_agg_fn;

/* Predicate kinds (common/Predicate.java Type); they select the physical filter operator exactly as
 * plan/FilterPlanNode.java:118-132 does and drive the numEntriesScannedInFilter statistic. */
typedef enum { PGX_PRED_EQ = 0, PGX_PRED_NEQ = 1, PGX_PRED_IN = 2, PGX_PRED_NOT_IN = 3, PGX_PRED_RANGE = 4 } pgx_pred_kind;

typedef enum { PGX_F_LEAF = 0, PGX_F_AND = 1, PGX_F_OR = 2 } pgx_filter_op;

typedef enum { PGX_MEM_HOST = 0, PGX_MEM_DEVICE = 1 } pgx_mem_kind;

typedef struct pgx_ctx pgx_ctx;
typedef struct pgx_segment pgx_segment;
typedef struct pgx_query pgx_query;
typedef struct pgx_result pgx_result;

typedef struct {
  int32_t device;          /* HIP device ordinal */
  uint32_t flags;          /* reserved, 0 */
} pgx_ctx_opts;

/* ---- context -------------------------------------------------------------------------------- */
pgx_status pgx_ctx_create(const pgx_ctx_opts* opts, pgx_ctx** out);
pgx_status pgx_ctx_destroy(pgx_ctx* ctx);
const char* pgx_last_error(void);
int32_t pgx_abi_version(void);

/* ---- segments (staging into HBM) ---------------------------------------------------------------
 * Buffers are the VERBATIM v1 file bytes (big-endian), see DESIGN.md "Data layout in HBM".
 * mem == PGX_MEM_DEVICE means fwd/dict/... already live in HBM on the context's device (e.g. produced
 * by pgx_synth_column); the library then references them without copying and the caller keeps them
 * alive until pgx_segment_release. */
typedef struct {
  const char* name;
  int32_t data_type;          /* pgx_data_type */
  int32_t cardinality;
  int32_t bits_per_element;   /* from metadata.properties, never recomputed */
  int32_t is_sorted;
  int32_t dict_width;         /* bytes per dictionary entry (lengthOfEachEntry for STRING) */
  const void* fwd;            /* <col>.sv.unsorted.fwd, ceil(total_docs*bits/8) bytes (NULL if sorted) */
  uint64_t fwd_len;
  const void* sorted_pairs;   /* <col>.sv.sorted.fwd, card x (int32 BE start, int32 BE end) (NULL if unsorted) */
  uint64_t sorted_len;
  const void* dict;           /* <col>.dict */
  uint64_t dict_len;
  const void* inv;            /* <col>.bitmap.inv (optional, host memory) */
  uint64_t inv_len;
  int32_t pad_char;           /* STRING padding byte: metadata "segment.padding.character" ('\0'), '%' when the key
                                 is absent (legacy segments, ColumnMetadata.java:93-98); StringDictionary.get cuts at
                                 its first occurrence (StringDictionary.java:53-66) */
  int32_t is_multi_value;     /* 1: fwd holds <col>.mv.fwd (io/writer/impl/v1/FixedBitMultiValueWriter.java: chunk
                                 offsets, doc-start bitset, fixed-bit values; ColumnIndexContainer.java:78) */
  int32_t total_entries;      /* metadata totalNumberOfEntries (multi-value columns) */
} pgx_column_desc;

typedef struct {
  const char* name;
  int32_t total_docs;
  int32_t total_raw_docs;
  int32_t num_columns;
  const pgx_column_desc* columns;
  const void* star_tree;      /* star-tree.bin in OFF_HEAP format (optional, host memory) */
  uint64_t star_tree_len;
  int32_t mem;                /* pgx_mem_kind of fwd/sorted_pairs/dict */
  int32_t num_star_skip_dims; /* metadata "star.tree.skip.materialization.for.dimensions": dimensions the star tree */
  const char* const* star_skip_dims;  /* does not materialise (RequestUtils.isFitForStarTreeIndex:149-163) */
} pgx_segment_desc;

pgx_status pgx_segment_stage(pgx_ctx* ctx, const pgx_segment_desc* desc, pgx_segment** out);
pgx_status pgx_segment_release(pgx_segment* seg);
/* HBM bytes held by the staged segment (forward indexes + dictionaries + inverted indexes). */
pgx_status pgx_segment_device_bytes(const pgx_segment* seg, uint64_t* out);

/* ---- realtime (consuming) segments, in place -----------------------------------------------------
 * RealtimeSegmentImpl.index (core/realtime/impl/RealtimeSegmentImpl.java:185-334) gives every column value an
 * arrival-order dictId in a mutable dictionary and appends one dictId per doc (a list per doc for multi-value columns).
 * A pgx_mutable keeps those dictIds in HBM: pgx_mutable_append sends only the new docs' ids.  The caller owns the
 * mutable dictionaries; whenever one grew it hands the column's current dictionary SORTED (v1 bytes, as
 * RealtimeSegmentConverter would write it) with the arrival -> sorted id map (pgx_mutable_set_dictionary, O(card)).
 * pgx_mutable_snapshot returns the docs indexed so far as a queryable pgx_segment: the forward indexes are re-packed
 * on the device through the maps (no row crosses PCIe again), unsorted (RealtimeColumnDataSource.isSorted() is false),
 * and columns with has_inverted keep bitmap-filter semantics (FilterPlanNode, numEntriesScannedInFilter) evaluated by
 * scanning the dictIds.  Release snapshots with pgx_segment_release; they stay valid after more appends. */
typedef struct pgx_mutable pgx_mutable;
typedef struct {
  const char* name;
  int32_t data_type;          /* pgx_data_type (multi-value: numeric only) */
  int32_t is_multi_value;
  int32_t has_inverted;       /* in the table's invertedIndexColumns */
} pgx_mutable_column;
pgx_status pgx_mutable_create(pgx_ctx* ctx, const char* name, int32_t capacity, int32_t num_columns,
                              const pgx_mutable_column* columns, pgx_mutable** out);
/* ndocs new docs.  ids[c]: column c's arrival-order dictIds, one per doc, or (multi-value) every value of the new docs
 * in doc order with counts[c][d] values for doc d (>= 1).  counts may be NULL when no column is multi-value. */
pgx_status pgx_mutable_append(pgx_mutable* m, int32_t ndocs, const int32_t* const* ids, const int32_t* const* counts);
pgx_status pgx_mutable_set_dictionary(pgx_mutable* m, int32_t column, int32_t cardinality, const void* dict,
                                      uint64_t dict_len, int32_t dict_width, int32_t pad_char,
                                      const int32_t* arrival_to_sorted);
pgx_status pgx_mutable_snapshot(pgx_mutable* m, pgx_segment** out);
pgx_status pgx_mutable_num_docs(const pgx_mutable* m, int32_t* out);
pgx_status pgx_mutable_release(pgx_mutable* m);

/* ---- query ---------------------------------------------------------------------------------- */
typedef struct {
  int32_t fn;                 /* pgx_agg_fn */
  const char* column;         /* NULL or "*" for COUNT(*) */
} pgx_agg;

/* Filter tree in postfix order.  LEAF: arg = leaf index.  AND / OR: arg = number of children popped. */
typedef struct {
  int32_t op;                 /* pgx_filter_op */
  int32_t arg;
} pgx_filter_node;

typedef struct {
  const char* column;
  int32_t kind;               /* pgx_pred_kind */
} pgx_leaf;

typedef struct {
  int32_t num_aggs;
  const pgx_agg* aggs;
  int32_t num_group_cols;     /* 0 => aggregation-only query */
  const char* const* group_cols;
  int32_t top_n;              /* GROUP BY ... TOP n (reference default 10) */
  int32_t num_filter_nodes;   /* 0 => MatchEntireSegment */
  const pgx_filter_node* filter;
  int32_t num_leaves;
  const pgx_leaf* leaves;
  uint32_t flags;             /* PGX_Q_* */
} pgx_query_desc;

#define PGX_Q_NO_STAR_TREE 0x1u /* debug option useStarTree=false (common/utils/request/RequestUtils.java:229-236) */

pgx_status pgx_query_compile(pgx_ctx* ctx, const pgx_query_desc* desc, pgx_query** out);
/* Cross-process key identity (SURVEY 8e "a host-side global dictionary per group-by column"; ABI 5): the key space of
 * group-by column group_col becomes the caller's sorted distinct values (type PGX_INT / PGX_LONG -> ivals, PGX_FLOAT /
 * PGX_DOUBLE -> dvals, PGX_STRING -> svals, compared bytewise) instead of the union of the executed segments'
 * dictionaries.  Processes that set the same domains plan the same dense slots / packed keys, so their partials merge
 * by slot (RCCL all-reduce) or by packed key (all-to-all + pgx_result_merge_groups) -- the value-keyed merge of
 * MCombineGroupByOperator.java:166-191 without shipping strings.  Results of such a query report seg_index -1 and
 * dict_id = the index into the domain for that column (pgx_result_group_keys / pgx_result_gather).  Every segment value
 * must be in the domain (PGX_ERR_INVALID_ARG otherwise).  num_values 0 clears it. */
pgx_status pgx_query_set_key_domain(pgx_query* q, int32_t group_col, int32_t type, int64_t num_values,
                                    const int64_t* ivals, const double* dvals, const char* const* svals);
pgx_status pgx_query_release(pgx_query* q);

/* ---- selection with ORDER BY --------------------------------------------------------------------
 * SELECT cols | * FROM t [WHERE ...] ORDER BY c1 [ASC|DESC], ... LIMIT [offset,] size.  The resulting pgx_query works
 * with pgx_bind_predicates, pgx_execute, pgx_execute_async, pgx_result_stats, pgx_result_wait and pgx_query_release.
 * Per segment the rows rank by (order key, docId) ascending: the key is the order columns' dictIds (v1 dictionaries are
 * sorted; DESC takes cardinality - 1 - dictId), max(1, ceil(log2 cardinality)) bits each, most significant first; the
 * docId as last component makes the result unique (the reference's choice among ties at the boundary follows
 * java.util.PriorityQueue's heap order).  PGX_ERR_UNSUPPORTED (the caller falls back to the Java operators): no ORDER
 * BY (MSelectionOnlyOperator), more than 8 order columns, a key wider than 64 bits, offset + size of 0 or above
 * PGX_SEL_MAX_ROWS, a multi-value column among the order or selected columns, pgx_execute_multi, key domains, dense
 * outputs, pgx_execute_timed.  Selection runs never use a star tree (every raw row is ranked).  The data schema is
 * that of SelectionOperatorUtils.extractDataSchema: the order columns in ORDER BY order, then the selected columns
 * sorted by name, minus those already present; "*" is the first segment's columns.
 * Multi-value columns: only with PGX_Q_SELECT_MV in flags, by which the caller declares that it reads them through
 * pgx_result_select_kinds / _mv_offsets / _mv_values (pgx_result_select_rows has one int per column and row; without the
 * flag every status and message is as above).  With it a multi-value column may be among the selected columns, also
 * through "*" (SelectionFetcher's *ArraySelectionColumnIterator; the reference types it <TYPE>_ARRAY), and among the
 * ORDER BY columns: there it is a schema column like any order column but no part of the key, per segment or in the
 * caller's merge (CompositeDocIdValComparator.java:40-44, SelectionOperatorService.getComparator).  The limits of 8
 * order columns and 64 key bits then count the single-value order columns only, and one of them must remain:
 * PGX_ERR_UNSUPPORTED "ORDER BY multi-value columns only" otherwise (the reference returns whatever its heap leaves).
 * A column that is multi-value in one segment of the call and single-value in another: PGX_ERR_UNSUPPORTED.
 * Without ORDER BY (plan/SelectionPlanNode.java:42-47 -> operator/query/MSelectionOnlyOperator.java:58-110): only with
 * PGX_Q_SELECT_ONLY in flags, by which the caller declares that it merges the segments' lists in call order
 * (SelectionOperatorUtils.mergeWithoutOrdering) and applies no offset (renderSelectionResultsWithoutOrdering); without
 * the flag every status and message is as above, and with the flag and num_order_by >= 1 the query is the ORDER BY
 * query as before.  With it and num_order_by == 0 the result holds per segment its first min(matches, size) docs in
 * ascending docId (the offset plays no part in what is returned: _limitDocs = size); the schema is the selected columns
 * sorted by name.  Limits: size >= 1, offset + size <= PGX_SEL_MAX_ROWS (the doc-id operator hands out blocks of
 * offset + size docs, and the statistics below depend on that block), multi-value selected columns only together with
 * PGX_Q_SELECT_MV; pgx_execute_multi, key domains, dense outputs and pgx_execute_timed are refused as for ORDER BY.
 * pgx_result_stats, summed over the segments, with c = min(matches, size) per segment: numDocsScanned = c,
 * numEntriesScannedPostFilter = c x schema size, numTotalRawDocs = the segment's raw docs, and
 * numEntriesScannedInFilter = what the filter's iterators had counted when the operator stopped pulling, after
 * P = offset + size calls of next() on the root (BReusableFilteredDocIdSetOperator.java:68-93) or at its end.  That
 * number is computed for three classes of filter:
 *   (a) no scan leaf (no filter, or sorted / bitmap leaves only): 0;
 *   (b) the whole filter is one scan leaf on a single-value column: docId of the P-th match + 1 in a segment with at
 *       least P matches, the segment's raw docs otherwise (the scan ran to its end);
 *   (d) a root AND whose children are all leaves, at least one of them sorted / bitmap: the full run's number, whatever
 *       P (AndBlockDocIdSet.fastIterator builds its answer before the first next()).
 * Every other filter (an AND of scan leaves only, any OR with a scan leaf, nested operators over a scan leaf) leaves
 * its scan iterators in a state that depends on where the pulling stopped: PGX_ERR_UNSUPPORTED at execution, with
 * "numEntriesScannedInFilter" in the message, also when the segments of one call fall into different classes. */
#define PGX_SEL_MAX_ROWS 2048
#define PGX_Q_SELECT_MV 0x2u /* pgx_select_desc.flags: the caller reads multi-value columns (pgx_result_select_mv_*) */
#define PGX_Q_SELECT_ONLY 0x4u /* pgx_select_desc.flags: num_order_by == 0 is accepted (MSelectionOnlyOperator) */
typedef struct {
  const char* column;
  int32_t ascending;
} pgx_order_by;
typedef struct {
  int32_t num_columns;
  const char* const* columns; /* as written; a single "*" = all columns */
  int32_t num_order_by;       /* >= 1; 0 with PGX_Q_SELECT_ONLY */
  const pgx_order_by* order_by;
  int32_t offset, size;       /* LIMIT offset, size */
  int32_t num_filter_nodes;
  const pgx_filter_node* filter;
  int32_t num_leaves;
  const pgx_leaf* leaves;
  uint32_t flags;             /* PGX_Q_* */
} pgx_select_desc;
pgx_status pgx_select_compile(pgx_ctx* ctx, const pgx_select_desc* desc, pgx_query** out);
/* Selection results: per segment its best <= offset + size rows, best first; the caller merges the segments' lists by
 * value (MCombineOperator -> SelectionOperatorService.mergeWithOrdering in the reference: dictIds of different segments
 * do not compare).  Without ORDER BY (PGX_Q_SELECT_ONLY): per segment its first <= size rows in ascending docId; the
 * caller appends the segments' lists in call order up to size rows.  They return PGX_ERR_INVALID_ARG on an aggregation or group-by result, as pgx_result_agg and the
 * group accessors do on a selection result.
 * schema: *num_columns, and names[c] (may be NULL; the strings live as long as the result).
 * counts: rows_per_segment[n].  rows: the segments' rows back to back (total = sum of the counts): seg_index[row],
 * doc_id[row], dict_ids[c * total + row] for schema column c (a multi-value column: the row's value count).  Any output
 * may be NULL.
 * kinds: is_mv[c] per schema column, 1 for a multi-value column (PGX_Q_SELECT_MV), else 0.
 * mv_offsets / mv_values, for a multi-value schema column (PGX_ERR_INVALID_ARG for a single-value one): over the same
 * row order as rows, offsets[total + 1]: row j owns values [offsets[j], offsets[j + 1]) of dict_ids[offsets[total]],
 * the values' dictIds in the doc's own value order (as FixedBitMultiValueReader yields them).  numEntriesScannedPostFilter
 * stays numDocsScanned x schema size (MSelectionOrderByOperator.java:103). */
pgx_status pgx_result_select_schema(const pgx_result* r, int32_t* num_columns, const char** names);
pgx_status pgx_result_select_counts(const pgx_result* r, int32_t* rows_per_segment);
pgx_status pgx_result_select_rows(const pgx_result* r, int32_t* seg_index, int32_t* doc_id, int32_t* dict_ids);
pgx_status pgx_result_select_kinds(const pgx_result* r, int32_t* is_mv);
pgx_status pgx_result_select_mv_offsets(const pgx_result* r, int32_t column, int64_t* offsets);
pgx_status pgx_result_select_mv_values(const pgx_result* r, int32_t column, int32_t* dict_ids);

/* Per-(segment, leaf) predicate in dictionary-id space, as produced by the caller's PredicateEvaluator:
 * a doc matches iff its dictId d satisfies  (words ? bit d of words : lo <= d <= hi).
 * For NEQ / NOT_IN the binding describes the MATCHING ids (the complement); the library derives the
 * non-matching list for bitmap exclusion itself.  words has ceil(card/32) little-endian uint32. */
typedef struct {
  int32_t lo;
  int32_t hi;
  const uint32_t* words;      /* host memory, optional */
} pgx_leaf_binding;

/* a-4 inside the library: resolve each leaf's raw predicate values against every segment's dictionary, as
 * PredicateEvaluatorProvider (operator/filter/predicate/PredicateEvaluatorProvider.java:31-54) and the Equals /
 * NotEquals / In / NotIn / RangeOffline evaluators do per segment; Dictionary.indexOf parses the value with the column's
 * type (Integer.parseInt, Long.parseLong, Float.parseFloat, Double.parseDouble; STRING padded with the padding char,
 * StringDictionary.java:37-51).  Segments whose dictionaries are byte-identical share one resolution. */
typedef struct {
  int32_t num_values;         /* EQ / NEQ 1, IN / NOT_IN n, RANGE 2 (lower, upper; "*" = unbounded) */
  const char* const* values;
  int32_t lower_inclusive;    /* RANGE only (RangePredicate.java:31-57) */
  int32_t upper_inclusive;
} pgx_predicate;

typedef struct pgx_bindings pgx_bindings;
/* preds[num_leaves] in the query's leaf order; the result holds bindings[n][num_leaves] for pgx_execute. */
pgx_status pgx_bind_predicates(const pgx_query* q, pgx_segment* const* segs, int32_t n, const pgx_predicate* preds,
                               pgx_bindings** out);
const pgx_leaf_binding* pgx_bindings_array(const pgx_bindings* b);
pgx_status pgx_bindings_release(pgx_bindings* b);

typedef struct {
  uint64_t stream;            /* hipStream_t (0 = the context's own stream) */
  void* dense_out;            /* optional device buffer for the dense group table (multi-GPU merge) */
  uint64_t dense_out_bytes;
  uint32_t flags;             /* PGX_X_* */
} pgx_exec_opts;

#define PGX_X_KEEP_DENSE_ON_DEVICE 0x1u /* leave the dense table in dense_out; do not compact to host */
#define PGX_X_FORCE_HASH 0x2u           /* testing: use the hash group-by path even for small key spaces */
#define PGX_X_NO_PARTITION 0x4u         /* testing: sparse group-by through the global hash table, not the partitioned
                                           record path (pgx_part.cpp run_partitioned) */
#define PGX_X_THROUGHPUT 0x8u           /* the caller keeps several queries in flight (pgx_execute_async): plan every
                                           segment into one launch per kernel instead of the batched pipeline, whose
                                           early start only shortens a lone query's latency (ABI 6) */
#define PGX_X_SPARSE_GROUP_SETS 0x10u    /* PGX_DISTINCTCOUNTHLL[MV], PGX_DISTINCTCOUNT[MV] and PGX_PERCENTILE[MV] under
                                           GROUP BY over a key space that is not dense, is partitioned or has more than
                                           PGX_HLL_MAX_GROUP_SLOTS slots: their tables get one row per group of the
                                           result (see PGX_SET_MAX_SPARSE_GROUPS below).  Opt-in: on this route a
                                           table-size refusal can only come after the scan has run.  Dense key spaces
                                           of up to PGX_HLL_MAX_GROUP_SLOTS slots run as without the flag. */

/* Execute the query over n segments on the context's device and merge the per-segment partials
 * (the combine).  bindings is [n][num_leaves].  Synchronous w.r.t. the returned result. */
pgx_status pgx_execute(pgx_ctx* ctx, const pgx_query* q, pgx_segment* const* segs, int32_t n,
                       const pgx_leaf_binding* bindings, const pgx_exec_opts* opts, pgx_result** out);
pgx_status pgx_result_release(pgx_result* r);  /* an async result waits for its execution first */

/* Asynchronous execute (SURVEY 8b "async on the stream, then pgx_result_wait"): returns at once with a pending result
 * while the query plans, launches on the context's stream (or opts->stream) and reads back on a library thread.  The
 * segment list, the bindings (including their bitsets) and opts are copied before the call returns; the query and the
 * segments must stay alive until the result is complete.  Every pgx_result_* accessor waits for completion first.
 * Replaces the per-query task the reference submits to its executor (query/executor/ServerQueryExecutorV1Impl.java:
 * 118-134 -> plan/CombinePlanNode.java:66-124 futures). */
pgx_status pgx_execute_async(pgx_ctx* ctx, const pgx_query* q, pgx_segment* const* segs, int32_t n,
                             const pgx_leaf_binding* bindings, const pgx_exec_opts* opts, pgx_result** out);
/* timeout_ms < 0: wait until done.  PGX_ERR_TIMEOUT if still running; otherwise the execution's own status. */
pgx_status pgx_result_wait(pgx_result* r, int64_t timeout_ms);

/* Multi-GPU in one process (SURVEY 8b/8e pgx_execute_multi): ctxs[k] is the context of one device; every segment runs
 * on the device it was staged on (segments never move per query).  The per-device executions run concurrently and
 * their partials merge on ctxs[0]'s device: one key space over ALL segments (the union dictionary per group-by
 * column), dense tables copied over xGMI (hipMemcpyPeerAsync) and reduced plane by plane, device-resident sparse groups
 * copied and merged by a device hash merge (pgx_merge.hip), the rest by key on the host.  Group keys of the result
 * index into THIS segs[] list.  opts: flags only (stream / dense_out must be 0).  Replaces the reference server's one
 * combine over all of its segments (operator/MCombineOperator.java:84-199, MCombineGroupByOperator.java:139-233). */
pgx_status pgx_execute_multi(pgx_ctx* const* ctxs, int32_t nctx, const pgx_query* q, pgx_segment* const* segs,
                             int32_t n, const pgx_leaf_binding* bindings, const pgx_exec_opts* opts, pgx_result** out);

/* Cross-process merge of sparse group-by results (one process per GPU; the caller exchanges the groups, e.g. an RCCL
 * all-to-all by key hash).  A group travels as a record of W uint64 (pgx_result_record_words: W = 1 + planes):
 * packed group key, doc count, then per value column sum, ordered min, ordered max (the layout of the partitioned
 * sparse group-by; an INT / LONG column's sum is int64, a FLOAT / DOUBLE column's the f64 bits).  One value column:
 * W = 5.  pgx_result_device_groups: *n = the number of groups of a result whose groups stay in device memory
 * (PGX_ERR_UNSUPPORTED otherwise) and, when records is non-NULL, the records written to that device buffer
 * (n x W x 8 bytes, on the result's device).  pgx_result_merge_groups: merge n records of like's layout (equal keys
 * combine: counts and integer sums add, f64 sums add in f64 -- in arbitrary order, so within rounding of the
 * reference's sequential order -- minima and maxima take the extreme) into a device-resident result decoded with
 * `like`'s key tables -- valid when every source planned the same key space (identical dictionaries on all ranks);
 * stats (may be NULL: like's) become the result's ExecutionStatistics.  Replaces the cross-server half of
 * MCombineGroupByOperator.java:139-233 (per-function combineTwoValues over equal keys). */
pgx_status pgx_result_device_groups(const pgx_result* r, int64_t* n, void* records);
pgx_status pgx_result_record_words(const pgx_result* r, int32_t* words);
pgx_status pgx_result_merge_groups(pgx_ctx* ctx, const pgx_result* like, const void* records, int64_t n,
                                   const int64_t stats[4], pgx_result** out);

/* ExecutionStatistics: numDocsScanned, numEntriesScannedInFilter, numEntriesScannedPostFilter, totalRawDocs
 * (operator/ExecutionStatistics.java:21-74). */
pgx_status pgx_result_stats(const pgx_result* r, int64_t out[4]);

/* Aggregation-only results.  COUNT: *count. SUM/MIN/MAX: *value. AVG: *value = sum, *count = count.
 * Empty input gives the reference defaults (MIN +inf, MAX -inf, AvgPair(0.0, 0)). */
pgx_status pgx_result_agg(const pgx_result* r, int32_t fn_index, double* value, int64_t* count);

/* Group-by results (combined over the segments, untrimmed). */
pgx_status pgx_result_num_groups(const pgx_result* r, int64_t* n);
/* For group-by column c: per group, the index (into the segs[] given to pgx_execute) of a segment that
 * holds the group's value and that segment's local dictId for it. */
pgx_status pgx_result_group_keys(const pgx_result* r, int32_t c, int32_t* seg_index, int32_t* dict_id);
/* Per group: value (SUM/MIN/MAX; AVG sum) and count (COUNT; AVG count; for SUM/MIN/MAX the group's doc count). */
pgx_status pgx_result_group_values(const pgx_result* r, int32_t fn_index, double* value, int64_t* count);
/* Storage mode the reference would pick for a single segment: 0 ARRAY_BASED, 1 LONG_MAP_BASED, 2 ARRAY_MAP_BASED
 * (operator/aggregation/groupby/DefaultGroupKeyGenerator.java:167-186). */
pgx_status pgx_result_group_mode(const pgx_result* r, int32_t* mode);
/* Combine trim (query/aggregation/groupby/AggregationGroupByOperatorService.java:59-77,284-361): if the number of
 * groups exceeds 20*max(top_n,1000), the indices of the top 5*max(top_n,1000) groups for function fn (MIN ascending,
 * AVG by sum/count, others descending), else all groups.  *n in: capacity, out: count written. */
pgx_status pgx_result_trim(const pgx_result* r, int32_t fn_index, int64_t* group_index, int64_t* n);
/* Keys and values of selected groups only (e.g. the indices pgx_result_trim returned): for group-by column c,
 * seg_index[c*n + j] / dict_id[c*n + j] as pgx_result_group_keys; for function f, value[f*n + j] / count[f*n + j] as
 * pgx_result_group_values.  Results that stay in device memory (sparse group-by) gather on the device and read back
 * only these n groups.  Any output may be NULL. */
pgx_status pgx_result_gather(const pgx_result* r, const int64_t* group_index, int64_t n, int32_t* seg_index,
                             int32_t* dict_id, double* value, int64_t* count);

/* ---- DISTINCTCOUNTHLL ---------------------------------------------------------------------------
 * A query may mix PGX_DISTINCTCOUNTHLL functions (also several over one column) with the standard single-value
 * functions in any order, aggregation-only or under GROUP BY; results keep the request's function order.  The filter,
 * the standard functions and the groups run as they do without the HLL functions (never from a star tree: every raw
 * row is offered), and numEntriesScannedPostFilter counts each HLL column among the projected columns once.
 * pgx_result_hll writes num_groups x 256 bytes: register j of group first_group + i at registers[i * 256 + j], the
 * groups in the order of pgx_result_group_keys / _values; an aggregation-only result has exactly one group
 * (first_group 0, num_groups 1).  The registers are those of stream-lib's HyperLogLog(log2m = 8) after
 * offer((int) hashCode(value)) of every selected doc's value: exact, whatever the order.  PGX_ERR_INVALID_ARG: agg_index
 * is not a PGX_DISTINCTCOUNTHLL[MV] or PGX_FASTHLL function, or the range lies outside the result.
 * PGX_DISTINCTCOUNTHLLMV offers every value of every selected doc of a multi-value column (one slot per doc under
 * GROUP BY: the doc's single-value group columns).  Same registers, same accessor, same statistics: its column counts
 * once among the projected ones (docs x columns, not docs x values).  It mixes with PGX_DISTINCTCOUNTHLL and the
 * standard single-value functions in any order; two functions over one column share their registers.  The function's
 * column must be multi-value in every executed segment ("multi-value function on single-value column" otherwise), as
 * PGX_DISTINCTCOUNTHLL's must be single-value.  pgx_query_compile already returns that PGX_ERR_UNSUPPORTED when the
 * context holds staged segments with a column of that name and every one of them holds it single-value; a column no
 * staged segment has, or one that is multi-value somewhere, compiles, and the execution checks its own segments.  The filter may hold leaves on multi-value columns.
 * Numeric accessors on an HLL function index: those that address ONE function -- pgx_result_agg,
 * pgx_result_group_values, pgx_result_trim -- return PGX_ERR_INVALID_ARG; pgx_result_gather, which returns every
 * function at once, puts value 0 and count 0 there.
 * PGX_ERR_UNSUPPORTED (the caller falls back): under GROUP BY a key space that is not dense (hash or partitioned keys,
 * PGX_X_FORCE_HASH) or has more than PGX_HLL_MAX_GROUP_SLOTS slots (the product of the group columns' cardinalities
 * over the executed segments); PGX_DISTINCTCOUNTHLL on a multi-value column or PGX_DISTINCTCOUNTHLLMV on a
 * single-value one; a multi-value group column or a standard multi-value function (PGX_COUNTMV .. PGX_AVGMV) in the
 * same query; pgx_execute_multi;
 * key domains; a caller's dense table (dense_out, PGX_X_KEEP_DENSE_ON_DEVICE, pgx_query_dense_slots and the other
 * dense-table calls); pgx_execute_timed; PGX_JIT=0.
 * With PGX_X_SPARSE_GROUP_SETS the first of these limits goes: a key space that is not dense (hash keys,
 * PGX_X_FORCE_HASH) or has more than PGX_HLL_MAX_GROUP_SLOTS slots runs through the global hash table (never the
 * partitioned record path), and the registers, presence bitmaps and counter tables of all three families are indexed
 * by the groups the result holds, in the result's order, found per row through a device-side directory from the group
 * columns' global ids to the group's index.  Same accessors, same contents.  PGX_ERR_UNSUPPORTED on this route, after
 * the scan: more than PGX_SET_MAX_SPARSE_GROUPS groups; group columns whose global ids take more than 128 bits
 * (ceil(log2(cardinality)) bits each, at least 1); HLL registers -- 4 bytes x 256 per column and group -- of more than
 * PGX_HLL_MAX_TABLE_BYTES; the DISTINCTCOUNT and PERCENTILE limits below with the groups in place of the slots.  The
 * other limits hold as without the flag. */
#define PGX_HLL_MAX_GROUP_SLOTS 65536
#define PGX_SET_MAX_SPARSE_GROUPS 131072
#define PGX_HLL_MAX_TABLE_BYTES (256u << 20)
pgx_status pgx_result_hll(const pgx_result* r, int32_t agg_index, int64_t first_group, int64_t num_groups,
                          uint8_t* registers);
/* Host only, no device needed: codes[i] = (register << 8) | rank of offer((int) hashCode(value i)), the per-dictId
 * table the kernels gather from.  values: int32 / int64 / float / double per data_type, or for PGX_STRING the values'
 * UTF-8 bytes back to back with n + 1 offsets (string_offsets, else NULL).  hashCode is the boxed Java value's:
 * Integer the value, Long (int)(v ^ v >>> 32), Float floatToIntBits, Double (int)(bits ^ bits >>> 32), String
 * 31 * h + unit over the UTF-16 code units (surrogate pairs for supplementary code points); then MurmurHash.hashLong
 * x, register x >>> 24, rank numberOfLeadingZeros((x << 8) | 0x81) + 1 (1..25). */
pgx_status pgx_hll_codes(int32_t data_type, const void* values, const int32_t* string_offsets, int64_t n,
                         uint16_t* codes);

/* ---- DISTINCTCOUNT ------------------------------------------------------------------------------
 * PGX_DISTINCTCOUNT takes a single-value column of any of the five data types, PGX_DISTINCTCOUNTMV a multi-value one
 * (every value of every selected doc).  The intermediate is the set of (int) hashCode(value), hashCode as described at
 * pgx_java_hash_codes: two different values with equal hash codes count once (LONG 0 and 0x0000000100000001 both hash
 * to 0).  The functions mix with the PGX_DISTINCTCOUNTHLL[MV] and the standard single-value functions in any order and
 * run in the same scan; two of them over one column share their state; statistics are those of the HLL forms, and a
 * column that an HLL and a DISTINCTCOUNT function both name counts once among the projected ones.
 * pgx_result_distinct_counts writes the set size of groups first_group .. first_group + num_groups - 1, in the order
 * of pgx_result_group_keys (an aggregation-only result has exactly one group).  pgx_result_distinct writes those groups'
 * hash codes back to back, ascending and unique within each group; group i's codes start at the sum of the preceding
 * counts.  PGX_ERR_INVALID_ARG: agg_index is not a PGX_DISTINCTCOUNT[MV] function (an HLL index among them), the range
 * lies outside the result, or `capacity` (in codes) is smaller than the sum of the counts.  pgx_result_hll refuses a
 * DISTINCTCOUNT index; pgx_result_agg, _group_values and _trim refuse it as they refuse an HLL index, and
 * pgx_result_gather puts value 0 and count 0 there.
 * pgx_query_compile returns PGX_ERR_UNSUPPORTED for PGX_DISTINCTCOUNTMV when every staged segment of the context that
 * holds the column holds it single-value, and for PGX_DISTINCTCOUNT when every one holds it multi-value; a column no
 * staged segment has compiles, and the execution checks its own segments ("DISTINCTCOUNT on multi-value column",
 * "multi-value function on single-value column").
 * PGX_ERR_UNSUPPORTED (the caller falls back): every limit of the HLL forms above, and presence bitmaps -- one bit per
 * dictId, per group slot (with PGX_X_SPARSE_GROUP_SETS: per group of the result) and per distinct dictionary of the
 * executed segments -- of more than PGX_DISTINCT_MAX_TABLE_BYTES in all. */
#define PGX_DISTINCT_MAX_TABLE_BYTES (256u << 20)
pgx_status pgx_result_distinct_counts(const pgx_result* r, int32_t agg_index, int64_t first_group, int64_t num_groups,
                                      int64_t* counts);
pgx_status pgx_result_distinct(const pgx_result* r, int32_t agg_index, int64_t first_group, int64_t num_groups,
                               int32_t* hash_codes, int64_t capacity);
/* Host only, no device needed: hash_codes[i] = (int) hashCode of value i, the boxed Java value's: Integer the value,
 * Long (int)(v ^ v >>> 32), Float floatToIntBits, Double (int)(bits ^ bits >>> 32), String 31 * h + unit over the
 * UTF-16 code units.  Arguments and checks as for pgx_hll_codes. */
pgx_status pgx_java_hash_codes(int32_t data_type, const void* values, const int32_t* string_offsets, int64_t n,
                               int32_t* hash_codes);

/* ---- PERCENTILE ---------------------------------------------------------------------------------
 * PGX_PERCENTILE takes a single-value INT, LONG, FLOAT or DOUBLE column, PGX_PERCENTILEMV a multi-value one (every
 * value of every selected doc).  The intermediate is the multiset of the selected values as doubles (the dictionary's
 * getDoubleValue), which is all that PercentileAggregationFunction.java's DoubleArrayList holds once
 * quantile/PercentileUtil.java:40-52 has sorted it (PercentileMVAggregationFunction.java: the same over every value).
 * The percentile number is not part of the function: PERCENTILE50/90/95/99, the digest of PERCENTILEEST and the
 * extremes of MINMAXRANGEMV are all reduced from the same histogram by the caller (pgx_histogram_percentile below).
 * The functions mix with the standard single-value functions and with PGX_DISTINCTCOUNTHLL[MV] and
 * PGX_DISTINCTCOUNT[MV] in any order and run in the same scan; two of them over one column share one histogram;
 * statistics are those of the HLL forms, and a column that several of these families name counts once among the
 * projected ones.
 * pgx_result_percentile_counts writes the number of distinct values of groups first_group .. first_group + num_groups
 * - 1, in the order of pgx_result_group_keys (an aggregation-only result has exactly one group).
 * pgx_result_percentile writes those groups' (value, count) pairs back to back, values ascending within each group and
 * values that compare equal merged into one entry; group i's pairs start at the sum of the preceding counts.
 * PGX_ERR_INVALID_ARG: agg_index is not a PGX_PERCENTILE[MV] function, the range lies outside the result, or
 * `capacity` (in pairs) is smaller than the sum of the counts.  pgx_result_hll and pgx_result_distinct[_counts] refuse a
 * percentile index; pgx_result_agg, _group_values and _trim refuse it as they refuse an HLL index, and
 * pgx_result_gather puts value 0 and count 0 there.
 * pgx_query_compile returns PGX_ERR_UNSUPPORTED for PGX_PERCENTILEMV when every staged segment of the context that
 * holds the column holds it single-value, and for PGX_PERCENTILE when every one holds it multi-value; a column no
 * staged segment has compiles, and the execution checks its own segments.
 * PGX_ERR_UNSUPPORTED (the caller falls back): every limit of the HLL forms above; a STRING column (the reference's
 * executor cannot hand one to these functions); and counter tables -- 8 bytes per dictId, per group slot (with
 * PGX_X_SPARSE_GROUP_SETS: per group of the result) and per distinct dictionary of the executed segments -- of more
 * than PGX_PERCENTILE_MAX_TABLE_BYTES in all. */
#define PGX_PERCENTILE_MAX_TABLE_BYTES (256u << 20)
pgx_status pgx_result_percentile_counts(const pgx_result* r, int32_t agg_index, int64_t first_group,
                                        int64_t num_groups, int64_t* counts);
pgx_status pgx_result_percentile(const pgx_result* r, int32_t agg_index, int64_t first_group, int64_t num_groups,
                                 double* values, int64_t* value_counts, int64_t capacity);
/* Host only, no device needed: PercentileUtil.getValueOnQuantile over a histogram.  values: n doubles, strictly
 * ascending; counts: how often each occurs; *out = element (int)(total * (percentile / 100.0)) of the expanded sorted
 * multiset.  PGX_ERR_INVALID_ARG: a percentile outside 0..100, a negative count, values not ascending, or an empty
 * multiset (the reference throws there), or an index at or past the total (percentile 100).  The index is not cut to
 * 32 bits: counts may sum past 2^31. */
pgx_status pgx_histogram_percentile(const double* values, const int64_t* counts, int64_t n, int32_t percentile,
                                    double* out);

/* ---- FASTHLL ------------------------------------------------------------------------------------
 * PGX_FASTHLL takes a single-value STRING column whose values are HyperLogLogs of log2m 8 as
 * startree/hll/HllUtil.java convertHllToString writes them: 180 chars, char = byte + 129 over HyperLogLog.getBytes().
 * The intermediate is the register-wise maximum over the selected docs' estimators (FastHllAggregationFunction.java:
 * addAll into a fresh HyperLogLog(8)), read with pgx_result_hll as a PGX_DISTINCTCOUNTHLL function's; every other
 * accessor treats the index as an HLL index.  The maximum is idempotent, so the registers are a function of the set of
 * dictIds selected: the query marks DISTINCTCOUNT's presence bitmaps (a set of their own, counted on their own
 * against PGX_DISTINCT_MAX_TABLE_BYTES) and folds the set bits' rows of a per-dictionary register image -- 256 bytes
 * per dictId in device memory, built on the first query over the dictionary -- into the result's groups on the device;
 * segments with different dictionaries fold into the same registers.  The function mixes with the standard
 * single-value functions and with codes 10-15 in any order and runs in the same scan; two of them over one column share
 * their state; statistics are those of the HLL forms.
 * pgx_query_compile returns PGX_ERR_UNSUPPORTED when every staged segment of the context that holds the column holds
 * it multi-value or not as STRING; a column no staged segment has compiles, and the execution checks its own segments.
 * PGX_ERR_UNSUPPORTED (the caller falls back): every limit of the HLL forms above, PGX_X_SPARSE_GROUP_SETS lifting the
 * same one (the sparse route counts FASTHLL's u32 registers against PGX_HLL_MAX_TABLE_BYTES too); a multi-value or
 * non-STRING column; a dictionary value that is not such an estimator (the reference throws there); register images
 * of the query's distinct dictionaries of more than PGX_FASTHLL_MAX_IMAGE_BYTES in all, refused before anything is
 * allocated or launched. */
#define PGX_FASTHLL_MAX_IMAGE_BYTES (256u << 20)
/* Host only, no device needed: registers[i * 256 + j] = register j of value i, the rows of the register image.
 * values_utf8: the values' UTF-8 bytes back to back with n + 1 ascending offsets.  Per value: byte = (byte)(UTF-16 code
 * unit - 129) (HllUtil.convertStringToHll), then HyperLogLog.Builder.build: big-endian log2m and byte count, then 43
 * big-endian words of six 5-bit registers (register i: word i / 6, shift 5 * (i % 6)).  A value that is not a 180-byte
 * estimator of log2m 8 (wrong length, log2m or byte count) returns PGX_ERR_UNSUPPORTED with its index in *bad_index
 * (may be NULL; -1 when no value is bad); rows before it are written. */
pgx_status pgx_fasthll_registers(const void* values_utf8, const int32_t* string_offsets, int64_t n, uint8_t* registers,
                                 int64_t* bad_index);

/* Dense-table layout for PGX_X_KEEP_DENSE_ON_DEVICE (multi-GPU RCCL merge):
 * slots = product of group cardinalities; buffer = (1 + num_aggs) planes of slots x 8 bytes.
 * plane 0: int64 doc count; plane 1+i: function i in its accumulator encoding (pgx_result_dense_plane_op).
 * slots = -1: the query has no such table (GROUP BY a multi-value column, or multi-value functions under GROUP BY:
 * their partials merge by key, pgx_result_group_keys / _values, MCombineGroupByOperator.java:166-191). */
pgx_status pgx_query_dense_slots(const pgx_query* q, pgx_segment* const* segs, int32_t n, int64_t* slots);
/* For plane p: 0 = int64 add, 1 = double add, 2 = uint64 ordered-min, 3 = uint64 ordered-max. */
pgx_status pgx_query_dense_plane_op(const pgx_query* q, pgx_segment* const* segs, int32_t n, int32_t plane, int32_t* op);
/* Decode a (possibly RCCL-reduced) dense table living in device memory into a host-side result. */
pgx_status pgx_result_from_dense(pgx_ctx* ctx, const pgx_query* q, pgx_segment* const* segs, int32_t n,
                                 const void* dense_device, const int64_t stats[4], pgx_result** out);

/* ---- synthetic data (benchmarks) ------------------------------------------------------------
 * Fill a device buffer with the fixed-bit forward index of n rows whose dictId is
 * pgx_synth_value(seed, row) = splitmix64(seed ^ (row * 0x9E3779B97F4A7C15)) % card  (DESIGN.md). */
pgx_status pgx_synth_column(pgx_ctx* ctx, void* device_fwd, int64_t n_rows, int32_t bits, int32_t card,
                            uint64_t seed);
/* Joint columns: the row first draws pair = pgx_synth_value(pair_seed, row) % npairs, the dictId is then
 * pgx_synth_value(seed, pair) % card; columns sharing pair_seed / npairs take values from npairs fixed combinations. */
pgx_status pgx_synth_column_paired(pgx_ctx* ctx, void* device_fwd, int64_t n_rows, int32_t bits, int32_t card,
                                   uint64_t seed, uint64_t pair_seed, uint32_t npairs);
/* Host twin of pgx_synth_column's dictIds (int32 per row). */
pgx_status pgx_synth_dict_ids(uint64_t seed, int64_t n_rows, int32_t card, int32_t* out);
/* Segment creation: the <col>.bitmap.inv bytes of a column (HeapBitmapInvertedIndexCreator.java:42-81 layout, roaring
 * portable format).  out == NULL or cap too small: *len receives the size only. */
/* Segment creation: the <col>.sv.unsorted.fwd bytes of n dictIds at `bits` per value (FixedBitSingleValueWriter:
 * MSB-first, big-endian, values back to back); out holds ceil(n * bits / 8) bytes. */
pgx_status pgx_pack_fixed_bit(const int32_t* ids, int64_t n, int32_t bits, uint8_t* out);
pgx_status pgx_inverted_index_build(const int32_t* ids, int64_t n, int32_t card, uint8_t* out, uint64_t cap,
                                    uint64_t* len);
pgx_status pgx_device_alloc(pgx_ctx* ctx, uint64_t bytes, void** out);
pgx_status pgx_device_free(pgx_ctx* ctx, void* p);
pgx_status pgx_copy_to_device(pgx_ctx* ctx, void* dst, const void* src, uint64_t bytes);
pgx_status pgx_copy_to_host(pgx_ctx* ctx, void* dst, const void* src, uint64_t bytes);

/* ---- timing (bench) ---------------------------------------------------------------------------
 * Kernel time of whole executions (ABI 6): between pgx_timing_start and pgx_timing_stop every kernel the library
 * launches (on any stream: the context's, the side stream of batched plans, a caller's) is bracketed by HIP events on
 * its own stream.  pgx_timing_stop waits for the device and returns out[0] = the union of the launches' busy intervals
 * (concurrent kernels count once: the GPU time the executions cost), out[1] = the summed per-launch durations,
 * out[2] = the span from the first launch's start to the last one's end, all in ms; json (optional) receives the same
 * plus per kernel name [launches, summed ms].  One window at a time per process; no reference counterpart. */
pgx_status pgx_timing_start(pgx_ctx* ctx);
pgx_status pgx_timing_stop(pgx_ctx* ctx, double out[3], char* json, uint64_t json_cap);

/* Run the query `iters` times back to back as ONE plan over all n segments (one launch per kernel), returning the
 * average kernel time per iteration measured with HIP events on the stream it is launched on (diagnostics). */
pgx_status pgx_execute_timed(pgx_ctx* ctx, const pgx_query* q, pgx_segment* const* segs, int32_t n,
                             const pgx_leaf_binding* bindings, int32_t iters, double* total_ms,
                             double* kernel_ms, pgx_result** out);

/* ---- query compiler build checks (no device needed) ---------------------------------------------
 * The scan/aggregate kernels are generated per query shape and compiled by hiprtc for gfx950.
 * pgx_jit_compile_check compiles one generated source; pgx_jit_selftest generates and compiles a representative set
 * of shapes and returns the number that failed (*n_total = number tried), with the compiler log in log. */
int pgx_jit_compile_check(const char* source, char* log, unsigned long log_cap);
int pgx_jit_selftest(int* n_total, char* log, unsigned long log_cap);

#ifdef __cplusplus
}
#endif
#endif /* PGX_H_ */
