"""DISTINCTCOUNT, MINMAXRANGE and PERCENTILE{50,90,95,99} for aggregation-only requests,
decomposed on the host into GPU sub-queries the fused scan kernels already run:

* MINMAXRANGE(c) -> MIN(c) and MAX(c) in the base query; intermediate (min, max)
  (core/operator/aggregation/function/MinMaxRangeAggregationFunction.java aggregate: a Pair of block extremes);
* DISTINCTCOUNT(c) -> a function of the base query itself (PGX_DISTINCTCOUNT, DISTINCTCOUNTMV(c) PGX_DISTINCTCOUNTMV:
  presence bits per dictId marked on the device, the set read with pgx_result_distinct; ``native_distinct``).  Where
  the library refuses the shape, or with PGX_DISTINCT_NATIVE=0, ``GROUP BY c`` with COUNT(*) under the same filter;
  intermediate the set of the values' Java
  hashCode()s: the executor hands DISTINCTCOUNT / DISTINCTCOUNTHLL ``getSVHashCodeArray()``
  (operator/aggregation/DefaultAggregationExecutor.java:135-139, common/DataFetcher.java:242-248:
  ``dictionary.get(dictId).hashCode()``), and the function adds ``(int) hash`` (operator/aggregation/function/
  DistinctCountAggregationFunction.java aggregate), so STRING columns are supported and FLOAT 0.25 / 0.75 stay distinct;
* PERCENTILEnn(c), PERCENTILEESTnn(c), their MV forms and MINMAXRANGEMV(c) -> one function of the base query itself per
  column (PGX_PERCENTILE / PGX_PERCENTILEMV: one counter per dictId on the device, the (value, count) pairs read with
  pgx_result_percentile; ``native_percentile``).  Where the library refuses the shape, or with PGX_PERCENTILE_NATIVE=0,
  the same ``GROUP BY c`` histogram; intermediate the (value, count) pairs in value order, i.e. the
  reference's DoubleArrayList of every selected value (PercentileAggregationFunction.java aggregate) held as a multiset;
* DISTINCTCOUNTHLL(c) -> a function of the base query itself (PGX_DISTINCTCOUNTHLL: the registers are built on the
  device and read with pgx_result_hll; ``native_hll``), and DISTINCTCOUNTHLLMV(c) likewise (PGX_DISTINCTCOUNTHLLMV:
  every value of every selected doc).  Where the library refuses the shape, or with PGX_HLL_NATIVE=0, the same histogram; intermediate the HyperLogLog registers of the distinct hash codes (operator/aggregation/function/
  DistinctCountHLLAggregationFunction.java aggregate: hll.offer((int) hash)), which depend only on that set (hll.py);
* FASTHLL(c) -> a function of the base query itself (PGX_FASTHLL: the selected dictIds' decoded estimators are merged on
  the device, pgx_fasthll.hip, and read with pgx_result_hll; ``native_fasthll``).  Where the library refuses the shape,
  or with PGX_FASTHLL_NATIVE=0, the same histogram, whose distinct serialized values are deserialized and merged here.

One histogram sub-query serves every DISTINCTCOUNT / PERCENTILE over the same column.  Statistics are the base query's,
with numEntriesScannedPostFilter counted over the ORIGINAL projection columns (AggregationOperator.java:93-98).
Group-by requests keep their GROUP BY columns in the base query, and the histograms group by those columns plus c
(``_run_group_by``).  A STRING column under PERCENTILE / MINMAXRANGE raises ``PgxError(UNSUPPORTED)`` (the executor
hands those functions String[] values and their aggregate() requires double[]).
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Sequence

import numpy as np

from . import engine as E
from . import hll as HLL
from . import qdigest as QD
from . import native as N
from .pql import EXT_FUNCTIONS, EXT_MV_FUNCTIONS


_HIST_FNS = ("distinctcount", "distinctcounthll", "fasthll")
_NATIVE_HLL_FNS = ("distinctcounthll", "distinctcounthllmv")  # functions of the base query when `native_hll`
_NATIVE_DISTINCT_FNS = ("distinctcount", "distinctcountmv")  # ... when `native_distinct`
_NATIVE_FASTHLL_FNS = ("fasthll",)  # ... when `native_fasthll`
# ... when `native_percentile`: everything reduced from the value histogram of one column
_NATIVE_PERCENTILE_FNS = tuple("percentile%s%d%s" % (e, p, m) for e in ("", "est") for p in (50, 90, 95, 99)
                               for m in ("", "mv")) + ("minmaxrangemv",)


def base_fn(fn: str) -> str:
    """DISTINCTCOUNTMV, DISTINCTCOUNTHLLMV, MINMAXRANGEMV, PERCENTILEnnMV, PERCENTILEESTnnMV are their single-value
    functions over every value of a multi-value column (DistinctCountMVAggregationFunction.java aggregate: every value's
    hash code; MinMaxRangeMV / PercentileMV / PercentileestMV: every value): the ``GROUP BY c`` histogram of a
    multi-value c counts one entry per value occurrence (pgx_mv_group), which is exactly that multiset."""
    return fn[:-2] if fn in EXT_MV_FUNCTIONS else fn


def has_extended(request: dict) -> bool:
    return any(a["fn"] in EXT_FUNCTIONS for a in request["aggregations"])


def java_int_cast(x) -> int:
    """Java (int) of a double: truncation toward zero, saturating at the int range, NaN -> 0 (JLS 5.1.3)."""
    x = float(x)
    if x != x:
        return 0
    if x >= 2147483647.0:
        return 2147483647
    if x <= -2147483648.0:
        return -2147483648
    return int(x)


def java_hash_code(dtype: str, v) -> int:
    """Boxed dictionary value's hashCode(): Integer -> value; Long -> (int)(v ^ v >>> 32); Float -> floatToIntBits;
    Double -> (int)(bits ^ bits >>> 32) of doubleToLongBits (NaN canonical); String -> s[0]*31^(n-1) + ... over UTF-16
    code units; all in Java int arithmetic."""
    def i32(x: int) -> int:
        x &= 0xFFFFFFFF
        return x - (1 << 32) if x & 0x80000000 else x
    if dtype == "INT":
        return i32(int(v))
    if dtype == "LONG":
        u = int(v) & 0xFFFFFFFFFFFFFFFF
        return i32(u ^ (u >> 32))
    if dtype == "FLOAT":
        f = np.float32(v)
        return 0x7FC00000 if f != f else int(np.array([f], dtype=np.float32).view(np.int32)[0])
    if dtype == "DOUBLE":
        d = float(v)
        u = 0x7FF8000000000000 if d != d else int(np.array([d]).view(np.uint64)[0])
        return i32(u ^ (u >> 32))
    h = 0
    b = str(v).encode("utf-16-be", "surrogatepass")
    for i in range(0, len(b), 2):
        h = (31 * h + (b[i] << 8 | b[i + 1])) & 0xFFFFFFFF
    return i32(h)


def _parse_value(dtype: str, s: str):
    """A group-key field back to the column's value (keys render INT/LONG as integers, FLOAT/DOUBLE as Double.toString,
    which identifies the value exactly)."""
    if dtype in ("INT", "LONG"):
        return int(s)
    if dtype == "STRING":
        return s
    return float(np.float32(float(s))) if dtype == "FLOAT" else float(s)


def percentile_of_histogram(fn: str, hist: Sequence) -> float:
    """quantile/PercentileUtil.getValueOnQuantile over the multiset: element (int)(size * p / 100) of the sorted
    values (query/aggregation/function/quantile/PercentileUtil.java:40-52)."""
    p = int(fn[len("percentile"):])
    total = sum(int(c) for _, c in hist)
    idx = int(total * (p / 100.0))
    if idx >= total:
        raise IndexError("percentile of an empty value list")
    for v, c in hist:
        if idx < c:
            return float(v)
        idx -= int(c)
    raise AssertionError("unreachable")


def merge_histograms(a: Sequence, b: Sequence) -> List:
    d: Dict[float, int] = {}
    for v, c in list(a) + list(b):
        d[v] = d.get(v, 0) + int(c)
    return sorted(d.items())


def _projection_count(request: dict) -> int:
    cols = []
    for a in request["aggregations"]:
        if a["fn"] != "count" and a["column"] not in cols:
            cols.append(a["column"])
    for g in (request.get("group_by") or {}).get("columns", []):
        if g not in cols:
            cols.append(g)
    return len(cols)


def _star_tree_request(request: dict, segments) -> bool:
    use_st = str((request.get("debug_options") or {}).get("useStarTree", "true")).lower() != "false"
    return use_st and any(getattr(s.data, "star_tree", None) is not None for s in segments)


def native_hll(request: dict, segments) -> bool:
    """Whether the request's DISTINCTCOUNTHLL and DISTINCTCOUNTHLLMV functions run inside the base query
    (PGX_DISTINCTCOUNTHLL / PGX_DISTINCTCOUNTHLLMV: registers computed on the device, pgx_hll.hip) instead of through the ``GROUP BY c`` histogram.  PGX_HLL_NATIVE=0
    forces the histogram (A/B, tests).  The native query never uses a star tree (every raw row is offered), so a request
    whose base query a star tree could answer keeps the decomposition, and with it its statistics."""
    if os.environ.get("PGX_HLL_NATIVE", "1") == "0":
        return False
    if not any(a["fn"] in _NATIVE_HLL_FNS for a in request["aggregations"]):
        return False
    return not _star_tree_request(request, segments)


def native_distinct(request: dict, segments) -> bool:
    """Whether the request's DISTINCTCOUNT and DISTINCTCOUNTMV functions run inside the base query (PGX_DISTINCTCOUNT /
    PGX_DISTINCTCOUNTMV, pgx_distinct.hip), by ``native_hll``'s rules: PGX_DISTINCT_NATIVE=0 forces the histogram, and a
    request whose base query a star tree could answer keeps the decomposition."""
    if os.environ.get("PGX_DISTINCT_NATIVE", "1") == "0":
        return False
    if not any(a["fn"] in _NATIVE_DISTINCT_FNS for a in request["aggregations"]):
        return False
    return not _star_tree_request(request, segments)


def native_percentile(request: dict, segments) -> bool:
    """Whether the request's PERCENTILEnn, PERCENTILEESTnn (also MV) and MINMAXRANGEMV functions read their value
    histogram from a PGX_PERCENTILE / PGX_PERCENTILEMV function of the base query (pgx_percentile.hip), by
    ``native_hll``'s rules: PGX_PERCENTILE_NATIVE=0 forces the ``GROUP BY c`` histogram, and a request whose base query
    a star tree could answer keeps the decomposition."""
    if os.environ.get("PGX_PERCENTILE_NATIVE", "1") == "0":
        return False
    if not any(a["fn"] in _NATIVE_PERCENTILE_FNS for a in request["aggregations"]):
        return False
    return not _star_tree_request(request, segments)


def native_fasthll(request: dict, segments) -> bool:
    """Whether the request's FASTHLL functions run inside the base query (PGX_FASTHLL, pgx_fasthll.hip), by
    ``native_hll``'s rules: PGX_FASTHLL_NATIVE=0 forces the histogram, and a request whose base query a star tree could
    answer keeps the decomposition."""
    if os.environ.get("PGX_FASTHLL_NATIVE", "1") == "0":
        return False
    if not any(a["fn"] in _NATIVE_FASTHLL_FNS for a in request["aggregations"]):
        return False
    return not _star_tree_request(request, segments)


def sparse_sets_flag() -> int:
    """The execution flag of a group-by base query that holds native functions (``native_hll``, ``native_distinct``,
    ``native_percentile``): PGX_X_SPARSE_GROUP_SETS, with which the library also takes key spaces that are not dense or
    have more than PGX_HLL_MAX_GROUP_SLOTS slots (tables of one row per group of the result).  What it still refuses
    (PGX_ERR_UNSUPPORTED) runs as the next route of ``run``, down to the decomposition.  The flag is passed only with
    PGX_SPARSE_SETS_NATIVE=1 (read here, at every request).  Without it, or with PGX_SPARSE_SETS_NATIVE=0, such key
    spaces are refused at once and decomposed, as before the flag: the plan maker's route for them is pinned by
    tests/test_gpu_percentile.py and tests/test_gpu_distinct.py (no native histogram or set is read for a refused
    shape), so the sparse route through the plan maker is opt-in, as it is at the ABI."""
    return N.PGX_X_SPARSE_GROUP_SETS if os.environ.get("PGX_SPARSE_SETS_NATIVE", "0") == "1" else 0


def _is_hist_slot(s) -> bool:
    return isinstance(s, tuple) and s[0] == "hist"


def _from_native_histogram(fn: str, h):
    """The intermediate of a `_NATIVE_PERCENTILE_FNS` function from its column's (value, count) pairs, as the
    decomposition builds it from the ``GROUP BY c`` histogram."""
    if fn == "minmaxrange":
        return (float(h[0][0]), float(h[-1][0])) if h else (math.inf, -math.inf)
    if fn.startswith("percentileest"):
        return QD.from_histogram(_numeric(h))
    return _numeric(h)


def _base_request(request: dict, native: Sequence[str] = ()):
    """The base GPU request (COUNT(*), the standard functions, MIN + MAX for each MINMAXRANGE, and the functions named
    in `native`: DISTINCTCOUNTHLL[MV], DISTINCTCOUNT[MV], FASTHLL, and one PERCENTILE[MV] per column for the functions
    reduced from its value histogram) and, per original function, its base slot: an index, a (min, max) index pair,
    ("hist", index) for a native value histogram, or None (histogram sub-query functions)."""
    base = [{"fn": "count", "column": "*"}]
    slot = []
    for a in request["aggregations"]:
        fn = a["fn"]
        if fn in native and fn in _NATIVE_PERCENTILE_FNS:
            f = {"fn": "percentilemv" if fn in EXT_MV_FUNCTIONS else "percentile", "column": a["column"]}
            if f not in base:  # the functions of one column share one histogram
                base.append(f)
            slot.append(("hist", base.index(f)))
        elif fn in native:
            base.append(dict(a))
            slot.append(len(base) - 1)
        elif fn == "minmaxrange":
            base += [{"fn": "min", "column": a["column"]}, {"fn": "max", "column": a["column"]}]
            slot.append((len(base) - 2, len(base) - 1))
        elif fn in _HIST_FNS or fn.startswith("percentile") or fn in EXT_MV_FUNCTIONS:
            slot.append(None)  # MINMAXRANGEMV too: from the histogram (MINMV / MAXMV fold differently by group)
        else:
            base.append(dict(a))
            slot.append(len(base) - 1)
    return base, slot


def _dtype(segments, col: str) -> str:
    return segments[0].column(col).meta.data_type if segments else "INT"


def _hist_columns(request: dict, segments, native: Sequence[str] = ()) -> List[str]:
    cols = []
    for a in request["aggregations"]:
        mv = a["fn"] in EXT_MV_FUNCTIONS
        fn = base_fn(a["fn"])
        if a["fn"] in native:  # in the base query: no histogram on its account
            continue
        if fn not in _HIST_FNS and fn != "minmaxrange" and not fn.startswith("percentile"):
            continue
        if segments and bool(segments[0].column(a["column"]).meta.is_mv) != mv:
            raise N.PgxError(N.PGX_ERR_UNSUPPORTED, "%s over a %s column" % (
                a["fn"], "single-value" if mv else "multi-value"))
        if fn not in _HIST_FNS and _dtype(segments, a["column"]) == "STRING":
            raise N.PgxError(N.PGX_ERR_UNSUPPORTED, "%s over a STRING column" % fn)
        if fn == "fasthll" and _dtype(segments, a["column"]) != "STRING":  # aggregate() requires String[]
            raise N.PgxError(N.PGX_ERR_UNSUPPORTED, "fasthll over a non-STRING column")
        if (fn != "minmaxrange" or mv) and a["column"] not in cols:
            cols.append(a["column"])
    return cols


def _hash_set(dtype: str, hist) -> set:
    return {java_hash_code(dtype, v) for v, _ in hist}


def _fast_hll(hist) -> np.ndarray:
    """FastHllAggregationFunction.aggregate: addAll of every selected doc's deserialized HLL into a fresh HyperLogLog(8)
    (operator/aggregation/function/FastHllAggregationFunction.java aggregate); max is idempotent, so each distinct
    serialized value is merged once."""
    regs = HLL.empty()
    for v, _ in hist:
        try:
            regs = HLL.merge(regs, HLL.from_string(v))
        except ValueError as e:
            raise N.PgxError(N.PGX_ERR_UNSUPPORTED, "fasthll: %s" % e)
    return regs


def _numeric(hist) -> List:
    return [(float(v), c) for v, c in hist]


def _run_group_by(ctx, request, segments, combine, native: Sequence[str] = ()) -> E.IntermediateResultsBlock:
    """Group-by: the base request keeps the GROUP BY columns; each histogram column c runs ``GROUP BY <columns>, c``
    with COUNT(*), and its groups are folded back per leading key (the group string minus its last field).  The
    combine trim keeps the base request's trimmed maps for the standard functions; functions whose intermediates the
    reference cannot order keep every group (AggregationGroupByOperatorService.java:336-349)."""
    gb = request["group_by"]
    base, slot = _base_request(request, native)
    bq = E._Query(ctx, {"aggregations": base, "group_by": dict(gb), "filter": request.get("filter")})
    r = bq.execute(segments, flags=sparse_sets_flag() if native else 0)
    try:
        bblk = E.decode_result(bq, r, segments, trim=combine)
    finally:
        N.lib().pgx_result_release(r)
        bq.close()
    bmap = bblk.get_aggregation_group_by_result().as_map()
    ng = len(gb["columns"])
    hists: Dict[str, Dict[str, List]] = {}
    for c in _hist_columns(request, segments, native):
        hq = E._Query(ctx, {"aggregations": [{"fn": "count", "column": "*"}],
                            "group_by": {"columns": list(gb["columns"]) + [c], "top_n": gb.get("top_n", 10)},
                            "filter": request.get("filter")})
        r = hq.execute(segments)
        try:
            hres = E.decode_result(hq, r, segments).get_aggregation_group_by_result()
        finally:
            N.lib().pgx_result_release(r)
            hq.close()
        dt = _dtype(segments, c)
        per: Dict[str, Dict[object, int]] = {}
        parts = hres.key_parts  # per column: any field, leading or last, may itself hold tabs (STRING values)
        for gk in hres.get_group_key_iterator():
            i, cnt = gk.group_id, hres.get_result_for_key(gk, 0)
            g, v = "\t".join(parts[j][i] for j in range(ng)), _parse_value(dt, parts[ng][i])
            d = per.setdefault(g, {})
            d[v] = d.get(v, 0) + int(cnt)
        hists[c] = {g: sorted(d.items()) for g, d in per.items()}
    aggs = request["aggregations"]

    def value(a, s, key, bvals):
        fn = base_fn(a["fn"])
        if _is_hist_slot(s):
            return _from_native_histogram(fn, bvals[s[1]])
        if fn == "minmaxrange" and s is None:  # MINMAXRANGEMV: the extremes of the value multiset
            h = hists[a["column"]].get(key, [])
            return (float(h[0][0]), float(h[-1][0])) if h else (math.inf, -math.inf)
        if fn == "minmaxrange":
            return (float(bvals[s[0]]), float(bvals[s[1]]))
        if fn == "distinctcount" and s is None:
            return _hash_set(_dtype(segments, a["column"]), hists[a["column"]].get(key, []))
        if fn == "distinctcounthll" and s is None:
            return HLL.from_ints(_hash_set(_dtype(segments, a["column"]), hists[a["column"]].get(key, [])))
        if fn == "fasthll" and s is None:
            return _fast_hll(hists[a["column"]].get(key, []))
        if fn.startswith("percentileest"):
            return QD.from_histogram(_numeric(hists[a["column"]].get(key, [])))
        if fn.startswith("percentile"):
            return _numeric(hists[a["column"]].get(key, []))
        return bvals[s]

    keys = list(bmap)
    per_group = [[value(a, s, k, bmap[k]) for a, s in zip(aggs, slot)] for k in keys]
    res = E.AggregationGroupByResult(keys, per_group, [a["fn"] for a in aggs],
                                     bblk.get_aggregation_group_by_result().storage_mode)
    st = bblk.stats
    docs = st.num_docs_scanned
    blk = E.IntermediateResultsBlock(aggregation_group_by_result=res, stats=E.ExecutionStatistics(
        docs, st.num_entries_scanned_in_filter, docs * _projection_count(request), st.num_total_raw_docs))
    if combine:
        trimmed = []
        for i, (a, s) in enumerate(zip(aggs, slot)):
            if a["fn"] in EXT_FUNCTIONS:
                trimmed.append({k: per_group[j][i] for j, k in enumerate(keys)})
            else:
                trimmed.append(dict(bblk.trimmed[s]))
        blk.trimmed = trimmed
    return blk


def run(ctx: E.Context, request: dict, segments: Sequence[E.IndexSegment],
        combine: bool = True) -> E.IntermediateResultsBlock:
    """Native where the library takes the shape: first with every enabled family in the base query, then without the
    FASTHLL family (a refused FASTHLL leaves the others on the routes they take without it), then without the
    percentile family, then with the HLL functions alone (an HLL function keeps its native path when a DISTINCTCOUNT
    beside it is refused), then the full decomposition.  No measured shape ran slower natively than decomposed
    (tools/bench_percentile.py, tools/bench_fasthll.py), so none is routed away beforehand."""
    families = [(native_fasthll(request, segments), _NATIVE_FASTHLL_FNS),
                (native_percentile(request, segments), _NATIVE_PERCENTILE_FNS),
                (native_distinct(request, segments), _NATIVE_DISTINCT_FNS),
                (native_hll(request, segments), _NATIVE_HLL_FNS)]
    routes = []
    for i, (on, _) in enumerate(families):
        if on:
            routes.append(sum((fns for on_j, fns in families[i:] if on_j), ()))
    for native in routes:
        try:
            return _run(ctx, request, segments, combine, native)
        except N.PgxError as e:  # a shape the native path refuses runs as the next route
            if e.status != N.PGX_ERR_UNSUPPORTED:
                raise
    return _run(ctx, request, segments, combine, ())


def _run(ctx, request, segments, combine, native) -> E.IntermediateResultsBlock:
    if request.get("group_by"):
        return _run_group_by(ctx, request, segments, combine, native)
    aggs = request["aggregations"]
    base, slot = _base_request(request, native)
    bq = E._Query(ctx, {"aggregations": base, "group_by": None, "filter": request.get("filter")})
    r = bq.execute(segments)
    try:
        bblk = E.decode_result(bq, r, segments)
    finally:
        N.lib().pgx_result_release(r)
        bq.close()
    hists = {}
    for c in _hist_columns(request, segments, native):
        hq = E._Query(ctx, {"aggregations": [{"fn": "count", "column": "*"}],
                            "group_by": {"columns": [c], "top_n": 10}, "filter": request.get("filter")})
        r = hq.execute(segments)
        try:
            cols, _, cnts = E.group_partials(hq, r, segments)
        finally:
            N.lib().pgx_result_release(r)
            hq.close()
        order = np.argsort(cols[0], kind="stable")
        hists[c] = [(cols[0][i], int(cnts[0][i])) for i in order]
    base_res = bblk.get_aggregation_result()
    out = []
    for a, s in zip(aggs, slot):
        fn = base_fn(a["fn"])
        if _is_hist_slot(s):
            out.append(_from_native_histogram(fn, base_res[s[1]]))
        elif fn == "minmaxrange" and s is None:  # MINMAXRANGEMV
            h = hists[a["column"]]
            out.append((float(h[0][0]), float(h[-1][0])) if h else (math.inf, -math.inf))
        elif fn == "minmaxrange":
            out.append((float(base_res[s[0]]), float(base_res[s[1]])))
        elif fn == "distinctcount" and s is None:
            out.append(_hash_set(_dtype(segments, a["column"]), hists[a["column"]]))
        elif fn == "distinctcounthll" and s is None:
            out.append(HLL.from_ints(_hash_set(_dtype(segments, a["column"]), hists[a["column"]])))
        elif fn == "fasthll" and s is None:
            out.append(_fast_hll(hists[a["column"]]))
        elif fn.startswith("percentileest"):  # QuantileDigest of the selected values (pinot_amd/qdigest.py)
            out.append(QD.from_histogram(_numeric(hists[a["column"]])))
        elif fn.startswith("percentile"):
            out.append(_numeric(hists[a["column"]]))
        else:
            out.append(base_res[s])
    st = bblk.stats
    docs = st.num_docs_scanned
    stats = E.ExecutionStatistics(docs, st.num_entries_scanned_in_filter, docs * _projection_count(request),
                                  st.num_total_raw_docs)
    return E.IntermediateResultsBlock(aggregation_result=out, stats=stats)


def reduce_value(fn: str, v):
    """Final value of an extended function's (combined) intermediate (DistinctCountAggregationFunction.java:136-145,
    MinMaxRangeAggregationFunction.java:129-146 with DEFAULT_MIN_MAX_RANGE_VALUE = -1, PercentileUtil)."""
    fn = base_fn(fn)
    if fn == "distinctcount":
        return len(v)
    if fn in ("distinctcounthll", "fasthll"):  # query/aggregation/function/{DistinctCountHLL,FastHll}... reduce
        return HLL.cardinality(v)
    if fn == "minmaxrange":
        return v[1] - v[0] if v[0] != math.inf and v[1] != -math.inf else -1.0
    if fn.startswith("percentileest"):  # DigestAggregationFunction.reduce (quantile/digest/...:134-141): a long
        return 0 if v is None else v.get_quantile(int(fn[len("percentileest"):]) / 100.0)
    return percentile_of_histogram(fn, v)


def combine_two(fn: str, a, b):
    """combineTwoValues: set union, pair extremes, list concatenation (histogram merge)."""
    fn = base_fn(fn)
    if fn == "distinctcount":
        return set(a) | set(b)
    if fn in ("distinctcounthll", "fasthll"):  # HyperLogLog.addAll
        return HLL.merge(a, b)
    if fn == "minmaxrange":
        return (min(a[0], b[0]), max(a[1], b[1]))
    if fn.startswith("percentileest"):  # DigestAggregationFunction.combineTwoValues: merge into the first
        return QD.merge_all([QD.QuantileDigest.deserialize(a.serialize()), b])
    return merge_histograms(a, b)
