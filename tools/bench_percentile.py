#!/usr/bin/env python3
"""PERCENTILE / PERCENTILEMV: the native path (one counter per dictId added to on the device, pgx_percentile.hip) next
to the scan that feeds it and next to the host decomposition it replaces.

Two data sets, those of tools/bench_distinct.py.  "sv": synthetic device columns, 64 segments x 2M rows
(pgx_synth_column), c with 2^20 distinct values and g with 1000, plus cs with 512 values and gs with 16 (512 counters,
and 16 x 512 = 8192 under GROUP BY gs: the tables counted in LDS), the C5-style filter ((f1 IN 32 ids OR f2 = 7) AND
f3 <> 3) and match-all.  "mv": the host-built multi-value set of tools/bench_hll_mv.py, 8 segments x 250,000 docs, c
with 1..4 values per doc, the filter f < 10 and match-all, aggregation-only and GROUP BY g.  GPU figures are kernel time
from the library's timing window (pgx_timing_start / pgx_timing_stop), after warm-up:
  scan_ms         the COUNT(*) step with the same filter (and GROUP BY) on the same segments: the scan
  native_ms       the PERCENTILE[MV] step: the same scan writing selection bits, the counts, sizes + emit; the step
                  reads the sizes and the (value, count) pairs of every group (wall time includes that and the host's
                  dictId -> double mapping and merge per group)
  count_ms        pgx_percentile_count[_group|_mv|_mv_group] alone, against its byte floor: the mask words, the
                  selected rows' (values') bits of the value column and the selected docs' bits of the group column, and
                  the counters (8 bytes each), over the MI355X's measured HBM copy rate (6.29 TB/s); and, for the
                  tables counted in HBM, the added bytes per second (8 per selected row or value)
  emit_ms         pgx_percentile_sizes + pgx_percentile_emit
  decomp_*        the same request (PERCENTILE50) through the plan maker with PGX_PERCENTILE_NATIVE=0 (the GROUP BY
                  [g,] c histogram read back as Python values), one step: GPU time and wall time.  Not run under GROUP BY
                  when the filter selects more than --decomp-max-docs docs (every distinct (g, c) pair becomes a Python
                  string there: minutes per step).
A shape the library refuses (PGX_ERR_UNSUPPORTED: the counter tables over PGX_PERCENTILE_MAX_TABLE_BYTES) is recorded
as such; the plan maker runs it as the decomposition.  Prints one JSON line per case and writes them all to --out.

  python tools/bench_percentile.py --out profiles/percentile/bench_percentile.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_BYTES_PER_S = 6.29e12  # MI355X HBM3E as measured by a float4 copy; the spec peak is 8.0 TB/s
LDS_COUNTERS = 8192        # pgx_internal.h kPercentileLdsCounters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="sv,mv")
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--mv-segments", type=int, default=8)
    ap.add_argument("--mv-docs", type=int, default=250_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--decomp-steps", type=int, default=1)
    ap.add_argument("--decomp-max-docs", type=int, default=6_000_000)
    ap.add_argument("--mv-decomp-max-docs", type=int, default=200_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    from bench_hll_mv import mv_column
    from pinot_amd import engine as E
    from pinot_amd import native as N
    from pinot_amd import pql
    from pinot_amd import segment as SEG
    from pinot_amd import synth as S

    ctx = E.Context(0)
    L = N.lib()

    def window(fn, steps, warmup):
        """(GPU ms per step, wall ms per step, per-kernel ms per step, last return value) of `fn`."""
        ret = None
        for _ in range(warmup):
            ret = fn()
        out = (C.c_double * 3)()
        js = C.create_string_buffer(1 << 16)
        N.check(L.pgx_timing_start(ctx.handle))
        t0 = time.perf_counter()
        for _ in range(steps):
            ret = fn()
        wall = (time.perf_counter() - t0) * 1e3 / steps
        N.check(L.pgx_timing_stop(ctx.handle, out, js, len(js)))
        detail = json.loads(js.value.decode())
        kern = detail.get("kernels", detail)
        per = {name: v[1] / steps for name, v in kern.items() if isinstance(v, list) and len(v) == 2}
        return out[0] / steps, wall, per, ret

    def query_step(q, segs, percentile, grouped):
        def step():
            r = q.execute(segs)
            try:
                st = (C.c_int64 * 4)()
                N.check(L.pgx_result_stats(r, st))
                hist = None
                if percentile:
                    ng = C.c_int64(1)
                    if grouped:
                        N.check(L.pgx_result_num_groups(r, C.byref(ng)))
                    hist = E.result_percentile(r, 0, 0, ng.value)
                return list(st), hist
            finally:
                L.pgx_result_release(r)
        return step

    results = []

    def run_set(name, segs, mv, cases, shapes, floor_of, max_docs, shape):
        for fname, flt in cases:
            for col, gcol in shapes:
                grouped = gcol is not None
                gb = " GROUP BY %s" % gcol if grouped else ""
                cq = E._Query(ctx, pql.compile("SELECT COUNT(*) FROM T" + flt + gb))
                scan_ms, _, _, (cstats, _) = window(query_step(cq, segs, False, grouped), args.steps, args.warmup)
                cq.close()
                request = pql.compile("SELECT PERCENTILE50%s(%s) FROM T" % ("MV" if mv else "", col) + flt + gb)
                lib = {"aggregations": [{"fn": "percentilemv" if mv else "percentile", "column": col}],
                       "group_by": request.get("group_by"), "filter": request.get("filter")}
                row = dict(shape, set=name, case=fname, column=col, group_by=gcol, docs_selected=cstats[0],
                           scan_ms=round(scan_ms, 4), steps=args.steps, warmup=args.warmup,
                           hbm_bytes_per_s=HBM_BYTES_PER_S)
                hq = E._Query(ctx, lib)
                hist = None
                try:
                    native_ms, native_wall, per, (hstats, hist) = window(query_step(hq, segs, True, grouped),
                                                                         args.steps, args.warmup)
                except N.PgxError as e:
                    if e.status != N.PGX_ERR_UNSUPPORTED:
                        raise
                    row.update({"native_ms": None, "native_refused": str(e)})
                finally:
                    hq.close()
                if hist is not None:
                    assert hstats[0] == cstats[0] and hstats[1] == cstats[1], (hstats, cstats)
                    count = sum(v for k, v in per.items() if k.startswith("pgx_percentile_count"))
                    emit = per.get("pgx_percentile_sizes", 0.0) + per.get("pgx_percentile_emit", 0.0)
                    floor_bytes, counters, adds = floor_of(hstats[0], col, gcol, flt)
                    floor_ms = 1e3 * floor_bytes / HBM_BYTES_PER_S
                    in_lds = counters <= LDS_COUNTERS
                    row.update({"groups": len(hist), "pairs_total": sum(len(h) for h in hist),
                                "values_counted": sum(c for h in hist for _, c in h),
                                "native_ms": round(native_ms, 4), "native_wall_ms": round(native_wall, 3),
                                "count_ms": round(count, 4), "emit_ms": round(emit, 4),
                                "table_counters": int(counters), "count_mode": "lds" if in_lds else "hbm",
                                "count_floor_bytes": int(floor_bytes), "count_floor_ms": round(floor_ms, 4),
                                "count_over_floor": round(count / floor_ms, 2) if count else None,
                                "hbm_atomic_bytes_per_s": None if in_lds or not count else round(8 * adds / (count * 1e-3)),
                                "kernels_ms_per_step": {n: round(v, 4) for n, v in sorted(per.items())}})
                # the decomposition on the same build: the parent commit's behaviour
                if args.decomp_steps > 0 and not (grouped and cstats[0] > max_docs):
                    print("# %s %s %s%s: decomposition ..." % (name, fname, col, gb), file=sys.stderr, flush=True)
                    os.environ["PGX_PERCENTILE_NATIVE"] = "0"
                    try:
                        pm = E.InstancePlanMakerImplV2(ctx)
                        d_ms, d_wall, dper, blk = window(lambda: pm.make_inter_segment_plan(segs, request).execute(),
                                                         args.decomp_steps, 0)
                    finally:
                        del os.environ["PGX_PERCENTILE_NATIVE"]
                    if hist is not None:
                        t0 = time.perf_counter()
                        on = pm.make_inter_segment_plan(segs, request).execute()  # the native path, the same door
                        row["native_plan_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                        if grouped:
                            mon = on.get_aggregation_group_by_result().as_map()
                            moff = blk.get_aggregation_group_by_result().as_map()
                            assert set(mon) == set(moff) and all(mon[k][0] == moff[k][0] for k in mon)
                            assert sorted(map(len, hist)) == sorted(len(v[0]) for v in moff.values())
                        else:
                            assert on.get_aggregation_result()[0] == blk.get_aggregation_result()[0] == hist[0]
                    row.update({"decomp_gpu_ms": round(d_ms, 4), "decomp_wall_ms": round(d_wall, 1),
                                "decomp_steps": args.decomp_steps, "decomp_equal": hist is not None or None,
                                "decomp_kernels_ms_per_step": {n: round(v, 4) for n, v in sorted(dper.items())}})
                else:
                    row.update({"decomp_gpu_ms": None, "decomp_wall_ms": None, "decomp_steps": 0,
                                "decomp_skipped": "not run: selects %d docs under GROUP BY, every distinct (g, c) pair "
                                                  "becomes a Python string" % cstats[0]})
                results.append(row)
                print(json.dumps(row), flush=True)

    sets = args.sets.split(",")
    if "sv" in sets:
        cols = [S.ColSpec("f1", 1000, inverted=True), S.ColSpec("f2", 100, inverted=True),
                S.ColSpec("f3", 10, inverted=True), S.ColSpec("c", 1 << 20), S.ColSpec("g", 1000),
                S.ColSpec("cs", 512), S.ColSpec("gs", 16)]
        wl = S.Workload("percentile", "PERCENTILE50(c) [GROUP BY g]", args.segments, args.rows, cols, "", 11, "weak")
        print("# staging %d segments x %d rows ..." % (args.segments, args.rows), file=sys.stderr, flush=True)
        dev = S.DeviceSegments(ctx, wl, list(range(args.segments)), rows=args.rows)
        bits = {c.name: c.bits for c in cols}
        cards = {"c": 1 << 20, "g": 1000, "cs": 512, "gs": 16}
        mask_bytes = args.segments * ((args.rows + 31) // 32) * 4

        def sv_floor(docs, col, gcol, flt):
            counters = (cards[gcol] if gcol else 1) * cards[col]  # one shared dictionary: one table
            return (mask_bytes + (docs * (bits[col] + (bits[gcol] if gcol else 0)) + 7) // 8 + counters * 8, counters,
                    docs)

        run_set("sv", dev.segments, False, (("c5_filter", c5_filter()), ("match_all", "")),
                (("c", None), ("c", "g"), ("cs", None), ("cs", "gs"), ("cs", "g")), sv_floor, args.decomp_max_docs,
                {"segments": args.segments, "rows_per_segment": args.rows})
        dev.free()
    if "mv" in sets:
        segs, host = [], []
        for i in range(args.mv_segments):
            rng = np.random.default_rng(1000 + i)
            lens = rng.integers(1, 5, args.mv_docs).astype(np.int64)
            vals = rng.integers(0, 1 << 20, int(lens.sum()))
            g = rng.integers(0, 1000, args.mv_docs).astype(np.int32)
            f = rng.integers(0, 1000, args.mv_docs).astype(np.int32)
            seg = SEG.make_segment("pmv%d" % i, [mv_column(SEG, np, "c", vals, lens), SEG.make_column("g", g),
                                                 SEG.make_column("f", f)])
            host.append((lens, f, seg.columns["c"].bits, seg.columns["g"].bits, seg.columns["c"].cardinality))
            segs.append(E.IndexSegment(ctx, seg))
        mv_mask_bytes = args.mv_segments * ((args.mv_docs + 31) // 32) * 4

        def mv_floor(docs, col, gcol, flt):
            total, counters, adds = mv_mask_bytes, 0, 0
            for lens, f, cb, gbits, card in host:
                sel = (f < 10) if flt else np.ones(len(f), bool)
                nd, nv = int(sel.sum()), int(lens[sel].sum())
                total += 8 * nd + (nv * cb + (nd * gbits if gcol else 0) + 7) // 8
                counters = max(counters, (1000 if gcol else 1) * card)  # every segment its own dictionary and table
                total += (1000 if gcol else 1) * card * 8
                adds += nv
            return total, counters, adds

        run_set("mv", segs, True, (("f_lt_10", " WHERE f < 10"), ("match_all", "")), (("c", None), ("c", "g")),
                mv_floor, args.mv_decomp_max_docs, {"segments": args.mv_segments, "docs_per_segment": args.mv_docs})
        for s in segs:
            s.destroy()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


def c5_filter():
    return " WHERE (f1 IN (%s) OR f2 = 7) AND f3 <> 3" % ",".join(str(v) for v in range(3, 1000, 31)[:32])


if __name__ == "__main__":
    main()
