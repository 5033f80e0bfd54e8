#!/usr/bin/env python3
"""The sparse GROUP BY of DISTINCTCOUNTHLL, DISTINCTCOUNT and PERCENTILE (PGX_X_SPARSE_GROUP_SETS) on synthetic device
columns, beside tools/bench_hll.py, bench_distinct.py and bench_percentile.py and on their data: 64 segments x 2M rows
(pgx_synth_column), the C5-style filter ((f1 IN 32 ids OR f2 = 7) AND f3 <> 3, bitmap inverted indexes) and match-all.
Value columns: c with 2^20 distinct values (HLL), d with 4,096 (DISTINCTCOUNT: 512 bytes of presence bits per group),
p with 256 (PERCENTILE: 2 KiB of counters per group).  Group columns: g1 x g2, 300 x 300 = 90,000 slots (past
PGX_HLL_MAX_GROUP_SLOTS), and g with 1,000.

  sparse   GROUP BY g1, g2 with the flag, per family and filter: GPU ms per step (the library's timing window: the
           union of the launches' busy intervals) and wall ms per step of pgx_execute, the directory build and the
           sparse group kernel on their own; and the same request through the plan maker with PGX_SPARSE_SETS_NATIVE=0
           on the same build, one step (the decomposition: what the request cost before the flag), unless the filter
           selects more than --decomp-max-docs rows (minutes per step: "not run").
  dense    GROUP BY g: the dense group kernel (no flag; twice, for its run-to-run spread) and the sparse one forced on
           the same key space (PGX_X_FORCE_HASH with the flag): what the per-row lookup costs over the multiply-add.
Prints one JSON line per case and writes them all to --out.

  python tools/bench_sparse_sets.py --out profiles/sparse_sets/bench_sparse_sets.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FAMILIES = {  # family: (library function, value column, PQL function, dense group kernel)
    "hll": ("distinctcounthll", "c", "DISTINCTCOUNTHLL", "pgx_hll_offer_group"),
    "distinct": ("distinctcount", "d", "DISTINCTCOUNT", "pgx_distinct_mark_group"),
    "percentile": ("percentile", "p", "PERCENTILE50", "pgx_percentile_count_group"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--decomp-steps", type=int, default=1)
    ap.add_argument("--decomp-max-docs", type=int, default=6_000_000)
    ap.add_argument("--families", default="hll,distinct,percentile")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from pinot_amd import engine as E
    from pinot_amd import native as N
    from pinot_amd import pql
    from pinot_amd import synth as S

    cols = [S.ColSpec("f1", 1000, inverted=True), S.ColSpec("f2", 100, inverted=True), S.ColSpec("f3", 10, inverted=True),
            S.ColSpec("c", 1 << 20), S.ColSpec("d", 4096), S.ColSpec("p", 256), S.ColSpec("g", 1000),
            S.ColSpec("g1", 300), S.ColSpec("g2", 300)]
    wl = S.Workload("sparse_sets", "set functions GROUP BY g1, g2", args.segments, args.rows, cols, "", 11, "weak")
    ctx = E.Context(0)
    L = N.lib()
    print("# staging %d segments x %d rows ..." % (args.segments, args.rows), file=sys.stderr, flush=True)
    dev = S.DeviceSegments(ctx, wl, list(range(args.segments)), rows=args.rows)
    segs = dev.segments
    c5 = " WHERE (f1 IN (%s) OR f2 = 7) AND f3 <> 3" % ",".join(str(v) for v in range(3, 1000, 31)[:32])

    def window(fn, steps, warmup):
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

    def step_of(q, flags):
        def step():
            r = q.execute(segs, flags)
            try:
                st = (C.c_int64 * 4)()
                N.check(L.pgx_result_stats(r, st))
                ng = C.c_int64(0)
                N.check(L.pgx_result_num_groups(r, C.byref(ng)))
                return list(st), ng.value
            finally:
                L.pgx_result_release(r)
        return step

    def request(fam, flt, gcols):
        fn, col = FAMILIES[fam][:2]
        q = pql.compile("SELECT COUNT(*) FROM T%s GROUP BY %s" % (flt, gcols))
        return {"aggregations": [{"fn": fn, "column": col}], "group_by": q["group_by"], "filter": q.get("filter")}

    results = []
    for fam in args.families.split(","):
        fn, col, pfn, dense_kernel = FAMILIES[fam]
        for fname, flt in (("c5_filter", c5), ("match_all", "")):
            q = E._Query(ctx, request(fam, flt, "g1, g2"))
            gpu, wall, per, (st, groups) = window(step_of(q, N.PGX_X_SPARSE_GROUP_SETS), args.steps, args.warmup)
            q.close()
            row = {"case": "sparse", "family": fam, "filter": fname, "group_by": "g1, g2", "docs_selected": st[0],
                   "groups": groups, "native_ms": round(gpu, 4), "native_wall_ms": round(wall, 3),
                   "dir_build_ms": round(per.get("pgx_sel_dir_build", 0.0), 4),
                   "group_kernel_ms": round(per.get(dense_kernel + "_sparse", 0.0), 4), "steps": args.steps,
                   "warmup": args.warmup, "kernels_ms_per_step": {n: round(v, 4) for n, v in sorted(per.items())}}
            if args.decomp_steps > 0 and st[0] <= args.decomp_max_docs:
                print("# %s %s: decomposition ..." % (fam, fname), file=sys.stderr, flush=True)
                preq = pql.compile("SELECT %s(%s) FROM T%s GROUP BY g1, g2" % (pfn, col, flt))
                pm = E.InstancePlanMakerImplV2(ctx)
                os.environ["PGX_SPARSE_SETS_NATIVE"] = "0"
                try:
                    d_ms, d_wall, _, _ = window(lambda: pm.make_inter_segment_plan(segs, preq).execute(),
                                                args.decomp_steps, 0)
                finally:
                    del os.environ["PGX_SPARSE_SETS_NATIVE"]
                os.environ["PGX_SPARSE_SETS_NATIVE"] = "1"  # the sparse route through the same door
                try:
                    o_ms, o_wall, _, _ = window(lambda: pm.make_inter_segment_plan(segs, preq).execute(), 1, 0)
                finally:
                    del os.environ["PGX_SPARSE_SETS_NATIVE"]
                row.update({"decomp_gpu_ms": round(d_ms, 4), "decomp_wall_ms": round(d_wall, 1),
                            "decomp_steps": args.decomp_steps, "plan_maker_native_gpu_ms": round(o_ms, 4),
                            "plan_maker_native_wall_ms": round(o_wall, 1)})
            else:
                row.update({"decomp_gpu_ms": None, "decomp_wall_ms": None, "decomp_steps": 0,
                            "decomp_skipped": "not run: selects %d docs under GROUP BY (minutes per step)" % st[0]})
            results.append(row)
            print(json.dumps(row), flush=True)
        # the same key space through the multiply-add and through the directory
        for fname, flt in (("c5_filter", c5), ("match_all", "")):
            runs = []
            for how, flags in (("dense", 0), ("dense", 0), ("sparse", N.PGX_X_FORCE_HASH | N.PGX_X_SPARSE_GROUP_SETS)):
                q = E._Query(ctx, request(fam, flt, "g"))
                gpu, wall, per, (st, groups) = window(step_of(q, flags), args.steps, args.warmup)
                q.close()
                k = per.get(dense_kernel + ("_sparse" if how == "sparse" else ""), 0.0)
                runs.append((how, gpu, wall, k, groups, st[0], per))
            d1, d2, sp = runs
            spread = abs(d1[3] - d2[3]) / max(min(d1[3], d2[3]), 1e-9)
            row = {"case": "dense_vs_sparse", "family": fam, "filter": fname, "group_by": "g", "docs_selected": sp[5],
                   "groups": sp[4], "dense_group_kernel_ms": [round(d1[3], 4), round(d2[3], 4)],
                   "dense_spread": round(spread, 4), "sparse_group_kernel_ms": round(sp[3], 4),
                   "sparse_over_dense": round(sp[3] / max(d1[3], d2[3], 1e-9), 3),
                   "dense_native_ms": [round(d1[1], 4), round(d2[1], 4)], "sparse_native_ms": round(sp[1], 4),
                   "dense_wall_ms": [round(d1[2], 3), round(d2[2], 3)], "sparse_wall_ms": round(sp[2], 3),
                   "steps": args.steps, "warmup": args.warmup,
                   "sparse_kernels_ms_per_step": {n: round(v, 4) for n, v in sorted(sp[6].items())}}
            results.append(row)
            print(json.dumps(row), flush=True)
    dev.free()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
