#!/usr/bin/env python3
"""DISTINCTCOUNTHLL on synthetic device columns: the native path (registers built on the device, pgx_hll.hip) next to
the scan that feeds it and next to the host decomposition it replaces.

64 segments x 2M rows (pgx_synth_column), c with 2^20 distinct values (20 bits), g with 1000, the C5-style filter
((f1 IN 32 ids OR f2 = 7) AND f3 <> 3, bitmap inverted indexes) and match-all, aggregation-only and GROUP BY g.  GPU
figures are kernel time from the library's timing window (pgx_timing_start / pgx_timing_stop: the union of the
launches' busy intervals per step), after warm-up:
  count_ms      the COUNT(*) step with the same filter (and GROUP BY) on the same segments
  native_ms     the DISTINCTCOUNTHLL(c) step: the same scan writing selection bits, then pgx_hll_offer[_group]
  offer_ms      pgx_hll_offer[_group] alone, against its byte floor: the mask words plus the selected rows' bits of c
                (and of g), over the MI355X's measured HBM copy rate (6.29 TB/s)
  decomp_*      the same request through the plan maker with PGX_HLL_NATIVE=0 (the GROUP BY [g,] c histogram read back
                and hashed per value in Python): GPU time and wall time per step.  It runs --decomp-steps times, and
                not at all when the filter selects more than --decomp-max-docs rows under GROUP BY (every distinct
                (g, c) pair becomes a Python string there: minutes per step).
Prints one JSON line per case and writes them all to --out.

  python tools/bench_hll.py --out profiles/hll/bench_hll.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12  # MI355X HBM3E as measured by a float4 copy; the spec peak is 8.0 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--decomp-steps", type=int, default=1)
    ap.add_argument("--decomp-max-docs", type=int, default=6_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    from pinot_amd import engine as E
    from pinot_amd import native as N
    from pinot_amd import pql
    from pinot_amd import synth as S

    cols = [S.ColSpec("f1", 1000, inverted=True), S.ColSpec("f2", 100, inverted=True), S.ColSpec("f3", 10, inverted=True),
            S.ColSpec("c", 1 << 20), S.ColSpec("g", 1000)]
    wl = S.Workload("hll", "DISTINCTCOUNTHLL(c) [GROUP BY g]", args.segments, args.rows, cols, "", 11, "weak")
    ctx = E.Context(0)
    L = N.lib()
    print("# staging %d segments x %d rows ..." % (args.segments, args.rows), file=sys.stderr, flush=True)
    dev = S.DeviceSegments(ctx, wl, list(range(args.segments)), rows=args.rows)
    segs = dev.segments
    c5 = " WHERE (f1 IN (%s) OR f2 = 7) AND f3 <> 3" % ",".join(str(v) for v in range(3, 1000, 31)[:32])
    bits = {c.name: c.bits for c in cols}
    total_rows = args.segments * args.rows
    mask_bytes = args.segments * ((args.rows + 31) // 32) * 4

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

    def query_step(q, hll_index=None, grouped=False):
        def step():
            r = q.execute(segs)
            try:
                st = (C.c_int64 * 4)()
                N.check(L.pgx_result_stats(r, st))
                regs = None
                if hll_index is not None:
                    ng = C.c_int64(1)
                    if grouped:
                        N.check(L.pgx_result_num_groups(r, C.byref(ng)))
                    regs = E.result_hll(r, hll_index, 0, ng.value)
                return list(st), regs
            finally:
                L.pgx_result_release(r)
        return step

    results = []
    for fname, flt in (("c5_filter", c5), ("match_all", "")):
        for grouped in (False, True):
            gb = " GROUP BY g" if grouped else ""
            cq = E._Query(ctx, pql.compile("SELECT COUNT(*) FROM T" + flt + gb))
            count_ms, _, _, (cstats, _) = window(query_step(cq), args.steps, args.warmup)
            cq.close()
            text = "SELECT DISTINCTCOUNTHLL(c) FROM T" + flt + gb
            request = pql.compile(text)
            hq = E._Query(ctx, request)
            native_ms, native_wall, per, (hstats, regs) = window(query_step(hq, 0, grouped), args.steps, args.warmup)
            hq.close()
            assert hstats[0] == cstats[0] and hstats[1] == cstats[1], (hstats, cstats)
            kname = "pgx_hll_offer_group" if grouped else "pgx_hll_offer"
            offer_ms = per.get(kname)
            sel_bits = bits["c"] + (bits["g"] if grouped else 0)
            floor_bytes = mask_bytes + (hstats[0] * sel_bits + 7) // 8
            floor_ms = 1e3 * floor_bytes / HBM_BYTES_PER_S
            row = {"case": fname, "group_by": grouped, "segments": args.segments, "rows_per_segment": args.rows,
                   "total_rows": total_rows, "docs_selected": hstats[0], "groups": int(len(regs)),
                   "count_ms": round(count_ms, 4), "native_ms": round(native_ms, 4),
                   "native_wall_ms": round(native_wall, 3),
                   "offer_ms": None if offer_ms is None else round(offer_ms, 4),
                   "offer_floor_bytes": floor_bytes, "offer_floor_ms": round(floor_ms, 4),
                   "offer_over_floor": None if not offer_ms else round(offer_ms / floor_ms, 2),
                   "hbm_bytes_per_s": HBM_BYTES_PER_S, "steps": args.steps, "warmup": args.warmup,
                   "kernels_ms_per_step": {n: round(v, 4) for n, v in sorted(per.items())}}
            # the decomposition on the same build: the parent commit's behaviour
            if args.decomp_steps > 0 and not (grouped and hstats[0] > args.decomp_max_docs):
                print("# %s%s: decomposition ..." % (fname, gb), file=sys.stderr, flush=True)
                os.environ["PGX_HLL_NATIVE"] = "0"
                try:
                    pm = E.InstancePlanMakerImplV2(ctx)
                    d_ms, d_wall, dper, blk = window(lambda: pm.make_inter_segment_plan(segs, request).execute(),
                                                     args.decomp_steps, 0)
                finally:
                    del os.environ["PGX_HLL_NATIVE"]
                on = pm.make_inter_segment_plan(segs, request).execute()  # the native path, through the same door
                if grouped:
                    mon = on.get_aggregation_group_by_result().as_map()
                    moff = blk.get_aggregation_group_by_result().as_map()
                    same = set(mon) == set(moff) and len(mon) == len(regs) and all(
                        np.array_equal(mon[k][0], moff[k][0]) for k in mon)
                else:
                    same = np.array_equal(blk.get_aggregation_result()[0], regs[0]) and np.array_equal(
                        on.get_aggregation_result()[0], regs[0])
                assert same, "native and decomposed registers differ"
                assert blk.stats.as_list()[:2] == hstats[:2]
                row.update({"decomp_gpu_ms": round(d_ms, 4), "decomp_wall_ms": round(d_wall, 1),
                            "decomp_steps": args.decomp_steps, "decomp_registers_equal": True,
                            "decomp_kernels_ms_per_step": {n: round(v, 4) for n, v in sorted(dper.items())}})
            else:
                row.update({"decomp_gpu_ms": None, "decomp_wall_ms": None, "decomp_steps": 0,
                            "decomp_skipped": "selects %d docs under GROUP BY: every distinct (g, c) pair becomes a "
                                              "Python string" % hstats[0]})
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
