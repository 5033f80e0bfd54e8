#!/usr/bin/env python3
"""FASTHLL on host-built segments: the native path (presence bits marked and the dictionaries' register images folded
on the device, pgx_fasthll.hip) next to the host decomposition it replaces (PGX_FASTHLL_NATIVE=0).

8 segments x 500,000 rows; h is a STRING column over pools of 4,096 serialized estimators (segments alternate between
two pools, so two dictionaries fold into every group's registers), g has 1,000 values, the C5-style filter is
((f1 IN 32 ids OR f2 = 7) AND f3 <> 3, bitmap inverted indexes).  Match-all and the filter, aggregation-only and
GROUP BY g.  GPU figures are kernel time from the library's timing window (pgx_timing_start / pgx_timing_stop), after
warm-up:
  native_ms     the FASTHLL(h) step: the scan writing selection bits, the marks, the fold, the narrowing
  mark_ms       pgx_distinct_mark[_group] alone
  fold_ms       pgx_fasthll_fold alone, against its byte floor: the bitmaps' words plus 256 bytes per distinct
                (group, dictId) pair, over the MI355X's measured HBM copy rate (6.29 TB/s)
  native_wall   wall time per step of the request through the plan maker, natively
  decomp_*      the same with PGX_FASTHLL_NATIVE=0 (the GROUP BY [g,] h histogram read back, every distinct string
                deserialized and merged in Python): GPU time and wall time per step.  It runs --decomp-steps times, and
                not at all when more than --decomp-max-pairs distinct (group, value) pairs would cross to Python.
Prints one JSON line per case and writes them all to --out.

  python tools/bench_fasthll.py --out profiles/fasthll/bench_fasthll.json
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
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--rows", type=int, default=500_000)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--decomp-steps", type=int, default=1)
    ap.add_argument("--decomp-max-pairs", type=int, default=400_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    from pinot_amd import engine as E
    from pinot_amd import hll as HLL
    from pinot_amd import native as N
    from pinot_amd import pql
    from pinot_amd import segment as S

    rng = np.random.default_rng(11)
    pools = []
    for _ in range(2):
        regs = np.minimum(rng.geometric(0.5, (args.pool, 256)), 25).astype(np.uint8)
        regs[rng.random((args.pool, 256)) < 0.3] = 0
        strs = [HLL.to_string(r) for r in regs]
        width = max(len(s.encode("utf-8")) for s in strs)
        pools.append(S._java_string_sort(sorted(set(strs)), width, S.DEFAULT_PAD))
    ctx = E.Context(0)
    L = N.lib()
    print("# building %d segments x %d rows ..." % (args.segments, args.rows), file=sys.stderr, flush=True)
    segs, raws = [], []
    for i in range(args.segments):
        n = args.rows
        pool = pools[i % 2]
        raw = {"f1": rng.integers(0, 1000, n).astype(np.int32), "f2": rng.integers(0, 100, n).astype(np.int32),
               "f3": rng.integers(0, 10, n).astype(np.int32), "g": rng.integers(0, 1000, n).astype(np.int32),
               "h": rng.integers(0, len(pool), n)}
        cols = [S.make_column(c, raw[c], inverted=c != "g") for c in ("f1", "f2", "f3", "g")]
        cols.append(S.make_column("h", None, data_type="STRING", dictionary=pool, dict_ids=raw["h"]))
        segs.append(E.IndexSegment(ctx, S.make_segment("fh%d" % i, cols)))
        raws.append(raw)
    in_ids = list(range(3, 1000, 31))[:32]
    c5 = " WHERE (f1 IN (%s) OR f2 = 7) AND f3 <> 3" % ",".join(str(v) for v in in_ids)

    def c5_mask(r):
        return (np.isin(r["f1"], in_ids) | (r["f2"] == 7)) & (r["f3"] != 3)

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

    def query_step(q, grouped):
        def step():
            r = q.execute(segs)
            try:
                st = (C.c_int64 * 4)()
                N.check(L.pgx_result_stats(r, st))
                ng = C.c_int64(1)
                if grouped:
                    N.check(L.pgx_result_num_groups(r, C.byref(ng)))
                return list(st), E.result_hll(r, 0, 0, ng.value)
            finally:
                L.pgx_result_release(r)
        return step

    pm = E.InstancePlanMakerImplV2(ctx)
    results = []
    for fname, flt, mask in (("match_all", "", lambda r: np.ones(len(r["g"]), bool)), ("c5_filter", c5, c5_mask)):
        for grouped in (False, True):
            gb = " GROUP BY g" if grouped else ""
            request = pql.compile("SELECT FASTHLL(h) FROM T" + flt + gb)
            # the distinct (group, dictId) pairs per dictionary, and the bitmaps' words: the fold's byte floor
            pairs, rows = 0, 1
            for d in range(2):
                keys = [((r["g"].astype(np.int64) if grouped else 0) * len(pools[d]) + r["h"])[mask(r)]
                        for i, r in enumerate(raws) if i % 2 == d]
                if keys:
                    pairs += len(np.unique(np.concatenate(keys)))
            hq = E._Query(ctx, request)
            native_ms, _, per, (hstats, regs) = window(query_step(hq, grouped), args.steps, args.warmup)
            hq.close()
            rows = len(regs)
            ndict = min(2, args.segments)
            bitmap_bytes = sum(((len(pools[d]) + 31) // 32) * 4 for d in range(ndict)) * (1000 if grouped else 1)
            floor_bytes = bitmap_bytes + 256 * pairs
            floor_ms = 1e3 * floor_bytes / HBM_BYTES_PER_S
            fold_ms = per.get("pgx_fasthll_fold")
            mark_ms = per.get("pgx_distinct_mark_group" if grouped else "pgx_distinct_mark")
            _, native_wall, _, on = window(lambda: pm.make_inter_segment_plan(segs, request).execute(), args.steps,
                                           args.warmup)
            row = {"case": fname, "group_by": grouped, "segments": args.segments, "rows_per_segment": args.rows,
                   "pool": args.pool, "docs_selected": hstats[0], "groups": int(rows), "pairs": int(pairs),
                   "native_ms": round(native_ms, 4), "native_wall_ms": round(native_wall, 3),
                   "mark_ms": None if mark_ms is None else round(mark_ms, 4),
                   "fold_ms": None if fold_ms is None else round(fold_ms, 4),
                   "fold_floor_bytes": floor_bytes, "fold_floor_ms": round(floor_ms, 5),
                   "fold_over_floor": None if not fold_ms else round(fold_ms / floor_ms, 1),
                   "hbm_bytes_per_s": HBM_BYTES_PER_S, "steps": args.steps, "warmup": args.warmup,
                   "kernels_ms_per_step": {n: round(v, 4) for n, v in sorted(per.items())}}
            if args.decomp_steps > 0 and pairs <= args.decomp_max_pairs:
                print("# %s%s: decomposition ..." % (fname, gb), file=sys.stderr, flush=True)
                os.environ["PGX_FASTHLL_NATIVE"] = "0"
                try:
                    d_ms, d_wall, dper, blk = window(lambda: pm.make_inter_segment_plan(segs, request).execute(),
                                                     args.decomp_steps, 0)
                finally:
                    del os.environ["PGX_FASTHLL_NATIVE"]
                if grouped:
                    mon = on.get_aggregation_group_by_result().as_map()
                    moff = blk.get_aggregation_group_by_result().as_map()
                    same = set(mon) == set(moff) and len(mon) == len(regs) and all(
                        np.array_equal(mon[k][0], moff[k][0]) for k in mon)
                else:
                    same = np.array_equal(blk.get_aggregation_result()[0], regs[0]) and np.array_equal(
                        on.get_aggregation_result()[0], regs[0])
                assert same, "native and decomposed registers differ"
                assert blk.stats.as_list() == on.stats.as_list()
                row.update({"decomp_gpu_ms": round(d_ms, 4), "decomp_wall_ms": round(d_wall, 1),
                            "decomp_steps": args.decomp_steps, "decomp_registers_equal": True,
                            "decomp_kernels_ms_per_step": {n: round(v, 4) for n, v in sorted(dper.items())}})
            else:
                row.update({"decomp_gpu_ms": None, "decomp_wall_ms": None, "decomp_steps": 0,
                            "decomp_skipped": "%d distinct (g, h) pairs would each be deserialized in Python" % pairs})
            results.append(row)
            print(json.dumps(row), flush=True)
            if args.out:  # (after every case: a run cut short keeps what it measured)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(results, f, indent=1)
                    f.write("\n")
    for s in segs:
        s.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
