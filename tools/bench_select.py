#!/usr/bin/env python3
"""Selection ORDER BY on synthetic device columns: what the top-K costs next to the scan that feeds it.

64 segments x 2M rows (pgx_synth_column), a 20-bit and a 10-bit order column, the C5-style filter
((f1 IN 32 ids OR f2 = 7) AND f3 <> 3, bitmap inverted indexes) and match-all, K = 10 and K = 1000.  Every figure is GPU
kernel time from the library's timing window (pgx_timing_start / pgx_timing_stop: the union of the launches' busy
intervals per step), after warm-up:
  count_ms      the COUNT(*) step with the same filter on the same segments (what producing the mask costs)
  select_ms     the selection step (the same scan, then pgx_select_topk / _merge / _gather)
  topk_ms       pgx_select_topk alone, against its byte floor: the mask words plus the order-column bits of the rows
                it must decode (the selected ones), over the MI355X's measured HBM copy rate (6.29 TB/s)
Prints one JSON line per case and writes them all to --out.

  python tools/bench_select.py --out profiles/select/bench_select.json
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12  # MI355X HBM3E as measured by a float4 copy; the spec peak is 8.0 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from pinot_amd import engine as E
    from pinot_amd import native as N
    from pinot_amd import pql
    from pinot_amd import synth as S

    cols = [S.ColSpec("f1", 1000, inverted=True), S.ColSpec("f2", 100, inverted=True), S.ColSpec("f3", 10, inverted=True),
            S.ColSpec("o1", 1 << 20), S.ColSpec("o2", 1 << 10)]
    wl = S.Workload("sel", "selection ORDER BY o1, o2 DESC", args.segments, args.rows, cols, "", 9, "weak")
    ctx = E.Context(0)
    L = N.lib()
    dev = S.DeviceSegments(ctx, wl, list(range(args.segments)), rows=args.rows)
    segs = dev.segments
    c5 = " WHERE (f1 IN (%s) OR f2 = 7) AND f3 <> 3" % ",".join(str(v) for v in range(3, 1000, 31)[:32])
    order_bits = sum(c.bits for c in cols if c.name in ("o1", "o2"))
    total_rows = args.segments * args.rows
    mask_bytes = args.segments * ((args.rows + 31) // 32) * 4

    def timed(q):
        """Kernel time per step (ms) and the per-kernel sums of the window, after warm-up."""
        def step():
            r = q.execute(segs)
            st = (C.c_int64 * 4)()
            N.check(L.pgx_result_stats(r, st))
            L.pgx_result_release(r)
            return list(st)
        for _ in range(args.warmup):
            stats = step()
        out = (C.c_double * 3)()
        js = C.create_string_buffer(1 << 16)
        N.check(L.pgx_timing_start(ctx.handle))
        for _ in range(args.steps):
            step()
        N.check(L.pgx_timing_stop(ctx.handle, out, js, len(js)))
        return out[0] / args.steps, json.loads(js.value.decode()), stats

    results = []
    for fname, flt in (("c5_filter", c5), ("match_all", "")):
        cq = E._Query(ctx, pql.compile("SELECT COUNT(*) FROM T" + flt))
        count_ms, _, cstats = timed(cq)
        cq.close()
        for k in (10, 1000):
            sq = E._SelectQuery(ctx, pql.compile("SELECT f2 FROM T%s ORDER BY o1, o2 DESC LIMIT %d" % (flt, k)))
            select_ms, detail, sstats = timed(sq)
            sq.close()
            assert sstats[0] == cstats[0] and sstats[1] == cstats[1], (sstats, cstats)
            kern = detail.get("kernels", detail)
            per = {name: v[1] / args.steps for name, v in kern.items() if isinstance(v, list) and len(v) == 2}
            floor_bytes = mask_bytes + (sstats[0] * order_bits + 7) // 8
            floor_ms = 1e3 * floor_bytes / HBM_BYTES_PER_S
            topk_ms = per.get("pgx_select_topk")
            row = {"case": fname, "k": k, "segments": args.segments, "rows_per_segment": args.rows,
                   "total_rows": total_rows, "docs_selected": sstats[0], "count_ms": round(count_ms, 4),
                   "select_ms": round(select_ms, 4), "topk_ms": None if topk_ms is None else round(topk_ms, 4),
                   "merge_ms": per.get("pgx_select_merge"), "gather_ms": per.get("pgx_select_gather"),
                   "topk_floor_bytes": floor_bytes, "topk_floor_ms": round(floor_ms, 4),
                   "topk_over_floor": None if not topk_ms else round(topk_ms / floor_ms, 2),
                   "hbm_bytes_per_s": HBM_BYTES_PER_S, "steps": args.steps, "warmup": args.warmup,
                   "kernels_ms_per_step": {n: round(v, 4) for n, v in sorted(per.items())}}
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
