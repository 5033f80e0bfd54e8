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

--mv adds one multi-value column (10-bit dictIds, 1 .. 5 values per doc, 3 on average, the same content in every
segment) to the same shape and times, beside each single-value row, the selection that also returns that column
(PGX_Q_SELECT_MV): its step, the three pgx_select_mv_* launches, and the bytes that cross to the host.

--no-order-by times the selection without ORDER BY (PGX_Q_SELECT_ONLY, pgx_select_first) on the same segments instead:
`SELECT f1, f2 FROM T WHERE o2 < 64 LIMIT 10` (one scan leaf: the filter statistic's class b), its ORDER BY o1, o2 DESC
twin and the same filter as COUNT(*), one step of each in turn, round after round; and the form without a filter on the
segments and on a second set of an eighth of the rows.  Per query: the median of the steps' wall times (a step ends with
the result's statistics on the host), their spread (10th and 90th percentile, minimum and maximum) and the kernel time
per step from the library's timing window.  Then pgx_select_first's kernel time with one workgroup per segment and
with run_select's own choice (PGX_DEBUG firstg=N, read when the query is compiled), over a mask it leaves early
(o2 < 64) and one it walks to the end (o1 < 2: fewer matches than the limit), on all segments and on one.

  python tools/bench_select.py --out profiles/select/bench_select.json
  python tools/bench_select.py --mv --out profiles/select_mv/bench_select_mv.json
  python tools/bench_select.py --no-order-by --out profiles/select_only/bench_select_only.json
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12  # MI355X HBM3E as measured by a float4 copy; the spec peak is 8.0 TB/s


def mv_column(name, rows, card=1000, seed=5):
    """A multi-value INT column of `rows` docs in the v1 format (segment.pack_mv_fwd, without a list per doc): doc d
    holds 1 + d % 5 values, dictIds uniform below card."""
    import numpy as np

    from pinot_amd import segment as S
    lens = 1 + np.arange(rows, dtype=np.int64) % 5
    starts = np.concatenate([[0], np.cumsum(lens)])
    tv = int(starts[-1])
    bits = S.num_bits(card)
    dpc = S.mv_docs_per_chunk(rows, tv)
    head = starts[np.arange((rows + dpc - 1) // dpc) * dpc].astype(">i4").tobytes()
    first = np.zeros((tv + 7) // 8 * 8, dtype=np.uint8)
    first[starts[:-1]] = 1
    ids = np.random.default_rng(seed).integers(0, card, tv).astype(np.int64)
    fwd = head + np.packbits(first).tobytes()[:(tv + 7) // 8] + \
        S.pack_fixed_bit_chunked(ids, bits)[:(tv * bits + 7) // 8]
    return S.Column(name, "INT", "DIMENSION", card, bits, rows, rows, False, False,
                    np.arange(card).astype(">i4").tobytes(), 4, fwd, None, None, S.DEFAULT_PAD, True, tv, 5)


def no_order_by(args):
    """The --no-order-by mode (module docstring)."""
    import time

    import numpy as np

    from pinot_amd import engine as E
    from pinot_amd import native as N
    from pinot_amd import pql
    from pinot_amd import synth as S

    cols = [S.ColSpec("f1", 1000, inverted=True), S.ColSpec("f2", 100, inverted=True), S.ColSpec("f3", 10, inverted=True),
            S.ColSpec("o1", 1 << 20), S.ColSpec("o2", 1 << 10)]
    wl = S.Workload("sel", "selection without ORDER BY", args.segments, args.rows, cols, "", 9, "weak")
    ctx = E.Context(0)
    L = N.lib()
    flt = " WHERE o2 < 64"
    results = []

    def compiled(text, firstg=None):
        """The query for `text`; firstg: workgroups per segment of pgx_select_first (PGX_DEBUG is read at compile)."""
        old = os.environ.get("PGX_DEBUG")
        if firstg is not None:
            os.environ["PGX_DEBUG"] = "firstg=%d" % firstg
        try:
            req = pql.compile(text)
            return E._SelectQuery(ctx, req, flags=N.PGX_Q_SELECT_ONLY) if req.get("selections") else E._Query(ctx, req)
        finally:
            if firstg is not None:
                if old is None:
                    del os.environ["PGX_DEBUG"]
                else:
                    os.environ["PGX_DEBUG"] = old

    def step(q, segs):
        t0 = time.perf_counter()
        r = q.execute(segs)
        st = (C.c_int64 * 4)()
        N.check(L.pgx_result_stats(r, st))
        dt = time.perf_counter() - t0
        L.pgx_result_release(r)
        return 1e3 * dt, list(st)

    def rounds(queries, segs):
        """{name: (wall times in ms, one per round, the queries taking turns; statistics; kernel ms per step by name)}"""
        for _ in range(args.warmup):
            for q in queries.values():
                step(q, segs)
        wall = {name: [] for name in queries}
        stats = {}
        for _ in range(args.steps):
            for name, q in queries.items():
                ms, stats[name] = step(q, segs)
                wall[name].append(ms)
        kern = {}
        for name, q in queries.items():  # kernel times in a window of their own
            out = (C.c_double * 3)()
            js = C.create_string_buffer(1 << 16)
            N.check(L.pgx_timing_start(ctx.handle))
            for _ in range(args.steps):
                step(q, segs)
            N.check(L.pgx_timing_stop(ctx.handle, out, js, len(js)))
            detail = json.loads(js.value.decode())
            detail = detail.get("kernels", detail)
            kern[name] = (out[0] / args.steps, {k: round(v[1] / args.steps, 5) for k, v in sorted(detail.items())
                                                if isinstance(v, list) and len(v) == 2})
        return {name: (wall[name], stats[name], kern[name]) for name in queries}

    def summary(case, name, segs, rows, res):
        wall, stats, (kernel_ms, per) = res
        w = np.sort(np.asarray(wall))
        row = {"case": case, "query": name, "segments": len(segs), "rows_per_segment": rows, "stats": stats,
               "wall_ms_median": round(float(np.median(w)), 4), "wall_ms_p10": round(float(np.percentile(w, 10)), 4),
               "wall_ms_p90": round(float(np.percentile(w, 90)), 4), "wall_ms_min": round(float(w[0]), 4),
               "wall_ms_max": round(float(w[-1]), 4), "kernel_ms_per_step": round(kernel_ms, 4),
               "kernels_ms_per_step": per, "steps": args.steps, "warmup": args.warmup}
        results.append(row)
        print(json.dumps(row), flush=True)

    sets = []
    for rows in (args.rows, max(1, args.rows // 8)):
        dev = S.DeviceSegments(ctx, wl, list(range(args.segments)), rows=rows)
        sets.append((rows, dev))
    rows, dev = sets[0]
    segs = dev.segments
    texts = {"select_only": "SELECT f1, f2 FROM T%s LIMIT 10" % flt,
             "select_order_by": "SELECT f1, f2 FROM T%s ORDER BY o1, o2 DESC LIMIT 10" % flt,
             "count": "SELECT COUNT(*) FROM T%s" % flt}
    queries = {name: compiled(t) for name, t in texts.items()}
    for name, res in rounds(queries, segs).items():
        summary("scan_leaf_filter", name, segs, rows, res)
    for q in queries.values():
        q.close()
    # the form without a filter, on both sets: its time must not grow with the segments' rows
    q = compiled("SELECT f1, f2 FROM T LIMIT 10")
    for rows_i, dev_i in sets:
        for name, res in rounds({"select_only": q}, dev_i.segments).items():
            summary("no_filter", name, dev_i.segments, rows_i, res)
    q.close()
    # pgx_select_first alone: one workgroup per segment against run_select's choice
    for fname, f in (("early_exit", flt), ("walks_whole_mask", " WHERE o1 < 2")):
        for nseg in (len(segs), 1):
            for firstg in (1, 0):
                q = compiled("SELECT f1, f2 FROM T%s LIMIT 10" % f, firstg=firstg)
                res = rounds({"select_only": q}, segs[:nseg])["select_only"]
                q.close()
                per = res[2][1]
                row = {"case": "first_kernel_" + fname, "segments": nseg, "rows_per_segment": rows,
                       "workgroups_per_segment": "1" if firstg == 1 else "auto", "docs_found": res[1][0],
                       "first_ms": per.get("pgx_select_first"), "first_count_ms": per.get("pgx_select_first_count"),
                       "kernel_ms_per_step": round(res[2][0], 4), "wall_ms_median": round(float(np.median(res[0])), 4),
                       "steps": args.steps, "warmup": args.warmup}
                results.append(row)
                print(json.dumps(row), flush=True)
    for _, dev_i in sets:
        dev_i.free()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"command": " ".join(["python", "tools/bench_select.py"] + sys.argv[1:]), "results": results}, f,
                      indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mv", action="store_true", help="also select one multi-value column of about 3 values per doc")
    ap.add_argument("--no-order-by", action="store_true",
                    help="time the selection without ORDER BY against its ORDER BY twin and COUNT(*)")
    args = ap.parse_args()
    if args.no_order_by:
        return no_order_by(args)

    from pinot_amd import engine as E
    from pinot_amd import native as N
    from pinot_amd import pql
    from pinot_amd import synth as S

    cols = [S.ColSpec("f1", 1000, inverted=True), S.ColSpec("f2", 100, inverted=True), S.ColSpec("f3", 10, inverted=True),
            S.ColSpec("o1", 1 << 20), S.ColSpec("o2", 1 << 10)]
    wl = S.Workload("sel", "selection ORDER BY o1, o2 DESC", args.segments, args.rows, cols, "", 9, "weak")
    ctx = E.Context(0)
    L = N.lib()
    dev = S.DeviceSegments(ctx, wl, list(range(args.segments)), rows=args.rows,
                           extra=[mv_column("mv", args.rows)] if args.mv else ())
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
            if args.mv:
                mq = E._SelectQuery(ctx, pql.compile("SELECT f2, mv FROM T%s ORDER BY o1, o2 DESC LIMIT %d" % (flt, k)),
                                    flags=N.PGX_Q_SELECT_MV)
                mv_ms, mdetail, mstats = timed(mq)
                r = mq.execute(segs)
                _, names, _, lists = E.decode_selection(mq, r, segs)
                L.pgx_result_release(r)
                mq.close()
                assert mstats[:2] == sstats[:2] and names == ["o1", "o2", "f2", "mv"], (mstats, names)
                nrows = sum(len(x) for x in lists)
                values = sum(len(rw[0][3]) for x in lists for rw in x)
                mkern = mdetail.get("kernels", mdetail)
                mper = {name: v[1] / args.steps for name, v in mkern.items() if isinstance(v, list) and len(v) == 2}
                # what run_select copies to the host: counts, docIds, the single-value dictIds; per (column, segment) the
                # K + 1 offsets and a base, the grand total; the selected values
                row["mv"] = {"select_ms": round(mv_ms, 4), "rows": nrows, "values": values,
                             "offsets_ms": mper.get("pgx_select_mv_offsets"), "bases_ms": mper.get("pgx_select_mv_bases"),
                             "gather_ms": mper.get("pgx_select_mv_gather"),
                             "bytes_returned": args.segments * (4 + k * 4 * 4 + (k + 1) * 4 + 8) + 8 + values * 4,
                             "bytes_returned_single_value": args.segments * (4 + k * 4 * 4),
                             "kernels_ms_per_step": {n: round(v, 4) for n, v in sorted(mper.items())}}
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
