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

  python tools/bench_select.py --out profiles/select/bench_select.json
  python tools/bench_select.py --mv --out profiles/select_mv/bench_select_mv.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mv", action="store_true", help="also select one multi-value column of about 3 values per doc")
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
