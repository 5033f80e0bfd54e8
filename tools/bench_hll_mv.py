#!/usr/bin/env python3
"""DISTINCTCOUNTHLLMV on a multi-value column: the native path (registers built on the device, pgx_hll.hip
pgx_hll_offer_mv[_group]) next to the host decomposition it replaces.

--segments x --docs docs built on the host (defaults 8 x 250,000: about 5 M values, some seconds to build): a
multi-value INT column c with 1..4 values per doc drawn from 2^20 values, a single-value g with 1000 values and a
single-value f with 1000 values for the filter.  Cases: match-all and the selective filter f < 10 (1% of the docs),
each aggregation-only and GROUP BY g.  GPU figures are kernel time from the library's timing window (pgx_timing_start /
pgx_timing_stop: the union of the launches' busy intervals per step), after warm-up:
  native_ms     the DISTINCTCOUNTHLLMV(c) step: the scan writing selection bits, then pgx_hll_offer_mv[_group]
  offer_ms      pgx_hll_offer_mv[_group] alone, against its byte floor: the mask words, the start entries of the
                selected docs, the selected values' bits of c and the selected docs' bits of g, over the MI355X's
                measured HBM copy rate (6.29 TB/s)
  decomp_*      the same request through the plan maker with PGX_HLL_NATIVE=0 (the GROUP BY [g,] c histogram over the
                multi-value column read back and hashed per value in Python): GPU time and wall time per step.  It runs
                --decomp-steps times, and not at all under GROUP BY when the filter selects more than --decomp-max-docs
                docs (every distinct (g, value) pair becomes a Python string there: minutes per step).
Prints one JSON line per case and writes them all to --out.

  python tools/bench_hll_mv.py --out profiles/hll/bench_hll_mv.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12  # MI355X HBM3E as measured by a float4 copy; the spec peak is 8.0 TB/s


def mv_column(S, np, name, values, lens):
    """segment.make_mv_column for an INT column given as flat values and per-doc counts, without per-doc lists."""
    dictionary, ids = np.unique(values.astype(np.int32), return_inverse=True)
    card, n = len(dictionary), len(lens)
    bits = S.num_bits(card)
    starts = np.concatenate([[0], np.cumsum(lens)])
    tv = int(starts[-1])
    dpc = S.mv_docs_per_chunk(n, tv)
    nchunks = (n + dpc - 1) // dpc
    head = starts[np.arange(nchunks) * dpc].astype(">i4").tobytes()
    bitset = np.zeros((tv + 7) // 8 * 8, dtype=np.uint8)
    bitset[starts[:-1]] = 1
    bs = np.packbits(bitset).tobytes()[:(tv + 7) // 8]
    raw = S.pack_fixed_bit(ids.astype(np.int64), bits)[:(tv * bits + 7) // 8]
    return S.Column(name, "INT", "DIMENSION", card, bits, n, n, False, False, dictionary.astype(">i4").tobytes(), 4,
                    head + bs + raw, None, None, S.DEFAULT_PAD, True, tv, int(lens.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--docs", type=int, default=250_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--decomp-steps", type=int, default=1)
    ap.add_argument("--decomp-max-docs", type=int, default=200_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    from pinot_amd import engine as E
    from pinot_amd import native as N
    from pinot_amd import pql
    from pinot_amd import segment as S

    ctx = E.Context(0)
    L = N.lib()
    t0 = time.perf_counter()
    segs, host = [], []
    for i in range(args.segments):
        rng = np.random.default_rng(1000 + i)
        lens = rng.integers(1, 5, args.docs).astype(np.int64)
        vals = rng.integers(0, 1 << 20, int(lens.sum()))
        g = rng.integers(0, 1000, args.docs).astype(np.int32)
        f = rng.integers(0, 1000, args.docs).astype(np.int32)
        cols = [mv_column(S, np, "c", vals, lens), S.make_column("g", g), S.make_column("f", f)]
        seg = S.make_segment("hllmv%d" % i, cols)
        host.append((lens, f, seg.columns["c"].bits, seg.columns["g"].bits))
        segs.append(E.IndexSegment(ctx, seg))
    build_s = time.perf_counter() - t0
    print("# built and staged %d segments x %d docs in %.1f s" % (args.segments, args.docs, build_s), file=sys.stderr,
          flush=True)
    total_docs = args.segments * args.docs
    total_values = int(sum(int(h[0].sum()) for h in host))
    mask_bytes = args.segments * ((args.docs + 31) // 32) * 4

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

    results = []
    for fname, flt, pred in (("f_lt_10", " WHERE f < 10", lambda f: f < 10),
                             ("match_all", "", lambda f: np.ones(len(f), bool))):
        sel_docs = sum(int(pred(f).sum()) for _, f, _, _ in host)
        sel_values = sum(int(lens[pred(f)].sum()) for lens, f, _, _ in host)
        for grouped in (False, True):
            gb = " GROUP BY g" if grouped else ""
            request = pql.compile("SELECT DISTINCTCOUNTHLLMV(c) FROM T" + flt + gb)
            hq = E._Query(ctx, request)
            native_ms, native_wall, per, (hstats, regs) = window(query_step(hq, grouped), args.steps, args.warmup)
            hq.close()
            assert hstats[0] == sel_docs, (hstats, sel_docs)
            kname = "pgx_hll_offer_mv_group" if grouped else "pgx_hll_offer_mv"
            offer_ms = per.get(kname)
            floor_bits = sum(int(lens[pred(f)].sum()) * cb + (int(pred(f).sum()) * gbits if grouped else 0)
                             for lens, f, cb, gbits in host)
            floor_bytes = mask_bytes + 4 * sel_docs + (floor_bits + 7) // 8
            floor_ms = 1e3 * floor_bytes / HBM_BYTES_PER_S
            row = {"case": fname, "group_by": grouped, "segments": args.segments, "docs_per_segment": args.docs,
                   "total_docs": total_docs, "total_values": total_values, "docs_selected": sel_docs,
                   "values_selected": sel_values, "groups": int(len(regs)), "host_build_s": round(build_s, 1),
                   "native_ms": round(native_ms, 4), "native_wall_ms": round(native_wall, 3),
                   "offer_ms": None if offer_ms is None else round(offer_ms, 4),
                   "offer_floor_bytes": floor_bytes, "offer_floor_ms": round(floor_ms, 5),
                   "offer_over_floor": None if not offer_ms else round(offer_ms / floor_ms, 1),
                   "hbm_bytes_per_s": HBM_BYTES_PER_S, "steps": args.steps, "warmup": args.warmup,
                   "kernels_ms_per_step": {n: round(v, 4) for n, v in sorted(per.items())},
                   "note": "one run on one MI355X"}
            # the decomposition on the same build: the parent commit's behaviour
            if args.decomp_steps > 0 and not (grouped and sel_docs > args.decomp_max_docs):
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
                assert blk.stats.as_list() == on.stats.as_list() == hstats
                row.update({"decomp_gpu_ms": round(d_ms, 4), "decomp_wall_ms": round(d_wall, 1),
                            "decomp_steps": args.decomp_steps, "decomp_registers_equal": True,
                            "decomp_kernels_ms_per_step": {n: round(v, 4) for n, v in sorted(dper.items())}})
            else:
                row.update({"decomp_gpu_ms": None, "decomp_wall_ms": None, "decomp_steps": 0,
                            "decomp_skipped": "selects %d docs under GROUP BY: every distinct (g, value) pair becomes "
                                              "a Python string" % sel_docs})
            results.append(row)
            print(json.dumps(row), flush=True)
    for s in segs:
        s.destroy()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
