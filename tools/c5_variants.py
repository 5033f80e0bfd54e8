"""GPU experiment harness (not a test): C5-shaped queries over the C5 segments (2M rows each) via pgx_execute_timed, one
query per process -- doc masks of other densities than the bench line's 3.75 % through the same kernel shape.
usage: VARIANT_QUERY=<name> python tools/c5_variants.py [segments] [repetitions]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pinot_amd import engine as E  # noqa: E402
from pinot_amd import native as N  # noqa: E402
from pinot_amd import pql, synth  # noqa: E402

IDS = ",".join(str(v) for v in range(3, 1000, 31)[:32])
QUERIES = {"bench": "SELECT SUM(m) FROM T WHERE (f1 IN (%s) OR f2 = 7) AND f3 <> 3 GROUP BY gk TOP 10" % IDS,  # 3.75 %
           "f3ne": "SELECT SUM(m) FROM T WHERE f3 <> 3 GROUP BY gk TOP 10",                                  # 90 %
           "f3in": "SELECT SUM(m) FROM T WHERE f3 IN (1, 2, 4) GROUP BY gk TOP 10",                          # 30 %
           "f3eq": "SELECT SUM(m) FROM T WHERE f3 = 3 GROUP BY gk TOP 10",                                   # 10 %
           "f2eq": "SELECT SUM(m) FROM T WHERE f2 = 7 GROUP BY gk TOP 10"}                                   # 1 %


def main():
    nseg = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ctx = E.Context(0)
    wl = synth.WORKLOADS["c5"]
    data = synth.DeviceSegments(ctx, wl, list(range(nseg)))
    segs = data.segments
    arr = (C.c_void_p * len(segs))(*[s.handle.value for s in segs])
    L = N.lib()
    for name in os.environ.get("VARIANT_QUERY", "bench").split(","):
        q = E._Query(ctx, pql.compile(QUERIES[name]))
        binds, keep = q.bindings(segs)
        tot, kern = C.c_double(), C.c_double()
        N.check(L.pgx_execute_timed(ctx.handle, q.handle, arr, len(segs), binds, reps, C.byref(tot), C.byref(kern), None))
        print(json.dumps({"query": name, "segments": nseg, "kernel_ms": round(kern.value, 4),
                          "total_ms": round(tot.value, 4)}), flush=True)
    data.free()
    ctx.close()


if __name__ == "__main__":
    main()
