"""DISTINCTCOUNTHLLMV on the device (PGX_DISTINCTCOUNTHLLMV, pinot_amd/csrc/pgx_hll.cpp run_hll over pgx_hll.hip
pgx_hll_offer_mv[_group]): the registers pgx_result_hll returns are compared bit for bit with hll.from_ints over the
Java hash codes of every value of the numpy-selected docs, and with the host decomposition (PGX_HLL_NATIVE=0: a
GROUP BY histogram over the multi-value column hashed in Python), statistics included.  Every comparison is exact: an
offer is a register-wise max."""
import ctypes as C

import numpy as np
import pytest

from pinot_amd import extended as X
from pinot_amd import hll as HLL
from pinot_amd import pql
from pinot_amd import segment as S

pytestmark = pytest.mark.gpu

SIZES = (1, 500, 8192 + 37)
MV_COLS = {"ti": "INT", "tl": "LONG", "td": "DOUBLE", "ts": "STRING"}
TI_PROBE = 250  # a value of ti in every segment's range


def _raw(i, n):
    """Segment i's raw columns; every multi-value column has its own dictionary per segment, the value ranges
    overlapping; 1..4 values per doc, and in the large segment one doc of 70 and one of 300 values."""
    rng = np.random.default_rng(200 + i)
    words = np.array(["w%d" % k for k in range(40 * i, 40 * i + 120)] + ["tab\there", "été", "中"])
    cnt = rng.integers(1, 5, n)
    if n > 100:
        cnt[31], cnt[n - 1] = 70, 300
    raw = {
        "ti": [(rng.integers(0, 300, c) + 100 * i).astype(np.int32).tolist() for c in cnt],
        "tl": [(rng.integers(0, 5000, c).astype(np.int64) * (1 << 20) - (1 << 34) + i).tolist() for c in cnt],
        "td": [(rng.integers(-2000, 2000, c) * 0.37 + 1e-3 * i).tolist() for c in cnt],
        "ts": [words[rng.integers(0, len(words), c)].tolist() for c in cnt],
        "ci": (rng.integers(0, 300, n) + 100 * i).astype(np.int32),
        "m": rng.integers(0, 1000, n).astype(np.int32),
        "g1": rng.permutation(np.arange(n) % 50).astype(np.int32),
        "g2": (rng.integers(0, 20 + 5 * i, n) + (0, 15, 5)[i]).astype(np.int32),
        "h": rng.permutation(np.arange(n) % 1400).astype(np.int32),                  # 50 x 1400 = 70,000 slots
    }
    return raw


@pytest.fixture(scope="module")
def env():
    from pinot_amd import engine as E
    ctx = E.Context(0)
    gsegs, raws = [], []
    for i, n in enumerate(SIZES):
        raw = _raw(i, n)
        cols = [S.make_mv_column(c, v, MV_COLS[c]) if c in MV_COLS else S.make_column(c, v) for c, v in raw.items()]
        seg = S.make_segment("hmv%d" % i, cols)
        assert seg.columns["ti"].is_mv and seg.columns["ts"].data_type == "STRING"
        gsegs.append(E.IndexSegment(ctx, seg))
        raws.append(raw)
    assert len({tuple(np.unique(np.concatenate(r["ti"]))) for r in raws}) == 3  # different dictionaries
    yield ctx, gsegs, raws
    ctx.close()


def _n(r):
    return len(r["m"])


def _has(r, col, value):
    return np.array([value in doc for doc in r[col]], bool)


# (WHERE clause, the same predicate over a segment's raw columns)
FILTERS = [
    ("", lambda r: np.ones(_n(r), bool)),
    (" WHERE m BETWEEN 100 AND 140", lambda r: (r["m"] >= 100) & (r["m"] <= 140)),
    (" WHERE ti = %d" % TI_PROBE, lambda r: _has(r, "ti", TI_PROBE)),          # a leaf on the multi-value column itself
    (" WHERE ti = %d OR m < 50" % TI_PROBE, lambda r: _has(r, "ti", TI_PROBE) | (r["m"] < 50)),
    (" WHERE m = 123456", lambda r: np.zeros(_n(r), bool)),                     # matches nothing
]


def _hashes(r, col, sel):
    dt = MV_COLS.get(col, "INT")
    if col not in MV_COLS:
        return {X.java_hash_code(dt, v) for v in np.unique(r[col][sel]).tolist()}
    return {X.java_hash_code(dt, v) for d in np.flatnonzero(sel) for v in r[col][d]}


def _model(raws, col, masks, groups=None):
    """Registers of every value of the selected docs: hll.from_ints over their Java hash codes; per group key if
    `groups` (a function raw -> array of string keys per doc)."""
    if groups is None:
        hs = set()
        for r, m in zip(raws, masks):
            hs |= _hashes(r, col, m)
        return HLL.from_ints(hs)
    per = {}
    for r, m in zip(raws, masks):
        keys = groups(r)
        for k in np.unique(keys[m]):
            per.setdefault(k, set()).update(_hashes(r, col, m & (keys == k)))
    return {k: HLL.from_ints(v) for k, v in per.items()}


def _native(ctx, gsegs, q, flags=0):
    """The request as ONE library query through E._Query (function code 11, registers from pgx_result_hll)."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    qq = E._Query(ctx, q)
    try:
        r = qq.execute(gsegs, flags)
        try:
            return E.decode_result(qq, r, gsegs)
        finally:
            N.lib().pgx_result_release(r)
    finally:
        qq.close()


def _plan(ctx, gsegs, q):
    from pinot_amd import engine as E
    return E.InstancePlanMakerImplV2(ctx).make_inter_segment_plan(gsegs, q).execute()


def _off(monkeypatch, ctx, gsegs, q):
    monkeypatch.setenv("PGX_HLL_NATIVE", "0")
    try:
        return _plan(ctx, gsegs, q)
    finally:
        monkeypatch.delenv("PGX_HLL_NATIVE")


def _status(fn):
    from pinot_amd import native as N
    with pytest.raises(N.PgxError) as e:
        fn()
    return e.value.status


def _same_blocks(on, off, q):
    assert on.stats.as_list() == off.stats.as_list()
    if q.get("group_by"):
        mon, moff = on.get_aggregation_group_by_result(), off.get_aggregation_group_by_result()
        mon, moff = (mon.as_map() if mon is not None else {}), (moff.as_map() if moff is not None else {})
        assert set(mon) == set(moff)
        for k in mon:
            for a, b in zip(mon[k], moff[k]):
                assert np.array_equal(np.asarray(a), np.asarray(b)), k
        return len(mon)
    for a, b in zip(on.get_aggregation_result(), off.get_aggregation_result()):
        assert (a == b) if isinstance(a, set) else np.array_equal(np.asarray(a), np.asarray(b))
    return 1


def test_function_code_compiles(env):
    """Function code 11 compiles and runs.  Without the feature pgx_query_compile refuses it ("aggregation function
    not on the GPU path") and the binding has no such code."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, raws = env
    assert E._FN["distinctcounthllmv"] == N.PGX_DISTINCTCOUNTHLLMV == 11
    agg = (N.Agg * 1)()
    agg[0].fn, agg[0].column = 11, b"ti"
    qd = N.QueryDesc(1, agg, 0, None, 10, 0, None, 0, None, 0)
    h = C.c_void_p()
    assert N.lib().pgx_query_compile(ctx.handle, C.byref(qd), C.byref(h)) == 0
    N.check(N.lib().pgx_query_release(h))
    agg[0].fn = 12
    assert N.lib().pgx_query_compile(ctx.handle, C.byref(qd), C.byref(h)) == N.PGX_ERR_UNSUPPORTED
    # a column every staged segment of the context holds single-value is refused at compile time already; a column
    # no staged segment has compiles (the execution looks at its own segments)
    agg[0].fn, agg[0].column = 11, b"m"
    assert N.lib().pgx_query_compile(ctx.handle, C.byref(qd), C.byref(h)) == N.PGX_ERR_UNSUPPORTED
    agg[0].column = b"no_such_column"
    assert N.lib().pgx_query_compile(ctx.handle, C.byref(qd), C.byref(h)) == 0
    N.check(N.lib().pgx_query_release(h))
    blk = _native(ctx, gsegs, pql.compile("SELECT DISTINCTCOUNTHLLMV(ti) FROM t"))
    got = blk.get_aggregation_result()[0]
    assert got.dtype == np.uint8 and got.tobytes() == _model(raws, "ti", [np.ones(_n(r), bool) for r in raws]).tobytes()


def test_compile_time_refusal_follows_the_staged_segments():
    """pgx_query_compile refuses code 11 on column x only while every staged segment holding x holds it single-value."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx = E.Context(0)
    try:
        agg = (N.Agg * 1)()
        agg[0].fn, agg[0].column = 11, b"x"
        qd = N.QueryDesc(1, agg, 0, None, 10, 0, None, 0, None, 0)

        def compile_status():
            h = C.c_void_p()
            st = N.lib().pgx_query_compile(ctx.handle, C.byref(qd), C.byref(h))
            if st == 0:
                N.check(N.lib().pgx_query_release(h))
            return st

        assert compile_status() == 0
        sv = E.IndexSegment(ctx, S.make_segment("kx0", [S.make_column("x", np.arange(40, dtype=np.int32) % 7)]))
        assert compile_status() == N.PGX_ERR_UNSUPPORTED
        mv = E.IndexSegment(ctx, S.make_segment("kx1", [S.make_mv_column("x", [[1, 2], [3]], "INT")]))
        assert compile_status() == 0  # multi-value somewhere: the execution decides
        mv.destroy()
        assert compile_status() == N.PGX_ERR_UNSUPPORTED
        sv.destroy()
        assert compile_status() == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("fi", range(len(FILTERS)))
def test_aggregation_only(env, monkeypatch, fi):
    ctx, gsegs, raws = env
    where, pred = FILTERS[fi]
    masks = [pred(r) for r in raws]
    assert fi in (0, 4) or 0 < sum(int(m.sum()) for m in masks) < sum(SIZES)
    q = pql.compile("SELECT " + ", ".join("DISTINCTCOUNTHLLMV(%s)" % c for c in MV_COLS) + " FROM t" + where)
    blk = _native(ctx, gsegs, q)
    got = blk.get_aggregation_result()
    off, on = _off(monkeypatch, ctx, gsegs, q), _plan(ctx, gsegs, q)
    for i, col in enumerate(MV_COLS):
        model = _model(raws, col, masks)
        assert got[i].dtype == np.uint8 and got[i].tobytes() == model.tobytes(), col
        assert list(on.get_aggregation_result()[i]) == list(off.get_aggregation_result()[i]) == list(model), col
        assert X.reduce_value("distinctcounthllmv", got[i]) == HLL.cardinality(model)
    if fi == 4:
        assert all(not g.any() for g in got)
    docs = int(sum(m.sum() for m in masks))
    st = blk.stats.as_list()
    assert st[0] == docs and st[2] == docs * len(MV_COLS) and st[3] == sum(SIZES)  # docs x columns, not x values
    assert st == off.stats.as_list() == on.stats.as_list()


def test_functions_mixed_in_any_order(env, monkeypatch):
    """A standard function, a single-value DISTINCTCOUNTHLL and two DISTINCTCOUNTHLLMV over one column, aggregation-only
    and under GROUP BY: values and order kept, the two MV functions share their registers."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, raws = env
    where, pred = FILTERS[3]
    masks = [pred(r) for r in raws]
    sel = "SELECT DISTINCTCOUNTHLLMV(ti), SUM(m), DISTINCTCOUNTHLL(ci), DISTINCTCOUNTHLLMV(ts), COUNT(*), " \
          "DISTINCTCOUNTHLLMV(ti) FROM t" + where
    q = pql.compile(sel)
    blk = _native(ctx, gsegs, q)
    res = blk.get_aggregation_result()
    docs = int(sum(m.sum() for m in masks))
    assert res[1] == float(sum(int(r["m"][m].sum()) for r, m in zip(raws, masks))) and res[4] == docs
    assert res[0].tobytes() == res[5].tobytes() == _model(raws, "ti", masks).tobytes()
    assert res[2].tobytes() == _model(raws, "ci", masks).tobytes()
    assert res[3].tobytes() == _model(raws, "ts", masks).tobytes()
    assert blk.stats.as_list()[2] == docs * 4  # ti, m, ci, ts: each projected column once
    off, on = _off(monkeypatch, ctx, gsegs, q), _plan(ctx, gsegs, q)
    assert blk.stats.as_list() == on.stats.as_list()
    _same_blocks(on, off, q)
    L = N.lib()
    qq = E._Query(ctx, q)
    r = qq.execute(gsegs)
    try:
        v, c = C.c_double(), C.c_int64()
        regs = np.zeros(256, np.uint8)
        assert L.pgx_result_agg(r, 0, C.byref(v), C.byref(c)) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_hll(r, 1, 0, 1, regs.ctypes.data) == N.PGX_ERR_INVALID_ARG      # SUM(m)
        assert L.pgx_result_hll(r, 5, 0, 1, regs.ctypes.data) == 0 and regs.tobytes() == res[0].tobytes()
    finally:
        L.pgx_result_release(r)
        qq.close()
    # the same under GROUP BY
    q = pql.compile(sel + " GROUP BY g1")
    got = _native(ctx, gsegs, q).get_aggregation_group_by_result().as_map()

    def keys(r):
        return np.array([str(int(v)) for v in r["g1"]])

    for i, col in ((0, "ti"), (2, "ci"), (3, "ts"), (5, "ti")):
        model = _model(raws, col, masks, keys)
        assert set(model) == set(got)
        for k in got:
            assert got[k][i].tobytes() == model[k].tobytes(), (col, k)
    for k in got:
        sums = sum(int(r["m"][m & (keys(r) == k)].sum()) for r, m in zip(raws, masks))
        assert got[k][1] == float(sums)
    assert _same_blocks(_plan(ctx, gsegs, q), _off(monkeypatch, ctx, gsegs, q), q) == len(got)


GROUPED = [
    ("SELECT DISTINCTCOUNTHLLMV(tl), SUM(m), DISTINCTCOUNTHLLMV(ts) FROM t%s GROUP BY g1", ("g1",)),              # 50 slots
    ("SELECT COUNT(*), DISTINCTCOUNTHLLMV(ti), DISTINCTCOUNTHLLMV(td) FROM t%s GROUP BY g1, g2", ("g1", "g2")),  # 50 x 40
]


@pytest.mark.parametrize("gi", range(len(GROUPED)))
@pytest.mark.parametrize("fi", [0, 3, 4])
def test_group_by(env, monkeypatch, gi, fi):
    """The group columns' dictionaries differ between the segments (remaps); registers per group of the result."""
    ctx, gsegs, raws = env
    where, pred = FILTERS[fi]
    masks = [pred(r) for r in raws]
    text, gcols = GROUPED[gi]
    q = pql.compile(text % where)

    def keys(r):
        return np.array(["\t".join(str(int(r[g][d])) for g in gcols) for d in range(_n(r))])

    blk = _native(ctx, gsegs, q)
    gr = blk.get_aggregation_group_by_result()
    got = gr.as_map() if gr is not None else {}
    assert (len(got) == 0) == (fi == 4)
    for i, a in enumerate(q["aggregations"]):
        if a["fn"] != "distinctcounthllmv":
            continue
        model = _model(raws, a["column"], masks, keys)
        assert set(model) == set(got)
        for k in got:  # every group of the result
            assert got[k][i].tobytes() == model[k].tobytes(), (a, k)
    off, on = _off(monkeypatch, ctx, gsegs, q), _plan(ctx, gsegs, q)
    assert blk.stats.as_list() == off.stats.as_list() == on.stats.as_list()
    assert _same_blocks(on, off, q) == len(got)


def test_result_hll_ranges(env):
    """pgx_result_hll over sub-ranges of the groups, in the order of the other group accessors: first, last, empty,
    out of range."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, raws = env
    L = N.lib()
    q = pql.compile(GROUPED[0][0] % "")
    qq = E._Query(ctx, q)
    r = qq.execute(gsegs)
    try:
        blk = E.decode_result(qq, r, gsegs)
        gr = blk.get_aggregation_group_by_result()
        keys = [k.string_key for k in gr.get_group_key_iterator()]
        n = len(keys)
        assert n == 50
        full = E.result_hll(r, 0, 0, n)
        model = _model(raws, "tl", [np.ones(_n(x), bool) for x in raws],
                       lambda x: np.array([str(int(v)) for v in x["g1"]]))
        for i, k in enumerate(keys):
            assert full[i].tobytes() == model[k].tobytes()
        for first, cnt in ((0, 1), (7, 13), (n - 1, 1), (n, 0), (0, 0)):
            part = E.result_hll(r, 0, first, cnt)
            assert part.tobytes() == full[first:first + cnt].tobytes()
        buf = np.zeros((n + 1) * 256, np.uint8)
        for agg, first, cnt in ((0, -1, 1), (0, 0, n + 1), (0, n, 1), (0, n + 1, 0), (0, 0, -1), (1, 0, 1), (3, 0, 1),
                                (-1, 0, 1)):
            assert L.pgx_result_hll(r, agg, first, cnt, buf.ctypes.data) == N.PGX_ERR_INVALID_ARG, (agg, first, cnt)
    finally:
        L.pgx_result_release(r)
        qq.close()


def test_refusals_fall_back_to_the_decomposition(env, monkeypatch):
    """PGX_ERR_UNSUPPORTED at the ABI: code 11 on a single-value column, a standard multi-value function beside it,
    GROUP BY a multi-value column, a key space above 65,536 slots, PGX_X_FORCE_HASH.  Through the plan maker the
    request gives what it gives with the knob off."""
    from pinot_amd import native as N
    ctx, gsegs, raws = env
    q = pql.compile("SELECT DISTINCTCOUNTHLLMV(m) FROM t")  # the decomposition refuses it too
    assert _status(lambda: _native(ctx, gsegs, q)) == N.PGX_ERR_UNSUPPORTED
    assert _status(lambda: _plan(ctx, gsegs, q)) == N.PGX_ERR_UNSUPPORTED
    assert _status(lambda: _off(monkeypatch, ctx, gsegs, q)) == N.PGX_ERR_UNSUPPORTED
    for text in ("SELECT DISTINCTCOUNTHLLMV(ti), SUMMV(ti) FROM t WHERE m < 500",
                 "SELECT DISTINCTCOUNTHLLMV(tl), COUNT(*) FROM t WHERE m < 100 GROUP BY ti",
                 "SELECT DISTINCTCOUNTHLLMV(ti), COUNT(*) FROM t WHERE m < 300 GROUP BY g1, h"):
        q = pql.compile(text)
        assert _status(lambda: _native(ctx, gsegs, q)) == N.PGX_ERR_UNSUPPORTED, text
        assert _same_blocks(_plan(ctx, gsegs, q), _off(monkeypatch, ctx, gsegs, q), q) > 0, text
    q = pql.compile("SELECT DISTINCTCOUNTHLLMV(ti), SUMMV(ti) FROM t WHERE m < 500")
    masks = [r["m"] < 500 for r in raws]
    assert _plan(ctx, gsegs, q).get_aggregation_result()[0].tobytes() == _model(raws, "ti", masks).tobytes()
    q = pql.compile(GROUPED[0][0] % "")
    assert _status(lambda: _native(ctx, gsegs, q, flags=N.PGX_X_FORCE_HASH)) == N.PGX_ERR_UNSUPPORTED
    # DISTINCTCOUNTHLL (code 10) on the multi-value column stays refused
    q = pql.compile("SELECT DISTINCTCOUNTHLLMV(ti) FROM t")
    q["aggregations"] = [dict(a, fn="distinctcounthll") for a in q["aggregations"]]
    assert _status(lambda: _native(ctx, gsegs, q)) == N.PGX_ERR_UNSUPPORTED


def test_async_and_repeated_executions(env):
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, _ = env
    for text in ("SELECT DISTINCTCOUNTHLLMV(tl), DISTINCTCOUNTHLLMV(ts) FROM t" + FILTERS[3][0], GROUPED[1][0] % ""):
        q = pql.compile(text)
        qq = E._Query(ctx, q)
        outs = []
        try:
            for how in ("sync", "sync", "async"):
                r = qq.execute_async(gsegs) if how == "async" else qq.execute(gsegs)
                try:
                    ng = C.c_int64(1)
                    if q.get("group_by"):
                        N.check(N.lib().pgx_result_num_groups(r, C.byref(ng)))
                    st = (C.c_int64 * 4)()
                    N.check(N.lib().pgx_result_stats(r, st))
                    outs.append((list(st), [E.result_hll(r, i, 0, ng.value).tobytes()
                                            for i, a in enumerate(q["aggregations"]) if a["fn"] == "distinctcounthllmv"]))
                finally:
                    N.lib().pgx_result_release(r)
        finally:
            qq.close()
        assert outs[0] == outs[1] == outs[2] and len(outs[0][1]) == 2 and any(outs[0][1][0])


def test_consuming_segment_with_a_growing_multi_value_dictionary(monkeypatch):
    """A consuming segment queried after 700 and after 9,000 docs: the multi-value column's dictionary grows in
    between, and the second snapshot must not see a code table built for the first."""
    from pinot_amd import engine as E
    from pinot_amd.realtime import RealtimeSegment
    from tests.test_realtime import SCHEMA, _rows
    ctx = E.Context(0)
    try:
        rng = np.random.default_rng(9)
        rt = RealtimeSegment("rt_hllmv", SCHEMA, capacity=100000, inverted=["dim"])
        rows = _rows(rng, 9000)
        for r in rows:
            r["tags"] = [int(x) for x in rng.integers(-3000, 3000, size=int(rng.integers(1, 5)))]
        done = 0
        cards = []
        for stop in (700, 9000):
            for r in rows[done:stop]:
                rt.index(r)
            done = stop
            cards.append(rt.dictionaries["tags"].length())
            seg = rt.device_segment(ctx)
            for text in ("SELECT DISTINCTCOUNTHLLMV(tags), DISTINCTCOUNTHLL(lng), COUNT(*) FROM rt "
                         "WHERE dim BETWEEN -20 AND 20",
                         "SELECT DISTINCTCOUNTHLLMV(tags), SUM(met) FROM rt GROUP BY name"):
                q = pql.compile(text)
                on, off = _plan(ctx, [seg], q), _off(monkeypatch, ctx, [seg], q)
                groups = _same_blocks(on, off, q)
                if q.get("group_by"):
                    assert groups == 8
                else:
                    sel = [r for r in rows[:stop] if -20 <= r["dim"] <= 20]
                    exp = HLL.from_ints({X.java_hash_code("INT", v) for r in sel for v in r["tags"]})
                    assert on.get_aggregation_result()[0].tobytes() == exp.tobytes()
                    blk = _native(ctx, [seg], q)
                    assert blk.get_aggregation_result()[0].tobytes() == exp.tobytes()
        assert cards[1] > cards[0]
    finally:
        ctx.close()


def test_request_texts_of_the_multi_value_suite(monkeypatch):
    """The DISTINCTCOUNTHLLMV requests of tests/test_gpu_mv.py (EXT_QUERIES), knob on against knob off: equal blocks."""
    from pinot_amd import engine as E
    from tests.test_gpu_mv import EXT_QUERIES, _segment
    ctx = E.Context(0)
    try:
        gsegs = [E.IndexSegment(ctx, _segment("mvx%d" % i, 40 + i, 3000 + 13 * i, False)[0]) for i in range(2)]
        texts = [t for t in EXT_QUERIES if "DISTINCTCOUNTHLLMV" in t]
        assert len(texts) == 2
        for text in texts:
            q = pql.compile(text)
            on, off = _plan(ctx, gsegs, q), _off(monkeypatch, ctx, gsegs, q)
            assert on.stats.as_list() == off.stats.as_list()
            for a, fn, g, e in zip(q["aggregations"], [a["fn"] for a in q["aggregations"]],
                                   on.get_aggregation_result(), off.get_aggregation_result()):
                if X.base_fn(fn).startswith("percentileest"):
                    assert g.count == e.count
                elif isinstance(g, (set, list, tuple, int, float)):
                    assert g == e, fn
                else:
                    assert np.array_equal(np.asarray(g), np.asarray(e)), fn
    finally:
        ctx.close()
