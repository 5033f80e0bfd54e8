"""DISTINCTCOUNTHLL on the device (PGX_DISTINCTCOUNTHLL, pinot_amd/csrc/pgx_hll.cpp run_hll over pgx_hll.hip): the
registers pgx_result_hll returns are compared bit for bit with hll.from_ints over the numpy-selected rows' Java hash
codes, with the oracle's per-doc restatement, and with the host decomposition (PGX_HLL_NATIVE=0: a GROUP BY histogram
hashed in Python), statistics included.  Every comparison is exact: an offer is a register-wise max."""
import ctypes as C

import numpy as np
import pytest

from oracle import pinot_oracle as O
from pinot_amd import extended as X
from pinot_amd import hll as HLL
from pinot_amd import pql
from pinot_amd import segment as S
from tests import helpers as H

pytestmark = pytest.mark.gpu

SIZES = (9001, 8192, 700)
HLL_COLS = {"ci": "INT", "cl": "LONG", "cf": "FLOAT", "cd": "DOUBLE", "s": "STRING"}


def _raw(i, n):
    """Segment i's raw columns and the pre-built dictionaries of ci (300 values) and cl (20,000 values, 15 bits; a
    segment holds fewer docs than that, so part of the dictionary is unused).  Every HLL column has its own dictionary
    per segment, the value ranges overlapping."""
    rng = np.random.default_rng(100 + i)
    words = np.array(["w%d" % k for k in range(40 * i, 40 * i + 120)] + ["tab\there", "été", "中"])
    dicts = {"ci": (np.arange(300) + 100 * i).astype(np.int32),
             "cl": np.sort(rng.choice(60000, 20000, replace=False)).astype(np.int64) * (1 << 20) - (1 << 34)}
    ids = {"ci": rng.integers(0, 300, n), "cl": rng.integers(0, 20000, n)}
    raw = {
        "ci": dicts["ci"][ids["ci"]],
        "cl": dicts["cl"][ids["cl"]],
        "cf": (rng.integers(0, 500, n) * 0.25 + i).astype(np.float32),
        "cd": rng.integers(-2000, 2000, n) * 0.37 + 1e-3 * i,
        "s": words[rng.integers(0, len(words), n)],
        "m": rng.integers(0, 1000, n).astype(np.int32),
        "b": rng.integers(0, 20, n).astype(np.int32),                                     # inverted index
        "g1": rng.permutation(np.arange(n) % 50).astype(np.int32),                       # 50 values in every segment
        "g2": (rng.integers(0, 20 + 5 * i, n) + (0, 15, 5)[i]).astype(np.int32),         # union: 0..39
        "h": rng.permutation(np.arange(n) % 1400).astype(np.int32),                      # 50 x 1400 = 70,000 slots
    }
    return raw, dicts, ids


@pytest.fixture(scope="module")
def env():
    from pinot_amd import engine as E
    ctx = E.Context(0)
    gsegs, osegs, raws = [], [], []
    types = {"cl": "LONG", "cf": "FLOAT", "cd": "DOUBLE"}
    for i, n in enumerate(SIZES):
        raw, dicts, ids = _raw(i, n)
        cols = [S.make_column(c, None, data_type=types.get(c, "INT"), dictionary=dicts[c], dict_ids=ids[c])
                if c in dicts else S.make_column(c, v, data_type=types.get(c), inverted=c == "b")
                for c, v in raw.items()]
        seg = S.make_segment("hll%d" % i, cols)
        assert seg.columns["ci"].cardinality == 300
        assert seg.columns["cl"].cardinality == 20000 and seg.columns["cl"].bits == 15
        gsegs.append(E.IndexSegment(ctx, seg))
        osegs.append(O.OSegment.from_raw(raw, inverted=("b",), dtypes=types))
        raws.append(raw)
    assert len(np.unique(np.concatenate([r["g2"] for r in raws]))) == 40
    yield ctx, gsegs, osegs, raws
    ctx.close()


# (WHERE clause, the same predicate over a segment's raw columns)
FILTERS = [
    ("", lambda r: np.ones(len(r["m"]), bool)),
    (" WHERE m BETWEEN 100 AND 140", lambda r: (r["m"] >= 100) & (r["m"] <= 140)),
    (" WHERE b = 3 OR m < 50", lambda r: (r["b"] == 3) | (r["m"] < 50)),      # a bitmap leaf OR a scan leaf
    (" WHERE m = 123456", lambda r: np.zeros(len(r["m"]), bool)),             # matches nothing
]


def _model(raws, col, masks, groups=None):
    """Registers of the selected rows' values: hll.from_ints over their Java hash codes; per group key if `groups`
    (a function raw, row mask -> array of string keys)."""
    dt = HLL_COLS[col]
    if groups is None:
        hs = set()
        for r, m in zip(raws, masks):
            hs |= {X.java_hash_code(dt, v) for v in np.unique(r[col][m]).tolist()}
        return HLL.from_ints(hs)
    per = {}
    for r, m in zip(raws, masks):
        keys = groups(r)
        for k in np.unique(keys[m]):
            sel = m & (keys == k)
            per.setdefault(k, set()).update(X.java_hash_code(dt, v) for v in np.unique(r[col][sel]).tolist())
    return {k: HLL.from_ints(v) for k, v in per.items()}


def _native(ctx, gsegs, q, flags=0):
    """The request as ONE library query through E._Query (function code 10, registers from pgx_result_hll): the
    decoded block."""
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


def test_function_code_compiles(env):
    """Without the feature pgx_query_compile refuses function code 10 ("aggregation function not on the GPU path")."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, _, _ = env
    assert E._FN["distinctcounthll"] == N.PGX_DISTINCTCOUNTHLL == 10
    q = E._Query(ctx, pql.compile("SELECT DISTINCTCOUNTHLL(ci) FROM t"))
    q.close()
    agg = (N.Agg * 1)()
    agg[0].fn, agg[0].column = 11, b"ci"
    qd = N.QueryDesc(1, agg, 0, None, 10, 0, None, 0, None, 0)
    h = C.c_void_p()
    assert N.lib().pgx_query_compile(ctx.handle, C.byref(qd), C.byref(h)) == N.PGX_ERR_UNSUPPORTED


@pytest.mark.parametrize("fi", range(len(FILTERS)))
def test_aggregation_only(env, monkeypatch, fi):
    ctx, gsegs, osegs, raws = env
    where, pred = FILTERS[fi]
    masks = [pred(r) for r in raws]
    text = "SELECT " + ", ".join("DISTINCTCOUNTHLL(%s)" % c for c in HLL_COLS) + " FROM t" + where
    q = pql.compile(text)
    blk = _native(ctx, gsegs, q)
    got = blk.get_aggregation_result()
    exp = O.combine_aggregation([O.run_aggregation(s, q, literal_filter=False) for s in osegs], q)
    off = _off(monkeypatch, ctx, gsegs, q)
    on = _plan(ctx, gsegs, q)
    for i, col in enumerate(HLL_COLS):
        model = _model(raws, col, masks)
        assert got[i].dtype == np.uint8 and got[i].tobytes() == model.tobytes(), col
        assert list(got[i]) == list(exp["results"][i]), col
        assert list(on.get_aggregation_result()[i]) == list(off.get_aggregation_result()[i]) == list(model), col
        assert X.reduce_value("distinctcounthll", got[i]) == O.reduce_extended("distinctcounthll", exp["results"][i])
    if fi == 3:
        assert all(not g.any() for g in got)
    docs = int(sum(m.sum() for m in masks))
    st = blk.stats.as_list()
    assert st[0] == docs and st[2] == docs * len(HLL_COLS) and st[3] == sum(SIZES)
    assert st == off.stats.as_list() == on.stats.as_list()
    assert st[1] == H.literal_entries(osegs, q) and st[0] == exp["stats"][0] and st[2] == exp["stats"][2]


def test_standard_functions_mixed_in(env, monkeypatch):
    """Standard and HLL functions in any order, two HLL functions over one column: values and order kept."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, osegs, raws = env
    where, pred = FILTERS[1]
    masks = [pred(r) for r in raws]
    q = pql.compile("SELECT SUM(m), DISTINCTCOUNTHLL(ci), COUNT(*), DISTINCTCOUNTHLL(ci), DISTINCTCOUNTHLL(s), MAX(cd) "
                    "FROM t" + where)
    got = _native(ctx, gsegs, q)
    res = got.get_aggregation_result()
    assert res[0] == float(sum(int(r["m"][m].sum()) for r, m in zip(raws, masks)))
    assert res[2] == int(sum(m.sum() for m in masks))
    assert res[5] == max(float(r["cd"][m].max()) for r, m in zip(raws, masks))
    assert res[1].tobytes() == res[3].tobytes() == _model(raws, "ci", masks).tobytes()
    assert res[4].tobytes() == _model(raws, "s", masks).tobytes()
    docs = res[2]
    assert got.stats.as_list()[2] == docs * 4  # m, ci, s, cd: each projected column once
    off, on = _off(monkeypatch, ctx, gsegs, q), _plan(ctx, gsegs, q)
    assert on.stats.as_list() == off.stats.as_list() == got.stats.as_list()
    for a, b in zip(on.get_aggregation_result(), off.get_aggregation_result()):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    # numeric accessors on an HLL function index
    L = N.lib()
    qq = E._Query(ctx, q)
    r = qq.execute(gsegs)
    try:
        v, c = C.c_double(), C.c_int64()
        assert L.pgx_result_agg(r, 1, C.byref(v), C.byref(c)) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_agg(r, 0, C.byref(v), C.byref(c)) == 0 and v.value == res[0]
        regs = np.zeros(256, np.uint8)
        assert L.pgx_result_hll(r, 0, 0, 1, regs.ctypes.data) == N.PGX_ERR_INVALID_ARG      # SUM(m)
        assert L.pgx_result_hll(r, 6, 0, 1, regs.ctypes.data) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_hll(r, 1, 1, 1, regs.ctypes.data) == N.PGX_ERR_INVALID_ARG      # one "group" only
        assert L.pgx_result_hll(r, 1, 0, 2, regs.ctypes.data) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_hll(r, 1, 0, 1, regs.ctypes.data) == 0 and regs.tobytes() == res[1].tobytes()
    finally:
        L.pgx_result_release(r)
        qq.close()


GROUPED = [
    ("SELECT DISTINCTCOUNTHLL(cl), SUM(m), DISTINCTCOUNTHLL(s) FROM t%s GROUP BY g1", ("g1",)),              # 50 slots
    ("SELECT COUNT(*), DISTINCTCOUNTHLL(ci), DISTINCTCOUNTHLL(cf) FROM t%s GROUP BY g1, g2", ("g1", "g2")),  # 50 x 40
]


@pytest.mark.parametrize("gi", range(len(GROUPED)))
@pytest.mark.parametrize("fi", [0, 2, 3])
def test_group_by(env, monkeypatch, gi, fi):
    ctx, gsegs, osegs, raws = env
    where, pred = FILTERS[fi]
    masks = [pred(r) for r in raws]
    text, gcols = GROUPED[gi]
    q = pql.compile(text % where)
    fns = [a["fn"] for a in q["aggregations"]]

    def keys(r):
        return np.array(["\t".join(str(int(r[g][d])) for g in gcols) for d in range(len(r["m"]))])

    blk = _native(ctx, gsegs, q)
    gr = blk.get_aggregation_group_by_result()
    got = gr.as_map()
    exp = O.combine_group_by([O.run_group_by(s, q, literal_filter=False) for s in osegs], q)
    assert set(got) == set(exp["merged"])
    assert (len(got) == 0) == (fi == 3)
    for i, a in enumerate(q["aggregations"]):
        if a["fn"] != "distinctcounthll":
            for k in got:
                H.assert_values_equal([got[k][i]], [exp["merged"][k][i]], [a["fn"]])
            continue
        model = _model(raws, a["column"], masks, keys)
        assert set(model) == set(got)
        for k in got:  # every group of the result
            assert got[k][i].tobytes() == model[k].tobytes(), (a, k)
            assert list(got[k][i]) == list(exp["merged"][k][i])
    off, on = _off(monkeypatch, ctx, gsegs, q), _plan(ctx, gsegs, q)
    assert blk.stats.as_list() == off.stats.as_list() == on.stats.as_list()
    mon, moff = on.get_aggregation_group_by_result(), off.get_aggregation_group_by_result()
    mon, moff = (mon.as_map() if mon is not None else {}), (moff.as_map() if moff is not None else {})
    assert set(mon) == set(moff) == set(got)
    for k in mon:
        for fn, a, b in zip(fns, mon[k], moff[k]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (k, fn)


def test_result_hll_ranges(env):
    """pgx_result_hll over sub-ranges of the groups, in the order of the other group accessors, and its INVALID_ARG
    cases; pgx_result_group_values / _trim refuse an HLL index, pgx_result_gather puts 0 there."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, _, raws = env
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
        model = _model(raws, "cl", [np.ones(len(x["m"]), bool) for x in raws],
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
        v, c = np.zeros(n), np.zeros(n, np.int64)
        assert L.pgx_result_group_values(r, 0, v.ctypes.data, c.ctypes.data) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_group_values(r, 1, v.ctypes.data, c.ctypes.data) == 0
        cap = C.c_int64(n)
        idx = np.zeros(n, np.int64)
        assert L.pgx_result_trim(r, 2, idx.ctypes.data, C.byref(cap)) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_trim(r, 1, idx.ctypes.data, C.byref(cap)) == 0 and cap.value == n
        gv, gc = np.full(3 * n, -1.0), np.full(3 * n, -1, np.int64)
        assert L.pgx_result_gather(r, idx.ctypes.data, n, None, None, gv.ctypes.data, gc.ctypes.data) == 0
        assert not gv[:n].any() and not gc[:n].any() and not gv[2 * n:].any() and (gv[n:2 * n] == v[idx]).all()
    finally:
        L.pgx_result_release(r)
        qq.close()


def test_large_and_forced_key_spaces_are_refused(env, monkeypatch):
    """70,000 slots: PGX_ERR_UNSUPPORTED at the ABI, and through the plan maker the same answer as with the knob off
    (the request falls back to the decomposition); PGX_X_FORCE_HASH is refused at the ABI."""
    from pinot_amd import native as N
    ctx, gsegs, _, _ = env
    q = pql.compile("SELECT DISTINCTCOUNTHLL(ci), COUNT(*) FROM t WHERE m < 300 GROUP BY g1, h")
    with pytest.raises(N.PgxError) as ei:
        _native(ctx, gsegs, q)
    assert ei.value.status == N.PGX_ERR_UNSUPPORTED
    on, off = _plan(ctx, gsegs, q), _off(monkeypatch, ctx, gsegs, q)
    assert on.stats.as_list() == off.stats.as_list()
    mon, moff = on.get_aggregation_group_by_result().as_map(), off.get_aggregation_group_by_result().as_map()
    assert set(mon) == set(moff) and len(mon) > 1000
    for k in mon:
        assert np.array_equal(mon[k][0], moff[k][0]) and mon[k][1] == moff[k][1]
    q = pql.compile(GROUPED[0][0] % "")
    with pytest.raises(N.PgxError) as ei:
        _native(ctx, gsegs, q, flags=N.PGX_X_FORCE_HASH)
    assert ei.value.status == N.PGX_ERR_UNSUPPORTED


def test_async_and_repeated_executions(env):
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, _, _ = env
    for text in ("SELECT DISTINCTCOUNTHLL(cl), DISTINCTCOUNTHLL(s) FROM t WHERE b = 3 OR m < 50", GROUPED[1][0] % ""):
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
                                            for i, a in enumerate(q["aggregations"]) if a["fn"] == "distinctcounthll"]))
                finally:
                    N.lib().pgx_result_release(r)
        finally:
            qq.close()
        assert outs[0] == outs[1] == outs[2] and len(outs[0][1]) == 2 and any(outs[0][1][0])


def _status(fn):
    from pinot_amd import native as N
    with pytest.raises(N.PgxError) as e:
        fn()
    return e.value.status


def test_refusals(env, monkeypatch):
    """Multi-value columns beside an HLL function, pgx_execute_multi, key domains, a caller's dense table,
    pgx_execute_timed and PGX_JIT=0: PGX_ERR_UNSUPPORTED."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, _, _ = env
    L = N.lib()
    rng = np.random.default_rng(3)
    n = 500
    tags = [rng.integers(0, 9, rng.integers(1, 4)).tolist() for _ in range(n)]
    mv = E.IndexSegment(ctx, S.make_segment("hllmv", [S.make_mv_column("tags", tags, "INT"),
                                                      S.make_column("d", rng.integers(0, 7, n).astype(np.int32))]))
    for text in ("SELECT DISTINCTCOUNTHLL(tags) FROM t",                      # an MV column under the function
                 "SELECT DISTINCTCOUNTHLL(d), SUMMV(tags) FROM t",            # an MV function beside it
                 "SELECT DISTINCTCOUNTHLL(d) FROM t GROUP BY tags",           # an MV group column
                 "SELECT DISTINCTCOUNTHLL(d), COUNTMV(tags) FROM t GROUP BY d"):
        q = pql.compile(text)
        q["aggregations"] = [dict(a, fn="distinctcounthll") if a["fn"] == "distinctcounthllmv" else a
                             for a in q["aggregations"]]
        assert _status(lambda: _native(ctx, [mv], q)) == N.PGX_ERR_UNSUPPORTED, text
    q = pql.compile(GROUPED[0][0] % "")
    qq = E._Query(ctx, q)
    try:
        assert _status(lambda: qq.execute_multi(gsegs)) == N.PGX_ERR_UNSUPPORTED
        assert _status(lambda: qq.set_key_domain(0, list(range(60)), "INT")) == N.PGX_ERR_UNSUPPORTED
        assert _status(lambda: qq.execute(gsegs, flags=N.PGX_X_KEEP_DENSE_ON_DEVICE)) == N.PGX_ERR_UNSUPPORTED
        dense = C.c_void_p()
        N.check(L.pgx_device_alloc(ctx.handle, 1 << 16, C.byref(dense)))
        try:
            assert _status(lambda: qq.execute(gsegs, dense_out=dense, dense_out_bytes=1 << 16)) == N.PGX_ERR_UNSUPPORTED
        finally:
            L.pgx_device_free(ctx.handle, dense)
        segs = (C.c_void_p * len(gsegs))(*[s.handle.value for s in gsegs])
        slots, op = C.c_int64(), C.c_int32()
        assert L.pgx_query_dense_slots(qq.handle, segs, len(gsegs), C.byref(slots)) == N.PGX_ERR_UNSUPPORTED
        assert L.pgx_query_dense_plane_op(qq.handle, segs, len(gsegs), 1, C.byref(op)) == N.PGX_ERR_UNSUPPORTED
        binds, keep = qq.bindings(gsegs)
        t, k, out = C.c_double(), C.c_double(), C.c_void_p()
        assert L.pgx_execute_timed(ctx.handle, qq.handle, segs, len(gsegs), binds, 1, C.byref(t), C.byref(k),
                                   C.byref(out)) == N.PGX_ERR_UNSUPPORTED
    finally:
        qq.close()
    monkeypatch.setenv("PGX_JIT", "0")  # the knobs are read when the query is compiled
    try:
        assert _status(lambda: _native(ctx, gsegs, q)) == N.PGX_ERR_UNSUPPORTED
    finally:
        monkeypatch.delenv("PGX_JIT")
    mv.destroy()


def test_consuming_segment_with_growing_dictionaries(monkeypatch):
    """A consuming segment queried after 700 and after 9,000 docs: the dictionaries grow in between, and the second
    snapshot must not see a code table built for the first."""
    from pinot_amd import engine as E
    from pinot_amd.realtime import RealtimeSegment
    from tests.test_realtime import SCHEMA, _rows
    ctx = E.Context(0)
    try:
        rng = np.random.default_rng(9)
        rt = RealtimeSegment("rt_hll", SCHEMA, capacity=100000, inverted=["dim"])
        rows = _rows(rng, 9000)
        done = 0
        cards = []
        for stop in (700, 9000):
            for r in rows[done:stop]:
                rt.index(r)
            done = stop
            cards.append(rt.dictionaries["lng"].length())
            seg = rt.device_segment(ctx)
            for text in ("SELECT DISTINCTCOUNTHLL(lng), DISTINCTCOUNTHLL(name), DISTINCTCOUNTHLL(dbl), COUNT(*) FROM rt "
                         "WHERE dim BETWEEN -20 AND 20",
                         "SELECT DISTINCTCOUNTHLL(lng), DISTINCTCOUNTHLL(ts), SUM(met) FROM rt GROUP BY name"):
                q = pql.compile(text)
                on, off = _plan(ctx, [seg], q), _off(monkeypatch, ctx, [seg], q)
                assert on.stats.as_list() == off.stats.as_list()
                if q.get("group_by"):
                    mon = on.get_aggregation_group_by_result().as_map()
                    moff = off.get_aggregation_group_by_result().as_map()
                    assert set(mon) == set(moff) and len(mon) == 8
                    for k in mon:
                        for a, b in zip(mon[k], moff[k]):
                            assert np.array_equal(np.asarray(a), np.asarray(b))
                else:
                    for a, b in zip(on.get_aggregation_result(), off.get_aggregation_result()):
                        assert np.array_equal(np.asarray(a), np.asarray(b))
                    sel = [r for r in rows[:stop] if -20 <= r["dim"] <= 20]
                    exp = HLL.from_ints({X.java_hash_code("LONG", r["lng"]) for r in sel})
                    assert on.get_aggregation_result()[0].tobytes() == exp.tobytes()
        assert cards[1] > cards[0]
    finally:
        ctx.close()


def test_request_texts_of_the_extended_suite(monkeypatch):
    """The HLL requests of tests/test_gpu_extended.py, knob on against knob off: equal registers and statistics."""
    from pinot_amd import engine as E
    ctx = E.Context(0)
    try:
        rng = np.random.default_rng(17)
        gsegs = []
        for i in range(3):
            n = 4000 + 900 * i
            raw = {"d": rng.integers(0, 50 + 10 * i, n).astype(np.int32),
                   "v": rng.integers(-(1 << 20), 1 << 20, n).astype(np.int32) // (i + 1),
                   "w": (rng.integers(0, 3000, n) * 0.37 - 300.0).astype(np.float32),
                   "m": rng.integers(0, 5000, n).astype(np.int32)}
            gsegs.append(E.IndexSegment(ctx, H.build_pair("extx%d" % i, raw, types={"w": "FLOAT"})[0]))
        for text in ("SELECT DISTINCTCOUNTHLL(v), DISTINCTCOUNT(v), DISTINCTCOUNTHLL(w), DISTINCTCOUNTHLL(d) FROM t "
                     "WHERE m < 4000",
                     "SELECT DISTINCTCOUNTHLL(m), COUNT(*) FROM t WHERE d = 123456",
                     "SELECT DISTINCTCOUNTHLL(v), SUM(m), DISTINCTCOUNTHLL(w) FROM t WHERE m > 100 GROUP BY d"):
            q = pql.compile(text)
            on, off = _plan(ctx, gsegs, q), _off(monkeypatch, ctx, gsegs, q)
            assert on.stats.as_list() == off.stats.as_list()
            if q.get("group_by"):
                mon = on.get_aggregation_group_by_result().as_map()
                moff = off.get_aggregation_group_by_result().as_map()
                assert set(mon) == set(moff) and len(mon) > 0
                for k in mon:
                    for a, b in zip(mon[k], moff[k]):
                        assert np.array_equal(np.asarray(a), np.asarray(b))
                for a, b in zip(on.trimmed, off.trimmed):
                    assert set(a) == set(b)
            else:
                for a, b in zip(on.get_aggregation_result(), off.get_aggregation_result()):
                    assert (a == b) if isinstance(a, set) else np.array_equal(np.asarray(a), np.asarray(b))
    finally:
        ctx.close()
