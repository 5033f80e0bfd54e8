"""PERCENTILE and PERCENTILEMV on the device (PGX_PERCENTILE / PGX_PERCENTILEMV, pinot_amd/csrc/pgx_hll.cpp run_hll
with pgx_percentile.cpp over pgx_percentile.hip): the (value, count) pairs pgx_result_percentile returns are compared
with a numpy count of the selected values, with the oracle's per-doc restatement, and with the host decomposition
(PGX_PERCENTILE_NATIVE=0: a GROUP BY histogram), statistics included.  Every comparison is exact: the intermediates are
integer counts of dictionary values.  The data (five segments, two of them sharing dictionaries), the filters and the
plumbing are those of tests/test_gpu_distinct.py; it holds no -0.0 and no NaN."""
import copy
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from oracle import pinot_oracle as O
from pinot_amd import extended as X
from pinot_amd import hll as HLL
from pinot_amd import pql
from pinot_amd import segment as S
from tests import helpers as H
from tests.test_gpu_distinct import (FILTERS, MV_COLS, SIZES, TYPES, _columns, _compile_status, _n, _native, _plan,
                                     _raw, _status)

pytestmark = pytest.mark.gpu

PCT_COLS = ("ci", "cl", "cf", "cd", "ti")


@pytest.fixture(scope="module")
def env():
    from pinot_amd import engine as E
    ctx = E.Context(0)
    gsegs, osegs, raws = [], [], []
    for i, n in enumerate(SIZES):
        raw, dicts, ids = _raw(i, n)
        seg = S.make_segment("pc%d" % i, _columns(raw, dicts, ids))
        gsegs.append(E.IndexSegment(ctx, seg))
        osegs.append(O.OSegment.from_raw(raw, inverted=("b",), dtypes={k: v for k, v in TYPES.items() if v != "INT"}))
        raws.append(raw)
    for r in raws:  # no -0.0, no NaN
        for c in ("cf", "cd"):
            assert not np.isnan(r[c]).any() and not (np.signbit(r[c]) & (r[c] == 0)).any()
    yield ctx, gsegs, osegs, raws
    ctx.close()


def _values(r, col, sel):
    """The selected values of one segment as doubles (FLOAT widened), every value of every selected doc for `ti`."""
    if col in MV_COLS:
        return [float(v) for d in np.flatnonzero(sel) for v in r[col][d]]
    return [float(v) for v in r[col][sel]]


def _model(raws, col, masks, groups=None):
    """The ascending (value, count) pairs of the selected values; with `groups` a dict of them per group key."""
    if groups is None:
        c = Counter()
        for r, m in zip(raws, masks):
            c.update(_values(r, col, m))
        return sorted(c.items())
    per = {}
    for r, m in zip(raws, masks):
        keys = groups(r)
        for k in np.unique(keys[m]):
            per.setdefault(k, Counter()).update(_values(r, col, m & (keys == k)))
    return {k: sorted(c.items()) for k, c in per.items()}


def _pairs_of_list(values):
    return sorted(Counter(float(v) for v in values).items())


def _library_request(q, cols=PCT_COLS):
    """The request with one PGX_PERCENTILE / PGX_PERCENTILEMV function per column (codes 15 / 14), as E._Query takes it."""
    return {"aggregations": [{"fn": "percentilemv" if c in MV_COLS else "percentile", "column": c} for c in cols],
            "group_by": copy.deepcopy(q.get("group_by")), "filter": q.get("filter")}


def _off(monkeypatch, ctx, gsegs, q, others_too=False):
    names = ["PGX_PERCENTILE_NATIVE"] + (["PGX_DISTINCT_NATIVE", "PGX_HLL_NATIVE"] if others_too else [])
    for n in names:
        monkeypatch.setenv(n, "0")
    try:
        return _plan(ctx, gsegs, q)
    finally:
        for n in names:
            monkeypatch.delenv(n)


def _eq(a, b):
    if hasattr(a, "serialize"):  # a QuantileDigest: equal bytes
        return a.serialize() == b.serialize()
    if isinstance(a, (set, int, float, tuple, list)):
        return type(a) is type(b) and a == b
    return np.array_equal(np.asarray(a), np.asarray(b))


def _reduced_equal(f, a, b):
    if X.base_fn(f).startswith("percentile") and not X.base_fn(f).startswith("percentileest") and not a:
        return not b  # (the reference throws on an empty list)
    return X.reduce_value(f, a) == X.reduce_value(f, b)


def _same_blocks(on, off, q):
    """Intermediates, reduced values, trimmed maps and all four statistics of two blocks."""
    assert on.stats.as_list() == off.stats.as_list()
    fns = [a["fn"] for a in q["aggregations"]]
    if q.get("group_by"):
        mon, moff = on.get_aggregation_group_by_result(), off.get_aggregation_group_by_result()
        mon, moff = (mon.as_map() if mon is not None else {}), (moff.as_map() if moff is not None else {})
        assert set(mon) == set(moff)
        for k in mon:
            for f, a, b in zip(fns, mon[k], moff[k]):
                assert _eq(a, b), (k, f)
                if f in X.EXT_FUNCTIONS:
                    assert _reduced_equal(f, a, b)
        ton, toff = getattr(on, "trimmed", None), getattr(off, "trimmed", None)
        assert (ton is None) == (toff is None)
        for f, a, b in zip(fns, ton or [], toff or []):
            assert set(a) == set(b) and all(_eq(a[k], b[k]) for k in a), f
        return len(mon)
    for f, a, b in zip(fns, on.get_aggregation_result(), off.get_aggregation_result()):
        assert _eq(a, b), f
        if f in X.EXT_FUNCTIONS:
            assert _reduced_equal(f, a, b)
    return 1


def _calls(monkeypatch):
    from pinot_amd import engine as E
    calls = {"n": 0}
    real = E.result_percentile

    def counting(*a, **k):
        calls["n"] += 1
        return real(*a, **k)

    monkeypatch.setattr(E, "result_percentile", counting)
    return calls


def test_function_code_compiles(env):
    """Function codes 15 (single-value) and 14 (multi-value) compile and run; 14 on a column every staged segment holds
    single-value and 15 on one every staged segment holds multi-value are refused at compile time.  Without the
    feature pgx_query_compile refuses both codes and the binding has no such names."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, _, raws = env
    assert E._FN["percentile"] == N.PGX_PERCENTILE == 15 and E._FN["percentilemv"] == N.PGX_PERCENTILEMV == 14
    assert _compile_status(ctx, 15, b"ci") == 0 and _compile_status(ctx, 14, b"ti") == 0
    assert _compile_status(ctx, 14, b"ci") == N.PGX_ERR_UNSUPPORTED
    assert _compile_status(ctx, 15, b"ti") == N.PGX_ERR_UNSUPPORTED
    assert _compile_status(ctx, 15, b"no_such_column") == 0 and _compile_status(ctx, 14, b"no_such_column") == 0
    all_rows = [np.ones(_n(r), bool) for r in raws]
    got = _native(ctx, gsegs, _library_request({}, ("ci", "ti"))).get_aggregation_result()
    assert got[0] == _model(raws, "ci", all_rows) and got[1] == _model(raws, "ti", all_rows)
    assert all(isinstance(v, float) and isinstance(c, int) for v, c in got[0])


def test_compile_time_refusals_follow_the_staged_segments():
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx = E.Context(0)
    try:
        assert _compile_status(ctx, 15, b"x") == 0 and _compile_status(ctx, 14, b"x") == 0
        mv = E.IndexSegment(ctx, S.make_segment("kp1", [S.make_mv_column("x", [[1, 2], [3]], "INT")]))
        assert _compile_status(ctx, 15, b"x") == N.PGX_ERR_UNSUPPORTED and _compile_status(ctx, 14, b"x") == 0
        sv = E.IndexSegment(ctx, S.make_segment("kp0", [S.make_column("x", np.arange(40, dtype=np.int32) % 7)]))
        assert _compile_status(ctx, 15, b"x") == 0 and _compile_status(ctx, 14, b"x") == 0  # the execution decides
        for fn, text in (("percentile", "PERCENTILE on multi-value column"),
                         ("percentilemv", "multi-value function on single-value")):
            with pytest.raises(N.PgxError) as e:
                _native(ctx, [sv, mv], {"aggregations": [{"fn": fn, "column": "x"}], "group_by": None, "filter": None})
            assert e.value.status == N.PGX_ERR_UNSUPPORTED and text in str(e.value)
        got = _native(ctx, [mv], {"aggregations": [{"fn": "percentilemv", "column": "x"}], "group_by": None,
                                  "filter": None}).get_aggregation_result()
        assert got == [[(1.0, 1), (2.0, 1), (3.0, 1)]]
        mv.destroy()
        assert _compile_status(ctx, 15, b"x") == 0 and _compile_status(ctx, 14, b"x") == N.PGX_ERR_UNSUPPORTED
        sv.destroy()
    finally:
        ctx.close()


AGG_TEXT = ("SELECT PERCENTILE50(ci), PERCENTILE90(cl), PERCENTILE95(cf), PERCENTILE99(cd), PERCENTILE50MV(ti), "
            "PERCENTILEEST90(ci), PERCENTILEEST50MV(ti), MINMAXRANGEMV(ti), PERCENTILE99(ci) FROM t")


@pytest.mark.parametrize("fi", range(len(FILTERS)))
def test_aggregation_only(env, monkeypatch, fi):
    ctx, gsegs, osegs, raws = env
    where, pred = FILTERS[fi]
    masks = [pred(r) for r in raws]
    q = pql.compile(AGG_TEXT + where)
    blk = _native(ctx, gsegs, _library_request(q))
    got = blk.get_aggregation_result()
    exp = H.oracle_answer(osegs, q)
    calls = _calls(monkeypatch)
    on = _plan(ctx, gsegs, q)
    assert calls["n"] >= 5  # the request's nine functions name five columns: one native histogram each
    calls["n"] = 0
    off = _off(monkeypatch, ctx, gsegs, q)
    assert calls["n"] == 0
    models = {c: _model(raws, c, masks) for c in PCT_COLS}
    for i, col in enumerate(PCT_COLS):
        assert got[i] == models[col], col
        assert all(a[0] < b[0] for a, b in zip(got[i], got[i][1:]))  # ascending, equal values one entry
    for i, a in enumerate(q["aggregations"]):
        fn, col = X.base_fn(a["fn"]), a["column"]
        mine, theirs = on.get_aggregation_result()[i], off.get_aggregation_result()[i]
        if fn == "minmaxrange":
            assert mine == theirs == tuple(exp["results"][i])
        elif fn.startswith("percentileest"):
            assert mine.serialize() == theirs.serialize()
        else:
            assert mine == theirs == models[col] == _pairs_of_list(exp["results"][i]), a
            if fi != 1:  # reduced PERCENTILEnn: element (int)(size * p / 100) of the sorted list
                assert X.reduce_value(a["fn"], mine) == O.reduce_extended(a["fn"], exp["results"][i])
    if fi == 1:
        assert all(g == [] for g in got)
    docs = int(sum(m.sum() for m in masks))
    st = blk.stats.as_list()
    assert st[0] == docs and st[2] == docs * len(PCT_COLS) and st[3] == sum(SIZES)  # docs x columns, not x values
    assert on.stats.as_list() == off.stats.as_list()
    assert on.stats.as_list()[1] == H.literal_entries(osegs, q) and on.stats.as_list()[0] == exp["stats"][0]
    assert on.stats.as_list()[2] == exp["stats"][2] == docs * 5
    _same_blocks(on, off, q)


def test_aggregation_only_call_count_is_one_per_column(env, monkeypatch):
    """Nine functions over five columns in AGG_TEXT: the base query holds one percentile function per column."""
    base, slot = X._base_request(pql.compile(AGG_TEXT), X._NATIVE_PERCENTILE_FNS)
    assert [b["fn"] for b in base] == ["count", "percentile", "percentile", "percentile", "percentile", "percentilemv"]
    assert slot[0] == slot[5] == slot[8] == ("hist", 1) and slot[4] == slot[6] == slot[7] == ("hist", 5)


GROUPED = [
    ("SELECT PERCENTILE50(cl), SUM(m), PERCENTILE90MV(ti), PERCENTILEEST95(cl) FROM t%s GROUP BY g1", ("g1",)),
    ("SELECT COUNT(*), PERCENTILE95(ci), PERCENTILE50(cf), MINMAXRANGEMV(ti), PERCENTILE99(cd), "
     "PERCENTILEEST50MV(ti) FROM t%s GROUP BY g1, g2", ("g1", "g2")),                                   # 50 x 40 slots
]


@pytest.mark.parametrize("gi", range(len(GROUPED)))
@pytest.mark.parametrize("fi", [0, 1, 2, 5])
def test_group_by(env, monkeypatch, gi, fi):
    """The group columns' dictionaries differ between the segments (remaps); histograms per group of the result."""
    ctx, gsegs, osegs, raws = env
    where, pred = FILTERS[fi]
    masks = [pred(r) for r in raws]
    text, gcols = GROUPED[gi]
    q = pql.compile(text % where)
    cols = []
    for a in q["aggregations"]:
        if a["fn"] in X._NATIVE_PERCENTILE_FNS and a["column"] not in cols:
            cols.append(a["column"])

    def keys(r):
        return np.array(["\t".join(str(int(r[g][d])) for g in gcols) for d in range(_n(r))])

    blk = _native(ctx, gsegs, _library_request(q, cols))
    gr = blk.get_aggregation_group_by_result()
    got = gr.as_map() if gr is not None else {}
    exp = H.oracle_answer(osegs, q)
    assert (len(got) == 0) == (fi == 1) and set(got) == set(exp["map"])
    models = {c: _model(raws, c, masks, keys) for c in cols}
    for i, col in enumerate(cols):
        assert set(models[col]) == set(got)
        for k in got:  # every group of the result
            assert got[k][i] == models[col][k], (col, k)
    on, off = _plan(ctx, gsegs, q), _off(monkeypatch, ctx, gsegs, q)
    mon = on.get_aggregation_group_by_result()
    mon = mon.as_map() if mon is not None else {}
    for i, a in enumerate(q["aggregations"]):
        fn = X.base_fn(a["fn"])
        if not fn.startswith("percentile") or fn.startswith("percentileest"):
            continue
        for k in mon:
            assert mon[k][i] == models[a["column"]][k] == _pairs_of_list(exp["map"][k][i]), (a, k)
            assert X.reduce_value(a["fn"], mon[k][i]) == O.reduce_extended(a["fn"], exp["map"][k][i])
    assert on.stats.as_list() == off.stats.as_list()
    assert _same_blocks(on, off, q) == len(got)


def test_families_mixed_over_one_column(env, monkeypatch):
    """Standard, HLL, DISTINCTCOUNT and percentile functions in any order, over one column among others (counted once
    among the projected ones); two percentile functions over one column share one histogram; the accessors' argument
    errors."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, osegs, raws = env
    where, pred = FILTERS[4]
    masks = [pred(r) for r in raws]
    q = pql.compile("SELECT SUM(m), PERCENTILE50(cl), DISTINCTCOUNTHLL(cl), DISTINCTCOUNT(cl), MIN(m), "
                    "PERCENTILE90MV(ti), DISTINCTCOUNTMV(ti), PERCENTILE99(cl) FROM t" + where)
    on, off = _plan(ctx, gsegs, q), _off(monkeypatch, ctx, gsegs, q, others_too=True)
    _same_blocks(on, off, q)
    docs = int(sum(m.sum() for m in masks))
    assert on.stats.as_list()[2] == docs * 3  # m, cl, ti: each projected column once
    lib = {"aggregations": [{"fn": "sum", "column": "m"}, {"fn": "percentile", "column": "cl"},
                            {"fn": "distinctcounthll", "column": "cl"}, {"fn": "distinctcount", "column": "cl"},
                            {"fn": "percentilemv", "column": "ti"}, {"fn": "percentile", "column": "cl"},
                            {"fn": "distinctcountmv", "column": "ti"}],
           "group_by": None, "filter": q.get("filter")}
    blk = _native(ctx, gsegs, lib)
    res = blk.get_aggregation_result()
    assert blk.stats.as_list()[2] == docs * 3
    assert res[0] == float(sum(int(r["m"][m].sum()) for r, m in zip(raws, masks)))
    assert res[1] == res[5] == _model(raws, "cl", masks) and res[4] == _model(raws, "ti", masks)
    hashes = {X.java_hash_code("LONG", int(v)) for r, m in zip(raws, masks) for v in r["cl"][m]}
    assert res[3] == hashes and res[2].tobytes() == HLL.from_ints(hashes).tobytes()
    L = N.lib()
    qq = E._Query(ctx, lib)
    r = qq.execute(gsegs)
    try:
        n = len(res[1])
        v, c = C.c_double(), C.c_int64()
        cnt = np.zeros(2, np.int64)
        vals, vcnt = np.zeros(n + 8), np.zeros(n + 8, np.int64)
        codes, regs = np.zeros(4096, np.int32), np.zeros(256, np.uint8)
        assert L.pgx_result_agg(r, 1, C.byref(v), C.byref(c)) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_agg(r, 0, C.byref(v), C.byref(c)) == 0 and v.value == res[0]
        assert L.pgx_result_hll(r, 1, 0, 1, regs.ctypes.data) == N.PGX_ERR_INVALID_ARG        # a percentile index
        assert L.pgx_result_distinct_counts(r, 1, 0, 1, cnt.ctypes.data) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_distinct(r, 1, 0, 1, codes.ctypes.data, len(codes)) == N.PGX_ERR_INVALID_ARG
        for agg, first, k in ((0, 0, 1), (2, 0, 1), (3, 0, 1), (7, 0, 1), (-1, 0, 1), (1, 1, 1), (1, 0, 2), (1, -1, 1),
                              (1, 0, -1)):
            assert L.pgx_result_percentile_counts(r, agg, first, k, cnt.ctypes.data) == N.PGX_ERR_INVALID_ARG
            assert L.pgx_result_percentile(r, agg, first, k, vals.ctypes.data, vcnt.ctypes.data,
                                           len(vals)) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_percentile_counts(r, 1, 0, 1, None) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_percentile_counts(r, 5, 0, 1, cnt.ctypes.data) == 0 and cnt[0] == n
        assert L.pgx_result_percentile(r, 5, 0, 1, vals.ctypes.data, vcnt.ctypes.data, n - 1) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_percentile(r, 5, 0, 1, None, vcnt.ctypes.data, n) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_percentile(r, 5, 0, 1, vals.ctypes.data, None, n) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_percentile(r, 5, 0, 1, vals.ctypes.data, vcnt.ctypes.data, n) == 0
        assert list(zip(vals[:n].tolist(), vcnt[:n].tolist())) == res[1] and (vals[n:] == 0).all()
        assert L.pgx_result_percentile(r, 5, 1, 0, None, None, 0) == 0                        # an empty range
    finally:
        L.pgx_result_release(r)
        qq.close()


def test_group_accessors(env):
    """pgx_result_percentile_counts / pgx_result_percentile over sub-ranges of the groups, in the order of the other
    group accessors; the numeric accessors on a percentile index."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, _, raws = env
    L = N.lib()
    lib = {"aggregations": [{"fn": "percentile", "column": "cl"}, {"fn": "sum", "column": "m"},
                            {"fn": "percentilemv", "column": "ti"}],
           "group_by": {"columns": ["g1"], "top_n": 10}, "filter": None}
    qq = E._Query(ctx, lib)
    r = qq.execute(gsegs)
    try:
        gr = E.decode_result(qq, r, gsegs).get_aggregation_group_by_result()
        keys = [k.string_key for k in gr.get_group_key_iterator()]
        n = len(keys)
        assert n == 50
        model = _model(raws, "cl", [np.ones(_n(x), bool) for x in raws],
                       lambda x: np.array([str(int(v)) for v in x["g1"]]))
        full = E.result_percentile(r, 0, 0, n)
        assert [full[i] == model[k] for i, k in enumerate(keys)] == [True] * n
        for first, cnt in ((0, 1), (7, 13), (n - 1, 1), (n, 0), (0, 0)):
            assert E.result_percentile(r, 0, first, cnt) == full[first:first + cnt]
        counts = np.zeros(n, np.int64)
        assert L.pgx_result_percentile_counts(r, 0, 0, n, counts.ctypes.data) == 0
        assert counts.tolist() == [len(s) for s in full]
        for agg, first, cnt in ((0, -1, 1), (0, 0, n + 1), (0, n, 1), (0, n + 1, 0), (0, 0, -1), (1, 0, 1), (3, 0, 1)):
            assert L.pgx_result_percentile_counts(r, agg, first, cnt, counts.ctypes.data) == N.PGX_ERR_INVALID_ARG
        v, c = np.zeros(n), np.zeros(n, np.int64)
        cap = C.c_int64(n)
        idx = np.zeros(n, np.int64)
        assert L.pgx_result_group_values(r, 0, v.ctypes.data, c.ctypes.data) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_trim(r, 2, idx.ctypes.data, C.byref(cap)) == N.PGX_ERR_INVALID_ARG
        gi = np.array([3, 0], np.int64)
        gv, gc = np.full(6, -1.0), np.full(6, -1, np.int64)
        assert L.pgx_result_gather(r, gi.ctypes.data, 2, None, None, gv.ctypes.data, gc.ctypes.data) == 0
        assert L.pgx_result_group_values(r, 1, v.ctypes.data, c.ctypes.data) == 0
        assert gv.reshape(3, 2)[1].tolist() == [v[3], v[0]]                       # SUM(m)
        for a in (0, 2):
            assert gv.reshape(3, 2)[a].tolist() == [0.0, 0.0] and gc.reshape(3, 2)[a].tolist() == [0, 0]
    finally:
        L.pgx_result_release(r)
        qq.close()


def test_refused_shapes_fall_back_and_agree(env, monkeypatch):
    """A 70,000-slot key space: the library refuses, the plan maker gives what the decomposition gives, without a
    native histogram.  A STRING column: refused by the library and by the decomposition alike."""
    from pinot_amd import native as N
    ctx, gsegs, _, _ = env
    q = pql.compile("SELECT PERCENTILE50(ci), PERCENTILE90MV(ti), COUNT(*) FROM t WHERE m < 300 GROUP BY g1, h")
    assert _status(lambda: _native(ctx, gsegs, _library_request(q, ("ci", "ti")))) == N.PGX_ERR_UNSUPPORTED
    calls = _calls(monkeypatch)
    on = _plan(ctx, gsegs, q)
    assert calls["n"] == 0
    assert _same_blocks(on, _off(monkeypatch, ctx, gsegs, q), q) > 0
    lib = {"aggregations": [{"fn": "percentile", "column": "s"}], "group_by": None, "filter": None}
    with pytest.raises(N.PgxError) as e:
        _native(ctx, gsegs, lib)
    assert e.value.status == N.PGX_ERR_UNSUPPORTED and "STRING" in str(e.value)
    sq = pql.compile("SELECT PERCENTILE50(s) FROM t")
    assert _status(lambda: _plan(ctx, gsegs, sq)) == N.PGX_ERR_UNSUPPORTED
    assert _status(lambda: _off(monkeypatch, ctx, gsegs, sq)) == N.PGX_ERR_UNSUPPORTED


def test_table_limit(monkeypatch):
    """65,536 slots x a 600-value dictionary x 8 bytes is above PGX_PERCENTILE_MAX_TABLE_BYTES: refused before anything
    runs; the plan maker's answer equals the decomposition's.  GROUP BY one of the two columns fits."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx = E.Context(0)
    try:
        rng = np.random.default_rng(78)
        n = 1000
        ids = {"wide": rng.integers(0, 600, n), "k1": rng.integers(0, 256, n), "k2": rng.integers(0, 256, n)}
        dicts = {"wide": np.arange(600, dtype=np.int32) * 3, "k1": np.arange(256, dtype=np.int32),
                 "k2": np.arange(256, dtype=np.int32)}
        cols = [S.make_column(c, None, data_type="INT", dictionary=dicts[c], dict_ids=ids[c]) for c in ids]
        segs = [E.IndexSegment(ctx, S.make_segment("pcwide", cols))]
        assert 65536 * 600 * 8 > N.PGX_PERCENTILE_MAX_TABLE_BYTES
        q = pql.compile("SELECT PERCENTILE50(wide), COUNT(*) FROM t GROUP BY k1, k2")
        with pytest.raises(N.PgxError) as e:
            _native(ctx, segs, _library_request(q, ("wide",)))
        assert e.value.status == N.PGX_ERR_UNSUPPORTED and "PGX_PERCENTILE_MAX_TABLE_BYTES" in str(e.value)
        assert _same_blocks(_plan(ctx, segs, q), _off(monkeypatch, ctx, segs, q), q) > 256
        small = pql.compile("SELECT PERCENTILE50(wide), COUNT(*) FROM t GROUP BY k1")
        got = _native(ctx, segs, _library_request(small, ("wide",))).get_aggregation_group_by_result().as_map()
        raw = {c: dicts[c][ids[c]] for c in ids}
        for k in list(got)[:40]:
            assert got[k][0] == _pairs_of_list(raw["wide"][raw["k1"] == int(k)])
    finally:
        ctx.close()


def test_consuming_segment_after_an_append(monkeypatch):
    """A consuming segment queried after 700 and after 9,000 docs: the dictionaries grow in between."""
    from pinot_amd import engine as E
    from pinot_amd.realtime import RealtimeSegment
    from tests.test_realtime import SCHEMA, _rows
    ctx = E.Context(0)
    try:
        rng = np.random.default_rng(9)
        rt = RealtimeSegment("rt_percentile", SCHEMA, capacity=100000, inverted=["dim"])
        rows = _rows(rng, 9000)
        for r in rows:
            r["tags"] = [int(x) for x in rng.integers(-3000, 3000, size=int(rng.integers(1, 5)))]
        done = 0
        for stop in (700, 9000):
            for r in rows[done:stop]:
                rt.index(r)
            done = stop
            seg = rt.device_segment(ctx)
            for text in ("SELECT PERCENTILE50MV(tags), PERCENTILE90(lng), COUNT(*) FROM rt "
                         "WHERE dim BETWEEN -20 AND 20",
                         "SELECT PERCENTILE95MV(tags), SUM(met), PERCENTILEEST50(lng) FROM rt GROUP BY name"):
                q = pql.compile(text)
                on, off = _plan(ctx, [seg], q), _off(monkeypatch, ctx, [seg], q)
                groups = _same_blocks(on, off, q)
                if q.get("group_by"):
                    assert groups == 8
                else:
                    sel = [r for r in rows[:stop] if -20 <= r["dim"] <= 20]
                    exp = [_pairs_of_list(v for r in sel for v in r["tags"]), _pairs_of_list(r["lng"] for r in sel)]
                    assert on.get_aggregation_result()[:2] == exp
    finally:
        ctx.close()


def test_a_star_tree_request_keeps_the_decomposition(monkeypatch):
    from pinot_amd import engine as E
    from pinot_amd import startree as ST
    from tests.test_startree import make_raw
    ctx = E.Context(0)
    try:
        dims, mets = make_raw(6000, seed=5)
        gseg = E.IndexSegment(ctx, ST.make_star_tree_segment("pcst", dims, mets, max_leaf_records=500))
        q = pql.compile("SELECT PERCENTILE50(m2), SUM(m1) FROM T WHERE d1 = 1")
        raw_q = copy.deepcopy(q)
        raw_q["debug_options"] = {"useStarTree": "false"}
        assert not X.native_percentile(q, [gseg]) and X.native_percentile(raw_q, [gseg])
        calls = _calls(monkeypatch)
        star = _plan(ctx, [gseg], q)
        assert calls["n"] == 0
        on = _plan(ctx, [gseg], raw_q)
        assert calls["n"] >= 1
        _same_blocks(on, _off(monkeypatch, ctx, [gseg], raw_q), raw_q)
        sel = np.asarray(dims["d1"]) == 1
        assert on.get_aggregation_result()[0] == _pairs_of_list(np.asarray(mets["m2"])[sel])
        assert star.get_aggregation_result()[1] == on.get_aggregation_result()[1]  # SUM(m1) either way
    finally:
        ctx.close()
