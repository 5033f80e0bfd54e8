"""FASTHLL on the device (PGX_FASTHLL, pinot_amd/csrc/pgx_hll.cpp run_hll with pgx_fasthll.cpp over pgx_fasthll.hip):
the registers pgx_result_hll returns are compared, bit for bit, with the oracle's per-doc restatement (addAll of every
selected doc's deserialized estimator) and with the host decomposition (PGX_FASTHLL_NATIVE=0: a GROUP BY histogram
whose distinct strings are deserialized and merged in Python), statistics included.  Three segments of 3,000-5,000 rows
over pools of serialized estimators; segments 1 and 2 stage equal dictionaries of `h`, segment 0 another."""
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

SIZES = (3000, 4200, 5000)
TYPES = {"h": "STRING", "h2": "STRING", "ti": "INT"}


def _pool(seed, n):
    rng = np.random.default_rng(seed)
    return [HLL.to_string(HLL.from_ints(rng.integers(0, 1 << 24, int(rng.integers(1, 600))).tolist())) for _ in range(n)]


POOLS = (_pool(1, 60) + [HLL.to_string(HLL.empty())], _pool(2, 300))
POOL2 = _pool(3, 90)


def _raw(i, n):
    rng = np.random.default_rng(500 + i)
    pool = np.array(POOLS[min(i, 1)], dtype=object)
    h = pool[rng.integers(0, len(pool), n)]
    h[:len(pool)] = pool  # every value occurs: segments 1 and 2 stage equal dictionaries
    return {"h": h, "h2": np.array(POOL2, dtype=object)[rng.integers(0, len(POOL2), n)],
            "m": rng.integers(0, 1000, n).astype(np.int32),
            "v": rng.integers(0, 400, n).astype(np.int32),
            "g1": rng.permutation(np.arange(n) % 30).astype(np.int32),
            "g2": (rng.integers(0, 8 + 3 * i, n) + 2 * i).astype(np.int32),
            "ti": [rng.integers(0, 50, c).astype(np.int32).tolist() for c in rng.integers(1, 4, n)]}


def _segment(name, raw):
    cols = [S.make_mv_column(c, v, "INT") if c == "ti" else S.make_column(c, v, data_type=TYPES.get(c))
            for c, v in raw.items()]
    return S.make_segment(name, cols)


@pytest.fixture(scope="module")
def env():
    from pinot_amd import engine as E
    ctx = E.Context(0)
    gsegs, osegs, raws = [], [], []
    for i, n in enumerate(SIZES):
        raw = _raw(i, n)
        gsegs.append(E.IndexSegment(ctx, _segment("fh%d" % i, raw)))
        osegs.append(O.OSegment.from_raw(raw, dtypes={k: v for k, v in TYPES.items() if v != "INT"}))
        raws.append(raw)
    assert set(raws[1]["h"]) == set(raws[2]["h"]) != set(raws[0]["h"])
    yield ctx, gsegs, osegs, raws
    ctx.close()


FILTERS = [("", lambda r: np.ones(len(r["m"]), bool)),
           (" WHERE m BETWEEN 100 AND 140", lambda r: (r["m"] >= 100) & (r["m"] <= 140)),
           (" WHERE m = 123456", lambda r: np.zeros(len(r["m"]), bool))]


def _merged(raws, col, masks, keys=None):
    """The model: register-wise max over the selected docs' estimators (per group key)."""
    per = {}
    for r, m in zip(raws, masks):
        k = keys(r) if keys else np.zeros(len(m), dtype=object)
        for key in np.unique(k[m]):
            regs = per.setdefault(key, HLL.empty())
            for s in set(r[col][m & (k == key)].tolist()):
                regs = np.maximum(regs, HLL.from_string(s))
            per[key] = regs
    return per if keys else per.get(0, HLL.empty())


def _native(ctx, gsegs, q, flags=0):
    """The request as ONE library query through E._Query (function code 16, registers from pgx_result_hll)."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    qq = E._Query(ctx, q)
    try:
        r = qq.execute(gsegs, flags)
        try:
            return E.decode_result(qq, r, gsegs, trim=bool(q.get("group_by")))
        finally:
            N.lib().pgx_result_release(r)
    finally:
        qq.close()


def _plan(ctx, gsegs, q):
    from pinot_amd import engine as E
    return E.InstancePlanMakerImplV2(ctx).make_inter_segment_plan(gsegs, q).execute()


def _off(monkeypatch, ctx, gsegs, q):
    monkeypatch.setenv("PGX_FASTHLL_NATIVE", "0")
    try:
        return _plan(ctx, gsegs, q)
    finally:
        monkeypatch.delenv("PGX_FASTHLL_NATIVE")


def _status(fn):
    from pinot_amd import native as N
    with pytest.raises(N.PgxError) as e:
        fn()
    return e.value.status


def _eq(a, b):
    return (a == b) if isinstance(a, (set, int, float, tuple)) else np.array_equal(np.asarray(a), np.asarray(b))


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
                    assert X.reduce_value(f, a) == X.reduce_value(f, b)
        ton, toff = getattr(on, "trimmed", None), getattr(off, "trimmed", None)
        assert (ton is None) == (toff is None)
        for f, a, b in zip(fns, ton or [], toff or []):
            assert set(a) == set(b) and all(_eq(a[k], b[k]) for k in a), f
        return len(mon)
    for f, a, b in zip(fns, on.get_aggregation_result(), off.get_aggregation_result()):
        assert _eq(a, b), f
        if f in X.EXT_FUNCTIONS and not (f.startswith("percentile") and not a):
            assert X.reduce_value(f, a) == X.reduce_value(f, b)
    return 1


def _count_native(monkeypatch):
    """Counts the register reads (pgx_result_hll) of the blocks decoded from now on."""
    from pinot_amd import engine as E
    calls = {"hll": 0}
    real = E.result_hll

    def counted(*a, **k):
        calls["hll"] += 1
        return real(*a, **k)
    monkeypatch.setattr(E, "result_hll", counted)
    return calls


def _compile_status(ctx, fn, column):
    from pinot_amd import native as N
    agg = (N.Agg * 1)()
    agg[0].fn, agg[0].column = fn, column
    qd = N.QueryDesc(1, agg, 0, None, 10, 0, None, 0, None, 0)
    h = C.c_void_p()
    st = N.lib().pgx_query_compile(ctx.handle, C.byref(qd), C.byref(h))
    if st == 0:
        N.check(N.lib().pgx_query_release(h))
    return st


def test_function_code_and_compile_time_refusals(env):
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, _, _, _ = env
    assert E._FN["fasthll"] == N.PGX_FASTHLL == 16
    assert _compile_status(ctx, 16, b"h") == 0 and _compile_status(ctx, 16, b"no_such_column") == 0
    assert _compile_status(ctx, 16, b"m") == N.PGX_ERR_UNSUPPORTED   # single-value, not STRING
    assert _compile_status(ctx, 16, b"ti") == N.PGX_ERR_UNSUPPORTED  # multi-value
    assert _compile_status(ctx, 17, b"h") == N.PGX_ERR_UNSUPPORTED
    other = E.Context(0)
    try:
        assert _compile_status(other, 16, b"x") == 0
        num = E.IndexSegment(other, S.make_segment("k0", [S.make_column("x", np.arange(40, dtype=np.int32) % 7)]))
        assert _compile_status(other, 16, b"x") == N.PGX_ERR_UNSUPPORTED
        st = E.IndexSegment(other, S.make_segment("k1", [S.make_column("x", np.array(POOL2[:5], dtype=object))]))
        assert _compile_status(other, 16, b"x") == 0  # the execution decides, and refuses the numeric segment
        q = pql.compile("SELECT FASTHLL(x) FROM t")
        with pytest.raises(N.PgxError) as e:
            _native(other, [st, num], q)
        assert e.value.status == N.PGX_ERR_UNSUPPORTED and "non-STRING" in str(e.value)
        got = _native(other, [st], q).get_aggregation_result()[0]
        assert np.array_equal(got, np.maximum.reduce([HLL.from_string(s) for s in POOL2[:5]]))
        st.destroy()
        assert _compile_status(other, 16, b"x") == N.PGX_ERR_UNSUPPORTED
        num.destroy()
    finally:
        other.close()


@pytest.mark.parametrize("fi", range(len(FILTERS)))
def test_aggregation_only(env, monkeypatch, fi):
    ctx, gsegs, osegs, raws = env
    where, pred = FILTERS[fi]
    masks = [pred(r) for r in raws]
    docs = sum(int(m.sum()) for m in masks)
    assert (fi == 0 and docs == sum(SIZES)) or (fi == 2 and docs == 0) or 0 < docs < sum(SIZES) // 10
    q = pql.compile("SELECT FASTHLL(h), COUNT(*) FROM t" + where)
    blk = _native(ctx, gsegs, q)
    got = blk.get_aggregation_result()
    exp = H.oracle_answer(osegs, q)["results"]
    assert got[0].dtype == np.uint8 and got[0].shape == (256,)
    assert np.array_equal(got[0], np.asarray(exp[0])) and np.array_equal(got[0], _merged(raws, "h", masks))
    assert int(got[1]) == int(exp[1]) == docs
    assert HLL.cardinality(got[0]) == O.reduce_extended("fasthll", exp[0])
    assert blk.stats.as_list()[2] == docs  # h counts once among the projected columns
    calls = _count_native(monkeypatch)
    on = _plan(ctx, gsegs, q)
    assert calls["hll"] > 0
    calls["hll"] = 0
    off = _off(monkeypatch, ctx, gsegs, q)
    assert calls["hll"] == 0
    assert blk.stats.as_list() == on.stats.as_list()
    _same_blocks(on, off, q)


GROUPED = [("SELECT FASTHLL(h), SUM(m) FROM t%s GROUP BY g1", ("g1",)),
           ("SELECT COUNT(*), FASTHLL(h2), FASTHLL(h) FROM t%s GROUP BY g1, g2", ("g1", "g2"))]


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("gi", range(len(GROUPED)))
@pytest.mark.parametrize("fi", range(len(FILTERS)))
def test_group_by(env, monkeypatch, gi, fi, sparse):
    """Dense key spaces of one and two columns (g2's dictionaries differ between the segments), and the same requests
    through the hash table and the group directory (PGX_X_SPARSE_GROUP_SETS with PGX_X_FORCE_HASH)."""
    from pinot_amd import native as N
    ctx, gsegs, osegs, raws = env
    where, pred = FILTERS[fi]
    masks = [pred(r) for r in raws]
    text, gcols = GROUPED[gi]
    q = pql.compile(text % where)

    def keys(r):
        return np.array(["\t".join(str(int(r[g][d])) for g in gcols) for d in range(len(r["m"]))], dtype=object)
    blk = _native(ctx, gsegs, q, flags=(N.PGX_X_SPARSE_GROUP_SETS | N.PGX_X_FORCE_HASH) if sparse else 0)
    gr = blk.get_aggregation_group_by_result()
    got = gr.as_map() if gr is not None else {}
    exp = H.oracle_answer(osegs, q)["map"]
    assert (len(got) == 0) == (fi == 2) and set(got) == set(exp)
    for i, a in enumerate(q["aggregations"]):
        if a["fn"] != "fasthll":
            continue
        model = _merged(raws, a["column"], masks, keys)
        assert set(model) == set(got)
        for k in got:
            assert np.array_equal(got[k][i], model[k]) and np.array_equal(got[k][i], np.asarray(exp[k][i])), (a, k)
    if not sparse:
        on, off = _plan(ctx, gsegs, q), _off(monkeypatch, ctx, gsegs, q)
        assert blk.stats.as_list() == on.stats.as_list()
        assert _same_blocks(on, off, q) == len(got)


def test_sparse_flag_is_needed_for_a_hash_key_space(env):
    from pinot_amd import native as N
    ctx, gsegs, _, _ = env
    q = pql.compile(GROUPED[0][0] % "")
    assert _status(lambda: _native(ctx, gsegs, q, flags=N.PGX_X_FORCE_HASH)) == N.PGX_ERR_UNSUPPORTED


@pytest.mark.parametrize("seed", [0, 1])
def test_functions_mixed_in_shuffled_order(env, monkeypatch, seed):
    """FASTHLL beside COUNT, SUM, DISTINCTCOUNTHLL, DISTINCTCOUNT and PERCENTILE, twice over one column, in a shuffled
    order; aggregation-only and grouped."""
    ctx, gsegs, osegs, raws = env
    fns = ["FASTHLL(h)", "COUNT(*)", "SUM(m)", "DISTINCTCOUNTHLL(v)", "DISTINCTCOUNT(h)", "PERCENTILE90(v)",
           "FASTHLL(h)", "FASTHLL(h2)", "DISTINCTCOUNTHLL(h)"]
    order = np.random.default_rng(seed).permutation(len(fns))
    where, pred = FILTERS[1]
    masks = [pred(r) for r in raws]
    docs = sum(int(m.sum()) for m in masks)
    for tail in ("", " GROUP BY g1"):
        q = pql.compile("SELECT " + ", ".join(fns[i] for i in order) + " FROM t" + where + tail)
        on, off = _plan(ctx, gsegs, q), _off(monkeypatch, ctx, gsegs, q)
        _same_blocks(on, off, q)
        assert on.stats.as_list()[2] == docs * (4 + (1 if tail else 0))  # h, m, v, h2 (and g1): each once
        exp = H.oracle_answer(osegs, q)
        if tail:
            got = on.get_aggregation_group_by_result().as_map()
            model = {c: _merged(raws, c, masks, lambda r: np.array([str(int(x)) for x in r["g1"]], dtype=object))
                     for c in ("h", "h2")}
            for k in got:
                for j, a in enumerate(q["aggregations"]):
                    if a["fn"] == "fasthll":
                        assert np.array_equal(got[k][j], model[a["column"]][k]), (k, j)
                        assert np.array_equal(got[k][j], np.asarray(exp["map"][k][j]))
        else:
            got = on.get_aggregation_result()
            for j, a in enumerate(q["aggregations"]):
                if a["fn"] == "fasthll":
                    assert np.array_equal(got[j], _merged(raws, a["column"], masks))
                    assert np.array_equal(got[j], np.asarray(exp["results"][j]))


def test_accessors_treat_the_index_as_an_hll_index(env):
    """The raw ABI: one query holds all four families, in this order: codes 12, 16, 1, 10, 15."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, _, _ = env
    L = N.lib()
    q = {"aggregations": [{"fn": f, "column": c} for f, c in (("distinctcount", "h"), ("fasthll", "h"), ("sum", "m"),
                                                               ("distinctcounthll", "v"), ("percentile", "v"))],
         "group_by": {"columns": ["g1"], "top_n": 10}, "filter": None}
    qq = E._Query(ctx, q)
    r = qq.execute(gsegs)
    try:
        n = 30
        regs = E.result_hll(r, 1, 0, n)
        assert regs.shape == (n, 256) and np.array_equal(E.result_hll(r, 1, 7, 5), regs[7:12])
        buf = np.zeros(256, np.uint8)
        for agg in (0, 2, 4, 5, -1):
            assert L.pgx_result_hll(r, agg, 0, 1, buf.ctypes.data) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_hll(r, 1, 0, n + 1, buf.ctypes.data) == N.PGX_ERR_INVALID_ARG
        v, c, idx, cap = np.zeros(n), np.zeros(n, np.int64), np.zeros(n, np.int64), C.c_int64(n)
        assert L.pgx_result_group_values(r, 1, v.ctypes.data, c.ctypes.data) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_trim(r, 1, idx.ctypes.data, C.byref(cap)) == N.PGX_ERR_INVALID_ARG
        cnt = np.zeros(n, np.int64)
        assert L.pgx_result_distinct_counts(r, 1, 0, 1, cnt.ctypes.data) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_percentile_counts(r, 1, 0, 1, cnt.ctypes.data) == N.PGX_ERR_INVALID_ARG
        gi = np.array([3, 0], np.int64)
        gv, gc = np.full(10, -1.0), np.full(10, -1, np.int64)
        assert L.pgx_result_gather(r, gi.ctypes.data, 2, None, None, gv.ctypes.data, gc.ctypes.data) == 0
        assert gv.reshape(5, 2)[1].tolist() == [0.0, 0.0] and gc.reshape(5, 2)[1].tolist() == [0, 0]
        assert L.pgx_result_group_values(r, 2, v.ctypes.data, c.ctypes.data) == 0
        assert gv.reshape(5, 2)[2].tolist() == [v[3], v[0]]
    finally:
        L.pgx_result_release(r)
        qq.close()


def test_refusals(env, monkeypatch):
    """Every refusal of the HLL forms holds for FASTHLL: PGX_ERR_UNSUPPORTED, and through the plan maker the request
    gives what the decomposition gives."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, _, _ = env
    L = N.lib()
    for text in ("SELECT FASTHLL(h), SUMMV(ti) FROM t WHERE m < 500",             # a standard MV function
                 "SELECT FASTHLL(h), COUNT(*) FROM t WHERE m < 100 GROUP BY ti"):  # a multi-value group column
        q = pql.compile(text)
        assert _status(lambda: _native(ctx, gsegs, q)) == N.PGX_ERR_UNSUPPORTED, text
        assert _same_blocks(_plan(ctx, gsegs, q), _off(monkeypatch, ctx, gsegs, q), q) > 0, text
    for text in ("SELECT FASTHLL(ti) FROM t", "SELECT FASTHLL(m) FROM t"):  # multi-value; not STRING
        q = pql.compile(text)
        assert _status(lambda: _native(ctx, gsegs, q)) == N.PGX_ERR_UNSUPPORTED
        assert _status(lambda: _plan(ctx, gsegs, q)) == N.PGX_ERR_UNSUPPORTED  # the decomposition refuses it too
    q = pql.compile(GROUPED[0][0] % "")
    qq = E._Query(ctx, q)
    try:
        assert _status(lambda: qq.execute_multi(gsegs)) == N.PGX_ERR_UNSUPPORTED
        assert _status(lambda: qq.set_key_domain(0, list(range(30)), "INT")) == N.PGX_ERR_UNSUPPORTED
        assert _status(lambda: qq.execute(gsegs, flags=N.PGX_X_KEEP_DENSE_ON_DEVICE)) == N.PGX_ERR_UNSUPPORTED
        dense = C.c_void_p()
        N.check(L.pgx_device_alloc(ctx.handle, 1 << 16, C.byref(dense)))
        try:
            assert _status(lambda: qq.execute(gsegs, dense_out=dense, dense_out_bytes=1 << 16)) == N.PGX_ERR_UNSUPPORTED
        finally:
            L.pgx_device_free(ctx.handle, dense)
        segs = (C.c_void_p * len(gsegs))(*[s.handle.value for s in gsegs])
        slots = C.c_int64()
        assert L.pgx_query_dense_slots(qq.handle, segs, len(gsegs), C.byref(slots)) == N.PGX_ERR_UNSUPPORTED
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


def test_a_refused_fasthll_leaves_the_other_families_native(env, monkeypatch):
    """A dictionary value that is no estimator: the library refuses the FASTHLL function and the request ends as the
    decomposition ends it; a DISTINCTCOUNTHLL beside a FASTHLL over a sound column of that segment stays native."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, _, raws = env
    raw = dict(_raw(0, 3000))
    raw["h"] = raw["h"].copy()
    raw["h"][17] = POOLS[0][3][:-1]  # 179 chars
    bad = E.IndexSegment(ctx, _segment("fh_bad", raw))
    try:
        q = pql.compile("SELECT FASTHLL(h), DISTINCTCOUNTHLL(v) FROM t WHERE m < 900")
        with pytest.raises(N.PgxError) as e:
            _native(ctx, [gsegs[1], bad], q)
        assert e.value.status == N.PGX_ERR_UNSUPPORTED and "not a serialized" in str(e.value)
        ends = []
        for native in ("1", "0"):
            monkeypatch.setenv("PGX_FASTHLL_NATIVE", native)
            try:
                _plan(ctx, [gsegs[1], bad], q)
                ends.append(None)
            except Exception as ex:  # noqa: BLE001  (whatever the decomposition raises, the native route raises too)
                ends.append((type(ex), getattr(ex, "status", None)))
            finally:
                monkeypatch.delenv("PGX_FASTHLL_NATIVE")
        assert ends[0] == ends[1] and ends[0] is not None
        # rows the filter leaves out do not matter: the image holds the whole dictionary
        q2 = pql.compile("SELECT FASTHLL(h) FROM t WHERE m = 123456")
        assert _status(lambda: _native(ctx, [bad], q2)) == N.PGX_ERR_UNSUPPORTED
        # beside a good FASTHLL column the other family stays on its route: registers are read natively
        q3 = pql.compile("SELECT FASTHLL(h2), DISTINCTCOUNTHLL(v) FROM t WHERE m < 900")
        calls = _count_native(monkeypatch)
        on = _plan(ctx, [gsegs[1], bad], q3)
        assert calls["hll"] >= 2
        _same_blocks(on, _off(monkeypatch, ctx, [gsegs[1], bad], q3), q3)
    finally:
        bad.destroy()
