"""Selection with ORDER BY over segments with multi-value columns, end to end on the GPU path: at the ABI with
PGX_Q_SELECT_MV (pgx_select_compile / pgx_execute / pgx_result_select_kinds, _mv_offsets, _mv_values), through the plan
maker, the server and the broker reduce with PGX_SELECT_MV_NATIVE=1, and over a realtime snapshot -- against a numpy
restatement by value.  The project's (key, docId) tie rule, (segment, docId) across segments, makes that restatement
unique."""
import ctypes as C

import numpy as np
import pytest

from pinot_amd import pql

pytestmark = pytest.mark.gpu

TYPES = {"a": "INT", "b": "INT", "v": "INT", "s": "STRING", "f": "FLOAT"}
MV = ("v", "s", "f")


@pytest.fixture(scope="module")
def ctx():
    from pinot_amd import engine as E
    c = E.Context(0)
    yield c
    c.close()


def _raw(seed, n, shift):
    """One segment's raw columns; `shift` moves every value domain, so two segments get different dictionaries that
    overlap in value."""
    rng = np.random.default_rng(seed)
    return {"a": (rng.integers(0, 50, n) * 2 + shift).astype(np.int32),
            "b": (rng.integers(0, 700, n) + 3 * shift).astype(np.int32),
            "v": [rng.integers(shift, shift + 9, 1 + i % 3).astype(np.int32) for i in range(n)],
            "s": [["t%02d" % x for x in rng.integers(shift, shift + 30, 1 + (i // 7) % 2)] for i in range(n)],
            "f": [(rng.integers(-8, 9 + shift, 1 + i % 4) / 4.0).astype(np.float32) for i in range(n)]}


def _stage(ctx, name, raw):
    from pinot_amd import engine as E
    from pinot_amd import segment as S
    cols = [S.make_mv_column(c, raw[c], TYPES[c]) if c in MV else S.make_column(c, raw[c]) for c in raw]
    return E.IndexSegment(ctx, S.make_segment(name, cols))


@pytest.fixture(scope="module")
def two(ctx):
    raws = [_raw(31, 9000, 0), _raw(32, 7000, 5)]
    return raws, [_stage(ctx, "mv%d" % i, r) for i, r in enumerate(raws)]


def _cell(col, x):
    if col in MV:
        return [_cell(None, y) for y in x]
    if isinstance(x, (str, np.str_)):
        return str(x)
    return float(x) if isinstance(x, (np.floating, float)) else int(x)


def _model(raws, masks, order, schema, k):
    """order: [(single-value column, ascending)] -> (per-segment lists, merged list) of (row in schema order,
    (segment, docId)), each cut to k: by value, ties by (segment, docId)."""
    seg = np.concatenate([np.full(int(m.sum()), s) for s, m in enumerate(masks)])
    doc = np.concatenate([np.flatnonzero(m) for m in masks])
    keys = []
    for c, asc in order:
        vals = np.concatenate([np.asarray(r[c])[m] for r, m in zip(raws, masks)]).astype(np.int64)
        keys.append(vals if asc else -vals)
    idx = np.lexsort([doc, seg] + keys[::-1])
    def rows(ids):
        return [([_cell(c, raws[s][c][d]) for c in schema], (int(s), int(d))) for s, d in ids]

    ranked = [(seg[i], doc[i]) for i in idx]
    return [rows([x for x in ranked if x[0] == s][:k]) for s in range(len(raws))], rows(ranked[:k])


def _abi(ctx, gsegs, text, flags=None):
    """The request at the ABI with PGX_Q_SELECT_MV (or `flags`): decode_selection's (stats, names, types, lists)."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    q = E._SelectQuery(ctx, pql.compile(text), flags=N.PGX_Q_SELECT_MV if flags is None else flags)
    try:
        r = q.execute(gsegs)
        try:
            return E.decode_selection(q, r, gsegs)
        finally:
            N.lib().pgx_result_release(r)
    finally:
        q.close()


def _refusal(fn):
    from pinot_amd import native as N
    with pytest.raises(N.PgxError) as e:
        fn()
    return e.value.status, str(e.value)


def _count_stats(ctx, gsegs, where):
    from pinot_amd import engine as E
    return E.InstancePlanMakerImplV2(ctx).make_inter_segment_plan(gsegs, pql.compile("SELECT COUNT(*) FROM t" + where)) \
        .execute().stats.as_list()


def _mask(raw, where):
    n = len(raw["a"])
    if not where:
        return np.ones(n, bool)
    assert where == " WHERE v IN (3, 7) AND a > 10"
    return np.array([bool(set(x.tolist()) & {3, 7}) for x in raw["v"]]) & (raw["a"] > 10)


CASES = [
    ("SELECT a, v FROM t%s ORDER BY a, b LIMIT 20", "", [("a", True), ("b", True)], ["a", "b", "v"]),
    ("SELECT * FROM t%s ORDER BY b DESC, a LIMIT 15", "", [("b", False), ("a", True)], ["b", "a", "f", "s", "v"]),
    ("SELECT f, s FROM t%s ORDER BY a DESC, b LIMIT 5, 40", " WHERE v IN (3, 7) AND a > 10",
     [("a", False), ("b", True)], ["a", "b", "f", "s"]),
    ("SELECT v FROM t%s ORDER BY a, v DESC, b LIMIT 300", "", [("a", True), ("b", True)], ["a", "v", "b"]),
]


@pytest.mark.parametrize("text,where,order,schema", CASES)
def test_abi_with_the_flag(ctx, two, text, where, order, schema):
    """Selected multi-value columns (INT, STRING and FLOAT; also through *), a filter with a multi-value leaf, a
    multi-value ORDER BY column that takes no part in the key, two segments with different dictionaries merged by
    value, and all four statistics."""
    from pinot_amd import engine as E
    raws, gsegs = two
    q = pql.compile(text % where)
    k = q["selections"]["offset"] + q["selections"]["size"]
    per, merged = _model(raws, [_mask(r, where) for r in raws], order, schema, k)
    stats, names, types, lists = _abi(ctx, gsegs, text % where)
    assert names == schema
    assert types == [TYPES[c] + ("_ARRAY" if c in MV else "") for c in schema]
    assert lists == per
    assert E.merge_selection_rows(lists, types, q["selections"]["order_by"], k) == merged
    matched = sum(int(_mask(r, where).sum()) for r in raws)
    assert matched > k
    assert stats.as_list() == [matched, _count_stats(ctx, gsegs, where)[1], matched * len(schema),
                               sum(len(r["a"]) for r in raws)]
    for s, gseg in enumerate(gsegs):  # one segment alone returns the same rows
        one = _abi(ctx, [gseg], text % where)[3][0]
        assert [(row, d) for row, (_, d) in one] == [(row, d) for row, (_, d) in per[s]]


def test_multi_value_order_column_is_no_part_of_the_key(ctx, two):
    """ORDER BY a, v DESC, b equals ORDER BY a, b plus the v column in second schema position."""
    raws, gsegs = two
    _, names, _, with_v = _abi(ctx, gsegs, "SELECT s FROM t ORDER BY a, v DESC, b LIMIT 50")
    _, plain_names, _, plain = _abi(ctx, gsegs, "SELECT s, v FROM t ORDER BY a, b LIMIT 50")
    assert names == ["a", "v", "b", "s"] and plain_names == ["a", "b", "s", "v"]
    assert [[([r[0], r[2], r[3], r[1]], d) for r, d in lst] for lst in with_v] == plain
    assert sum(len(lst) for lst in plain) == 100


def test_accessors(ctx, two):
    """The raw accessors: kinds, the value count in pgx_result_select_rows' dict_ids, offsets over the same row order,
    dictIds in the doc's own value order; PGX_ERR_INVALID_ARG for a single-value column and on another kind of
    result."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    L = N.lib()
    raws, gsegs = two
    q = E._SelectQuery(ctx, pql.compile("SELECT v, a FROM t ORDER BY b, a LIMIT 2048"), flags=N.PGX_Q_SELECT_MV)
    aq = E._Query(ctx, pql.compile("SELECT COUNT(*) FROM t"))
    try:
        r = q.execute(gsegs)
        kinds = np.full(3, -1, np.int32)
        assert L.pgx_result_select_kinds(r, kinds.ctypes.data) == 0 and kinds.tolist() == [0, 0, 1]
        counts = np.zeros(2, np.int32)
        N.check(L.pgx_result_select_counts(r, counts.ctypes.data))
        total = int(counts.sum())
        assert counts.tolist() == [2048, 2048]
        seg, doc, ids = np.zeros(total, np.int32), np.zeros(total, np.int32), np.zeros(3 * total, np.int32)
        N.check(L.pgx_result_select_rows(r, seg.ctypes.data, doc.ctypes.data, ids.ctypes.data))
        off = np.full(total + 1, -1, np.int64)
        assert L.pgx_result_select_mv_offsets(r, 2, off.ctypes.data) == 0
        assert off[0] == 0 and (np.diff(off) == ids[2 * total:]).all()
        val = np.full(int(off[-1]), -1, np.int32)
        assert L.pgx_result_select_mv_values(r, 2, val.ctypes.data) == 0
        dicts = [np.unique(np.concatenate(r["v"])) for r in raws]  # the segments' sorted dictionaries
        for j in range(total):
            np.testing.assert_array_equal(dicts[seg[j]][val[off[j]:off[j + 1]]], raws[seg[j]]["v"][doc[j]])
        for c in (0, 1, -1, 3):
            assert L.pgx_result_select_mv_offsets(r, c, off.ctypes.data) == N.PGX_ERR_INVALID_ARG
            assert L.pgx_result_select_mv_values(r, c, val.ctypes.data) == N.PGX_ERR_INVALID_ARG
        L.pgx_result_release(r)
        r = aq.execute(gsegs)
        assert L.pgx_result_select_kinds(r, kinds.ctypes.data) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_select_mv_offsets(r, 0, off.ctypes.data) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_select_mv_values(r, 0, val.ctypes.data) == N.PGX_ERR_INVALID_ARG
        L.pgx_result_release(r)
    finally:
        q.close()
        aq.close()


def test_refusals_with_and_without_the_flag(ctx, two):
    from pinot_amd import native as N
    from pinot_amd import segment as S
    from pinot_amd import engine as E
    raws, gsegs = two
    status, msg = _refusal(lambda: _abi(ctx, gsegs, "SELECT a FROM t ORDER BY v LIMIT 5"))
    assert status == N.PGX_ERR_UNSUPPORTED and "ORDER BY multi-value columns only" in msg
    status, msg = _refusal(lambda: _abi(ctx, gsegs, "SELECT a FROM t ORDER BY v, s DESC LIMIT 5"))
    assert status == N.PGX_ERR_UNSUPPORTED and "ORDER BY multi-value columns only" in msg
    # v multi-value in one segment of the call and single-value in the other
    rng = np.random.default_rng(4)
    sv = E.IndexSegment(ctx, S.make_segment("flat", [S.make_column(c, rng.integers(0, 9, 500).astype(np.int32))
                                                     for c in ("a", "b", "v")]))
    for segs in ([gsegs[0], sv], [sv, gsegs[0]]):
        status, msg = _refusal(lambda: _abi(ctx, segs, "SELECT v FROM t ORDER BY a LIMIT 5"))
        assert status == N.PGX_ERR_UNSUPPORTED and "in one segment" in msg
        status, _ = _refusal(lambda: _abi(ctx, segs, "SELECT b FROM t ORDER BY a, v LIMIT 5"))
        assert status == N.PGX_ERR_UNSUPPORTED
    assert len(_abi(ctx, [sv], "SELECT v FROM t ORDER BY a LIMIT 5")[3][0]) == 5  # single-value everywhere: runs
    sv.destroy()
    # the limits count the single-value order columns only
    eight = "SELECT b FROM t ORDER BY a, a, a, a, a, a, a, a%s LIMIT 3"
    assert len(_abi(ctx, gsegs[:1], eight % ", v")[3][0]) == 3
    status, msg = _refusal(lambda: _abi(ctx, gsegs[:1], eight % ", v, b"))
    assert status == N.PGX_ERR_UNSUPPORTED and "more than 8 ORDER BY columns" in msg
    # without the flag every request with a multi-value column is refused as before
    for text, part in (("SELECT a, v FROM t ORDER BY a, b LIMIT 20", "selection of multi-value column v"),
                       ("SELECT * FROM t ORDER BY a LIMIT 20", "selection of multi-value column f"),
                       ("SELECT a FROM t ORDER BY a, v DESC, b", "ORDER BY multi-value column v"),
                       (eight % ", v", "more than 8 ORDER BY columns")):
        status, msg = _refusal(lambda: _abi(ctx, gsegs, text, flags=0))
        assert status == N.PGX_ERR_UNSUPPORTED and part in msg


def test_plan_maker_server_and_broker(ctx, two, monkeypatch):
    """Through InstancePlanMakerImplV2, ServerQueryExecutor, the DataTable and the broker reduce: refused by default,
    typed rows under an _ARRAY schema and rendered rows with PGX_SELECT_MV_NATIVE=1 (read at every request)."""
    from pinot_amd import broker as B
    from pinot_amd import datatable as D
    from pinot_amd import engine as E
    from pinot_amd import native as N
    raws, gsegs = two
    q = pql.compile("SELECT s, v, f, a FROM t WHERE v IN (3, 7) AND a > 10 ORDER BY b DESC, a LIMIT 3, 12")
    where = " WHERE v IN (3, 7) AND a > 10"
    schema = ["b", "a", "f", "s", "v"]
    pm = E.InstancePlanMakerImplV2(ctx)
    monkeypatch.delenv("PGX_SELECT_MV_NATIVE", raising=False)
    assert _refusal(lambda: pm.make_inter_segment_plan(gsegs, q).execute())[0] == N.PGX_ERR_UNSUPPORTED
    assert B.ServerQueryExecutor(ctx).process_query(q, gsegs).exceptions
    monkeypatch.setenv("PGX_SELECT_MV_NATIVE", "1")
    per, merged = _model(raws, [_mask(r, where) for r in raws], [("b", False), ("a", True)], schema, 15)
    blk = pm.make_inter_segment_plan(gsegs, q).execute()
    assert blk.get_selection_data_schema() == (schema, ["INT", "INT", "FLOAT_ARRAY", "STRING_ARRAY", "INT_ARRAY"])
    assert blk.get_selection_result() == [r[0] for r in merged] and blk.selection_row_ids == [r[1] for r in merged]
    op = pm.make_inner_segment_plan(gsegs[1], q).run()
    assert op.next_block().get_selection_result() == [r[0] for r in per[1]]
    resp = B.ServerQueryExecutor(ctx).process_query(q, gsegs)
    assert not resp.exceptions
    wire = D.response_to_datatable(q, resp)
    assert D.response_to_datatable(q, D.datatable_to_response(q, wire)) == wire
    # two servers, a segment each
    wires = {"s%d" % i: D.response_to_datatable(q, B.ServerQueryExecutor(ctx).process_query(q, [g]))
             for i, g in enumerate(gsegs)}
    for out in (B.BrokerReduceService().reduce_on_data_table(q, {"server0": wire}),
                B.BrokerReduceService().reduce_on_data_table(q, wires)):
        assert out.processing_exceptions == []
        matched = sum(int(_mask(r, where).sum()) for r in raws)
        assert (out.num_docs_scanned, out.num_entries_scanned_post_filter) == (matched, matched * 5)
        assert out.selection_results.columns == ["s", "v", "f", "a"]
        exp = [[row[3], [str(x) for x in row[4]], [B.format_selection_value("FLOAT", x) for x in row[2]], str(row[1])]
               for row, _ in merged[3:]]
        assert out.selection_results.results == exp and len(exp) == 12
    monkeypatch.setenv("PGX_SELECT_MV_NATIVE", "0")
    assert _refusal(lambda: pm.make_inter_segment_plan(gsegs, q).execute())[0] == N.PGX_ERR_UNSUPPORTED


def test_realtime_snapshot(ctx, monkeypatch):
    """A consuming segment with a multi-value dimension, queried after each of two ingestion steps."""
    from pinot_amd import engine as E
    from pinot_amd.realtime import RealtimeSegment
    schema = {"dim": ("INT", True, "DIMENSION"), "tags": ("INT", False, "DIMENSION"), "met": ("INT", True, "METRIC"),
              "ts": ("LONG", True, "TIME")}
    rng = np.random.default_rng(17)
    rows = [{"dim": int(rng.integers(-40, 40)), "tags": [int(x) for x in rng.integers(0, 12, int(rng.integers(1, 5)))],
             "met": i, "ts": 1_600_000_000 + i} for i in range(9000)]
    rt = RealtimeSegment("rt_sel", schema, capacity=20000, inverted=["tags"])
    monkeypatch.setenv("PGX_SELECT_MV_NATIVE", "1")
    q = pql.compile("SELECT tags FROM rt WHERE tags IN (2, 11) ORDER BY dim DESC, met LIMIT 30")
    for stop in (2500, 9000):
        for r in rows[rt.num_docs_indexed:stop]:
            rt.index(r)
        op = E.InstancePlanMakerImplV2(ctx).make_inner_segment_plan(rt.device_segment(ctx), q).run()
        blk = op.next_block()
        seen = [r for r in rows[:stop] if set(r["tags"]) & {2, 11}]
        exp = sorted(seen, key=lambda r: (-r["dim"], r["met"]))[:30]
        assert blk.get_selection_data_schema() == (["dim", "met", "tags"], ["INT", "INT", "INT_ARRAY"])
        assert blk.get_selection_result() == [[r["dim"], r["met"], r["tags"]] for r in exp]
        assert [d for _, d in blk.selection_row_ids] == [r["met"] for r in exp]  # met is the docId
        assert op.get_execution_statistics().as_list()[0] == len(seen)
        assert op.get_execution_statistics().as_list()[2:] == [3 * len(seen), stop]
