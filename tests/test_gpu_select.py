"""Selection queries with ORDER BY end to end on the GPU path: pql.compile -> plan maker -> pgx_select_compile /
pgx_execute -> the selection kernels, against the numpy model of tests/select_ref.py, the reference's known answers
(SelectionSingleValueQueriesTest.testSelectionOrderBy) and a value model over several segments."""
import ctypes as C

import numpy as np
import pytest

from oracle import pinot_oracle as O
from pinot_amd import pql
from tests import helpers as H
from tests import select_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = "SELECT column1, column5, column11 FROM testTable%s ORDER BY column6, column1"


@pytest.fixture(scope="module")
def ctx():
    from pinot_amd import engine as E
    c = E.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=["as_loaded", "bitmaps_loaded"])
def sv(ctx, request):
    """The golden segment as the Java test loads it (no bitmap inverted indexes) and with its bitmaps staged."""
    from pinot_amd import engine as E
    exp = H.load_expected()
    inv = exp["loaded_inverted"] if request.param == "as_loaded" else exp["inverted"]
    seg, oseg = H.build_pair("testTable_126164076_167572854_", H.sv_raw(), inverted=inv)
    return E.IndexSegment(ctx, seg), oseg, exp, request.param


def _typed(v):
    if isinstance(v, (bytes, np.bytes_)):
        return v.decode()
    if isinstance(v, (str, np.str_)):
        return str(v)
    return int(v) if isinstance(v, (int, np.integer)) else float(v)


def _value_model(raws, osegs, q):
    """Rows of a selection over several segments by VALUE: the order columns' ranks in the union of the segments'
    values (descending: reversed), then (segment, docId).  Returns (schema, per-segment row lists, merged rows), rows as
    (typed values in schema order, (segment, docId)), each list cut to offset + size."""
    sel = q["selections"]
    order = sel["order_by"]
    cols = sorted(raws[0]) if sel["columns"] == ["*"] else sorted(sel["columns"])
    schema = [o["column"] for o in order] + [c for c in cols if c not in [o["column"] for o in order]]
    masks = [O.filter_mask_vectorized(os_, q["filter"]) if q["filter"] else np.ones(len(next(iter(r.values()))), bool)
             for r, os_ in zip(raws, osegs)]
    seg = np.concatenate([np.full(int(m.sum()), s) for s, m in enumerate(masks)])
    doc = np.concatenate([np.flatnonzero(m) for m in masks])
    keys = []
    for o in order:
        vals = np.concatenate([r[o["column"]][m] for r, m in zip(raws, masks)])
        uniq, rank = np.unique(np.concatenate([r[o["column"]] for r in raws] + [vals]), return_inverse=True)
        rank = rank[-len(vals):] if len(vals) else rank[:0]
        keys.append(rank if o["asc"] else len(uniq) - 1 - rank)
    idx = np.lexsort([doc, seg] + keys[::-1])
    k = sel["offset"] + sel["size"]
    rows = [([_typed(raws[seg[i]][c][doc[i]]) for c in schema], (int(seg[i]), int(doc[i]))) for i in idx]
    per_seg = [[r for r in rows if r[1][0] == s][:k] for s in range(len(raws))]
    return schema, per_seg, rows[:k]


def _inner(ctx, gseg, q):
    from pinot_amd import engine as E
    op = E.InstancePlanMakerImplV2(ctx).make_inner_segment_plan(gseg, q).run()
    blk = op.next_block()
    assert op.next_block() is None
    return blk, op.get_execution_statistics().as_list()


# ---------------------------------------------------------------------------------------------------------------------
# the golden segment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filtered", [False, True])
def test_golden_selection_order_by(ctx, sv, filtered):
    gseg, oseg, exp, loaded = sv
    flt = exp["filter"]["text"] if filtered else ""
    q = pql.compile(GOLDEN % flt)
    blk, stats = _inner(ctx, gseg, q)
    raw = H.sv_raw()
    # the kernels' model over dictIds
    mask = O.filter_mask_vectorized(oseg, q["filter"]) if filtered else np.ones(30000, bool)
    cols = []
    for c in ("column6", "column1"):
        d, ids = np.unique(raw[c], return_inverse=True)
        cols.append((ids, len(d), True))
    docs = R.top_k(mask, cols, 10)
    assert [r[1] for r in blk.selection_row_ids] == docs.tolist()
    rows = blk.get_selection_result()
    assert len(rows) == 10
    assert rows == [[int(raw["column6"][d]), int(raw["column1"][d]), raw["column11"][d].decode(),
                     raw["column5"][d].decode()] for d in docs]
    # SelectionSingleValueQueriesTest.testSelectionOrderBy: the last (tenth-best) row
    assert tuple(rows[-1][:2]) == ((6043515, 462769197) if filtered else (6043515, 10542595))
    assert blk.get_selection_data_schema() == (["column6", "column1", "column11", "column5"],
                                               ["INT", "INT", "STRING", "STRING"])
    if not filtered:
        assert stats == [30000, 0, 120000, 30000]
    else:
        cblk, cstats = _inner(ctx, gseg, pql.compile("SELECT COUNT(*) FROM testTable" + flt))
        assert cblk.get_aggregation_result() == [6129]
        if loaded == "as_loaded":
            assert cstats[1] == 84134
        assert stats == [6129, cstats[1], 24516, 30000]


def test_golden_server_datatable_broker_reduce(ctx, sv):
    from pinot_amd import broker as B
    from pinot_amd import datatable as D
    gseg, oseg, exp, loaded = sv
    q = pql.compile(GOLDEN % exp["filter"]["text"] + " LIMIT 2, 6")
    resp = B.ServerQueryExecutor(ctx).process_query(q, [gseg])
    assert not resp.exceptions
    wire = D.response_to_datatable(q, resp)
    assert D.response_to_datatable(q, D.datatable_to_response(q, wire)) == wire
    out = B.BrokerReduceService().reduce_on_data_table(q, {"server0": wire})
    assert out.processing_exceptions == []
    assert (out.num_docs_scanned, out.num_entries_scanned_post_filter, out.total_docs) == (6129, 24516, 30000)
    raw = H.sv_raw()
    _, _, merged = _value_model([raw], [oseg], q)
    assert out.selection_results.columns == ["column1", "column5", "column11"]
    assert out.selection_results.results == [[str(r[0][1]), r[0][3], r[0][2]] for r in merged[2:]]
    assert len(out.selection_results.results) == 6


# ---------------------------------------------------------------------------------------------------------------------
# several segments, each with its own dictionaries
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three(ctx):
    from pinot_amd import engine as E
    rng = np.random.default_rng(21)
    raws, gsegs, osegs = [], [], []
    types = {"l": "LONG", "d": "DOUBLE"}
    for i in range(3):
        n = 4000 + 2777 * i
        raw = {"k": rng.integers(0, 40 + 15 * i, size=n).astype(np.int32) * 3 - 30,
               "x": np.array(["v%02d" % v for v in rng.integers(i, 9 + 2 * i, size=n)]),
               "l": rng.integers(-5, 6 + i, size=n).astype(np.int64) * (1 << 40),
               "d": rng.integers(-8, 9 + i, size=n).astype(np.float64) / 4.0,
               "m": rng.integers(-1000, 1000, size=n).astype(np.int32)}
        if i == 1:
            raw["m"] = raw["m"] + 5000  # no doc of segment 1 passes m < 1500
        seg, oseg = H.build_pair("sel%d" % i, raw, types=types)
        raws.append(raw)
        gsegs.append(E.IndexSegment(ctx, seg))
        osegs.append(oseg)
    return raws, gsegs, osegs


@pytest.mark.parametrize("text", [
    "SELECT m FROM t WHERE m > -700 ORDER BY k, x DESC LIMIT 5, 20",       # INT ascending + STRING descending
    "SELECT x, m FROM t ORDER BY l DESC, d, k LIMIT 40",                   # a LONG and a DOUBLE order column
    "SELECT k FROM t WHERE m < 1500 ORDER BY d DESC, x LIMIT 30",          # segment 1 has no match
    "SELECT * FROM t WHERE k > 0 ORDER BY x, l DESC, m LIMIT 25",
    "SELECT * FROM t WHERE m > 100000 ORDER BY k",                         # no match anywhere
])
def test_three_segments_against_the_value_model(ctx, three, text):
    from pinot_amd import engine as E
    raws, gsegs, osegs = three
    q = pql.compile(text)
    schema, per_seg, merged = _value_model(raws, osegs, q)
    pm = E.InstancePlanMakerImplV2(ctx)
    blk = pm.make_inter_segment_plan(gsegs, q).execute()
    assert blk.get_selection_data_schema()[0] == schema
    assert blk.selection_row_ids == [r[1] for r in merged]
    assert blk.get_selection_result() == [r[0] for r in merged]
    matched = sum(int(O.filter_mask_vectorized(o, q["filter"]).sum()) if q["filter"] else len(r["k"])
                  for r, o in zip(raws, osegs))
    cstats = pm.make_inter_segment_plan(gsegs, dict(pql.compile("SELECT COUNT(*) FROM t"), filter=q["filter"])) \
        .execute().stats.as_list()
    assert blk.stats.as_list() == [matched, cstats[1], matched * len(schema), sum(len(r["k"]) for r in raws)]
    for s, gseg in enumerate(gsegs):  # the inner-segment plan returns one segment's rows
        b, _ = _inner(ctx, gseg, q)
        assert b.get_selection_result() == [r[0] for r in per_seg[s]]
        assert [d for _, d in b.selection_row_ids] == [r[1][1] for r in per_seg[s]]


FILTERS = ["", " WHERE a > 0", " WHERE b IN (%(b0)s, %(b1)s)", " WHERE s = %(s0)s", " WHERE (a > 0 OR b = %(b1)s) AND s <> %(s0)s",
           " WHERE a = 12345"]
ORDERS = [" ORDER BY g2 DESC, a", " ORDER BY s, b DESC, c LIMIT 3, 50", " ORDER BY c LIMIT 1"]


@pytest.fixture(scope="module")
def rand_seg(ctx):
    from pinot_amd import engine as E
    rng = np.random.default_rng(7)
    n = 8192 * 3 + 1000
    raw = {"a": rng.integers(-3000, 3000, size=n).astype(np.int32), "b": rng.integers(0, 40, size=n).astype(np.int32) * 11,
           "c": rng.integers(0, 700, size=n).astype(np.int32), "s": np.sort(rng.integers(0, 6, size=n)).astype(np.int32),
           "g2": rng.integers(0, 900, size=n).astype(np.int32)}
    seg, oseg = H.build_pair("r", raw, inverted=("b", "c"))
    fmt = {"b0": 0, "b1": 55, "s0": 4}
    return raw, E.IndexSegment(ctx, seg), oseg, fmt


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("flt", FILTERS)
def test_random_filters_and_orders(ctx, rand_seg, flt, order):
    """Scan, sorted-range and bitmap leaves under the selection (s is a sorted column, b and c carry bitmaps)."""
    raw, gseg, oseg, fmt = rand_seg
    q = pql.compile("SELECT a, s FROM t" + (flt % fmt) + order)
    _, _, merged = _value_model([raw], [oseg], q)
    blk, stats = _inner(ctx, gseg, q)
    assert blk.selection_row_ids == [r[1] for r in merged]
    assert blk.get_selection_result() == [r[0] for r in merged]
    _, cstats = _inner(ctx, gseg, dict(pql.compile("SELECT COUNT(*) FROM t"), filter=q["filter"]))
    assert stats == [cstats[0], cstats[1], cstats[0] * len(blk.get_selection_data_schema()[0]), len(raw["a"])]


def test_execute_async_gives_the_same_rows(ctx, three):
    from pinot_amd import engine as E
    from pinot_amd import native as N
    raws, gsegs, osegs = three
    req = pql.compile("SELECT m FROM t WHERE m > -700 ORDER BY k, x DESC LIMIT 5, 20")
    q = E._SelectQuery(ctx, req)
    try:
        r = q.execute(gsegs)
        sync = E.decode_selection(q, r, gsegs)
        N.lib().pgx_result_release(r)
        r = q.execute_async(gsegs)
        assert N.lib().pgx_result_wait(r, -1) == 0
        assert E.decode_selection(q, r, gsegs) == sync
        N.lib().pgx_result_release(r)
    finally:
        q.close()
    assert sum(len(x) for x in sync[3]) > 0


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mv_seg(ctx):
    from pinot_amd import engine as E
    from pinot_amd import segment as S
    rng = np.random.default_rng(3)
    n = 9000
    cols = [S.make_column("a", rng.integers(0, 50, size=n).astype(np.int32)),
            S.make_mv_column("v", [rng.integers(0, 9, size=1 + i % 3) for i in range(n)])]
    cols += [S.make_column("w%d" % i, rng.permutation(n).astype(np.int32)) for i in range(5)]  # 14 key bits each
    return E.IndexSegment(ctx, S.make_segment("mv", cols))


def _status(fn):
    from pinot_amd import native as N
    with pytest.raises(N.PgxError) as e:
        fn()
    return e.value.status


@pytest.mark.parametrize("text", [
    "SELECT a FROM t",                                       # no ORDER BY (MSelectionOnlyOperator)
    "SELECT a FROM t LIMIT 5",
    "SELECT a FROM t ORDER BY v",                            # a multi-value order column
    "SELECT a, v FROM t ORDER BY a",                         # a multi-value selected column
    "SELECT * FROM t ORDER BY a",                            # ... through *
    "SELECT a FROM t ORDER BY a LIMIT 0",
    "SELECT a FROM t ORDER BY a LIMIT 2049",                 # above PGX_SEL_MAX_ROWS
    "SELECT a FROM t ORDER BY a LIMIT 2000, 49",
    "SELECT a FROM t ORDER BY w0, w1, w2, w3, w4",           # a 70-bit key
    "SELECT a FROM t ORDER BY a, a, a, a, a, a, a, a, a",    # nine order columns
])
def test_unsupported_shapes_are_refused(ctx, mv_seg, text):
    from pinot_amd import engine as E
    from pinot_amd import native as N
    q = pql.compile(text)
    assert _status(lambda: _inner(ctx, mv_seg, q)) == N.PGX_ERR_UNSUPPORTED
    assert _status(lambda: E.InstancePlanMakerImplV2(ctx).make_inter_segment_plan([mv_seg], q).execute()) \
        == N.PGX_ERR_UNSUPPORTED


def test_limit_at_max_rows_and_a_64_bit_key_run(ctx, mv_seg):
    blk, _ = _inner(ctx, mv_seg, pql.compile("SELECT a FROM t ORDER BY w0, w1, w2, w3, a LIMIT 48, 2000"))  # 62 bits
    assert len(blk.get_selection_result()) == R.MAX_ROWS
    w0 = [r[0] for r in blk.get_selection_result()]
    assert w0 == list(range(R.MAX_ROWS))  # w0 is a permutation of 0..n-1


def test_other_entry_points_refuse_a_selection_query(ctx, mv_seg):
    from pinot_amd import engine as E
    from pinot_amd import native as N
    L = N.lib()
    q = E._SelectQuery(ctx, pql.compile("SELECT a FROM t WHERE a > 3 ORDER BY a"))
    aq = E._Query(ctx, pql.compile("SELECT COUNT(*) FROM t"))
    try:
        assert _status(lambda: q.execute_multi([mv_seg])) == N.PGX_ERR_UNSUPPORTED
        assert _status(lambda: q.set_key_domain(0, [1, 2], "INT")) == N.PGX_ERR_UNSUPPORTED
        assert _status(lambda: q.execute([mv_seg], flags=N.PGX_X_KEEP_DENSE_ON_DEVICE)) == N.PGX_ERR_UNSUPPORTED
        segs = (C.c_void_p * 1)(mv_seg.handle.value)
        binds, keep = q.bindings([mv_seg])
        t, k, out = C.c_double(), C.c_double(), C.c_void_p()
        assert L.pgx_execute_timed(ctx.handle, q.handle, segs, 1, binds, 1, C.byref(t), C.byref(k), C.byref(out)) \
            == N.PGX_ERR_UNSUPPORTED
        slots = C.c_int64()
        assert L.pgx_query_dense_slots(q.handle, segs, 1, C.byref(slots)) == N.PGX_ERR_UNSUPPORTED
        # the accessors keep to their own kind of result
        r = q.execute([mv_seg])
        v, c, n64, n32 = C.c_double(), C.c_int64(), C.c_int64(), C.c_int32()
        assert L.pgx_result_agg(r, 0, C.byref(v), C.byref(c)) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_num_groups(r, C.byref(n64)) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_group_keys(r, 0, None, None) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_select_schema(r, C.byref(n32), None) == 0 and n32.value == 1
        L.pgx_result_release(r)
        r = aq.execute([mv_seg])
        assert L.pgx_result_select_schema(r, C.byref(n32), None) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_select_counts(r, C.byref(n32)) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_select_rows(r, None, None, None) == N.PGX_ERR_INVALID_ARG
        L.pgx_result_release(r)
    finally:
        q.close()
        aq.close()
    # a column the segment does not have
    assert _status(lambda: _inner(ctx, mv_seg, pql.compile("SELECT a FROM t ORDER BY nope"))) == N.PGX_ERR_INVALID_ARG
    assert _status(lambda: _inner(ctx, mv_seg, pql.compile("SELECT nope FROM t ORDER BY a"))) == N.PGX_ERR_INVALID_ARG
