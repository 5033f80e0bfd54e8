"""Selection queries without ORDER BY end to end on the GPU path: pql.compile -> plan maker (PGX_SELECT_ONLY_NATIVE=1) or
the ABI (PGX_Q_SELECT_ONLY) -> pgx_select_compile / pgx_execute -> pgx_select_first and the gathers, against the model
of tests/select_only_ref.py (first docs per segment, the merge without ordering, the oracle's filter iterators pulled
offset + size times for the statistics) and the reference's known answers
(SelectionSingleValueQueriesTest.testSelectionOnly / testSelectionStar).  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from oracle import pinot_oracle as O
from pinot_amd import pql
from tests import helpers as H
from tests import select_only_ref as F
from tests import select_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = "SELECT column1, column5, column11 FROM testTable%s"


@pytest.fixture(scope="module")
def ctx():
    from pinot_amd import engine as E
    c = E.Context(0)
    yield c
    c.close()


@pytest.fixture()
def native(monkeypatch):
    """The plan maker's route to the library's selection without ORDER BY."""
    monkeypatch.setenv("PGX_SELECT_ONLY_NATIVE", "1")


@pytest.fixture(scope="module", params=["as_loaded", "bitmaps_loaded"])
def sv(ctx, request):
    """The golden segment as the Java test loads it (no bitmap inverted indexes) and with its bitmaps staged."""
    from pinot_amd import engine as E
    exp = H.load_expected()
    inv = exp["loaded_inverted"] if request.param == "as_loaded" else exp["inverted"]
    seg, oseg = H.build_pair("testTable_126164076_167572854_", H.sv_raw(), inverted=inv)
    return E.IndexSegment(ctx, seg), oseg, exp


def _typed(v):
    if isinstance(v, (bytes, np.bytes_)):
        return v.decode()
    if isinstance(v, (str, np.str_)):
        return str(v)
    return int(v) if isinstance(v, (int, np.integer)) else float(v)


def _model(raws, osegs, q):
    """(schema, per-segment row lists, merged rows, statistics) of a selection without ORDER BY: per segment its first
    `size` matching docs, the lists appended in order up to `size`; rows as (typed values in schema order, (segment,
    docId)).  The statistics come from the oracle's filter iterators pulled offset + size times per segment."""
    sel = q["selections"]
    schema = sorted(raws[0]) if sel["columns"] == ["*"] else sorted(sel["columns"])
    per_seg, stats = [], [0, 0, 0, 0]
    for s, (raw, oseg) in enumerate(zip(raws, osegs)):
        n = oseg.total_raw_docs
        docs = F.first_docs(O.filter_mask_vectorized(oseg, q["filter"]), sel["size"])
        per_seg.append([([_typed(raw[c][d]) for c in schema], (s, int(d))) for d in docs])
        pulled, entries = F.pulled(oseg, q["filter"], sel["offset"] + sel["size"])
        assert pulled[:sel["size"]] == docs.tolist()
        stats = [stats[0] + len(docs), stats[1] + entries, stats[2] + len(docs) * len(schema), stats[3] + n]
    return schema, per_seg, F.merge_unordered(per_seg, sel["size"]), stats


def _inner(ctx, gseg, q):
    from pinot_amd import engine as E
    op = E.InstancePlanMakerImplV2(ctx).make_inner_segment_plan(gseg, q).run()
    blk = op.next_block()
    assert op.next_block() is None
    return blk, op.get_execution_statistics().as_list()


def _abi(ctx, gsegs, text, flags):
    """The request at the ABI with `flags`: decode_selection's (stats, names, types, lists)."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    q = E._SelectQuery(ctx, pql.compile(text), flags=flags)
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


# ---------------------------------------------------------------------------------------------------------------------
# the golden segment
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_selection_only(ctx, sv, native):
    """SelectionSingleValueQueriesTest.testSelectionOnly without a filter."""
    from pinot_amd import engine as E
    gseg, oseg, exp = sv
    blk, stats = _inner(ctx, gseg, pql.compile(GOLDEN % ""))
    assert isinstance(E.InstancePlanMakerImplV2(ctx).make_inner_segment_plan(gseg, pql.compile(GOLDEN % "")).run(),
                      E.MSelectionOnlyOperator)
    assert stats == [10, 0, 30, 30000]
    assert blk.get_selection_data_schema() == (["column1", "column11", "column5"], ["INT", "STRING", "STRING"])
    rows = blk.get_selection_result()
    raw = H.sv_raw()
    assert len(rows) == 10 and tuple(rows[0][:2]) == (1578964907, "P")
    assert rows == [[int(raw["column1"][d]), raw["column11"][d].decode(), raw["column5"][d].decode()] for d in range(10)]
    assert blk.selection_row_ids == [(0, d) for d in range(10)]


def test_golden_selection_star(ctx, sv, native):
    """SelectionSingleValueQueriesTest.testSelectionStar without a filter."""
    gseg, oseg, exp = sv
    blk, stats = _inner(ctx, gseg, pql.compile("SELECT * FROM testTable"))
    raw = H.sv_raw()
    names, types = blk.get_selection_data_schema()
    assert names == sorted(raw) and len(names) == 11
    assert stats == [10, 0, 110, 30000]
    assert blk.get_selection_result() == [[_typed(raw[c][d]) for c in names] for d in range(10)]


def test_golden_filter_is_refused(ctx, sv, native):
    """Its filter statistic (48241 in the reference) depends on the state of lazily iterated scan leaves at the stop."""
    from pinot_amd import native as N
    gseg, oseg, exp = sv
    q = pql.compile(GOLDEN % exp["filter"]["text"])
    assert F.classify(q["filter"], oseg) is None
    status, msg = _refusal(lambda: _inner(ctx, gseg, q))
    assert status == N.PGX_ERR_UNSUPPORTED and "numEntriesScannedInFilter" in msg


# ---------------------------------------------------------------------------------------------------------------------
# several segments, each with its own dictionaries (k carries bitmaps)
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
        seg, oseg = H.build_pair("only%d" % i, raw, inverted=("k",), types=types)
        raws.append(raw)
        gsegs.append(E.IndexSegment(ctx, seg))
        osegs.append(oseg)
    return raws, gsegs, osegs


THREE = [
    ("SELECT m FROM t LIMIT 7", "a"),                                        # no filter
    ("SELECT x, m FROM t WHERE k IN (0, 3, 33) LIMIT 40", "a"),              # a bitmap leaf
    ("SELECT m FROM t WHERE m > 900 LIMIT 25", "b"),                         # one scan leaf
    ("SELECT k FROM t WHERE m > -700 LIMIT 5, 20", "b"),                     # an offset: 20 rows, 25 docs pulled
    ("SELECT k, d FROM t WHERE m > -700 AND k IN (0, 3, 33, 60) LIMIT 30", "d"),
    ("SELECT k FROM t WHERE m < 1500 LIMIT 30", "b"),                        # segment 1 has no match
    ("SELECT * FROM t WHERE m < 1500 AND k <> 3 LIMIT 3, 9", "d"),
    ("SELECT * FROM t WHERE m > 100000", "b"),                               # no match anywhere
    ("SELECT * FROM t WHERE k > 0 LIMIT 25", "b"),                           # a range on the bitmap column scans
    ("SELECT l FROM t WHERE m = 123456", "b"),                               # a value outside every dictionary
    ("SELECT l FROM t WHERE k = 1", "a"),                                    # ... on the bitmap column
    ("SELECT l FROM t WHERE m = 123456 AND k = 3", "d"),                     # an always-false scan behind a bitmap
]


@pytest.mark.parametrize("text,cls", THREE)
def test_three_segments_against_the_model(ctx, three, native, text, cls):
    from pinot_amd import engine as E
    raws, gsegs, osegs = three
    q = pql.compile(text)
    assert [F.classify(q["filter"], o) for o in osegs] == [cls] * 3
    schema, per_seg, merged, stats = _model(raws, osegs, q)
    pm = E.InstancePlanMakerImplV2(ctx)
    blk = pm.make_inter_segment_plan(gsegs, q).execute()
    assert blk.get_selection_data_schema()[0] == schema
    assert blk.selection_row_ids == [r[1] for r in merged]
    assert blk.get_selection_result() == [r[0] for r in merged]
    assert blk.stats.as_list() == stats
    for s, gseg in enumerate(gsegs):  # the inner-segment plan returns one segment's rows and statistics
        b, st = _inner(ctx, gseg, q)
        assert b.get_selection_result() == [r[0] for r in per_seg[s]]
        assert [d for _, d in b.selection_row_ids] == [r[1][1] for r in per_seg[s]]
        assert st == _model([raws[s]], [osegs[s]], q)[3]


def test_one_segment_stops_early_and_another_reaches_its_end(ctx, three, native):
    """The same one-leaf scan filter: segments 0 and 2 hold 30 matches and stop at the 30th, segment 1 has none and is
    scanned to its end."""
    from pinot_amd import engine as E
    raws, gsegs, osegs = three
    q = pql.compile("SELECT m FROM t WHERE m < 1500 LIMIT 30")
    blk = E.InstancePlanMakerImplV2(ctx).make_inter_segment_plan(gsegs, q).execute()
    last = [int(np.flatnonzero(r["m"] < 1500)[29]) if s != 1 else None for s, r in enumerate(raws)]
    assert blk.stats.as_list() == [60, last[0] + 1 + len(raws[1]["m"]) + last[2] + 1, 60, sum(len(r["m"]) for r in raws)]
    assert blk.selection_row_ids == [(0, int(d)) for d in np.flatnonzero(raws[0]["m"] < 1500)[:30]]


def test_segments_of_different_classes_are_refused(ctx, native):
    """k carries a bitmap in one segment only: `k = 3` is class a there and class b in the other."""
    from pinot_amd import engine as E
    from pinot_amd import native as N
    rng = np.random.default_rng(4)
    raw = {"k": rng.integers(0, 9, size=500).astype(np.int32), "m": rng.integers(0, 99, size=500).astype(np.int32)}
    gsegs = [E.IndexSegment(ctx, H.build_pair("mix%d" % i, raw, inverted=inv)[0]) for i, inv in enumerate([("k",), ()])]
    q = pql.compile("SELECT m FROM t WHERE k = 3")
    status, msg = _refusal(lambda: E.InstancePlanMakerImplV2(ctx).make_inter_segment_plan(gsegs, q).execute())
    assert status == N.PGX_ERR_UNSUPPORTED and "numEntriesScannedInFilter" in msg
    for g in gsegs:
        blk, _ = _inner(ctx, g, q)  # each on its own runs
        assert [d for _, d in blk.selection_row_ids] == np.flatnonzero(raw["k"] == 3)[:10].tolist()
        g.destroy()


@pytest.mark.parametrize("text", [
    "SELECT m FROM t WHERE m > 0 AND d < 1",            # an AND of scans
    "SELECT m FROM t WHERE m > 0 OR k = 3",             # an OR with a scan leaf
    "SELECT m FROM t WHERE k = 3 AND (m > 0 OR d < 1)",  # a nested operator over a scan leaf
])
def test_filters_without_a_closed_form_are_refused(ctx, three, native, text):
    from pinot_amd import native as N
    raws, gsegs, osegs = three
    q = pql.compile(text)
    assert F.classify(q["filter"], osegs[0]) is None
    status, msg = _refusal(lambda: _inner(ctx, gsegs[0], q))
    assert status == N.PGX_ERR_UNSUPPORTED and "numEntriesScannedInFilter" in msg


# ---------------------------------------------------------------------------------------------------------------------
# limits, multi-value columns, the other entry points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mv_seg(ctx):
    from pinot_amd import engine as E
    from pinot_amd import segment as S
    rng = np.random.default_rng(3)
    n = 9000
    raw = {"a": rng.integers(0, 50, size=n).astype(np.int32),
           "v": [rng.integers(0, 9, size=1 + i % 3).astype(np.int32) for i in range(n)]}
    cols = [S.make_column("a", raw["a"]), S.make_mv_column("v", raw["v"])]
    return raw, E.IndexSegment(ctx, S.make_segment("mvonly", cols))


def test_limits(ctx, mv_seg, native):
    from pinot_amd import native as N
    raw, gseg = mv_seg
    for text, rows in (("SELECT a FROM t LIMIT 2048", 2048), ("SELECT a FROM t WHERE a > 4 LIMIT 2000, 48", 48)):
        blk, stats = _inner(ctx, gseg, pql.compile(text))
        keep = np.flatnonzero(raw["a"] > 4) if "WHERE" in text else np.arange(len(raw["a"]))
        assert [d for _, d in blk.selection_row_ids] == keep[:rows].tolist()
        assert blk.get_selection_result() == [[int(raw["a"][d])] for d in keep[:rows]]
        assert stats == [rows, int(keep[2047]) + 1 if "WHERE" in text else 0, rows, len(raw["a"])]
    for text in ("SELECT a FROM t LIMIT 2049", "SELECT a FROM t LIMIT 0", "SELECT a FROM t LIMIT 2001, 48",
                 "SELECT a FROM t LIMIT 5, 0"):
        assert _refusal(lambda: _inner(ctx, gseg, pql.compile(text)))[0] == N.PGX_ERR_UNSUPPORTED


@pytest.mark.parametrize("text", ["SELECT a, v FROM t WHERE a > 40 LIMIT 3, 12", "SELECT * FROM t LIMIT 300"])
def test_multi_value_selected_column(ctx, mv_seg, text):
    from pinot_amd import native as N
    raw, gseg = mv_seg
    status, msg = _refusal(lambda: _abi(ctx, [gseg], text, N.PGX_Q_SELECT_ONLY))
    assert status == N.PGX_ERR_UNSUPPORTED and "multi-value column v" in msg
    stats, names, types, lists = _abi(ctx, [gseg], text, N.PGX_Q_SELECT_ONLY | N.PGX_Q_SELECT_MV)
    q = pql.compile(text)["selections"]
    keep = (np.flatnonzero(raw["a"] > 40) if "WHERE" in text else np.arange(len(raw["a"])))
    assert (names, types) == (["a", "v"], ["INT", "INT_ARRAY"])
    assert lists == [[([int(raw["a"][d]), [int(x) for x in raw["v"][d]]], (0, int(d))) for d in keep[:q["size"]]]]
    p = q["offset"] + q["size"]
    assert stats.as_list() == [q["size"], int(keep[p - 1]) + 1 if "WHERE" in text else 0, 2 * q["size"], len(raw["a"])]


def test_execute_async_gives_the_same_rows(ctx, three):
    from pinot_amd import engine as E
    from pinot_amd import native as N
    raws, gsegs, osegs = three
    req = pql.compile("SELECT k FROM t WHERE m > -700 LIMIT 5, 20")
    q = E._SelectQuery(ctx, req, flags=N.PGX_Q_SELECT_ONLY)
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
    assert [len(x) for x in sync[3]] == [20, 20, 20]


def test_other_entry_points_refuse_as_for_order_by(ctx, mv_seg):
    from pinot_amd import engine as E
    from pinot_amd import native as N
    L = N.lib()
    raw, gseg = mv_seg
    q = E._SelectQuery(ctx, pql.compile("SELECT a FROM t WHERE a > 3"), flags=N.PGX_Q_SELECT_ONLY)
    try:
        assert _refusal(lambda: q.execute_multi([gseg]))[0] == N.PGX_ERR_UNSUPPORTED
        assert _refusal(lambda: q.set_key_domain(0, [1, 2], "INT"))[0] == N.PGX_ERR_UNSUPPORTED
        assert _refusal(lambda: q.execute([gseg], flags=N.PGX_X_KEEP_DENSE_ON_DEVICE))[0] == N.PGX_ERR_UNSUPPORTED
        segs = (C.c_void_p * 1)(gseg.handle.value)
        binds, keep = q.bindings([gseg])
        t, k, out = C.c_double(), C.c_double(), C.c_void_p()
        assert L.pgx_execute_timed(ctx.handle, q.handle, segs, 1, binds, 1, C.byref(t), C.byref(k), C.byref(out)) \
            == N.PGX_ERR_UNSUPPORTED
        slots = C.c_int64()
        assert L.pgx_query_dense_slots(q.handle, segs, 1, C.byref(slots)) == N.PGX_ERR_UNSUPPORTED
        r = q.execute([gseg])
        v, c, n32 = C.c_double(), C.c_int64(), C.c_int32()
        assert L.pgx_result_agg(r, 0, C.byref(v), C.byref(c)) == N.PGX_ERR_INVALID_ARG
        assert L.pgx_result_select_schema(r, C.byref(n32), None) == 0 and n32.value == 1
        L.pgx_result_release(r)
    finally:
        q.close()
    # with the flag and an ORDER BY the query is the ORDER BY query as before
    stats, names, types, lists = _abi(ctx, [gseg], "SELECT a FROM t ORDER BY a DESC LIMIT 3", N.PGX_Q_SELECT_ONLY)
    assert [r[0] for r in lists[0]] == [[49], [49], [49]] and stats.as_list()[0] == len(raw["a"])


def test_server_datatable_broker_reduce(ctx, three, native):
    from pinot_amd import broker as B
    from pinot_amd import datatable as D
    raws, gsegs, osegs = three
    q = pql.compile("SELECT x, m FROM t WHERE m > 900 LIMIT 2, 12")
    servers = {"server0": ([0, 1], gsegs[:2]), "server1": ([2], gsegs[2:])}
    wires, rows, stats = {}, [], [0, 0, 0, 0]
    for name, (idx, segs) in servers.items():
        resp = B.ServerQueryExecutor(ctx).process_query(q, segs)
        assert not resp.exceptions
        wires[name] = D.response_to_datatable(q, resp)
        assert D.response_to_datatable(q, D.datatable_to_response(q, wires[name])) == wires[name]
        _, _, merged, st = _model([raws[i] for i in idx], [osegs[i] for i in idx], q)
        rows.append(merged)
        stats = [a + b for a, b in zip(stats, st)]
    out = B.BrokerReduceService().reduce_on_data_table(q, wires)
    assert out.processing_exceptions == []
    assert [out.num_docs_scanned, out.num_entries_scanned_in_filter, out.num_entries_scanned_post_filter,
            out.total_docs] == stats
    assert out.selection_results.columns == ["x", "m"]
    exp = F.merge_unordered(rows, 12)  # no offset cut: 12 rows from the first
    assert out.selection_results.results == [[r[0][1], str(r[0][0])] for r in exp] and len(exp) == 12


def test_without_the_flag_the_refusal_is_unchanged(ctx, mv_seg, monkeypatch):
    from pinot_amd import native as N
    monkeypatch.delenv("PGX_SELECT_ONLY_NATIVE", raising=False)
    raw, gseg = mv_seg
    for fn in (lambda: _inner(ctx, gseg, pql.compile("SELECT a FROM t")),
               lambda: _abi(ctx, [gseg], "SELECT a FROM t", 0),
               lambda: _abi(ctx, [gseg], "SELECT a FROM t", N.PGX_Q_SELECT_MV)):
        status, msg = _refusal(fn)
        assert status == N.PGX_ERR_UNSUPPORTED
        assert msg == "pgx error 2: selection without ORDER BY (MSelectionOnlyOperator)"
