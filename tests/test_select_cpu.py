"""Selection ORDER BY, the parts that need no GPU: the PQL forms, the numpy model of tests/select_ref.py against the
reference's known answers (SelectionSingleValueQueriesTest.testSelectionOrderBy), the engine's value merge, the broker
reduce and render, and the DataTable round trip."""
import numpy as np
import pytest

from oracle import pinot_oracle as O
from pinot_amd import broker as B
from pinot_amd import datatable as D
from pinot_amd import engine as E
from pinot_amd import pql
from tests import helpers as H
from tests import select_ref as R


# ---------------------------------------------------------------------------------------------------------------------
# pql
# ---------------------------------------------------------------------------------------------------------------------
def test_pql_selection_forms():
    q = pql.compile("SELECT column1, column5, column11 FROM testTable ORDER BY column6, column1")
    assert q["aggregations"] == [] and q["group_by"] is None and q["filter"] is None and q["table"] == "testTable"
    assert q["selections"] == {"columns": ["column1", "column5", "column11"],
                               "order_by": [{"column": "column6", "asc": True}, {"column": "column1", "asc": True}],
                               "offset": 0, "size": 10}
    q = pql.compile("select * from t order by a desc, b ASC, c limit 5, 20")
    assert q["selections"] == {"columns": ["*"], "order_by": [{"column": "a", "asc": False}, {"column": "b", "asc": True},
                                                              {"column": "c", "asc": True}], "offset": 5, "size": 20}
    # clauses in any order
    q = pql.compile("SELECT a FROM t LIMIT 3 ORDER BY a WHERE b > 5")
    assert q["selections"]["size"] == 3 and q["selections"]["offset"] == 0
    assert q["selections"]["order_by"] == [{"column": "a", "asc": True}]
    assert q["filter"] == {"op": "RANGE", "column": "b", "values": ["(5\t\t*)"]}
    # no ORDER BY parses (the engine refuses it), LIMIT 0 too
    q = pql.compile("SELECT a, b FROM t LIMIT 0")
    assert q["selections"] == {"columns": ["a", "b"], "order_by": [], "offset": 0, "size": 0}


@pytest.mark.parametrize("text", [
    "SELECT a FROM t ORDER BY a ORDER BY b",
    "SELECT a FROM t LIMIT 1 LIMIT 2",
    "SELECT a FROM t WHERE a = 1 WHERE b = 2",
    "SELECT a FROM t ORDER a",
    "SELECT a FROM t ORDER BY",
    "SELECT a FROM t LIMIT",
    "SELECT a FROM t LIMIT 1.5",
    "SELECT a FROM t LIMIT x",
    "SELECT a FROM t LIMIT 1,",
    "SELECT a, FROM t",
    "SELECT a, COUNT(*) FROM t",
    "SELECT a FROM t GROUP BY a",
    "SELECT a FROM t TOP 5",
    "SELECT COUNT(*) FROM t ORDER BY a",
    "SELECT COUNT(*) FROM t LIMIT 5",
])
def test_pql_selection_errors(text):
    with pytest.raises(pql.PqlError):
        pql.compile(text)


def test_pql_aggregation_requests_unchanged():
    assert pql.compile("SELECT COUNT(*), SUM(m) FROM t WHERE d BETWEEN 64 AND 191") == {
        "table": "t", "aggregations": [{"fn": "count", "column": "*"}, {"fn": "sum", "column": "m"}], "group_by": None,
        "filter": {"op": "RANGE", "column": "d", "values": ["[64\t\t191]"]}}
    assert pql.compile("SELECT SUM(m) FROM t WHERE d < 128 GROUP BY g, h TOP 7") == {
        "table": "t", "aggregations": [{"fn": "sum", "column": "m"}], "group_by": {"columns": ["g", "h"], "top_n": 7},
        "filter": {"op": "RANGE", "column": "d", "values": ["(*\t\t128)"]}}


# ---------------------------------------------------------------------------------------------------------------------
# the model against the reference's constants
# ---------------------------------------------------------------------------------------------------------------------
def _dict_ids(values):
    d, ids = np.unique(values, return_inverse=True)
    return ids, len(d)


@pytest.mark.parametrize("filtered, last", [(False, (6043515, 10542595)), (True, (6043515, 462769197))])
def test_model_reproduces_the_java_constants(filtered, last):
    """SelectionSingleValueQueriesTest.testSelectionOrderBy: ORDER BY column6, column1, the tenth row's two keys."""
    raw = H.sv_raw()
    exp = H.load_expected()
    n = len(raw["column6"])
    sel = np.ones(n, bool)
    if filtered:
        q = pql.compile("SELECT COUNT(*) FROM testTable" + exp["filter"]["text"])
        sel = O.filter_mask_vectorized(O.OSegment.from_raw(raw), q["filter"])
        assert sel.dtype == bool and sel.sum() == 6129
    (i6, c6), (i1, c1) = _dict_ids(raw["column6"]), _dict_ids(raw["column1"])
    docs = R.top_k(sel, [(i6, c6, True), (i1, c1, True)], 10)
    assert len(docs) == 10
    assert (int(raw["column6"][docs[-1]]), int(raw["column1"][docs[-1]])) == last
    # the ten are unambiguous: every selected doc carrying the boundary key is among them
    same = sel & (raw["column6"] == last[0]) & (raw["column1"] == last[1])
    assert set(np.flatnonzero(same)) <= set(docs.tolist())
    # descending, through card - 1 - id: the mirror image
    worst = R.top_k(sel, [(i6, c6, False), (i1, c1, False)], 1)
    key = np.lexsort((raw["column1"][sel], raw["column6"][sel]))
    assert (raw["column6"][worst[0]], raw["column1"][worst[0]]) == \
        (raw["column6"][sel][key[-1]], raw["column1"][sel][key[-1]])


def test_model_key_layout_and_ties():
    assert [R.key_bits(c) for c in (1, 2, 3, 4, 5, 1000, 1024, 1025)] == [1, 1, 2, 2, 3, 10, 10, 11]
    ids_a, ids_b = np.array([1, 0, 1, 0, 1]), np.array([2, 4, 2, 0, 1])
    key, bits = R.order_keys([(ids_a, 2, True), (ids_b, 5, False)])
    assert bits == 4 and key.tolist() == [(1 << 3) | 2, 0, (1 << 3) | 2, 4, (1 << 3) | 3]
    assert R.top_k(np.ones(5, bool), [(ids_a, 2, True), (ids_b, 5, False)], 4).tolist() == [1, 3, 0, 2]
    assert R.top_k(np.array([1, 0, 1, 0, 1], bool), [(ids_a, 2, True)], 2).tolist() == [0, 2]
    # the packed forms the kernels read
    assert R.pack_mask([True, False, True], ones_past_end=False).tolist() == [5, 0]
    assert R.pack_mask([True, False, True]).tolist() == [0xFFFFFFFD, 0xFFFFFFFF]
    assert R.pack_fwd([5, 2], 3)[:1].tolist() == [0b10101000]
    assert len(R.pack_fwd([1], 7)) == 8192 * 7 // 8 + 64


# ---------------------------------------------------------------------------------------------------------------------
# the engine's value merge
# ---------------------------------------------------------------------------------------------------------------------
def test_merge_selection_rows_values_directions_and_ties():
    types = ["INT", "STRING", "DOUBLE"]
    order = [{"column": "a", "asc": True}, {"column": "s", "asc": False}]
    seg0 = [([-5, "b", 1.0], (0, 7)), ([3, "zz", 2.0], (0, 1)), ([3, "a", 3.0], (0, 2))]
    seg1 = [([-7, "q", 4.0], (1, 0)), ([3, "zz", 5.0], (1, 9)), ([3, "zz", 6.0], (1, 3))]
    seg2 = []
    rows = E.merge_selection_rows([seg0, seg1, seg2], types, order, 100)
    assert [r[1] for r in rows] == [(1, 0), (0, 7), (0, 1), (1, 3), (1, 9), (0, 2)]
    assert [r[1] for r in E.merge_selection_rows([seg0, seg1, seg2], types, order, 4)] == [(1, 0), (0, 7), (0, 1), (1, 3)]
    # offset is the caller's: the merge keeps offset + size rows
    assert E.merge_selection_rows([seg0, seg1], types, order, 0) == []


def test_merge_selection_rows_java_comparisons():
    # Double.compareTo: -0.0 below 0.0, NaN above +inf; negative numbers; String.compareTo by UTF-16 code unit
    vals = [0.0, -0.0, float("nan"), float("inf"), -1.5, float("-inf")]
    rows = [[([v], (0, i))] for i, v in enumerate(vals)]
    got = [r[1][1] for r in E.merge_selection_rows(rows, ["DOUBLE"], [{"column": "d", "asc": True}], 10)]
    assert got == [5, 4, 1, 0, 3, 2]
    got = [r[1][1] for r in E.merge_selection_rows(rows, ["DOUBLE"], [{"column": "d", "asc": False}], 10)]
    assert got == [2, 3, 0, 1, 4, 5]
    strs = ["b", "B", "", "￿", "\U00010000", "ab"]  # a supplementary char's surrogates sort below U+FFFF
    rows = [[([v], (0, i))] for i, v in enumerate(strs)]
    got = [strs[r[1][1]] for r in E.merge_selection_rows(rows, ["STRING"], [{"column": "s", "asc": True}], 10)]
    assert got == ["", "B", "ab", "b", "\U00010000", "￿"]
    longs = [2 ** 62, -2 ** 63, 0]
    rows = [[([v], (i, 0)) for i, v in enumerate(longs)]]
    got = [r[0][0] for r in E.merge_selection_rows(rows, ["LONG"], [{"column": "l", "asc": True}], 2)]
    assert got == [-2 ** 63, 0]


# ---------------------------------------------------------------------------------------------------------------------
# broker reduce / render, DataTable
# ---------------------------------------------------------------------------------------------------------------------
_REQ = {"table": "t", "aggregations": [], "group_by": None, "filter": None,
        "selections": {"columns": ["s", "f", "a"], "order_by": [{"column": "a", "asc": False}], "offset": 1, "size": 3}}
_SCHEMA = (["a", "d", "f", "l", "s"], ["INT", "DOUBLE", "FLOAT", "LONG", "STRING"])


def _resp(rows, stats):
    return B.InstanceResponse(selection=rows, selection_schema=_SCHEMA, stats=stats)


def test_format_selection_value():
    f = B.format_selection_value
    assert f("INT", -12) == "-12" and f("INT", 0) == "0" and f("LONG", 2 ** 62) == str(2 ** 62)
    assert f("FLOAT", 2.0) == "2.0" and f("FLOAT", float(np.float32(0.1))) == "0.1"
    assert f("FLOAT", 0.123456789) == "0.12346" and f("DOUBLE", 0.123456789) == "0.123456789"
    assert f("DOUBLE", 1234567.25) == "1234567.25" and f("DOUBLE", 1e20) == "100000000000000000000.0"
    assert f("DOUBLE", 1e-11) == "0.0" and f("DOUBLE", -2.5) == "-2.5" and f("DOUBLE", 0.00000000125) == "0.0000000012"
    assert f("STRING", "x\ty") == "x\ty"


def test_broker_reduce_and_render_selection():
    r0 = _resp([[9, 0.5, 1.5, 10, "x"], [7, 0.25, 2.0, 11, "y"], [1, 1.0, 3.0, 12, "z"]], [3, 5, 15, 100])
    r1 = _resp([[8, 2.0, 0.125, 13, "u"], [7, 4.0, 0.75, 14, "v"]], [2, 6, 10, 50])
    out = B.BrokerReduceService().reduce_on_data_table(_REQ, {"s0": r0, "s1": r1})
    assert out.processing_exceptions == []
    assert (out.num_docs_scanned, out.num_entries_scanned_in_filter, out.num_entries_scanned_post_filter,
            out.total_docs) == (5, 11, 25, 150)
    # a DESC: 9 | 8 7(s0) 7(s1) | 1 ; offset 1, size 3; the columns in the request's order
    assert out.selection_results.columns == ["s", "f", "a"]
    assert out.selection_results.results == [["u", "0.125", "8"], ["y", "2.0", "7"], ["v", "0.75", "7"]]
    # SELECT *: the schema's columns sorted; an exception-only response contributes its exception
    req = dict(_REQ, selections=dict(_REQ["selections"], columns=["*"], offset=0, size=1))
    bad = B.InstanceResponse(exceptions={200: "boom"})
    out = B.BrokerReduceService().reduce_on_data_table(req, {"s0": r0, "s1": bad})
    assert out.selection_results.columns == ["a", "d", "f", "l", "s"]
    assert out.selection_results.results == [["9", "0.5", "1.5", "10", "x"]]
    assert [(e.error_code, e.message) for e in out.processing_exceptions] == [(200, "boom")]
    # aggregation requests reduce as before
    agg = pql.compile("SELECT COUNT(*) FROM t")
    out = B.BrokerReduceService().reduce_on_data_table(agg, {"s": B.InstanceResponse(aggregation=[4], stats=[4, 0, 0, 9])})
    assert out.selection_results is None and out.aggregation_results[0].value == "4"


def test_selection_datatable_round_trip():
    rows = [[-3, 0.1, float(np.float32(0.1)), -2 ** 63, "café"], [2 ** 31 - 1, -0.0, 3.5, 2 ** 63 - 1, ""],
            [0, 1e300, -1.25, 0, "café"]]
    resp = _resp(rows, [3, 4, 15, 30])
    raw = D.response_to_datatable(_REQ, resp)
    dt = D.DataTable.from_bytes(raw)
    assert dt.columns == _SCHEMA[0] and dt.types == _SCHEMA[1] and len(dt.rows) == 3
    assert dt.metadata[D.NUM_DOCS_SCANNED] == "3" and dt.metadata[D.TOTAL_DOCS] == "30"
    back = D.datatable_to_response(_REQ, raw)
    assert back.selection == rows and back.selection_schema == _SCHEMA and back.stats == [3, 4, 15, 30]
    assert str(back.selection[1][1]) == "-0.0"
    assert D.response_to_datatable(_REQ, back) == raw
    # the reduce accepts the bytes; an empty selection keeps its schema
    out = B.BrokerReduceService().reduce_on_data_table(_REQ, {"s0": raw})
    assert out.selection_results.results == [["café", "-1.25", "0"], ["café", "0.1", "-3"]]  # a DESC, offset 1
    empty = D.datatable_to_response(_REQ, D.response_to_datatable(_REQ, _resp([], [0, 0, 0, 30])))
    assert empty.selection == [] and empty.selection_schema == _SCHEMA
