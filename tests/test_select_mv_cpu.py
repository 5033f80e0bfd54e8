"""Multi-value columns in selection queries, the parts that need no GPU: the numpy model of the pgx_select_mv_* kernels
(tests/select_mv_ref.py) against a per-doc brute force, the array cells of a selection DataTable, the value merge with an
array-typed order column, and the broker's rendering of array cells."""
import numpy as np
import pytest

from pinot_amd import broker as B
from pinot_amd import datatable as D
from pinot_amd import engine as E
from pinot_amd import pql
from tests import select_mv_ref as M


def _column(rng, num_docs, bits, max_len=4):
    lengths = rng.integers(0, max_len + 1, num_docs)
    start = M.starts_of(lengths)
    hi = (1 << bits) if bits < 32 else (1 << 32) - 1
    return start, rng.integers(0, hi, int(start[-1]), dtype=np.uint64)


@pytest.mark.parametrize("k", [1, 10, 300])
def test_model_against_brute_force(k):
    rng = np.random.default_rng(k)
    sizes, counts = (500, 40, 7), (min(k, 500), min(k, 3), 0)
    cols = [[_column(rng, n, bits) for n in sizes] for bits in (7, 32)]
    docs = [rng.permutation(n)[:k] if n >= k else np.concatenate([rng.permutation(n), np.full(k - n, -7)])
            for n in sizes]
    counts = tuple(min(c, n) for c, n in zip(counts, sizes))
    rel, totals, bases, values = M.mv_model(cols, docs, counts, k)
    rows = M.brute_force(cols, docs, counts)
    assert rel.shape == (6, k + 1) and bases[0] == 0 and bases[-1] == len(values) == sum(len(v) for r in rows for v in r)
    for p, pair_rows in enumerate(rows):
        cnt = counts[p % len(sizes)]
        assert len(pair_rows) == cnt and totals[p] == rel[p, k] == bases[p + 1] - bases[p]
        assert (rel[p, cnt:] == totals[p]).all()  # ranks at or past the count own nothing
        for r, exp in enumerate(pair_rows):
            np.testing.assert_array_equal(values[bases[p] + rel[p, r]:bases[p] + rel[p, r + 1]], exp)


def test_model_packs_the_stream_msb_first():
    packed = M.pack_values([5, 1, 7], 3)  # 101 001 111 -> 1010 0111 1000 0000
    assert packed[:2].tolist() == [0xA7, 0x80] and not packed[2:].any() and len(packed) >= 2 + 8


_NAMES = ["i", "l", "f", "d", "s", "k"]
_TYPES = ["INT_ARRAY", "LONG_ARRAY", "FLOAT_ARRAY", "DOUBLE_ARRAY", "STRING_ARRAY", "INT"]
_ROWS = [[[1, -2, 2147483647], [1 << 40, -(1 << 62)], [0.5, -1.25], [0.1, 1e300, -0.0], ["a", "zürich", "a"], 7],
         [[], [], [], [], [], -1],
         [[9], [-9], [float(np.float32(3.1))], [2.5], ["日本"], 0],
         [[3, 3], [5], [], [7.0], ["", "zürich"], 2]]


def test_array_cells_round_trip():
    """Empty arrays, a one-element array, non-ASCII strings, a string twice in one array and across rows.  No reference
    fixture holds such bytes: a round trip only, parity unpinned."""
    dt = D.DataTable(_NAMES, _TYPES)
    dt.rows = [list(r) for r in _ROWS]
    dt.metadata["numDocsScanned"] = "4"
    wire = dt.to_bytes()
    back = D.DataTable.from_bytes(wire)
    assert (back.columns, back.types, back.rows, back.metadata) == (_NAMES, _TYPES, _ROWS, dt.metadata)
    assert back.to_bytes() == wire
    # the fixed cell is (position in the variable-size section, number of elements): row 0's arrays lie back to back
    # from position 0 (3 ints, 2 longs, 2 floats of 4 bytes, 3 doubles, 3 dictionary ids)
    import struct
    head = struct.unpack_from(">13i", wire, 0)
    assert struct.unpack_from(">10i", wire, head[9]) == (0, 3, 12, 2, 28, 2, 36, 3, 60, 3)
    assert head[10] == 4 * (5 * 8 + 4)


def test_array_cells_through_the_response():
    q = pql.compile("SELECT * FROM t ORDER BY k LIMIT 5")
    resp = B.InstanceResponse(selection=[list(r) for r in _ROWS], selection_schema=(_NAMES, _TYPES), stats=[4, 0, 24, 4])
    wire = D.response_to_datatable(q, resp)
    back = D.datatable_to_response(q, wire)
    assert back.selection == _ROWS and back.selection_schema == (_NAMES, _TYPES) and back.stats == [4, 0, 24, 4]
    assert D.response_to_datatable(q, back) == wire


def test_merge_skips_an_array_typed_order_column():
    """ORDER BY a, v DESC, b with v multi-value: the order of (a, b) alone -- the arrays, which differ in every row and
    would decide before b, take no part."""
    types = ["INT", "INT_ARRAY", "STRING", "LONG"]
    order = [{"column": "a", "asc": True}, {"column": "v", "asc": False}, {"column": "b", "asc": False}]
    seg0 = [([1, [9], "x", 0], (0, 4)), ([1, [], "y", 0], (0, 2)), ([2, [5, 1], "x", 0], (0, 9))]
    seg1 = [([0, [3], "a", 0], (1, 1)), ([1, [0], "y", 0], (1, 0)), ([1, [8, 8], "z", 0], (1, 5))]
    rows = E.merge_selection_rows([seg0, seg1], types, order, 10)
    assert [r[1] for r in rows] == [(1, 1), (1, 5), (0, 2), (1, 0), (0, 4), (0, 9)]
    plain = E.merge_selection_rows([[([r[0][0], r[0][2]], r[1]) for r in s] for s in (seg0, seg1)], ["INT", "STRING"],
                                   [order[0], order[2]], 10)
    assert [r[1] for r in rows] == [r[1] for r in plain]
    assert [r[1] for r in E.merge_selection_rows([seg0, seg1], types, order, 2)] == [(1, 1), (1, 5)]


def test_broker_renders_array_cells():
    q = pql.compile("SELECT v, d, s, k FROM t ORDER BY k LIMIT 1, 2")
    schema = (["k", "d", "s", "v"], ["INT", "DOUBLE_ARRAY", "STRING_ARRAY", "INT_ARRAY"])
    a = B.InstanceResponse(selection=[[1, [0.5, 3.0], ["p", "q"], [1, 2]], [4, [], [], []]], selection_schema=schema,
                           stats=[2, 0, 8, 5])
    b = B.InstanceResponse(selection=[[0, [1.0], ["z"], [7]], [2, [1e-3, -2.25], ["é"], [-5]]], selection_schema=schema,
                           stats=[2, 0, 8, 5])
    wires = {"s0": D.response_to_datatable(q, a), "s1": D.response_to_datatable(q, b)}
    out = B.BrokerReduceService().reduce_on_data_table(q, wires)
    assert out.processing_exceptions == []
    assert out.selection_results.columns == ["v", "d", "s", "k"]
    assert out.selection_results.results == [[["1", "2"], ["0.5", "3.0"], ["p", "q"], "1"],
                                             [["-5"], ["0.001", "-2.25"], ["é"], "2"]]
    assert B.format_selection_cell("INT_ARRAY", [1, 2]) == ["1", "2"]
    assert B.format_selection_cell("DOUBLE_ARRAY", [2.0]) == [B.format_selection_value("DOUBLE", 2.0)] == ["2.0"]
    assert B.format_selection_cell("FLOAT_ARRAY", []) == []
    assert B.format_selection_cell("LONG", 5) == "5"
