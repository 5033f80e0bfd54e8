"""Selection without ORDER BY, the parts that need no GPU: the model of tests/select_only_ref.py against the oracle's
literal filter iterators pulled p times (the classes of filter whose numEntriesScannedInFilter has a closed form under
MSelectionOnlyOperator's early stop, and why the other shapes are refused), the engine's merge without ordering, the
broker reduce and render, and the DataTable round trip."""
import numpy as np
import pytest

from oracle import pinot_oracle as O
from pinot_amd import broker as B
from pinot_amd import datatable as D
from pinot_amd import engine as E
from pinot_amd import pql
from tests import select_only_ref as R

PULLS = (1, 10, 2048)

# (filter text, class).  a: no filter, sorted / bitmap leaves only; b: one scan leaf; d: a root AND of leaves with a
# sorted / bitmap leaf; None: refused.  a has no index, b and c carry bitmaps, s is sorted; a range predicate scans.
FILTERS = [
    ("", "a"),
    (" WHERE b IN (0, 55)", "a"),
    (" WHERE s = 4", "a"),
    (" WHERE b = 55 OR c = 7 OR s = 1", "a"),
    (" WHERE s = 2 AND (b IN (0, 55, 110) OR c = 9)", "a"),
    (" WHERE a > 2900", "b"),
    (" WHERE a = 12345", "b"),                       # a value outside the dictionary: nothing matches
    (" WHERE c > 690", "b"),                         # a range on a bitmap column scans
    (" WHERE a > 0 AND b IN (0, 55)", "d"),
    (" WHERE a > 0 AND s = 2 AND c < 300", "d"),     # two scans behind a sorted range
    (" WHERE a = 12345 AND b = 55", "d"),            # an always-false scan behind a bitmap
    (" WHERE a > 0 AND c < 300", None),              # an AND of scans
    (" WHERE a > 2000 OR b = 55", None),             # an OR with a scan leaf
    (" WHERE a > 2000 OR c > 600", None),            # an OR of scans
    (" WHERE b <> 55 AND (a > 0 OR c = 7)", None),   # a nested operator over a lazily iterated scan
    (" WHERE s = 2 AND (a > 1000 AND c < 500)", None),
]


@pytest.fixture(scope="module")
def seg():
    rng = np.random.default_rng(5)
    n = 20000
    raw = {"a": rng.integers(-3000, 3000, size=n).astype(np.int32),
           "b": rng.integers(0, 40, size=n).astype(np.int32) * 11,
           "c": rng.integers(0, 700, size=n).astype(np.int32),
           "s": np.sort(rng.integers(0, 6, size=n)).astype(np.int32)}
    return O.OSegment.from_raw(raw, inverted=("b", "c")), n


@pytest.fixture(scope="module")
def full(seg):
    """The full run of every filter, computed once: (docIds, numEntriesScannedInFilter)."""
    oseg, _ = seg
    out = {}
    for text, _ in FILTERS:
        docs, entries = O.filter_docs(oseg, pql.compile("SELECT a FROM t" + text)["filter"])
        out[text] = (docs.tolist(), entries)
    return out


@pytest.mark.parametrize("text,cls", FILTERS)
def test_classes_and_closed_forms(seg, full, text, cls):
    oseg, n = seg
    tree = pql.compile("SELECT a FROM t" + text)["filter"]
    assert R.classify(tree, oseg) == cls
    docs_full, entries_full = full[text]
    differs = False
    for p in PULLS:
        docs, entries = R.pulled(oseg, tree, p)
        assert docs == docs_full[:p]
        assert docs == R.first_docs(O.filter_mask_vectorized(oseg, tree), p).tolist()
        if cls is not None:
            assert R.early_entries(cls, docs, p, n, entries_full) == entries, (p, entries, entries_full)
        differs |= entries not in (0, entries_full)
    if cls is None:
        assert differs  # neither 0 nor the full run's number: the shape has to be refused
    if cls == "b":
        assert entries_full == n


def test_first_docs_and_stripes():
    sel = np.zeros(1000, bool)
    sel[[3, 500, 999]] = True
    assert R.first_docs(sel, 2).tolist() == [3, 500] and R.first_docs(sel, 10).tolist() == [3, 500, 999]
    assert R.first_docs(np.zeros(0, bool), 5).tolist() == []
    assert R.stripes(1000, 1) == [(0, 1000)]
    assert R.stripes(1000, 3) == [(0, 384), (384, 768), (768, 1000)]      # 8 chunks of 128 rows: 3 + 3 + 2
    assert R.stripes(100, 3) == [(0, 100), (100, 100), (100, 100)]
    assert R.stripes(0, 2) == [(0, 0), (0, 0)]
    assert R.stripe_counts(sel, 10, 3).tolist() == [1, 1, 1] and R.stripe_counts(np.ones(1000, bool), 200, 3).tolist() \
        == [200, 200, 200]


# ---------------------------------------------------------------------------------------------------------------------
# the merge without ordering
# ---------------------------------------------------------------------------------------------------------------------
def _lists(counts):
    return [[([s * 100 + i], (s, i * 3)) for i in range(c)] for s, c in enumerate(counts)]


@pytest.mark.parametrize("counts,size", [
    ((4, 0, 3), 5),      # a segment with no rows
    ((6, 2, 2), 5),      # the first segment already fills `size`
    ((5, 5), 5),
    ((2, 1, 0), 10),     # fewer rows than `size` in all
    ((0, 0), 3),
    ((3,), 0),
])
def test_merge_selection_rows_unordered(counts, size):
    lists = _lists(counts)
    got = E.merge_selection_rows_unordered(lists, size)
    assert got == R.merge_unordered(lists, size)
    assert len(got) == min(size, sum(counts))
    assert [r[1] for r in got] == sorted(r[1] for r in got)  # segments in call order, rows in docId order


# ---------------------------------------------------------------------------------------------------------------------
# broker reduce / render, DataTable
# ---------------------------------------------------------------------------------------------------------------------
_SCHEMA = (["a", "d", "s", "v"], ["INT", "DOUBLE", "STRING", "INT_ARRAY"])


def _req(columns, offset, size):
    return {"table": "t", "aggregations": [], "group_by": None, "filter": None,
            "selections": {"columns": columns, "order_by": [], "offset": offset, "size": size}}


def _responses():
    r0 = B.InstanceResponse(selection=[[9, 0.5, "x", [1, 2]], [1, 0.25, "y", []], [7, 1.0, "z", [3]]],
                            selection_schema=_SCHEMA, stats=[3, 5, 12, 100])
    r1 = B.InstanceResponse(selection=[[8, 2.0, "u", [4, 5, 6]], [2, 4.0, "v", [7]], [3, 8.0, "w", [8]]],
                            selection_schema=_SCHEMA, stats=[3, 6, 12, 50])
    return r0, r1


def test_broker_reduce_without_order_by():
    r0, r1 = _responses()
    red = B.BrokerReduceService()
    # the responses in the given order, their rows in order, cut at `size`; the offset plays no part: LIMIT 3, 5
    # renders 5 rows, from the first
    out = red.reduce_on_data_table(_req(["s", "a"], 3, 5), {"s0": r0, "s1": r1})
    assert out.processing_exceptions == []
    assert (out.num_docs_scanned, out.num_entries_scanned_in_filter, out.num_entries_scanned_post_filter,
            out.total_docs) == (6, 11, 24, 150)
    assert out.selection_results.columns == ["s", "a"]
    assert out.selection_results.results == [["x", "9"], ["y", "1"], ["z", "7"], ["u", "8"], ["v", "2"]]
    out = red.reduce_on_data_table(_req(["s", "a"], 3, 5), {"s1": r1, "s0": r0})
    assert out.selection_results.results == [["u", "8"], ["v", "2"], ["w", "3"], ["x", "9"], ["y", "1"]]
    assert red.reduce_on_data_table(_req(["a"], 0, 2), {"s0": r0, "s1": r1}).selection_results.results == [["9"], ["1"]]
    assert len(red.reduce_on_data_table(_req(["a"], 0, 50), {"s0": r0, "s1": r1}).selection_results.results) == 6
    # "*" renders the schema's columns sorted by name; an _ARRAY cell is the list of its values
    out = red.reduce_on_data_table(_req(["*"], 0, 4), {"s0": r0, "s1": r1})
    assert out.selection_results.columns == ["a", "d", "s", "v"]
    assert out.selection_results.results == [["9", "0.5", "x", ["1", "2"]], ["1", "0.25", "y", []],
                                             ["7", "1.0", "z", ["3"]], ["8", "2.0", "u", ["4", "5", "6"]]]
    # the compiled request takes the same route
    q = pql.compile("SELECT s, a FROM t LIMIT 3, 5")
    assert q["selections"]["order_by"] == [] and (q["selections"]["offset"], q["selections"]["size"]) == (3, 5)
    assert len(red.reduce_on_data_table(q, {"s0": r0, "s1": r1}).selection_results.results) == 5


def test_datatable_round_trip_without_order_by():
    r0, r1 = _responses()
    req = _req(["*"], 0, 4)
    wires = [D.response_to_datatable(req, r) for r in (r0, r1)]
    for wire, r in zip(wires, (r0, r1)):
        back = D.datatable_to_response(req, wire)
        assert back.selection == r.selection and back.selection_schema == _SCHEMA and back.stats == r.stats
        assert D.response_to_datatable(req, back) == wire
    out = B.BrokerReduceService().reduce_on_data_table(req, {"s0": wires[0], "s1": wires[1]})
    direct = B.BrokerReduceService().reduce_on_data_table(req, {"s0": r0, "s1": r1})
    assert out.selection_results == direct.selection_results and len(out.selection_results.results) == 4
