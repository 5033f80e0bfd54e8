"""GPU parity of filters with more than 16 leaves (up to 64): leaf slots past 16 live in the per-segment extension
tables of the generated and the generic kernels, the device program is longer than 64 ops, and an all-bitmap AND / OR
past one bitmap program (24 ops, depth 4) is split into several programs whose masks the query program joins.

Three segments of 70,001 / 30,000 / 8,193 rows (two roaring chunks and a partial last tile; one whole 8,192-row tile
plus one row) with their own value ranges, so their dictionaries and leaf bindings differ, each with a twin without
inverted indexes.  Every query is checked against the CPU oracle: the answer and all four ExecutionStatistics,
numEntriesScannedInFilter from the oracle's literal iterator algebra.

The 16-leaf scan OR and the 8- and 9-leaf bitmap ORs are shapes the 16-leaf library ran before: they guard the old
path.  Every case of more than 16 leaves was refused with "too many filter leaves"."""
import copy
import json

import numpy as np
import pytest

from oracle import pinot_oracle as O
from pinot_amd import pql
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROWS = (70001, 30000, 8193)
MIXED = [(0, False), (1, False), (0, True), (2, False)]  # (segment, scan twin?): segment 0's twin among the three
SEL = "SELECT COUNT(*), SUM(m), MIN(m), MAX(m) FROM t WHERE "


@pytest.fixture(scope="module")
def ctx():
    from pinot_amd import engine as E
    c = E.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def segs(ctx):
    """[(inverted IndexSegment, scan-twin IndexSegment, inverted OSegment, scan-twin OSegment)] x 3."""
    from pinot_amd import engine as E
    rng = np.random.default_rng(23)
    out = []
    for k, n in enumerate(ROWS):
        raw = {"a": (rng.integers(0, 200, n) + 3 * k).astype(np.int32),
               "b": (rng.integers(0, 100, n) + 5 * k).astype(np.int32),
               "c": (rng.integers(0, 3000, n) + 11 * k).astype(np.int32),    # 12-bit dictIds
               "x": (rng.integers(0, 5, n) + k % 2).astype(np.int32),        # bitmap containers
               "y": (rng.integers(0, 300, n) + 2 * k).astype(np.int32),      # array containers
               "s": (np.arange(n, dtype=np.int64) * 40 // n + k).astype(np.int32),  # sorted
               "g": rng.integers(0, 17, n).astype(np.int32),
               "m": rng.integers(0, 1 << 20, n).astype(np.int32)}
        inv, oinv = H.build_pair("w%d" % k, raw, inverted=("x", "y"))
        scan, oscan = H.build_pair("w%ds" % k, raw)
        assert inv.columns["y"].inv_bytes is not None and inv.columns["s"].is_sorted
        out.append((E.IndexSegment(ctx, inv), E.IndexSegment(ctx, scan), oinv, oscan))
    return out


@pytest.fixture(scope="module", autouse=True)
def shared_filter_walks():
    """The oracle's literal walk of a filter is the slow step here.  The same filter over the same segment (with and
    without GROUP BY, under every knob) is walked once and its docs and entries shared, unchanged."""
    real, walks = O.filter_docs, {}

    def filter_docs(seg, tree):
        key = (id(seg), json.dumps(tree, sort_keys=True))
        if key not in walks:
            walks[key] = (seg, real(seg, tree))  # (the segment stays alive, so its id stays its own)
        docs, entries = walks[key][1]
        return docs.copy(), entries

    O.filter_docs = filter_docs
    yield
    O.filter_docs = real


_PARTS = {}  # (query text, segment, twin) -> the oracle's per-segment part (computed once, copied for every use)


def _oracle(segs, text, picks):
    """Oracle answer over picks = [(segment index, twin?)], in H.oracle_answer's form."""
    q = pql.compile(text)
    parts = []
    for k, twin in picks:
        key = (text, k, twin)
        if key not in _PARTS:
            run = O.run_group_by if q.get("group_by") else O.run_aggregation
            _PARTS[key] = run(segs[k][3 if twin else 2], q, literal_filter=True)
        parts.append(copy.deepcopy(_PARTS[key]))
    if q.get("group_by"):
        if len(parts) == 1:
            p = parts[0]
            return {"map": {p["string_key"](key): v for key, v in p["map"].items()}, "stats": p["stats"]}
        c = O.combine_group_by(parts, q)
        return {"map": c["merged"], "stats": c["stats"]}
    c = O.combine_aggregation(parts, q)
    return {"results": c["results"], "stats": c["stats"]}


def _answer(q, blk):
    if q.get("group_by"):
        m = blk.get_aggregation_group_by_result()
        return m.as_map() if m is not None else {}
    return blk.get_aggregation_result()


def _check(q, blk, stats, o, entries=True):
    fns = [a["fn"] for a in q["aggregations"]]
    got_st, exp_st = stats.as_list(), list(o["stats"])
    if not entries:  # (a list that mixes index kinds: see _check_each_and_combined)
        del got_st[1], exp_st[1]
    assert got_st == exp_st
    got = _answer(q, blk)
    if q.get("group_by"):
        assert set(got) == set(o["map"])
        for key, v in o["map"].items():
            H.assert_values_equal(got[key], v, fns)
    else:
        H.assert_values_equal(got, o["results"], fns)


def _run_inner(ctx, gseg, q):
    from pinot_amd import engine as E
    op = E.InstancePlanMakerImplV2(ctx).make_inner_segment_plan(gseg, q).run()
    blk = op.next_block()
    return blk, op.get_execution_statistics()


def _check_each_and_combined(ctx, segs, text, mixed=True):
    """The query per segment, as one inter-segment plan over the three segments, and as one with segment 0's scan twin
    mixed in.  One plan takes every leaf's operator kind from its first segment (as before this file), so with the
    twin in the list numEntriesScannedInFilter counts the twin's rows like an inverted segment's, not like the
    oracle's scan of them: there the answer and the other three statistics are checked (tests/test_gpu_bitmap.py's mixed
    lists check the answer alone)."""
    from pinot_amd import engine as E
    q = pql.compile(text)
    pm = E.InstancePlanMakerImplV2(ctx)
    for k in range(len(segs)):
        blk, st = _run_inner(ctx, segs[k][0], q)
        _check(q, blk, st, _oracle(segs, text, [(k, False)]))
    picks = [(k, False) for k in range(len(segs))]
    blk = pm.make_inter_segment_plan([segs[k][0] for k, _ in picks], q).execute()
    _check(q, blk, blk.stats, _oracle(segs, text, picks))
    if not mixed:
        return
    blk = pm.make_inter_segment_plan([segs[k][1 if t else 0] for k, t in MIXED], q).execute()
    _check(q, blk, blk.stats, _oracle(segs, text, MIXED), entries=False)


# 1. flat OR of 40 mixed leaves: 14 scan EQ, 6 scan ranges, 12 + 1 bitmap leaves (one program cannot hold 13), 7 sorted
OR40 = " OR ".join(["a = %d" % v for v in range(10, 150, 10)] + ["b > %d" % v for v in range(90, 96)] +
                   ["y = %d" % v for v in range(20, 260, 20)] + ["x = 4"] + ["s = %d" % v for v in range(3, 38, 5)])
assert OR40.count(" OR ") == 39

# 3. flat AND with statistics: a bitmap leaf and a sorted leaf, then 20 scan leaves (non-empty in every segment), whose
# entries are the running candidates' popcounts
AND22 = " AND ".join(["x <> 9", "s BETWEEN 5 AND 34"] + ["a <> %d" % v for v in range(12, 132, 10)] +
                     ["b < %d" % v for v in range(97, 89, -1)])
assert AND22.count(" AND ") == 22  # (BETWEEN's own AND included)


@pytest.mark.parametrize("group", ["", " GROUP BY g"])
def test_flat_or_of_40_mixed_leaves(ctx, segs, group):
    _check_each_and_combined(ctx, segs, SEL + OR40 + group)


def _scan_or(n):
    """Flat OR of n scan leaves over a, b and c (EQ, IN with a bitset binding, ranges)."""
    leaves = []
    for i in range(n):
        if i % 3 == 0:
            leaves.append("a = %d" % (8 + 2 * i))
        elif i % 3 == 1:
            leaves.append("b IN (%d, %d)" % (6 + i, 60 + i // 2))
        else:
            leaves.append("c BETWEEN %d AND %d" % (40 * i, 40 * i + 9))
    return " OR ".join(leaves)


@pytest.mark.parametrize("n", [16, 17, 32, 33, 64])
def test_leaf_count_boundaries(ctx, segs, n):
    """17: the first extension slot.  33: the first program past 64 ops (65).  64: the limit."""
    text = SEL + _scan_or(n)
    q = pql.compile(text)
    for k in range(len(segs)):
        blk, st = _run_inner(ctx, segs[k][0], q)
        _check(q, blk, st, _oracle(segs, text, [(k, False)]))


def test_65_leaves_are_refused_and_the_context_stays_usable(ctx, segs):
    from pinot_amd import native as N
    with pytest.raises(N.PgxError) as e:
        _run_inner(ctx, segs[2][0], pql.compile(SEL + _scan_or(65)))
    assert e.value.status == N.PGX_ERR_UNSUPPORTED
    assert "64" in str(e.value)  # the message names the limit
    text = SEL + _scan_or(17)
    q = pql.compile(text)
    blk, st = _run_inner(ctx, segs[2][0], q)
    _check(q, blk, st, _oracle(segs, text, [(2, False)]))


@pytest.mark.parametrize("group", ["", " GROUP BY g"])
def test_flat_and_with_statistics(ctx, segs, group):
    _check_each_and_combined(ctx, segs, SEL + AND22 + group, mixed=False)


# 4. all-bitmap trees past one program
def _y_or(n, first=3, step=7):
    return " OR ".join("y = %d" % (first + step * i) for i in range(n))


NESTED40 = ("(" + _y_or(12) + " OR y = 123456) AND ((" + _y_or(10, 5, 11) + " OR x = 1 OR x = 3) OR (y NOT IN (7, 8, 9)"
            " AND (" + _y_or(6, 100, 3) + ") AND x <> 2)) AND (" + _y_or(6, 4, 9) + " OR x IN (0, 4))")
BITMAP_TREES = {
    "or8": _y_or(8),
    "or9": _y_or(9),
    "or13": _y_or(13),
    "or40": _y_or(40),
    "neq8": " OR ".join(["y <> %d" % (10 + 9 * i) for i in range(8)] + ["x = 2"]),  # 8 RP_NOTs: 26 ops
    "nested40": NESTED40,
}
assert sum(NESTED40.count(t) for t in (" = ", " <> ", " IN ")) == 40


@pytest.mark.parametrize("rchunk", [None, "0"])
@pytest.mark.parametrize("name", list(BITMAP_TREES))
def test_all_bitmap_trees_past_one_program(ctx, segs, name, rchunk, monkeypatch):
    """Under the planner's default and with the separate pass forced.  Each answer also equals the scan twin's.  The
    nested tree's twin is an AND of ORs over 40 scan leaves: its statistic needs the automaton, which stays at 10
    leaves, so the library refuses the twin and the oracle's answer over the twin stands in for it."""
    from pinot_amd import native as N
    if rchunk is not None:
        monkeypatch.setenv("PGX_RCHUNK", rchunk)
    text = SEL + BITMAP_TREES[name]
    q = pql.compile(text)
    for k in range(len(segs)):
        blk, st = _run_inner(ctx, segs[k][0], q)
        o = _oracle(segs, text, [(k, False)])
        _check(q, blk, st, o)
        assert o["stats"][1] == 0  # no scan leaf
        if name == "nested40":
            with pytest.raises(N.PgxError) as e:
                _run_inner(ctx, segs[k][1], q)
            assert e.value.status == N.PGX_ERR_UNSUPPORTED
            twin = _oracle(segs, text, [(k, True)])["results"]
        else:
            twin = _run_inner(ctx, segs[k][1], q)[0].get_aggregation_result()
        assert blk.get_aggregation_result() == twin


@pytest.mark.parametrize("group", ["", " GROUP BY g"])
def test_sorted_leaf_and_two_bitmap_ors(ctx, segs, group):
    # (s IN: a sorted-index leaf; a range over s would be a scan leaf)
    text = (SEL + "s IN (%s) AND (" % ", ".join(str(v) for v in range(4, 31)) + _y_or(20) + ") AND (" +
            _y_or(11, 3, 14) + " OR x = 1)" + group)
    q = pql.compile(text)
    for k in range(len(segs)):
        blk, st = _run_inner(ctx, segs[k][0], q)
        o = _oracle(segs, text, [(k, False)])
        _check(q, blk, st, o)
        assert st.num_entries_scanned_in_filter == 0


@pytest.mark.parametrize("flt", [OR40, AND22], ids=["or40", "and22"])
def test_generic_kernel_agrees(ctx, segs, flt, monkeypatch):
    """PGX_JIT=0: the generic kernel reads leaves past 16 from KQuery's table and runs the longer program."""
    monkeypatch.setenv("PGX_JIT", "0")
    _check_each_and_combined(ctx, segs, SEL + flt, mixed=flt is OR40)
    _check_each_and_combined(ctx, segs, SEL + flt + " GROUP BY g", mixed=flt is OR40)


def test_plan_cache_replay_is_identical(ctx, segs):
    from pinot_amd import engine as E
    text = SEL + OR40 + " GROUP BY g"
    q = pql.compile(text)
    pm = E.InstancePlanMakerImplV2(ctx)
    gsegs = [segs[k][1 if t else 0] for k, t in MIXED]
    first = pm.make_inter_segment_plan(gsegs, q).execute()
    second = pm.make_inter_segment_plan(gsegs, q).execute()
    assert _answer(q, first) == _answer(q, second)
    assert first.stats.as_list() == second.stats.as_list()
    assert first.trimmed == second.trimmed
    _check(q, second, second.stats, _oracle(segs, text, MIXED), entries=False)
