"""pgx_histogram_percentile (pinot_amd/csrc/pgx_percentile.cpp), the host helper that reduces a (value, count) histogram
as PercentileUtil.getValueOnQuantile reduces the sorted value list, against extended.percentile_of_histogram and against
sorting the expanded list; and the numpy model of the counter tables (tests/percentile_ref.py) against Python Counters.
No GPU needed."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from pinot_amd import extended as X
from pinot_amd import native as N
from tests import hll_mv_ref as M
from tests import percentile_ref as P


def _native(hist, p):
    values = np.ascontiguousarray([v for v, _ in hist], dtype=np.float64)
    counts = np.ascontiguousarray([c for _, c in hist], dtype=np.int64)
    out = C.c_double(-12345.0)
    st = N.lib().pgx_histogram_percentile(values.ctypes.data if len(hist) else None,
                                          counts.ctypes.data if len(hist) else None, len(hist), p, C.byref(out))
    return st, out.value


def _hist(rng, size):
    """`size` values drawn with repeats from a few dozen doubles, as the ascending (value, count) pairs."""
    pool = np.unique(np.round(rng.normal(0, 100, max(2, size // 3 + 1)), 2))
    return sorted(Counter(rng.choice(pool, size).tolist()).items())


@pytest.mark.parametrize("size", [1, 2, 3, 100, 101])
@pytest.mark.parametrize("p", [50, 90, 95, 99])
def test_percentile_of_a_histogram(size, p):
    rng = np.random.default_rng(size * 1000 + p)
    hist = _hist(rng, size)
    assert sum(c for _, c in hist) == size
    st, got = _native(hist, p)
    assert st == 0
    assert got == X.percentile_of_histogram("percentile%d" % p, hist)
    expanded = sorted(v for v, c in hist for _ in range(c))
    assert got == expanded[int(size * (p / 100.0))]


def test_a_count_above_two_to_the_32():
    hist = [(-2.5, 3), (0.0, (1 << 32) + 7), (1.5, 1 << 33), (7.25, 5)]
    for p in (0, 50, 90, 95, 99):
        st, got = _native(hist, p)
        assert st == 0 and got == X.percentile_of_histogram("percentile%d" % p, hist)
    assert _native(hist, 0)[1] == -2.5 and _native(hist, 99)[1] == 1.5
    assert _native([(1.0, 1 << 40), (2.0, 1 << 40)], 50)[1] == 2.0  # index 2^40 is the first element of the second run


def test_refusals_leave_the_output_alone():
    hist = [(1.0, 2), (2.0, 3)]
    for bad_p in (-1, 101):
        assert _native(hist, bad_p) == (N.PGX_ERR_INVALID_ARG, -12345.0)
    assert _native([(1.0, 2), (2.0, -3)], 50) == (N.PGX_ERR_INVALID_ARG, -12345.0)       # a negative count
    assert _native([(2.0, 2), (1.0, 3)], 50) == (N.PGX_ERR_INVALID_ARG, -12345.0)        # unsorted
    assert _native([(1.0, 2), (1.0, 3)], 50) == (N.PGX_ERR_INVALID_ARG, -12345.0)        # equal values: not one entry
    assert _native([], 50) == (N.PGX_ERR_INVALID_ARG, -12345.0)                          # empty
    assert _native([(1.0, 0), (2.0, 0)], 50) == (N.PGX_ERR_INVALID_ARG, -12345.0)        # empty multiset
    with pytest.raises(IndexError):
        X.percentile_of_histogram("percentile50", [])
    assert _native(hist, 50) == (0, 2.0)


def test_function_codes_and_limits_are_bound():
    assert (N.PGX_PERCENTILEMV, N.PGX_PERCENTILE) == (14, 15)
    assert N.PGX_PERCENTILE_MAX_TABLE_BYTES == 256 << 20
    from pinot_amd import engine as E
    assert E._FN["percentile"] == 15 and E._FN["percentilemv"] == 14
    for name in ("pgx_result_percentile_counts", "pgx_result_percentile") + tuple(
            "pgx_launch_percentile_" + k for k in ("count", "count_group", "count_mv", "count_mv_group", "sizes",
                                                   "emit")):
        assert hasattr(N.lib(), name)


# ---- the numpy model against Python Counters ---------------------------------------------------------------------------
def test_model_count_matches_a_counter():
    rng = np.random.default_rng(3)
    n, card = 5000, 37
    ids = rng.integers(0, card + 4, n)  # ids at and past card count nothing
    sel = rng.random(n) < 0.4
    pre = rng.integers(0, 1000, card).astype(np.uint64)
    got = P.count(sel, ids, card, pre)
    cnt = Counter(int(i) for i, s in zip(ids, sel) if s and i < card)
    assert [int(x) for x in got] == [int(pre[i]) + cnt.get(i, 0) for i in range(card)]
    assert (P.count(np.zeros(n, bool), ids, card) == 0).all()
    pids, pcounts = P.nonzero_pairs(P.count(sel, ids, card))
    assert list(zip(pids.tolist(), pcounts.tolist())) == sorted(cnt.items())


def test_model_count_group_matches_counters_per_slot():
    rng = np.random.default_rng(4)
    n, card, slots = 4000, 11, 6
    ids, slot = rng.integers(0, card + 2, n), rng.integers(-1, slots + 2, n)
    sel = rng.random(n) < 0.7
    got = P.count_group(sel, ids, card, slot, slots)
    exp = Counter((int(s), int(i)) for i, s, k in zip(ids, slot, sel) if k and i < card and 0 <= s < slots)
    assert got.shape == (slots, card)
    assert {(s, i): int(got[s, i]) for s in range(slots) for i in range(card) if got[s, i]} == dict(exp)


def test_model_mv_counts_every_value_of_every_selected_doc():
    rng = np.random.default_rng(5)
    ndocs, card, slots = 900, 23, 4
    counts = rng.integers(0, 5, ndocs)
    counts[17] = 70
    total = int(counts.sum())
    ids, slot = rng.integers(0, card, total), rng.integers(-1, slots + 1, ndocs)
    sel = rng.random(ndocs) < 0.5
    start = M.starts(counts)
    exp, gexp = Counter(), Counter()
    for d in range(ndocs):
        if sel[d]:
            for r in range(start[d], start[d + 1]):
                exp[int(ids[r])] += 1
                if 0 <= slot[d] < slots:
                    gexp[(int(slot[d]), int(ids[r]))] += 1
    got = P.count_mv(sel, counts, ids, card)
    assert {i: int(c) for i, c in enumerate(got) if c} == dict(exp)
    cut = P.count_mv(sel, counts, ids, card, total=total - 40)
    assert int(cut.sum()) == sum(1 for d in range(ndocs) if sel[d] for r in range(start[d], start[d + 1])
                                 if r < total - 40)
    ggot = P.count_mv_group(sel, counts, ids, card, slot, slots)
    assert {(s, i): int(ggot[s, i]) for s in range(slots) for i in range(card) if ggot[s, i]} == dict(gexp)
