"""Reference model of the PERCENTILE / PERCENTILEMV kernels (pinot_amd/csrc/pgx_percentile.hip) in plain numpy: the
counter table of the selected rows' dictIds (one u64 counter per dictId, `card` of them, under GROUP BY one such row per
slot), its non-zero (dictId, count) pairs in dictId order, and the descriptor structs and ctypes prototypes of the six
launchers libpgx.so exports.  The selection mask and the forward index are those of tests/select_ref.py, the slots
those of tests/hll_ref.py, the value rows of a multi-value column those of tests/hll_mv_ref.py.  A helper, not a test:
nothing here touches a GPU."""
import ctypes as C

import numpy as np

from tests import hll_mv_ref as M
from tests import hll_ref as R
from tests.select_ref import INVALID_VALUE, pack_fwd, pack_mask  # noqa: F401  (re-exported)

MAX_GROUP_COLS = R.MAX_GROUP_COLS
MAX_GROUP_SLOTS = R.MAX_GROUP_SLOTS
LDS_COUNTERS = 8192  # kPercentileLdsCounters: tables of up to that many counters (slots x card) are counted in LDS


def count(selected, ids, card, into=None):
    """The counters (uint64[card]) after adding one per selected row whose dictId lies below card."""
    t = np.zeros(card, np.uint64) if into is None else np.asarray(into, np.uint64).copy()
    ids = np.asarray(ids, np.int64)[np.asarray(selected, dtype=bool)]
    ids = ids[(ids >= 0) & (ids < card)]
    t += np.bincount(ids, minlength=card).astype(np.uint64)  # (u64 addition wraps as the device's does)
    return t


def count_group(selected, ids, card, slot, slots, into=None):
    """slots x card; slot: one per row (a row outside 0..slots-1 counts nothing)."""
    t = np.zeros((slots, card), np.uint64) if into is None else np.asarray(into, np.uint64).copy()
    ids, slot = np.asarray(ids, np.int64), np.asarray(slot, np.int64)
    ok = np.asarray(selected, dtype=bool) & (ids >= 0) & (ids < card) & (slot >= 0) & (slot < slots)
    flat = np.bincount(slot[ok] * card + ids[ok], minlength=slots * card).astype(np.uint64)
    return t + flat.reshape(slots, card)


def count_mv(selected, counts, ids, card, into=None, total=None):
    """Every value (ids: one dictId per value row) of every selected doc; value rows at or past `total` are not read."""
    rows = M.value_rows(selected, counts)
    if total is not None:
        rows = rows & (np.arange(len(rows)) < total)
    return count(rows, ids, card, into)


def count_mv_group(selected, counts, ids, card, slot, slots, into=None):
    slot = np.asarray(slot, np.int64)
    ok = np.asarray(selected, dtype=bool) & (slot >= 0) & (slot < slots)
    return count_group(M.value_rows(ok, counts), ids, card, np.repeat(np.where(ok, slot, 0), counts), slots, into)


def nonzero_pairs(row):
    """(dictIds, counts) of one table row's non-zero counters, dictIds ascending."""
    row = np.asarray(row, np.uint64)
    ids = np.flatnonzero(row)
    return ids.astype(np.int32), row[ids]


class PercentileItem(C.Structure):
    _fields_ = [("sel", C.c_void_p), ("fwd", C.c_void_p), ("out", C.c_void_p),
                ("bits", C.c_int32), ("num_docs", C.c_int32), ("card", C.c_int32), ("pad", C.c_int32)]


class PercentileGroupItem(C.Structure):
    _fields_ = [("d", PercentileItem), ("g", R.HllGCol * MAX_GROUP_COLS)]


class PercentileMvItem(C.Structure):
    _fields_ = [("d", PercentileItem), ("start", C.c_void_p), ("total", C.c_int32), ("pad", C.c_int32)]


class PercentileMvGroupItem(C.Structure):
    _fields_ = [("g", PercentileGroupItem), ("start", C.c_void_p), ("total", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(PercentileItem) == 40 and C.sizeof(PercentileGroupItem) == 40 + MAX_GROUP_COLS * 24
assert C.sizeof(PercentileMvItem) == 56 and C.sizeof(PercentileMvGroupItem) == C.sizeof(PercentileGroupItem) + 16


def bind(L):
    """Set the prototypes of the launchers on the loaded libpgx.so; returns a dict by kernel name.
    count / count_mv(items_dev, items_host, nitems, wgs_per_item, stream); count_group / count_mv_group(items_dev,
    items_host, nitems, ngcols, gmul_host, slots, wgs_per_item, stream); sizes(table, card, rows, nrows, slots, sizes,
    wgs, stream); emit(table, card, rows, offsets, nrows, slots, ids, counts, capacity, wgs_per_row, wgs, stream)."""
    out = {}
    for name, args in (
            ("count", [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
            ("count_mv", [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
            ("count_group", [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
            ("count_mv_group", [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
            ("sizes", [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]),
            ("emit", [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                      C.c_int64, C.c_int, C.c_int, C.c_void_p])):
        f = getattr(L, "pgx_launch_percentile_" + name)
        f.restype = C.c_int
        f.argtypes = args
        out[name] = f
    return out
