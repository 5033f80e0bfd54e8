"""Reference model of the DISTINCTCOUNT / DISTINCTCOUNTMV kernels (pinot_amd/csrc/pgx_distinct.hip) in plain numpy: the
presence bitmap of the selected rows' dictIds (one bit per dictId, (card + 31) // 32 u32 words, under GROUP BY one such
row per slot), its set sizes and its hash codes in dictId order, and the descriptor structs and ctypes prototypes of
the six launchers libpgx.so exports.  The selection mask and the forward index are those of tests/select_ref.py, the
slots those of tests/hll_ref.py, the value rows of a multi-value column those of tests/hll_mv_ref.py.  A helper, not a
test: nothing here touches a GPU."""
import ctypes as C

import numpy as np

from tests import hll_mv_ref as M
from tests import hll_ref as R
from tests.select_ref import INVALID_VALUE, pack_fwd, pack_mask  # noqa: F401  (re-exported)

MAX_GROUP_COLS = R.MAX_GROUP_COLS
MAX_GROUP_SLOTS = R.MAX_GROUP_SLOTS
LDS_WORDS = 8192  # kDistinctLdsWords: bitmaps of up to that many words are marked in LDS


def words(card):
    return (card + 31) // 32


def mark(selected, ids, card, into=None):
    """The bitmap (uint32[words]) after ORing in the bit of every selected row's dictId below card."""
    bm = np.zeros(words(card), np.uint32) if into is None else np.asarray(into, np.uint32).copy()
    ids = np.asarray(ids, np.int64)[np.asarray(selected, dtype=bool)]
    ids = np.unique(ids[ids < card])
    np.bitwise_or.at(bm, ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
    return bm


def mark_group(selected, ids, card, slot, slots, into=None):
    """slots x words; slot: one per row (a row outside 0..slots-1 marks nothing)."""
    w = words(card)
    bm = np.zeros((slots, w), np.uint32) if into is None else np.asarray(into, np.uint32).copy()
    ids, slot = np.asarray(ids, np.int64), np.asarray(slot, np.int64)
    ok = np.asarray(selected, dtype=bool) & (ids < card) & (slot >= 0) & (slot < slots)
    np.bitwise_or.at(bm, (slot[ok], ids[ok] >> 5), (np.uint32(1) << (ids[ok] & 31).astype(np.uint32)))
    return bm


def mark_mv(selected, counts, ids, card, into=None, total=None):
    """Every value (ids: one dictId per value row) of every selected doc; value rows at or past `total` are not read."""
    rows = M.value_rows(selected, counts)
    if total is not None:
        rows = rows & (np.arange(len(rows)) < total)
    return mark(rows, ids, card, into)


def mark_mv_group(selected, counts, ids, card, slot, slots, into=None):
    slot = np.asarray(slot, np.int64)
    ok = np.asarray(selected, dtype=bool) & (slot >= 0) & (slot < slots)
    return mark_group(M.value_rows(ok, counts), ids, card, np.repeat(np.where(ok, slot, 0), counts), slots, into)


def set_ids(row, card):
    """Ascending dictIds below card whose bit is set in one bitmap row."""
    bits = np.unpackbits(np.asarray(row, np.uint32).view(np.uint8), bitorder="little")[:card]
    return np.flatnonzero(bits)


class DistinctItem(C.Structure):
    _fields_ = [("sel", C.c_void_p), ("fwd", C.c_void_p), ("out", C.c_void_p),
                ("bits", C.c_int32), ("num_docs", C.c_int32), ("card", C.c_int32), ("pad", C.c_int32)]


class DistinctGroupItem(C.Structure):
    _fields_ = [("d", DistinctItem), ("g", R.HllGCol * MAX_GROUP_COLS)]


class DistinctMvItem(C.Structure):
    _fields_ = [("d", DistinctItem), ("start", C.c_void_p), ("total", C.c_int32), ("pad", C.c_int32)]


class DistinctMvGroupItem(C.Structure):
    _fields_ = [("g", DistinctGroupItem), ("start", C.c_void_p), ("total", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(DistinctItem) == 40 and C.sizeof(DistinctGroupItem) == 40 + MAX_GROUP_COLS * 24
assert C.sizeof(DistinctMvItem) == 56 and C.sizeof(DistinctMvGroupItem) == C.sizeof(DistinctGroupItem) + 16


def bind(L):
    """Set the prototypes of the launchers on the loaded libpgx.so; returns a dict by kernel name.
    mark / mark_mv(items_dev, items_host, nitems, wgs_per_item, stream); mark_group / mark_mv_group(items_dev,
    items_host, nitems, ngcols, gmul_host, slots, wgs_per_item, stream); count(table, card, rows, nrows, slots, counts,
    wgs, stream); emit(table, card, rows, offsets, nrows, slots, hash, out, capacity, wgs_per_row, wgs, stream)."""
    out = {}
    for name, args in (
            ("mark", [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
            ("mark_mv", [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
            ("mark_group", [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
            ("mark_mv_group", [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
            ("count", [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]),
            ("emit", [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                      C.c_int64, C.c_int, C.c_int, C.c_void_p])):
        f = getattr(L, "pgx_launch_distinct_" + name)
        f.restype = C.c_int
        f.argtypes = args
        out[name] = f
    return out
