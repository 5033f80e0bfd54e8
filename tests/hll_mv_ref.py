"""Reference model of the DISTINCTCOUNTHLLMV kernels (pinot_amd/csrc/pgx_hll.hip: pgx_hll_offer_mv,
pgx_hll_offer_mv_group) in plain numpy: the selected docs are expanded to selected value rows and handed to the
single-value model of tests/hll_ref.py, because offering every value of every selected doc is offering every selected
value row.  Also the descriptor structs and ctypes prototypes of the two launchers.  A helper, not a test: nothing here
touches a GPU."""
import ctypes as C

import numpy as np

from tests import hll_ref as R


def starts(counts):
    """The per-doc start array (int32, docs + 1 entries) of value counts per doc."""
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int32)


def value_rows(selected, counts):
    """bool per value row: the row belongs to a selected doc."""
    return np.repeat(np.asarray(selected, dtype=bool), np.asarray(counts, np.int64))


def offer(selected, counts, ids, code_table, into=None):
    """The 256 registers after offering every value (ids: one dictId per value row) of every selected doc."""
    return R.offer(value_rows(selected, counts), ids, code_table, into)


def offer_group(selected, counts, ids, code_table, slot, slots, into=None):
    """slots x 256 registers; slot: one per DOC (a doc outside 0..slots-1 offers nothing)."""
    slot = np.asarray(slot, np.int64)
    ok = np.asarray(selected, dtype=bool) & (slot >= 0) & (slot < slots)
    return R.offer_group(value_rows(ok, counts), ids, code_table, np.repeat(np.where(ok, slot, 0), counts), slots, into)


class HllMvItem(C.Structure):
    _fields_ = [("h", R.HllItem), ("start", C.c_void_p), ("total", C.c_int32), ("pad", C.c_int32)]


class HllMvGroupItem(C.Structure):
    _fields_ = [("g", R.HllGroupItem), ("start", C.c_void_p), ("total", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(HllMvItem) == 64 and C.sizeof(HllMvGroupItem) == C.sizeof(R.HllGroupItem) + 16


def bind(L):
    """Set the prototypes of the DISTINCTCOUNTHLLMV launchers on the loaded libpgx.so; returns (offer_mv,
    offer_mv_group), called like their single-value counterparts (tests/hll_ref.bind)."""
    of = L.pgx_launch_hll_offer_mv
    of.restype = C.c_int
    of.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    og = L.pgx_launch_hll_offer_mv_group
    og.restype = C.c_int
    og.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    return of, og
