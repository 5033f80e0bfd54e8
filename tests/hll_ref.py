"""Reference model of the DISTINCTCOUNTHLL kernels (pinot_amd/csrc/pgx_hll.hip) in plain numpy: the per-dictId codes
(pinot_amd/hll.py's hash and offer over extended.java_hash_code), the register-wise max of the selected rows' offers,
aggregation-only and per group slot, and the descriptor structs and ctypes prototypes of the launchers libpgx.so
exports.  The selection mask and the forward index are those of tests/select_ref.py.  A helper, not a test: nothing here
touches a GPU (tests/test_hll_codes_cpu.py checks pgx_hll_codes against the model, tests/test_gpu_hll_kernels.py the
kernels)."""
import ctypes as C

import numpy as np

from pinot_amd import extended as X
from pinot_amd import hll as H
from tests.select_ref import INVALID_VALUE, pack_fwd, pack_mask  # noqa: F401  (re-exported)

REGS = 256               # kHllRegs
MAX_GROUP_COLS = 16      # kMaxGroupCols
MAX_GROUP_SLOTS = 65536  # PGX_HLL_MAX_GROUP_SLOTS
MAX_RANK = 25            # nlz((x << 8) | 0x81) + 1 with bit 7 forced on


def codes_of_hashes(hash_codes):
    """(register << 8) | rank of HyperLogLog.offer(int) for every Java int hash code."""
    h = H.hash_long(np.asarray(hash_codes, dtype=np.int64))
    j = (h >> np.uint32(32 - H.LOG2M)).astype(np.uint32)
    with np.errstate(over="ignore"):
        w = (h << np.uint32(H.LOG2M)) | np.uint32((1 << (H.LOG2M - 1)) + 1)
    r = (H._nlz32(w) + 1).astype(np.uint32)
    return ((j << np.uint32(8)) | r).astype(np.uint16)


def codes(dtype, values):
    """One code per value of a column of type INT / LONG / FLOAT / DOUBLE / STRING."""
    return codes_of_hashes([X.java_hash_code(dtype, v) for v in values])


def offer(selected, ids, code_table, into=None):
    """The 256 registers after offering every selected row's value, maxed into `into` (uint32)."""
    regs = np.zeros(REGS, np.uint32) if into is None else np.asarray(into, np.uint32).copy()
    c = np.asarray(code_table, np.uint32)[np.asarray(ids)[np.asarray(selected, dtype=bool)]]
    np.maximum.at(regs, c >> 8, c & 0xFF)
    return regs


def group_slots(gcols, gmul):
    """Slot per row: sum over the group columns of remap[id] * gmul (remap None: identity).  gcols: [(ids, remap)]."""
    slot = 0
    for (ids, remap), m in zip(gcols, gmul):
        g = np.asarray(ids, np.int64)
        if remap is not None:
            g = np.asarray(remap, np.int64)[g]
        slot = slot + g * int(m)
    return np.asarray(slot, np.int64)


def offer_group(selected, ids, code_table, slot, slots, into=None):
    """slots x 256 registers after offering every selected row's value to its slot's registers."""
    regs = np.zeros((slots, REGS), np.uint32) if into is None else np.asarray(into, np.uint32).copy()
    sel = np.asarray(selected, dtype=bool)
    c = np.asarray(code_table, np.uint32)[np.asarray(ids)[sel]]
    np.maximum.at(regs, (np.asarray(slot)[sel], c >> 8), c & 0xFF)
    return regs


class HllItem(C.Structure):
    _fields_ = [("sel", C.c_void_p), ("fwd", C.c_void_p), ("codes", C.c_void_p), ("out", C.c_void_p),
                ("bits", C.c_int32), ("num_docs", C.c_int32), ("ncodes", C.c_int32), ("pad", C.c_int32)]


class HllGCol(C.Structure):
    _fields_ = [("fwd", C.c_void_p), ("remap", C.c_void_p), ("bits", C.c_int32), ("pad", C.c_int32)]


class HllGroupItem(C.Structure):
    _fields_ = [("h", HllItem), ("g", HllGCol * MAX_GROUP_COLS)]


def bind(L):
    """Set the prototypes of the HLL launchers on the loaded libpgx.so; returns (offer, offer_group, narrow).
    offer(items_dev, items_host, nitems, wgs_per_item, stream); offer_group(items_dev, items_host, nitems, ngcols,
    gmul_host, slots, wgs_per_item, stream); narrow(table, slot_list, ngroups, slots, out, stream)."""
    of = L.pgx_launch_hll_offer
    of.restype = C.c_int
    of.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    og = L.pgx_launch_hll_offer_group
    og.restype = C.c_int
    og.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    na = L.pgx_launch_hll_narrow
    na.restype = C.c_int
    na.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    return of, og, na
