"""Reference model of the selection ORDER BY kernels (pinot_amd/csrc/pgx_select.hip) in plain numpy: the order key, the
(key, docId) ranking, the fixed-bit forward index the kernels read, and the descriptor structs and ctypes prototypes of
the three launchers libpgx.so exports.  A helper, not a test: nothing here touches a GPU (tests/test_select_cpu.py
checks the model, tests/test_gpu_select_kernels.py the kernels against it)."""
import ctypes as C

import numpy as np

MAX_ROWS = 2048          # PGX_SEL_MAX_ROWS
MAX_ORDER_COLS = 8       # kSelMaxOrderCols
TILE_ROWS = 8192         # kTileRows: forward indexes are padded to whole tiles
INVALID_VALUE = 1        # hipErrorInvalidValue


def key_bits(card):
    """Bits an order column takes in the key: max(1, ceil(log2 card))."""
    b = 1
    while (1 << b) < card:
        b += 1
    return b


def order_keys(cols):
    """cols: [(dictIds, cardinality, ascending[, kbits])] in ORDER BY order -> (uint64 key per doc, total bits)."""
    key = None
    total = 0
    for col in cols:
        ids, card, asc = col[0], int(col[1]), col[2]
        kb = col[3] if len(col) > 3 else key_bits(card)
        v = np.asarray(ids).astype(np.uint64)
        if not asc:
            v = np.uint64(card - 1) - v
        key = v if key is None else ((key << np.uint64(kb)) | v)
        total += kb
    assert total <= 64
    return key, total


def top_k(selected, cols, k):
    """The model: docIds of the k best selected docs under (key, docId) ascending, best first.
    selected: bool per doc."""
    key, _ = order_keys(cols)
    docs = np.flatnonzero(np.asarray(selected, dtype=bool))
    order = np.lexsort((docs, key[docs]))  # last key is the primary one
    return docs[order][:k].astype(np.int64)


def pack_fwd(ids, bits, num_docs=None):
    """<col>.sv.unsorted.fwd as staged: MSB-first big-endian, values back to back, padded with dictId 0 to whole
    8192-row tiles plus 64 bytes.  Returns uint8."""
    ids = np.asarray(ids, dtype=np.uint64)
    n = len(ids) if num_docs is None else num_docs
    tiles = max(1, -(-n // TILE_ROWS))
    rows = tiles * TILE_ROWS
    full = np.zeros(rows, np.uint64)
    full[:len(ids)] = ids
    shifts = np.arange(bits - 1, -1, -1, dtype=np.uint64)
    bitmat = ((full[:, None] >> shifts[None, :]) & np.uint64(1)).astype(np.uint8)
    packed = np.packbits(bitmat.reshape(-1))
    return np.concatenate([packed, np.zeros(64, np.uint8)])


def pack_mask(selected, ones_past_end=True):
    """Selection bits as the query kernels write them: bit (d & 31) of little-endian word d >> 5, plus one spare word.
    With ones_past_end the bits past num_docs and the spare word are all ones (the kernels must ignore them)."""
    sel = np.asarray(selected, dtype=bool)
    n = len(sel)
    words = (n + 31) // 32
    bits = np.ones((words + 1) * 32, bool) if ones_past_end else np.zeros((words + 1) * 32, bool)
    bits[:n] = sel
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).copy()


class SelCol(C.Structure):
    _fields_ = [("fwd", C.c_void_p), ("bits", C.c_int32), ("kbits", C.c_int32), ("card", C.c_uint32),
                ("desc", C.c_int32)]


class SelItem(C.Structure):
    _fields_ = [("sel", C.c_void_p), ("num_docs", C.c_int32), ("ncols", C.c_int32), ("c", SelCol * MAX_ORDER_COLS)]


class SelGatherCol(C.Structure):
    _fields_ = [("fwd", C.c_void_p), ("bits", C.c_int32), ("pad", C.c_int32)]


def buffer_entries(k):
    """LDS candidate entries of a workgroup (sel_buffer_entries)."""
    p = 1
    while p < k:
        p <<= 1
    return max(512, 2 * p)


def bind(L):
    """Set the prototypes of the selection launchers on the loaded libpgx.so; returns (topk, merge, gather)."""
    tk = L.pgx_launch_select_topk
    tk.restype = C.c_int
    tk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    mg = L.pgx_launch_select_merge
    mg.restype = C.c_int
    mg.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ga = L.pgx_launch_select_gather
    ga.restype = C.c_int
    ga.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return tk, mg, ga
