"""Reference model of the FASTHLL fold kernel (pinot_amd/csrc/pgx_fasthll.hip) in plain numpy: the register-wise maximum
of the register-image rows of a presence bitmap row's set bits, per listed row.  The bitmaps are those of
tests/distinct_ref.py.  A helper, not a test: nothing here touches a GPU (tests/test_fasthll_cpu.py checks the model
and the launcher's refusals, tests/test_gpu_fasthll_kernels.py the kernel)."""
import ctypes as C

import numpy as np

from tests.distinct_ref import set_ids, words  # noqa: F401  (re-exported)

REGS = 256
SPLIT_WORDS = 64                # kFoldSplitWords: a row of more bitmap words is shared by several workgroups
SPLIT_CARD = SPLIT_WORDS * 32   # the largest cardinality one workgroup folds alone


def bind(L):
    """Set the prototypes of the fold launcher and its split rule on the loaded libpgx.so; returns (fold, split).
    fold(table, card, image, rows_dev, rows_host, nrows, slots, out, wgs, stream); split(card): workgroups per row."""
    fo = L.pgx_launch_fasthll_fold
    fo.restype = C.c_int
    fo.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int,
                   C.c_void_p]
    sp = L.pgx_fasthll_fold_split
    sp.restype = C.c_int
    sp.argtypes = [C.c_int32]
    return fo, sp


def pack_image(image):
    """[card, 256] uint8 registers as the device image: [card, 64] uint32, register 4l + b in byte b of dword l."""
    a = np.ascontiguousarray(np.asarray(image, np.uint8))
    assert a.ndim == 2 and a.shape[1] == REGS
    return a.view("<u4")


def fold(table, card, image, rows, into=None):
    """[len(rows), 256] uint32: `into` (or zeros) maxed with the image rows of the set bits below card of table row
    rows[r]; a row outside the table folds nothing."""
    table = np.asarray(table, np.uint32).reshape(-1, words(card))
    out = np.zeros((len(rows), REGS), np.uint32) if into is None else np.asarray(into, np.uint32).copy()
    img = np.asarray(image, np.uint8)
    for r, s in enumerate(rows):
        if 0 <= s < len(table):
            ids = set_ids(table[s], card)
            if len(ids):
                out[r] = np.maximum(out[r], img[ids].max(axis=0))
    return out
