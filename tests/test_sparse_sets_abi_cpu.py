"""What the sparse GROUP BY of the set functions adds to the library's surface, checked without a device: the flag and
the constants in include/pgx.h and pinot_amd/native.py, the launchers libpgx.so exports (tests/sel_dir_ref.bind), their
refusals that are decided on the host copy of the arguments before anything touches the device, and the plan maker's
knob (pinot_amd/extended.sparse_sets_flag).  No GPU."""
import ctypes as C
import os
import re

import numpy as np

from pinot_amd import extended as X
from pinot_amd import native as N
from tests import hll_ref as R
from tests import sel_dir_ref as S

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pgx.h")


def test_header_and_python_mirror_agree():
    text = open(HEADER).read()

    def define(name):
        return re.search(r"^#define %s\s+(.+?)\s*(/\*.*)?$" % name, text, re.M).group(1)

    assert define("PGX_X_SPARSE_GROUP_SETS") == "0x10u" and N.PGX_X_SPARSE_GROUP_SETS == 0x10
    assert int(define("PGX_SET_MAX_SPARSE_GROUPS")) == S.MAX_SPARSE_GROUPS == 131072 <= S.NO_SLOT  # every index is below the sentinel
    assert define("PGX_HLL_MAX_TABLE_BYTES") == "(256u << 20)"
    assert define("PGX_ABI_VERSION").split()[0] == "8" and int(define("PGX_HLL_MAX_GROUP_SLOTS")) == R.MAX_GROUP_SLOTS
    flags = [int(v, 16) for v in re.findall(r"^#define PGX_X_\w+\s+(0x[0-9a-f]+)u", text, re.M)]
    assert sorted(flags) == [1, 2, 4, 8, 16]  # the next free bit


def test_launchers_are_exported_and_refuse_on_the_host():
    fn = S.bind(N.lib())
    assert set(fn) == {"build", "find"} | {n[len("pgx_launch_"):] for n in S.SPARSE_LAUNCHERS}
    keys = np.arange(4, dtype=np.uint64)
    p = keys.ctypes.data  # (never dereferenced on the device: every call below is refused first)
    for args in ((None, p, 4, 1, p, p, p, 8), (p, None, 4, 1, p, p, p, 8), (p, p, 4, 1, None, p, p, 8),
                 (p, p, 4, 1, p, p, None, 8), (p, p, 4, 2, p, None, p, 8), (p, p, -1, 1, p, p, p, 8),
                 (p, p, 4, 1, p, p, p, 6), (p, p, 4, 1, p, p, p, 2), (p, p, 4, 3, p, p, p, 8),
                 (p, p, S.MAX_SPARSE_GROUPS + 1, 1, p, p, p, 1 << 18)):
        assert fn["build"](*args, None) == R.INVALID_VALUE, args
    ones = np.array([1, 0xFFFFFFFFFFFFFFFF], np.uint64)
    assert fn["build"](p, ones.ctypes.data, 2, 1, p, None, p, 8, None) == R.INVALID_VALUE
    key = S.fill_key(S.SelSparseKey(), S.layout([300, 300]), 4)
    key.keys = key.state = key.index = key.miss = p
    key.cap = 8
    out = np.zeros(4, np.uint32)
    assert fn["find"](None, 4, C.addressof(key), out.ctypes.data, None) == R.INVALID_VALUE
    assert fn["find"](p, 4, None, out.ctypes.data, None) == R.INVALID_VALUE
    item = (C.c_uint8 * 4096)()  # an item of any of the six kinds, all zero: no selection words, no column
    for name in S.SPARSE_LAUNCHERS:
        launch = fn[name[len("pgx_launch_"):]]
        assert launch(C.addressof(item), C.addressof(item), 1, None, 1, None) == R.INVALID_VALUE
        for field, bad in (("groups", 0), ("groups", S.MAX_SPARSE_GROUPS + 1), ("W", 3), ("cap", 6), ("cap", 2),
                           ("ngcols", 0), ("ngcols", 17), ("keys", None)):
            k = S.SelSparseKey.from_buffer_copy(key)
            setattr(k, field, bad)
            assert launch(C.addressof(item), C.addressof(item), 1, C.addressof(k), 1, None) == R.INVALID_VALUE
        # a good key: refused for the grid and for the (empty) item, still without a launch
        assert launch(C.addressof(item), C.addressof(item), 1, C.addressof(key), 0, None) == R.INVALID_VALUE
        assert launch(C.addressof(item), C.addressof(item), 1, C.addressof(key), 1, None) == R.INVALID_VALUE


def test_plan_maker_knob(monkeypatch):
    monkeypatch.delenv("PGX_SPARSE_SETS_NATIVE", raising=False)
    assert X.sparse_sets_flag() == 0
    monkeypatch.setenv("PGX_SPARSE_SETS_NATIVE", "0")
    assert X.sparse_sets_flag() == 0
    monkeypatch.setenv("PGX_SPARSE_SETS_NATIVE", "1")
    assert X.sparse_sets_flag() == N.PGX_X_SPARSE_GROUP_SETS
