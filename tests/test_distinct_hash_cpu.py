"""pgx_java_hash_codes (pinot_amd/csrc/pgx_hll.cpp over pgx_hash.h), the host helper that gives the per-value Java
hashCode the DISTINCTCOUNT hash tables hold, against extended.java_hash_code; and the numpy model of the presence
bitmaps (tests/distinct_ref.py) against Python sets.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from pinot_amd import extended as X
from pinot_amd import native as N
from tests import distinct_ref as D

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1
GUARD = np.int32(-1515870811)

_NP = {"INT": (N.PGX_INT, np.int32), "LONG": (N.PGX_LONG, np.int64), "FLOAT": (N.PGX_FLOAT, np.float32),
       "DOUBLE": (N.PGX_DOUBLE, np.float64)}


def _native(dtype, values):
    L = N.lib()
    n = len(values)
    out = np.full(n + 8, GUARD, np.int32)  # guard entries past the end
    if dtype == "STRING":
        enc = [v.encode("utf-8") for v in values]
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([len(e) for e in enc])
        blob = np.frombuffer(b"".join(enc) + b"\0", np.uint8).copy()
        N.check(L.pgx_java_hash_codes(N.PGX_STRING, blob.ctypes.data, offs.ctypes.data, n, out.ctypes.data))
    else:
        code, npt = _NP[dtype]
        a = np.ascontiguousarray(np.asarray(values, dtype=npt))
        N.check(L.pgx_java_hash_codes(code, a.ctypes.data, None, n, out.ctypes.data))
    assert (out[n:] == GUARD).all()
    return out[:n]


CASES = {
    "INT": [0, 1, -1, INT_MIN, INT_MAX, 12345, -98765],
    "LONG": [0, 0x0000000100000001, 1, -1, LONG_MIN, LONG_MAX, (1 << 32) + 5, -(1 << 33) - 7, 1 << 62],
    "FLOAT": [0.25, 0.75, 0.0, -0.0, float("nan"), float("inf"), -3.5, 1e30],
    "DOUBLE": [0.25, 0.75, 0.0, -0.0, float("nan"), float("-inf"), -3.5, 1e300,
               float(np.array([0x4010000040100000], np.uint64).view(np.float64)[0])],  # high half == low half
    "STRING": ["", "a", "abc", "tab\there", "\t", "été", "中", "中文", "x\U0001F600y", "\U00010000"],
}


@pytest.mark.parametrize("dtype", sorted(CASES))
def test_hash_codes_match_java_hash_code(dtype):
    vals = CASES[dtype]
    got = _native(dtype, vals)
    assert got.tolist() == [X.java_hash_code(dtype, v) for v in vals]


def test_collisions_and_values_that_stay_apart():
    """LONG 0 and 0x0000000100000001 both hash to 0 (they count once); FLOAT 0.25 / 0.75 and 0.0 / -0.0 stay distinct;
    every NaN is the canonical one."""
    h = _native("LONG", [0, 0x0000000100000001])
    assert h[0] == h[1] == 0
    assert len(set(_native("FLOAT", [0.25, 0.75, 0.0, -0.0]).tolist())) == 4
    assert len(set(_native("DOUBLE", [0.25, 0.75, 0.0, -0.0]).tolist())) == 4
    other_nan = np.array([0x7FC01234], np.uint32).view(np.float32)
    assert _native("FLOAT", other_nan)[0] == 0x7FC00000 == _native("FLOAT", [float("nan")])[0]
    other_dnan = np.array([0x7FF8000000000123], np.uint64).view(np.float64)
    assert _native("DOUBLE", other_dnan)[0] == X.java_hash_code("DOUBLE", float("nan"))


def test_random_values():
    rng = np.random.default_rng(2)
    longs = rng.integers(LONG_MIN, LONG_MAX, 2000, dtype=np.int64)
    assert _native("LONG", longs).tolist() == [X.java_hash_code("LONG", int(v)) for v in longs]
    dbl = rng.standard_normal(2000) * 1e6
    assert _native("DOUBLE", dbl).tolist() == [X.java_hash_code("DOUBLE", v) for v in dbl]
    flt = dbl.astype(np.float32)
    assert _native("FLOAT", flt).tolist() == [X.java_hash_code("FLOAT", v) for v in flt]
    alphabet = list("abcXYZ 09\t") + ["é", "€", "中", "\U0001F600"]
    strs = ["".join(rng.choice(alphabet, rng.integers(0, 12))) for _ in range(500)]
    assert _native("STRING", strs).tolist() == [X.java_hash_code("STRING", s) for s in strs]


def test_bad_arguments():
    L = N.lib()
    out = np.full(4, GUARD, np.int32)
    a = np.zeros(4, np.int32)
    assert L.pgx_java_hash_codes(N.PGX_INT, a.ctypes.data, None, -1, out.ctypes.data) == N.PGX_ERR_INVALID_ARG
    assert L.pgx_java_hash_codes(7, a.ctypes.data, None, 4, out.ctypes.data) == N.PGX_ERR_INVALID_ARG
    assert L.pgx_java_hash_codes(-1, a.ctypes.data, None, 4, out.ctypes.data) == N.PGX_ERR_INVALID_ARG
    assert L.pgx_java_hash_codes(N.PGX_STRING, a.ctypes.data, None, 1, out.ctypes.data) == N.PGX_ERR_INVALID_ARG
    assert L.pgx_java_hash_codes(N.PGX_INT, None, None, 4, out.ctypes.data) == N.PGX_ERR_INVALID_ARG
    assert L.pgx_java_hash_codes(N.PGX_INT, a.ctypes.data, None, 4, None) == N.PGX_ERR_INVALID_ARG
    offs = np.array([0, 3, 2], np.int32)  # descending
    blob = np.frombuffer(b"abcd", np.uint8).copy()
    assert L.pgx_java_hash_codes(N.PGX_STRING, blob.ctypes.data, offs.ctypes.data, 2,
                                 out.ctypes.data) == N.PGX_ERR_INVALID_ARG
    assert (out[1:] == GUARD).all()
    assert L.pgx_java_hash_codes(N.PGX_INT, None, None, 0, None) == 0


def test_function_codes_limits_and_item_layouts():
    from pinot_amd import engine as E
    assert E._FN["distinctcount"] == N.PGX_DISTINCTCOUNT == 12
    assert E._FN["distinctcountmv"] == N.PGX_DISTINCTCOUNTMV == 13
    assert N.PGX_DISTINCT_MAX_TABLE_BYTES == 256 << 20
    for name in ("pgx_result_distinct", "pgx_result_distinct_counts", "pgx_java_hash_codes"):
        assert name in N.EXPORTS
    assert C.sizeof(D.DistinctItem) == 40 and C.sizeof(D.DistinctMvItem) == 56


def test_bitmap_model_is_the_set_of_selected_ids():
    rng = np.random.default_rng(3)
    for card in (1, 33, 1000):
        n = 5000
        ids = rng.integers(0, card + 5, n)  # some at or past card: they mark nothing
        sel = rng.random(n) < 0.3
        pre = rng.integers(0, 1 << 32, D.words(card), dtype=np.uint64).astype(np.uint32)
        bm = D.mark(sel, ids, card, pre)
        want = set(ids[sel & (ids < card)].tolist()) | set(D.set_ids(pre, card).tolist())
        assert set(D.set_ids(bm, card).tolist()) == want
        assert ((bm & pre) == pre).all()
        slot = rng.integers(-1, 5, n)
        g = D.mark_group(sel, ids, card, slot, 4)
        for s in range(4):
            assert set(D.set_ids(g[s], card).tolist()) == set(ids[sel & (ids < card) & (slot == s)].tolist())
    counts = rng.integers(0, 4, 100)
    vids = rng.integers(0, 50, int(counts.sum()))
    dsel = rng.random(100) < 0.5
    got = set(D.set_ids(D.mark_mv(dsel, counts, vids, 50), 50).tolist())
    st = np.concatenate([[0], np.cumsum(counts)])
    assert got == {int(v) for d in np.flatnonzero(dsel) for v in vids[st[d]:st[d + 1]]}
