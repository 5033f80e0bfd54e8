"""pgx_hll_codes (pinot_amd/csrc/pgx_hll.cpp), the host helper that builds the per-dictId DISTINCTCOUNTHLL code tables,
against the numpy model of tests/hll_ref.py (pinot_amd/hll.py over extended.java_hash_code).  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from pinot_amd import hll as H
from pinot_amd import native as N
from tests import hll_ref as R

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
LONG_MIN = -(1 << 63)

_NP = {"INT": (N.PGX_INT, np.int32), "LONG": (N.PGX_LONG, np.int64), "FLOAT": (N.PGX_FLOAT, np.float32),
       "DOUBLE": (N.PGX_DOUBLE, np.float64)}


def _native(dtype, values):
    L = N.lib()
    n = len(values)
    out = np.full(n + 8, 0xA5A5, np.uint16)  # guard entries past the end
    if dtype == "STRING":
        enc = [v.encode("utf-8") for v in values]
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([len(e) for e in enc])
        blob = np.frombuffer(b"".join(enc) + b"\0", np.uint8).copy()
        N.check(L.pgx_hll_codes(N.PGX_STRING, blob.ctypes.data, offs.ctypes.data, n, out.ctypes.data))
    else:
        code, npt = _NP[dtype]
        a = np.ascontiguousarray(np.asarray(values, dtype=npt))
        N.check(L.pgx_hll_codes(code, a.ctypes.data, None, n, out.ctypes.data))
    assert (out[n:] == 0xA5A5).all()
    return out[:n]


CASES = {
    "INT": [0, 1, -1, INT_MIN, INT_MAX, 12345, -98765],
    "LONG": [0, 1, -1, (1 << 32) + 5, (1 << 40) + 123, (1 << 62), -(1 << 33) - 7, LONG_MIN, (1 << 63) - 1,
             0x0000000100000001],  # halves that cancel
    "FLOAT": [0.25, 0.75, 0.0, -0.0, 1e30, -3.5, 1.0],
    "DOUBLE": [0.25, 0.75, 0.0, -0.0, 1e30, -3.5, 1.0,
               float(np.array([0x4010000040100000], np.uint64).view(np.float64)[0]),   # high half == low half
               float(np.array([0x3FF000003FF00000], np.uint64).view(np.float64)[0])],
    "STRING": ["", "a", "abc", "hello world", "tab\there", "\t", "café", "üö", "€ uro", "中文",
               "x\U0001F600y", "\U00010000"],
}


@pytest.mark.parametrize("dtype", sorted(CASES))
def test_codes_match_the_model(dtype):
    vals = CASES[dtype]
    got = _native(dtype, vals)
    np.testing.assert_array_equal(got, R.codes(dtype, vals))
    rank = got & 0xFF
    assert ((rank >= 1) & (rank <= R.MAX_RANK)).all()


def test_float_halves_and_signed_zero_stay_distinct():
    """floatToIntBits keeps 0.25 / 0.75 and 0.0 / -0.0 apart; a double whose halves cancel hashes to 0 like INT 0."""
    f = _native("FLOAT", [0.25, 0.75, 0.0, -0.0])
    assert len(set(f.tolist())) == 4
    d = _native("DOUBLE", [CASES["DOUBLE"][-2]])
    assert d[0] == _native("INT", [0])[0]


def test_random_ints_give_from_ints_registers():
    rng = np.random.default_rng(1)
    v = rng.integers(INT_MIN, INT_MAX, 100000, dtype=np.int64)
    c = _native("INT", v).astype(np.uint32)
    rank = c & 0xFF
    assert ((rank >= 1) & (rank <= R.MAX_RANK)).all()
    regs = np.zeros(R.REGS, np.uint8)
    np.maximum.at(regs, c >> 8, rank.astype(np.uint8))
    np.testing.assert_array_equal(regs, H.from_ints(v.tolist()))
    np.testing.assert_array_equal(regs, R.offer(np.ones(len(v), bool), np.arange(len(v)), c).astype(np.uint8))


def test_random_longs_doubles_and_strings():
    rng = np.random.default_rng(2)
    longs = rng.integers(LONG_MIN, (1 << 63) - 1, 2000, dtype=np.int64)
    np.testing.assert_array_equal(_native("LONG", longs), R.codes("LONG", longs.tolist()))
    dbl = rng.standard_normal(2000) * 1e6
    np.testing.assert_array_equal(_native("DOUBLE", dbl), R.codes("DOUBLE", dbl.tolist()))
    flt = dbl.astype(np.float32)
    np.testing.assert_array_equal(_native("FLOAT", flt), R.codes("FLOAT", flt.tolist()))
    alphabet = list("abcXYZ 09\t") + ["é", "€", "\U0001F600"]
    strs = ["".join(rng.choice(alphabet, rng.integers(0, 12))) for _ in range(500)]
    np.testing.assert_array_equal(_native("STRING", strs), R.codes("STRING", strs))


def test_bad_arguments():
    L = N.lib()
    out = np.zeros(4, np.uint16)
    a = np.zeros(4, np.int32)
    assert L.pgx_hll_codes(N.PGX_INT, a.ctypes.data, None, -1, out.ctypes.data) == N.PGX_ERR_INVALID_ARG
    assert L.pgx_hll_codes(7, a.ctypes.data, None, 4, out.ctypes.data) == N.PGX_ERR_INVALID_ARG
    assert L.pgx_hll_codes(N.PGX_STRING, a.ctypes.data, None, 1, out.ctypes.data) == N.PGX_ERR_INVALID_ARG
    assert L.pgx_hll_codes(N.PGX_INT, None, None, 4, out.ctypes.data) == N.PGX_ERR_INVALID_ARG
    assert L.pgx_hll_codes(N.PGX_INT, None, None, 0, None) == 0


def test_function_code_and_limits():
    assert N.PGX_DISTINCTCOUNTHLL == 10
    assert N.PGX_HLL_MAX_GROUP_SLOTS == R.MAX_GROUP_SLOTS == 65536
    assert "pgx_result_hll" in N.EXPORTS and "pgx_hll_codes" in N.EXPORTS
    assert C.sizeof(R.HllItem) == 48 and C.sizeof(R.HllGroupItem) == 48 + 16 * 24
