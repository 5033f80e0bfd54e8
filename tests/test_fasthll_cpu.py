"""pgx_fasthll_registers (pinot_amd/csrc/pgx_fasthll.cpp), the host decode that fills the FASTHLL register images,
against pinot_amd/hll.py from_string; the header and its Python mirror; and the fold launcher's refusals of bad host
arguments, which need no device: nothing is launched.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pinot_amd import hll as HLL
from pinot_amd import native as N
from tests import fasthll_ref as F

GUARD = np.uint8(0xA5)
HIP_INVALID_VALUE = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _native(values, expect=0):
    """(registers [n, 256], bad_index) of pgx_fasthll_registers over `values` (str); guard bytes past the end."""
    n = len(values)
    enc = [v.encode("utf-8", "surrogatepass") for v in values]
    offs = np.zeros(n + 1, np.int32)
    offs[1:] = np.cumsum([len(e) for e in enc])
    blob = np.frombuffer(b"".join(enc) + b"\0", np.uint8).copy()
    out = np.full(n * 256 + 64, GUARD, np.uint8)
    bad = C.c_int64(-7)
    st = N.lib().pgx_fasthll_registers(blob.ctypes.data, offs.ctypes.data, n, out.ctypes.data, C.byref(bad))
    assert st == expect
    assert (out[n * 256:] == GUARD).all()
    return out[:n * 256].reshape(n, 256), bad.value


def test_registers_match_from_string():
    rng = np.random.default_rng(5)
    regs = [rng.integers(0, 32, 256).astype(np.uint8) for _ in range(40)]
    regs += [HLL.from_ints(rng.integers(0, 1 << 30, int(rng.integers(1, 3000))).tolist()) for _ in range(40)]
    regs += [HLL.empty(), np.full(256, 31, np.uint8)]
    strs = [HLL.to_string(r) for r in regs]
    assert all(len(s) == 180 for s in strs)
    # bytes of 127 .. 255 and -128 .. -2 give chars of 128 and more: two UTF-8 bytes each
    assert any(len(s.encode("utf-8")) > 180 for s in strs) and len(strs[-1].encode("utf-8")) > 180
    got, bad = _native(strs)
    assert bad == -1
    for g, s, r in zip(got, strs, regs):
        assert np.array_equal(g, HLL.from_string(s)) and np.array_equal(g, r)


def test_malformed_values_are_refused_with_their_index():
    good = HLL.to_string(HLL.from_ints(range(100)))
    b = bytearray(HLL.to_bytes(HLL.from_ints(range(50))))

    def as_string(raw):
        return "".join(chr(((x - 256) if x > 127 else x) + 129) for x in raw)
    wrong_log2m = bytearray(b)
    wrong_log2m[3] = 9
    wrong_count = bytearray(b)
    wrong_count[7] = 168
    for k, badv in enumerate((as_string(wrong_log2m), as_string(wrong_count), good[:-1], good + good[:1], "")):
        for pos in (0, 2):
            vals = [good] * pos + [badv] + [good]
            got, bad = _native(vals, expect=N.PGX_ERR_UNSUPPORTED)
            assert bad == pos, (k, pos)
            assert all(np.array_equal(got[i], HLL.from_string(good)) for i in range(pos))  # rows before it are written
    # a log2m-9 estimator as stream-lib writes it (more bytes): the reference cannot merge it either
    with pytest.raises(ValueError):
        HLL.from_string(as_string(wrong_log2m))


def test_bad_arguments():
    L = N.lib()
    out = np.zeros(256, np.uint8)
    s = HLL.to_string(HLL.empty()).encode("utf-8")
    blob = np.frombuffer(s, np.uint8).copy()
    offs = np.array([0, len(s)], np.int32)
    assert L.pgx_fasthll_registers(blob.ctypes.data, offs.ctypes.data, 1, out.ctypes.data, None) == 0  # NULL bad_index
    assert L.pgx_fasthll_registers(blob.ctypes.data, offs.ctypes.data, -1, out.ctypes.data, None) == N.PGX_ERR_INVALID_ARG
    assert L.pgx_fasthll_registers(None, offs.ctypes.data, 1, out.ctypes.data, None) == N.PGX_ERR_INVALID_ARG
    assert L.pgx_fasthll_registers(blob.ctypes.data, None, 1, out.ctypes.data, None) == N.PGX_ERR_INVALID_ARG
    assert L.pgx_fasthll_registers(blob.ctypes.data, offs.ctypes.data, 1, None, None) == N.PGX_ERR_INVALID_ARG
    desc = np.array([len(s), 0], np.int32)
    assert L.pgx_fasthll_registers(blob.ctypes.data, desc.ctypes.data, 1, out.ctypes.data, None) == N.PGX_ERR_INVALID_ARG
    assert L.pgx_fasthll_registers(None, None, 0, None, None) == 0


def test_header_and_python_mirror_agree():
    from pinot_amd import engine as E
    from pinot_amd import extended as X
    h = open(os.path.join(ROOT, "include", "pgx.h")).read()
    assert re.search(r"PGX_FASTHLL = 16\b", h) and N.PGX_FASTHLL == 16 == E._FN["fasthll"]
    assert re.search(r"#define PGX_ABI_VERSION 8\b", h)
    assert re.search(r"#define PGX_FASTHLL_MAX_IMAGE_BYTES \(256u << 20\)", h) and N.PGX_FASTHLL_MAX_IMAGE_BYTES == 256 << 20
    assert "pgx_fasthll_registers" in N.EXPORTS and "pgx_fasthll_registers(" in h
    for name in ("pgx_launch_fasthll_fold", "pgx_fasthll_fold_split"):  # exported for the runner and the tests
        assert hasattr(N.lib(), name)
    assert "fasthll" in E._HLL_FNS and X._NATIVE_FASTHLL_FNS == ("fasthll",)


def test_model_folds_the_set_bits():
    rng = np.random.default_rng(6)
    card = 70
    image = rng.integers(0, 32, (card, 256)).astype(np.uint8)
    table = np.zeros((3, F.words(card)), np.uint32)
    for d in (0, 33, 69):
        table[1, d >> 5] |= np.uint32(1 << (d & 31))
    table[2, 2] = 0xFFFFFFFF  # dictIds 64 .. 95: those at and past card fold nothing
    out = F.fold(table, card, image, [1, 2, 0, 1], None)
    assert np.array_equal(out[0], np.maximum.reduce(image[[0, 33, 69]]).astype(np.uint32))
    assert np.array_equal(out[1], np.maximum.reduce(image[64:70]).astype(np.uint32))
    assert not out[2].any() and np.array_equal(out[3], out[0])
    pre = np.full((4, 256), 9, np.uint32)
    assert np.array_equal(F.fold(table, card, image, [1, 2, 0, 1], pre), np.maximum(out, 9))
    packed = F.pack_image(image)
    assert packed.dtype == np.uint32 and packed.shape == (card, 64)
    assert packed[5, 3] == int(image[5, 12]) | int(image[5, 13]) << 8 | int(image[5, 14]) << 16 | int(image[5, 15]) << 24


def test_split_rule():
    _, split = F.bind(N.lib())
    assert split(0) == 0 and split(-3) == 0
    assert split(1) == 1 and split(F.SPLIT_CARD) == 1
    assert split(F.SPLIT_CARD + 1) == 2
    assert split(64 * F.SPLIT_CARD + 1) == 64 == split((1 << 31) - 1)


def test_launcher_refuses_bad_host_arguments_without_a_device():
    """Every refusal comes before the launch, so the (fake, never dereferenced) device pointers are never used."""
    fold, _ = F.bind(N.lib())
    P = 0x1000  # stands for a device pointer
    rows = np.array([0, 3, 2], np.int64)
    ok = dict(table=P, card=40, image=P, rows=P, check=rows.ctypes.data, nrows=3, slots=4, out=P, wgs=2)

    def call(**kw):
        a = dict(ok, **kw)
        return fold(a["table"], a["card"], a["image"], a["rows"], a["check"], a["nrows"], a["slots"], a["out"],
                    a["wgs"], None)
    for name in ("table", "image", "rows", "check", "out"):
        assert call(**{name: None}) == HIP_INVALID_VALUE, name
    for kw in (dict(nrows=-1), dict(card=0), dict(card=-5), dict(wgs=0), dict(wgs=-1), dict(wgs=65536), dict(slots=0),
               dict(slots=-1), dict(slots=65537), dict(nrows=65537, slots=65536), dict(slots=3), dict(slots=2)):
        assert call(**kw) == HIP_INVALID_VALUE, kw
    neg = np.array([0, -1, 2], np.int64)
    assert call(check=neg.ctypes.data) == HIP_INVALID_VALUE
    assert call(nrows=0) == 0  # nothing to do: nothing launched
