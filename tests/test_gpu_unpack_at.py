"""Direct test of the query kernels' single-row decode at a run-time position (pgx_jit_device.h pgx_unpack_at and its
frac twin pgx_unpack_frac_at) against the whole-lane unpack (pgx_unpack / pgx_unpack_frac), through the launcher
pgx_launch_unpack_at_check (pgx_unpack_check.hip): for every bit width 1..32, every legal rows-per-lane count and every
row position, on random words.  The whole-lane unpack itself is checked against a numpy decode of the MSB-first,
big-endian bit stream, so both sides stand on the forward-index format and not on each other."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LANES = 300  # more than one 256-thread block, not a multiple of the wave


@pytest.fixture(scope="module")
def dev():
    import torch
    from pinot_amd import native as N
    f = N.lib().pgx_launch_unpack_at_check
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    d = torch.device("cuda:0")
    return torch, d, f, C.c_void_p(torch.cuda.current_stream(d).cuda_stream)


def _decode(words, bits, nrows):
    """Rows of a bits-wide forward index held in little-endian-loaded u32 words of a big-endian bit stream."""
    by = words.astype("<u4").view(np.uint8)
    bs = np.unpackbits(by)[:nrows * bits].reshape(nrows, bits).astype(np.uint64)
    return (bs << np.arange(bits - 1, -1, -1, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def _run(dev, bits, R, frac, rng):
    torch, d, f, stream = dev
    nrows = LANES * R
    nwords = (nrows * bits + 31) // 32 + 2
    words = rng.integers(0, 1 << 32, nwords, dtype=np.uint64).astype(np.uint32)
    js = rng.permutation(R).astype(np.uint32)  # every position once, in a random order
    t_w = torch.from_numpy(words.view(np.int32).copy()).to(d)
    t_j = torch.from_numpy(js.view(np.int32).copy()).to(d)
    t_at = torch.full((nrows + 64,), -1, dtype=torch.int32, device=d)
    t_ref = torch.full((nrows + 64,), -1, dtype=torch.int32, device=d)
    rc = f(bits, R, int(frac), t_w.data_ptr(), LANES, t_j.data_ptr(), t_at.data_ptr(), t_ref.data_ptr(), stream)
    assert rc == 0, rc
    torch.cuda.synchronize(d)
    at = t_at.cpu().numpy().view(np.uint32)
    ref = t_ref.cpu().numpy().view(np.uint32)
    assert (at[nrows:] == 0xFFFFFFFF).all() and (ref[nrows:] == 0xFFFFFFFF).all()  # nothing past the last lane
    exp = _decode(words, bits, nrows).reshape(LANES, R)
    assert np.array_equal(ref[:nrows].reshape(LANES, R), exp)
    assert np.array_equal(at[:nrows].reshape(LANES, R), exp[:, js])


@pytest.mark.parametrize("R", [8, 16, 32])
def test_unpack_at_equals_unpack_every_width_and_position(dev, R):
    rng = np.random.default_rng(100 + R)
    ran = 0
    for bits in range(1, 33):
        if (R * bits) % 32:
            continue  # not a legal whole-dword shape: the frac form reads it (below)
        _run(dev, bits, R, False, rng)
        ran += 1
    assert ran == {8: 8, 16: 16, 32: 32}[R]


@pytest.mark.parametrize("R", [8, 16, 32])
def test_unpack_frac_at_equals_unpack_frac_every_width_and_position(dev, R):
    """Lanes whose rows start mid-dword (R * bits not a multiple of 32), and the aligned widths through the same form."""
    rng = np.random.default_rng(200 + R)
    for bits in range(1, 32):
        _run(dev, bits, R, True, rng)


def test_launcher_rejects_what_it_cannot_run(dev):
    torch, d, f, stream = dev
    t = torch.zeros(64, dtype=torch.int32, device=d)
    p = t.data_ptr()
    assert f(10, 8, 0, p, 1, p, p, p, stream) != 0   # 80 bits per lane: not whole dwords
    assert f(32, 8, 1, p, 1, p, p, p, stream) != 0   # 32-bit rows are never frac
    assert f(0, 8, 0, p, 1, p, p, p, stream) != 0
    assert f(8, 12, 0, p, 1, p, p, p, stream) != 0
