"""The wave kernel's wide container reader (pgx_roaring_program_wave: array containers as aligned 16-byte granules,
bitmap containers as 16 bytes per lane from any 2-byte alignment) against the numpy model of tests/roaring_ref.py and
against the two-byte reader it replaced (PGX_DEBUG=rnarrow).  pgx_launch_roaring_program_wave is launched directly on
sentinel-filled masks with guard words behind them; every comparison is exact.

Every case runs four ways: the wide reader with the launcher's own parts (these launches hold few programs, so every
wave takes one chunk and starts by a cursor seek), the wide reader with one wave walking the whole segment
(PGX_DEBUG=rparts=1: the cursor's advance), and the same two with the two-byte reader.

Alignment is set by a filler bitmap of 1 to 8 docs in front (its blob is 16 + 2 k bytes), as ODD does in
test_gpu_roaring_kernels.py; every case asserts the offsets it is about.  Every segment a test launches is kept alive
(lru_cache): the device copies are cached by the segment object's id.  A roaring blob starts with at least 16 bytes
of header, so containers of two different bitmaps are never less than 16 bytes apart: what shares a granule with a
bitmap's last container is the next bitmap's header, and with its first container its own offset table."""
import functools

import numpy as np
import pytest

from tests import roaring_ref as R
from tests.roaring_ref import AND, NOT, OR
from tests.test_gpu_roaring_kernels import _Descs, _RK

pytestmark = pytest.mark.gpu

MODES = (None, "rparts=1", "rnarrow", "rnarrow,rparts=1")


@pytest.fixture(scope="module")
def rk():
    return _RK()


def _in_chunk(rng, num_docs, c, k):
    lo, hi = c << 16, min(num_docs, (c + 1) << 16)
    return lo + rng.choice(hi - lo, k, replace=False)


def _docs(rng, num_docs, per_chunk):
    return np.concatenate([_in_chunk(rng, num_docs, c, k) for c, k in per_chunk.items()])


def _shifted(num_docs, bitmaps, which, cont, want, mod=16):
    """A segment of a filler bitmap and `bitmaps`, the filler sized so that container `cont` of bitmaps[which] starts
    at `want` modulo `mod`.  Bitmap i of `bitmaps` is bitmap i + 1 of the segment."""
    for k in range(1, 9):
        seg = R.Seg(num_docs, [np.arange(k)] + list(bitmaps))
        if seg.containers(which + 1)[cont][2] % mod == want:
            return seg
    raise AssertionError("no filler gives offset %d modulo %d" % (want, mod))


def _launch(rk, progs, nslots):
    segs = [s for s, _ in progs]
    buf, offs = rk.masks(segs)
    descs = _Descs(rk)
    arr = (R.JRProg * len(progs))()
    for r, off, (seg, prog) in zip(arr, offs, progs):
        assert len(prog) <= R.MAX_RPROG
        r.mask, r.nchunks, r.num_docs, r.nops = buf.data_ptr() + 4 * off, seg.nchunks, seg.num_docs, len(prog)
        nl = 0
        for i, t in enumerate(prog):
            if R.is_leaf(t):
                r.op[i], r.arg[i] = R.LEAF, descs.of(seg, t) if len(t) else -1
                if nl < R.MAX_RLEAVES:
                    r.ldesc[nl] = r.arg[i]
                nl += 1
            else:
                r.op[i], r.arg[i] = t, 0
    ddev, pdev = descs.dev(), rk.up(np.frombuffer(bytes(arr), np.uint8))
    maxchunks = max(s.nchunks for s in segs)
    assert rk.wave(pdev.data_ptr(), ddev.data_ptr(), len(progs), maxchunks, nslots, rk.stream) == 0
    return [m.copy() for m in rk.back(buf, offs, segs)]


def _check(rk, monkeypatch, progs, nslots=None, modes=MODES):
    """Every mode against the model; the wide reader's masks against the two-byte reader's."""
    if nslots is None:
        nslots = max(R.wave_slots(p) for _, p in progs)
    assert all(R.wave_slots(p) <= nslots <= 3 for _, p in progs)
    assert all(sum(len(t) for t in p if R.is_leaf(t)) <= 64 for _, p in progs)
    want = [R.evaluate(s, p) for s, p in progs]
    got = {}
    for mode in modes:
        if mode:
            monkeypatch.setenv("PGX_DEBUG", mode)
        else:
            monkeypatch.delenv("PGX_DEBUG", raising=False)
        got[mode] = _launch(rk, progs, nslots)
        for g, w, (_, p) in zip(got[mode], want, progs):
            np.testing.assert_array_equal(g, w, err_msg="%s %r" % (mode, p))
    for mode in modes[1:]:  # (the two readers against each other, and the two walks)
        for a, b in zip(got[modes[0]], got[mode]):
            np.testing.assert_array_equal(a, b)


THREE = 2 * 65536 + 40001  # three chunks, the last ragged (no multiple of 32)


@functools.lru_cache(None)
def _start_seg(want):
    rng = np.random.default_rng(100 + want)
    t = _docs(rng, THREE, {0: 100, 1: 100, 2: 100})
    other = _docs(rng, THREE, {0: 50, 1: 3000, 2: 9})
    seg = _shifted(THREE, [t, other], 0, 0, want)
    assert seg.containers(1)[0][2] % 16 == want
    return seg


@pytest.mark.parametrize("want", range(0, 16, 2))
def test_array_container_starts_at_each_position_of_a_granule(rk, monkeypatch, want):
    """The first container starts `want` bytes into a granule; the next two follow at + 200 and + 400 bytes (8 and 0
    more modulo 16).  Alone, ORed with another bitmap, and cleared out of it."""
    seg = _start_seg(want)
    assert [o % 16 for _, _, o in seg.containers(1)] == [want, (want + 8) % 16, want]
    _check(rk, monkeypatch, [(seg, [[1]]), (seg, [[2], [1], OR]), (seg, [[2], [1], NOT, AND])])


@functools.lru_cache(None)
def _end_seg(e):
    rng = np.random.default_rng(200 + e)
    card = 16 + (e // 2 if e else 8)  # 17 .. 24 elements: the container ends e bytes into a granule
    t = _docs(rng, THREE, {0: card, 2: card})
    seg = _shifted(THREE, [t, _docs(rng, THREE, {0: 700, 1: 5, 2: 33})], 0, 0, 0)
    k, c, o = seg.containers(1)[0]
    assert (k, o % 16, (o + 2 * c) % 16) == (0, 0, e)
    return seg


@pytest.mark.parametrize("e", range(0, 16, 2))
def test_array_container_ends_at_each_position_of_a_granule(rk, monkeypatch, e):
    seg = _end_seg(e)
    _check(rk, monkeypatch, [(seg, [[1]]), (seg, [[1, 2]]), (seg, [[2], [1], NOT, AND])])


CARDS = (1, 2, 7, 8, 9, 4095, 4096)


@functools.lru_cache(None)
def _card_seg():
    rng = np.random.default_rng(300)
    bm = [_docs(rng, THREE, {0: c, 1: CARDS[(i + 3) % len(CARDS)], 2: c}) for i, c in enumerate(CARDS)]
    seg = R.Seg(THREE, bm + [_docs(rng, THREE, {0: 20000, 1: 20000, 2: 9000})])
    assert [seg.containers(i)[0][1] for i in range(len(CARDS))] == list(CARDS)
    return seg


def test_array_container_cardinalities(rk, monkeypatch):
    """1, 2, 7, 8, 9, 4095 and 4096 elements: each alone, all in one leaf, and each cleared out of a dense operand."""
    seg = _card_seg()
    n = len(CARDS)
    progs = [(seg, [[i]]) for i in range(n)] + [(seg, [list(range(n))])]
    progs += [(seg, [[n], [i], NOT, AND]) for i in range(n)]
    _check(rk, monkeypatch, progs)


@functools.lru_cache(None)
def _shared_seg():
    rng = np.random.default_rng(400)
    a = _docs(rng, THREE, {0: 101, 1: 77, 2: 203})   # 202, 154 and 406 bytes: every boundary inside a granule
    b = _docs(rng, THREE, {2: 45})
    return _shifted(THREE, [a, b], 0, 0, 4)


def test_consecutive_containers_of_one_bitmap_share_a_granule(rk, monkeypatch):
    """Chunk c's container ends and chunk c + 1's starts inside one granule: no element of c + 1 in c's mask (the
    model has none) and none lost, whether one wave walks both chunks or each chunk has its own wave."""
    seg = _shared_seg()
    cs = seg.containers(1)
    for (_, c0, o0), (_, _, o1) in zip(cs, cs[1:]):
        assert o1 == o0 + 2 * c0 and o1 % 16 != 0
    _check(rk, monkeypatch, [(seg, [[1]]), (seg, [[2], [1], OR]), (seg, [[2], NOT, [1], NOT, AND])])


def test_neighbouring_bitmaps_in_one_leaf_and_in_two(rk, monkeypatch):
    """Bitmap 2's header follows bitmap 1's last container in the same granule, and bitmap 2's only container starts
    16 bytes after that container's end, neither on a granule boundary."""
    seg = _shared_seg()
    last, nxt = seg.containers(1)[-1], seg.containers(2)[0]
    assert (last[2] + 2 * last[1]) % 16 != 0 and seg.offs[2] == last[2] + 2 * last[1]
    assert nxt[2] % 16 != 0
    _check(rk, monkeypatch, [(seg, [[1, 2]]), (seg, [[1], [2], AND]), (seg, [[1], [2], NOT, AND])])


@functools.lru_cache(None)
def _bitmap_seg(want):
    rng = np.random.default_rng(500 + want)
    full = np.arange(65536, 2 * 65536)
    t = np.concatenate([_in_chunk(rng, THREE, 0, 4097), full, _in_chunk(rng, THREE, 2, 300)])
    dense = _docs(rng, THREE, {0: 30000, 1: 40000, 2: 20000})
    seg = _shifted(THREE, [t, dense, _docs(rng, THREE, {0: 64, 1: 64, 2: 64})], 0, 0, want)
    assert [(c, o % 16) for _, c, o in seg.containers(1)[:2]] == [(4097, want), (65536, want)]
    return seg


@pytest.mark.parametrize("want", range(0, 16, 2))
def test_bitmap_containers_at_every_alignment(rk, monkeypatch, want):
    """The smallest bitmap container (4097) and a full one, `want` bytes into a granule: ORed (phase 0), alone and
    beside array and bitmap containers of other bitmaps, and cleared (phase 1) out of a dense operand."""
    seg = _bitmap_seg(want)
    _check(rk, monkeypatch, [(seg, [[1]]), (seg, [[3, 1, 2]]), (seg, [[2, 3], [1], NOT, AND]),
                             (seg, [[3], [2], OR, [1], NOT, AND])])


@functools.lru_cache(None)
def _file_end_seg(kind, want, mod):
    """The file ends with the last bitmap's last container: an array container or a bitmap container."""
    rng = np.random.default_rng(600 + want + mod)
    two = 65536 + 5000
    first = _docs(rng, two, {0: 300, 1: 20})
    last = _docs(rng, two, {0: 40, 1: 13} if kind == "array" else {0: 4, 1: 4500})
    for k in range(1, 9):
        seg = R.Seg(two, [first, np.arange(k), last])
        if len(seg.inv) % mod == want:
            key, c, o = seg.containers(2)[-1]
            assert key == 1 and o + (2 * c if c <= 4096 else 8192) == len(seg.inv)
            return seg
    raise AssertionError("no file length %d modulo %d" % (want, mod))


@pytest.mark.parametrize("kind", ["array", "bitmap"])
@pytest.mark.parametrize("want,mod", [(2, 4), (0, 16)])
def test_last_container_ends_at_the_files_last_byte(rk, monkeypatch, kind, want, mod):
    """File length 2 modulo 4 (a bitmap container there takes its last two bytes from the dword that crosses the end
    of the file; an array container's last granule reaches past it) and 0 modulo 16 (nothing past the end is read)."""
    seg = _file_end_seg(kind, want, mod)
    assert len(seg.inv) % mod == want
    _check(rk, monkeypatch, [(seg, [[2]]), (seg, [[0], [2], OR]), (seg, [[0], [2], NOT, AND])])


@functools.lru_cache(None)
def _many_seg():
    rng = np.random.default_rng(700)
    n = 4 * 65536 + 4321
    small = []
    for _ in range(70):
        chunks = rng.choice(5, int(rng.integers(1, 4)), replace=False)
        small.append(_docs(rng, n, {int(c): int(rng.integers(1, 40)) for c in chunks if c != 3}
                           or {0: 3}))
    big = [_docs(rng, n, {0: 4096, 1: 3000, 2: 4096, 4: 100}), _docs(rng, n, {0: 4000, 1: 4096, 2: 4090}),
           _docs(rng, n, {0: 3900, 2: 4096, 4: 4000}), _docs(rng, n, {0: 4096, 1: 5000, 2: 3500}),
           _docs(rng, n, {0: 30000, 1: 200, 2: 50000, 4: 4321})]
    seg = R.Seg(n, small + big)
    assert all(k != 3 for i in range(len(seg.bitmaps)) for k, _, _ in seg.containers(i))
    return seg


def test_exactly_64_bitmaps(rk, monkeypatch):
    """Every lane owns a bitmap; chunk 3 holds no container of any of them."""
    seg = _many_seg()
    big = [70, 71, 72, 73, 74]
    progs = [(seg, [list(range(0, 30)), list(range(30, 59)), OR, big, NOT, AND]),
             (seg, [list(range(0, 59)) + big]),
             (seg, [list(range(5, 35)), big, AND, list(range(35, 64)), AND])]
    assert all(sum(len(t) for t in p if R.is_leaf(t)) == 64 for _, p in progs)
    assert sorted(R.wave_slots(p) for _, p in progs) == [1, 1, 3]
    for p in progs:
        _check(rk, monkeypatch, [p])


def test_more_array_granules_than_one_round(rk, monkeypatch):
    """Four containers of about 4,000 elements in one chunk are about 2,000 granules, several rounds of the 64 lanes'
    granules, in phase 0 and in phase 1; with a bitmap container of either phase beside them."""
    seg = _many_seg()
    arrays, dense = [70, 71, 72, 73], [74]
    for c in (0, 2):
        assert sum(-(-2 * card // 16) for i in arrays for k, card, _ in seg.containers(i) if k == c) > 3 * 512
    _check(rk, monkeypatch, [(seg, [arrays]), (seg, [arrays + dense]), (seg, [dense, arrays, NOT, AND]),
                             (seg, [[70, 71], [72, 73] + dense, NOT, AND]), (seg, [[0, 1, 2], arrays, NOT, AND])])


def test_chunk_without_any_container(rk, monkeypatch):
    seg = _many_seg()
    _check(rk, monkeypatch, [(seg, [[0, 1, 2, 70]]), (seg, [[3, 4], [71, 74], NOT, AND]), (seg, [[5], NOT])])
    for p in ([[0, 1, 2, 70]], [[3, 4], [71, 74], NOT, AND]):
        assert not R.evaluate(seg, p)[3 * R.CHUNK_WORDS:4 * R.CHUNK_WORDS].any()


@functools.lru_cache(None)
def _c5_seg():
    """C5's shape per chunk: 32 array containers of about 65 elements, one of about 655, one bitmap container."""
    rng = np.random.default_rng(800)
    n = 3 * 65536 + 12345
    per = lambda k: {c: max(1, int(k * (min(n, (c + 1) << 16) - (c << 16)) / 65536 + rng.integers(-3, 4)))
                     for c in range(4)}
    return R.Seg(n, [_docs(rng, n, per(65)) for _ in range(32)] + [_docs(rng, n, per(655)), _docs(rng, n, per(19600))])


@pytest.mark.parametrize("nslots", [1, 2, 3])
def test_c5_shape_with_1_2_and_3_mask_slots(rk, monkeypatch, nslots):
    """a b OR c NOT AND needs one slot; the kernels built for two and three must give the same masks."""
    seg = _c5_seg()
    prog = [list(range(32)), [32], OR, [33], NOT, AND]
    assert R.wave_slots(prog) == 1
    assert [c > 4096 for _, c, _ in seg.containers(33)] == [True, True, True, False]
    _check(rk, monkeypatch, [(seg, prog)] * 3, nslots=nslots)


@pytest.mark.parametrize("parts", [2, 3])
def test_wave_range_starting_past_chunk_0(rk, monkeypatch, parts):
    """Segments of four and five chunks in 2 or 3 parts: walks of two or three chunks that start at chunk 2 or 3 by a
    cursor seek (with 3 parts the four-chunk segment's third range is empty)."""
    c5, many = _c5_seg(), _many_seg()
    progs = [(c5, [list(range(32)), [32], OR, [33], NOT, AND]), (many, [[70, 71, 74], [0, 1, 2], NOT, AND]),
             (many, [[72], [73, 74], OR])]
    _check(rk, monkeypatch, progs, modes=("rparts=%d" % parts, "rnarrow,rparts=%d" % parts))


@functools.lru_cache(None)
def _short_segs():
    rng = np.random.default_rng(900)
    two = 65536 + 777
    a = R.Seg(two, [_docs(rng, two, {0: 5000, 1: 300}), _docs(rng, two, {1: 100}), _docs(rng, two, {0: 9, 1: 777})])
    b = R.Seg(27, [np.array([0, 5, 26]), np.array([3])])
    assert a.containers(2)[1][1] == 777 and two % 32 != 0
    return a, b


def test_ragged_last_chunk_and_a_segment_shorter_than_a_mask_word(rk, monkeypatch):
    a, b = _short_segs()
    _check(rk, monkeypatch, [(a, [[0, 1], [2], AND]), (a, [[1], NOT]), (a, [[0], [2], NOT, AND]), (b, [[0], [1], OR, NOT]),
                             (b, [[0], [1], NOT, AND]), (b, [[], NOT])])
