"""The bitmap inverted-index kernels (pgx_roaring_expand, pgx_roaring_program and its _wide, _seg and _wave forms)
launched directly, through their launchers, on torch device buffers and compared with the numpy model of
tests/roaring_ref.py.  Every mask is pre-filled with a sentinel and has guard words behind it, which must come back
untouched; all comparisons are exact.  Every launch stays inside its kernel's contract (what the host would send): the
stack kernel programs at most 4 operands deep, the wide and seg kernels at most 8 leaves, the seg kernel at most 512
bitmaps, the wave kernel at most 64 bitmaps and 3 mask slots.

The main segment has three full 65536-doc chunks and a ragged tail (num_docs is no multiple of 32).  Its first eight
bitmaps are built for the kernels' edges (see _main_seg); 600 small ones make up the leaves of many bitmaps."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import roaring_ref as R
from tests.roaring_ref import AND, NOT, OR

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = np.uint32(0xA5A5A5A5)
N_DOCS = 3 * 65536 + 4321
EVERY, NO_FIRST, NO_MID, LAST, BIG, EDGE, ODD, SHIFTED, SMALL0, NSMALL = 0, 1, 2, 3, 4, 5, 6, 7, 8, 600


def _docs(rng, num_docs, per_chunk):
    """Random docs: per_chunk[c] of them in chunk c."""
    out = []
    for c, k in per_chunk.items():
        lo, hi = c << 16, min(num_docs, (c + 1) << 16)
        out.append(lo + rng.choice(hi - lo, k, replace=False))
    return np.concatenate(out)


def _small(rng, num_docs, count):
    nch = (num_docs + 65535) >> 16
    out = []
    for _ in range(count):  # 1 to 3 chunks, 1 to 6 docs in each
        chunks = rng.choice(nch, int(rng.integers(1, min(3, nch) + 1)), replace=False)
        out.append(_docs(rng, num_docs, {int(c): int(rng.integers(1, 7)) for c in chunks}))
    return out


@functools.lru_cache(None)
def _main_seg():
    rng = np.random.default_rng(20)
    bm = [_docs(rng, N_DOCS, {0: 300, 1: 300, 2: 300, 3: 300}),      # EVERY: key[c] == c, the probe at index c hits
          _docs(rng, N_DOCS, {1: 200, 2: 200, 3: 200}),              # NO_FIRST: binary search / cursor seek
          _docs(rng, N_DOCS, {0: 150, 3: 150}),                      # NO_MID: nothing in chunks 1 and 2
          _docs(rng, N_DOCS, {3: 78}),                               # LAST: the ragged tail only
          _docs(rng, N_DOCS, {0: 30000, 1: 101, 2: 20000, 3: 51}),   # BIG: bitmap containers, 4-byte aligned
          _docs(rng, N_DOCS, {1: 4096, 2: 4097}),                    # EDGE: largest array, smallest bitmap container
          _docs(rng, N_DOCS, {0: 7}),                                # ODD: 30 bytes, shifts what follows by 2 modulo 4
          _docs(rng, N_DOCS, {0: 10000, 3: 4200})]                   # SHIFTED: bitmap containers at 2 modulo 4
    seg = R.Seg(N_DOCS, bm + _small(rng, N_DOCS, NSMALL))
    assert [k for k, _, _ in seg.containers(EVERY)] == [0, 1, 2, 3]
    assert [k for k, _, _ in seg.containers(NO_FIRST)] == [1, 2, 3]
    assert [(c, o % 4) for _, c, o in seg.containers(BIG)] == [(30000, 0), (101, 0), (20000, 2), (51, 2)]
    assert [c for _, c, _ in seg.containers(EDGE)] == [4096, 4097]
    assert [(c, o % 4) for _, c, o in seg.containers(SHIFTED)] == [(10000, 2), (4200, 2)]
    return seg


@functools.lru_cache(None)
def _short_segs():
    """Two chunks with a ragged tail, and a segment shorter than one mask word."""
    rng = np.random.default_rng(21)
    two = 65536 + 777
    first = [_docs(rng, two, {0: 5000, 1: 300}), _docs(rng, two, {1: 100}), _docs(rng, two, {0: 9})]
    a = R.Seg(two, first + _small(rng, two, 20))
    b = R.Seg(27, [np.array([0, 5, 26]), np.array([3])])
    return a, b


def _small_ids(first, count):
    return list(range(SMALL0 + first, SMALL0 + first + count))


_EXPECTED = {}


def _expected(seg, prog):
    key = (id(seg), repr(prog))
    if key not in _EXPECTED:
        _EXPECTED[key] = R.evaluate(seg, prog)
    return _EXPECTED[key]


def _depth(prog):
    d = m = 0
    for t in prog:
        d += 1 if R.is_leaf(t) else (0 if t == NOT else -1)
        m = max(m, d)
    return m


class _RK:
    def __init__(self):
        import torch
        from pinot_amd import native as N
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.expand, self.program, self.wave = R.bind(N.lib())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        self._inv = {}

    def up(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.dev)

    def inv(self, seg):
        if id(seg) not in self._inv:
            self._inv[id(seg)] = self.up(np.frombuffer(seg.inv, np.uint8))
            assert self._inv[id(seg)].data_ptr() % 4 == 0
        return self._inv[id(seg)]

    def masks(self, segs):
        """One buffer of sentinel words: a mask of nchunks x 2048 words per entry of segs, guard words behind each."""
        offs, total = [], 0
        for s in segs:
            offs.append(total)
            total += s.nchunks * R.CHUNK_WORDS + GUARD
        return self.up(np.full(total, SENT, np.uint32)), offs

    def back(self, buf, offs, segs):
        self.torch.cuda.synchronize(self.dev)
        a = buf.cpu().numpy().view(np.uint32)
        out = []
        for o, s in zip(offs, segs):
            n = s.nchunks * R.CHUNK_WORDS
            assert (a[o + n:o + n + GUARD] == SENT).all()
            out.append(a[o:o + n])
        return out


@pytest.fixture(scope="module")
def rk():
    return _RK()


class _Descs:
    """The JRDesc array of a launch: one descriptor per distinct (segment, leaf), shared by the programs that use it."""

    def __init__(self, rk):
        self.rk, self.index, self.descs, self.keep = rk, {}, [], []

    def of(self, seg, ids, mask=0):
        key = (id(seg), tuple(ids), mask)
        if key not in self.index:
            assert len(ids) > 0 and max(ids) < len(seg.bitmaps)
            idt = self.rk.up(np.asarray(ids, np.uint32))
            self.keep.append(idt)
            self.index[key] = len(self.descs)
            self.descs.append(R.JRDesc(mask, self.rk.inv(seg).data_ptr(), idt.data_ptr(), len(ids), seg.nchunks))
        return self.index[key]

    def dev(self):
        arr = (R.JRDesc * max(1, len(self.descs)))(*self.descs)
        return self.rk.up(np.frombuffer(bytes(arr), np.uint8))


def _run(rk, progs, kind, param):
    """Launches progs = [(segment, postfix program)] with one kernel and compares every mask with the model."""
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
    launch = rk.wave if kind == "wave" else rk.program
    assert launch(pdev.data_ptr(), ddev.data_ptr(), len(progs), maxchunks, param, rk.stream) == 0
    for got, (seg, prog) in zip(rk.back(buf, offs, segs), progs):
        np.testing.assert_array_equal(got, _expected(seg, prog))


def _check(rk, progs, kinds=("stack", "wide", "seg", "wave")):
    """Every kernel of `kinds` whose contract holds for all of progs; returns the kernels run."""
    leaves = [sum(R.is_leaf(t) for t in p) for _, p in progs]
    nb = [sum(len(t) for t in p if R.is_leaf(t)) for _, p in progs]
    depth = max(_depth(p) for _, p in progs)
    slots = max(R.wave_slots(p) for _, p in progs)
    ran = []
    for kind in kinds:
        if kind == "stack" and depth <= 4:
            _run(rk, progs, kind, 0)
        elif kind == "wide" and max(leaves) <= 8 and depth <= 4:
            _run(rk, progs, kind, max(leaves))
        elif kind == "seg" and max(leaves) <= 8 and depth <= 4 and max(nb) <= 512:
            _run(rk, progs, kind, -max(leaves))
        elif kind == "wave" and max(nb) <= 64 and slots <= 3 and depth <= 4:
            _run(rk, progs, kind, slots)
        else:
            continue
        ran.append(kind)
    return ran


# (program, the wave kernel's mask slots).  a b OR c NOT AND is the shape of C5's filter.
SHAPES = [
    ([[EVERY, BIG]], 1),                                              # array and bitmap containers in the same chunks
    ([[NO_FIRST], [NO_MID], OR, [LAST, SHIFTED], NOT, AND], 1),      # both fusions
    ([[BIG], NOT], 1),                                                # a leading a NOT
    ([[], NOT], 1),                                                   # the empty leaf alone under NOT: [0, num_docs)
    ([[], [EVERY, SHIFTED], OR], 1),
    ([[EDGE], [ODD, BIG], OR, [], NOT, AND], 1),                      # clearing the empty leaf out leaves the OR
    ([[EVERY, EDGE], [BIG], AND], 2),
    ([[], [EVERY, SHIFTED], AND], 2),
    ([[], [LAST], NOT, OR], 2),                                       # the empty leaf next to a flipped one
    ([[LAST], NOT, [], AND], 2),
    ([[EDGE], [ODD, SHIFTED], NOT, AND, [EVERY], OR], 2),             # AND-NOT fused, the OR after it is not
    ([[NO_MID], NOT, [NO_FIRST], NOT, AND], 2),
    ([[EVERY, BIG], [SHIFTED, EDGE], AND, [BIG, NO_MID], AND], 3),
    ([[BIG], [EDGE], AND, [LAST], [SHIFTED], OR, NOT, AND], 3),
    ([[EVERY], [SHIFTED], AND, [EDGE], [NO_FIRST, NO_MID], AND, OR], 4),   # a b AND c d AND OR: not for the wave kernel
]


def test_stated_slot_counts():
    for prog, slots in SHAPES:
        assert R.wave_slots(prog) == slots


@pytest.mark.parametrize("nslots", [1, 2, 3])
def test_wave_programs_by_slot_count(rk, nslots):
    seg = _main_seg()
    progs = [(seg, p) for p, s in SHAPES if s == nslots]
    assert len(progs) >= 2
    _run(rk, progs, "wave", nslots)


@pytest.mark.parametrize("kind", ["stack", "wide", "seg"])
def test_program_kernels(rk, kind):
    seg = _main_seg()
    assert _check(rk, [(seg, p) for p, _ in SHAPES], (kind,)) == [kind]


def test_not_at_the_ragged_tail():
    """The model itself: the flipped empty leaf is exactly [0, num_docs), so the last word is partial and the words
    past it are 0."""
    m = _expected(_main_seg(), [[], NOT])
    w = N_DOCS // 32
    assert (m[:w] == 0xFFFFFFFF).all() and m[w] == (1 << (N_DOCS % 32)) - 1 and N_DOCS % 32 and (m[w + 1:] == 0).all()
    assert len(m) == 4 * R.CHUNK_WORDS


def test_leaf_of_more_than_256_bitmaps(rk):
    """A second container-search batch, with the large containers in it; in the wide kernel the second batch also
    starts in the middle of a leaf."""
    seg = _main_seg()
    big = _small_ids(0, 300) + [BIG, EDGE, SHIFTED]
    progs = [(seg, [big]), (seg, [big, [EVERY], NOT, AND]), (seg, [_small_ids(300, 200), big, OR, [NO_FIRST], AND])]
    assert _check(rk, progs) == ["stack", "wide", "seg"]


def test_seg_with_up_to_512_bitmaps(rk):
    seg = _main_seg()
    progs = [(seg, [_small_ids(0, 200) + [BIG], [NO_FIRST, NO_MID], NOT, AND]),
             (seg, [_small_ids(0, 400), _small_ids(400, 107) + [BIG, EDGE, SHIFTED, EVERY], OR, [LAST], NOT, AND])]
    assert [sum(len(t) for t in p if R.is_leaf(t)) for _, p in progs] == [203, 512]
    assert _check(rk, progs, ("seg", "wide")) == ["seg", "wide"]


def test_wave_with_exactly_64_bitmaps(rk):
    seg = _main_seg()
    last = [EVERY, BIG, EDGE, SHIFTED]
    progs = [(seg, [_small_ids(0, 30), _small_ids(30, 30), OR, last, NOT, AND]),
             (seg, [_small_ids(100, 30), _small_ids(60, 30), OR, last, AND]),
             (seg, [_small_ids(200, 20), last, AND, _small_ids(220, 20), _small_ids(240, 20), OR, AND])]
    assert all(sum(len(t) for t in p if R.is_leaf(t)) == 64 for _, p in progs)
    for p in progs:
        assert _check(rk, [p], ("wave",)) == ["wave"]
    assert sorted(R.wave_slots(p) for _, p in progs) == [1, 2, 3]


def test_segments_of_different_lengths_in_one_launch(rk):
    """nchunks 4, 2 and 1 under one maxchunks; the short segments' masks are followed by guard words as well."""
    seg, (two, tiny) = _main_seg(), _short_segs()
    progs = [(two, [[0, 1], [2], AND]),
             (seg, [[NO_FIRST], [BIG], OR, [EVERY], NOT, AND]),
             (tiny, [[0], [1], OR, NOT]),
             (two, [list(range(3, 23)), [0], OR]),
             (tiny, [[], NOT]),
             (seg, [[LAST], NOT])]
    assert _check(rk, progs) == ["stack", "wide", "seg", "wave"]


@pytest.mark.parametrize("kind,nprogs,parts", [("wave", 2731, 3), ("seg", 683, 3), ("seg", 2048, 1)])
def test_a_walk_of_several_chunks_starting_past_chunk_0(rk, kind, nprogs, parts):
    """The launchers derive the parts of a segment's walk from nprogs: with 3 parts of 2 chunks the second walk starts
    at chunk 2, where EVERY holds key[2] == 2 and NO_FIRST / NO_MID / LAST need the seek; with 1 part one workgroup
    walks all four chunks.  The programs share their descriptors."""
    seg = _main_seg()
    if kind == "wave":
        assert parts == max(1, min(seg.nchunks, (8192 + nprogs - 1) // nprogs))
    else:
        assert parts == max(1, min(min(seg.nchunks, 8), (2048 + nprogs - 1) // nprogs))
    assert parts < seg.nchunks
    shapes = [[[EVERY], [NO_FIRST, BIG], OR, [NO_MID, LAST], NOT, AND],
              [[EVERY, NO_MID, SHIFTED], [NO_FIRST, LAST, EDGE], AND],
              [[LAST], NOT]]
    progs = [(seg, shapes[i % 3]) for i in range(nprogs)]
    assert _check(rk, progs, (kind,)) == [kind]


def test_expand(rk):
    """pgx_roaring_expand: one mask per (segment, leaf) descriptor."""
    seg, (two, tiny) = _main_seg(), _short_segs()
    leaves = [(seg, [EVERY, BIG]), (seg, [LAST]), (two, [0, 1, 2]), (seg, _small_ids(0, 300) + [BIG, EDGE, SHIFTED]),
              (seg, [ODD, SHIFTED, NO_FIRST]), (tiny, [1]), (seg, [NO_MID, EDGE])]
    segs = [s for s, _ in leaves]
    buf, offs = rk.masks(segs)
    descs = _Descs(rk)
    for off, (s, ids) in zip(offs, leaves):
        descs.of(s, ids, buf.data_ptr() + 4 * off)
    ddev = descs.dev()
    assert rk.expand(ddev.data_ptr(), len(leaves), max(s.nchunks for s in segs), rk.stream) == 0
    for got, (s, ids) in zip(rk.back(buf, offs, segs), leaves):
        np.testing.assert_array_equal(got, _expected(s, [ids]))
