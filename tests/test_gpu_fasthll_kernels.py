"""The FASTHLL fold kernel (pinot_amd/csrc/pgx_fasthll.hip: pgx_fasthll_fold) launched directly on torch device buffers
and compared with the numpy model of tests/fasthll_ref.py, on hand-built bitmaps and random register images with
registers 0 .. 31.  The output is pre-filled (the kernel takes the maximum with what is there) and has guard words past
its end, which must come back untouched.  The comparisons are exact: a maximum depends on neither grid nor scheduling."""
import ctypes as C

import numpy as np
import pytest

from tests import fasthll_ref as F

pytestmark = pytest.mark.gpu

GUARD = 64
S32 = np.uint32(0xA5A5A5A5)


class _FK:
    def __init__(self):
        import torch
        from pinot_amd import native as N
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.launch, self.split = F.bind(N.lib())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.dev)

    def fold(self, table, card, image, rows, slots, pre, wgs=3):
        """One launch into a copy of `pre` ([len(rows), 256] u32); returns the registers."""
        rows = np.asarray(rows, np.int64)
        n = len(rows) * F.REGS
        out = self.up(np.concatenate([np.asarray(pre, np.uint32).reshape(-1), np.full(GUARD, S32, np.uint32)]))
        t, im, rd = self.up(np.asarray(table, np.uint32)), self.up(F.pack_image(image)), self.up(rows)
        st = self.launch(t.data_ptr(), card, im.data_ptr(), rd.data_ptr(), rows.ctypes.data, len(rows), slots,
                         out.data_ptr(), wgs, self.stream)
        assert st == 0
        self.torch.cuda.synchronize(self.dev)
        a = out.cpu().numpy().view(np.uint32)
        assert len(a) == n + GUARD and (a[n:] == S32).all()
        return a[:n].reshape(len(rows), F.REGS).copy()


@pytest.fixture(scope="module")
def fk():
    return _FK()


def _image(rng, card):
    img = rng.integers(0, 32, (card, F.REGS)).astype(np.uint8)
    img[rng.random((card, F.REGS)) < 0.5] = 0  # estimators are mostly small registers
    return img


def _table(rng, card, slots, density):
    """slots rows of random bits; the spare bits of the last word are all set on purpose."""
    w = F.words(card)
    bits = rng.random((slots, w * 32)) < density
    t = np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(slots, w).copy()
    if card % 32:
        t[:, -1] |= np.uint32(~((1 << (card % 32)) - 1) & 0xFFFFFFFF)
    return t


@pytest.mark.parametrize("card", [1, 31, 32, 33, 1000, 40000])
def test_small_cards_and_spare_bits(fk, card):
    rng = np.random.default_rng(card)
    img, slots = _image(rng, card), 5
    t = _table(rng, card, slots, 0.3)
    t[0] = _table(rng, card, 1, 1.0)[0]  # a full row, spare bits included
    rows = list(range(slots))
    pre = np.zeros((slots, F.REGS), np.uint32)
    got = fk.fold(t, card, img, rows, slots, pre)
    assert np.array_equal(got, F.fold(t, card, img, rows))
    assert np.array_equal(got[0], img.max(axis=0))
    assert got.max() <= 31


def test_zero_and_full_bitmaps(fk):
    rng = np.random.default_rng(40)
    card = 2500
    img = _image(rng, card)
    t = np.zeros((3, F.words(card)), np.uint32)
    t[1] = 0xFFFFFFFF
    t[2, 40] = 1 << 7  # one bit in the middle of an otherwise zero row: dictId 1287
    pre = rng.integers(0, 4, (3, F.REGS)).astype(np.uint32)
    got = fk.fold(t, card, img, [0, 1, 2], 3, pre)
    assert np.array_equal(got[0], pre[0])
    assert np.array_equal(got[1], np.maximum(pre[1], img.max(axis=0)))
    assert np.array_equal(got[2], np.maximum(pre[2], img[1287]))
    assert not fk.fold(t, card, img, [0], 3, np.zeros((1, F.REGS), np.uint32)).any()


def test_listed_rows_unsorted_repeated_and_a_subset(fk):
    rng = np.random.default_rng(41)
    card, slots = 700, 9
    img, t = _image(rng, card), _table(rng, card, 9, 0.02)
    rows = [7, 2, 2, 8, 0, 7]
    got = fk.fold(t, card, img, rows, slots, np.zeros((len(rows), F.REGS), np.uint32), wgs=4)
    assert np.array_equal(got, F.fold(t, card, img, rows))
    assert np.array_equal(got[1], got[2]) and np.array_equal(got[0], got[5]) and got.any()
    one = fk.fold(t, card, img, rows, slots, np.zeros((len(rows), F.REGS), np.uint32), wgs=1)  # one workgroup strides
    assert np.array_equal(one, got)


def test_two_dictionaries_fold_into_one_output(fk):
    """The second launch takes the maximum with what the first left: it must not overwrite."""
    rng = np.random.default_rng(42)
    rows, slots = [0, 1, 2, 3], 4
    ca, cb = 333, 90
    ia, ib = _image(rng, ca), _image(rng, cb)
    ta, tb = _table(rng, ca, slots, 0.05), _table(rng, cb, slots, 0.1)
    tb[2] = 0  # group 2 holds nothing of the second dictionary
    first = fk.fold(ta, ca, ia, rows, slots, np.zeros((4, F.REGS), np.uint32))
    both = fk.fold(tb, cb, ib, rows, slots, first)
    want = F.fold(tb, cb, ib, rows, F.fold(ta, ca, ia, rows))
    assert np.array_equal(both, want)
    assert np.array_equal(both[2], first[2]) and (both >= first).all() and (both != first).any()
    assert (first > F.fold(tb, cb, ib, rows)).any()  # some registers of the first survive only if maxed


@pytest.mark.parametrize("card", [F.SPLIT_CARD, F.SPLIT_CARD + 1, 3 * F.SPLIT_CARD + 77])
def test_rows_at_the_split_boundary(fk, card):
    """Up to SPLIT_CARD values one workgroup folds a row; one value more and two share it (the launcher's own rule);
    the last card gives four, the fourth with a short stretch.  Largest image: 1.6 MB."""
    assert fk.split(card) == (1 if card == F.SPLIT_CARD else 2 if card == F.SPLIT_CARD + 1 else 4)
    rng = np.random.default_rng(card)
    img, slots = _image(rng, card), 3
    t = _table(rng, card, slots, 0.01)
    t[1] = 0
    t[1, -1] = 1           # only the last word's first bit: dictId 32 * (words - 1), the second workgroup's at + 1
    t[1, 0] = 1 << 31      # and dictId 31, the first workgroup's
    t[2, F.SPLIT_WORDS - 1] |= np.uint32(1 << 31)  # the last bit before the boundary
    rows = [2, 0, 1]
    pre = rng.integers(0, 3, (3, F.REGS)).astype(np.uint32)
    got = fk.fold(t, card, img, rows, slots, pre, wgs=2)
    assert np.array_equal(got, F.fold(t, card, img, rows, pre))
    last = 32 * (F.words(card) - 1)
    assert np.array_equal(got[2], np.maximum(pre[2], np.maximum(img[31], img[last])))
