"""The DISTINCTCOUNT kernels (pinot_amd/csrc/pgx_distinct.hip: pgx_distinct_mark, _mark_group, _mark_mv, _mark_mv_group,
pgx_distinct_count, pgx_distinct_emit) launched directly on torch device buffers and compared with the numpy model of
tests/distinct_ref.py.  Every output is pre-filled with random bits, which must survive (the kernels OR), and has guard
words past its end, which must come back untouched.  The comparisons are exact: a mark is an OR, so neither the grid
size nor the scheduling can change a bit.

Real rows hold dictIds of 1 and more wherever the cardinality allows, and bit 0 of every pre-fill is clear: a padding
row of a forward index (dictId 0), a mask bit at or past num_docs or the spare mask word read as rows would set it."""
import ctypes as C

import numpy as np
import pytest

from tests import distinct_ref as D
from tests import hll_mv_ref as M

pytestmark = pytest.mark.gpu

GUARD = 64
S32 = np.uint32(0xA5A5A5A5)
LDS_CARD = D.LDS_WORDS * 32  # 262,144: the largest bitmap marked in LDS


class _DK:
    def __init__(self):
        import torch
        from pinot_amd import native as N
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.k = D.bind(N.lib())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.dev)

    def out(self, prefill):
        a = np.concatenate([np.asarray(prefill).view(np.uint32).reshape(-1), np.full(GUARD, S32, np.uint32)])
        return self.up(a)

    def back(self, buf, n):
        self.torch.cuda.synchronize(self.dev)
        a = buf.cpu().numpy().view(np.uint32)
        assert len(a) == n + GUARD and (a[n:] == S32).all()
        return a[:n]


@pytest.fixture(scope="module")
def dk():
    return _DK()


def _bits_for(card):
    return max(1, int(card - 1).bit_length())


def _selected(rng, n, density):
    if density == 0:
        return np.zeros(n, bool)
    if density == 1:
        return np.ones(n, bool)
    return rng.random(n) < density


def _item(rng, n, density, bits, card, out=0):
    ids = rng.integers(1, card, n) if card > 1 else np.zeros(n, np.int64)
    return {"selected": _selected(rng, n, density), "ids": ids, "bits": bits, "card": card, "out": out}


def _prefill(rng, card, rows=1):
    """Random bits below card, bit 0 of every row clear."""
    w = D.words(card)
    p = rng.integers(0, 1 << 32, (rows, w), dtype=np.uint64).astype(np.uint32)
    if card % 32:
        p[:, -1] &= np.uint32((1 << (card % 32)) - 1)
    if card > 1:
        p[:, 0] &= np.uint32(0xFFFFFFFE)
    return p if rows > 1 else p[0]


def _fill(dk, d, it, keep, out_ptr):
    n = len(it["selected"])
    mask, fwd = dk.up(D.pack_mask(it["selected"])), dk.up(D.pack_fwd(it["ids"], it["bits"], it.get("rows", n)))
    keep += [mask, fwd]
    d.sel, d.fwd, d.out = mask.data_ptr(), fwd.data_ptr(), out_ptr
    d.bits, d.num_docs, d.card = it["bits"], n, it["card"]


def _run(dk, items, prefills, wgs, expect_status=0, mutate=None, nitems=None):
    """pgx_distinct_mark over `items` into len(prefills) bitmaps; returns them."""
    keep = []
    outs = [dk.out(p) for p in prefills]
    arr = (D.DistinctItem * max(1, len(items)))()
    for i, it in enumerate(items):
        _fill(dk, arr[i], it, keep, outs[it["out"]].data_ptr())
    if mutate:
        mutate(arr)
    dev_items = dk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    st = dk.k["mark"](dev_items.data_ptr(), C.addressof(arr), len(items) if nitems is None else nitems, wgs, dk.stream)
    assert (st == 0) == (expect_status == 0) and (expect_status == 0 or st == expect_status)
    return [dk.back(o, len(p)).copy() for o, p in zip(outs, prefills)]


def _model(items, prefills):
    exp = [np.asarray(p, np.uint32).copy() for p in prefills]
    for it in items:
        exp[it["out"]] = D.mark(it["selected"], it["ids"], it["card"], exp[it["out"]])
    return exp


def _check(dk, items, prefills, wgs=3):
    got = _run(dk, items, prefills, wgs)
    for g, e in zip(got, _model(items, prefills)):
        np.testing.assert_array_equal(g, e)
    return got


_CARD = {1: 2, 7: 128, 10: 300, 17: 70000, 20: 1 << 20, 32: 70000}  # 2^20: an HBM-mode bitmap


@pytest.mark.parametrize("num_docs", [0, 1, 31, 32, 33, 8191, 8192, 8193])
def test_sizes_densities_and_widths(dk, num_docs):
    """Densities 0, 0.03 (sparse words: rows read one by one), 0.5 and 1 (dense words: the whole word decoded); the
    mask bits at and past num_docs and the spare word are all ones (pack_mask), the padding rows hold dictId 0."""
    rng = np.random.default_rng(num_docs)
    for bits in (1, 7, 10, 17, 20, 32):
        for density in (0, 0.03, 0.5, 1):
            card = _CARD[bits]
            pre = _prefill(rng, card)
            it = _item(rng, num_docs, density, bits, card)
            got = _check(dk, [it], [pre])[0]
            assert (got[0] & 1) == 0
            assert ((got & pre) == pre).all()
            if density == 0 or num_docs == 0:
                np.testing.assert_array_equal(got, pre)


@pytest.mark.parametrize("card", [1, 33, LDS_CARD, LDS_CARD + 1])
def test_cardinalities_and_both_bitmap_modes(dk, card):
    """card 1; card 33: the spare bits of the last word stay clear; the largest LDS bitmap and the smallest HBM one, with
    the last dictId marked.  dictIds at or past card in the data mark nothing."""
    rng = np.random.default_rng(card)
    n = 3 * 8192 + 37
    bits = _bits_for(card) + 1                      # the data can hold ids at and past card
    ids = rng.integers(min(1, card - 1), card + 3, n)
    ids[5] = card - 1
    it = {"selected": rng.random(n) < 0.5, "ids": ids, "bits": bits, "card": card, "out": 0}
    it["selected"][5] = True
    pre = np.zeros(D.words(card), np.uint32)
    got = _check(dk, [it], [pre])[0]
    assert set(D.set_ids(got, D.words(card) * 32).tolist()) == set(ids[it["selected"] & (ids < card)].tolist())
    assert ((got[-1] >> ((card - 1) & 31)) & 1) == 1
    if card > 1:
        assert (got[0] & 1) == 0


def test_workgroups_per_item_do_not_change_the_result(dk):
    rng = np.random.default_rng(11)
    for card, bits in ((70000, 17), (1 << 20, 20)):
        it = _item(rng, 3 * 8192 + 37, 0.5, bits, card)
        pre = _prefill(rng, card)
        outs = [_check(dk, [it], [pre], wgs=w)[0] for w in (1, 3, 64)]
        assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()


def test_five_items_in_one_launch_two_sharing_a_bitmap(dk):
    rng = np.random.default_rng(12)
    items = [_item(rng, 20000, 0.5, 12, 4000, out=0),
             _item(rng, 300, 1, 7, 100, out=1),
             _item(rng, 8192, 0, 10, 300, out=2),           # an empty item between two full ones
             _item(rng, 8193, 0.03, 12, 4000, out=0),       # the same dictionary: ORs into the first item's bitmap
             _item(rng, 1, 1, 3, 8, out=3)]
    pres = [np.zeros(D.words(c), np.uint32) for c in (4000, 100, 300, 8)]
    got = _check(dk, items, pres, wgs=4)
    np.testing.assert_array_equal(got[2], pres[2])
    alone = _model([items[0]], [pres[0]])[0]
    assert ((got[0] & alone) == alone).all() and (got[0] != alone).any()


# ---- pgx_distinct_mark_group -------------------------------------------------------------------------------------------
def _group_cols(rng, n, gcards, locals0):
    """Two group columns: column 0 holds local ids 0..locals0-1 remapped into 0..gcards[0]-1 with some entries -1,
    column 1 global ids as they are (a null remap), a few of them at or past gcards[1]: slots past the key space."""
    remap = rng.permutation(gcards[0])[:locals0].astype(np.int32)
    if locals0 > 2:
        remap[rng.integers(0, locals0, 2)] = -1
    g1 = rng.integers(0, gcards[1], n)
    if n > 40:
        g1[rng.integers(0, n, 8)] = gcards[1] + 1   # slot >= slots whatever column 0 says
    return [(rng.integers(0, locals0, n), remap, _bits_for(locals0)), (g1, None, _bits_for(gcards[1] + 2))]


def _slots_of(it, gcards):
    slot = np.zeros(len(it["g"][0][0]), np.int64)
    bad = np.zeros(len(slot), bool)
    for (ids, remap, _), m in zip(it["g"], (1, gcards[0])):
        g = np.asarray(ids, np.int64)
        if remap is not None:
            g = np.asarray(remap, np.int64)[g]
        bad |= g < 0
        slot += np.where(g < 0, 0, g) * m
    return np.where(bad, -1, slot)


def _fill_gcols(dk, g, it, keep):
    for c, (ids, remap, gbits) in enumerate(it["g"]):
        fwd = dk.up(D.pack_fwd(ids, gbits, len(ids)))
        keep.append(fwd)
        g[c].fwd, g[c].bits = fwd.data_ptr(), gbits
        if remap is not None:
            rm = dk.up(remap)
            keep.append(rm)
            g[c].remap = rm.data_ptr()


def _run_group(dk, items, gcards, pre, wgs=3, expect_status=0, slots=None, mutate=None, ngcols=2, gmul1=None):
    true_slots = gcards[0] * gcards[1]
    table = dk.out(pre)
    keep = []
    arr = (D.DistinctGroupItem * max(1, len(items)))()
    for i, it in enumerate(items):
        _fill(dk, arr[i].d, it, keep, table.data_ptr())
        _fill_gcols(dk, arr[i].g, it, keep)
    if mutate:
        mutate(arr)
    gmul = (C.c_uint64 * 2)(1, gcards[0] if gmul1 is None else gmul1)
    dev_items = dk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    st = dk.k["mark_group"](dev_items.data_ptr(), C.addressof(arr), len(items), ngcols, C.addressof(gmul),
                            true_slots if slots is None else slots, wgs, dk.stream)
    assert (st == 0) == (expect_status == 0) and (expect_status == 0 or st == expect_status)
    return dk.back(table, pre.size).reshape(pre.shape)


def _group_model(items, gcards, pre):
    exp = pre.copy()
    for it in items:
        exp = D.mark_group(it["selected"], it["ids"], it["card"], _slots_of(it, gcards), gcards[0] * gcards[1], exp)
    return exp


@pytest.mark.parametrize("gcards", [(1, 1), (2, 1), (257, 3), (256, 256)])
def test_group_slots(dk, gcards):
    """slots 1, 2, 771 and 65536 (the limit); two items (segments with their own remap tables) share the table."""
    rng = np.random.default_rng(gcards[0] * 1000 + gcards[1])
    slots = gcards[0] * gcards[1]
    card = 40 if slots == 65536 else 3000
    items = []
    for n, density in ((3 * 8192 + 37, 0.5), (8193, 0.03)):
        it = _item(rng, n, density, _bits_for(card), card)
        it["g"] = _group_cols(rng, n, gcards, max(1, gcards[0] - gcards[0] // 3))
        items.append(it)
    pre = _prefill(rng, card, slots).reshape(slots, D.words(card))
    got = _run_group(dk, items, gcards, pre)
    np.testing.assert_array_equal(got, _group_model(items, gcards, pre))
    assert ((got[:, 0] & 1) == 0).all()  # padding rows, bits past num_docs, the spare word
    outs = [_run_group(dk, items, gcards, pre, wgs=w).tobytes() for w in (1, 64)]
    assert outs[0] == outs[1] == got.tobytes()


def test_group_ids_past_card_mark_nothing(dk):
    rng = np.random.default_rng(23)
    gcards = (5, 4)
    n = 9000
    it = {"selected": np.ones(n, bool), "ids": rng.integers(1, 64, n), "bits": 6, "card": 33, "out": 0}
    it["g"] = _group_cols(rng, n, gcards, 5)
    pre = np.zeros((20, D.words(33)), np.uint32)
    got = _run_group(dk, [it], gcards, pre)
    np.testing.assert_array_equal(got, _group_model([it], gcards, pre))
    assert (got[:, 1] <= 1).all()  # card 33: only bit 32 exists in the last word


# ---- the multi-value forms -------------------------------------------------------------------------------------------
def _mv_item(rng, ndocs, density, card, long_doc=None, out=0):
    counts = rng.integers(0, 4, ndocs)  # docs with 0 values among them
    if long_doc is not None and ndocs > long_doc:
        counts[long_doc] = 300
    total = int(counts.sum())
    ids = rng.integers(1, card, total) if card > 1 else np.zeros(total, np.int64)
    return {"selected": _selected(rng, ndocs, density), "counts": counts, "ids": ids, "bits": _bits_for(card),
            "card": card, "out": out, "rows": max(total, 1), "total": total}


def _fill_mv(dk, m, it, keep, start=None):
    st = dk.up(M.starts(it["counts"]) if start is None else start)
    keep.append(st)
    m.start, m.total = st.data_ptr(), it["total"]


def _run_mv(dk, items, prefills, wgs=3, expect_status=0, mutate=None, starts=None):
    keep = []
    outs = [dk.out(p) for p in prefills]
    arr = (D.DistinctMvItem * max(1, len(items)))()
    for i, it in enumerate(items):
        _fill(dk, arr[i].d, it, keep, outs[it["out"]].data_ptr())
        _fill_mv(dk, arr[i], it, keep, None if starts is None else starts[i])
    if mutate:
        mutate(arr)
    dev_items = dk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    st = dk.k["mark_mv"](dev_items.data_ptr(), C.addressof(arr), len(items), wgs, dk.stream)
    assert (st == 0) == (expect_status == 0) and (expect_status == 0 or st == expect_status)
    return [dk.back(o, len(p)).copy() for o, p in zip(outs, prefills)]


@pytest.mark.parametrize("ndocs", [0, 1, 33, 8193])
def test_mv_marks_every_value_of_every_selected_doc(dk, ndocs):
    rng = np.random.default_rng(100 + ndocs)
    for card in (300, LDS_CARD + 1):
        for density in (0, 0.03, 0.5, 1):  # density 1: a fully selected word is one range
            it = _mv_item(rng, ndocs, density, card, long_doc=17)
            pre = _prefill(rng, card)
            outs = [_run_mv(dk, [it], [pre], wgs=w)[0] for w in (1, 3, 64)]
            exp = D.mark_mv(it["selected"], it["counts"], it["ids"], card, pre)
            np.testing.assert_array_equal(outs[1], exp)
            assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()
            assert (exp[0] & 1) == 0


def test_mv_ranges_are_clamped_to_the_stream(dk):
    """start[] ends past the row count: the rows at and past `total` are never read (they hold dictId 0 here, the
    padding, whose bit stays clear), whatever start[] says."""
    rng = np.random.default_rng(31)
    it = _mv_item(rng, 5000, 1, 300, long_doc=40)
    start = M.starts(it["counts"]).copy()
    start[-10:] += 100000
    short = dict(it, total=it["total"] - 50)
    for item in (it, short):
        pre = np.zeros(D.words(300), np.uint32)
        got = _run_mv(dk, [item], [pre], starts=[start])[0]
        exp_rows = M.value_rows(item["selected"], item["counts"]) & (np.arange(len(item["ids"])) < item["total"])
        # the last ten docs' ranges now run to the end of the stream
        exp_rows[M.starts(item["counts"])[-11]:item["total"]] = True
        np.testing.assert_array_equal(got, D.mark(exp_rows, item["ids"], 300, pre))
        assert (got[0] & 1) == 0


def _run_mv_group(dk, items, gcards, pre, wgs=3, expect_status=0, slots=None, mutate=None, ngcols=2):
    true_slots = gcards[0] * gcards[1]
    table = dk.out(pre)
    keep = []
    arr = (D.DistinctMvGroupItem * max(1, len(items)))()
    for i, it in enumerate(items):
        _fill(dk, arr[i].g.d, it, keep, table.data_ptr())
        _fill_gcols(dk, arr[i].g.g, it, keep)
        _fill_mv(dk, arr[i], it, keep)
    if mutate:
        mutate(arr)
    gmul = (C.c_uint64 * 2)(1, gcards[0])
    dev_items = dk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    st = dk.k["mark_mv_group"](dev_items.data_ptr(), C.addressof(arr), len(items), ngcols, C.addressof(gmul),
                               true_slots if slots is None else slots, wgs, dk.stream)
    assert (st == 0) == (expect_status == 0) and (expect_status == 0 or st == expect_status)
    return dk.back(table, pre.size).reshape(pre.shape)


@pytest.mark.parametrize("gcards", [(1, 1), (7, 5), (256, 256)])
def test_mv_group(dk, gcards):
    rng = np.random.default_rng(gcards[0] * 77 + gcards[1])
    slots = gcards[0] * gcards[1]
    card = 40 if slots == 65536 else 1000
    items = []
    for ndocs, density in ((8193, 0.5), (4000, 0.03), (0, 1)):
        it = _mv_item(rng, ndocs, density, card, long_doc=17)
        it["g"] = _group_cols(rng, ndocs, gcards, max(1, gcards[0] - gcards[0] // 3))
        items.append(it)
    pre = _prefill(rng, card, slots).reshape(slots, D.words(card))
    exp = pre.copy()
    for it in items:
        exp = D.mark_mv_group(it["selected"], it["counts"], it["ids"], card, _slots_of(it, gcards), slots, exp)
    outs = [_run_mv_group(dk, items, gcards, pre, wgs=w) for w in (1, 3)]
    np.testing.assert_array_equal(outs[1], exp)
    assert outs[0].tobytes() == outs[1].tobytes()
    assert ((exp[:, 0] & 1) == 0).all()


# ---- pgx_distinct_count / pgx_distinct_emit -----------------------------------------------------------------------------
def _count_emit(dk, table, card, rows, slots=None, wgs=5, hash_codes=None, cap_less=0, per_row=1):
    slots = table.shape[0] if slots is None else slots
    hash_codes = (np.arange(card, dtype=np.int64) * 2654435761 % (1 << 32)).astype(np.uint32).view(np.int32) \
        if hash_codes is None else hash_codes
    tdev, rdev, hdev = dk.up(table), dk.up(np.asarray(rows, np.int64)), dk.up(hash_codes)
    cbuf = dk.out(np.full(len(rows), S32, np.uint32))
    assert dk.k["count"](tdev.data_ptr(), card, rdev.data_ptr(), len(rows), slots, cbuf.data_ptr(), wgs, dk.stream) == 0
    counts = dk.back(cbuf, len(rows)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(off[-1]) - cap_less
    obuf = dk.out(np.full(max(total, 0), S32, np.uint32))
    odev = dk.up(off[:-1].copy() if len(rows) else np.zeros(1, np.int64))
    assert dk.k["emit"](tdev.data_ptr(), card, rdev.data_ptr(), odev.data_ptr(), len(rows), slots, hdev.data_ptr(),
                        obuf.data_ptr(), max(total, 0), per_row, wgs, dk.stream) == 0
    return counts, dk.back(obuf, max(total, 0)).view(np.int32), hash_codes, off


@pytest.mark.parametrize("card", [1, 33, 8192 * 32, 300000])
def test_count_and_emit(dk, card):
    """Empty rows, a full row, a single bit in the last word, a non-contiguous row list with a repeat and a row outside
    the table; the codes are hash[dictId] in exactly ascending dictId order, whatever the grid."""
    rng = np.random.default_rng(card)
    w = D.words(card)
    table = np.zeros((6, w), np.uint32)
    table[1] = 0xFFFFFFFF                                             # full (bits at and past card are not counted)
    table[2, -1] = np.uint32(1) << ((card - 1) & 31)                  # the last dictId alone
    table[4] = rng.integers(0, 1 << 32, w, dtype=np.uint64).astype(np.uint32)
    table[5] = table[4] & rng.integers(0, 1 << 32, w, dtype=np.uint64).astype(np.uint32)
    rows = [5, 0, 2, 1, 4, 2, 9, 3]
    results = []
    for wgs, per_row in ((1, 1), (5, 3), (64, 1), (2, 64), (3, 1024)):  # (more workgroups per row than 256-word steps)
        counts, codes, h, off = _count_emit(dk, table, card, rows, wgs=wgs, per_row=per_row)
        for i, r in enumerate(rows):
            ids = D.set_ids(table[r], card) if r < 6 else np.zeros(0, np.int64)
            assert counts[i] == len(ids)
            np.testing.assert_array_equal(codes[off[i]:off[i + 1]], h[ids])
        results.append(codes.tobytes())
    assert len(set(results)) == 1
    assert counts[1] == 0 and counts[3] == card and counts[2] == 1 and counts[6] == 0


def test_emit_never_writes_past_its_capacity(dk):
    rng = np.random.default_rng(41)
    table = rng.integers(0, 1 << 32, (3, D.words(1000)), dtype=np.uint64).astype(np.uint32)
    full = _count_emit(dk, table, 1000, [0, 1, 2])[1]
    short = _count_emit(dk, table, 1000, [0, 1, 2], cap_less=7)[1]  # (back() checks the guards behind the output)
    np.testing.assert_array_equal(short, full[:-7])


# ---- launchers -------------------------------------------------------------------------------------------------------
def test_launchers_refuse_bad_arguments(dk):
    """Null pointers, a negative or too large count, bits outside 1..32, card < 1, slots < 1 or above the limit, gmul
    outside 1..slots, a negative stream row count, a zero grid: a status, no launch, every buffer left as it was."""
    rng = np.random.default_rng(14)
    it = _item(rng, 100, 1, 7, 100)
    pre = np.full(D.words(100), S32, np.uint32)

    def setter(field, value, path=()):
        def f(arr):
            o = arr[0]
            for p in path:
                o = getattr(o, p)
            setattr(o, field, value)
        return f

    sv = [{"wgs": 0}, {"wgs": 1025}, {"wgs": 3, "nitems": -1}, {"wgs": 3, "nitems": 65536}]
    for field, value in (("num_docs", -1), ("bits", 0), ("bits", 33), ("card", 0), ("card", -4), ("sel", None),
                         ("fwd", None), ("out", None)):
        sv.append({"wgs": 3, "mutate": setter(field, value)})
    for kw in sv:
        got = _run(dk, [it], [pre], kw.pop("wgs"), expect_status=D.INVALID_VALUE, **kw)[0]
        assert (got == pre).all()
    arr = (D.DistinctItem * 1)()
    assert dk.k["mark"](None, C.addressof(arr), 1, 1, dk.stream) == D.INVALID_VALUE
    assert dk.k["mark"](dk.up(np.zeros(64, np.uint8)).data_ptr(), None, 1, 1, dk.stream) == D.INVALID_VALUE
    assert dk.k["mark"](dk.up(np.zeros(64, np.uint8)).data_ptr(), C.addressof(arr), 0, 1, dk.stream) == 0  # no items

    gcards = (3, 2)
    git = dict(it, g=_group_cols(rng, 100, gcards, 3))
    gpre = np.full((6, D.words(100)), S32, np.uint32)

    def gbits(value, path):
        def f(arr):
            o = arr[0]
            for p in path:
                o = getattr(o, p)
            o[1].bits = value
        return f

    group = [{"wgs": 0}, {"slots": 0}, {"slots": -5}, {"slots": D.MAX_GROUP_SLOTS + 1}, {"ngcols": 0},
             {"ngcols": D.MAX_GROUP_COLS + 1}, {"gmul1": 0}, {"gmul1": 7}]
    for kw in group + [{"mutate": setter("num_docs", -1, ("d",))}, {"mutate": setter("bits", 33, ("d",))},
                       {"mutate": setter("card", 0, ("d",))}, {"mutate": gbits(0, ("g",))},
                       {"mutate": gbits(33, ("g",))}]:
        got = _run_group(dk, [git], gcards, gpre, expect_status=D.INVALID_VALUE, **kw)
        assert (got == gpre).all()

    mit = _mv_item(rng, 100, 1, 100)
    for mut in (setter("total", -1), setter("start", None), setter("card", 0, ("d",)), setter("bits", 0, ("d",))):
        got = _run_mv(dk, [mit], [pre], expect_status=D.INVALID_VALUE, mutate=mut)[0]
        assert (got == pre).all()
    assert (_run_mv(dk, [mit], [pre], wgs=0, expect_status=D.INVALID_VALUE)[0] == pre).all()
    mgit = dict(mit, g=_group_cols(rng, 100, gcards, 3))
    for kw in ({"wgs": 0}, {"slots": 0}, {"slots": D.MAX_GROUP_SLOTS + 1}, {"ngcols": 0},
               {"mutate": setter("total", -1)}, {"mutate": setter("start", None)},
               {"mutate": setter("card", 0, ("g", "d"))}, {"mutate": gbits(33, ("g", "g"))}):
        got = _run_mv_group(dk, [mgit], gcards, gpre, expect_status=D.INVALID_VALUE, **kw)
        assert (got == gpre).all()

    table = dk.up(np.zeros((4, 4), np.uint32))
    rows, off, h = dk.up(np.arange(4, dtype=np.int64)), dk.up(np.zeros(4, np.int64)), dk.up(np.zeros(128, np.int32))
    out = dk.out(np.full(16, S32, np.uint32))
    t, r, o, hp, op = table.data_ptr(), rows.data_ptr(), off.data_ptr(), h.data_ptr(), out.data_ptr()
    for args in ((None, 100, r, 4, 4, op, 1), (t, 0, r, 4, 4, op, 1), (t, 100, None, 4, 4, op, 1),
                 (t, 100, r, -1, 4, op, 1), (t, 100, r, 4, 0, op, 1), (t, 100, r, 4, D.MAX_GROUP_SLOTS + 1, op, 1),
                 (t, 100, r, 4, 4, None, 1), (t, 100, r, 4, 4, op, 0)):
        assert dk.k["count"](*args, dk.stream) == D.INVALID_VALUE
    for args in ((None, 100, r, o, 4, 4, hp, op, 16, 1, 1), (t, 0, r, o, 4, 4, hp, op, 16, 1, 1),
                 (t, 100, None, o, 4, 4, hp, op, 16, 1, 1), (t, 100, r, None, 4, 4, hp, op, 16, 1, 1),
                 (t, 100, r, o, -1, 4, hp, op, 16, 1, 1), (t, 100, r, o, 4, 0, hp, op, 16, 1, 1),
                 (t, 100, r, o, 4, 4, None, op, 16, 1, 1), (t, 100, r, o, 4, 4, hp, None, 16, 1, 1),
                 (t, 100, r, o, 4, 4, hp, op, -1, 1, 1), (t, 100, r, o, 4, 4, hp, op, 16, 1, 0),
                 (t, 100, r, o, 4, 4, hp, op, 16, 0, 1), (t, 100, r, o, 4, 4, hp, op, 16, 1025, 1)):
        assert dk.k["emit"](*args, dk.stream) == D.INVALID_VALUE
    assert (dk.back(out, 16) == S32).all()


def test_every_stored_width(dk):
    """Widths 1 .. 32 over 100 docs (three full mask words and a partial one), each with a sparse selection (three
    rows of every word, the index's last row among them: rows are read one by one) and a dense one (whole words are
    decoded).  Half the ids use the whole width, so a wrongly cut row marks another bit or lands past card."""
    rng = np.random.default_rng(18)
    n = 100
    sparse = np.zeros(n, bool)
    sparse[[1, 17, 31, 32, 40, 63, 64, 77, 95, 96, 98, n - 1]] = True
    items, pre = [], []
    for bits in range(1, 33):
        card = min(1 << bits, 1 << 16)
        ids = np.where(rng.random(n) < 0.5, rng.integers(0, card, n).astype(np.uint64),
                       rng.integers(0, 1 << bits, n, dtype=np.uint64))
        ids[n - 1] = card - 1
        for sel in (sparse, np.ones(n, bool)):
            items.append({"selected": sel, "ids": ids, "bits": bits, "card": card, "out": len(items)})
            pre.append(np.zeros(D.words(card), np.uint32))
    got = _check(dk, items, pre, wgs=2)
    assert all(g.any() for g in got)
