"""The PERCENTILE kernels (pinot_amd/csrc/pgx_percentile.hip: pgx_percentile_count, _count_group, _count_mv,
_count_mv_group, pgx_percentile_sizes, pgx_percentile_emit) launched directly on torch device buffers and compared with
the numpy model of tests/percentile_ref.py.  Every table is pre-filled with random counts, which must be added to, not
overwritten, and has guard words past its end, which must come back untouched.  The comparisons are exact: the adds are
integer adds, so neither the grid size nor the scheduling can change a counter.

Real rows hold dictIds of 1 and more wherever the cardinality allows: a padding row of a forward index (dictId 0), a
mask bit at or past num_docs or the spare mask word read as rows would show up in counter 0, which must keep its
pre-fill."""
import ctypes as C

import numpy as np
import pytest

from tests import hll_mv_ref as M
from tests import percentile_ref as P

pytestmark = pytest.mark.gpu

GUARD = 64
S32 = np.uint32(0xA5A5A5A5)
LDS = P.LDS_COUNTERS  # 8192: the largest table counted in LDS


class _PK:
    def __init__(self):
        import torch
        from pinot_amd import native as N
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.k = P.bind(N.lib())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.dev)

    def out(self, prefill):
        """A device buffer holding `prefill` (any dtype, as u32 words) and GUARD guard words behind it."""
        a = np.concatenate([np.ascontiguousarray(prefill).view(np.uint32).reshape(-1), np.full(GUARD, S32, np.uint32)])
        return self.up(a)

    def back(self, buf, nwords):
        self.torch.cuda.synchronize(self.dev)
        a = buf.cpu().numpy().view(np.uint32)
        assert len(a) == nwords + GUARD and (a[nwords:] == S32).all()
        return a[:nwords].copy()

    def back64(self, buf, n):
        return self.back(buf, 2 * n).view(np.uint64)


@pytest.fixture(scope="module")
def pk():
    return _PK()


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
    p = rng.integers(0, 1000, (rows, card)).astype(np.uint64)
    return p if rows > 1 else p[0]


def _fill(pk, d, it, keep, out_ptr):
    n = len(it["selected"])
    mask, fwd = pk.up(P.pack_mask(it["selected"])), pk.up(P.pack_fwd(it["ids"], it["bits"], it.get("rows", n)))
    keep += [mask, fwd]
    d.sel, d.fwd, d.out = mask.data_ptr(), fwd.data_ptr(), out_ptr
    d.bits, d.num_docs, d.card = it["bits"], n, it["card"]


def _status(st, expect_status):
    assert (st == 0) == (expect_status == 0) and (expect_status == 0 or st == expect_status)


def _run(pk, items, prefills, wgs, expect_status=0, mutate=None, nitems=None):
    """pgx_percentile_count over `items` into len(prefills) tables; returns them."""
    keep = []
    outs = [pk.out(p) for p in prefills]
    arr = (P.PercentileItem * max(1, len(items)))()
    for i, it in enumerate(items):
        _fill(pk, arr[i], it, keep, outs[it["out"]].data_ptr())
    if mutate:
        mutate(arr)
    dev_items = pk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    st = pk.k["count"](dev_items.data_ptr(), C.addressof(arr), len(items) if nitems is None else nitems, wgs, pk.stream)
    _status(st, expect_status)
    return [pk.back64(o, len(p)) for o, p in zip(outs, prefills)]


def _model(items, prefills):
    exp = [np.asarray(p, np.uint64).copy() for p in prefills]
    for it in items:
        exp[it["out"]] = P.count(it["selected"], it["ids"], it["card"], exp[it["out"]])
    return exp


def _check(pk, items, prefills, wgs=3):
    got = _run(pk, items, prefills, wgs)
    for g, e in zip(got, _model(items, prefills)):
        np.testing.assert_array_equal(g, e)
    return got


_CARD = {1: 2, 7: 128, 10: 300, 13: LDS, 14: LDS + 1, 17: 70000}  # 8192: LDS mode; 8193 and 70000: HBM mode


@pytest.mark.parametrize("num_docs", [0, 1, 31, 32, 33, 8191, 8192, 8193])
def test_sizes_densities_and_both_modes(pk, num_docs):
    """Densities 0, 0.03 (sparse words: rows read one by one), 0.5 and 1 (dense words: the whole word decoded); the
    mask bits at and past num_docs and the spare word are all ones (pack_mask), the padding rows hold dictId 0."""
    rng = np.random.default_rng(num_docs)
    for bits, card in _CARD.items():
        for density in (0, 0.03, 0.5, 1):
            pre = _prefill(rng, card)
            it = _item(rng, num_docs, density, bits, card)
            got = _check(pk, [it], [pre])[0]
            assert got[0] == pre[0]
            assert int(got.sum() - pre.sum()) == int(it["selected"].sum())
            if density == 0 or num_docs == 0:
                np.testing.assert_array_equal(got, pre)


@pytest.mark.parametrize("card", [1, 33, LDS, LDS + 1])
def test_cardinalities(pk, card):
    """card 1; card 33; the largest LDS table and the smallest HBM one, with the last dictId counted.  dictIds at or
    past card in the data count nothing (the guard words behind the table stay as they were)."""
    rng = np.random.default_rng(card)
    n = 3 * 8192 + 37
    bits = _bits_for(card) + 1                      # the data can hold ids at and past card
    ids = rng.integers(min(1, card - 1), card + 3, n)
    ids[5] = card - 1
    it = {"selected": rng.random(n) < 0.5, "ids": ids, "bits": bits, "card": card, "out": 0}
    it["selected"][5] = True
    pre = _prefill(rng, card)
    got = _check(pk, [it], [pre])[0]
    assert got[card - 1] > pre[card - 1]
    assert int(got.sum() - pre.sum()) == int((it["selected"] & (ids < card)).sum())
    if card > 1:
        assert got[0] == pre[0]


@pytest.mark.parametrize("card", [100, 9000])
def test_contention_on_one_counter(pk, card):
    """8193 selected rows all holding one dictId, in LDS and in HBM mode: exactly 8193 more."""
    n = 8193
    it = {"selected": np.ones(n, bool), "ids": np.full(n, 77), "bits": _bits_for(card), "card": card, "out": 0}
    pre = _prefill(np.random.default_rng(card), card)
    for wgs in (1, 3):
        got = _check(pk, [it], [pre], wgs=wgs)[0]
        assert int(got[77]) == int(pre[77]) + 8193
        assert (np.delete(got, 77) == np.delete(pre, 77)).all()


@pytest.mark.parametrize("card", [4000, 20000])
def test_items_sharing_a_table_and_workgroups_per_item(pk, card):
    """Five items in one launch, two of them (segments sharing a dictionary) adding into one table; 1 and 3 workgroups
    per item give the same counters."""
    rng = np.random.default_rng(card)
    bits = _bits_for(card)
    items = [_item(rng, 20000, 0.5, bits, card, out=0),
             _item(rng, 300, 1, 7, 100, out=1),
             _item(rng, 8192, 0, 10, 300, out=2),           # an empty item between two full ones
             _item(rng, 8193, 0.03, bits, card, out=0),     # the same dictionary: adds into the first item's table
             _item(rng, 1, 1, 3, 8, out=3)]
    pres = [_prefill(rng, c) for c in (card, 100, 300, 8)]
    got = [_check(pk, items, pres, wgs=w) for w in (1, 3)]
    for a, b in zip(*got):
        assert a.tobytes() == b.tobytes()
    np.testing.assert_array_equal(got[0][2], pres[2])
    assert int(got[0][0].sum() - pres[0].sum()) == int(items[0]["selected"].sum() + items[3]["selected"].sum())


@pytest.mark.parametrize("card", [300, LDS + 1])
def test_a_counter_carries_into_its_high_word(pk, card):
    """A pre-filled counter of 2^32 - 1: the HBM add (and the LDS mode's flush) is a 64-bit add."""
    rng = np.random.default_rng(card + 1)
    it = _item(rng, 5000, 1, _bits_for(card), card)
    it["ids"][:40] = 9
    pre = _prefill(rng, card)
    pre[9] = (1 << 32) - 1
    got = _check(pk, [it], [pre])[0]
    assert int(got[9]) == (1 << 32) - 1 + int((it["ids"] == 9).sum()) and int(got[9]) >> 32 == 1


# ---- pgx_percentile_count_group -----------------------------------------------------------------------------------------
def _group_cols(rng, n, gcards, locals0, ncols=2):
    """Column 0 holds local ids 0..locals0-1 remapped into 0..gcards[0]-1 with some entries -1; column 1 (when there is
    one) global ids as they are (a null remap), a few of them at or past gcards[1]: slots past the key space."""
    remap = rng.permutation(gcards[0])[:locals0].astype(np.int32)
    if locals0 > 2:
        remap[rng.integers(0, locals0, 2)] = -1
    cols = [(rng.integers(0, locals0, n), remap, _bits_for(locals0))]
    if ncols == 2:
        g1 = rng.integers(0, gcards[1], n)
        if n > 40:
            g1[rng.integers(0, n, 8)] = gcards[1] + 1   # slot >= slots whatever column 0 says
        cols.append((g1, None, _bits_for(gcards[1] + 2)))
    return cols


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


def _fill_gcols(pk, g, it, keep):
    for c, (ids, remap, gbits) in enumerate(it["g"]):
        fwd = pk.up(P.pack_fwd(ids, gbits, len(ids)))
        keep.append(fwd)
        g[c].fwd, g[c].bits = fwd.data_ptr(), gbits
        if remap is not None:
            rm = pk.up(remap)
            keep.append(rm)
            g[c].remap = rm.data_ptr()


def _run_group(pk, items, gcards, pre, wgs=3, expect_status=0, slots=None, mutate=None, ngcols=2, gmul1=None):
    true_slots = gcards[0] * (gcards[1] if ngcols == 2 else 1)
    table = pk.out(pre)
    keep = []
    arr = (P.PercentileGroupItem * max(1, len(items)))()
    for i, it in enumerate(items):
        _fill(pk, arr[i].d, it, keep, table.data_ptr())
        _fill_gcols(pk, arr[i].g, it, keep)
    if mutate:
        mutate(arr)
    gmul = (C.c_uint64 * 2)(1, gcards[0] if gmul1 is None else gmul1)
    dev_items = pk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    st = pk.k["count_group"](dev_items.data_ptr(), C.addressof(arr), len(items), ngcols, C.addressof(gmul),
                             true_slots if slots is None else slots, wgs, pk.stream)
    _status(st, expect_status)
    return pk.back64(table, pre.size).reshape(pre.shape)


@pytest.mark.parametrize("gcards,card,ncols", [
    ((1, 1), 300, 2), ((7, 1), 300, 1),              # one group column (with a remap)
    ((2, 1), 4096, 2), ((3, 1), 2731, 2),            # slots x card 8192 (LDS) and 8193 (HBM)
    ((257, 3), 10, 2), ((257, 3), 3000, 2),          # 771 slots, in LDS and in HBM
    ((256, 256), 2, 2)])                             # 65536 slots (the limit) with card 2
def test_group_counts(pk, gcards, card, ncols):
    """Two items (segments with their own remap tables) share the table; a remap entry of -1 and a slot at or past
    `slots` count nothing; 1 and 3 workgroups per item give the same counters."""
    rng = np.random.default_rng(gcards[0] * 1000 + gcards[1] + card)
    slots = gcards[0] * (gcards[1] if ncols == 2 else 1)
    items = []
    for n, density in ((3 * 8192 + 37, 0.5), (8193, 0.03)):
        it = _item(rng, n, density, _bits_for(card), card)
        it["g"] = _group_cols(rng, n, gcards, max(1, gcards[0] - gcards[0] // 3), ncols)
        items.append(it)
    pre = _prefill(rng, card, slots).reshape(slots, card)
    exp = pre.copy()
    for it in items:
        exp = P.count_group(it["selected"], it["ids"], card, _slots_of(it, gcards), slots, exp)
    outs = [_run_group(pk, items, gcards, pre, wgs=w, ngcols=ncols) for w in (1, 3)]
    np.testing.assert_array_equal(outs[1], exp)
    assert outs[0].tobytes() == outs[1].tobytes()
    assert (outs[1][:, 0] == pre[:, 0]).all()  # padding rows, bits past num_docs, the spare word
    assert exp.sum() > pre.sum()


def test_group_ids_past_card_count_nothing(pk):
    rng = np.random.default_rng(23)
    gcards = (5, 4)
    n = 9000
    it = {"selected": np.ones(n, bool), "ids": rng.integers(1, 64, n), "bits": 6, "card": 33, "out": 0}
    it["g"] = _group_cols(rng, n, gcards, 5)
    pre = np.zeros((20, 33), np.uint64)
    got = _run_group(pk, [it], gcards, pre)
    np.testing.assert_array_equal(got, P.count_group(it["selected"], it["ids"], 33, _slots_of(it, gcards), 20, pre))


# ---- the multi-value forms -------------------------------------------------------------------------------------------
def _mv_item(rng, ndocs, density, card, out=0):
    """Docs with 0, 1, 2, 3 values, one with 70 and one with 300."""
    counts = rng.integers(0, 4, ndocs)
    if ndocs > 40:
        counts[17], counts[40] = 300, 70
    total = int(counts.sum())
    ids = rng.integers(1, card, total) if card > 1 else np.zeros(total, np.int64)
    return {"selected": _selected(rng, ndocs, density), "counts": counts, "ids": ids, "bits": _bits_for(card),
            "card": card, "out": out, "rows": max(total, 1), "total": total}


def _fill_mv(pk, m, it, keep, start=None):
    st = pk.up(M.starts(it["counts"]) if start is None else start)
    keep.append(st)
    m.start, m.total = st.data_ptr(), it["total"]


def _run_mv(pk, items, prefills, wgs=3, expect_status=0, mutate=None, starts=None):
    keep = []
    outs = [pk.out(p) for p in prefills]
    arr = (P.PercentileMvItem * max(1, len(items)))()
    for i, it in enumerate(items):
        _fill(pk, arr[i].d, it, keep, outs[it["out"]].data_ptr())
        _fill_mv(pk, arr[i], it, keep, None if starts is None else starts[i])
    if mutate:
        mutate(arr)
    dev_items = pk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    st = pk.k["count_mv"](dev_items.data_ptr(), C.addressof(arr), len(items), wgs, pk.stream)
    _status(st, expect_status)
    return [pk.back64(o, len(p)) for o, p in zip(outs, prefills)]


@pytest.mark.parametrize("ndocs", [0, 1, 33, 8193])
def test_mv_counts_every_value_of_every_selected_doc(pk, ndocs):
    rng = np.random.default_rng(100 + ndocs)
    for card in (300, LDS + 1):
        for density in (0, 0.03, 0.5, 1):  # density 1: a fully selected word is one range
            it = _mv_item(rng, ndocs, density, card)
            pre = _prefill(rng, card)
            outs = [_run_mv(pk, [it], [pre], wgs=w)[0] for w in (1, 3)]
            exp = P.count_mv(it["selected"], it["counts"], it["ids"], card, pre)
            np.testing.assert_array_equal(outs[1], exp)
            assert outs[0].tobytes() == outs[1].tobytes()
            assert exp[0] == pre[0]
            assert int(exp.sum() - pre.sum()) == int(it["counts"][it["selected"]].sum())


@pytest.mark.parametrize("card", [300, LDS + 1])
def test_mv_ranges_are_clamped_to_the_stream(pk, card):
    """start[] ends past the row count: the rows at and past `total` are never read (they hold dictId 0 here, the
    padding, whose counter keeps its pre-fill), whatever start[] says; and a `total` that cuts the last docs short."""
    rng = np.random.default_rng(31)
    it = _mv_item(rng, 5000, 1, card)
    start = M.starts(it["counts"]).copy()
    start[-10:] += 100000
    short = dict(it, total=it["total"] - 50)
    for item in (it, short):
        pre = _prefill(rng, card)
        got = _run_mv(pk, [item], [pre], starts=[start])[0]
        exp_rows = M.value_rows(item["selected"], item["counts"]) & (np.arange(len(item["ids"])) < item["total"])
        # the last ten docs' ranges now run to the end of the stream
        exp_rows[M.starts(item["counts"])[-11]:item["total"]] = True
        np.testing.assert_array_equal(got, P.count(exp_rows, item["ids"], card, pre))
        assert got[0] == pre[0]
    pre = _prefill(rng, card)
    got = _run_mv(pk, [short], [pre])[0]  # the true start[], the short total
    np.testing.assert_array_equal(got, P.count_mv(short["selected"], short["counts"], short["ids"], card, pre,
                                                  total=short["total"]))


def _run_mv_group(pk, items, gcards, pre, wgs=3, expect_status=0, slots=None, mutate=None, ngcols=2):
    true_slots = gcards[0] * gcards[1]
    table = pk.out(pre)
    keep = []
    arr = (P.PercentileMvGroupItem * max(1, len(items)))()
    for i, it in enumerate(items):
        _fill(pk, arr[i].g.d, it, keep, table.data_ptr())
        _fill_gcols(pk, arr[i].g.g, it, keep)
        _fill_mv(pk, arr[i], it, keep)
    if mutate:
        mutate(arr)
    gmul = (C.c_uint64 * 2)(1, gcards[0])
    dev_items = pk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    st = pk.k["count_mv_group"](dev_items.data_ptr(), C.addressof(arr), len(items), ngcols, C.addressof(gmul),
                                true_slots if slots is None else slots, wgs, pk.stream)
    _status(st, expect_status)
    return pk.back64(table, pre.size).reshape(pre.shape)


@pytest.mark.parametrize("gcards,card", [((1, 1), 1000), ((7, 5), 200), ((7, 5), 1000), ((256, 256), 2)])
def test_mv_group(pk, gcards, card):
    """35 slots x 200 values in LDS, x 1000 in HBM; 65536 slots with card 2."""
    rng = np.random.default_rng(gcards[0] * 77 + gcards[1] + card)
    slots = gcards[0] * gcards[1]
    items = []
    for ndocs, density in ((8193, 0.5), (4000, 0.03), (0, 1)):
        it = _mv_item(rng, ndocs, density, card)
        it["g"] = _group_cols(rng, ndocs, gcards, max(1, gcards[0] - gcards[0] // 3))
        items.append(it)
    pre = _prefill(rng, card, slots).reshape(slots, card)
    exp = pre.copy()
    for it in items:
        exp = P.count_mv_group(it["selected"], it["counts"], it["ids"], card, _slots_of(it, gcards), slots, exp)
    outs = [_run_mv_group(pk, items, gcards, pre, wgs=w) for w in (1, 3)]
    np.testing.assert_array_equal(outs[1], exp)
    assert outs[0].tobytes() == outs[1].tobytes()
    if card > 1:
        assert (exp[:, 0] == pre[:, 0]).all()


# ---- pgx_percentile_sizes / pgx_percentile_emit -----------------------------------------------------------------------
def _sizes_emit(pk, table, rows, slots=None, wgs=5, cap_less=0, per_row=1):
    card = table.shape[1]
    slots = table.shape[0] if slots is None else slots
    tdev, rdev = pk.up(table), pk.up(np.asarray(rows, np.int64))
    sbuf = pk.out(np.full(len(rows), S32, np.uint32))
    assert pk.k["sizes"](tdev.data_ptr(), card, rdev.data_ptr(), len(rows), slots, sbuf.data_ptr(), wgs, pk.stream) == 0
    sizes = pk.back(sbuf, len(rows)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cap = max(int(off[-1]) - cap_less, 0)
    ibuf, cbuf = pk.out(np.full(cap, S32, np.uint32)), pk.out(np.full(2 * cap, S32, np.uint32))
    odev = pk.up(off[:-1].copy() if len(rows) else np.zeros(1, np.int64))
    assert pk.k["emit"](tdev.data_ptr(), card, rdev.data_ptr(), odev.data_ptr(), len(rows), slots, ibuf.data_ptr(),
                        cbuf.data_ptr(), cap, per_row, wgs, pk.stream) == 0
    return sizes, pk.back(ibuf, cap).view(np.int32), pk.back64(cbuf, cap), off


@pytest.mark.parametrize("card", [1, 255, 256, 257, 3 * 256 + 1])
def test_sizes_and_emit(pk, card):
    """A row of all zeros, a full row, the last counter alone, sparse rows, a counter above 2^32, a non-contiguous row
    list with a repeat and a row outside the table; the pairs are in exactly ascending dictId order, whatever the
    grid."""
    rng = np.random.default_rng(card)
    table = np.zeros((6, card), np.uint64)
    table[1] = rng.integers(1, 1000, card)
    table[2, -1] = 5
    table[4] = np.where(rng.random(card) < 0.5, rng.integers(1, 1000, card), 0)
    table[5] = np.where(rng.random(card) < 0.1, rng.integers(1, 1000, card), 0)
    table[5, card // 2] = (1 << 40) + 3
    rows = [5, 0, 2, 1, 4, 2, 9, 3, -1]
    results = []
    for wgs, per_row in ((1, 1), (5, 2), (5, 3), (64, 1), (2, 64)):  # (more workgroups per row than 256-counter steps)
        sizes, ids, counts, off = _sizes_emit(pk, table, rows, wgs=wgs, per_row=per_row)
        for i, r in enumerate(rows):
            eids, ecounts = P.nonzero_pairs(table[r]) if 0 <= r < 6 else (np.zeros(0, np.int32), np.zeros(0, np.uint64))
            assert sizes[i] == len(eids)
            np.testing.assert_array_equal(ids[off[i]:off[i + 1]], eids)
            np.testing.assert_array_equal(counts[off[i]:off[i + 1]], ecounts)
        results.append(ids.tobytes() + counts.tobytes())
    assert len(set(results)) == 1
    assert sizes[1] == 0 and sizes[3] == card and sizes[2] == 1 and sizes[6] == 0 and sizes[8] == 0


def test_emit_never_writes_past_its_capacity(pk):
    rng = np.random.default_rng(41)
    table = np.where(rng.random((3, 1000)) < 0.5, rng.integers(1, 1000, (3, 1000)), 0).astype(np.uint64)
    _, ids, counts, _ = _sizes_emit(pk, table, [0, 1, 2], per_row=2)
    _, sids, scounts, _ = _sizes_emit(pk, table, [0, 1, 2], cap_less=7, per_row=2)  # (back() checks the guards)
    np.testing.assert_array_equal(sids, ids[:-7])
    np.testing.assert_array_equal(scounts, counts[:-7])


# ---- launchers -------------------------------------------------------------------------------------------------------
def test_launchers_refuse_bad_arguments(pk):
    """Null pointers, a negative or too large count, bits outside 1..32, card < 1, slots < 1 or above the limit, gmul
    outside 1..slots, a negative stream row count, a zero grid: a status, no launch, every buffer left as it was."""
    rng = np.random.default_rng(14)
    it = _item(rng, 100, 1, 7, 100)
    pre = np.full(100, 0xA5A5A5A5A5A5A5A5, np.uint64)

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
        got = _run(pk, [it], [pre], kw.pop("wgs"), expect_status=P.INVALID_VALUE, **kw)[0]
        assert (got == pre).all()
    arr = (P.PercentileItem * 1)()
    assert pk.k["count"](None, C.addressof(arr), 1, 1, pk.stream) == P.INVALID_VALUE
    assert pk.k["count"](pk.up(np.zeros(64, np.uint8)).data_ptr(), None, 1, 1, pk.stream) == P.INVALID_VALUE
    assert pk.k["count"](pk.up(np.zeros(64, np.uint8)).data_ptr(), C.addressof(arr), 0, 1, pk.stream) == 0  # no items

    gcards = (3, 2)
    git = dict(it, g=_group_cols(rng, 100, gcards, 3))
    gpre = np.full((6, 100), 0xA5A5A5A5A5A5A5A5, np.uint64)

    def gbits(value, path):
        def f(arr):
            o = arr[0]
            for p in path:
                o = getattr(o, p)
            o[1].bits = value
        return f

    group = [{"wgs": 0}, {"slots": 0}, {"slots": -5}, {"slots": P.MAX_GROUP_SLOTS + 1}, {"ngcols": 0},
             {"ngcols": P.MAX_GROUP_COLS + 1}, {"gmul1": 0}, {"gmul1": 7}]
    for kw in group + [{"mutate": setter("num_docs", -1, ("d",))}, {"mutate": setter("bits", 33, ("d",))},
                       {"mutate": setter("card", 0, ("d",))}, {"mutate": setter("out", None, ("d",))},
                       {"mutate": gbits(0, ("g",))}, {"mutate": gbits(33, ("g",))}]:
        if "ngcols" in kw or "slots" in kw:  # (the helper derives the true slot count from ngcols)
            kw = dict(kw, slots=kw.get("slots", 6))
        got = _run_group(pk, [git], gcards, gpre, expect_status=P.INVALID_VALUE, **kw)
        assert (got == gpre).all()

    mit = _mv_item(rng, 100, 1, 100)
    for mut in (setter("total", -1), setter("start", None), setter("card", 0, ("d",)), setter("bits", 0, ("d",))):
        got = _run_mv(pk, [mit], [pre], expect_status=P.INVALID_VALUE, mutate=mut)[0]
        assert (got == pre).all()
    assert (_run_mv(pk, [mit], [pre], wgs=0, expect_status=P.INVALID_VALUE)[0] == pre).all()
    mgit = dict(mit, g=_group_cols(rng, 100, gcards, 3))
    for kw in ({"wgs": 0}, {"slots": 0}, {"slots": P.MAX_GROUP_SLOTS + 1}, {"ngcols": 0},
               {"mutate": setter("total", -1)}, {"mutate": setter("start", None)},
               {"mutate": setter("card", 0, ("g", "d"))}, {"mutate": gbits(33, ("g", "g"))}):
        got = _run_mv_group(pk, [mgit], gcards, gpre, expect_status=P.INVALID_VALUE, **kw)
        assert (got == gpre).all()

    table = pk.up(np.zeros((4, 100), np.uint64))
    rows, off = pk.up(np.arange(4, dtype=np.int64)), pk.up(np.zeros(4, np.int64))
    out, out64 = pk.out(np.full(16, S32, np.uint32)), pk.out(np.full(32, S32, np.uint32))
    t, r, o, ip, cp = table.data_ptr(), rows.data_ptr(), off.data_ptr(), out.data_ptr(), out64.data_ptr()
    for args in ((None, 100, r, 4, 4, ip, 1), (t, 0, r, 4, 4, ip, 1), (t, 100, None, 4, 4, ip, 1),
                 (t, 100, r, -1, 4, ip, 1), (t, 100, r, 4, 0, ip, 1), (t, 100, r, 4, P.MAX_GROUP_SLOTS + 1, ip, 1),
                 (t, 100, r, 4, 4, None, 1), (t, 100, r, 4, 4, ip, 0)):
        assert pk.k["sizes"](*args, pk.stream) == P.INVALID_VALUE
    for args in ((None, 100, r, o, 4, 4, ip, cp, 16, 1, 1), (t, 0, r, o, 4, 4, ip, cp, 16, 1, 1),
                 (t, 100, None, o, 4, 4, ip, cp, 16, 1, 1), (t, 100, r, None, 4, 4, ip, cp, 16, 1, 1),
                 (t, 100, r, o, -1, 4, ip, cp, 16, 1, 1), (t, 100, r, o, 4, 0, ip, cp, 16, 1, 1),
                 (t, 100, r, o, 4, 4, None, cp, 16, 1, 1), (t, 100, r, o, 4, 4, ip, None, 16, 1, 1),
                 (t, 100, r, o, 4, 4, ip, cp, -1, 1, 1), (t, 100, r, o, 4, 4, ip, cp, 16, 1, 0),
                 (t, 100, r, o, 4, 4, ip, cp, 16, 0, 1), (t, 100, r, o, 4, 4, ip, cp, 16, 1025, 1)):
        assert pk.k["emit"](*args, pk.stream) == P.INVALID_VALUE
    assert (pk.back(out, 16) == S32).all() and (pk.back(out64, 32) == S32).all()


def test_every_stored_width(pk):
    """Widths 1 .. 32 over 100 docs (three full mask words and a partial one), each with a sparse selection (three
    rows of every word, the index's last row among them: rows are read one by one) and a dense one (whole words are
    decoded).  Half the ids use the whole width, so a wrongly cut row counts elsewhere or lands past card."""
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
            pre.append(_prefill(rng, card))
    got = _check(pk, items, pre, wgs=2)
    assert all((g != p).any() for g, p in zip(got, pre))
