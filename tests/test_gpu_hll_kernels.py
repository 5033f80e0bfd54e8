"""The DISTINCTCOUNTHLL kernels (pinot_amd/csrc/pgx_hll.hip: pgx_hll_offer, pgx_hll_offer_group, pgx_hll_narrow)
launched directly on torch device buffers and compared with the numpy model of tests/hll_ref.py.  Every output is
pre-filled and has guard words past its end, which must come back untouched.  The comparisons are exact: an offer is a
register-wise max, so neither the grid size nor the scheduling can change a byte.

The kernels take the code table as data, so most cases use synthetic tables: dictId 0, which is what the padding rows
of a forward index decode to, then owns register 255 with the top rank while every other dictId stays in registers
0..254 -- a padding row, a mask bit at or past num_docs or the spare mask word read as rows would show there."""
import ctypes as C

import numpy as np
import pytest

from pinot_amd import hll as H
from tests import hll_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
S32 = np.int32(-1515870811)            # 0xA5A5A5A5


class _HK:
    def __init__(self):
        import torch
        from pinot_amd import native as N
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.offer, self.offer_group, self.narrow = R.bind(N.lib())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.dev)

    def out(self, prefill):
        """A device buffer holding `prefill` (uint32) followed by GUARD sentinel words."""
        a = np.concatenate([np.asarray(prefill, np.uint32).reshape(-1), np.full(GUARD, S32.view(np.uint32), np.uint32)])
        return self.up(a)

    def back(self, buf, n):
        """The buffer's first n words, after checking the guard words behind them."""
        self.torch.cuda.synchronize(self.dev)
        a = buf.cpu().numpy().view(np.uint32)
        assert len(a) == n + GUARD and (a[n:] == S32.view(np.uint32)).all()
        return a[:n]


@pytest.fixture(scope="module")
def hk():
    return _HK()


def _table(rng, card):
    """Synthetic codes: dictId 0 -> register 255, rank 25; every other dictId a register 0..254, rank 1..25."""
    t = ((rng.integers(0, 255, card).astype(np.uint32) << 8) | rng.integers(1, R.MAX_RANK + 1, card).astype(np.uint32))
    t[0] = (255 << 8) | R.MAX_RANK
    return t.astype(np.uint16)


def _selected(rng, n, density):
    if density == 0:
        return np.zeros(n, bool)
    if density == 1:
        return np.ones(n, bool)
    return rng.random(n) < density


def _item(rng, n, density, bits, card, out=0):
    ids = rng.integers(1, card, n) if card > 1 else np.zeros(n, np.int64)
    return {"selected": _selected(rng, n, density), "ids": ids, "bits": bits, "codes": _table(rng, card), "out": out}


def _prefill(rng):
    p = rng.integers(0, R.MAX_RANK + 1, R.REGS).astype(np.uint32)
    p[255] = 0  # where a row that must not count would show
    return p


def _model(items, prefills):
    exp = [np.asarray(p, np.uint32).copy() for p in prefills]
    for it in items:
        exp[it["out"]] = R.offer(it["selected"], it["ids"], it["codes"], exp[it["out"]])
    return exp


def _fill(hk, arr, i, it, keep, out_ptr, h=None):
    h = arr[i] if h is None else h
    n = len(it["selected"])
    mask, fwd, codes = hk.up(R.pack_mask(it["selected"])), hk.up(R.pack_fwd(it["ids"], it["bits"], n)), hk.up(it["codes"])
    keep += [mask, fwd, codes]
    h.sel, h.fwd, h.codes, h.out = mask.data_ptr(), fwd.data_ptr(), codes.data_ptr(), out_ptr
    h.bits, h.num_docs, h.ncodes = it["bits"], n, len(it["codes"])


def _run(hk, items, prefills, wgs, expect_status=0, mutate=None, nitems=None):
    """pgx_hll_offer over `items` into len(prefills) outputs; returns the outputs (uint32[256] each)."""
    keep = []
    outs = [hk.out(p) for p in prefills]
    arr = (R.HllItem * max(1, len(items)))()
    for i, it in enumerate(items):
        _fill(hk, arr, i, it, keep, outs[it["out"]].data_ptr())
    if mutate:
        mutate(arr)
    dev_items = hk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    st = hk.offer(dev_items.data_ptr(), C.addressof(arr), len(items) if nitems is None else nitems, wgs, hk.stream)
    assert (st == 0) == (expect_status == 0) and (expect_status == 0 or st == expect_status)
    return [hk.back(o, R.REGS).copy() for o in outs]


def _check(hk, items, prefills, wgs=3):
    got = _run(hk, items, prefills, wgs)
    for g, e in zip(got, _model(items, prefills)):
        np.testing.assert_array_equal(g, e)
    return got


_CARD = {1: 1, 7: 128, 10: 300, 17: 70000, 32: 70000}  # 70,000 codes: a 140 KB table


@pytest.mark.parametrize("num_docs", [1, 31, 32, 33, 8191, 8192, 8193, 3 * 8192 + 37])
def test_sizes_densities_and_widths(hk, num_docs):
    """Densities 0, 0.02 (sparse words: rows read one by one), 0.5 and 1 (dense words: the whole word decoded); the
    mask bits at and past num_docs and the spare word are all ones (R.pack_mask), the padding rows hold dictId 0."""
    rng = np.random.default_rng(num_docs)
    for bits in (1, 7, 10, 17, 32):
        for density in (0, 0.02, 0.5, 1):
            pre = _prefill(rng)
            it = _item(rng, num_docs, density, bits, _CARD[bits])
            got = _check(hk, [it], [pre])[0]
            if _CARD[bits] > 1:
                assert got[255] == 0
            assert (got >= pre).all() and got.max() <= R.MAX_RANK
            if density == 0:
                np.testing.assert_array_equal(got, pre)


def test_cardinality_one_feeds_one_register(hk):
    rng = np.random.default_rng(5)
    n = 20000
    it = {"selected": np.ones(n, bool), "ids": np.zeros(n, np.int64), "bits": 1,
          "codes": np.array([(17 << 8) | 9], np.uint16), "out": 0}
    got = _check(hk, [it], [np.zeros(R.REGS, np.uint32)])[0]
    assert got[17] == 9 and got.sum() == 9


def test_real_codes_give_from_ints_registers(hk):
    """The codes of 300 INT values and of 70,000 LONG values: the registers are hll.from_ints of the selected rows'
    hash codes."""
    from pinot_amd import extended as X
    rng = np.random.default_rng(6)
    for dtype, card, bits in (("INT", 300, 9), ("LONG", 70000, 17)):
        vals = np.unique(rng.integers(-(1 << 40) if dtype == "LONG" else -(1 << 31), 1 << 31, card * 2))[:card]
        rng.shuffle(vals)
        n = 3 * 8192 + 37
        it = {"selected": rng.random(n) < 0.5, "ids": rng.integers(0, card, n), "bits": bits,
              "codes": R.codes(dtype, vals.tolist()), "out": 0}
        got = _check(hk, [it], [np.zeros(R.REGS, np.uint32)])[0]
        hashes = {X.java_hash_code(dtype, int(v)) for v in vals[np.unique(it["ids"][it["selected"]])]}
        np.testing.assert_array_equal(got.astype(np.uint8), H.from_ints(hashes))


def test_workgroups_per_item_do_not_change_the_result(hk):
    rng = np.random.default_rng(11)
    it = _item(rng, 3 * 8192 + 37, 0.5, 17, 70000)
    pre = _prefill(rng)
    outs = [_check(hk, [it], [pre], wgs=w)[0] for w in (1, 3, 64)]
    assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()


def test_five_items_in_one_launch_two_sharing_an_output(hk):
    rng = np.random.default_rng(12)
    items = [_item(rng, 20000, 0.5, 12, 4000, out=0),
             _item(rng, 300, 1, 7, 100, out=1),
             _item(rng, 8192, 0, 10, 300, out=2),           # an empty item between two full ones
             _item(rng, 8193, 0.02, 17, 70000, out=0),      # maxes into the first item's registers
             _item(rng, 1, 1, 3, 8, out=3)]
    pres = [_prefill(rng) for _ in range(4)]
    got = _check(hk, items, pres, wgs=4)
    np.testing.assert_array_equal(got[2], pres[2])
    alone = _model([items[0]], [pres[0]])[0]
    assert (got[0] >= alone).all() and (got[0] != alone).any()


def test_ids_past_the_table_are_never_looked_up(hk):
    """ncodes bounds the gather: rows whose dictId lies at or past it offer nothing."""
    rng = np.random.default_rng(13)
    it = _item(rng, 9000, 1, 10, 300)
    short = dict(it, codes=it["codes"][:100].copy())
    got = _run(hk, [short], [np.zeros(R.REGS, np.uint32)], 2)[0]
    keep = dict(it, selected=it["selected"] & (it["ids"] < 100))
    np.testing.assert_array_equal(got, _model([keep], [np.zeros(R.REGS, np.uint32)])[0])


# ---- pgx_hll_offer_group ---------------------------------------------------------------------------------------------
def _group_item(rng, n, density, bits, card, gcards, locals0):
    """Two group columns: column 0 holds local ids 0..locals0-1 remapped (injectively) into 0..gcards[0]-1, column 1
    global ids as they are."""
    it = _item(rng, n, density, bits, card)
    remap = rng.permutation(gcards[0])[:locals0].astype(np.int32)
    it["g"] = [(rng.integers(0, locals0, n), remap, max(1, int(locals0 - 1).bit_length())),
               (rng.integers(0, gcards[1], n), None, max(1, int(gcards[1] - 1).bit_length()))]
    return it


def _run_group(hk, items, gcards, prefill=None, wgs=3, expect_status=0, slots=None, mutate=None, ngcols=2):
    true_slots = gcards[0] * gcards[1]
    pre = np.zeros((true_slots, R.REGS), np.uint32) if prefill is None else prefill
    table = hk.out(pre)
    keep = []
    arr = (R.HllGroupItem * max(1, len(items)))()
    for i, it in enumerate(items):
        _fill(hk, arr, i, it, keep, table.data_ptr(), arr[i].h)
        for g, (ids, remap, gbits) in enumerate(it["g"]):
            fwd = hk.up(R.pack_fwd(ids, gbits, len(ids)))
            keep.append(fwd)
            arr[i].g[g].fwd, arr[i].g[g].bits = fwd.data_ptr(), gbits
            if remap is not None:
                rm = hk.up(remap)
                keep.append(rm)
                arr[i].g[g].remap = rm.data_ptr()
    if mutate:
        mutate(arr)
    gmul = (C.c_uint64 * 2)(1, gcards[0])
    dev_items = hk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    st = hk.offer_group(dev_items.data_ptr(), C.addressof(arr), len(items), ngcols, C.addressof(gmul),
                        true_slots if slots is None else slots, wgs, hk.stream)
    assert (st == 0) == (expect_status == 0) and (expect_status == 0 or st == expect_status)
    got = hk.back(table, true_slots * R.REGS).reshape(true_slots, R.REGS)
    return got, pre, table


def _group_model(items, gcards, pre):
    exp = pre.copy()
    for it in items:
        slot = R.group_slots([(ids, remap) for ids, remap, _ in it["g"]], (1, gcards[0]))
        exp = R.offer_group(it["selected"], it["ids"], it["codes"], slot, gcards[0] * gcards[1], exp)
    return exp


@pytest.mark.parametrize("gcards", [(1, 1), (2, 1), (257, 1), (256, 256)])
def test_group_slots(hk, gcards):
    """slots 1, 2, 257 and 65536 (the limit); two items (segments with their own remap tables and code tables) share
    the table; only the registers of (slot, register) pairs the model touches are non-zero."""
    rng = np.random.default_rng(gcards[0] * 1000 + gcards[1])
    items = [_group_item(rng, 3 * 8192 + 37, 0.5, 17, 70000, gcards, max(1, gcards[0] - gcards[0] // 3)),
             _group_item(rng, 8193, 0.02, 10, 300, gcards, gcards[0])]
    got, pre, _ = _run_group(hk, items, gcards)
    exp = _group_model(items, gcards, pre)
    np.testing.assert_array_equal(got, exp)
    assert (got[:, 255] == 0).all()  # padding rows, bits past num_docs, the spare word


@pytest.mark.parametrize("gcards", [(5, 3), (256, 256)])
def test_group_keys_outside_the_space_offer_nothing(hk, gcards):
    """A remap entry of -1 in column 0 and global ids at and just past gcards[1] in column 1 (null remap): those rows
    offer nothing, on the row-by-row path (density 0.05) and the whole-word path (0.9) alike, whatever the grid; the
    last mask word is partial."""
    rng = np.random.default_rng(31 + gcards[0])
    n, slots = 3001, gcards[0] * gcards[1]
    for density in (0.05, 0.9):
        it = _group_item(rng, n, density, 12, 4000, gcards, gcards[0])
        ids0, remap, bits0 = it["g"][0]
        remap = remap.copy()
        remap[[1, len(remap) - 1]] = -1             # (every local id stays inside the table)
        ids1 = it["g"][1][0].copy()
        past = rng.random(n) < 0.05
        ids1[past] = gcards[1] + rng.integers(0, 2, int(past.sum()))
        it["g"] = [(ids0, remap, bits0), (ids1, None, int(gcards[1] + 1).bit_length())]
        slot = R.group_slots([(ids0, remap), (ids1, None)], (1, gcards[0]))
        bad = (remap[ids0] < 0) | (ids1 >= gcards[1])
        assert (bad & it["selected"]).sum() > 2 and ((slot[~bad] >= 0) & (slot[~bad] < slots)).all()
        pre = np.zeros((slots, R.REGS), np.uint32)
        exp = R.offer_group(it["selected"] & ~bad, it["ids"], it["codes"], np.where(bad, -1, slot), slots, pre)
        for wgs in (1, 3):
            got, _, _ = _run_group(hk, [it], gcards, prefill=pre, wgs=wgs)  # (checks the guard words past the table)
            np.testing.assert_array_equal(got, exp)
        assert (got[:, 255] == 0).all() and got.any()


def test_group_table_is_maxed_into_and_grid_free(hk):
    rng = np.random.default_rng(21)
    gcards = (7, 5)
    items = [_group_item(rng, 20000, 1, 12, 4000, gcards, 5)]
    pre = rng.integers(0, R.MAX_RANK + 1, (35, R.REGS)).astype(np.uint32)
    pre[:, 255] = 0
    outs = []
    for w in (1, 3):
        got, _, _ = _run_group(hk, items, gcards, prefill=pre, wgs=w)
        np.testing.assert_array_equal(got, _group_model(items, gcards, pre))
        outs.append(got.tobytes())
    assert outs[0] == outs[1]


def test_narrow(hk):
    """pgx_hll_narrow: the listed slots' u32 registers as bytes, in list order."""
    rng = np.random.default_rng(22)
    slots = 300
    table = rng.integers(0, R.MAX_RANK + 1, (slots, R.REGS)).astype(np.uint32)
    pick = rng.permutation(slots)[:37].astype(np.int64)
    tdev, sdev = hk.up(table), hk.up(pick)
    out = hk.out(np.full(len(pick) * R.REGS // 4, S32.view(np.uint32), np.uint32))
    assert hk.narrow(tdev.data_ptr(), sdev.data_ptr(), len(pick), slots, out.data_ptr(), hk.stream) == 0
    got = hk.back(out, len(pick) * R.REGS // 4).view(np.uint8).reshape(len(pick), R.REGS)
    np.testing.assert_array_equal(got, table[pick].astype(np.uint8))
    for bad in ((-1, slots), (len(pick), 0), (len(pick), R.MAX_GROUP_SLOTS + 1)):
        out2 = hk.out(np.full(8, S32.view(np.uint32), np.uint32))
        assert hk.narrow(tdev.data_ptr(), sdev.data_ptr(), bad[0], bad[1], out2.data_ptr(), hk.stream) == R.INVALID_VALUE
        assert (hk.back(out2, 8) == S32.view(np.uint32)).all()


# ---- launchers -------------------------------------------------------------------------------------------------------
def test_launchers_refuse_bad_arguments(hk):
    """A negative count, bits outside 1..32, slots < 1 or above the limit, a zero grid: a status, no launch, every
    buffer left at its sentinel."""
    rng = np.random.default_rng(14)
    it = _item(rng, 100, 1, 7, 100)
    pre = np.full(R.REGS, S32.view(np.uint32), np.uint32)

    def setter(field, value):
        def f(arr):
            setattr(arr[0], field, value)
        return f

    for kw in ({"wgs": 0}, {"wgs": 3, "nitems": -1}, {"wgs": 3, "mutate": setter("num_docs", -1)},
               {"wgs": 3, "mutate": setter("bits", 0)}, {"wgs": 3, "mutate": setter("bits", 33)}):
        got = _run(hk, [it], [pre], kw.pop("wgs"), expect_status=R.INVALID_VALUE, **kw)[0]
        assert (got == pre).all()

    gcards = (3, 2)
    git = _group_item(rng, 100, 1, 7, 100, gcards, 3)
    gpre = np.full((6, R.REGS), S32.view(np.uint32), np.uint32)

    def hset(field, value):
        def f(arr):
            setattr(arr[0].h, field, value)
        return f

    def gbits(value):
        def f(arr):
            arr[0].g[1].bits = value
        return f

    for kw in ({"wgs": 0}, {"slots": 0}, {"slots": -5}, {"slots": R.MAX_GROUP_SLOTS + 1}, {"ngcols": 0},
               {"ngcols": R.MAX_GROUP_COLS + 1}, {"mutate": hset("num_docs", -1)}, {"mutate": hset("bits", 33)},
               {"mutate": gbits(0)}, {"mutate": gbits(33)}):
        got, _, _ = _run_group(hk, [git], gcards, prefill=gpre, expect_status=R.INVALID_VALUE, **kw)
        assert (got == gpre).all()
    # no items: nothing to launch, success
    assert hk.offer(hk.up(np.zeros(64, np.uint8)).data_ptr(), C.addressof((R.HllItem * 1)()), 0, 1, hk.stream) == 0


def test_every_stored_width(hk):
    """Widths 1 .. 32 over 100 docs (three full mask words and a partial one), each with a sparse selection (three
    rows of every word, the index's last row among them: rows are read one by one) and a dense one (whole words are
    decoded).  Half the ids use the whole width, so a wrongly cut row lands past the table (or on another code)."""
    rng = np.random.default_rng(17)
    n = 100
    sparse = np.zeros(n, bool)
    sparse[[1, 17, 31, 32, 40, 63, 64, 77, 95, 96, 98, n - 1]] = True
    items, model_items = [], []
    for bits in range(1, 33):
        card = min(1 << bits, 1 << 16)
        ids = np.where(rng.random(n) < 0.5, rng.integers(0, card, n).astype(np.uint64),
                       rng.integers(0, 1 << bits, n, dtype=np.uint64))
        ids[n - 1] = card - 1
        codes = _table(rng, card)
        for sel in (sparse, np.ones(n, bool)):
            items.append({"selected": sel, "ids": ids, "bits": bits, "codes": codes, "out": len(items)})
            model_items.append(dict(items[-1], selected=sel & (ids < card), ids=np.minimum(ids, card - 1)))
    pre = [np.zeros(R.REGS, np.uint32) for _ in items]
    got = _run(hk, items, pre, 2)
    for g, e in zip(got, _model(model_items, pre)):
        np.testing.assert_array_equal(g, e)
