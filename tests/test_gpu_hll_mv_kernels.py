"""The DISTINCTCOUNTHLLMV kernels (pinot_amd/csrc/pgx_hll.hip: pgx_hll_offer_mv, pgx_hll_offer_mv_group) launched
directly on torch device buffers and compared with the numpy model of tests/hll_mv_ref.py.  Every output is pre-filled
and has guard words past its end, which must come back untouched.  The comparisons are exact: an offer is a
register-wise max, so neither the grid size nor the scheduling can change a byte.

As in tests/test_gpu_hll_kernels.py the code tables are synthetic: dictId 0, which is what the padding rows of a value
stream decode to, owns register 255 with the top rank while real values use dictIds from 1 and registers 0..254 -- a
padding value row, a mask bit at or past num_docs, the spare mask word read as docs, or a start entry past index
num_docs (garbage here) used as a range bound would show there or fault the guard words."""
import ctypes as C

import numpy as np
import pytest

from pinot_amd import hll as H
from tests import hll_mv_ref as M
from tests import hll_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
S32 = np.int32(-1515870811)            # 0xA5A5A5A5
START_GARBAGE = np.array([0, 5, -7, 1 << 30, 3, 2147483647, 0, 1], np.int32)  # behind start[num_docs]


class _HK:
    def __init__(self):
        import torch
        from pinot_amd import native as N
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.offer, self.offer_group = M.bind(N.lib())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.dev)

    def out(self, prefill):
        a = np.concatenate([np.asarray(prefill, np.uint32).reshape(-1), np.full(GUARD, S32.view(np.uint32), np.uint32)])
        return self.up(a)

    def back(self, buf, n):
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


def _counts(rng, n, kind):
    """Values per doc: all 1; random 1..4; random 1..4 with a doc of 70 and a doc of 300 values (both longer than a
    batch of the kernel) as the first docs, the last docs, or on both sides of the first mask-word boundary."""
    if kind == "ones":
        return np.ones(n, np.int64), []
    c = rng.integers(1, 5, n).astype(np.int64)
    if kind == "rand":
        return c, []
    a = {"first": 0, "last": n - 2, "boundary": 31}[kind]
    long_docs = sorted({min(max(a, 0), n - 1), min(max(a + 1, 0), n - 1)})
    for d, k in zip(reversed(long_docs), (300, 70)):
        c[d] = k
    return c, long_docs


def _item(rng, n, density, bits, card, kind="rand", out=0):
    counts, long_docs = _counts(rng, n, kind)
    selected = np.zeros(n, bool) if density == 0 else (np.ones(n, bool) if density == 1 else rng.random(n) < density)
    if density != 0:
        selected[long_docs] = True
    total = int(counts.sum())
    ids = rng.integers(1, card, total) if card > 1 else np.zeros(total, np.int64)
    return {"selected": selected, "counts": counts, "ids": ids, "bits": bits, "codes": _table(rng, card), "out": out}


def _prefill(rng):
    p = rng.integers(0, R.MAX_RANK + 1, R.REGS).astype(np.uint32)
    p[255] = 0  # where a row that must not count would show
    return p


def _model(items, prefills):
    exp = [np.asarray(p, np.uint32).copy() for p in prefills]
    for it in items:
        exp[it["out"]] = M.offer(it["selected"], it["counts"], it["ids"], it["codes"], exp[it["out"]])
    return exp


def _fill(hk, m, h, it, keep, out_ptr):
    """m: the HllMvItem / HllMvGroupItem, h: its HllItem.  The last doc's range ends exactly at `total`; the stream is
    padded like a forward index of `total` rows (dictId 0), the start array is followed by garbage."""
    n, total = len(it["selected"]), len(it["ids"])
    start = M.starts(it["counts"])
    assert start[n] == total
    bufs = [hk.up(R.pack_mask(it["selected"])), hk.up(R.pack_fwd(it["ids"], it["bits"], total)), hk.up(it["codes"]),
            hk.up(np.concatenate([start, START_GARBAGE]))]
    keep += bufs
    h.sel, h.fwd, h.codes, h.out = bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), out_ptr
    h.bits, h.num_docs, h.ncodes = it["bits"], n, len(it["codes"])
    m.start, m.total = bufs[3].data_ptr(), total


def _run(hk, items, prefills, wgs, expect_status=0, mutate=None, nitems=None, null=None):
    """pgx_hll_offer_mv over `items` into len(prefills) outputs; returns the outputs (uint32[256] each)."""
    keep = []
    outs = [hk.out(p) for p in prefills]
    arr = (M.HllMvItem * max(1, len(items)))()
    for i, it in enumerate(items):
        _fill(hk, arr[i], arr[i].h, it, keep, outs[it["out"]].data_ptr())
    if mutate:
        mutate(arr)
    dev_items = hk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    st = hk.offer(None if null == "items" else dev_items.data_ptr(), None if null == "check" else C.addressof(arr),
                  len(items) if nitems is None else nitems, wgs, hk.stream)
    assert (st == 0) == (expect_status == 0) and (expect_status == 0 or st == expect_status)
    return [hk.back(o, R.REGS).copy() for o in outs]


def _check(hk, items, prefills, wgs=3):
    got = _run(hk, items, prefills, wgs)
    for g, e in zip(got, _model(items, prefills)):
        np.testing.assert_array_equal(g, e)
    return got


_CARD = {1: 1, 7: 128, 10: 300, 17: 70000, 32: 70000}  # 70,000 codes: a 140 KB table


@pytest.mark.parametrize("kinds", [("ones",), ("rand",), ("first", "last", "boundary")], ids=["ones", "rand", "long"])
@pytest.mark.parametrize("num_docs", [1, 31, 32, 33, 8191, 8192, 8193])
def test_sizes_counts_densities_and_widths(hk, num_docs, kinds):
    """Densities 0, 0.03 (single docs and short runs), 0.5 and 1 (every word one range).  The mask bits at and past
    num_docs and the spare word are all ones (R.pack_mask), the padding value rows hold dictId 0."""
    rng = np.random.default_rng(num_docs * 7 + len(kinds))
    for kind in kinds:
        for bits in (1, 7, 10, 17, 32):
            for density in (0, 0.03, 0.5, 1):
                pre = _prefill(rng)
                it = _item(rng, num_docs, density, bits, _CARD[bits], kind)
                got = _check(hk, [it], [pre])[0]
                if _CARD[bits] > 1:
                    assert got[255] == 0
                assert (got >= pre).all() and got.max() <= R.MAX_RANK
                if density == 0:
                    np.testing.assert_array_equal(got, pre)


def test_a_long_doc_alone_reaches_every_value(hk):
    """One selected doc of 300 values among unselected ones: its last values (past the whole batches) count."""
    rng = np.random.default_rng(3)
    it = _item(rng, 100, 0, 10, 300, "boundary")
    it["selected"][32] = True  # the doc of 300 values
    assert it["counts"][32] == 300
    first = int(M.starts(it["counts"])[32])
    it["ids"][first:first + 300] = 1
    it["ids"][first + 299] = 2    # only the last value of the doc holds dictId 2
    it["codes"][1], it["codes"][2] = (100 << 8) | 5, (200 << 8) | 20
    got = _check(hk, [it], [np.zeros(R.REGS, np.uint32)])[0]
    assert got[200] == 20 and np.count_nonzero(got) == 2


def test_cardinality_one_feeds_one_register(hk):
    n = 20000
    counts = np.full(n, 2, np.int64)
    it = {"selected": np.ones(n, bool), "counts": counts, "ids": np.zeros(2 * n, np.int64), "bits": 1,
          "codes": np.array([(17 << 8) | 9], np.uint16), "out": 0}
    got = _check(hk, [it], [np.zeros(R.REGS, np.uint32)])[0]
    assert got[17] == 9 and got.sum() == 9


def test_real_codes_give_from_ints_registers(hk):
    """The codes pgx_hll_codes computes for 300 INT and 70,000 LONG values: the registers are hll.from_ints of the
    selected docs' values' hash codes."""
    from pinot_amd import extended as X
    from pinot_amd import native as N
    rng = np.random.default_rng(6)
    for dtype, code, card, bits in (("INT", N.PGX_INT, 300, 9), ("LONG", N.PGX_LONG, 70000, 17)):
        vals = np.unique(rng.integers(-(1 << 40) if dtype == "LONG" else -(1 << 31), 1 << 31, card * 2))[:card]
        rng.shuffle(vals)
        arr = vals.astype(np.int32 if dtype == "INT" else np.int64)
        codes = np.zeros(card, np.uint16)
        N.check(N.lib().pgx_hll_codes(code, arr.ctypes.data, None, card, codes.ctypes.data))
        np.testing.assert_array_equal(codes, R.codes(dtype, vals.tolist()))
        n = 8192 + 37
        counts = rng.integers(1, 5, n).astype(np.int64)
        it = {"selected": rng.random(n) < 0.5, "counts": counts, "ids": rng.integers(0, card, int(counts.sum())),
              "bits": bits, "codes": codes, "out": 0}
        got = _check(hk, [it], [np.zeros(R.REGS, np.uint32)])[0]
        rows = M.value_rows(it["selected"], counts)
        hashes = {X.java_hash_code(dtype, int(v)) for v in vals[np.unique(it["ids"][rows])]}
        np.testing.assert_array_equal(got.astype(np.uint8), H.from_ints(hashes))


def test_workgroups_per_item_do_not_change_the_result(hk):
    rng = np.random.default_rng(11)
    it = _item(rng, 3 * 8192 + 37, 0.5, 17, 70000, "boundary")
    pre = _prefill(rng)
    outs = [_check(hk, [it], [pre], wgs=w)[0] for w in (1, 3, 64)]
    assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()


def test_five_items_in_one_launch_two_sharing_an_output(hk):
    rng = np.random.default_rng(12)
    items = [_item(rng, 9000, 0.5, 12, 4000, "first", out=0),
             _item(rng, 300, 1, 7, 100, "last", out=1),
             _item(rng, 8192, 0, 10, 300, "rand", out=2),          # an empty item between two full ones
             _item(rng, 8193, 0.03, 17, 70000, "ones", out=0),     # maxes into the first item's registers
             _item(rng, 1, 1, 3, 8, "rand", out=3)]
    pres = [_prefill(rng) for _ in range(4)]
    got = _check(hk, items, pres, wgs=4)
    np.testing.assert_array_equal(got[2], pres[2])
    alone = _model([items[0]], [pres[0]])[0]
    assert (got[0] >= alone).all() and (got[0] != alone).any()


def test_ids_past_the_table_are_never_looked_up(hk):
    """ncodes bounds the gather: values whose dictId lies at or past it offer nothing."""
    rng = np.random.default_rng(13)
    it = _item(rng, 9000, 1, 10, 300)
    short = dict(it, codes=it["codes"][:100].copy())
    got = _run(hk, [short], [np.zeros(R.REGS, np.uint32)], 2)[0]
    keep = dict(it, ids=np.where(it["ids"] < 100, it["ids"], 0), codes=it["codes"].copy())
    keep["codes"][0] = 0  # the model's stand-in for "offers nothing": register 0, rank 0
    np.testing.assert_array_equal(got, _model([keep], [np.zeros(R.REGS, np.uint32)])[0])
    assert got[255] == 0 and got.any()


def test_start_entries_are_clamped_to_the_stream(hk):
    """`total` bounds every range: with a total smaller than start[num_docs] the rows at and past it are not read."""
    rng = np.random.default_rng(15)
    it = _item(rng, 500, 1, 10, 300, "ones")

    def shrink(arr):
        arr[0].total = 123

    got = _run(hk, [it], [np.zeros(R.REGS, np.uint32)], 2, mutate=shrink)[0]
    keep = dict(it, selected=np.arange(500) < 123)
    np.testing.assert_array_equal(got, _model([keep], [np.zeros(R.REGS, np.uint32)])[0])


# ---- pgx_hll_offer_mv_group ------------------------------------------------------------------------------------------
def _group_item(rng, n, density, bits, card, gcards, locals0, kind="rand", holes=False):
    """Two single-value group columns (one id per DOC): column 0 holds local ids 0..locals0-1 remapped (injectively)
    into 0..gcards[0]-1 -- with `holes` every third local id maps to -1 --, column 1 global ids as they are."""
    it = _item(rng, n, density, bits, card, kind)
    remap = rng.permutation(gcards[0])[:locals0].astype(np.int32)
    if holes:
        remap[::3] = -1
    it["g"] = [(rng.integers(0, locals0, n), remap, max(1, int(locals0 - 1).bit_length())),
               (rng.integers(0, gcards[1], n), None, max(1, int(gcards[1] - 1).bit_length()))]
    return it


def _run_group(hk, items, gcards, prefill=None, wgs=3, expect_status=0, slots=None, mutate=None, ngcols=2, gmul=None,
               null=None):
    true_slots = gcards[0] * gcards[1]
    pre = np.zeros((true_slots, R.REGS), np.uint32) if prefill is None else prefill
    table = hk.out(pre)
    keep = []
    arr = (M.HllMvGroupItem * max(1, len(items)))()
    for i, it in enumerate(items):
        _fill(hk, arr[i], arr[i].g.h, it, keep, table.data_ptr())
        for g, (ids, remap, gbits) in enumerate(it["g"]):
            fwd = hk.up(R.pack_fwd(ids, gbits, len(ids)))
            keep.append(fwd)
            arr[i].g.g[g].fwd, arr[i].g.g[g].bits = fwd.data_ptr(), gbits
            if remap is not None:
                rm = hk.up(remap)
                keep.append(rm)
                arr[i].g.g[g].remap = rm.data_ptr()
    if mutate:
        mutate(arr)
    gm = (C.c_uint64 * 2)(*((1, gcards[0]) if gmul is None else gmul))
    dev_items = hk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    st = hk.offer_group(None if null == "items" else dev_items.data_ptr(),
                        None if null == "check" else C.addressof(arr), len(items), ngcols,
                        None if null == "gmul" else C.addressof(gm), true_slots if slots is None else slots, wgs,
                        hk.stream)
    assert (st == 0) == (expect_status == 0) and (expect_status == 0 or st == expect_status)
    got = hk.back(table, true_slots * R.REGS).reshape(true_slots, R.REGS)
    return got, pre


def _group_model(items, gcards, pre, slots=None):
    """Registers of slots 0..slots-1 of a table of gcards[0] x gcards[1] slots (the rest keeps `pre`)."""
    exp = pre.copy()
    true_slots = gcards[0] * gcards[1]
    for it in items:
        slot = np.zeros(len(it["selected"]), np.int64)
        for (ids, remap, _), m in zip(it["g"], (1, gcards[0])):
            gid = np.asarray(ids, np.int64) if remap is None else np.asarray(remap, np.int64)[ids]
            slot = np.where((gid < 0) | (slot < 0), -1, slot + gid * m)
        slot = np.where(slot >= (true_slots if slots is None else slots), -1, slot)
        exp = M.offer_group(it["selected"], it["counts"], it["ids"], it["codes"], slot, true_slots, exp)
    return exp


@pytest.mark.parametrize("gcards", [(1, 1), (2, 1), (257, 1), (256, 256)])
def test_group_slots(hk, gcards):
    """slots 1, 2, 257 and 65536 (the limit); two items (segments with their own remap tables and code tables) share
    the table: a dense one with long docs and a sparse one.  Only the registers of (slot, register) pairs the model
    touches are non-zero."""
    rng = np.random.default_rng(gcards[0] * 1000 + gcards[1])
    items = [_group_item(rng, 8192 + 37, 0.5, 17, 70000, gcards, max(1, gcards[0] - gcards[0] // 3), "boundary"),
             _group_item(rng, 8193, 0.03, 10, 300, gcards, gcards[0], "rand")]
    got, pre = _run_group(hk, items, gcards)
    np.testing.assert_array_equal(got, _group_model(items, gcards, pre))
    assert (got[:, 255] == 0).all() and got.any()  # padding rows, bits past num_docs, the spare word


@pytest.mark.parametrize("density", [0.03, 1])
def test_group_keys_outside_the_space_offer_nothing(hk, density):
    """A remap entry of -1, and slots at or past `slots` (the table is larger than the key space the launch names)."""
    rng = np.random.default_rng(23)
    gcards = (7, 5)
    items = [_group_item(rng, 5000, density, 12, 4000, gcards, 6, "last", holes=True)]
    pre = np.zeros((35, R.REGS), np.uint32)
    got, _ = _run_group(hk, items, gcards, prefill=pre, slots=20)
    exp = _group_model(items, gcards, pre, slots=20)
    np.testing.assert_array_equal(got, exp)
    assert not got[20:].any() and got[:20].any() and (got[:, 255] == 0).all()
    full = _group_model([dict(items[0], g=[(items[0]["g"][0][0], np.abs(items[0]["g"][0][1]), 3), items[0]["g"][1]])],
                        gcards, pre)
    assert (full != exp).any()  # the holes and the cut-off do remove offers


def test_group_table_is_maxed_into_and_grid_free(hk):
    rng = np.random.default_rng(21)
    gcards = (7, 5)
    items = [_group_item(rng, 9000, 1, 12, 4000, gcards, 5, "first")]
    pre = rng.integers(0, R.MAX_RANK + 1, (35, R.REGS)).astype(np.uint32)
    pre[:, 255] = 0
    outs = []
    for w in (1, 3, 64):
        got, _ = _run_group(hk, items, gcards, prefill=pre, wgs=w)
        np.testing.assert_array_equal(got, _group_model(items, gcards, pre))
        outs.append(got.tobytes())
    assert outs[0] == outs[1] == outs[2]


# ---- launchers -------------------------------------------------------------------------------------------------------
def test_launchers_refuse_bad_arguments(hk):
    """Null pointers, a negative count or more than 65535 items, bits outside 1..32, slots < 1 or above the limit, a
    gmul outside 1..slots, a zero grid: a status, no launch, every buffer left at its sentinel."""
    rng = np.random.default_rng(14)
    it = _item(rng, 100, 1, 7, 100)
    pre = np.full(R.REGS, S32.view(np.uint32), np.uint32)

    def setter(*path_value):
        *path, value = path_value

        def f(arr):
            o = arr[0]
            for p in path[:-1]:
                o = getattr(o, p)
            setattr(o, path[-1], value)
        return f

    for kw in ({"wgs": 0}, {"nitems": -1}, {"nitems": 65536}, {"null": "items"}, {"null": "check"},
               {"mutate": setter("h", "num_docs", -1)}, {"mutate": setter("h", "bits", 0)},
               {"mutate": setter("h", "bits", 33)}, {"mutate": setter("start", None)}, {"mutate": setter("total", -1)},
               {"mutate": setter("h", "codes", None)}, {"mutate": setter("h", "out", None)}):
        got = _run(hk, [it], [pre], kw.pop("wgs", 3), expect_status=R.INVALID_VALUE, **kw)[0]
        assert (got == pre).all()

    gcards = (3, 2)
    git = _group_item(rng, 100, 1, 7, 100, gcards, 3)
    gpre = np.full((6, R.REGS), S32.view(np.uint32), np.uint32)

    def gbits(value):
        def f(arr):
            arr[0].g.g[1].bits = value
        return f

    def gfwd_null(arr):
        arr[0].g.g[0].fwd = None

    for kw in ({"wgs": 0}, {"slots": 0}, {"slots": -5}, {"slots": R.MAX_GROUP_SLOTS + 1}, {"ngcols": 0},
               {"ngcols": R.MAX_GROUP_COLS + 1}, {"gmul": (0, 3)}, {"gmul": (1, 7)}, {"null": "items"},
               {"null": "check"}, {"null": "gmul"}, {"mutate": setter("g", "h", "num_docs", -1)},
               {"mutate": setter("g", "h", "bits", 33)}, {"mutate": setter("g", "h", "bits", 0)},
               {"mutate": gbits(0)}, {"mutate": gbits(33)}, {"mutate": gfwd_null}, {"mutate": setter("start", None)},
               {"mutate": setter("total", -1)}):
        got, _ = _run_group(hk, [git], gcards, prefill=gpre, expect_status=R.INVALID_VALUE, **kw)
        assert (got == gpre).all()
    # no items: nothing to launch, success
    assert hk.offer(hk.up(np.zeros(64, np.uint8)).data_ptr(), C.addressof((M.HllMvItem * 1)()), 0, 1, hk.stream) == 0
