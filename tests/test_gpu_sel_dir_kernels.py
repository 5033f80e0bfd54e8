"""The sparse GROUP BY kernels (PGX_X_SPARSE_GROUP_SETS) launched directly on torch device buffers: the group directory
(pgx_sel_dir_build, pgx_sel_dir_find: pinot_amd/csrc/pgx_hll.hip) and the sparse forms of the six group kernels
(pgx_hll_offer[_mv]_group, pgx_distinct_mark[_mv]_group, pgx_percentile_count[_mv]_group instantiated over
SelSparseKey), compared with the numpy models: tests/sel_dir_ref.py gives every row its group, the dense models of
hll_ref / hll_mv_ref / distinct_ref / percentile_ref the tables at slots = groups.  Every output has guard words past
its end, which must come back untouched; registers, bitmaps and counters are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import distinct_ref as D
from tests import hll_mv_ref as M
from tests import hll_ref as R
from tests import percentile_ref as P
from tests import sel_dir_ref as S

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = 0xA5A5A5A5A5A5A5A5
C31 = 1 << 31


class _K:
    def __init__(self):
        import torch
        from pinot_amd import native as N
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.fn = S.bind(N.lib())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.dev)

    def out(self, prefill):
        """A device buffer holding `prefill` followed by GUARD sentinel words of its type."""
        a = np.asarray(prefill).reshape(-1)
        return self.up(np.concatenate([a, np.full(GUARD, SENT & ((1 << (8 * a.itemsize)) - 1), a.dtype)]))

    def back(self, buf, n, dtype):
        """The buffer's first n words, after checking the guard words behind them."""
        self.torch.cuda.synchronize(self.dev)
        a = buf.cpu().numpy().view(dtype)
        assert len(a) == n + GUARD and (a[n:] == (SENT & ((1 << (8 * a.itemsize)) - 1))).all()
        return a[:n].copy()


@pytest.fixture(scope="module")
def hk():
    return _K()


def _pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


class _Dir:
    """A directory on the device: keys (uint64[n, 2], the first W words of each are the key), built with capacity
    cap; .key is the host struct the sparse launchers take."""

    def __init__(self, hk, keys, W, cap, lay=None, expect=0):
        keys = np.asarray(keys, np.uint64).reshape(-1, 2)
        n = len(keys)
        flat = np.ascontiguousarray(keys[:, :W]).reshape(-1)
        self.host = flat if n else np.zeros(1, np.uint64)
        self.keys = hk.up(self.host)
        self.tkey = hk.out(np.full(max(cap, 1) * W, 0x1234567, np.uint64))
        self.tstate = hk.out(np.full(max(cap, 1), 7, np.uint32))
        self.tidx = hk.out(np.full(max(cap, 1), 0xFFFFFFFF, np.uint32))
        self.miss = hk.up(np.zeros(1, np.uint64))
        self.status = hk.fn["build"](self.keys.data_ptr(), self.host.ctypes.data, n, W, self.tkey.data_ptr(),
                                     self.tstate.data_ptr(), self.tidx.data_ptr(), cap, hk.stream)
        assert self.status == expect
        self.key = S.SelSparseKey()
        self.key.keys, self.key.state = self.tkey.data_ptr(), self.tstate.data_ptr()
        self.key.index, self.key.miss, self.key.cap = self.tidx.data_ptr(), self.miss.data_ptr(), cap
        S.fill_key(self.key, lay or S.layout([C31, C31] if W == 1 else [C31] * 4), max(n, 1), W)
        self.hk, self.n, self.W, self.cap = hk, n, W, cap

    def misses(self):
        self.hk.torch.cuda.synchronize(self.hk.dev)
        return int(self.miss.cpu().numpy().view(np.uint64)[0])

    def find(self, queries, expect=0):
        q = np.ascontiguousarray(np.asarray(queries, np.uint64).reshape(-1, 2)[:, :self.W]).reshape(-1)
        n = len(q) // self.W
        qd, out = self.hk.up(q if n else np.zeros(1, np.uint64)), self.hk.out(np.full(n, 0xDEAD, np.uint32))
        st = self.hk.fn["find"](qd.data_ptr(), n, C.addressof(self.key), out.data_ptr(), self.hk.stream)
        assert st == expect
        return self.hk.back(out, n, np.uint32)


def _keys(rng, n, W):
    """n distinct keys: key 0, for W = 2 keys that differ only in the high word, the rest random (never ~0)."""
    seen, keys = set(), []

    def add(lo, hi):
        if (lo, hi) not in seen and len(keys) < n:
            seen.add((lo, hi))
            keys.append((lo, hi))
    add(0, 0)
    if W == 2:
        for hi in (1, 2, 1 << 63):
            add(5, hi)
        add(5, 0)
    add((1 << 63) | 12345, 0)
    while len(keys) < n:
        add(int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 62)) if W == 2 else 0)
    k = np.array(keys, np.uint64).reshape(-1, 2)
    assert not (k[:, 0] == np.uint64(0xFFFFFFFFFFFFFFFF)).any()
    return k, seen


@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 33, 1000])
def test_directory_build_and_lookup(hk, W, n):
    """Twice the power of two at or above n, and the smallest legal capacity (n = 1000 in 1024 slots: long probe
    chains, the table nearly full); every key finds its index, absent keys miss and are counted."""
    rng = np.random.default_rng(100 * W + n)
    keys, seen = _keys(rng, n, W)
    absent = []
    while len(absent) < 40:
        k = (int(rng.integers(1, 1 << 62)), int(rng.integers(0, 1 << 62)) if W == 2 else 0)
        if k not in seen:
            absent.append(k)
    if W == 2 and n >= 5:
        absent.append((5, 3))  # the low word of keys that are there
    for cap in (2 * _pow2(n), _pow2(n)):
        d = _Dir(hk, keys, W, cap)
        got = d.find(keys)
        np.testing.assert_array_equal(got, np.arange(n, dtype=np.uint32))
        assert d.misses() == 0
        got = d.find(np.array(absent, np.uint64))
        assert (got == S.NO_SLOT).all() and d.misses() == len(absent)
        tidx = hk.back(d.tidx, cap, np.uint32)
        assert sorted(tidx[tidx != 0xFFFFFFFF].tolist()) == list(range(n))  # every key once, nothing else written


def test_directory_launcher_refusals_launch_nothing(hk):
    rng = np.random.default_rng(9)
    keys, _ = _keys(rng, 33, 2)
    d = _Dir(hk, keys, 2, 64)  # a good table to refuse over
    before = (hk.back(d.tkey, 128, np.uint64), hk.back(d.tstate, 64, np.uint32), hk.back(d.tidx, 64, np.uint32))
    # a capacity that is no power of two, one below the count, none; a W other than 1 or 2; a bad count
    for W, n, cap in ((2, 33, 48), (2, 33, 32), (2, 33, 0), (3, 33, 64), (0, 33, 64), (2, -1, 64),
                      (2, S.MAX_SPARSE_GROUPS + 1, 1 << 18)):
        st = hk.fn["build"](d.keys.data_ptr(), d.host.ctypes.data, n, W, d.tkey.data_ptr(), d.tstate.data_ptr(),
                            d.tidx.data_ptr(), cap, hk.stream)
        assert st == R.INVALID_VALUE
    args = [d.keys.data_ptr(), d.host.ctypes.data, 33, 2, d.tkey.data_ptr(), d.tstate.data_ptr(), d.tidx.data_ptr()]
    for null in (0, 1, 4, 5, 6):
        a = list(args)
        a[null] = None
        assert hk.fn["build"](*a, 64, hk.stream) == R.INVALID_VALUE
    ones = np.array([3, 0xFFFFFFFFFFFFFFFF, 9], np.uint64)  # a one-word key of ~0 is the empty slot
    assert hk.fn["build"](d.keys.data_ptr(), ones.ctypes.data, 3, 1, d.tkey.data_ptr(), None, d.tidx.data_ptr(), 64,
                          hk.stream) == R.INVALID_VALUE
    after = (hk.back(d.tkey, 128, np.uint64), hk.back(d.tstate, 64, np.uint32), hk.back(d.tidx, 64, np.uint32))
    for b, a in zip(before, after):
        np.testing.assert_array_equal(a, b)
    # the lookup's own checks
    q = hk.up(np.zeros(4, np.uint64))
    o = hk.out(np.zeros(2, np.uint32))
    assert hk.fn["find"](None, 2, C.addressof(d.key), o.data_ptr(), hk.stream) == R.INVALID_VALUE
    assert hk.fn["find"](q.data_ptr(), 2, None, o.data_ptr(), hk.stream) == R.INVALID_VALUE
    assert hk.fn["find"](q.data_ptr(), -1, C.addressof(d.key), o.data_ptr(), hk.stream) == R.INVALID_VALUE
    np.testing.assert_array_equal(hk.back(o, 2, np.uint32), 0)


# ---- the sparse group kernels ----------------------------------------------------------------------------------------
_FAMILIES = ("hll", "hll_mv", "distinct", "distinct_mv", "percentile", "percentile_mv")
_LAUNCH = {"hll": "hll_offer_group_sparse", "hll_mv": "hll_offer_mv_group_sparse",
           "distinct": "distinct_mark_group_sparse", "distinct_mv": "distinct_mark_mv_group_sparse",
           "percentile": "percentile_count_group_sparse", "percentile_mv": "percentile_count_mv_group_sparse"}
_ITEM = {"hll": R.HllGroupItem, "hll_mv": M.HllMvGroupItem, "distinct": D.DistinctGroupItem,
         "distinct_mv": D.DistinctMvGroupItem, "percentile": P.PercentileGroupItem,
         "percentile_mv": P.PercentileMvGroupItem}
_VALUE = {1: 2, 7: 100, 32: 1000}  # value column: bits -> cardinality


def _selection(kind, n):
    """empty; one bit; mixed: word 0 dense (12 rows), word 1 sparse (3 rows), the partial last word 2 rows."""
    sel = np.zeros(n, bool)
    if kind == "one":
        sel[min(n - 1, 37)] = True
    elif kind == "mixed":
        sel[[0, 1, 2, 5, 8, 9, 13, 17, 20, 25, 30, 31]] = True
        sel[[33, 47, 62]] = True
        sel[[n - 5, n - 1]] = True
    elif kind == "all":
        sel[:] = True
    return sel


def _segment(rng, W, n, kind, seg):
    """One segment's group columns [(local ids, remap)].  W = 1: two columns of 300 global ids (18 bits), column 0
    remapped (segment 1: with a -1 entry), column 1 the identity in segment 0.  W = 2: three columns, 31 + 31 + 9
    bits, the first two remapped into ids of up to 31 bits."""
    lim = 300 if W == 1 else C31
    r0 = rng.choice(lim, 12, replace=False).astype(np.int64) if W == 1 else rng.integers(0, lim, 12)
    r0 = (np.unique(r0).tolist() + list(range(12)))[:12]
    r0 = np.array(r0, np.int32)
    rng.shuffle(r0)
    if seg == 1:
        r0[3] = -1
    g0 = (rng.integers(0, 12, n), r0)
    if W == 1:
        g1 = (rng.integers(0, 6, n), None if seg == 0 else np.array([7, 6, 5, 4, 3, 2], np.int32))
        return [g0, g1], _selection(kind, n)
    r1 = np.array(sorted(rng.integers(0, lim, 5).tolist()), np.int32)
    return [g0, (rng.integers(0, 5, n), r1), (rng.integers(0, 4, n), None)], _selection(kind, n)


def _values(rng, family, n, bits):
    card = _VALUE[bits]
    if family.endswith("_mv"):
        counts = rng.choice([0, 1, 1, 2, 5, 40], n)  # docs with no, one and several values
        counts[0] = max(counts[0], 1)
        return counts, rng.integers(0, card, int(counts.sum())), card
    return None, rng.integers(0, card, n), card


def _hll_table(rng, card):
    return ((rng.integers(0, 256, card).astype(np.uint32) << 8) |
            rng.integers(1, R.MAX_RANK + 1, card).astype(np.uint32)).astype(np.uint16)


def _run_family(hk, family, W, segs, bits, directory, lay, wgs=2, mutate=None, expect=0):
    """segs: [(gcols, selected, counts, ids, card, codes)]; all write one table.  Returns (table, misses)."""
    groups = directory.n
    card = segs[0][4]
    if family.startswith("hll"):
        shape, dtype = (groups, R.REGS), np.uint32
    elif family.startswith("distinct"):
        shape, dtype = (groups, D.words(card)), np.uint32
    else:
        shape, dtype = (groups, card), np.uint64
    out = hk.out(np.zeros(shape, dtype))
    arr = (_ITEM[family] * len(segs))()
    keep = []
    for i, (gcols, selected, counts, ids, card, codes) in enumerate(segs):
        n = len(selected)
        it = arr[i]
        g = it.g if family.endswith("_mv") else it
        inner = g.h if family.startswith("hll") else g.d
        rows = len(ids)
        mask, fwd = hk.up(R.pack_mask(selected)), hk.up(R.pack_fwd(ids, bits, max(rows, 1)))
        keep += [mask, fwd]
        inner.sel, inner.fwd, inner.out, inner.bits, inner.num_docs = mask.data_ptr(), fwd.data_ptr(), out.data_ptr(), bits, n
        if family.startswith("hll"):
            ct = hk.up(codes)
            keep.append(ct)
            inner.codes, inner.ncodes = ct.data_ptr(), card
        else:
            inner.card = card
        if family.endswith("_mv"):
            st = hk.up(M.starts(counts))
            keep.append(st)
            it.start, it.total = st.data_ptr(), rows
        for c, (gid, remap) in enumerate(gcols):
            gb = max(1, int(np.max(gid)).bit_length()) + (c % 2)  # (a width of its own per column)
            gf = hk.up(R.pack_fwd(gid, gb, n))
            keep.append(gf)
            g.g[c].fwd, g.g[c].bits = gf.data_ptr(), gb
            if remap is not None:
                rm = hk.up(np.asarray(remap, np.int32))
                keep.append(rm)
                g.g[c].remap = rm.data_ptr()
    key = S.SelSparseKey.from_buffer_copy(directory.key)
    if mutate:
        mutate(arr, key)
    dev_items = hk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    st = hk.fn[_LAUNCH[family]](dev_items.data_ptr(), C.addressof(arr), len(segs), C.addressof(key), wgs, hk.stream)
    assert st == expect
    return hk.back(out, int(np.prod(shape)), dtype).reshape(shape), directory.misses()


def _model(family, segs, lay, group_keys):
    groups = len(group_keys)
    table, misses = None, 0
    for gcols, selected, counts, ids, card, codes in segs:
        slot = S.row_groups(lay, group_keys, S.global_ids(gcols))
        misses += int((selected & (slot < 0)).sum())
        ok = selected & (slot >= 0)
        s0 = np.where(ok, slot, 0)
        if family == "hll":
            table = R.offer_group(ok, ids, codes, s0, groups, table)
        elif family == "hll_mv":
            table = M.offer_group(ok, counts, ids, codes, s0, groups, table)
        elif family == "distinct":
            table = D.mark_group(ok, ids, card, s0, groups, table)
        elif family == "distinct_mv":
            table = D.mark_mv_group(ok, counts, ids, card, s0, groups, table)
        elif family == "percentile":
            table = P.count_group(ok, ids, card, s0, groups, table)
        else:
            table = P.count_mv_group(ok, counts, ids, card, s0, groups, table)
    return table, misses


def _case(hk, rng, family, W, bits, shapes, drop=0):
    """shapes: [(docs, selection kind)], one segment each.  The directory holds the keys of every row whose ids are
    keys at all, selected or not (groups nothing touches keep zero rows), minus `drop` of the selected rows' keys."""
    lay = S.layout([300, 300] if W == 1 else [C31, C31, 300])
    segs, allk, selk = [], [], []
    for seg, (n, kind) in enumerate(shapes):
        gcols, selected = _segment(rng, W, n, kind, seg)
        counts, ids, card = _values(rng, family, n, bits)
        codes = _hll_table(rng, card) if family.startswith("hll") else None
        segs.append((gcols, selected, counts, ids, card, codes))
        keys, ok = S.pack(lay, S.global_ids(gcols))
        allk += [tuple(k) for k in keys[ok].tolist()]
        selk += [tuple(k) for k in keys[ok & selected].tolist()]
    dropped = set(sorted(set(selk))[:drop])
    group_keys = np.array([k for k in sorted(set(allk)) if k not in dropped] or [(1 << 40, 0)], np.uint64)
    rng.shuffle(group_keys)  # the result's order is any order
    d = _Dir(hk, group_keys, lay["W"], S.capacity(len(group_keys)), lay)
    got, missed = _run_family(hk, family, W, segs, bits, d, lay)
    want, want_missed = _model(family, segs, lay, group_keys)
    np.testing.assert_array_equal(got, want)
    assert missed == want_missed
    return got, missed, segs


@pytest.mark.parametrize("family", _FAMILIES)
@pytest.mark.parametrize("W", [1, 2])
def test_one_segment_of_70_docs(hk, family, W):
    """70 docs: a partial last mask word.  Selections: none, one bit, a dense and a sparse word; value widths 1, 7
    and 32 bits."""
    rng = np.random.default_rng(_FAMILIES.index(family) * 10 + W)
    for bits in (1, 7, 32):
        for kind in ("empty", "one", "mixed", "all"):
            got, missed, _ = _case(hk, rng, family, W, bits, [(70, kind)])
            assert missed == 0
            if kind == "empty":
                assert not got.any()
            elif kind == "all":
                assert got.any()


@pytest.mark.parametrize("family", _FAMILIES)
@pytest.mark.parametrize("W", [1, 2])
def test_two_segments_with_their_own_remaps(hk, family, W):
    """Two items in one launch into one table; the second segment's remap holds a -1: its rows are in no group and
    are counted as misses."""
    rng = np.random.default_rng(_FAMILIES.index(family) * 10 + W + 100)
    for bits in (1, 7, 32):
        got, missed, segs = _case(hk, rng, family, W, bits, [(70, "mixed"), (200, "all")])
        gcols, selected = segs[1][0], segs[1][1]
        assert missed == int((selected & (gcols[0][0] == 3)).sum()) > 0


@pytest.mark.parametrize("family", _FAMILIES)
def test_keys_the_directory_does_not_hold(hk, family):
    """Four of the selected rows' groups are left out of the directory: their rows change no table word (the table
    equals the model's, which skips them) and every one is counted."""
    rng = np.random.default_rng(_FAMILIES.index(family) + 300)
    for W in (1, 2):
        got, missed, _ = _case(hk, rng, family, W, 7, [(70, "all"), (200, "mixed")], drop=4)
        assert missed >= 4


def test_sparse_launcher_refusals_launch_nothing(hk):
    rng = np.random.default_rng(77)
    lay = S.layout([300, 300])
    for family in _FAMILIES:
        gcols, selected = _segment(rng, 1, 70, "all", 0)
        counts, ids, card = _values(rng, family, 70, 7)
        codes = _hll_table(rng, card) if family.startswith("hll") else None
        segs = [(gcols, selected, counts, ids, card, codes)]
        keys, _ = S.pack(lay, S.global_ids(gcols))
        uniq = np.unique(keys, axis=0)
        d = _Dir(hk, uniq, 1, S.capacity(len(uniq)), lay)

        def inner(arr):
            g = arr[0].g if family.endswith("_mv") else arr[0]
            return g.h if family.startswith("hll") else g.d

        bad = [lambda a, k: setattr(k, "groups", 0),
               lambda a, k: setattr(k, "groups", S.MAX_SPARSE_GROUPS + 1),
               lambda a, k: setattr(k, "W", 3),
               lambda a, k: setattr(k, "W", 0),
               lambda a, k: setattr(k, "cap", 48),
               lambda a, k: setattr(k, "cap", 4),  # below the groups
               lambda a, k: setattr(k, "keys", None),
               lambda a, k: setattr(k, "index", None),
               lambda a, k: setattr(k, "miss", None),
               lambda a, k: setattr(k, "ngcols", 0),
               lambda a, k: setattr(k, "ngcols", 17),
               lambda a, k: k.bits.__setitem__(0, 0),
               lambda a, k: k.shift.__setitem__(1, 60),  # the field would end past the key's one word
               lambda a, k: setattr(inner(a), "bits", 0),
               lambda a, k: setattr(inner(a), "bits", 33),
               lambda a, k: setattr(inner(a), "sel", None),
               lambda a, k: setattr(inner(a), "out", None)]
        for m in bad:
            got, missed = _run_family(hk, family, 1, segs, 7, d, lay, mutate=m, expect=R.INVALID_VALUE)
            assert not got.any() and missed == 0
        for wgs in (0, 1025):
            got, missed = _run_family(hk, family, 1, segs, 7, d, lay, wgs=wgs, expect=R.INVALID_VALUE)
            assert not got.any() and missed == 0
