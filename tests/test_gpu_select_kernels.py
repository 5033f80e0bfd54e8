"""The selection ORDER BY kernels (pinot_amd/csrc/pgx_select.hip: pgx_select_topk, pgx_select_merge,
pgx_select_gather) launched directly on torch device buffers and compared with the numpy model of tests/select_ref.py.
Every output is pre-filled with a sentinel and has guard words past its end; both must come back untouched."""
import ctypes as C

import numpy as np
import pytest

from tests import select_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
S32 = np.int32(-1515870811)            # 0xA5A5A5A5
S64 = np.int64(0x5A5A5A5A5A5A5A5A)


class _SK:
    def __init__(self):
        import torch
        from pinot_amd import native as N
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.topk, self.merge, self.gather = R.bind(N.lib())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.dev)

    def filled(self, n, value, dtype):
        return self.torch.full((n + GUARD,), int(value), dtype=dtype, device=self.dev)

    def sync(self):
        self.torch.cuda.synchronize(self.dev)


@pytest.fixture(scope="module")
def sk():
    return _SK()


def _col(ids, card, asc=True, bits=None, kbits=None):
    """One order column of an item: dictIds, cardinality, direction, stored bits, key bits."""
    kb = R.key_bits(card) if kbits is None else kbits
    return {"ids": np.asarray(ids), "card": int(card), "asc": asc, "bits": kb if bits is None else bits, "kbits": kb}


def _model(item, k):
    cols = [(c["ids"], c["card"], c["asc"], c["kbits"]) for c in item["cols"]]
    return R.top_k(item["selected"], cols, k)


def _run(sk, items, k, wgs, expect_status=0):
    """Launch top-K and merge over `items` ([{"selected": bool per doc, "cols": [_col, ...]}]); check sentinels and
    guards; return (per-item docIds, raw outputs)."""
    t = sk.torch
    keep = []
    arr = (R.SelItem * max(1, len(items)))()
    for i, it in enumerate(items):
        n = len(it["selected"])
        mask = sk.up(R.pack_mask(it["selected"]))
        keep.append(mask)
        arr[i].sel = mask.data_ptr()
        arr[i].num_docs = n
        arr[i].ncols = len(it["cols"])
        for j, c in enumerate(it["cols"]):
            assert len(c["ids"]) == n
            fwd = sk.up(R.pack_fwd(c["ids"], c["bits"], n))
            keep.append(fwd)
            arr[i].c[j].fwd = fwd.data_ptr()
            arr[i].c[j].bits = c["bits"]
            arr[i].c[j].kbits = c["kbits"]
            arr[i].c[j].card = c["card"]
            arr[i].c[j].desc = 0 if c["asc"] else 1
    ni = len(items)
    dev_items = sk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    ckey = sk.filled(ni * wgs * k, S64, t.int64)
    cdoc = sk.filled(ni * wgs * k, S32, t.int32)
    ccnt = sk.filled(ni * wgs, S32, t.int32)
    odoc = sk.filled(ni * k, S32, t.int32)
    ocnt = sk.filled(ni, S32, t.int32)
    st = sk.topk(dev_items.data_ptr(), ni, k, wgs, ckey.data_ptr(), cdoc.data_ptr(), ccnt.data_ptr(), sk.stream)
    assert st == expect_status
    if st == 0:
        st = sk.merge(ni, k, wgs, ckey.data_ptr(), cdoc.data_ptr(), ccnt.data_ptr(), odoc.data_ptr(), ocnt.data_ptr(),
                      sk.stream)
        assert st == 0
    sk.sync()
    ckey, cdoc, ccnt, odoc, ocnt = (x.cpu().numpy() for x in (ckey, cdoc, ccnt, odoc, ocnt))
    if expect_status != 0:
        for a, s in ((ckey, S64), (cdoc, S32), (ccnt, S32), (odoc, S32), (ocnt, S32)):
            assert (a == s).all()
        return None, None
    # guards
    assert (ckey[ni * wgs * k:] == S64).all() and (cdoc[ni * wgs * k:] == S32).all()
    assert (ccnt[ni * wgs:] == S32).all() and (odoc[ni * k:] == S32).all() and (ocnt[ni:] == S32).all()
    # candidate lists: counts in range, entries past the count untouched
    cc = ccnt[:ni * wgs]
    assert ((cc >= 0) & (cc <= k)).all()
    ck, cd = ckey[:ni * wgs * k].reshape(ni * wgs, k), cdoc[:ni * wgs * k].reshape(ni * wgs, k)
    past = np.arange(k)[None, :] >= cc[:, None]
    assert (ck[past] == S64).all() and (cd[past] == S32).all()
    oc = ocnt[:ni]
    assert ((oc >= 0) & (oc <= k)).all()
    od = odoc[:ni * k].reshape(ni, k)
    assert (od[np.arange(k)[None, :] >= oc[:, None]] == S32).all()
    return [od[i, :oc[i]].astype(np.int64) for i in range(ni)], (ck, cd, cc)


def _check(sk, items, k, wgs=3):
    got, raw = _run(sk, items, k, wgs)
    for g, it in zip(got, items):
        np.testing.assert_array_equal(g, _model(it, k))
    return got, raw


def _random_item(rng, n, density, cards=(1000, 7), ascs=(True, False)):
    if density == 0:
        sel = np.zeros(n, bool)
    elif density == 1:
        sel = np.ones(n, bool)
    else:
        sel = rng.random(n) < density
    return {"selected": sel, "cols": [_col(rng.integers(0, c, n), c, a) for c, a in zip(cards, ascs)]}


@pytest.mark.parametrize("num_docs", [1, 63, 64, 65, 8191, 8192, 8193, 3 * 8192 + 37])
def test_sizes_k_and_densities(sk, num_docs):
    """The spare mask word and the bits past num_docs are all ones and the padding rows hold dictId 0 (the best key):
    neither may be selected (R.pack_mask / R.pack_fwd build them so)."""
    rng = np.random.default_rng(num_docs)
    for k in (1, 10):
        for density in (0, 1 / 64, 1 / 2, 1):
            it = _random_item(rng, num_docs, density)
            got, _ = _check(sk, [it], k)
            assert (got[0] < num_docs).all()


def test_fewer_exactly_and_zero_matches(sk):
    rng = np.random.default_rng(7)
    n, k = 5000, 10
    for matches in (0, 3, 10):
        it = _random_item(rng, n, 0)
        it["selected"][rng.choice(n, matches, replace=False)] = True
        got, _ = _check(sk, [it], k)
        assert len(got[0]) == matches


def test_all_keys_equal_gives_lowest_docids(sk):
    rng = np.random.default_rng(8)
    n = 20000
    sel = rng.random(n) < 0.5
    it = {"selected": sel, "cols": [_col(np.full(n, 5), 9)]}
    got, _ = _check(sk, [it], 10)
    np.testing.assert_array_equal(got[0], np.flatnonzero(sel)[:10])


@pytest.mark.parametrize("improving", [True, False])
def test_monotonic_keys_refill_the_buffer(sk, improving):
    """Keys strictly improving in doc order: every row beats the threshold, so the buffer refills every time; strictly
    worsening: the first K rows stay."""
    n, k = 40000, 1000
    ids = np.arange(n)[::-1] if improving else np.arange(n)
    it = {"selected": np.ones(n, bool), "cols": [_col(ids.copy(), n)]}
    got, _ = _check(sk, [it], k, wgs=1)
    exp = np.arange(n - 1, n - 1 - k, -1) if improving else np.arange(k)
    np.testing.assert_array_equal(got[0], exp)


def test_key_widths(sk):
    rng = np.random.default_rng(9)
    n = 9000
    sel = rng.random(n) < 0.7
    # 1 + 17 + 32 bits, ASC / DESC / ASC; few distinct values in the leading columns so the later ones decide
    a = {"selected": sel, "cols": [_col(rng.integers(0, 2, n), 2, True),
                                   _col(rng.integers(0, 3, n) + 100000, 1 << 17, False),
                                   _col(rng.integers(0, (1 << 32) - 1, n, dtype=np.uint64), (1 << 32) - 1, True, kbits=32)]}
    # exactly 64 bits (32 + 32), the second descending
    b = {"selected": sel, "cols": [_col(rng.integers(0, 4, n) + (1 << 31), (1 << 32) - 1, True, kbits=32),
                                   _col(rng.integers(0, (1 << 32) - 1, n, dtype=np.uint64), (1 << 32) - 1, False, kbits=32)]}
    # DESC with a cardinality that is no power of two, stored wider than the key needs
    c = {"selected": sel, "cols": [_col(rng.integers(0, 1000, n), 1000, False, bits=13)]}
    for it in (a, b, c):
        _check(sk, [it], 10)
    assert R.order_keys([(x["ids"], x["card"], x["asc"], x["kbits"]) for x in b["cols"]])[1] == 64


def test_k_max_rows(sk):
    rng = np.random.default_rng(10)
    it = _random_item(rng, 10000, 1 / 2, cards=(50, 300))
    got, _ = _check(sk, [it], R.MAX_ROWS, wgs=2)
    assert len(got[0]) == R.MAX_ROWS


def test_workgroups_per_item_do_not_change_the_result(sk):
    rng = np.random.default_rng(11)
    it = _random_item(rng, 3 * 8192 + 37, 1 / 2, cards=(20, 5))
    outs = [_check(sk, [it], 100, wgs=w)[0][0] for w in (1, 3, 64)]
    assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()


def test_five_items_in_one_launch(sk):
    rng = np.random.default_rng(12)
    items = [_random_item(rng, 20000, 1 / 2, cards=(1 << 12, 3)),
             _random_item(rng, 300, 1, cards=(2,), ascs=(False,)),
             _random_item(rng, 8192, 0),                                  # an empty item between two full ones
             _random_item(rng, 8193, 1 / 64, cards=(1 << 20, 1 << 10), ascs=(False, False)),
             _random_item(rng, 1, 1, cards=(1,), ascs=(True,))]
    got, _ = _check(sk, items, 25, wgs=4)
    assert len(got[2]) == 0 and len(got[4]) == 1


def test_candidate_lists_are_each_workgroups_best(sk):
    """pgx_select_topk alone: workgroup g of G owns the mask words w with (w // 256) % G == g and writes its best K."""
    rng = np.random.default_rng(13)
    n, k, wgs = 3 * 8192 + 37, 10, 3
    it = _random_item(rng, n, 1 / 2, cards=(100, 3))
    _, (ck, cd, cc) = _check(sk, [it], k, wgs)
    owner = (np.arange(n) // 32 // 256) % wgs
    for g in range(wgs):
        mine = dict(it, selected=it["selected"] & (owner == g))
        exp = _model(mine, k)
        assert cc[g] == len(exp)
        np.testing.assert_array_equal(cd[g, :cc[g]], exp)


def test_launchers_refuse_bad_arguments(sk):
    rng = np.random.default_rng(14)
    it = _random_item(rng, 100, 1)
    _run(sk, [it], R.MAX_ROWS + 1, 1, expect_status=R.INVALID_VALUE)
    _run(sk, [it], 5, 0, expect_status=R.INVALID_VALUE)


def test_gather(sk):
    """One thread per (schema column, item, rank): widths 1, 7, 17 and 32, a sorted column's packed view, and ranks
    past the count left as they were."""
    t = sk.torch
    rng = np.random.default_rng(15)
    k, sizes, counts = 10, (9000, 70), (10, 4)
    widths = (1, 7, 17, 32, 5)
    keep, ids = [], []
    cols = (R.SelGatherCol * (len(sizes) * len(widths)))()
    for i, n in enumerate(sizes):
        ids.append([])
        for j, w in enumerate(widths):
            v = rng.integers(0, 1 << w, n, dtype=np.uint64)
            if j == 4:
                v = np.sort(v)  # a sorted column: staging materialises the same packed view
            ids[i].append(v)
            fwd = sk.up(R.pack_fwd(v, w, n))
            keep.append(fwd)
            cols[i * len(widths) + j].fwd = fwd.data_ptr()
            cols[i * len(widths) + j].bits = w
    docs = np.full(len(sizes) * k + GUARD, S32, np.int32)
    for i, n in enumerate(sizes):
        docs[i * k:i * k + counts[i]] = rng.choice(n, counts[i], replace=False)
        if i == 0:
            docs[0] = n - 1  # the last row of the index
    odoc = sk.up(docs).view(t.int32)
    ocnt = sk.up(np.array(counts, np.int32)).view(t.int32)
    total = len(widths) * len(sizes) * k
    oids = sk.filled(total, S32, t.int32)
    dcols = sk.up(np.frombuffer(bytes(cols), dtype=np.uint8))
    st = sk.gather(dcols.data_ptr(), len(sizes), len(widths), k, odoc.data_ptr(), ocnt.data_ptr(), oids.data_ptr(),
                   sk.stream)
    assert st == 0
    sk.sync()
    out = oids.cpu().numpy()
    assert (out[total:] == S32).all()
    out = out[:total].reshape(len(widths), len(sizes), k)
    for i in range(len(sizes)):
        for j in range(len(widths)):
            exp = ids[i][j][docs[i * k:i * k + counts[i]]].astype(np.uint32).view(np.int32)
            np.testing.assert_array_equal(out[j, i, :counts[i]], exp)
            assert (out[j, i, counts[i]:] == S32).all()


def _width_selections(n=100):
    """Over n = 100 docs (three full mask words and a partial one): a sparse selection (three rows of every word, the
    index's last row among them: rows are read one by one) and a dense one (every row: whole words are decoded)."""
    sparse = np.zeros(n, bool)
    sparse[[1, 17, 31, 32, 40, 63, 64, 77, 95, 96, 98, n - 1]] = True
    return sparse, np.ones(n, bool)


def test_every_stored_width(sk):
    """Widths 1 .. 32 of the first order column, whose ids use the whole width: K = num_docs, so the answer is every
    selected row in key order and any wrongly decoded row moves."""
    rng = np.random.default_rng(16)
    n = 100
    items = []
    for bits in range(1, 33):
        card = (1 << bits) if bits < 32 else (1 << 32) - 1
        for sel in _width_selections(n):
            items.append({"selected": sel, "cols": [_col(rng.integers(0, card, n, dtype=np.uint64), card, kbits=bits)]})
    got, _ = _check(sk, items, n, wgs=1)
    assert [len(g) for g in got] == [12, n] * 32
