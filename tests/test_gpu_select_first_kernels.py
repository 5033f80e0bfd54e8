"""The kernels of the selection without ORDER BY (pinot_amd/csrc/pgx_select.hip: pgx_select_first_count,
pgx_select_first) launched directly on torch device buffers and compared with the numpy model of
tests/select_only_ref.py.  Every output is pre-filled with a sentinel and has guard words past its end; both must come
back untouched.  The masks come from select_ref.pack_mask(.., ones_past_end=True): the spare word and the bits past
num_docs are all ones and must be ignored."""
import ctypes as C

import numpy as np
import pytest

from tests import select_only_ref as F
from tests import select_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
S32 = np.int32(-1515870811)            # 0xA5A5A5A5
WGS = (1, 3, 64)


class _SF:
    def __init__(self):
        import torch
        from pinot_amd import native as N
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.count, self.first = F.bind(N.lib())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.dev)

    def filled(self, n):
        return self.torch.full((n + GUARD,), int(S32), dtype=self.torch.int32, device=self.dev)

    def sync(self):
        self.torch.cuda.synchronize(self.dev)


@pytest.fixture(scope="module")
def sf():
    return _SF()


def _items(sf, masks, shift=0):
    """SelItem array over `masks` (bool per doc, or an int: num_docs of an item with a null mask).  shift: words the
    mask's first word lies past a 16-byte boundary (the kernels then load word by word)."""
    keep = []
    arr = (R.SelItem * max(1, len(masks)))()
    for i, m in enumerate(masks):
        if isinstance(m, (int, np.integer)):
            arr[i].sel = None
            arr[i].num_docs = int(m)
            continue
        words = R.pack_mask(m, ones_past_end=True)
        dev = sf.up(np.concatenate([np.full(shift, 0xFFFFFFFF, "<u4"), words]))
        keep.append(dev)
        arr[i].sel = dev.data_ptr() + 4 * shift
        arr[i].num_docs = len(m)
    dev_items = sf.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    return dev_items, keep


def _selected(m):
    return np.ones(int(m), bool) if isinstance(m, (int, np.integer)) else np.asarray(m, bool)


def _run(sf, masks, k, wgs, limit=None, shift=0):
    """Launch the count (wgs > 1) and the first-K kernel; check sentinels and guards; returns (per-item docIds,
    counts, limited counts or None, stripe counts or None)."""
    ni = len(masks)
    dev_items, keep = _items(sf, masks, shift)
    scnt = sf.filled(ni * wgs)
    odoc = sf.filled(ni * k)
    ocnt = sf.filled(ni)
    olim = sf.filled(ni)
    if wgs > 1:
        assert sf.count(dev_items.data_ptr(), ni, k, wgs, scnt.data_ptr(), sf.stream) == 0
    st = sf.first(dev_items.data_ptr(), ni, k, wgs, scnt.data_ptr() if wgs > 1 else None, odoc.data_ptr(),
                  ocnt.data_ptr(), limit or 0, olim.data_ptr() if limit else None, sf.stream)
    assert st == 0
    sf.sync()
    scnt, odoc, ocnt, olim = (x.cpu().numpy() for x in (scnt, odoc, ocnt, olim))
    assert (odoc[ni * k:] == S32).all() and (ocnt[ni:] == S32).all() and (scnt[ni * wgs:] == S32).all()
    assert (olim[ni:] == S32).all()
    if wgs == 1:
        assert (scnt == S32).all()
    if not limit:
        assert (olim == S32).all()
    oc = ocnt[:ni]
    assert ((oc >= 0) & (oc <= k)).all()
    od = odoc[:ni * k].reshape(ni, k)
    assert (od[np.arange(k)[None, :] >= oc[:, None]] == S32).all()  # ranks past the count stay as they were
    return ([od[i, :oc[i]].astype(np.int64) for i in range(ni)], oc, olim[:ni] if limit else None,
            scnt[:ni * wgs].reshape(ni, wgs) if wgs > 1 else None)


def _check(sf, masks, k, wgs_list=WGS, shift=0):
    outs = []
    for wgs in wgs_list:
        got, oc, _, sc = _run(sf, masks, k, wgs, shift=shift)
        for i, m in enumerate(masks):
            sel = _selected(m)
            np.testing.assert_array_equal(got[i], F.first_docs(sel, k))
            assert oc[i] == min(k, int(sel.sum()))
            if sc is not None:
                np.testing.assert_array_equal(sc[i], F.stripe_counts(sel, k, wgs))
        outs.append(b"".join(g.tobytes() for g in got))
    assert all(o == outs[0] for o in outs)  # the same rows for every number of workgroups
    return got


def _random_mask(rng, n, density):
    if density == 0:
        return np.zeros(n, bool)
    if density == 1:
        return np.ones(n, bool)
    return rng.random(n) < density


@pytest.mark.parametrize("num_docs", [1, 31, 32, 33, 100, 8191, 8192, 8193, 3 * 8192 + 37])
def test_sizes_k_and_densities(sf, num_docs):
    rng = np.random.default_rng(num_docs)
    for k in (1, 10, 2048):
        masks = [_random_mask(rng, num_docs, d) for d in (0, 1 / 64, 1 / 2, 1)]
        got = _check(sf, masks, k)
        assert all((g < num_docs).all() for g in got)


def test_kth_match_at_the_edges(sf):
    """The K-th match in the mask's last valid bit, in the first and in the last bit of a stripe (3 workgroups over
    3 * 8192 + 37 docs: 193 chunks of 128 rows, 65 per stripe), with the other matches before, around or after it."""
    n, k = 3 * 8192 + 37, 10
    bounds = F.stripes(n, 3)
    assert bounds == [(0, 8320), (8320, 16640), (16640, n)]
    rng = np.random.default_rng(1)
    masks = []
    for kth in (n - 1, bounds[1][0], bounds[1][1] - 1, bounds[2][0], bounds[0][1] - 1):
        m = np.zeros(n, bool)
        m[rng.choice(kth, k - 1, replace=False)] = True  # K - 1 matches before it
        m[kth] = True
        masks.append(m)
        m2 = m.copy()
        m2[kth + 1:] = True                               # ... and every later doc selected too
        masks.append(m2)
    got = _check(sf, masks, k)
    assert [int(g[-1]) for g in got[::2]] == [n - 1, 8320, 16639, 16640, 8319]


def test_fewer_exactly_and_zero_matches(sf):
    rng = np.random.default_rng(7)
    n, k = 5000, 10
    masks = []
    for matches in (0, 3, 10, 11):
        m = np.zeros(n, bool)
        m[rng.choice(n, matches, replace=False)] = True
        masks.append(m)
    got = _check(sf, masks, k)
    assert [len(g) for g in got] == [0, 3, 10, 10]


def test_five_items_in_one_launch_with_an_empty_and_a_null_mask(sf):
    rng = np.random.default_rng(12)
    masks = [_random_mask(rng, 20000, 1 / 2), _random_mask(rng, 300, 1), np.zeros(0, bool),  # an item without docs
             _random_mask(rng, 8193, 1 / 64), 5000,                                           # a null mask: every doc
             _random_mask(rng, 1, 1)]
    got = _check(sf, masks, 25)
    assert len(got[2]) == 0 and got[4].tolist() == list(range(25)) and got[5].tolist() == [0]
    # null masks shorter than K, of K docs, and without docs
    got = _check(sf, [7, 25, 0, 26], 25)
    assert [len(g) for g in got] == [7, 25, 0, 25]


def test_a_mask_that_is_not_16_byte_aligned(sf):
    rng = np.random.default_rng(13)
    masks = [_random_mask(rng, 3 * 8192 + 37, 1 / 64), _random_mask(rng, 33, 1), _random_mask(rng, 100, 1 / 2)]
    for shift in (1, 2, 3):
        _check(sf, masks, 100, shift=shift)


def test_limited_counts(sf):
    """out_lim[i] = min(out_cnt[i], limit): the rows the gathers run over when the request has an offset."""
    rng = np.random.default_rng(14)
    masks = [_random_mask(rng, 9000, 1 / 2), _random_mask(rng, 9000, 0), 3, np.arange(9000) % 1000 == 0]
    for wgs in WGS:
        got, oc, ol, _ = _run(sf, masks, 25, wgs, limit=5)
        assert oc.tolist() == [25, 0, 3, 9] and ol.tolist() == [5, 0, 3, 5]


def test_stripe_counts_on_their_own(sf):
    """pgx_select_first_count alone: every stripe's popcount saturated at K, also for a null mask."""
    rng = np.random.default_rng(15)
    n, k, wgs = 3 * 8192 + 37, 100, 3
    masks = [_random_mask(rng, n, 1 / 2), _random_mask(rng, n, 1 / 1024), n, np.zeros(n, bool)]
    masks[3][[0, 8319, 8320, n - 1]] = True
    dev_items, keep = _items(sf, masks)
    scnt = sf.filled(len(masks) * wgs)
    assert sf.count(dev_items.data_ptr(), len(masks), k, wgs, scnt.data_ptr(), sf.stream) == 0
    sf.sync()
    out = scnt.cpu().numpy()
    assert (out[len(masks) * wgs:] == S32).all()
    out = out[:len(masks) * wgs].reshape(len(masks), wgs)
    for i, m in enumerate(masks):
        np.testing.assert_array_equal(out[i], F.stripe_counts(_selected(m), k, wgs))
    assert out[0].tolist() == [k, k, k] and out[2].tolist() == [k, k, k] and out[3].tolist() == [2, 1, 1]
    assert (out[1] < k).all()


def test_launchers_refuse_bad_arguments(sf):
    rng = np.random.default_rng(16)
    dev_items, keep = _items(sf, [_random_mask(rng, 100, 1)])
    scnt, odoc, ocnt, olim = sf.filled(64), sf.filled(R.MAX_ROWS), sf.filled(1), sf.filled(1)
    it, sc, od, oc, ol = (x.data_ptr() for x in (dev_items, scnt, odoc, ocnt, olim))
    bad = R.INVALID_VALUE
    for k, wgs in ((0, 1), (R.MAX_ROWS + 1, 1), (5, 0), (5, F.MAX_WGS + 1)):
        assert sf.count(it, 1, k, wgs, sc, sf.stream) == bad
        assert sf.first(it, 1, k, wgs, sc, od, oc, 0, None, sf.stream) == bad
    assert sf.count(it, -1, 5, 2, sc, sf.stream) == bad and sf.first(it, -1, 5, 1, sc, od, oc, 0, None, sf.stream) == bad
    assert sf.count(None, 1, 5, 2, sc, sf.stream) == bad and sf.count(it, 1, 5, 2, None, sf.stream) == bad
    assert sf.first(None, 1, 5, 1, sc, od, oc, 0, None, sf.stream) == bad
    assert sf.first(it, 1, 5, 1, sc, None, oc, 0, None, sf.stream) == bad
    assert sf.first(it, 1, 5, 1, sc, od, None, 0, None, sf.stream) == bad
    assert sf.first(it, 1, 5, 2, None, od, oc, 0, None, sf.stream) == bad    # several workgroups need the counts
    assert sf.first(it, 1, 5, 1, None, od, oc, 0, ol, sf.stream) == bad      # a limit outside 1 .. K
    assert sf.first(it, 1, 5, 1, None, od, oc, 6, ol, sf.stream) == bad
    assert sf.first(it, 0, 5, 1, None, od, oc, 0, None, sf.stream) == 0      # no items: nothing launched
    sf.sync()
    for x in (scnt, odoc, ocnt, olim):
        assert (x.cpu().numpy() == S32).all()
