"""The multi-value selection kernels (pinot_amd/csrc/pgx_select.hip: pgx_select_mv_offsets, pgx_select_mv_bases,
pgx_select_mv_gather) launched directly on torch device buffers over hand-built (start, packed values) pairs and
compared with the numpy model of tests/select_mv_ref.py.  Every output is pre-filled with a sentinel and has guard
words past its end; both must come back untouched.  The docIds at ranks at or past an item's count are the sentinel
too (a negative number): a kernel that read one as a doc would not get past the model."""
import ctypes as C

import numpy as np
import pytest

from tests import select_mv_ref as M

pytestmark = pytest.mark.gpu

GUARD = 64
S32 = np.int32(-1515870811)            # 0xA5A5A5A5
S64 = np.int64(0x5A5A5A5A5A5A5A5A)


class _MK:
    def __init__(self):
        import torch
        from pinot_amd import native as N
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.offsets, self.bases, self.gather = M.bind(N.lib())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.dev)

    def filled(self, n, value, dtype):
        return self.torch.full((n + GUARD,), int(value), dtype=dtype, device=self.dev)

    def sync(self):
        self.torch.cuda.synchronize(self.dev)


@pytest.fixture(scope="module")
def mk():
    return _MK()


def _column(rng, lengths, bits):
    """One multi-value column of one item: (start, values, bits), the values using the whole stored width."""
    start = M.starts_of(lengths)
    hi = (1 << bits) if bits < 32 else (1 << 32) - 1
    return start, rng.integers(0, hi, int(start[-1]), dtype=np.uint64), bits


def _docs(order, count, k):
    """An item's k docIds as the merge leaves them: `count` docs, then the sentinel."""
    d = np.full(k, S32, np.int32)
    d[:count] = np.asarray(order[:count], dtype=np.int32)
    return d


def _launch(mk, cols, docs, counts, k, wgs=1, capacity=None, bad=None, refuses=None):
    """The three launches over cols[m][i] = (start, values, bits); returns ((rel_off, totals, bases, values) with their
    guards, the launchers' statuses).  For the refusals: `bad` changes the arguments of launcher `refuses` (0 offsets,
    1 bases, 2 gather), which must answer hipErrorInvalidValue; the launchers before it run as they are, none after."""
    t = mk.torch
    nmv, ni = len(cols), len(docs)
    pairs = nmv * ni
    keep = []
    arr = (M.SelMvCol * max(1, pairs))()
    for m in range(nmv):
        for i in range(ni):
            start, values, bits = cols[m][i]
            ds, dv = mk.up(np.asarray(start, dtype=np.int32)), mk.up(M.pack_values(values, bits))
            keep += [ds, dv]
            arr[m * ni + i].values, arr[m * ni + i].start, arr[m * ni + i].bits = dv.data_ptr(), ds.data_ptr(), bits
    _, _, ebases, _ = M.mv_model([[c[:2] for c in col] for col in cols], docs, counts, k)
    cap = int(ebases[-1]) if capacity is None else capacity
    dcols = mk.up(np.frombuffer(bytes(arr), dtype=np.uint8))
    odoc = mk.up(np.concatenate([np.concatenate(docs), np.full(GUARD, S32, np.int32)])).view(t.int32)
    ocnt = mk.up(np.asarray(counts, dtype=np.int32)).view(t.int32)
    rel = mk.filled(pairs * (k + 1), S32, t.int32)
    tot = mk.filled(pairs, S32, t.int32)
    bas = mk.filled(pairs + 1, S64, t.int64)
    val = mk.filled(max(cap, int(ebases[-1])), S32, t.int32)
    a = {"cols": dcols.data_ptr(), "ni": ni, "nmv": nmv, "k": k, "wgs": wgs, "odoc": odoc.data_ptr(),
         "ocnt": ocnt.data_ptr(), "rel": rel.data_ptr(), "tot": tot.data_ptr(), "bas": bas.data_ptr(),
         "val": val.data_ptr(), "cap": cap, "pairs": pairs}
    calls = [lambda a: mk.offsets(a["cols"], a["ni"], a["nmv"], a["k"], a["odoc"], a["ocnt"], a["rel"], a["tot"],
                                  mk.stream),
             lambda a: mk.bases(a["tot"], a["pairs"], a["bas"], mk.stream),
             lambda a: mk.gather(a["cols"], a["ni"], a["nmv"], a["k"], a["wgs"], a["odoc"], a["ocnt"], a["rel"],
                                 a["bas"], a["val"], a["cap"], mk.stream)]
    sts = []
    for i, call in enumerate(calls):
        if i == refuses:
            changed = dict(a)
            bad(changed)
            sts.append(call(changed))
            assert sts[-1] == M.INVALID_VALUE
            break
        sts.append(call(a))
        assert sts[-1] == 0
    mk.sync()
    return [x.cpu().numpy() for x in (rel, tot, bas, val)], sts


def _check(mk, cols, docs, counts, k, wgs=1):
    (rel, tot, bas, val), _ = _launch(mk, cols, docs, counts, k, wgs)
    pairs = len(cols) * len(docs)
    erel, etot, ebas, eval_ = M.mv_model([[c[:2] for c in col] for col in cols], docs, counts, k)
    np.testing.assert_array_equal(rel[:pairs * (k + 1)].reshape(pairs, k + 1), erel)
    np.testing.assert_array_equal(tot[:pairs], etot)
    np.testing.assert_array_equal(bas[:pairs + 1], ebas)
    np.testing.assert_array_equal(val[:len(eval_)], eval_)
    assert (rel[pairs * (k + 1):] == S32).all() and (tot[pairs:] == S32).all() and (bas[pairs + 1:] == S64).all()
    assert (val[len(eval_):] == S32).all()  # nothing past the grand total
    return erel, ebas, eval_


def _lengths(rng, n):
    """Docs of 0 .. 4 values; doc 0 has one value, doc 1 none, doc 2 300 (more than a workgroup's 256 threads take in
    one step), the last doc two."""
    ln = rng.integers(0, 5, n)
    ln[:3] = (1, 0, 300)
    ln[-1] = 2
    return ln


@pytest.mark.parametrize("k", [1, 10, 2048])
@pytest.mark.parametrize("bits", [1, 7, 17, 32])
def test_widths_and_k(mk, bits, k):
    """Stored widths 1, 7, 17 and 32 (7 and 17: values whose bits straddle a dword, at every phase over the stream), K =
    1, 10 and PGX_SEL_MAX_ROWS; the docs with 300, 0 and 1 values and the segment's last doc rank first."""
    rng = np.random.default_rng(100 * bits + k)
    n = 3000
    col = _column(rng, _lengths(rng, n), bits)
    order = np.concatenate([[2, 1, 0, n - 1], 4 + rng.permutation(n - 5)])
    if k == 1:  # one doc per item: the long doc, the last doc, the empty doc
        docs = [_docs([2], 1, 1), _docs([n - 1], 1, 1), _docs([1], 1, 1)]
        erel, _, _ = _check(mk, [[col, col, col]], docs, (1, 1, 1), 1)
        assert erel[:, 1].tolist() == [300, 2, 0]
    else:
        erel, _, _ = _check(mk, [[col]], [_docs(order, k, k)], (k,), k, wgs=1 if k == 10 else 3)
        assert erel[0, :5].tolist() == [0, 300, 300, 301, 303]


def test_five_items_two_columns(mk):
    """Five items and two multi-value columns of different widths in one launch (the bases run across the pairs of both
    columns); an item with count 0 between two full ones, items with counts below K, every unused rank the sentinel."""
    rng = np.random.default_rng(5)
    k = 10
    sizes, counts = (2500, 300, 64, 9, 1), (10, 0, 3, 9, 1)
    lens = [_lengths(rng, n) if n >= 4 else np.array([3]) for n in sizes]
    cols = [[_column(rng, ln, bits) for ln in lens] for bits in (7, 17)]
    docs = [_docs(rng.permutation(n), c, k) for n, c in zip(sizes, counts)]
    first = [2, 1, sizes[0] - 1, 0]
    docs[0] = _docs(first + [d for d in rng.permutation(sizes[0]) if d not in first], k, k)
    erel, ebas, _ = _check(mk, cols, docs, counts, k, wgs=2)
    assert erel[1].tolist() == [0] * (k + 1) and ebas[1] == ebas[2]  # the empty item owns nothing
    assert ebas[5] > 0 and ebas[-1] == 2 * ebas[5]                   # the second column repeats the first's counts
    assert (erel[2, 3:] == erel[2, 3]).all()                         # ranks past the count own nothing


def test_workgroups_per_pair_do_not_change_the_result(mk):
    rng = np.random.default_rng(6)
    n, k = 2000, 100
    ln = rng.integers(0, 40, n)
    col = _column(rng, ln, 13)
    docs = [_docs(rng.permutation(n), k, k)]
    outs = [_launch(mk, [[col]], docs, (k,), k, wgs=w)[0][3].tobytes() for w in (1, 5, 64)]
    assert outs[0] == outs[1] == outs[2]
    _check(mk, [[col]], docs, (k,), k, wgs=5)


def test_capacity_bounds_the_stores(mk):
    """A value buffer shorter than the grand total: the values below the capacity are stored, nothing at or past it."""
    rng = np.random.default_rng(7)
    n, k = 500, 10
    col = _column(rng, _lengths(rng, n), 9)
    docs = [_docs([2, 5, 1, n - 1, 8, 9, 10, 11, 12, 13], k, k)]
    _, _, _, evalues = M.mv_model([[col[:2]]], docs, (k,), k)
    cap = len(evalues) - 37
    (_, _, bas, val), _ = _launch(mk, [[col]], docs, (k,), k, capacity=cap)
    assert bas[1] == len(evalues)
    np.testing.assert_array_equal(val[:cap], evalues[:cap])
    assert (val[cap:] == S32).all()


def test_launchers_refuse_bad_arguments(mk):
    rng = np.random.default_rng(8)
    n, k = 100, 5
    col = _column(rng, rng.integers(0, 4, n), 6)
    docs = [_docs(rng.permutation(n), k, k)]

    def refused(change, which):
        """Launcher `which` (0 offsets, 1 bases, 2 gather) answers hipErrorInvalidValue and launches nothing: what it
        and the launchers after it write stays the sentinel."""
        (rel, tot, bas, val), sts = _launch(mk, [[col]], docs, (k,), k, bad=change, refuses=which)
        assert sts == [0] * which + [M.INVALID_VALUE]
        assert (val == S32).all()
        if which < 2:
            assert (bas == S64).all()
        if which < 1:
            assert (rel == S32).all() and (tot == S32).all()

    refused(lambda a: a.update(k=M.MAX_ROWS + 1), 0)
    refused(lambda a: a.update(k=0), 0)
    refused(lambda a: a.update(ni=-1), 0)
    refused(lambda a: a.update(ni=65536), 0)
    refused(lambda a: a.update(nmv=-1), 0)
    refused(lambda a: a.update(cols=None), 0)
    refused(lambda a: a.update(rel=None), 0)
    refused(lambda a: a.update(pairs=-1), 1)
    refused(lambda a: a.update(bas=None), 1)
    refused(lambda a: a.update(tot=None), 1)
    refused(lambda a: a.update(k=M.MAX_ROWS + 1), 2)
    refused(lambda a: a.update(wgs=0), 2)
    refused(lambda a: a.update(wgs=65), 2)
    refused(lambda a: a.update(cap=-1), 2)
    refused(lambda a: a.update(val=None), 2)
    refused(lambda a: a.update(bas=None), 2)
    mk.sync()
