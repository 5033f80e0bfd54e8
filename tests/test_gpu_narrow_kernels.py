"""Direct tests of the narrow group-by kernels (pinot_amd/csrc/pgx_narrow.hip: pgx_narrow_split<W>,
pgx_narrow_aggregate<IMG, SUM, MN, MX, W>, pgx_narrow_compact), launched through libpgx.so's launchers on torch device
buffers and compared with the plain numpy / Python-int model of tests/narrow_ref.py at small, adversarial shapes.

Every output buffer is pre-filled with a sentinel and has guard words past its end; every test asserts that whatever
it did not expect to be written still holds the sentinel.  Order within a partition and among output groups is
arbitrary, so multisets and dicts are compared."""
import collections
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import narrow_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
S32 = 0xA5A5A5A5
S64 = 0x5A5A5A5A5A5A5A5A
M64 = R.M64


class _NK:
    def __init__(self):
        import torch
        from pinot_amd import native as N
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.split, self.agg, self.scratch_words = R.bind(N.lib())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        """numpy array of an unsigned type -> device tensor of the signed type of the same width."""
        a = np.ascontiguousarray(a)
        signed = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
        return self.torch.from_numpy(a.view(signed).copy()).to(self.dev)

    def down(self, t, dtype):
        return t.cpu().numpy().view(dtype)

    def sync(self):
        self.torch.cuda.synchronize(self.dev)


@pytest.fixture(scope="module")
def nk():
    return _NK()


def _ptr(t):
    return None if t is None else t.data_ptr()


# =====================================================================================================================
# split
# =====================================================================================================================
def _split_buffers(nk, inp):
    nb, nwg, cap1, W = len(inp["slabs"]), inp["nwg"], inp["cap1"], inp["W"]
    nsub = 1 << inp["k2"]
    # slots past a slab's records hold all-ones: a record the kernel must not read
    lo = np.full(nb * nwg * cap1, 0xFFFFFFFF, dtype=np.uint32)
    hi = np.full(nb * nwg * cap1, 0xFFFF, dtype=np.uint16)
    for b, bucket in enumerate(inp["slabs"]):
        for w, s in enumerate(bucket):
            at = (b * nwg + w) * cap1
            lo[at:at + len(s)] = (s & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            hi[at:at + len(s)] = (s >> np.uint64(32)).astype(np.uint16)
    cnt1 = np.array(inp["claim"], dtype=np.uint64).reshape(-1)
    out = np.full(nb * nsub * inp["cap2"] * W + GUARD, S32, dtype=np.uint32)
    cnt2 = np.full(nb * nsub + GUARD, S32, dtype=np.uint32)
    ovf = np.array([0, S64], dtype=np.uint64)
    return dict(lo=nk.up(lo), hi=nk.up(hi) if inp["hi"] else None, cnt1=nk.up(cnt1), out=nk.up(out), cnt2=nk.up(cnt2),
                ovf=nk.up(ovf), nb=nb, nsub=nsub)


def _launch_split(nk, inp, B, **over):
    a = dict(lo=_ptr(B["lo"]), hi=_ptr(B["hi"]), cnt1=_ptr(B["cnt1"]), nb=B["nb"], nwg=inp["nwg"], cap1=inp["cap1"],
             rb1=inp["rb1"], k2=inp["k2"], out=_ptr(B["out"]), cap2=inp["cap2"], cnt2=_ptr(B["cnt2"]),
             ovf=_ptr(B["ovf"]), wide=int(inp["W"] == 2))
    a.update(over)
    rc = nk.split(a["lo"], a["hi"], a["cnt1"], a["nb"], a["nwg"], a["cap1"], a["rb1"], a["k2"], a["out"], a["cap2"],
                  a["cnt2"], a["ovf"], a["wide"], nk.stream)
    nk.sync()
    return rc


def _untouched_split(nk, B):
    out = nk.down(B["out"], np.uint32)
    cnt2 = nk.down(B["cnt2"], np.uint32)
    ovf = nk.down(B["ovf"], np.uint64)
    return bool((out == S32).all() and (cnt2 == S32).all() and ovf[0] == 0 and ovf[1] == S64)


def _run_split(nk, inp):
    """Launch the split on inp and check it in full: cnt2 exact, every partition's multiset equal to the reference
    (an overflowing partition: its first cap2 records a sub-multiset), ovf exact, everything else untouched."""
    B = _split_buffers(nk, inp)
    assert _launch_split(nk, inp, B) == 0
    W, cap2, nparts = inp["W"], inp["cap2"], B["nb"] * B["nsub"]
    rdt, sent = (np.uint32, S32) if W == 1 else (np.uint64, (S32 << 32) | S32)
    out = nk.down(B["out"], np.uint32)
    assert (out[nparts * cap2 * W:] == S32).all(), "written past the output buffer"
    recs = out[:nparts * cap2 * W].view(rdt).reshape(nparts, cap2)
    cnt2 = nk.down(B["cnt2"], np.uint32)
    assert (cnt2[nparts:] == S32).all()
    ref = R.split_ref(inp["slabs"], inp["rb1"], inp["k2"])
    exp_cnt = np.array([len(ref.get(p, ())) for p in range(nparts)], dtype=np.uint32)
    assert (cnt2[:nparts] == exp_cnt).all(), np.flatnonzero(cnt2[:nparts] != exp_cnt)[:8]
    over = 0
    for p in range(nparts):
        n = int(exp_cnt[p])
        assert (recs[p, min(n, cap2):] == sent).all(), "partition %d written past its records" % p
        if n <= cap2:
            assert np.sort(recs[p, :n]).tolist() == ref.get(p, []), "partition %d" % p
        else:
            over += 1
            extra = collections.Counter(recs[p].tolist()) - collections.Counter(ref[p])
            assert not extra, "partition %d holds records that are not its own" % p
    ovf = nk.down(B["ovf"], np.uint64)
    assert int(ovf[0]) == over and int(ovf[1]) == S64
    return over


_A = [(n, a) for n, a in R.split_inputs() if a["case"] in ("slabs", "rb1_48", "rb2_0")]


@pytest.mark.parametrize("args", [a for _, a in _A], ids=[n for n, _ in _A])
def test_split_slabs_and_rounds(nk, args):
    """a: slab fills {0, 20000, 8192, 1}, a slab whose cnt1 exceeds cap1 (only cap1 records are read; the slots past a
    slab's records hold a record that must not appear), an empty bucket; k2 in {0, 1, 6, 10}; hi null and non-null
    (records wider than 32 bits); rb1 = 48; k2 = rb1 (rb2 = 0)."""
    inp = R.split_input(**args)
    assert _run_split(nk, inp) == 0


@pytest.mark.parametrize("W", [1, 2])
def test_split_ring_wrap(nk, W):
    """b: k2 = 10; the hot sub-buckets' rings (32 / 16 records) are passed 10 / 20 times, never by more than a ring
    per round."""
    inp = R.split_input("wrap", W)
    for bucket in inp["slabs"]:
        subs = [R.split_subs(s, inp["rb1"], 10) for s in bucket]
        assert np.bincount(np.concatenate(subs)).max() >= 10 * (32 // W)
        assert max(np.bincount(s).max() for s in subs) + 16 // W - 1 <= 32 // W  # pending + a round's fit the ring
    assert _run_split(nk, inp) == 0


@pytest.mark.parametrize("k2", [6, 10])
@pytest.mark.parametrize("W", [1, 2])
def test_split_skew(nk, W, k2):
    """c: 60 % of a bucket on one sub-bucket, rounds that bring it many rings' worth: straight-out stores, then units
    whose first positions lie below V."""
    inp = R.split_input("skew", W, k2=k2, hi=(W == 2))
    ring = (32768 // W) >> k2
    for bucket in inp["slabs"]:
        assert np.bincount(R.split_subs(bucket[0], inp["rb1"], k2)).max() > 3 * ring
    assert _run_split(nk, inp) == 0


@pytest.mark.parametrize("W", [1, 2])
def test_split_cap2_overflow(nk, W):
    """d: two sub-buckets per bucket receive more than cap2 (one far more, skewed; one 5 more, through the ring)."""
    inp = R.split_input("overflow", W, hi=(W == 2))
    assert _run_split(nk, inp) == 4


@pytest.mark.parametrize("W", [1, 2])
def test_split_worst_case_unit_list(nk, W):
    """e: the last round lists exactly the kernel's bound of units (1920 at W = 2, 1472 at W = 1; checked on the CPU by
    tests/test_narrow_ref.py).  Written for the kernel whose list holds that bound: not to be run on an older one."""
    inp = R.split_input("worst", W)
    assert _run_split(nk, inp) == 0


def test_split_argument_checks(nk):
    """f: refused launches return hipErrorInvalidValue and run no kernel (every buffer keeps its sentinel)."""
    for W in (1, 2):
        inp = R.split_input("wrap", W)
        B = _split_buffers(nk, inp)
        bad = [dict(cap2=inp["cap2"] + 8), dict(cap2=inp["cap2"] - 16 + 4), dict(cap2=0), dict(k2=11), dict(k2=-1),
               dict(rb1=9, k2=10), dict(rb1=49), dict(nwg=1025), dict(nwg=0), dict(cap1=0), dict(cap2=1 << 32),
               dict(lo=None), dict(out=None), dict(cnt1=None), dict(cnt2=None), dict(ovf=None)]
        for over in bad:
            assert _launch_split(nk, inp, B, **over) == R.INVALID_VALUE, over
        assert _untouched_split(nk, B)
        assert _launch_split(nk, inp, B, nb=0) == 0  # nothing to do
        assert _untouched_split(nk, B)


# =====================================================================================================================
# aggregate
# =====================================================================================================================
KINDS = {"0": (0, 0), "1": (1, 0), "2": (2, 0), "3": (3, 0), "4": (4, 0), "3w": (3, 1), "5": (5, 0), "5w": (5, 1),
         "6": (6, 0), "6w": (6, 1)}
KIND_MASKS = [(k, m) for k in KINDS for m in range(8) if not (k == "0" and m & 4)]  # mask: SUM 4, MIN 2, MAX 1


def _sizes(W):
    B = R.batch(W)
    return [0, 1, 3, 4, 5, B - 1, B, B + 1, 2 * B + 1, 3 * B + 2]


def _sorted_rel(rng, card, step):
    return np.cumsum(rng.integers(1, step + 1, card)).astype(np.int64)


def _values(kind, rng, rb2, W, img4=(11, 4, 130, 1000), dyadic=True):
    """The value side of a dataset for one kind: dict(card (value fields are < card), value_of, and the launcher's
    vbase / img / img_words / img_sh / vdict)."""
    ik = KINDS[kind][0]
    v = dict(vbase=0, img=None, img_words=0, img_sh=0, vdict=None)
    if ik == 0:  # MIN / MAX over dictIds of a sorted dictionary, looked up at the flush
        card = 3000
        d = np.sort(rng.integers(-(1 << 62), 1 << 62, card))
        v.update(card=card, vdict=d.astype(np.int64), value_of=lambda f: int(d[f]))
    elif ik in (1, 2, 4):  # sorted dictionary, image of value - vbase in LDS
        vbase = -(10 ** 12) - 7
        if ik == 1:
            rel = _sorted_rel(rng, 3000, 10 ** 6)
            img, sh = R.img1(rel)
        elif ik == 2:
            rel = _sorted_rel(rng, 64 << 4, 4000)  # every one of the 64 blocks is used
            img, sh = R.img2(rel, 4)
        else:
            b, bsh, step, card = img4
            rel = _sorted_rel(rng, card, step) + 999
            img, sh = R.img4(rel, bsh, b)
        assert all(R.img_value(ik, img, sh, d) == rel[d] for d in (0, len(rel) // 2, len(rel) - 1))
        v.update(card=len(rel), vbase=vbase, img=img, img_words=len(img), img_sh=sh,
                 value_of=lambda f: vbase + int(rel[f]))
    elif ik == 3:  # the field is value - vbase
        vbase = -(1 << 40) + 5
        v.update(card=1 << (32 if W == 2 else 32 - rb2), vbase=vbase, value_of=lambda f: vbase + f)
    elif ik == 5:  # the field indexes a global table of u32 value - vbase
        vbase = -123456789012
        t = rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32)
        t[:2] = (0, 0xFFFFFFFF)
        v.update(card=300, vbase=vbase, img=t, img_words=300, value_of=lambda f: vbase + int(t[f]))
    else:  # ... of doubles
        if dyadic:  # multiples of 1/8 below 2^20: every sum is exact in any order
            t = rng.integers(-(1 << 23) + 1, 1 << 23, 300).astype(np.float64) / 8.0
            t[:3] = (0.0, -0.0, -(2.0 ** 20) + 0.125)
        else:
            t = rng.standard_normal(300) * np.exp(rng.uniform(-20, 20, 300))
        v.update(card=300, img=t.view(np.uint64), img_words=300, value_of=lambda f: float(t[f]))
    return v


def _make_parts(rng, sizes, rb2, card, max_groups=40):
    """Partitions of the given sizes: up to max_groups distinct key bits each (never the all-ones key, which the tails
    use), value fields uniform in [0, card) with 0 and card - 1 present in every partition of 2 or more records."""
    parts = []
    nkeys = max(1, (1 << rb2) - 1)
    for n in sizes:
        keys = np.unique(rng.integers(0, nkeys, min(max_groups, max(1, n)))).astype(np.uint64)
        g = len(keys)
        f = rng.integers(0, card, n, dtype=np.uint64)
        if n >= 2:
            f[0], f[-1] = 0, card - 1
        parts.append(keys[rng.integers(0, g, n)] | (f << np.uint64(rb2)))
    return parts


def _run_agg(nk, parts, *, W, cap2, rb2, K, vals, mask, kind, cshift=44, ocap=None, grid=1, prange=True, tail=None,
             tail_field=0, over=None):
    """Launch the aggregation + compaction on parts (the records of partition p; the slots from cnt2 to cap2 hold
    `tail` records, by default poison: the all-ones key the partition does not contain with an in-range value field).
    Returns dict(rc, n, lost, key[ocap], plane[4][ocap], prange[8], clean)."""
    ik, wide = KINDS[kind]
    assert wide == W - 1
    nparts = len(parts)
    rdt = np.uint32 if W == 1 else np.uint64
    if tail is None:
        tail = ((1 << rb2) - 1) | (tail_field << rb2)
    buf = np.full((nparts, cap2), tail, dtype=rdt)
    for p, r in enumerate(parts):
        assert len(r) <= cap2 and (len(r) == 0 or int(r.max()) < 1 << (32 * W))
        buf[p, :len(r)] = r.astype(rdt)
    cnt2 = np.array([len(r) for r in parts], dtype=np.uint32)
    if ocap is None:
        ocap = sum(len(np.unique(r & np.uint64((1 << rb2) - 1))) for r in parts) + 7
    t = nk.torch
    d_in, d_cnt = nk.up(buf.reshape(-1)), nk.up(cnt2)
    okey = nk.up(np.full(ocap + GUARD, S64, dtype=np.uint64))
    oplane = nk.up(np.full(4 * ocap + GUARD, S64, dtype=np.uint64))
    ctr = nk.up(np.array([0, 0, 0, 0, S64, S64], dtype=np.uint64))
    pr = nk.up(np.array([M64] * 4 + [0] * 4 + [S64] * 2, dtype=np.uint64))
    img = nk.up(vals["img"]) if vals["img"] is not None else None
    vdict = nk.up(vals["vdict"].view(np.uint64)) if vals["vdict"] is not None else None
    sw = nk.scratch_words(nparts, ik, max(grid, 1))
    scratch = t.full((sw + GUARD,), S64, dtype=t.int64, device=nk.dev)
    a = dict(inp=_ptr(d_in), cnt2=_ptr(d_cnt), cap2=cap2, nparts=nparts, rb2=rb2, K=K, vbase=vals["vbase"], ik=ik,
             img=_ptr(img), img_words=vals["img_words"], img_sh=vals["img_sh"], vdict=_ptr(vdict), s=(mask >> 2) & 1,
             mn=(mask >> 1) & 1, mx=mask & 1, cshift=cshift, okey=_ptr(okey), oplane=_ptr(oplane), ocap=ocap,
             ctr=_ptr(ctr), prange=_ptr(pr) if prange else None, grid=grid, scratch=_ptr(scratch), sw=sw, wide=wide)
    a.update(over or {})  # (argument checks: what the launcher is given instead)
    rc = nk.agg(a["inp"], a["cnt2"], a["cap2"], a["nparts"], a["rb2"], a["K"], a["vbase"], a["ik"], a["img"],
                a["img_words"], a["img_sh"], a["vdict"], a["s"], a["mn"], a["mx"], a["cshift"], a["okey"], a["oplane"],
                a["ocap"], a["ctr"], a["prange"], a["grid"], a["scratch"], a["sw"], a["wide"], nk.stream)
    nk.sync()
    k, pl, c, r = (nk.down(x, np.uint64) for x in (okey, oplane, ctr, pr))
    sc = nk.down(scratch, np.uint64)
    clean = bool((k[ocap:] == S64).all() and (pl[4 * ocap:] == S64).all() and (c[4:] == S64).all() and
                 (r[8:] == S64).all() and (sc[sw:] == S64).all() and c[1] == 0 and c[2] == 0)
    return dict(rc=rc, n=int(c[0]), lost=int(c[3]), key=k[:ocap], plane=pl[:4 * ocap].reshape(4, ocap), prange=r[:8],
                clean=clean, ocap=ocap)


def _expected(ref, rb2, K):
    """{packed key: reference entry}."""
    exp = {R.group_key(p, r2, rb2, K): e for (p, r2), e in ref.items()}
    assert len(exp) == len(ref)
    return exp


def _check_agg(res, ref, rb2, K, mask, f64=False, prange=True, sum_bound=False):
    """Every group once, with the rebuilt key, its count and the requested functions; the rows past the groups and
    the guards untouched; the trim-key ranges of COUNT and of the requested functions."""
    assert res["rc"] == 0
    exp = _expected(ref, rb2, K)
    n = len(exp)
    assert res["n"] == n and res["lost"] == 0 and res["clean"]
    assert (res["key"][n:] == S64).all() and (res["plane"][:, n:] == S64).all()
    keys = res["key"][:n].tolist()
    assert len(set(keys)) == n and set(keys) == set(exp)
    pl = res["plane"]
    ord_of = R.ordered_f64 if f64 else R.ordered_i64
    for i, k in enumerate(keys):
        e = exp[k]
        assert int(pl[0, i]) == e[0], ("count", k)
        if mask & 4:
            if f64:
                got = float(pl[1, i:i + 1].view(np.float64)[0])
                if sum_bound:  # any-order summation bound, doubled: n * 2^-52 * sum |v|
                    assert abs(got - e[1]) <= e[0] * 2.0 ** -52 * e[4], ("sum", k, got, e[1])
                else:
                    assert got == e[1], ("sum", k, got, e[1])
            else:
                assert int(pl[1, i]) == e[1] & M64, ("sum", k)
        if mask & 2:
            assert int(pl[2, i]) == ord_of(e[2]), ("min", k)
        if mask & 1:
            assert int(pl[3, i]) == ord_of(e[3]), ("max", k)
    if prange and not f64:
        pr = [int(x) for x in res["prange"]]
        if not exp:
            assert pr == [M64] * 4 + [0] * 4
            return
        tk = [[e[0] for e in exp.values()], [(e[1] & M64) ^ R.SIGN for e in exp.values()],
              [~R.ordered_i64(e[2]) & M64 for e in exp.values()], [R.ordered_i64(e[3]) for e in exp.values()]]
        for kd, need in enumerate((True, mask & 4, mask & 2, mask & 1)):
            if need:
                assert pr[kd] == min(tk[kd]) and pr[4 + kd] == max(tk[kd]), ("prange", kd)


@functools.lru_cache(maxsize=None)
def _dataset(kind, variant="every", rb2=12, K=20, img4=(11, 4, 130, 1000), dyadic=True):
    """One small dataset per kind (and its reference, computed once): about 40 partitions of the boundary sizes, in
    an order that puts empty partitions between full ones.  variant "tails": no size is a multiple of 4."""
    W = KINDS[kind][1] + 1
    rng = np.random.default_rng([sum(map(ord, kind + variant)), rb2, K, img4[0], int(dyadic)])
    vals = _values(kind, rng, rb2, W, img4, dyadic)
    B = R.batch(W)
    if variant == "every":
        sizes = list(rng.permutation(_sizes(W) * 4))
    else:
        sizes = [1, 3, 5, 7, B - 1, B + 1, 2 * B + 1, 3 * B + 3, B - 3, 2, 6, 2 * B - 1] * 2
        sizes = [s | 1 if W == 2 else s for s in sizes]
        assert all(s % (4 // W) for s in sizes)
    sizes = sizes[:1 << min(K - rb2, 20)]  # partition << rb2 | key bits is a mix value: below 2^K
    parts = _make_parts(rng, sizes, rb2, vals["card"])
    ref = R.groupby_ref(parts, rb2, vals["value_of"])
    return dict(W=W, parts=parts, vals=vals, ref=ref, rb2=rb2, K=K, cap2=3 * B + 4)


def _run_dataset(nk, kind, D, mask, grid, **kw):
    return _run_agg(nk, D["parts"], W=D["W"], cap2=D["cap2"], rb2=D["rb2"], K=D["K"], vals=D["vals"], mask=mask,
                    kind=kind, grid=grid, prange=KINDS[kind][0] != 6, **kw)


@pytest.mark.parametrize("kind,mask", KIND_MASKS, ids=["%s-%d" % km for km in KIND_MASKS])
def test_aggregate_every_instantiation(nk, kind, mask):
    """g: each of the 76 instantiations the launcher selects, on 40 partitions of the boundary sizes (0, 1, 3, 4, 5,
    BATCH - 1, BATCH, BATCH + 1, 2 BATCH + 1, 3 BATCH + 2), with grid 1 and 3 (wavefronts walk several partitions, empty
    ones between full ones).  Sorted dictionaries and images, negative vbase, all 64 blocks of IMG 2, the last dictId
    of IMG 4 (which reads the pad dword), full 32-bit value offsets at W = 2."""
    D = _dataset(kind)
    for grid in (1, 3):
        res = _run_dataset(nk, kind, D, mask, grid)
        _check_agg(res, D["ref"], D["rb2"], D["K"], mask, f64=KINDS[kind][0] == 6)


@pytest.mark.parametrize("b,bsh,step,card", [(1, 1, 1, 601), (16, 6, 1000, 777)], ids=["b1", "b16"])
def test_aggregate_packed_image_widths(nk, b, bsh, step, card):
    """g: IMG 4 with 1-bit and 16-bit offsets (b = 11, whose offsets straddle dwords, is the dataset of the test
    above)."""
    D = _dataset("4", img4=(b, bsh, step, card))
    res = _run_dataset(nk, "4", D, 7, 3)
    _check_agg(res, D["ref"], D["rb2"], D["K"], 7)


@pytest.mark.parametrize("wide", [0, 1], ids=["W1", "W2"])
@pytest.mark.parametrize("rb2,K", [(0, 9), (1, 9), (16, 34), (31, 34), (0, 64), (1, 64), (16, 64), (31, 64)])
def test_aggregate_geometry_edges(nk, rb2, K, wide):
    """h: rb2 in {0, 1, 16, 31} x keybits in {9, 34, 64} (partition index and key bits are chosen directly and the
    expected key is the inverse mix of the two, so few partitions do even for 64-bit keys)."""
    kind = "3w" if wide else "3"
    D = _dataset(kind, rb2=rb2, K=K)
    for grid in (1, 3):
        res = _run_dataset(nk, kind, D, 7, grid)
        _check_agg(res, D["ref"], rb2, K, 7)


@pytest.mark.parametrize("wide,rb2", [(0, 0), (1, 16)], ids=["W1", "W2"])
def test_aggregate_cshift_exactly_tight(nk, wide, rb2):
    """h: the largest group has cap2 records whose value offsets sum to 2^cshift - 1: one more would carry into the
    count that shares the 64-bit LDS word."""
    W, cap2, cshift = wide + 1, 2048, 40
    kind = "3w" if wide else "3"
    rng = np.random.default_rng(40 + wide)
    vals = _values(kind, rng, rb2, W)
    q, r = divmod((1 << cshift) - 1, cap2)
    offs = np.full(cap2, q, dtype=np.uint64)
    offs[:r] += np.uint64(1)
    assert int(offs.sum()) == (1 << cshift) - 1 and int(offs.max()) < 1 << 32
    key = np.uint64(((1 << rb2) - 1) // 3)
    full = rng.permutation(offs << np.uint64(rb2)) | key
    parts = _make_parts(rng, [700, 0, 5], rb2, 1 << 20) + [full] + _make_parts(rng, [1, 1030], rb2, 1 << 20)
    ref = R.groupby_ref(parts, rb2, vals["value_of"])
    assert ref[(3, int(key))][0] == cap2
    res = _run_agg(nk, parts, W=W, cap2=cap2, rb2=rb2, K=40, vals=vals, mask=7, kind=kind, cshift=cshift, grid=1)
    _check_agg(res, ref, rb2, 40, 7)


@pytest.mark.parametrize("kind", list(KINDS))
def test_aggregate_tails_poison(nk, kind):
    """i: no cnt2 is a multiple of 4 (of 2 at W = 2), and the slots from cnt2 to cap2 hold well-formed records with a
    key the partition does not contain (and an in-range value field): aggregating one makes a spurious group."""
    D = _dataset(kind, "tails")
    mask = 3 if kind == "0" else 7
    res = _run_dataset(nk, kind, D, mask, 1, tail_field=D["vals"]["card"] - 1 if KINDS[kind][0] != 3 else 1)
    _check_agg(res, D["ref"], D["rb2"], D["K"], mask, f64=KINDS[kind][0] == 6)


@pytest.mark.parametrize("kind", ["5", "5w", "6", "6w"])
def test_aggregate_gather_stale_words_clamped(nk, kind):
    """i: the gathered kinds read the value table for every loaded word, also the up to three stale ones of a batch's
    last 16-byte load.  Here those are all-ones: an index far outside the 300-entry table, which the kernel clamps
    into it (the records are never aggregated)."""
    D = _dataset(kind, "tails")
    res = _run_dataset(nk, kind, D, 7, 1, tail=(1 << (32 * D["W"])) - 1)
    _check_agg(res, D["ref"], D["rb2"], D["K"], 7, f64=KINDS[kind][0] == 6)


def _one_bucket_parts(rng, nkeys, rb2=16):
    keys = rng.choice(1365, nkeys, replace=False).astype(np.uint64)  # (r2 * 48) >> 16 == 0
    assert all(R.home_bucket(int(k), rb2) == 0 for k in keys)
    pick = np.concatenate([np.arange(nkeys), rng.integers(0, nkeys, 1500 - nkeys)])
    f = rng.integers(0, 1 << 16, 1500, dtype=np.uint64)
    return [np.zeros(0, np.uint64), keys[rng.permutation(pick)] | (f << np.uint64(rb2)),
            _make_parts(rng, [37], rb2, 1 << 16)[0]]


@pytest.mark.parametrize("kind", ["3", "3w", "2"])
def test_aggregate_table_exactly_full(nk, kind):
    """j: one partition with exactly 192 distinct keys, all with home bucket 0: the table is full and every key but
    four was placed by probing."""
    rng = np.random.default_rng(192)
    W = KINDS[kind][1] + 1
    vals = _values(kind, rng, 16, W)
    parts = _one_bucket_parts(rng, 192)
    if kind == "2":
        parts = [(r & np.uint64(0xFFFF)) | ((r >> np.uint64(16)) % np.uint64(vals["card"])) << np.uint64(16)
                 for r in parts]
    ref = R.groupby_ref(parts, 16, vals["value_of"])
    assert sum(1 for p, _ in ref if p == 1) == 192
    res = _run_agg(nk, parts, W=W, cap2=1504, rb2=16, K=30, vals=vals, mask=7, kind=kind)
    _check_agg(res, ref, 16, 30, 7)


def test_aggregate_table_overflow_is_reported(nk):
    """j: 193 keys do not fit the 192 slots: the designed overflow path reports it in ctr[3] (the host then takes
    another path; nothing is asserted about the groups)."""
    rng = np.random.default_rng(193)
    vals = _values("3", rng, 16, 1)
    res = _run_agg(nk, _one_bucket_parts(rng, 193), W=1, cap2=1504, rb2=16, K=30, vals=vals, mask=7, kind="3")
    assert res["rc"] == 0 and res["lost"] >= 1 and res["clean"]


@pytest.mark.parametrize("kind", ["2", "4", "3w"])
def test_aggregate_ocap_clipping(nk, kind):
    """k: ocap smaller than the group count: ctr[0] holds the true total, ctr[3] reports it, and nothing is written
    at or past ocap in okey or past a plane's end; the rows below ocap are whole groups."""
    D = _dataset(kind)
    total = len(D["ref"])
    for ocap in (total - 1, total // 3):
        res = _run_dataset(nk, kind, D, 7, 3, ocap=ocap)
        assert res["rc"] == 0 and res["n"] == total and res["lost"] >= 1 and res["clean"]
        exp = _expected(D["ref"], D["rb2"], D["K"])
        keys = res["key"].tolist()
        assert len(set(keys)) == ocap and set(keys) <= set(exp)
        for i, k in enumerate(keys):  # a write past plane p's end would land in plane p + 1's first rows
            e = exp[k]
            got = [int(res["plane"][p, i]) for p in range(4)]
            assert got == [e[0], e[1] & M64, R.ordered_i64(e[2]), R.ordered_i64(e[3])], k


@pytest.mark.parametrize("kind", ["6", "6w"])
def test_aggregate_f64_non_dyadic_sum(nk, kind):
    """l: doubles of 40 binades: SUM within n * 2^-52 * sum |v| of math.fsum per group (twice the bound of a
    recursive summation in any order, (n - 1) * 2^-53 * sum |v| to first order); MIN / MAX exact."""
    D = _dataset(kind, dyadic=False)
    res = _run_dataset(nk, kind, D, 7, 3)
    _check_agg(res, D["ref"], D["rb2"], D["K"], 7, f64=True, sum_bound=True)


@pytest.mark.parametrize("kind", ["6", "6w"])
def test_aggregate_f64_signed_zeros(nk, kind):
    """l: -0.0 orders below 0.0 and above every negative: groups whose MIN or MAX is -0.0 (the dyadic table of the
    kind-6 datasets holds 0.0, -0.0 and a negative in its first entries)."""
    W = KINDS[kind][1] + 1
    vals = _values(kind, np.random.default_rng(60), 12, W)
    t = vals["img"].view(np.float64)
    assert not np.signbit(t[0]) and t[0] == 0 and np.signbit(t[1]) and t[1] == 0 and t[2] < 0
    groups = {5: [0, 1, 0, 1], 6: [1, 2], 7: [1], 8: [0, 2], 9: [1, 1, 0]}
    recs = np.array([k | (f << 12) for k, fs in groups.items() for f in fs], dtype=np.uint64)
    parts = [recs[::-1].copy(), np.zeros(0, np.uint64), recs]
    ref = R.groupby_ref(parts, 12, vals["value_of"])
    assert [str(x) for x in ref[(0, 5)][2:4]] == ["-0.0", "0.0"] and str(ref[(0, 6)][3]) == "-0.0"
    res = _run_agg(nk, parts, W=W, cap2=16, rb2=12, K=20, vals=vals, mask=7, kind=kind, prange=False)
    _check_agg(res, ref, 12, 20, 7, f64=True)


def _chain(nk, kind, K, rb1, k2, nwg, valbits, seed):
    """m: rows (key, value field) -> first-stage records (bucket = the mix's top bits) -> split -> aggregate."""
    rng = np.random.default_rng(seed)
    W = KINDS[kind][1] + 1
    rb2 = rb1 - k2
    nb = 1 << (K - rb1)
    vals = _values(kind, rng, rb2, W)
    keys = np.unique(rng.integers(0, 1 << K, 3000))
    keys = keys[rng.integers(0, len(keys), 20000)]
    field = rng.integers(0, min(vals["card"], 1 << valbits), len(keys), dtype=np.uint64)
    h = np.array([R.mix(int(k), K) for k in keys], dtype=np.uint64)
    x = (h & np.uint64((1 << rb1) - 1)) | (field << np.uint64(rb1))
    bucket, slab = (h >> np.uint64(rb1)).astype(np.int64), rng.integers(0, nwg, len(keys))
    slabs = [[x[(bucket == b) & (slab == w)] for w in range(nwg)] for b in range(nb)]
    cap1 = max(len(s) for bk in slabs for s in bk) + 3
    per = np.bincount((h >> np.uint64(rb2)).astype(np.int64), minlength=nb << k2)
    inp = dict(W=W, nwg=nwg, cap1=cap1, rb1=rb1, k2=k2, hi=rb1 + valbits > 32, cap2=(int(per.max()) + 63) // 32 * 32,
               slabs=slabs, claim=[[len(s) for s in bk] for bk in slabs])
    B = _split_buffers(nk, inp)
    assert _launch_split(nk, inp, B) == 0
    nparts, cap2 = nb << k2, inp["cap2"]
    cnt2 = nk.down(B["cnt2"], np.uint32)[:nparts]
    assert (cnt2 == per).all() and int(nk.down(B["ovf"], np.uint64)[0]) == 0
    recs = nk.down(B["out"], np.uint32)[:nparts * cap2 * W].view(np.uint32 if W == 1 else np.uint64)
    recs = recs.reshape(nparts, cap2)
    parts = [recs[p, :cnt2[p]].astype(np.uint64) for p in range(nparts)]  # the split's own output, re-uploaded
    res = _run_agg(nk, parts, W=W, cap2=cap2, rb2=rb2, K=K, vals=vals, mask=7, kind=kind, grid=2)
    rows = {}
    for k, f in zip(keys.tolist(), field.tolist()):
        rows.setdefault(k, []).append(vals["value_of"](f))
    assert res["rc"] == 0 and res["n"] == len(rows) and res["lost"] == 0 and res["clean"]
    got = {int(k): [int(res["plane"][p, i]) for p in range(4)] for i, k in enumerate(res["key"][:res["n"]])}
    exp = {k: [len(v), sum(v) & M64, R.ordered_i64(min(v)), R.ordered_i64(max(v))] for k, v in rows.items()}
    assert got == exp


def test_split_then_aggregate_image_records(nk):
    """m: W = 1, FOR16 image: 22-bit keys, 4 buckets x 16 sub-buckets, 10-bit dictIds."""
    _chain(nk, "2", K=22, rb1=20, k2=4, nwg=3, valbits=10, seed=5)


def test_split_then_aggregate_wide_direct_records(nk):
    """m: W = 2, value offsets of 32 bits in 48-bit first-stage records: 18-bit keys, 4 buckets x 16 sub-buckets."""
    _chain(nk, "3w", K=18, rb1=16, k2=4, nwg=3, valbits=32, seed=6)


def test_aggregate_argument_checks(nk):
    """n: every refusal of pgx_launch_narrow_aggregate returns hipErrorInvalidValue and writes nothing."""
    def refused(kind, mask, **over):
        D = _dataset(kind)
        res = _run_dataset(nk, kind, D, mask, 1, over=over)
        assert res["rc"] == R.INVALID_VALUE, (kind, over)
        assert res["n"] == 0 and res["lost"] == 0 and res["clean"], (kind, over)
        assert (res["key"] == S64).all() and (res["plane"] == S64).all(), (kind, over)
        assert [int(x) for x in res["prange"]] == [M64] * 4 + [0] * 4, (kind, over)

    for over in (dict(rb2=-1), dict(rb2=32), dict(K=0), dict(K=65), dict(cap2=0), dict(cap2=6), dict(cshift=0),
                 dict(cshift=64), dict(grid=0), dict(inp=None), dict(cnt2=None), dict(okey=None), dict(oplane=None),
                 dict(ctr=None), dict(ik=-1), dict(ik=7), dict(scratch=None), dict(sw=1)):
        refused("3", 7, **over)
    for kind, words in (("1", R.IMG_WORDS), ("2", R.IMG_WORDS), ("4", R.IMG4_WORDS)):
        for over in (dict(img=None), dict(img_words=0), dict(img_words=words + 1)):
            refused(kind, 7, **over)
    for kind in ("5", "6"):
        for over in (dict(img=None), dict(img_words=0)):
            refused(kind, 7, **over)
    refused("0", 4)                    # SUM without an image
    refused("0", 2, vdict=None)        # MIN / MAX over dictIds without the dictionary
    refused("0", 1, vdict=None)
    for kind in ("1", "2", "4"):
        refused(kind, 7, wide=1)       # 64-bit records: direct and gathered kinds only
    refused("0", 3, wide=1)
    D = _dataset("6")                  # doubles have no trim-key ranges
    res = _run_agg(nk, D["parts"], W=1, cap2=D["cap2"], rb2=D["rb2"], K=D["K"], vals=D["vals"], mask=7, kind="6",
                   prange=True)
    assert res["rc"] == R.INVALID_VALUE and res["n"] == 0 and res["clean"] and (res["key"] == S64).all()
