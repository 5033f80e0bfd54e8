"""Direct tests of the combine-stage kernels (pinot_amd/csrc/pgx_trim.hip: the radix select behind pgx_result_trim and
the gather of the kept groups; pgx_merge.hip: group merge, compaction, the several-column join, the record pack, the
key gather and the dense reduce), launched through libpgx.so's launchers on torch device buffers and compared with the
plain numpy / Python-int model of tests/combine_ref.py at small shapes chosen for the kernels' branches.

Every output buffer is pre-filled with a sentinel and has guard words past its end; every test asserts that whatever
it did not expect to be written still holds the sentinel.  Which threshold ties a trim keeps and the order of its
output are arbitrary, so multisets and sets are compared; everything is exact but one f64 sum with a derived bound."""
import ctypes as C
import fractions
import math

import numpy as np
import pytest

from tests import combine_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
S64 = 0x5A5A5A5A5A5A5A5A
M64 = R.M64


class _CK:
    def __init__(self):
        import torch
        from pinot_amd import native as N
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.K = R.bind(N.lib())
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        """numpy array of an unsigned type -> device tensor of the signed type of the same width."""
        a = np.ascontiguousarray(a)
        signed = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
        return self.torch.from_numpy(a.view(signed).copy()).to(self.dev)

    def out(self, words, fill=S64):
        """An output buffer of `words` u64 and GUARD more, all holding the sentinel."""
        return self.up(np.full(words + GUARD, fill, dtype=np.uint64))

    def words(self, a):
        """Host words (any shape) -> device buffer followed by GUARD sentinel words."""
        return self.up(np.concatenate([np.asarray(a, dtype=np.uint64).reshape(-1), np.full(GUARD, S64, np.uint64)]))

    def down(self, t, dtype=np.uint64):
        self.torch.cuda.synchronize(self.dev)
        return t.cpu().numpy().view(dtype)


@pytest.fixture(scope="module")
def ck():
    return _CK()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _clean(a, start=0):
    return bool((a[start:] == np.uint64(S64)).all())


# =====================================================================================================================
# trim
# =====================================================================================================================
def _trim_buffers(ck, case):
    nf, cap, ccap = len(case["kinds"]), case["cap"], case["ccap"]
    st0 = np.concatenate([R.state_init(nf, case["k"]), np.full(GUARD * 8, 0x5A, dtype=np.uint8)])
    return dict(oplane=ck.up(case["oplane"].reshape(-1)), st0=st0, states=ck.up(st0), idx=ck.out(nf * cap),
                keys=ck.out(nf * cap), cidx=ck.out(nf * ccap), ckey=ck.out(nf * ccap),
                prange=None if case["prange"] is None else ck.up(case["prange"]))


def _launch_trim(ck, case, B, **over):
    a = dict(oplane=_ptr(B["oplane"]), nf=len(case["kinds"]), states=_ptr(B["states"]), idx=_ptr(B["idx"]),
             keys=_ptr(B["keys"]), cidx=_ptr(B["cidx"]), ckey=_ptr(B["ckey"]), ccap=case["ccap"],
             prange=_ptr(B["prange"]))
    a.update(over)
    kinds = (C.c_int * 16)(*case["kinds"])
    planes = (C.c_int * 16)(*case["planes"])
    return ck.K.trim(a["oplane"], case["ocap"], case["n"], kinds, planes, a["nf"], a["states"], a["idx"], a["keys"],
                     case["cap"], case["grid"], a["prange"], a["cidx"], a["ckey"], a["ccap"], ck.stream)


def _trim_untouched(ck, B):
    return (_clean(ck.down(B["idx"])) and _clean(ck.down(B["keys"])) and _clean(ck.down(B["cidx"]))
            and _clean(ck.down(B["ckey"])) and (ck.down(B["states"], np.uint8) == B["st0"]).all())


def _run_trim(ck, case):
    """Launch the trim on `case` and check every function slot in full against the model.  Returns, per function,
    whether the later passes and the select read the candidate list (decided from the state's n_cand and ccap)."""
    B = _trim_buffers(ck, case)
    assert _launch_trim(ck, case, B) == 0
    n, k, cap, ccap, nf = case["n"], case["k"], case["cap"], case["ccap"], len(case["kinds"])
    idx, keys = ck.down(B["idx"], np.int64), ck.down(B["keys"])
    cidx, ckey = ck.down(B["cidx"], np.int64), ck.down(B["ckey"])
    states = ck.down(B["states"], np.uint8)
    assert (ck.down(B["oplane"]) == case["oplane"].reshape(-1)).all(), "the planes were written"
    assert _clean(idx.view(np.uint64), nf * cap) and _clean(keys, nf * cap), "written past the selection strips"
    assert _clean(cidx.view(np.uint64), nf * ccap) and _clean(ckey, nf * ccap), "written past the candidate lists"
    assert (states[nf * R.STATE_BYTES:] == 0x5A).all(), "written past the state blocks"
    used = []
    for f in range(nf):
        st, ref, fkeys = R.state_read(states, f), R.case_ref(case, f), R.case_keys(case, f)
        print("fn %d kind %d: n_sel %d n_tie %d n_cand %d k %d prefix %#x (model: n_eq %d ties %d n_cand %s hb %d)" % (
            f, case["kinds"][f], st["n_sel"], st["n_tie"], st["n_cand"], st["k"], st["prefix"], ref.n_eq, ref.ties,
            ref.n_cand, ref.hb))
        nsel = min(k, n)
        assert st["n_sel"] == nsel
        ix, ky = idx[f * cap:f * cap + nsel], keys[f * cap:f * cap + nsel]
        assert ((ix >= 0) & (ix < n)).all() and len(np.unique(ix)) == nsel, "kept indices not distinct groups"
        assert (ky == fkeys[ix]).all(), "a kept group does not carry its own key"
        assert (np.sort(ky) == ref.kept).all(), "kept keys differ from the model's multiset"
        thr = 0 if ref.thr is None else ref.thr
        top = ix[ky > np.uint64(thr)] if ref.thr is not None else ix
        assert (np.sort(top) == ref.above).all(), "the groups above the threshold are not exactly the model's"
        assert _clean(idx.view(np.uint64)[f * cap + nsel:(f + 1) * cap]) and _clean(keys[f * cap + nsel:(f + 1) * cap])
        # the state block
        assert st["done"] == 1 and st["shift"] == 0 and st["mask"] == M64 and not st["hist"].any()
        if R.case_seeded(case):
            kind = case["kinds"][f]
            assert (st["kmin"], st["kmax"]) == (int(case["prange"][kind]), int(case["prange"][4 + kind]))
        else:
            assert (st["kmin"], st["kmax"]) == ((int(fkeys.min()), int(fkeys.max())) if n else (M64, 0))
        if n >= k:
            assert st["prefix"] == ref.thr and st["k"] == ref.ties and st["n_tie"] == ref.n_eq
            if ccap > 0:
                assert st["n_cand"] == ref.n_cand
        if ccap == 0:
            assert st["n_cand"] == 0
        if ref.hb <= R.DIGIT:
            assert st["n_cand"] == 0  # the threshold was complete (done) after one digit: the candidate kernel returned
        # the candidate list: complete when it fits, never past min(n_cand, ccap)
        wrote = min(st["n_cand"], ccap)
        ci, cy = cidx[f * ccap:f * ccap + wrote], ckey[f * ccap:f * ccap + wrote]
        rest = slice(f * ccap + wrote, (f + 1) * ccap)
        assert _clean(cidx.view(np.uint64)[rest]) and _clean(ckey[rest])
        use = 0 < st["n_cand"] <= ccap
        if use:
            assert ((ci >= 0) & (ci < n)).all() and (cy == fkeys[ci]).all()
            if n >= k:
                first = ref.thr >> (ref.hb - R.DIGIT) << (ref.hb - R.DIGIT)
                assert (np.sort(ci) == np.flatnonzero(fkeys >= np.uint64(first))).all()
        used.append(use)
    return used


_HB = ["hb_%d" % hb for hb in R.HBS] + ["sum_signed"]


@pytest.mark.parametrize("name", _HB)
def test_trim_key_width(ck, name):
    """The digit schedule's edges: keys varying in exactly hb bits (one digit that overlaps the fixed bits at
    hb <= 11; a last digit that overlaps the one before wherever hb is no multiple of 11; mask = 0 at hb = 64, which
    SUM keys of both signs reach too).  The candidate list is used exactly when more than one digit is needed."""
    case = R.trim_case(name)
    assert _run_trim(ck, case) == [case["premise"]["hb"] > R.DIGIT]


@pytest.mark.parametrize("kind", range(7))
def test_trim_kinds(ck, kind):
    """Every TrimKind once, its value in a plane of the second value column (1 + 3c + r): AVG with counts 0, negative
    sums and sums above 2^53; SUMF / AVGF with signed zeros, negative and subnormal values."""
    _run_trim(ck, R.trim_case("kind_%d" % kind))


@pytest.mark.parametrize("name", ["all_equal", "two_keys_upper", "two_keys_lower"])
def test_trim_ties(ck, name):
    """Every key equal (the threshold is known before any digit: done in pgx_trim_begin); two distinct keys with k
    inside the upper and inside the lower one."""
    assert _run_trim(ck, R.trim_case(name)) == [False]


@pytest.mark.parametrize("v", ["g1", "g1w", "g1c", "g3", "g3w", "g3s"])
def test_trim_ties_beyond_the_lds_list(ck, v):
    """More than kTieCap = 2048 threshold ties in one workgroup's range (asserted on the CPU by
    tests/test_combine_ref.py): the ties past the LDS list are reserved per wave on n_tie, which the workgroups' own
    end-of-range reservations share.  g1: grid 1, n = 6000, 5000 ties, 2500 wanted (the per-wave reservations fill
    the quota and refuse 452; the LDS list is refused whole); g1w: 3500 wanted (all 2952 per-wave ties are taken, the
    LDS list keeps 548 and refuses 1500); g1c: g1 scanning the candidate list; g3 / g3w: grid 3, n = 18000, the ties
    in the middle range; g3s: ties in all three ranges, one overflowing.  n_tie == n_eq proves every tie was counted
    once, n_sel == k that exactly the wanted number was kept."""
    case = R.trim_case("tiecap_" + v)
    assert _run_trim(ck, case) == [v == "g1c"]


@pytest.mark.parametrize("v", ["none", "all", "exact", "short", "flush"])
@pytest.mark.parametrize("w", [22, 64])
def test_trim_candidate_list(ck, w, v):
    """The candidate list with keys needing two passes (w = 22) and six (w = 64): no list (ccap = 0), room for every
    group, exactly the candidate count, one below it (the list is abandoned partly written: n_cand > ccap, and the
    later passes and the select re-read the planes), and one workgroup with more than 1792 candidates (the LDS list
    is flushed before its range ends)."""
    case = R.trim_case("cand_w%d_%s" % (w, v))
    assert _run_trim(ck, case) == [v in ("all", "exact", "flush")]


@pytest.mark.parametrize("n,k,grid", R.COUNT_CASES)
def test_trim_counts(ck, n, k, grid):
    """n around the workgroup size, k in {1, n - 1, n} and above n (every group is kept: no threshold), one
    workgroup and more workgroups than there are groups for."""
    _run_trim(ck, R.trim_case("cnt_n%d_k%d_g%d" % (n, k, grid)))


@pytest.mark.parametrize("name", ["nf8", "nf1"])
def test_trim_functions_side_by_side(ck, name):
    """Eight functions of mixed kinds over three value columns in one launch, and one alone; cap (the strip stride)
    larger than k."""
    _run_trim(ck, R.trim_case(name))


@pytest.mark.parametrize("v", ["exact", "loose", "poison", "null"])
def test_trim_seeded_ranges(ck, v):
    """prange exact, a loose bracket (a wider first digit, the same selection), ignored because one function is an
    AVG (filled with ranges that would end the select at a wrong threshold), and null."""
    _run_trim(ck, R.trim_case("seed_" + v))


def test_trim_argument_checks(ck):
    """Refused launches return hipErrorInvalidValue and run no kernel: every buffer keeps its contents."""
    case = R.trim_case("nf1")
    B = _trim_buffers(ck, case)
    for over in (dict(nf=0), dict(nf=9), dict(nf=-1), dict(cidx=None), dict(ckey=None), dict(cidx=None, ckey=None),
                 dict(ccap=-1)):
        assert _launch_trim(ck, case, B, **over) == R.INVALID_VALUE, over
    assert _trim_untouched(ck, B)


# =====================================================================================================================
# gather
# =====================================================================================================================
@pytest.mark.parametrize("nplanes", [1, 4, 25])
@pytest.mark.parametrize("m", [1, 255, 257])
def test_group_gather(ck, m, nplanes):
    rng = np.random.default_rng(m * 100 + nplanes)
    ocap = 300
    okey = rng.integers(0, 1 << 64, size=ocap, dtype=np.uint64)
    opl = rng.integers(0, 1 << 64, size=(nplanes, ocap), dtype=np.uint64)
    for idx in (rng.integers(0, ocap, size=m), np.arange(ocap - 1, ocap - 1 - m, -1)):  # repeats; reverse order
        out = ck.out((1 + nplanes) * m)
        assert ck.K.gather(_ptr(ck.up(okey)), _ptr(ck.up(opl.reshape(-1))), ocap, nplanes,
                           _ptr(ck.up(idx.astype(np.int64).view(np.uint64))), m, _ptr(out), ck.stream) == 0
        got = ck.down(out)
        assert _clean(got, (1 + nplanes) * m)
        assert (got[:m] == okey[idx]).all() and (got[m:(1 + nplanes) * m].reshape(nplanes, m) == opl[:, idx]).all()


def test_group_gather_argument_checks(ck):
    okey, opl, idx, out = ck.up(np.zeros(8, np.uint64)), ck.up(np.zeros(26 * 8, np.uint64)), ck.up(
        np.zeros(8, np.uint64)), ck.out(27 * 8)
    assert ck.K.gather(_ptr(okey), _ptr(opl), 8, 4, _ptr(idx), 0, _ptr(out), ck.stream) == 0  # m = 0: nothing to do
    assert ck.K.gather(_ptr(okey), _ptr(opl), 8, 26, _ptr(idx), 8, _ptr(out), ck.stream) == R.INVALID_VALUE
    assert ck.K.gather(_ptr(okey), _ptr(opl), 8, 0, _ptr(idx), 8, _ptr(out), ck.stream) == R.INVALID_VALUE
    assert _clean(ck.down(out))


# =====================================================================================================================
# merge and compact
# =====================================================================================================================
def _ops(nplanes):
    """All four ops (at 4 and 32 planes; plane 31's op sits in the top two of the 64 ops bits)."""
    return [R.OP_ADD] if nplanes == 1 else [[R.OP_ADD, R.OP_ADDF, R.OP_MIN, R.OP_MAX][p % 4] for p in range(nplanes)]


def _planes(rng, n, ops, fmax):
    """Inputs of n groups: integer planes of random 64-bit words (sums wrap; min / max see both sides of the ordered
    encoding's sign bit), f64 planes of integer-valued doubles below fmax in magnitude."""
    pl = rng.integers(0, 1 << 64, size=(len(ops), n), dtype=np.uint64)
    for p, op in enumerate(ops):
        if op == R.OP_ADDF:
            pl[p] = rng.integers(-fmax + 1, fmax, size=n).astype(np.float64).view(np.uint64)
    return pl


def _merge(ck, keys, planes, ops, cap, layout):
    """Merge the inputs into a table (a fresh one as merge_device_groups initialises it); returns the table's key
    and plane arrays and the overflow count."""
    n, npl = len(keys), len(ops)
    keys = np.asarray(keys, dtype=np.uint64)
    tkey0, tpl0 = R.table_init(cap, ops)
    tkey, tpl, ovf = ck.words(tkey0), ck.words(tpl0), ck.up(np.array([0, S64], dtype=np.uint64))
    if layout == "columnar":
        kd, pd = ck.up(keys), ck.up(planes.reshape(-1))
        rc = ck.K.merge(_ptr(kd), _ptr(pd), 1, n, n, _ptr(tkey), _ptr(tpl), cap, npl, R.ops_pack(ops), _ptr(ovf),
                        ck.stream)
    else:
        rec = ck.up(R.pack_ref(keys, planes, n).reshape(-1))
        rc = ck.K.merge(_ptr(rec), _ptr(rec) + 8, 1 + npl, 1, n, _ptr(tkey), _ptr(tpl), cap, npl, R.ops_pack(ops),
                        _ptr(ovf), ck.stream)
    assert rc == 0
    tk, tp, ov = ck.down(tkey), ck.down(tpl), ck.down(ovf)
    assert _clean(tk, cap) and _clean(tp, npl * cap) and int(ov[1]) == S64
    return tk[:cap].copy(), tp[:npl * cap].reshape(npl, cap).copy(), int(ov[0])


def _table_dict(tk, tp):
    live = np.flatnonzero(tk != np.uint64(R.EMPTY))
    d = {int(tk[s]): [int(x) for x in tp[:, s]] for s in live}
    assert len(d) == len(live), "a key sits in two slots"
    return d


def _compact(ck, tk, tp, ocap):
    """Compact a table (host arrays) into okey / opl of ocap groups; checks the counter and that nothing is written
    past min(live, ocap); returns key -> planes of what was written."""
    npl, cap = tp.shape
    okey, opl, cnt = ck.out(ocap), ck.out(npl * ocap), ck.up(np.array([0, S64], dtype=np.uint64))
    assert ck.K.compact(_ptr(ck.up(tk)), _ptr(ck.up(tp.reshape(-1))), cap, npl, _ptr(okey), _ptr(opl), ocap, _ptr(cnt),
                        ck.stream) == 0
    ok, op, c = ck.down(okey), ck.down(opl), ck.down(cnt)
    live = int((tk != np.uint64(R.EMPTY)).sum())
    assert int(c[0]) == live and int(c[1]) == S64
    m = min(live, ocap)
    assert _clean(ok, m) and _clean(op, npl * ocap)
    op = op[:npl * ocap].reshape(npl, ocap)
    assert _clean(op[:, m:].reshape(-1))
    d = {int(ok[j]): [int(x) for x in op[:, j]] for j in range(m)}
    assert len(d) == m, "a key was written twice"
    return d


def _merge_shape(shape, rng):
    """(keys, cap, bound on the magnitude of an f64 plane's integer-valued inputs).  With at most A addends per key
    below 2^53 / A in magnitude every partial sum, in any order, is an integer below 2^53: exact."""
    if shape == "full":  # as many distinct keys as slots
        keys = rng.integers(0, 1 << 63, size=1024, dtype=np.uint64)
        assert len(np.unique(keys)) == 1024
        return keys, 1024, 1 << 40
    if shape == "wrap":  # 64 keys homed on the last slot: all but one probe past the table's end
        keys = R.keys_homed_at(256, 255, 64) + R.keys_homed_at(256, 0, 8) + R.keys_homed_at(256, 100, 8)
        return rng.permutation(np.array(keys * 3, dtype=np.uint64)), 256, 1 << 40
    if shape == "hot":  # one key 10000 times beside 1000 singletons: 10000 x 2^39 < 2^53
        keys = np.concatenate([np.full(10000, 77, dtype=np.uint64), np.arange(1000, 2000, dtype=np.uint64)])
        return rng.permutation(keys), 4096, 1 << 39
    assert shape == "edge"  # the smallest and largest packed keys
    return rng.permutation(np.array([0, (1 << 63) - 1, 1, (1 << 63) - 2] * 50, dtype=np.uint64)), 64, 1 << 40


@pytest.mark.parametrize("nplanes", [1, 4, 32])
@pytest.mark.parametrize("shape", ["full", "wrap", "hot", "edge"])
def test_group_merge_and_compact(ck, shape, nplanes):
    """Columnar and record inputs give the model's table, slot for key; the compacted groups are the table's, the
    counter the number of distinct keys.  Integer planes exactly (sums mod 2^64), f64 planes bit for bit (exact
    integer-valued inputs, see _merge_shape)."""
    rng = np.random.default_rng(nplanes)
    keys, cap, fmax = _merge_shape(shape, rng)
    if shape == "wrap":
        assert sum(1 for k in set(keys.tolist()) if R.home_slot(k, cap) == cap - 1) == 64
    ops = _ops(nplanes)
    planes = _planes(rng, len(keys), ops, fmax)
    ref, _ = R.group_merge_ref(keys, planes, ops)
    for layout in ("columnar", "records"):
        tk, tp, ovf = _merge(ck, keys, planes, ops, cap, layout)
        assert ovf == 0
        assert _table_dict(tk, tp) == ref, layout
        if shape == "full":
            assert (tk != np.uint64(R.EMPTY)).all()
        assert _compact(ck, tk, tp, cap) == ref, layout


def test_group_merge_general_doubles(ck):
    """f64 sums of general doubles: against the exact sum (and math.fsum, its correct rounding) under
    (addends - 1) * 2^-53 * sum |v|, the worst case of recursive summation in any order (Rump 2012: the bound holds
    without higher-order terms).  The table's 0.0 + first addend is exact, so the inputs are the addends."""
    rng = np.random.default_rng(9)
    n = 4000
    keys = rng.integers(0, 200, size=n, dtype=np.uint64)
    v = rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, size=n).astype(np.float64))
    ops = [R.OP_ADDF]
    ref, aux = R.group_merge_ref(keys, v.view(np.uint64)[None, :], ops)
    tk, tp, ovf = _merge(ck, keys, np.ascontiguousarray(v).view(np.uint64)[None, :], ops, 512, "columnar")
    got = _table_dict(tk, tp)
    assert ovf == 0 and set(got) == set(ref)
    worst = 0.0
    F = fractions.Fraction
    for k, row in got.items():
        dev = float(np.uint64(row[0]).view(np.float64))
        mine = v[keys == np.uint64(k)]
        exact, sabs = sum(F(float(x)) for x in mine), sum(F(abs(float(x))) for x in mine)
        bound = (len(mine) - 1) * F(1, 1 << 53) * sabs
        fs = float(np.uint64(ref[k][0]).view(np.float64))
        assert fs == math.fsum(mine.tolist()) and aux[k][0][1] == len(mine)
        assert abs(F(dev) - exact) <= bound, (k, dev, fs)
        assert abs(F(dev) - F(fs)) <= bound, (k, dev, fs)
        if bound:
            worst = max(worst, float(abs(F(dev) - exact) / bound))
    print("largest error / bound: %.3g" % worst)


def test_group_merge_overflow(ck):
    """cap = 1024 and 1536 distinct keys given 3 times each: exactly the inputs of the 512 keys that found no slot
    count as overflow, and every key in the table carries all 3 of its inputs."""
    rng = np.random.default_rng(11)
    base = np.arange(1, 1537, dtype=np.uint64) * np.uint64(1000003)
    keys = rng.permutation(np.repeat(base, 3))
    ops = _ops(4)
    planes = _planes(rng, len(keys), ops, 1 << 40)
    ref, _ = R.group_merge_ref(keys, planes, ops)
    for layout in ("columnar", "records"):
        tk, tp, ovf = _merge(ck, keys, planes, ops, 1024, layout)
        got = _table_dict(tk, tp)
        assert ovf == 3 * 512 and len(got) == 1024
        assert all(ref[k] == row for k, row in got.items())


def _table(rng, cap, live, npl=3):
    tk = np.full(cap, R.EMPTY, dtype=np.uint64)
    at = {"none": [], "one": [cap - 1], "some": np.flatnonzero(rng.random(cap) < 0.4), "all": np.arange(cap)}[live]
    tk[at] = rng.permutation(np.arange(1, 1 + cap, dtype=np.uint64))[:len(at)]
    return tk, rng.integers(0, 1 << 64, size=(npl, cap), dtype=np.uint64)


@pytest.mark.parametrize("live", ["none", "one", "some", "all"])
@pytest.mark.parametrize("cap", [256, 4096, 8192])
def test_group_compact_alone(ck, cap, live):
    """Tables below, at and above the 4096-slot tile (two workgroups at 8192); empty, one live slot (the last), some
    and all."""
    tk, tp = _table(np.random.default_rng(cap), cap, live)
    assert _compact(ck, tk, tp, cap) == _table_dict(tk, tp)


@pytest.mark.parametrize("ocap", [1, 5000])
def test_group_compact_ocap_below_live(ck, ocap):
    """The counter still counts every live slot; nothing is written past ocap, and what is written are groups of the
    table (checked in _compact)."""
    tk, tp = _table(np.random.default_rng(3), 8192, "all")
    got, ref = _compact(ck, tk, tp, ocap), _table_dict(tk, tp)
    assert len(got) == ocap and all(ref[k] == row for k, row in got.items())


def test_merge_launcher_argument_checks(ck):
    rng = np.random.default_rng(4)
    ops = _ops(4)
    keys, planes = np.arange(1, 9, dtype=np.uint64), _planes(rng, 8, ops, 1 << 20)
    tkey0, tpl0 = R.table_init(64, ops)
    T = (ck.words(tkey0), ck.words(np.concatenate([tpl0.reshape(-1), np.zeros(29 * 64, np.uint64)])),
         ck.up(np.array([0, S64], dtype=np.uint64)))
    kd, pd = ck.up(keys), ck.up(np.concatenate([planes.reshape(-1), np.zeros(29 * 8, np.uint64)]))
    okey, opl, cnt = ck.out(64), ck.out(33 * 64), ck.up(np.array([0, S64], dtype=np.uint64))
    rec = ck.out(34 * 8)

    def merge(n=8, cap=64, npl=4):
        return ck.K.merge(_ptr(kd), _ptr(pd), 1, 8, n, _ptr(T[0]), _ptr(T[1]), cap, npl, R.ops_pack(ops), _ptr(T[2]),
                          ck.stream)

    for bad in (dict(cap=48), dict(cap=0), dict(cap=63), dict(npl=33), dict(npl=0)):
        assert merge(**bad) == R.INVALID_VALUE, bad
    assert merge(n=0) == 0 and merge(n=0, cap=48) == 0  # nothing to do
    for npl in (0, 33):
        assert ck.K.compact(_ptr(T[0]), _ptr(T[1]), 64, npl, _ptr(okey), _ptr(opl), 64, _ptr(cnt),
                            ck.stream) == R.INVALID_VALUE
        assert ck.K.pack(_ptr(kd), _ptr(pd), 8, 8, npl, _ptr(rec), ck.stream) == R.INVALID_VALUE
    assert ck.K.compact(_ptr(T[0]), _ptr(T[1]), 0, 4, _ptr(okey), _ptr(opl), 64, _ptr(cnt), ck.stream) == 0
    assert ck.K.pack(_ptr(kd), _ptr(pd), 8, 0, 4, _ptr(rec), ck.stream) == 0
    assert (ck.down(T[0])[:64] == tkey0).all() and (ck.down(T[1])[:4 * 64] == tpl0.reshape(-1)).all()
    assert int(ck.down(T[2])[0]) == 0 and int(ck.down(cnt)[0]) == 0
    assert _clean(ck.down(okey)) and _clean(ck.down(opl)) and _clean(ck.down(rec))


# =====================================================================================================================
# join
# =====================================================================================================================
JOIN_CAP = 2048


def _join_keys(which, rng):
    if which == "wrap":  # a cluster homed on the last slot beside random keys
        return np.array(R.keys_homed_at(JOIN_CAP, JOIN_CAP - 1, 64) + list(range(1 << 40, (1 << 40) + 100)), np.uint64)
    n0 = {"1": 1, "1000": 1000, "half": JOIN_CAP // 2}[which]
    keys = rng.integers(0, 1 << 63, size=n0, dtype=np.uint64)
    assert len(np.unique(keys)) == n0
    return keys


@pytest.mark.parametrize("base", [1, 4, 22])
@pytest.mark.parametrize("which", ["1", "1000", "half", "wrap"])
def test_join_build_and_scatter(ck, which, base):
    """Build the table from the first pass's keys, scatter a permuted later pass: its sum / min / max planes land at
    the first pass's indices in planes base .. base + 2 of the combined planes and nowhere else; miss stays 0.  A pass
    with 7 keys the table does not hold counts 7 misses and writes nothing for them."""
    rng = np.random.default_rng(base)
    keys0 = _join_keys(which, rng)
    n0, cap = len(keys0), JOIN_CAP
    tkey, tidx = ck.words(np.full(cap, R.EMPTY, dtype=np.uint64)), ck.out(cap)
    assert ck.K.join(_ptr(ck.up(keys0)), n0, None, None, 0, 0, _ptr(tkey), _ptr(tidx), cap, None, 0, 0, None,
                     ck.stream) == 0
    tk, ti = ck.down(tkey), ck.down(tidx, np.int64)
    assert _clean(tk, cap) and _clean(ti.view(np.uint64), cap)
    live = np.flatnonzero(tk[:cap] != np.uint64(R.EMPTY))
    assert len(live) == n0 and (keys0[ti[live]] == tk[live]).all() and len(np.unique(ti[live])) == n0
    assert _clean(ti.view(np.uint64)[:cap][tk[:cap] == np.uint64(R.EMPTY)])
    if which == "wrap":
        assert sum(1 for s in live if R.home_slot(int(tk[s]), cap) == cap - 1 and s < cap - 1) == 63  # wrapped

    ccap, ocap, nplanes = n0 + 3, n0 + 5, 25
    comb = ck.out(nplanes * ccap)
    expect = np.full((nplanes, ccap), S64, dtype=np.uint64)
    miss = ck.up(np.array([0, S64], dtype=np.uint64))
    absent = np.arange(7, dtype=np.uint64) + np.uint64(1 << 50)
    misses = 0
    for later in (rng.permutation(keys0), rng.permutation(np.concatenate([keys0, absent]))):
        n = len(later)
        opl = rng.integers(0, 1 << 64, size=(4, n + 2), dtype=np.uint64)
        assert ck.K.join(None, 0, _ptr(ck.up(later)), _ptr(ck.up(opl.reshape(-1))), n + 2, n, _ptr(tkey), _ptr(tidx),
                         cap, _ptr(comb), ccap, base, _ptr(miss), ck.stream) == 0
        expect, m = R.join_ref(keys0, later, opl, expect, base)
        misses += m
        got, ms = ck.down(comb), ck.down(miss)
        assert _clean(got, nplanes * ccap) and (got[:nplanes * ccap].reshape(nplanes, ccap) == expect).all()
        assert int(ms[0]) == misses and int(ms[1]) == S64
    assert misses == 7 and _clean(expect[:base].reshape(-1)) and _clean(expect[base + 3:].reshape(-1))
    assert (ck.down(tkey) == tk).all() and (ck.down(tidx, np.int64) == ti).all()


def test_join_argument_checks(ck):
    keys = ck.up(np.arange(1, 9, dtype=np.uint64))
    opl, comb, miss = ck.up(np.zeros(4 * 8, np.uint64)), ck.out(8 * 8), ck.up(np.array([0, S64], dtype=np.uint64))
    tkey, tidx = ck.words(np.full(16, R.EMPTY, dtype=np.uint64)), ck.out(16)

    def scatter(tk=tkey, ti=tidx, cap=16, base=1, n=8):
        return ck.K.join(None, 0, _ptr(keys), _ptr(opl), 8, n, _ptr(tk), _ptr(ti), cap, _ptr(comb), 8, base,
                         _ptr(miss), ck.stream)

    for bad in (dict(base=0), dict(base=-1), dict(tk=None), dict(ti=None), dict(cap=12), dict(cap=0)):
        assert scatter(**bad) == R.INVALID_VALUE, bad
    assert ck.K.join(_ptr(keys), 8, None, None, 0, 0, None, _ptr(tidx), 16, None, 0, 0, None,
                     ck.stream) == R.INVALID_VALUE  # a build with a null tkey
    assert scatter(n=0) == 0
    assert ck.K.join(_ptr(keys), 0, None, None, 0, 0, _ptr(tkey), _ptr(tidx), 16, None, 0, 0, None, ck.stream) == 0
    assert _clean(ck.down(comb)) and _clean(ck.down(tidx)) and (ck.down(tkey)[:16] == np.uint64(R.EMPTY)).all()
    assert int(ck.down(miss)[0]) == 0


# =====================================================================================================================
# pack, gather_keys, dense_reduce
# =====================================================================================================================
@pytest.mark.parametrize("nplanes", [1, 25])
@pytest.mark.parametrize("n", [1, 257])
def test_group_pack(ck, n, nplanes):
    rng = np.random.default_rng(n + nplanes)
    ocap = n + 5
    okey = rng.integers(0, 1 << 64, size=ocap, dtype=np.uint64)
    opl = rng.integers(0, 1 << 64, size=(nplanes, ocap), dtype=np.uint64)
    rec = ck.out((1 + nplanes) * n)
    assert ck.K.pack(_ptr(ck.up(okey)), _ptr(ck.up(opl.reshape(-1))), ocap, n, nplanes, _ptr(rec), ck.stream) == 0
    got = ck.down(rec)
    assert _clean(got, (1 + nplanes) * n)
    assert (got[:(1 + nplanes) * n].reshape(n, 1 + nplanes) == R.pack_ref(okey, opl, n)).all()


@pytest.mark.parametrize("ndev", [None, 100, 257, 400])
@pytest.mark.parametrize("kw", [1, 2, 3, 4])
def test_gather_keys(ck, kw, ndev):
    """min(*n_dev, n) keys of kw words are gathered (n when n_dev is null); the rest of out is untouched."""
    rng = np.random.default_rng(kw)
    n, slots = 257, 1000
    keys = rng.integers(0, 1 << 64, size=(slots, kw), dtype=np.uint64)
    slot = rng.integers(0, slots, size=n)
    out = ck.out(n * kw)
    nd = None if ndev is None else ck.up(np.array([ndev], dtype=np.uint64))
    assert ck.K.gather_keys(_ptr(ck.up(keys.reshape(-1))), _ptr(ck.up(slot.astype(np.int64).view(np.uint64))), _ptr(nd),
                            n, kw, _ptr(out), ck.stream) == 0
    m = n if ndev is None else min(ndev, n)
    got = ck.down(out)
    assert _clean(got, m * kw) and (got[:m * kw].reshape(m, kw) == keys[slot[:m]]).all()


def test_gather_keys_argument_checks(ck):
    keys, slot, out = ck.up(np.zeros(40, np.uint64)), ck.up(np.zeros(8, np.uint64)), ck.out(40)
    for kw in (0, 5):
        assert ck.K.gather_keys(_ptr(keys), _ptr(slot), None, 8, kw, _ptr(out), ck.stream) == R.INVALID_VALUE
    assert ck.K.gather_keys(_ptr(keys), _ptr(slot), None, 0, 2, _ptr(out), ck.stream) == 0
    assert _clean(ck.down(out))


def _reduce_inputs(rng, slots, ops):
    """dst, src planes: random words; f64 planes hold doubles of both signs with signed zeros and infinities (never
    opposite infinities in the same slot: no NaN)."""
    d = rng.integers(0, 1 << 64, size=(len(ops), slots), dtype=np.uint64)
    s = rng.integers(0, 1 << 64, size=(len(ops), slots), dtype=np.uint64)
    special = np.array([(0.0, -0.0), (-0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (np.inf, 1.0), (-np.inf, -np.inf),
                        (1.0, -1.0), (5e-324, 5e-324), (np.inf, np.inf), (-3.5, -np.inf)])
    for p, op in enumerate(ops):
        if op == R.OP_ADDF:
            a = rng.standard_normal(slots) * np.exp2(rng.integers(-60, 60, size=slots).astype(np.float64))
            b = rng.standard_normal(slots) * np.exp2(rng.integers(-60, 60, size=slots).astype(np.float64))
            at = rng.permutation(slots)[:len(special)]
            a[at], b[at] = special[:len(at), 0], special[:len(at), 1]
            d[p], s[p] = a.view(np.uint64), b.view(np.uint64)
    return d, s


_REDUCE = [(slots, [op]) for slots in (1, 257, 5000) for op in range(4)] + [
    (slots, [[1, 0, 3, 2][p % 4] for p in range(npl)]) for slots in (1, 257, 5000) for npl in (5, 32)]


@pytest.mark.parametrize("slots,ops", _REDUCE, ids=["%d-%s" % (s, "op%d" % o[0] if len(o) == 1 else len(o))
                                                    for s, o in _REDUCE])
def test_dense_reduce(ck, slots, ops):
    """dst op= src, plane by plane: one plane with each op, 5 and 32 planes with all four (plane 31's op in the top
    ops bits).  One IEEE addition is exact to the bit, signed zeros and infinities included."""
    rng = np.random.default_rng(slots + len(ops))
    d, s = _reduce_inputs(rng, slots, ops)
    dst, src = ck.words(d), ck.words(s)
    assert ck.K.dense_reduce(_ptr(dst), _ptr(src), slots, len(ops), R.ops_pack(ops), ck.stream) == 0
    got = ck.down(dst)
    ref = R.dense_reduce_ref(d, s, ops)
    assert not any(np.isnan(ref[p].view(np.float64)).any() for p, op in enumerate(ops) if op == R.OP_ADDF)
    assert _clean(got, len(ops) * slots) and (got[:len(ops) * slots].reshape(len(ops), slots) == ref).all()
    assert (ck.down(src)[:len(ops) * slots] == s.reshape(-1)).all()


def test_dense_reduce_argument_checks(ck):
    dst, src = ck.out(33 * 4), ck.out(33 * 4)
    assert ck.K.dense_reduce(_ptr(dst), _ptr(src), 0, 4, 0, ck.stream) == 0
    assert ck.K.dense_reduce(_ptr(dst), _ptr(src), 4, 0, 0, ck.stream) == 0
    assert ck.K.dense_reduce(_ptr(dst), _ptr(src), 4, 33, 0, ck.stream) == R.INVALID_VALUE
    assert _clean(ck.down(dst)) and _clean(ck.down(src))
