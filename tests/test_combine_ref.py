"""CPU checks of the combine-stage reference model (tests/combine_ref.py) itself, and of the premises of the case
generators the GPU tests use: a generator that drifts away from the branch it is meant to reach fails here."""
import math
import struct

import numpy as np
import pytest

from tests import combine_ref as R
from tests import narrow_ref as NR


def _plain_topk(keys, k):
    return sorted(sorted((int(x) for x in keys), reverse=True)[:k])


@pytest.mark.parametrize("n,k,span", [(1, 1, 10), (50, 7, 1 << 64), (500, 100, 8), (500, 500, 3), (500, 1, 1 << 40),
                                      (300, 299, 1 << 64), (64, 10, 1), (20, 30, 5)])
def test_trim_ref_matches_sorted(n, k, span):
    rng = np.random.default_rng(n * 1000 + k)
    keys = np.array([int(x) % span for x in rng.integers(0, 1 << 64, size=n, dtype=np.uint64)], dtype=np.uint64)
    ref = R.trim_ref(keys, k)
    assert ref.kept.tolist() == _plain_topk(keys, k)
    if k > n:
        assert ref.thr is None and len(ref.above) == n and ref.ties == 0 and ref.n_cand is None
        return
    assert ref.thr == sorted((int(x) for x in keys), reverse=True)[k - 1]
    assert ref.above.tolist() == [i for i, x in enumerate(keys) if int(x) > ref.thr]
    assert ref.n_eq == sum(1 for x in keys if int(x) == ref.thr)
    assert ref.ties == k - len(ref.above) and 1 <= ref.ties <= ref.n_eq
    lo, hi = int(keys.min()), int(keys.max())
    assert ref.hb == (lo ^ hi).bit_length()
    if ref.hb <= 11:
        assert ref.n_cand == 0
    else:
        sh = ref.hb - 11
        assert ref.n_cand == sum(1 for x in keys if int(x) >> sh >= ref.thr >> sh) >= k


def test_trim_ref_seeded_range_widens_hb():
    keys = np.array([0x1000, 0x1001, 0x1003, 0x1002], dtype=np.uint64)
    assert R.trim_ref(keys, 2).hb == 2 and R.trim_ref(keys, 2).n_cand == 0
    wide = R.trim_ref(keys, 2, krange=(0, 0x1FFF))
    assert wide.hb == 13 and wide.thr == 0x1002 and wide.n_cand == 4  # first digit: bits [2, 13)


def _f(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _b(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _i64(bits):
    return bits - (1 << 64) if bits >> 63 else bits


def _lt_f(a, b):
    """a < b as doubles, with -0.0 below +0.0."""
    return a < b or (a == b == 0.0 and math.copysign(1, a) < math.copysign(1, b))


def test_trim_key_preserves_order_of_each_kind():
    rng = np.random.default_rng(5)
    n = 400
    count = rng.integers(0, 50, size=n, dtype=np.uint64)
    count[:40] = 0
    ints = rng.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64)
    ints[40:80] = rng.integers(-5, 5, size=40)
    ints = ints.view(np.uint64)
    dbl = rng.standard_normal(n) * np.exp2(rng.integers(-200, 200, size=n).astype(np.float64))
    dbl[:6] = [-0.0, 0.0, 5e-324, -5e-324, 1.0, -1.0]
    dbl = dbl.view(np.uint64)
    u = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)

    def avg(c, s):
        return s / c if c else 0.0

    values = {  # kind -> (value plane, the underlying value, its "less than")
        R.TK_COUNT: (u, lambda i: int(count[i]), int.__lt__),
        R.TK_SUM: (ints, lambda i: _i64(int(ints[i])), int.__lt__),
        R.TK_MIN: (u, lambda i: -int(u[i]), int.__lt__),  # a smaller ordered minimum is the better group
        R.TK_MAX: (u, lambda i: int(u[i]), int.__lt__),
        R.TK_SUMF: (dbl, lambda i: _f(int(dbl[i])), _lt_f),
        R.TK_AVG: (ints, lambda i: avg(int(count[i]), float(_i64(int(ints[i])))), _lt_f),
        R.TK_AVGF: (dbl, lambda i: avg(int(count[i]), _f(int(dbl[i]))), _lt_f),
    }
    for kind, (plane, under, lt) in values.items():
        keys = R.trim_key(kind, count, plane)
        assert keys.dtype == np.uint64
        order = np.argsort(keys, kind="stable")
        for a, b in zip(order[:-1], order[1:]):
            ka, kb, va, vb = int(keys[a]), int(keys[b]), under(a), under(b)
            assert (ka < kb) == lt(va, vb) and (ka == kb) == (not lt(va, vb) and not lt(vb, va)), (kind, va, vb)
    # the cases named in the model's contract
    k = R.trim_key(R.TK_SUMF, [1, 1], np.array([_b(-0.0), _b(0.0)], dtype=np.uint64))
    assert k[0] < k[1]
    k = R.trim_key(R.TK_SUM, [1, 1, 1], np.array([-3, 0, 2], dtype=np.int64).view(np.uint64))
    assert k[0] < k[1] < k[2]
    k = R.trim_key(R.TK_AVG, [0, 2, 2], np.array([99, -4, 4], dtype=np.int64).view(np.uint64))
    assert k[1] < k[0] < k[2] and int(k[0]) == NR.ordered_f64(0.0)  # count 0: the ratio is 0.0
    k = R.trim_key(R.TK_AVGF, [0, 4], np.array([_b(-7.0), _b(-0.0)], dtype=np.uint64))
    assert int(k[0]) == NR.ordered_f64(0.0) and int(k[1]) == NR.ordered_f64(-0.0)
    # an int64 sum above 2^53 rounds to the nearest double (ties to even) before the division
    k = R.trim_key(R.TK_AVG, [1, 1], np.array([(1 << 53) + 1, (1 << 53) + 3], dtype=np.int64).view(np.uint64))
    assert int(k[0]) == NR.ordered_f64(float(1 << 53)) and int(k[1]) == NR.ordered_f64(float((1 << 53) + 4))


def test_ordered_f64_bits_is_narrow_refs_and_inverts():
    rng = np.random.default_rng(6)
    v = np.concatenate([rng.standard_normal(200) * 1e300, rng.standard_normal(200) * 1e-310, [0.0, -0.0, 5e-324]])
    bits = np.ascontiguousarray(v).view(np.uint64)
    keys = R.ordered_f64_bits(bits)
    assert keys.tolist() == [NR.ordered_f64(x) for x in v]
    assert R.ordered_f64_inv(keys).tolist() == bits.tolist()
    for kind in (R.TK_COUNT, R.TK_SUM, R.TK_MIN, R.TK_MAX, R.TK_SUMF):
        back = R.trim_key(kind, R.value_for_key(kind, keys), R.value_for_key(kind, keys))
        assert back.tolist() == keys.tolist()


def test_state_layout():
    assert R.STATE_BYTES == 64 + 4 * 2048 + 8 and R.ST_NCAND == 64 + 4 * 2048
    img = R.state_init(3, 77)
    assert len(img) == 3 * R.STATE_BYTES
    for f in range(3):
        st = R.state_read(img, f)
        assert st["k"] == 77 and st["kmin"] == R.M64 and not st["hist"].any()
        assert all(st[x] == 0 for x in ("prefix", "mask", "shift", "done", "n_sel", "n_tie", "kmax", "n_cand"))
    assert int(img.sum()) == 3 * (77 + 8 * 255)


def test_merge_mix_and_home_slot_search():
    assert R.merge_mix(0) == 0
    xs = [1, 2, 0xDEADBEEF, (1 << 63) - 1, R.M64]
    assert R.merge_mix_np(np.array(xs, dtype=np.uint64)).tolist() == [R.merge_mix(x) for x in xs]
    assert len({R.merge_mix(x) for x in range(4096)}) == 4096  # a bijection
    for cap, slot in ((1024, 1023), (256, 0), (8192, 4097)):
        keys = R.keys_homed_at(cap, slot, 64)
        assert len(set(keys)) == 64 and all(0 < k < (1 << 63) for k in keys)
        assert all(R.merge_mix(k) & (cap - 1) == slot for k in keys)


def test_merge_and_friends_models():
    ops = [R.OP_ADD, R.OP_ADDF, R.OP_MIN, R.OP_MAX]
    assert R.ops_pack(ops) == 0b11100100
    keys = [5, 9, 5, 5]
    planes = [np.array([R.M64, 1, 3, 4], dtype=np.uint64),
              np.array([1.5, 2.0, -0.25, 1e-3]).view(np.uint64),
              np.array([7, 8, 1 << 63, 9], dtype=np.uint64), np.array([7, 8, 1 << 63, 9], dtype=np.uint64)]
    out, aux = R.group_merge_ref(keys, planes, ops)
    assert out[5] == [6, _b(math.fsum([1.5, -0.25, 1e-3])), 7, 1 << 63] and out[9] == [1, _b(2.0), 8, 8]
    assert aux[5][1] == (math.fsum([1.5, 0.25, 1e-3]), 3)
    tkey, tpl = R.table_init(8, ops)
    assert (tkey == R.M64).all() and (tpl[2] == R.M64).all() and not tpl[[0, 1, 3]].any()
    d = np.array([[R.M64], [_b(1.0)], [5], [5]], dtype=np.uint64)
    s = np.array([[2], [_b(float("inf"))], [4], [4]], dtype=np.uint64)
    assert R.dense_reduce_ref(d, s, ops)[:, 0].tolist() == [1, _b(float("inf")), 4, 5]
    okey, opl = np.array([10, 11, 12], dtype=np.uint64), np.arange(6, dtype=np.uint64).reshape(2, 3)
    assert R.pack_ref(okey, opl, 2).tolist() == [[10, 0, 3], [11, 1, 4]]
    comb = np.zeros((5, 3), dtype=np.uint64)
    lat = np.arange(100, 112, dtype=np.uint64).reshape(4, 3)
    got, miss = R.join_ref([10, 11, 12], [12, 99, 10], lat, comb, 2)
    assert miss == 1 and got.tolist() == [[0, 0, 0], [0, 0, 0], [105, 0, 103], [108, 0, 106], [111, 0, 109]]


# ---------------------------------------------------------------------------------------------------------------------
# premises of the GPU cases
# ---------------------------------------------------------------------------------------------------------------------
def test_every_trim_case_builds_and_fits_the_launcher():
    assert len(set(R.TRIM_CASES)) == len(R.TRIM_CASES)
    for name in R.TRIM_CASES:
        c = R.trim_case(name)
        nf = len(c["kinds"])
        assert 1 <= nf <= R.MAX_FNS and len(c["planes"]) == nf and c["grid"] >= 1 and c["k"] >= 1
        assert c["n"] <= c["ocap"] and c["n"] <= 130000 and c["cap"] >= c["k"] and c["ccap"] >= 0
        assert all(0 <= p < c["oplane"].shape[0] for p in c["planes"])
        assert c["oplane"].dtype == np.uint64
        again = R.trim_case(name)
        assert (again["oplane"] == c["oplane"]).all()  # deterministic
        for f in range(nf):
            keys = R.case_keys(c, f)
            if c["kinds"][f] >= R.TK_AVG:  # inputs never give a NaN key
                assert not np.isnan(R.ordered_f64_inv(keys).view(np.float64)).any()
            if R.case_seeded(c) and c["n"]:  # a seeded range brackets the keys
                kind = c["kinds"][f]
                assert int(c["prange"][kind]) <= int(keys.min()) and int(keys.max()) <= int(c["prange"][4 + kind])


@pytest.mark.parametrize("hb", R.HBS)
def test_hb_cases_have_exactly_the_width_asked(hb):
    c = R.trim_case("hb_%d" % hb)
    ref = R.case_ref(c, 0)
    assert ref.hb == hb == c["premise"]["hb"]
    assert (ref.n_cand == 0) == (hb <= 11)


def test_signed_sums_vary_in_all_64_bits():
    c = R.trim_case("sum_signed")
    assert c["kinds"] == [R.TK_SUM] and R.case_ref(c, 0).hb == 64
    s = c["oplane"][1, :c["n"]].view(np.int64)
    assert (s < 0).any() and (s > 0).any()


@pytest.mark.parametrize("v", ["g1", "g1w", "g1c", "g3", "g3w", "g3s"])
def test_tie_cases_overflow_the_lds_tie_list(v):
    c = R.trim_case("tiecap_" + v)
    ref = R.case_ref(c, 0)
    ties = R.range_ties(c)
    assert ref.thr == c["premise"]["thr"] and ref.ties == c["premise"]["want"] and ref.n_eq == sum(ties) == 5000
    assert max(ties) > R.TIE_CAP  # one workgroup's range holds more threshold ties than its LDS list
    over = sum(max(t - R.TIE_CAP, 0) for t in ties)  # ties reserved per wave; the rest at the workgroups' ends
    assert 0 < ref.ties < ref.n_eq  # some ties are kept and some refused
    if v in ("g1w", "g3w"):
        assert ref.ties > over  # the per-wave reservations cannot fill the quota: the LDS lists take some too
    if v == "g3s":
        assert sum(1 for t in ties if 0 < t <= R.TIE_CAP) == 2  # n_tie shared with workgroups that only use the list
    if v == "g1c":  # the select scans the candidate list: every group at or above the first digit's bin, one range
        assert c["grid"] == 1 and 0 < ref.n_cand <= c["ccap"]
    else:
        assert c["ccap"] == 0  # the select scans the planes: the ranges above are the kernel's


@pytest.mark.parametrize("w", [22, 64])
def test_candidate_cases_stand_where_they_should(w):
    passes = {22: 2, 64: 6}[w]
    got = {}
    for v in ("none", "all", "exact", "short", "flush"):
        c = R.trim_case("cand_w%d_%s" % (w, v))
        ref = R.case_ref(c, 0)
        assert ref.hb == w and -(-w // R.DIGIT) == passes and ref.n_cand >= c["k"]
        got[v] = (c["ccap"], ref.n_cand)
        if v == "flush":
            assert c["grid"] == 1 and R.range_cands(c) == [ref.n_cand] and ref.n_cand > R.CAND_FLUSH
            # ... and the list passes CAND_FLUSH before the range's last round of 256 groups
            keys = R.case_keys(c, 0)
            sh = ref.hb - R.DIGIT
            early = keys[:c["n"] - 256] >= np.uint64(ref.thr >> sh << sh)
            assert int(early.sum()) > R.CAND_FLUSH
    assert got["none"][0] == 0
    assert got["all"][0] >= 20000
    assert got["exact"][0] == got["exact"][1]
    assert got["short"][0] == got["short"][1] - 1 > 0  # abandoned: candidate count > ccap
    assert got["flush"][1] <= got["flush"][0]


def test_count_cases_cover_the_edges():
    assert {n for n, _, _ in R.COUNT_CASES} == {0, 1, 255, 256, 257}
    for n, k, g in R.COUNT_CASES:
        assert k >= 1 and g in (1, 4)
    assert any(g > -(-n // 256) for n, _, g in R.COUNT_CASES)  # idle workgroups
    for n in (1, 255, 256, 257):
        ks = {k for m, k, _ in R.COUNT_CASES if m == n}
        assert {1, n, n + 5} <= ks and (n == 1 or n - 1 in ks)


def test_kind_cases_hold_the_values_they_claim():
    kinds = [R.trim_case("kind_%d" % kd) for kd in range(7)]
    assert [c["kinds"][0] for c in kinds] == list(range(7))
    assert all(c["planes"][0] != 1 + c["kinds"][0] - 1 or c["kinds"][0] == 0 for c in kinds[1:4])  # not planes 1..3
    assert [c["planes"][0] for c in kinds[1:4]] == [4, 5, 6]  # 1 + 3c + r at c = 1
    avg = kinds[R.TK_AVG]
    n = avg["n"]
    cnt, s = avg["oplane"][0, :n], avg["oplane"][4, :n].view(np.int64)
    assert (cnt == 0).any() and (s < 0).any() and (np.abs(s) > (1 << 53)).any()
    assert (s[np.abs(s) > (1 << 53)].astype(np.float64).astype(np.int64) != s[np.abs(s) > (1 << 53)]).any()
    v = kinds[R.TK_SUMF]["oplane"][4, :n]
    d = v.view(np.float64)
    assert {R.SIGN, 0} <= set(v.tolist()) and (d < 0).any()
    assert ((d != 0) & (np.abs(d) < 2.2250738585072014e-308)).sum() >= 4  # subnormals of both signs
    assert (kinds[R.TK_AVGF]["oplane"][0, :n] == 0).any()


def test_seed_cases():
    exact, loose, poison, null = (R.trim_case("seed_" + v) for v in ("exact", "loose", "poison", "null"))
    assert R.case_seeded(exact) and R.case_seeded(loose) and not R.case_seeded(poison) and not R.case_seeded(null)
    assert null["prange"] is None and poison["prange"] is not None and R.TK_AVG in poison["kinds"]
    widened = 0
    for f, kind in enumerate(exact["kinds"]):
        keys = R.case_keys(exact, f)
        assert (int(exact["prange"][kind]), int(exact["prange"][4 + kind])) == (int(keys.min()), int(keys.max()))
        assert int(loose["prange"][kind]) <= int(keys.min()) and int(keys.max()) <= int(loose["prange"][4 + kind])
        widened += (int(loose["prange"][kind]), int(loose["prange"][4 + kind])) != (int(keys.min()), int(keys.max()))
        assert R.case_ref(loose, f).kept.tolist() == R.case_ref(exact, f).kept.tolist()
    assert widened == len(exact["kinds"])
    # the poisoned ranges say "every key equals the smallest": read, they would end the select at a wrong threshold
    for f, kind in enumerate(poison["kinds"]):
        if kind < 4:
            assert int(poison["prange"][kind]) == int(poison["prange"][4 + kind]) != R.case_ref(poison, f).thr


def test_side_by_side_cases():
    c = R.trim_case("nf8")
    assert len(c["kinds"]) == 8 and set(c["kinds"]) == set(range(7)) and c["cap"] > c["k"]
    assert len(R.trim_case("nf1")["kinds"]) == 1
