"""CPU checks of tests/narrow_ref.py, the reference model the GPU tests of the narrow group-by kernels compare against:
the key mix inverts exactly, the value images round-trip, and the round model of the split's owner lanes gives the
unit counts the GPU tests rely on (the worst-case inputs reach the list's bound exactly; every input fits the list)."""
import numpy as np
import pytest

from tests import narrow_ref as R


@pytest.mark.parametrize("K", [1, 2, 31, 32, 33, 63, 64])
def test_mix_is_a_bijection_and_inverts(K):
    top = 1 << K
    rng = np.random.default_rng(K)
    keys = {0, 1, top - 1, top >> 1, (top >> 1) - 1 if K > 1 else 0}
    keys |= {int(x) & (top - 1) for x in rng.integers(0, 1 << 63, 4000, dtype=np.uint64) * 2 + 1}
    keys |= {(1 << i) & (top - 1) for i in range(K)}
    hs = set()
    for k in keys:
        h = R.mix(k, K)
        assert 0 <= h < top
        assert R.unmix(h, K) == k
        hs.add(h)
    assert len(hs) == len(keys)
    for h in list(keys)[:500]:  # and the other way round: the inverse is a right inverse too
        assert R.mix(R.unmix(h, K), K) == h
    mask, s, ic1 = R.mix_params(K)
    assert (R.C1 * ic1) & R.M64 == 1 and s == (K + 1) // 2 and 2 * s >= K


def test_small_mix_is_a_permutation():
    for K in (1, 2, 9):
        assert sorted(R.mix(k, K) for k in range(1 << K)) == list(range(1 << K))


def _sorted_rel(rng, card, step):
    return np.cumsum(rng.integers(1, step + 1, card)).astype(np.int64)


def test_images_round_trip():
    rng = np.random.default_rng(3)
    rel = _sorted_rel(rng, 1000, 4000)
    img, sh = R.img1(rel)
    assert [R.img_value(1, img, sh, d) for d in range(1000)] == rel.tolist()
    rel = _sorted_rel(rng, 64 << 4, 4000)  # all 64 blocks
    img, sh = R.img2(rel, 4)
    assert len(img) == 64 + 512 and len(img) <= R.IMG_WORDS
    assert [R.img_value(2, img, sh, d) for d in range(len(rel))] == rel.tolist()
    img, sh = R.img2(rel[:333], 4)  # odd cardinality: the last u16 pair is half used
    assert [R.img_value(2, img, sh, d) for d in range(333)] == rel[:333].tolist()
    for b, bsh, step, card in ((1, 1, 1, 601), (11, 4, 130, 1000), (16, 6, 1000, 777)):
        rel = _sorted_rel(rng, card, step) + 12345
        img, ish = R.img4(rel, bsh, b)
        nblk = (card + (1 << bsh) - 1) >> bsh
        assert ish == bsh | (b << 5) | (nblk << 10)
        assert len(img) == nblk + (card * b + 31) // 32 + 1 and img[-1] == 0  # the pad dword
        assert [R.img_value(4, img, ish, d) for d in range(card)] == rel.tolist()
    # offsets that straddle dwords exist at b = 11 and b = 16 never does
    assert any((d * 11 & 31) + 11 > 32 for d in range(1000))


def test_split_ref_small():
    # rb1 = 5, k2 = 2: x = d << 5 | sub << 3 | low
    x = [(9 << 5) | (2 << 3) | 5, (1 << 5) | (2 << 3) | 7, (3 << 5) | (0 << 3) | 1]
    got = R.split_ref([[x[:2]], [x[2:]]], 5, 2)
    assert got == {2: sorted([(9 << 3) | 5, (1 << 3) | 7]), 4: [(3 << 3) | 1]}


def test_groupby_ref_small():
    recs = [[(7 << 4) | 3, (2 << 4) | 3, (5 << 4) | 1], [], [(1 << 4) | 3]]
    got = R.groupby_ref(recs, 4, lambda f: f - 4)
    assert got == {(0, 3): [2, 1, -2, 3], (0, 1): [1, 1, 1, 1], (2, 3): [1, -3, -3, -3]}
    got = R.groupby_ref([[0, 1 << 4]], 4, lambda f: [0.0, -0.0][f])
    assert str(got[(0, 0)][2]) == "-0.0" and str(got[(0, 0)][3]) == "0.0"


@pytest.mark.parametrize("W,units", [(2, 1920), (1, 1472)])
def test_worst_case_input_reaches_the_list_bound(W, units):
    assert R.list_bound(W) == units and units <= R.list_cap(W)
    subs = R.worst_case_subs(W)
    assert len(subs) == (16384 if W == 2 else 24576)
    rounds = R.units_per_round([subs], 10, W)
    assert rounds[-1] == units and max(rounds) == units
    for k2 in range(0, 11):  # the bound is largest at the most sub-buckets
        assert R.list_bound(W, k2) <= units
    # the GPU test's input is this one
    inp = R.split_input("worst", W)
    for bucket in inp["slabs"]:
        got = R.units_per_round([R.split_subs(s, inp["rb1"], inp["k2"]) for s in bucket], inp["k2"], W)
        assert max(got) == units


def test_random_inputs_never_exceed_the_bound():
    """The bound is a bound: uniform, skewed and few-sub-bucket inputs, in one slab or many, for every k2."""
    rng = np.random.default_rng(0)
    for W in (1, 2):
        for k2 in (0, 3, 9, 10):
            n = 1 << k2
            for subs in (rng.integers(0, n, 1 << 16), rng.integers(0, max(1, n // 8), 1 << 16),
                         np.minimum(rng.geometric(0.01, 1 << 16) - 1, n - 1), R.worst_case_subs(W) % n):
                for slabs in ([subs], np.array_split(subs, 7)):
                    assert max(R.units_per_round(slabs, k2, W)) <= R.list_bound(W, k2) <= R.list_bound(W)


@pytest.mark.parametrize("name,args", R.split_inputs(), ids=[n for n, _ in R.split_inputs()])
def test_split_inputs_fit_the_unit_list(name, args):
    inp = R.split_input(**args)
    W, k2, rb1 = inp["W"], inp["k2"], inp["rb1"]
    assert inp["cap2"] % 32 == 0 and rb1 <= 48 and 0 <= k2 <= min(10, rb1)
    width = max(int(s.max()).bit_length() for bk in inp["slabs"] for s in bk if len(s))
    assert width <= (48 if inp["hi"] else 32)
    for bucket, claim in zip(inp["slabs"], inp["claim"]):
        assert all(len(s) == min(c, inp["cap1"]) for s, c in zip(bucket, claim))
        got = R.units_per_round([R.split_subs(s, rb1, k2) for s in bucket], k2, W)
        assert max(got, default=0) <= R.list_cap(W)
    for recs in R.split_ref(inp["slabs"], rb1, k2).values():  # output records fit W words
        assert recs[-1] < 1 << (32 * W)
