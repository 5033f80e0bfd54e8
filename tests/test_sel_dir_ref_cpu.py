"""The numpy model of the sparse GROUP BY's directory key and group lookup (tests/sel_dir_ref.py) against arithmetic
written out independently here: field widths, the one-word / two-word boundary at exactly 64 and 65 bits, the refusal
at 129 bits, injectivity on random ids at the boundaries, the lookup and the group-by-key answer.  No GPU."""
import numpy as np
import pytest

from tests import sel_dir_ref as S

C31 = 1 << 31


def test_field_widths():
    assert [S.field_bits(c) for c in (0, 1, 2, 3, 4, 5, 300, 65536, 65537, C31 - 1, C31)] == \
        [1, 1, 1, 2, 2, 3, 9, 16, 17, 31, 31]


@pytest.mark.parametrize("cards, total, W", [
    ([300, 300], 18, 1),
    ([C31, C31, 4], 64, 1),        # exactly 64 bits: one word
    ([C31, C31, 5], 65, 2),        # 65: two words, the last field straddles bit 64
    ([1 << 30] * 3, 90, 2),        # the third field starts at bit 60
    ([C31] * 4 + [16], 128, 2),    # exactly 128 bits
    ([2] * 16, 16, 1),
])
def test_layout_and_word_boundary(cards, total, W):
    lay = S.layout(cards)
    assert lay["total"] == total and lay["W"] == W
    at = 0
    for b, sh, w in zip(lay["bits"], lay["shift"], lay["word"]):
        assert 64 * w + sh == at
        at += b


def test_keys_over_128_bits_and_bad_column_counts_are_refused():
    with pytest.raises(ValueError):
        S.layout([C31] * 4 + [17])  # 129 bits
    with pytest.raises(ValueError):
        S.layout([])
    with pytest.raises(ValueError):
        S.layout([2] * 17)


@pytest.mark.parametrize("cards", [[300, 300], [C31, C31, 4], [C31, C31, 5], [1 << 30] * 3, [C31] * 4 + [16],
                                   [1, 1, 1], [2] * 16, [70000, 3, 1 << 20, 129]])
def test_packing_is_injective_and_matches_big_integer_arithmetic(cards):
    rng = np.random.default_rng(len(cards) * 1000 + sum(c % 97 for c in cards))
    lay = S.layout(cards)
    gids = np.stack([rng.integers(0, c, 3000) for c in cards], axis=1)
    gids[0] = 0
    gids[1] = [c - 1 for c in cards]  # every field all ones where the cardinality is a power of two
    keys, ok = S.pack(lay, gids)
    assert ok.all()
    want, at = [0] * len(gids), 0
    for g, c in enumerate(cards):
        for i in range(len(gids)):
            want[i] |= int(gids[i, g]) << at
        at += S.field_bits(c)
    got = S.key_ints(keys)
    assert got == want
    assert len(set(got)) == len({tuple(r) for r in gids.tolist()})
    if lay["W"] == 1:
        assert (keys[:, 1] == 0).all()


def test_ids_outside_their_field_are_no_keys():
    lay = S.layout([300, 300])
    keys, ok = S.pack(lay, [[-1, 5], [5, 512], [511, 511], [0, 0]])
    assert ok.tolist() == [False, False, True, True]
    assert S.key_ints(keys)[2] == 0x3FFFF


def test_row_groups_and_misses():
    lay = S.layout([300, 300])
    group_keys, _ = S.pack(lay, [[7, 9], [0, 0], [299, 299]])
    got = S.row_groups(lay, group_keys, [[0, 0], [7, 9], [9, 7], [299, 299], [-1, 0], [299, 298]])
    assert got.tolist() == [1, 0, -1, 2, -1, -1]


def test_group_by_key_answer():
    rng = np.random.default_rng(3)
    gids = np.stack([rng.integers(0, 5, 200), rng.integers(0, 7, 200)], axis=1)
    sel = rng.random(200) < 0.4
    uniq, idx = S.group_by(gids, sel)
    want = sorted({tuple(r) for r in gids[sel].tolist()})
    assert [tuple(r) for r in uniq.tolist()] == want
    for i in range(200):
        assert idx[i] == (want.index(tuple(gids[i].tolist())) if sel[i] else -1)
    uniq, idx = S.group_by(gids, np.zeros(200, bool))
    assert len(uniq) == 0 and (idx == -1).all()


def test_capacity_and_struct():
    assert [S.capacity(n) for n in (0, 1, 2, 3, 33, 1000, 131072)] == [2, 2, 4, 8, 128, 2048, 262144]
    import ctypes as C
    assert C.sizeof(S.SelSparseKey) == 104
