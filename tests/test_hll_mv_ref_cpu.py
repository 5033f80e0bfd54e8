"""The numpy model of the DISTINCTCOUNTHLLMV kernels (tests/hll_mv_ref.py) against the oracle's per-doc restatement of
DISTINCTCOUNTHLLMV and against hll.from_ints of the selected values' Java hash codes, on small random multi-value
data.  No GPU: this pins the model the kernel tests (tests/test_gpu_hll_mv_kernels.py) compare with."""
import numpy as np
import pytest

from oracle import pinot_oracle as O
from pinot_amd import extended as X
from pinot_amd import hll as H
from pinot_amd import pql
from tests import hll_mv_ref as M
from tests import hll_ref as R


def _data(dtype, seed, n=700):
    rng = np.random.default_rng(seed)
    if dtype == "STRING":
        pool = np.array(["t%d" % k for k in range(150)] + ["tab\there", "été", "中"])
    else:
        pool = np.unique(rng.integers(-(1 << 31), 1 << 31, 400)).astype(np.int64)
    counts = rng.integers(1, 5, n)
    counts[n // 2] = 70  # one long list
    docs = [pool[rng.integers(0, len(pool), c)].tolist() for c in counts]
    d = rng.integers(0, 10, n).astype(np.int32)
    return docs, counts, d


@pytest.mark.parametrize("dtype", ["INT", "STRING"])
@pytest.mark.parametrize("where", ["", " WHERE d < 3", " WHERE d = 77"])
def test_model_matches_oracle_and_from_ints(dtype, where):
    docs, counts, d = _data(dtype, 5 if dtype == "INT" else 6)
    oseg = O.OSegment.from_raw({"c": docs, "d": d}, dtypes={"c": dtype})
    q = pql.compile("SELECT DISTINCTCOUNTHLLMV(c) FROM t" + where)
    exp = O.run_aggregation(oseg, q, literal_filter=False)["results"][0]
    selected = {"": np.ones(len(d), bool), " WHERE d < 3": d < 3, " WHERE d = 77": d == 77}[where]
    flat = [v for doc in docs for v in doc]
    dictionary = sorted(set(flat))
    lookup = {v: i for i, v in enumerate(dictionary)}
    ids = np.array([lookup[v] for v in flat], np.int64)
    regs = M.offer(selected, counts, ids, R.codes(dtype, dictionary))
    assert regs.max() <= R.MAX_RANK
    assert list(regs.astype(np.uint8)) == list(exp)
    hashes = {X.java_hash_code(dtype, v) for doc, s in zip(docs, selected) if s for v in doc}
    assert regs.astype(np.uint8).tobytes() == H.from_ints(hashes).tobytes()
    assert regs.any() == bool(selected.any())


def test_group_model_is_the_per_slot_model():
    """offer_group: slot s's registers are offer() over the docs of slot s; docs outside the key space offer nothing."""
    docs, counts, d = _data("INT", 7, n=300)
    rng = np.random.default_rng(8)
    flat = np.array([v for doc in docs for v in doc])
    dictionary, ids = np.unique(flat, return_inverse=True)
    codes = R.codes("INT", dictionary.tolist())
    selected = rng.random(len(d)) < 0.6
    slot = d.astype(np.int64) - 1  # -1 .. 8: the docs of d = 0 and d = 9 fall outside 0..7
    table = M.offer_group(selected, counts, ids, codes, slot, 8)
    for s in range(8):
        np.testing.assert_array_equal(table[s], M.offer(selected & (slot == s), counts, ids, codes))
    assert M.starts(counts)[-1] == len(ids) and len(M.starts(counts)) == len(counts) + 1
