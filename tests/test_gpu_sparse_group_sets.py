"""DISTINCTCOUNTHLL[MV], DISTINCTCOUNT[MV] and PERCENTILE[MV] under GROUP BY over key spaces the dense route refuses
(PGX_X_SPARSE_GROUP_SETS: pinot_amd/csrc/pgx_hll.cpp run_hll, the group directory of pgx_hll.hip), end to end: at the
ABI with the flag against numpy models of the groups' registers, hash-code sets and (value, count) pairs, and through
the plan maker with PGX_SPARSE_SETS_NATIVE=1 against the same request with the knob at 0 (the decomposition): the
intermediates, the reduced values, the trimmed maps and all four statistics.  Every comparison is exact.

Two segments of 3,001 and 2,500 rows with per-segment dictionaries (tests/test_gpu_distinct.py's columns) and more
group columns: ka x kb is a key space of 400 x 350 = 140,000 slots; w0 .. w9 hold a value of their own in every row
(5,501 global ids, 13 bits each), so GROUP BY w0 .. w4 is a key of 65 bits -- two key words.  (With a few thousand rows
no three columns reach 64 bits: a column's field is ceil(log2(its global cardinality)) bits, at most 13 here, so the
two-word key takes five.)  GROUP BY w0 .. w9 is 130 bits, past every route.  `big` is an INT column with a dictionary
of 500,000 values that both segments share: 62,500 bytes of presence bits or 4,000,000 bytes of counters per group.
A third segment of 140,000 rows, every row a group of its own under GROUP BY x0, x1, is for the limits that only many
groups reach: PGX_SET_MAX_SPARSE_GROUPS and PGX_HLL_MAX_TABLE_BYTES."""
from collections import Counter

import numpy as np
import pytest

from pinot_amd import extended as X
from pinot_amd import hll as HLL
from pinot_amd import pql
from pinot_amd import segment as S
from tests.test_gpu_distinct import MV_COLS, TYPES, _columns, _n, _plan, _raw
from tests.test_gpu_percentile import _same_blocks

pytestmark = pytest.mark.gpu

SIZES = (3001, 2500)
BIG_CARD = 500000
MAX_SPARSE_GROUPS = 131072                     # PGX_SET_MAX_SPARSE_GROUPS
MAX_TABLE_BYTES = 256 << 20                    # PGX_HLL_ / PGX_DISTINCT_ / PGX_PERCENTILE_MAX_TABLE_BYTES
WIDE = ["w%d" % k for k in range(10)]
MANY = 140000


def _extra(i, n):
    rng = np.random.default_rng(900 + i)
    first = sum(SIZES[:i])
    raw = {"ka": (rng.integers(0, 300, n) + 100 * i).astype(np.int32),      # union: 400 values
           "kb": (rng.integers(0, 300, n) + 50 * i).astype(np.int32)}       # union: 350 values
    for w in WIDE:
        raw[w] = (rng.permutation(n) + first).astype(np.int32)             # a value of its own in every row
    return raw, rng.integers(0, BIG_CARD, n)


@pytest.fixture(scope="module")
def env():
    from pinot_amd import engine as E
    ctx = E.Context(0)
    gsegs, raws = [], []
    big_dict = np.arange(BIG_CARD, dtype=np.int32) * 3 - 700000
    for i, n in enumerate(SIZES):
        raw, dicts, ids = _raw(i, n)
        extra, big_ids = _extra(i, n)
        cols = _columns(raw, dicts, ids) + [S.make_column(c, v, data_type="INT") for c, v in extra.items()]
        cols.append(S.make_column("big", None, data_type="INT", dictionary=big_dict, dict_ids=big_ids))
        raw.update(extra)
        raw["big"] = big_dict[big_ids]
        gsegs.append(E.IndexSegment(ctx, S.make_segment("sg%d" % i, cols)))
        raws.append(raw)
    assert len(np.unique(np.concatenate([r["ka"] for r in raws]))) == 400
    assert len(np.unique(np.concatenate([r["kb"] for r in raws]))) == 350
    assert len(np.unique(np.concatenate([r["w0"] for r in raws]))) == sum(SIZES) > 4096
    yield ctx, gsegs, raws
    ctx.close()


@pytest.fixture(scope="module")
def many():
    """140,000 rows, every row a group under GROUP BY x0, x1 (two fields of 18 bits); r numbers the rows."""
    from pinot_amd import engine as E
    ctx = E.Context(0)
    rng = np.random.default_rng(77)
    raw = {"x0": rng.permutation(MANY).astype(np.int32), "x1": rng.permutation(MANY).astype(np.int32),
           "r": np.arange(MANY, dtype=np.int32)}
    for c in ("a", "b", "c"):
        raw[c] = rng.integers(0, 200, MANY).astype(np.int32)
    seg = E.IndexSegment(ctx, S.make_segment("many", [S.make_column(c, v, data_type="INT") for c, v in raw.items()]))
    yield ctx, [seg], raw
    ctx.close()


FILTERS = [
    ("", lambda r: np.ones(_n(r), bool)),                                      # match-all
    (" WHERE m < 300", lambda r: r["m"] < 300),                                # a scan leaf
    (" WHERE b = 3 OR m < 50", lambda r: (r["b"] == 3) | (r["m"] < 50)),       # a bitmap leaf OR a scan leaf
]
NOTHING = (" WHERE m = 123456", lambda r: np.zeros(_n(r), bool))

# the library's functions (E._Query), one of each family and form beside standard ones; and the same as PQL
LIB_FNS = [("distinctcounthll", "ci"), ("sum", "m"), ("distinctcount", "cl"), ("percentile", "cf"), ("count", "*"),
           ("distinctcounthllmv", "ti"), ("distinctcountmv", "ts"), ("percentilemv", "ti"), ("distinctcounthll", "s")]
PQL_FNS = ("DISTINCTCOUNTHLL(ci), SUM(m), DISTINCTCOUNT(cl), PERCENTILE90(cf), COUNT(*), DISTINCTCOUNTHLLMV(ti), "
           "DISTINCTCOUNTMV(ts), PERCENTILE50MV(ti), DISTINCTCOUNTHLL(s), PERCENTILEEST95(cf)")
ALONE = [[("distinctcounthll", "ci")], [("distinctcounthllmv", "ti")], [("distinctcount", "cl")],
         [("distinctcountmv", "ti")], [("percentile", "cd")], [("percentilemv", "ti")]]
KEYS = [("ka", "kb"), ("w0", "w1", "w2", "w3", "w4")]  # 18 bits: one key word; 65 bits: two


def _request(fns, gcols, where):
    q = pql.compile("SELECT COUNT(*) FROM t%s GROUP BY %s" % (where, ", ".join(gcols)))
    return {"aggregations": [{"fn": f, "column": c} for f, c in fns], "group_by": q["group_by"],
            "filter": q.get("filter")}


def _native(ctx, gsegs, q, flags):
    from pinot_amd import engine as E
    from pinot_amd import native as N
    qq = E._Query(ctx, q)
    try:
        r = qq.execute(gsegs, flags)
        try:
            return E.decode_result(qq, r, gsegs, trim=True)
        finally:
            N.lib().pgx_result_release(r)
    finally:
        qq.close()


def _status(fn):
    from pinot_amd import native as N
    with pytest.raises(N.PgxError) as e:
        fn()
    return e.value.status, str(e.value)


def _group_keys(r, gcols):
    return np.array(["\t".join(str(int(r[g][d])) for g in gcols) for d in range(_n(r))])


_ROW_CACHE = {}


def _row_values(r, col):
    """Per row of a segment the list of its values of `col` (one for a single-value column) and of their hash codes."""
    key = (id(r), col)
    if key not in _ROW_CACHE:
        vals = [list(v) for v in r[col]] if col in MV_COLS else [[v] for v in r[col].tolist()]
        code = {}
        for vs in vals:
            for v in vs:
                if v not in code:
                    code[v] = X.java_hash_code(TYPES.get(col, "INT"), v)
        _ROW_CACHE[key] = (vals, [[code[v] for v in vs] for vs in vals])
    return _ROW_CACHE[key]


def _model(raws, masks, gcols, fns):
    """{group key: [the intermediate of every function]}: registers (uint8[256]), the set of hash codes, ascending
    (value, count) pairs, a sum or a count.  One pass over the selected rows."""
    acc = {}
    for r, m in zip(raws, masks):
        keys = _group_keys(r, gcols)
        for d in np.flatnonzero(m):
            a = acc.get(keys[d])
            if a is None:
                a = acc[keys[d]] = [set() if f.startswith("distinctcount") else Counter() if f.startswith("percentile")
                                    else 0 for f, _ in fns]
            for i, (fn, col) in enumerate(fns):
                if fn.startswith("distinctcount"):
                    a[i].update(_row_values(r, col)[1][d])
                elif fn.startswith("percentile"):
                    a[i].update(float(v) for v in _row_values(r, col)[0][d])
                elif fn == "sum":
                    a[i] += int(r[col][d])
                else:
                    a[i] += 1
    out = {}
    for k, a in acc.items():
        out[k] = [HLL.from_ints(v) if "hll" in fn else v if fn.startswith("distinctcount")
                  else sorted(v.items()) if fn.startswith("percentile") else float(v) if fn == "sum" else v
                  for (fn, _), v in zip(fns, a)]
    return out


def _check_model(got, model, fns):
    assert set(got) == set(model)
    for k in got:
        for (fn, col), a, b in zip(fns, got[k], model[k]):
            if "hll" in fn:
                assert a.dtype == np.uint8 and a.tobytes() == b.tobytes(), (k, fn, col)  # byte for byte
            elif isinstance(b, (set, list)):
                assert type(a) is type(b) and a == b, (k, fn, col)
            else:
                assert a == b, (k, fn, col)


def _knob(monkeypatch, ctx, gsegs, q, value):
    monkeypatch.setenv("PGX_SPARSE_SETS_NATIVE", value)
    try:
        return _plan(ctx, gsegs, q)
    finally:
        monkeypatch.delenv("PGX_SPARSE_SETS_NATIVE")


def _on(monkeypatch, ctx, gsegs, q):
    """Through the plan maker with the sparse route (opt-in there: PGX_SPARSE_SETS_NATIVE=1)."""
    return _knob(monkeypatch, ctx, gsegs, q, "1")


def _off(monkeypatch, ctx, gsegs, q):
    return _knob(monkeypatch, ctx, gsegs, q, "0")


def _flag():
    from pinot_amd import native as N
    assert N.PGX_X_SPARSE_GROUP_SETS == 0x10
    return N.PGX_X_SPARSE_GROUP_SETS


@pytest.mark.parametrize("ki", range(len(KEYS)))
@pytest.mark.parametrize("fi", range(len(FILTERS)))
def test_mixed_functions_at_the_abi_equal_the_model(env, ki, fi):
    """One query with both forms of all three families beside SUM and COUNT; without the flag it is refused."""
    from pinot_amd import native as N
    ctx, gsegs, raws = env
    where, pred = FILTERS[fi]
    masks = [pred(r) for r in raws]
    q = _request(LIB_FNS, KEYS[ki], where)
    assert _status(lambda: _native(ctx, gsegs, q, 0))[0] == N.PGX_ERR_UNSUPPORTED
    blk = _native(ctx, gsegs, q, _flag())
    got = blk.get_aggregation_group_by_result().as_map()
    _check_model(got, _model(raws, masks, KEYS[ki], LIB_FNS), LIB_FNS)
    assert len(got) > (1000, 1000, 400)[fi]  # (the third filter selects a tenth of the 5,501 rows)
    docs = int(sum(m.sum() for m in masks))
    st = blk.stats.as_list()
    assert st[0] == docs and st[3] == sum(SIZES)


@pytest.mark.parametrize("ai", range(len(ALONE)))
def test_each_function_alone(env, ai):
    ctx, gsegs, raws = env
    where, pred = FILTERS[1]
    masks = [pred(r) for r in raws]
    for gcols in KEYS:
        q = _request(ALONE[ai], gcols, where)
        got = _native(ctx, gsegs, q, _flag()).get_aggregation_group_by_result().as_map()
        _check_model(got, _model(raws, masks, gcols, ALONE[ai]), ALONE[ai])


def test_forced_hash_on_a_small_key_space(env):
    """GROUP BY g1 (50 slots) with PGX_X_FORCE_HASH: refused without the flag, the sparse route with it; without
    PGX_X_FORCE_HASH the flag changes nothing (the dense route), and all three answers agree with the model."""
    from pinot_amd import native as N
    ctx, gsegs, raws = env
    where, pred = FILTERS[2]
    masks = [pred(r) for r in raws]
    q = _request(LIB_FNS, ("g1",), where)
    assert _status(lambda: _native(ctx, gsegs, q, N.PGX_X_FORCE_HASH))[0] == N.PGX_ERR_UNSUPPORTED
    model = _model(raws, masks, ("g1",), LIB_FNS)
    for flags in (N.PGX_X_FORCE_HASH | _flag(), _flag(), 0):
        got = _native(ctx, gsegs, q, flags).get_aggregation_group_by_result().as_map()
        _check_model(got, model, LIB_FNS)
        assert len(got) == 50


@pytest.mark.parametrize("ki", range(len(KEYS)))
@pytest.mark.parametrize("fi", [0, 1])
def test_plan_maker_equals_the_decomposition(env, monkeypatch, ki, fi):
    """Through the plan maker the request gives the same blocks with the sparse route (PGX_SPARSE_SETS_NATIVE=1) and
    with PGX_SPARSE_SETS_NATIVE=0."""
    ctx, gsegs, raws = env
    fns = PQL_FNS if ki == 0 else "DISTINCTCOUNTHLL(ci), DISTINCTCOUNT(cl), PERCENTILE50(cf), COUNT(*)"
    if ki == 1 and fi == 1:  # the multi-value forms under the two-word key
        fns = "DISTINCTCOUNTHLLMV(ti), DISTINCTCOUNTMV(ts), PERCENTILE50MV(ti), SUM(m)"
    q = pql.compile("SELECT %s FROM t%s GROUP BY %s" % (fns, FILTERS[fi][0], ", ".join(KEYS[ki])))
    on, off = _on(monkeypatch, ctx, gsegs, q), _off(monkeypatch, ctx, gsegs, q)
    assert _same_blocks(on, off, q) > 1000


def test_native_route_is_taken_through_the_plan_maker(env, monkeypatch):
    """The base query of a group-by request carries the flag with PGX_SPARSE_SETS_NATIVE=1, and only then."""
    from pinot_amd import engine as E
    ctx, gsegs, _ = env
    seen = []
    real = E._Query.execute

    def spy(self, segments, flags=0, *a, **k):
        seen.append(flags)
        return real(self, segments, flags, *a, **k)

    monkeypatch.setattr(E._Query, "execute", spy)
    q = pql.compile("SELECT DISTINCTCOUNT(cl), COUNT(*) FROM t WHERE m < 300 GROUP BY ka, kb")
    _on(monkeypatch, ctx, gsegs, q)
    assert seen == [_flag()]  # one library query: no histogram query beside it
    for run in (_off, lambda m, *a: _plan(*a)):  # the knob at 0, and not set at all
        del seen[:]
        run(monkeypatch, ctx, gsegs, q)
        assert seen[0] == 0 and len(seen) > 1 and not any(seen)  # refused, then decomposed


def test_a_filter_that_selects_nothing(env, monkeypatch):
    ctx, gsegs, _ = env
    for gcols in KEYS:
        q = _request(LIB_FNS, gcols, NOTHING[0])
        blk = _native(ctx, gsegs, q, _flag())
        gr = blk.get_aggregation_group_by_result()
        assert (gr.as_map() if gr is not None else {}) == {}
        assert blk.stats.as_list()[0] == 0
    q = pql.compile("SELECT %s FROM t%s GROUP BY ka, kb" % (PQL_FNS, NOTHING[0]))
    assert _same_blocks(_on(monkeypatch, ctx, gsegs, q), _off(monkeypatch, ctx, gsegs, q), q) == 0


def test_async_and_repeated_executions(env):
    from pinot_amd import engine as E
    from pinot_amd import native as N
    ctx, gsegs, raws = env
    L = N.lib()
    for gcols in KEYS:
        q = _request([("distinctcounthll", "ci"), ("distinctcount", "cl"), ("percentile", "cf"), ("count", "*")],
                     gcols, FILTERS[1][0])
        qq = E._Query(ctx, q)
        outs = []
        try:
            for how in ("sync", "sync", "async", "sync"):
                r = qq.execute_async(gsegs, _flag()) if how == "async" else qq.execute(gsegs, _flag())
                try:
                    blk = E.decode_result(qq, r, gsegs, trim=True)
                    m = blk.get_aggregation_group_by_result().as_map()
                    outs.append((blk.stats.as_list(),
                                 {k: (v[0].tobytes(), sorted(v[1]), v[2], v[3]) for k, v in m.items()}))
                finally:
                    L.pgx_result_release(r)
        finally:
            qq.close()
        assert outs[0] == outs[1] == outs[2] == outs[3] and len(outs[0][1]) > 1000


def test_a_key_of_more_than_128_bits_is_refused(env):
    """Ten 13-bit columns: 130 bits.  The refusal that fires is the base query's: a key of more than two 63-bit words
    runs on the generic kernel, which writes no selection bits ("needs the query kernels").  The directory's fields are
    as wide as the base key's, so every key the query kernels take (126 bits) fits the directory's 128, and the
    runner's own check of the layout is a guard no query reaches (tests/host/sel_key_host_check.cpp and
    tests/test_sel_dir_ref_cpu.py check the layout's refusal at 129 bits)."""
    from pinot_amd import native as N
    ctx, gsegs, _ = env
    assert 10 * 13 > 128
    q = _request([("distinctcounthll", "ci"), ("count", "*")], WIDE, FILTERS[1][0])
    for flags in (_flag(), 0):
        st, msg = _status(lambda: _native(ctx, gsegs, q, flags))
        assert st == N.PGX_ERR_UNSUPPORTED
    assert "needs the query kernels" in _status(lambda: _native(ctx, gsegs, q, _flag()))[1]


def test_a_64_bit_key_of_all_ones_takes_two_words():
    """Eight group columns of 256 values each: a key of exactly 64 bits, one word.  Row i of the first 256 holds i in
    every column, so row 255's key is ~0, the one-word table's empty slot: the runner gives such a result two key
    words.  With that row filtered out the same query runs with one word.  Both equal the model."""
    from pinot_amd import engine as E
    rng = np.random.default_rng(64)
    n = 700
    gcols = ["k%d" % k for k in range(8)]
    raw = {g: np.concatenate([np.arange(256), rng.integers(0, 256, n - 256)]).astype(np.int32) for g in gcols}
    raw["v"] = rng.integers(0, 90, n).astype(np.int32)
    raw["m"] = np.arange(n, dtype=np.int32)
    ctx = E.Context(0)
    try:
        seg = E.IndexSegment(ctx, S.make_segment("ones", [S.make_column(c, v, data_type="INT") for c, v in raw.items()]))
        fns = [("distinctcounthll", "v"), ("distinctcount", "v"), ("percentile", "v"), ("count", "*")]
        for where, mask in ((" WHERE m <> 255", raw["m"] != 255), ("", np.ones(n, bool))):
            got = _native(ctx, [seg], _request(fns, gcols, where), _flag()).get_aggregation_group_by_result().as_map()
            _check_model(got, _model([raw], [mask], gcols, fns), fns)
            assert ("\t".join(["255"] * 8) in got) == (where == "") and "\t".join(["0"] * 8) in got
    finally:
        ctx.close()


def test_distinct_and_percentile_table_limits_and_the_fallback(env, monkeypatch):
    """GROUP BY w0, w1 makes every selected row a group.  DISTINCTCOUNT(big) needs 62,500 bytes per group, so the
    5,501 groups of the match-all query cross PGX_DISTINCT_MAX_TABLE_BYTES and the 500-odd of `m < 100` do not;
    PERCENTILE(big) needs 4,000,000 bytes per group and crosses its limit with either.  The shapes come from the
    constants; nothing of that size is allocated.  Through the plan maker the refused request is decomposed."""
    from pinot_amd import native as N
    ctx, gsegs, raws = env
    gcols = ("w0", "w1")
    per_group = (BIG_CARD + 31) // 32 * 4
    few = int(sum((r["m"] < 100).sum() for r in raws))
    assert sum(SIZES) * per_group > MAX_TABLE_BYTES > few * per_group and few > 100
    assert few * BIG_CARD * 8 > MAX_TABLE_BYTES
    fns = [("distinctcount", "big"), ("count", "*")]
    st, msg = _status(lambda: _native(ctx, gsegs, _request(fns, gcols, ""), _flag()))
    assert st == N.PGX_ERR_UNSUPPORTED and "PGX_DISTINCT_MAX_TABLE_BYTES" in msg
    masks = [r["m"] < 100 for r in raws]
    got = _native(ctx, gsegs, _request(fns, gcols, " WHERE m < 100"), _flag()).get_aggregation_group_by_result().as_map()
    assert len(got) == few
    for r, m in zip(raws, masks):
        keys = _group_keys(r, gcols)
        for d in np.flatnonzero(m):
            assert got[keys[d]] == [{X.java_hash_code("INT", int(r["big"][d]))}, 1]
    st, msg = _status(lambda: _native(ctx, gsegs, _request([("percentile", "big")], gcols, " WHERE m < 100"), _flag()))
    assert st == N.PGX_ERR_UNSUPPORTED and "PGX_PERCENTILE_MAX_TABLE_BYTES" in msg
    q = pql.compile("SELECT DISTINCTCOUNT(big), COUNT(*) FROM t GROUP BY w0, w1")
    on, off = _on(monkeypatch, ctx, gsegs, q), _off(monkeypatch, ctx, gsegs, q)
    assert _same_blocks(on, off, q) == sum(SIZES)
    mon = on.get_aggregation_group_by_result().as_map()
    r = raws[1]
    assert mon["%d\t%d" % (r["w0"][7], r["w1"][7])] == [{X.java_hash_code("INT", int(r["big"][7]))}, 1]


def test_group_count_and_register_limits(many):
    """Every row of the 140,000 is a group.  All of them: more than PGX_SET_MAX_SPARSE_GROUPS.  The first 90,000:
    three register blocks of 90,000 x 1 KiB cross PGX_HLL_MAX_TABLE_BYTES, two do not."""
    from pinot_amd import native as N
    ctx, segs, raw = many
    few = 90000
    assert MANY > MAX_SPARSE_GROUPS >= few and 3 * few * 256 * 4 > MAX_TABLE_BYTES > 2 * few * 256 * 4

    def req(cols, where):
        q = pql.compile("SELECT COUNT(*) FROM t%s GROUP BY x0, x1" % where)
        return {"aggregations": [{"fn": "distinctcounthll", "column": c} for c in cols] +
                                [{"fn": "count", "column": "*"}], "group_by": q["group_by"], "filter": q.get("filter")}

    st, msg = _status(lambda: _native(ctx, segs, req("ab", ""), _flag()))
    assert st == N.PGX_ERR_UNSUPPORTED and "PGX_SET_MAX_SPARSE_GROUPS" in msg
    st, msg = _status(lambda: _native(ctx, segs, req("abc", " WHERE r < %d" % few), _flag()))
    assert st == N.PGX_ERR_UNSUPPORTED and "PGX_HLL_MAX_TABLE_BYTES" in msg
    assert _status(lambda: _native(ctx, segs, req("ab", " WHERE r < %d" % few), 0))[0] == N.PGX_ERR_UNSUPPORTED
    got = _native(ctx, segs, req("ab", " WHERE r < %d" % few), _flag()).get_aggregation_group_by_result().as_map()
    assert len(got) == few  # more groups than the result kernels take in one stretch (65,536)
    codes = {v: HLL.from_ints({X.java_hash_code("INT", v)}).tobytes() for v in range(200)}
    for d in (0, 1, 65535, 65536, 65537, few - 1):
        k = "%d\t%d" % (raw["x0"][d], raw["x1"][d])
        assert [got[k][0].tobytes(), got[k][1].tobytes(), got[k][2]] == [codes[int(raw["a"][d])],
                                                                        codes[int(raw["b"][d])], 1]
    assert all(v[2] == 1 and v[0].any() for v in got.values())
