"""GPU parity of the query kernels' sparse tile body (pgx_jit.cpp `sparse`): when every filter leaf is a doc mask, a
sub-step decodes and aggregates only the rows whose selection bit is set (pgx_unpack_at at the bit's position), unless
some lane of the wave holds more than K selected rows of it -- then the wave runs the dense row loop for that sub-step.

Every query runs twice, with the default body and under PGX_DEBUG=densebody (the dense row loop only); both answers
equal the CPU oracle bit-exactly (integer sums below 2^53, all four execution statistics) and each other.

The selection column x is built so that single lanes hold exactly 0, 1, K, K + 1 and all of their rows selected, whatever
the kernel's rows per lane (8, 16 or 32) and tile size: every 4096-row boundary (tiles are multiples of 4096 rows)
is followed by 32-row blocks whose first 8 rows hold that many selected rows and whose other rows hold none, then a
block with every row selected; the same blocks end right before the next boundary (a tile's last sub-step).  The
segment's last tile is partial (n = 3 * 65536 + 4321) and starts on such a boundary; its last rows, all selected,
leave the last lane straddling num_docs.  Elsewhere x = 1 in about 4 % of the rows.  Column w is all ones over one
32768-row span and all zeros over the next."""
import ctypes
import glob
import os

import numpy as np
import pytest

from pinot_amd import pql
from tests import helpers as H

pytestmark = pytest.mark.gpu

N1 = 3 * 65536 + 4321
N2 = 70003  # a second, smaller segment with other dictionaries: its last lane straddles num_docs too (70003 % 32 = 19)


def sparse_k():
    from pinot_amd import native
    f = native.lib().pgx_sparse_k
    f.restype = ctypes.c_int
    return int(f())


@pytest.fixture(scope="module")
def ctx():
    from pinot_amd import engine as E
    c = E.Context(0)
    yield c
    c.close()


def _raw(n, seed, K):
    rng = np.random.default_rng(seed)
    x = np.where(rng.random(n) < 0.04, 1, rng.choice([0, 2, 3, 4], n)).astype(np.int32)
    counts = [0, 1, min(K, 8), min(K + 1, 8)]
    blocks = len(counts) + 1
    for b0 in range(0, n, 4096):
        for start in (b0, b0 + 4096 - 32 * blocks):
            for i, c in enumerate(counts + [32]):
                lo = start + 32 * i
                if lo + 32 > n:
                    continue
                x[lo:lo + 32] = 0
                if c == 32:
                    x[lo:lo + 32] = 1
                else:
                    x[lo + rng.permutation(8)[:c]] = 1
    x[n - 40:] = 1
    off = 50 * (seed % 2)  # the second segment's dictionaries differ: group ids are remapped when both run together
    return {"x": x,
            "y": rng.integers(0, 300, n).astype(np.int32),
            "z": rng.integers(0, 10, n).astype(np.int32),
            "w": ((np.arange(n) // 32768) % 2 == 0).astype(np.int32),
            "g3": rng.integers(0, 8, n).astype(np.int32),
            "g7": (rng.integers(0, 100, n) + off).astype(np.int32),
            "g8": rng.integers(0, 200, n).astype(np.int32),
            "g10": (rng.integers(0, 1000, n) + off).astype(np.int32),
            "g13": rng.integers(0, 5000, n).astype(np.int32),
            "g17": rng.integers(0, 100000, n).astype(np.int32),
            "m8": rng.integers(-128, 128, n).astype(np.int32),
            "m16": rng.integers(-30000, 35536, n).astype(np.int32),
            "m20": rng.integers(-(1 << 19), 1 << 19, n).astype(np.int32)}


@pytest.fixture(scope="module")
def segs(ctx):
    from pinot_amd import engine as E
    K = sparse_k()
    assert 1 <= K < 8
    out = []
    for name, n, seed in (("sp1", N1, 20), ("sp2", N2, 21)):
        raw = _raw(n, seed, K)
        seg, oseg = H.build_pair(name, raw, inverted=("x", "y", "z", "w"))
        out.append((E.IndexSegment(ctx, seg), oseg))
    return out


Y32 = ", ".join(str(9 * i + 2) for i in range(32))
F_EQ = "x = 1"
F_NEQ = "x <> 1"
F_PROG = "(x = 1 OR y IN (%s)) AND z <> 3" % Y32
F_TILES = "w = 1"
F_NONE = "y = 123456"
A_PACK = "SELECT SUM(m16) FROM t WHERE %s GROUP BY g7"
A_TWO = "SELECT COUNT(*), SUM(m20), MIN(m20), MAX(m20) FROM t WHERE %s GROUP BY g7"
A_AGG = "SELECT SUM(m8), AVG(m16), MIN(m20), MAX(m8) FROM t WHERE %s"
A_KEY2 = "SELECT SUM(m8) FROM t WHERE %s GROUP BY g3, g13"
A_G17 = "SELECT SUM(m16), COUNT(*) FROM t WHERE %s GROUP BY g17"
A_R8 = "SELECT AVG(m8) FROM t WHERE %s GROUP BY g8"

CASES = [(a, f) for a, f in [
    (A_PACK, F_EQ), (A_TWO, F_EQ), (A_AGG, F_EQ), (A_KEY2, F_EQ), (A_G17, F_EQ), (A_R8, F_EQ),
    (A_PACK, F_NEQ), (A_AGG, F_NEQ), (A_R8, F_NEQ),
    (A_TWO, F_PROG), (A_AGG, F_PROG), (A_KEY2, F_PROG),
    (A_PACK, F_TILES), (A_AGG, F_TILES), (A_TWO, F_TILES),
    (A_PACK, F_NONE), (A_AGG, F_NONE),
]]


def _answer(ctx, gsegs, q):
    from pinot_amd import engine as E
    pm = E.InstancePlanMakerImplV2(ctx)
    if len(gsegs) == 1:
        op = pm.make_inner_segment_plan(gsegs[0], q).run()
        blk = op.next_block()
        st = op.get_execution_statistics().as_list()
    else:
        blk = pm.make_inter_segment_plan(gsegs, q).execute()
        st = None
    if q.get("group_by"):
        m = blk.get_aggregation_group_by_result()
        return (m.as_map() if m is not None else {}), st
    return blk.get_aggregation_result(), st


def _both_bodies(ctx, pairs, text, monkeypatch):
    """The query's answer with the default body and with the dense row loop only; both checked against the oracle."""
    q = pql.compile(text)
    o = H.oracle_answer([p[1] for p in pairs], q, literal=True)
    fns = [a["fn"] for a in q["aggregations"]]
    got = []
    for dense in (False, True):
        if dense:
            monkeypatch.setenv("PGX_DEBUG", "densebody")
        else:
            monkeypatch.delenv("PGX_DEBUG", raising=False)
        res, st = _answer(ctx, [p[0] for p in pairs], pql.compile(text))
        if st is not None:
            assert st == list(o["stats"]), ("densebody" if dense else "default", st, list(o["stats"]))
        if q.get("group_by"):
            assert set(res) == set(o["map"])
            for k, v in o["map"].items():
                H.assert_values_equal(res[k], v, fns)
        else:
            H.assert_values_equal(res, o["results"], fns)
        got.append((res, st))
    assert got[0] == got[1]


def test_c5_style_kernel_has_the_sparse_loop_unless_densebody(ctx, segs, monkeypatch, tmp_path):
    """The generated source of the C5-style shape (one program mask, packed dense LDS group-by of a 10-bit column, SUM
    of a 16-bit one) walks set bits by default and does not under PGX_DEBUG=densebody: a silently disabled path fails
    here.  (First in the file, and the only test of this shape: a kernel compiled earlier is not dumped again.)"""
    text = "SELECT SUM(m16) FROM t WHERE %s GROUP BY g10" % F_PROG
    q = pql.compile(text)
    o = H.oracle_answer([segs[0][1]], q, literal=True)
    found = {}
    for mode in ("default", "densebody"):
        d = tmp_path / mode
        d.mkdir()
        monkeypatch.setenv("PGX_JIT_DUMP", str(d))
        if mode == "densebody":
            monkeypatch.setenv("PGX_DEBUG", "densebody")
        res, st = _answer(ctx, [segs[0][0]], pql.compile(text))
        assert st == list(o["stats"])
        assert set(res) == set(o["map"])
        for k, v in o["map"].items():
            H.assert_values_equal(res[k], v, ["sum"])
        srcs = [open(f).read() for f in glob.glob(os.path.join(str(d), "pgxq_*.hip"))]
        assert srcs, "no kernel was generated for the " + mode + " run"
        found[mode] = [("pgx_unpack_at<" in s and "sel &= sel - 1u;" in s) for s in srcs]
    assert any(found["default"])
    assert not any(found["densebody"])


@pytest.mark.parametrize("agg,flt", CASES)
def test_sparse_and_dense_bodies_match_oracle(ctx, segs, agg, flt, monkeypatch):
    _both_bodies(ctx, segs[:1], agg % flt, monkeypatch)


@pytest.mark.parametrize("flt", ["x = 1 AND w = 1", "x = 1 OR w = 1", "x <> 1 AND w = 1", "x = 1 AND z <> 3"])
@pytest.mark.parametrize("agg", [A_PACK, A_AGG])
def test_separate_mask_leaves(ctx, segs, agg, flt, monkeypatch):
    """No program fusion (PGX_RPROG=off): every bitmap leaf reaches the query kernel as a doc-mask leaf of its own, and
    the selection word is the AND / OR / flip of their words."""
    monkeypatch.setenv("PGX_RPROG", "off")
    _both_bodies(ctx, segs[:1], agg % flt, monkeypatch)


@pytest.mark.parametrize("flt", [F_EQ, F_NEQ, F_PROG])
@pytest.mark.parametrize("agg", [A_PACK, A_TWO, A_AGG])
def test_small_segment_last_lane_straddles_num_docs(ctx, segs, agg, flt, monkeypatch):
    _both_bodies(ctx, segs[1:], agg % flt, monkeypatch)


@pytest.mark.parametrize("flt", [F_EQ, F_PROG])
@pytest.mark.parametrize("agg", [A_PACK, "SELECT COUNT(*), SUM(m16), MAX(m16) FROM t WHERE %s GROUP BY g10, g3"])
def test_two_segments_remapped_group_column(ctx, segs, agg, flt, monkeypatch):
    """Two segments whose g7 / g10 dictionaries differ in one launch: the group ids go through the remap tables."""
    _both_bodies(ctx, segs, agg % flt, monkeypatch)
