"""Synthetic benchmark segments generated directly in HBM (BASELINE.json configs; SURVEY.md 8d "Configs as concrete
synthetic inputs").  Forward indexes are the v1 fixed-bit bytes produced on the device by pgx_synth_column:

    dictId(row) = splitmix64(column_seed ^ row * 0x9E3779B97F4A7C15) % cardinality

The oracle's C twin (oracle/pinot_oracle_c.c: pgo_synth_fwd) regenerates the identical bytes on the host for the CPU
baseline and for full-size spot checks.  Dictionaries are small and built on the host:
    "ids"    dict[i] = i                                    (dimension columns)
    "metric" dict[i] = 16*i + splitmix64(0xD1C7 ^ i) % 16    (sorted, distinct, in [0, 2^20) for card <= 65536)
    "metric_seg"  the same shape with a per-segment jitter seed: every segment has its own dictionary (c3d)
    "metric_f64_seg"  metric_seg / 8 as a DOUBLE dictionary (exact in binary; c3f)
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, List

import numpy as np

from . import native as N
from .segment import Column, SegmentData, num_bits

M64 = (1 << 64) - 1
TILE_ROWS = 8192


def splitmix64_np(x: np.ndarray) -> np.ndarray:
    x = (x.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def column_seed(cfg_seed: int, seg: int, col: int) -> int:
    return (cfg_seed * 0x100000001B3 + seg * 0x9E3779B1 + col * 0x85EBCA77 + 1) & M64


def make_dictionary(kind: str, card: int, seg: int = 0) -> np.ndarray:
    i = np.arange(card, dtype=np.uint64)
    if kind == "ids":
        return i.astype(np.int64)
    if kind in ("metric", "metric_seg", "metric_f64_seg"):
        salt = np.uint64(0xD1C7 + (0x10001 * (seg + 1) if kind != "metric" else 0))
        with np.errstate(over="ignore"):
            jitter = splitmix64_np(salt ^ i) % np.uint64(16)
        v = (i * np.uint64(16) + jitter).astype(np.int64)
        return v / 8.0 if kind == "metric_f64_seg" else v
    raise ValueError(kind)


@dataclass
class ColSpec:
    name: str
    card: int
    dict_kind: str = "ids"
    inverted: bool = False  # build <col>.bitmap.inv (roaring) for the segment, like a Pinot invertedIndexColumns entry
    paired: bool = False    # value drawn jointly with the workload's other paired columns from `npairs` fixed combos

    @property
    def bits(self):
        return num_bits(self.card)


@dataclass
class Workload:
    name: str
    description: str
    segments: int
    rows: int
    columns: List[ColSpec]
    query: str
    seed: int
    scaling: str  # "weak" (every rank holds `segments` segments) or "strong" (segments sharded over ranks)
    npairs: int = 0


C6_CUT = (10, 40, 160)  # w_i < cut: ~4% of each leaf's dictIds

WORKLOADS: Dict[str, Workload] = {
    "c2": Workload("c2", "BASELINE configs[1]: 1B rows (8 x 125M), 8-bit filter dim + 16-bit metric, "
                   "count(*)+sum(metric) with a 50% range filter, 1 MI355X per 1B rows",
                   8, 125_000_000, [ColSpec("dA", 256), ColSpec("m", 65536, "metric")],
                   "SELECT COUNT(*), SUM(m) FROM T WHERE dA BETWEEN 64 AND 191", 2, "weak"),
    "c3": Workload("c3", "BASELINE configs[2]: 1B rows (8 x 125M), group by g1 (card 10k) x g2 (card 1M) drawn from "
                   "2^24 fixed pairs (high-cardinality LONG_MAP path), sum/min/max(m)",
                   8, 125_000_000, [ColSpec("g1", 10000, paired=True), ColSpec("g2", 1_000_000, paired=True),
                                    ColSpec("m", 65536, "metric")],
                   "SELECT SUM(m), MIN(m), MAX(m) FROM T GROUP BY g1, g2 TOP 10", 3, "weak", npairs=1 << 24),
    # C3 with its own metric dictionary in every segment (SegmentDictionaryCreator builds one per segment): no shared
    # value image, so value records rebased per segment (VERDICT r04 missing #1); same rows, keys and query as C3
    "c3d": Workload("c3d", "C3 (BASELINE configs[2] shape) with an independently generated metric dictionary per "
                    "segment: 1B rows (8 x 125M), group by g1 x g2 (2^24 pairs), sum/min/max(m)",
                    8, 125_000_000, [ColSpec("g1", 10000, paired=True), ColSpec("g2", 1_000_000, paired=True),
                                     ColSpec("m", 65536, "metric_seg")],
                    "SELECT SUM(m), MIN(m), MAX(m) FROM T GROUP BY g1, g2 TOP 10", 3, "weak", npairs=1 << 24),
    # C3 with a DOUBLE metric, its own dictionary in every segment: f64 aggregation of the concatenated dictionaries
    "c3f": Workload("c3f", "C3 (BASELINE configs[2] shape) with a DOUBLE metric (a dictionary per segment): 1B rows "
                    "(8 x 125M), group by g1 x g2 (2^24 pairs), sum/min/max(m)",
                    8, 125_000_000, [ColSpec("g1", 10000, paired=True), ColSpec("g2", 1_000_000, paired=True),
                                     ColSpec("m", 65536, "metric_f64_seg")],
                    "SELECT SUM(m), MIN(m), MAX(m) FROM T GROUP BY g1, g2 TOP 10", 3, "weak", npairs=1 << 24),
    # C3 with two metrics (SUM(m), SUM(m2)): two value columns, the generated hash kernels' shape at C3 cardinality
    "c3m2": Workload("c3m2", "C3 keys with two metric columns: 1B rows (8 x 125M), group by g1 x g2 (2^24 pairs), "
                     "sum(m), sum(m2), max(m)",
                     8, 125_000_000, [ColSpec("g1", 10000, paired=True), ColSpec("g2", 1_000_000, paired=True),
                                      ColSpec("m", 65536, "metric"), ColSpec("m2", 4096, "metric")],
                     "SELECT SUM(m), SUM(m2), MAX(m) FROM T GROUP BY g1, g2 TOP 10", 3, "weak", npairs=1 << 24),
    "c5": Workload("c5", "BASELINE configs[4]: 4096 x 2M rows sharded over the GPUs, (f1 IN 32 ids OR f2=7) AND "
                   "f3<>3, group by gk (card 1000), sum(m)",
                   4096, 2_000_000,
                   [ColSpec("f1", 1000, inverted=True), ColSpec("f2", 100, inverted=True),
                    ColSpec("f3", 10, inverted=True), ColSpec("gk", 1000), ColSpec("m", 65536, "metric")],
                   "SELECT SUM(m) FROM T WHERE (f1 IN (%s) OR f2 = 7) AND f3 <> 3 GROUP BY gk TOP 10"
                   % ",".join(str(v) for v in range(3, 1000, 31)[:32]), 5, "strong"),
    # C6: a query over twelve columns (ten filter leaves): more than the eight columns round 3's query kernels took,
    # the shape that ran on the interpreter kernel before (VERDICT r03 missing #3); not a BASELINE config
    # (an OR of scan leaves: its numEntriesScannedInFilter has a closed form the kernel counts, where an AND of scan
    # leaves needs the statistics automaton, pgx_plan.cpp stats_closed_form)
    "c6": Workload("c6", "12-column scan (ten range leaves ORed over 8/10/12-bit columns, ~34% of rows selected), "
                   "group by gk (card 1000), sum(m): 4 x 125M rows",
                   4, 125_000_000,
                   [ColSpec("w%d" % i, (256, 1000, 4000)[i % 3]) for i in range(10)]
                   + [ColSpec("gk", 1000), ColSpec("m", 65536, "metric")],
                   "SELECT SUM(m) FROM T WHERE " + " OR ".join(
                       "w%d < %d" % (i, C6_CUT[i % 3]) for i in range(10))
                   + " GROUP BY gk TOP 10", 6, "weak"),
    # C7: an ARRAY_MAP group key (five 14-bit columns: 70 bits > 64, DefaultGroupKeyGenerator.java:167-186) over 1024
    # distinct combinations (paired columns), the shape that ran on the interpreter kernel before (VERDICT r03
    # missing #3); not a BASELINE config
    "c7": Workload("c7", "ARRAY_MAP group-by: five 14-bit group columns (70-bit keys, 1024 distinct combinations), "
                   "sum(m) over a 4096-value metric: 4 x 125M rows",
                   4, 125_000_000,
                   [ColSpec("h%d" % i, 16384, paired=True) for i in range(5)] + [ColSpec("m", 4096, "metric")],
                   "SELECT SUM(m) FROM T GROUP BY h0, h1, h2, h3, h4 TOP 10", 7, "weak", npairs=1024),
}


# C4 (BASELINE configs[3]): star-tree segment over 6 dims + 3 metrics, SURVEY 8d's 100M raw rows (same dims, metrics,
# maxLeafRecords and query).  Built on the host by pinot_amd/startree.py (one int64 sort key per row, hash-based
# dictionaries); the GPU parity test uses a 10M-row instance (C4_TEST_ROWS) so the oracle stays quick.
C4_CARDS = [8, 16, 32, 64, 128, 1000]
C4_ROWS = 100_000_000
C4_TEST_ROWS = 10_000_000
C4_QUERY = "SELECT SUM(m1), SUM(m2), SUM(m3) FROM T WHERE d2 = 3 AND d4 IN (1, 2, 3) GROUP BY d1 TOP 10"


def c4_raw_rows(rows: int, seed: int = 4):
    """C4's raw rows: every dimension uniform over its cardinality (independently), metrics uniform in [0, 2^16).
    The rows come out already in the builder's sort order (split order = cardinality descending: d6 .. d1): the
    combined dimension key is drawn as the order statistics of `rows` uniform draws (cumulative exponential gaps), so
    the multiset of rows is distributed exactly as independent draws, and the builder's initial sort of 100M rows is
    a linear pass over sorted input."""
    rng = np.random.default_rng(seed)
    span = 1
    for c in C4_CARDS:
        span *= c
    gaps = rng.exponential(1.0, rows + 1)
    u = np.cumsum(gaps)
    key = np.minimum((u[:rows] * (span / u[rows])).astype(np.int64), span - 1)
    del gaps, u
    dims = {}
    for i, c in enumerate(C4_CARDS):  # d1 (the least significant digit of the sort order) first
        dims["d%d" % (i + 1)] = (key % c).astype(np.int32)
        key //= c
    mets = {"m%d" % (i + 1): rng.integers(0, 1 << 16, rows).astype(np.int32) for i in range(3)}
    return dims, mets


class StarTreeSegments:
    """One C4 star-tree segment staged from host bytes (synthetic, seed 4)."""

    def __init__(self, ctx, rows: int = None, seed: int = 4):
        from . import startree as ST
        from .engine import IndexSegment
        import sys
        import time
        self.rows = rows or C4_ROWS
        t0 = time.time()
        dims, mets = c4_raw_rows(self.rows, seed)
        print("[c4] building the star tree over %d raw rows" % self.rows, file=sys.stderr, flush=True)
        self.seg_data = ST.make_star_tree_segment("c4_0", dims, mets, max_leaf_records=ST.DEFAULT_MAX_LEAF_RECORDS)
        del dims, mets
        print("[c4] built in %.1f s (%d docs); staging" % (time.time() - t0, self.seg_data.total_docs), file=sys.stderr,
              flush=True)
        self.segments = [IndexSegment(ctx, self.seg_data)]
        self.seg_ids = [0]

    def algorithmic_bytes(self, used_columns, dict_columns, docs_scanned: int, nodes_visited: int) -> int:
        """docs scanned x (bits of the columns read)/8 + dictionaries + 28 B per star-tree node."""
        cols = self.seg_data.columns
        b = docs_scanned * sum(cols[c].bits for c in used_columns) // 8
        b += sum(cols[c].cardinality * 4 for c in dict_columns)
        return b + 28 * nodes_visited

    def free(self):
        for s in self.segments:
            s.destroy()
        self.segments = []


# C1 (BASELINE configs[0]): the baseball quick-start shape (baseball.csv is not in the reference tree, so the data is
# synthetic per SURVEY 8d: yearID uniform 1871..2013, playerName 17,000 distinct strings, runs 0..177; seed 1).
C1_ROWS = 100_000
C1_QUERY = "SELECT SUM(runs) FROM T WHERE yearID >= 2000 GROUP BY playerName TOP 10"


class BaseballSegments:
    """One C1 segment built on the host (v1 format) and staged through pgx_segment_stage."""

    def __init__(self, ctx, rows: int = None, seed: int = 1):
        from .engine import IndexSegment
        from .segment import make_column, make_segment
        self.rows = rows or C1_ROWS
        rng = np.random.default_rng(seed)
        names = np.array(["player%05d" % i for i in range(17000)])
        raw = {"yearID": rng.integers(1871, 2014, self.rows).astype(np.int32),
               "playerName": names[rng.integers(0, len(names), self.rows)],
               "runs": rng.integers(0, 178, self.rows).astype(np.int32)}
        self.raw = raw
        self.seg_data = make_segment("baseballStats_0", [make_column(k, v) for k, v in raw.items()])
        self.segments = [IndexSegment(ctx, self.seg_data)]
        self.seg_ids = [0]

    def is_inverted(self, name):
        return False

    def algorithmic_bytes(self, used_columns, dict_columns, bitmap_leaves=()) -> int:
        cols = self.seg_data.columns
        b = sum((self.rows * cols[c].bits + 7) // 8 for c in used_columns)
        return b + sum(cols[c].cardinality * 4 for c in dict_columns)

    def free(self):
        for s in self.segments:
            s.destroy()
        self.segments = []


def padded_fwd_bytes(rows: int, bits: int) -> int:
    tiles = max(1, (rows + TILE_ROWS - 1) // TILE_ROWS)
    return tiles * (TILE_ROWS // 8) * bits + 64


class DeviceSegments:
    """Synthetic segments resident in HBM, staged through the C-ABI (pgx_segment_stage with PGX_MEM_DEVICE)."""

    def __init__(self, ctx, wl: Workload, seg_ids: List[int], rows: int = None, extra=()):
        """extra: further columns (segment.Column with fwd_bytes, e.g. a multi-value column's <col>.mv.fwd) that every
        segment holds with the same content, beside the workload's generated ones."""
        from .engine import IndexSegment
        self.ctx = ctx
        self.wl = wl
        self.rows = rows or wl.rows
        self.seg_ids = list(seg_ids)
        self.buffers = []  # one pointer per (segment, column) forward index
        self.allocs = []   # the device allocations behind them: one per segment
        self.segments = []
        self.inv_offsets = {}
        L = N.lib()
        inv = self._inverted_indexes()  # futures: the host threads build them while this loop generates and stages
        # dictionaries that do not depend on the segment: their bytes made once, one device copy for every staging
        shared_bytes = {}
        shared_dev = {}
        for c in wl.columns:
            if c.dict_kind not in ("metric_seg", "metric_f64_seg"):
                b = make_dictionary(c.dict_kind, c.card).astype(">i4").tobytes()
                p = C.c_void_p()
                N.check(L.pgx_device_alloc(ctx.handle, len(b), C.byref(p)))
                N.check(L.pgx_copy_to_device(ctx.handle, p, b, len(b)))
                shared_bytes[c.name], shared_dev[c.name] = b, p
        extra_dev = {}
        for col in extra:  # one device copy of the index for every staging (staging copies it)
            p = C.c_void_p()
            N.check(L.pgx_device_alloc(ctx.handle, len(col.fwd_bytes), C.byref(p)))
            N.check(L.pgx_copy_to_device(ctx.handle, p, col.fwd_bytes, len(col.fwd_bytes)))
            extra_dev[col.name] = (p, len(col.fwd_bytes))
        for s in self.seg_ids:
            cols = []
            fwd_dev = {}
            # the segment's forward indexes in one allocation (padded_fwd_bytes is a multiple of 64: each stays aligned)
            sizes = [padded_fwd_bytes(self.rows, c.bits) for c in wl.columns]
            base = C.c_void_p()
            N.check(L.pgx_device_alloc(ctx.handle, sum(sizes), C.byref(base)))
            self.allocs.append(base)
            at = base.value
            for ci, c in enumerate(wl.columns):
                nbytes = sizes[ci]
                p = C.c_void_p(at)
                at += nbytes
                self.buffers.append(p)
                if c.paired:  # the pair -> value map is global; the row -> pair draw is per segment
                    N.check(L.pgx_synth_column_paired(ctx.handle, p, self.rows, c.bits, c.card,
                                                      column_seed(wl.seed, 0, ci), column_seed(wl.seed, s, 99),
                                                      wl.npairs))
                else:
                    N.check(L.pgx_synth_column(ctx.handle, p, self.rows, c.bits, c.card,
                                               column_seed(wl.seed, s, ci)))
                fwd_dev[c.name] = (p.value, nbytes)
                f64 = c.dict_kind == "metric_f64_seg"
                dict_bytes = shared_bytes.get(c.name)
                if dict_bytes is None:
                    dict_bytes = make_dictionary(c.dict_kind, c.card, s).astype(">f8" if f64 else ">i4").tobytes()
                inv_bytes = inv.pop((s, ci), None)
                if inv_bytes is not None:
                    inv_bytes = inv_bytes.result()
                    self.inv_offsets[(s, c.name)] = np.frombuffer(inv_bytes, dtype=">u4", count=c.card + 1).astype(
                        np.int64)
                cols.append(Column(c.name, "DOUBLE" if f64 else "INT", "DIMENSION", c.card, c.bits, self.rows, self.rows,
                                   False, inv_bytes is not None, dict_bytes, 8 if f64 else 4, None, None, inv_bytes))
            for col in extra:
                cols.append(col)
                fwd_dev[col.name] = (extra_dev[col.name][0].value, extra_dev[col.name][1])
            seg = SegmentData("%s_%d" % (wl.name, s), self.rows, self.rows, {c.name: c for c in cols})
            self.segments.append(IndexSegment.from_device(ctx, seg, fwd_dev, shared_dev))
            for col in cols:  # staging copied the index; inv_offsets keeps what algorithmic_bytes reads of it
                col.inv_bytes = None
        for p in list(shared_dev.values()) + [p for p, _ in extra_dev.values()]:  # staging copied them
            L.pgx_device_free(ctx.handle, p)

    def _inverted_indexes(self):
        """Roaring inverted indexes of the workload's inverted columns, built on host threads from the same dictIds
        the device generator packs (pgx_synth_dict_ids + pgx_inverted_index_build, both release the GIL): a future per
        (segment, column), submitted in segment order, so the caller stages segment s while later ones are built."""
        from concurrent.futures import ThreadPoolExecutor
        jobs = [(s, ci, c) for s in self.seg_ids for ci, c in enumerate(self.wl.columns) if c.inverted]
        if not jobs:
            return {}
        L = N.lib()

        def build(job):
            s, ci, c = job
            ids = np.empty(self.rows, dtype=np.int32)
            N.check(L.pgx_synth_dict_ids(column_seed(self.wl.seed, s, ci), self.rows, c.card, ids.ctypes.data))
            # one build into a buffer of the format's upper bound: the offsets, per dictId a header and a descriptor
            # per 64k-doc container, and at most 2 bytes per doc (a bitmap container only replaces a longer array)
            cap = 4 * (c.card + 1) + c.card * (8 + 8 * ((self.rows + 65535) >> 16)) + 2 * self.rows
            ln = C.c_uint64()
            buf = bytearray(cap)
            out = (C.c_uint8 * cap).from_buffer(buf)
            N.check(L.pgx_inverted_index_build(ids.ctypes.data, self.rows, c.card, out, cap, C.byref(ln)))
            del out
            if ln.value > cap:
                raise RuntimeError("inverted index of %d bytes over the bound of %d" % (ln.value, cap))
            return bytes(memoryview(buf)[:ln.value])

        ex = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))
        futures = {(s, ci): ex.submit(build, (s, ci, c)) for s, ci, c in jobs}
        ex.shutdown(wait=False)  # the queued builds still run; the threads end after the last one
        return futures

    def is_inverted(self, name: str) -> bool:
        return any(c.name == name and c.inverted for c in self.wl.columns)

    def algorithmic_bytes(self, used_columns: List[str], dict_columns: List[str], bitmap_leaves=()) -> int:
        """per segment, ceil(N*b/8) per distinct column read + the serialized bytes of every roaring bitmap
        a bitmap-index leaf reads (NEQ / NOT_IN read the non-matching ones); plus card*width per dictionary used, ONCE:
        the workload's segments share one dictionary per column, staged once (SharedDict) and read once per query, so
        crediting it per segment would count 1.07 GB at C5 that no kernel reads."""
        per_seg = ("metric_seg", "metric_f64_seg")
        width = {"metric_f64_seg": 8}
        total = sum(c.card * 4 for c in self.wl.columns if c.name in dict_columns and c.dict_kind not in per_seg)
        for s in self.seg_ids:
            total += sum(c.card * width.get(c.dict_kind, 4) for c in self.wl.columns
                         if c.name in dict_columns and c.dict_kind in per_seg)
            for c in self.wl.columns:
                if c.name in used_columns:
                    total += (self.rows * c.bits + 7) // 8
            for leaf, ids in bitmap_leaves:
                off = self.inv_offsets[(s, leaf["column"])]
                sel = np.zeros(len(off) - 1, dtype=bool)
                sel[ids] = True
                if leaf["op"] in ("NEQ", "NOT_IN"):
                    sel = ~sel
                total += int((off[1:] - off[:-1])[sel].sum())
        return total

    def free(self):
        for s in self.segments:
            s.destroy()
        L = N.lib()
        for p in self.allocs:
            L.pgx_device_free(self.ctx.handle, p)
        self.allocs = []
        self.buffers = []
        self.segments = []
