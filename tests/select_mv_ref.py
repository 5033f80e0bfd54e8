"""Reference model of the multi-value selection kernels (pinot_amd/csrc/pgx_select.hip: pgx_select_mv_offsets,
pgx_select_mv_bases, pgx_select_mv_gather) in plain numpy, the value stream they read, and the descriptor struct and
ctypes prototypes of the three launchers libpgx.so exports.  A helper, not a test: nothing here touches a GPU
(tests/test_select_mv_cpu.py checks the model against a per-doc brute force, tests/test_gpu_select_mv_kernels.py the
kernels against the model).

A launch runs over the pairs (multi-value column m, item i), pair m * nitems + i; item i's docs are docs[i][:counts[i]]
(its ranks at or past the count hold anything and are never read)."""
import ctypes as C

import numpy as np

from tests import select_ref as R

MAX_ROWS = R.MAX_ROWS
INVALID_VALUE = R.INVALID_VALUE


def pack_values(values, bits):
    """The staged value stream of a multi-value column: MSB-first big-endian, values back to back, zero-padded past
    the last value (the kernels' reader always loads two dwords).  Returns uint8."""
    return R.pack_fwd(np.asarray(values, dtype=np.uint64), bits)


def starts_of(lengths):
    """mv_start of a column whose doc d has lengths[d] values: num_docs + 1 int32."""
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int32)


def mv_model(cols, docs, counts, k):
    """cols[m][i] = (start, values) of multi-value column m in item i -> (rel_off (pairs, k + 1) int32, totals (pairs,)
    int32, bases (pairs + 1,) int64, values (grand total,) int32) as the three kernels write them."""
    nmv, ni = len(cols), len(docs)
    rel = np.zeros((nmv * ni, k + 1), np.int32)
    for m in range(nmv):
        for i in range(ni):
            start = np.asarray(cols[m][i][0], dtype=np.int64)
            d = np.asarray(docs[i][:counts[i]], dtype=np.int64)
            ln = np.zeros(k, np.int64)
            ln[:counts[i]] = start[d + 1] - start[d]
            rel[m * ni + i, 1:] = np.cumsum(ln)
    totals = rel[:, k].copy()
    bases = np.concatenate([[0], np.cumsum(totals.astype(np.int64))]).astype(np.int64)
    values = np.zeros(int(bases[-1]), np.int32)
    for m in range(nmv):
        for i in range(ni):
            p = m * ni + i
            start, vals = cols[m][i]
            d = np.asarray(docs[i][:counts[i]], dtype=np.int64)
            ln = np.diff(rel[p, :counts[i] + 1].astype(np.int64))
            # value j of the pair lies at start[doc of its rank] + (j - rel[rank])
            pos = np.repeat(np.asarray(start, dtype=np.int64)[d] - rel[p, :counts[i]], ln) + np.arange(int(totals[p]))
            values[bases[p]:bases[p + 1]] = np.asarray(vals, dtype=np.uint64)[pos].astype(np.uint32).view(np.int32)
    return rel, totals, bases, values


def brute_force(cols, docs, counts):
    """Per pair and doc, the doc's values in its own order: [[list of value arrays per row] per pair]."""
    out = []
    for m in range(len(cols)):
        for i in range(len(docs)):
            start, vals = cols[m][i]
            out.append([np.asarray(vals[start[d]:start[d + 1]], dtype=np.uint64).astype(np.uint32).view(np.int32)
                        for d in docs[i][:counts[i]]])
    return out


class SelMvCol(C.Structure):
    _fields_ = [("values", C.c_void_p), ("start", C.c_void_p), ("bits", C.c_int32), ("pad", C.c_int32)]


def bind(L):
    """Set the prototypes of the multi-value selection launchers on the loaded libpgx.so; returns (offsets, bases,
    gather)."""
    of = L.pgx_launch_select_mv_offsets
    of.restype = C.c_int
    of.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ba = L.pgx_launch_select_mv_bases
    ba.restype = C.c_int
    ba.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    ga = L.pgx_launch_select_mv_gather
    ga.restype = C.c_int
    ga.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_int64, C.c_void_p]
    return of, ba, ga
