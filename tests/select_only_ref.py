"""Reference model of the selection without ORDER BY (MSelectionOnlyOperator; pinot_amd/csrc/pgx_select.hip
pgx_select_first_count / pgx_select_first, pgx_select.cpp run_select's `only` branch) in plain Python: the first-K docs of
a mask, the stripes the kernels split a mask into, the merge without ordering, the oracle's filter iterators pulled a
given number of times, the classes of filter whose numEntriesScannedInFilter has a closed form under that early stop,
and the ctypes prototypes of the two launchers libpgx.so exports.  A helper, not a test: nothing here touches a GPU."""
import ctypes as C

import numpy as np

from oracle import pinot_oracle as O

CHUNK_ROWS = 128         # kSelFirstWords mask words of 32 rows: what one thread loads per step
MAX_WGS = 64             # workgroups per item the launchers take


def first_docs(selected, k):
    """docIds of the first k selected docs, ascending.  selected: bool per doc."""
    return np.flatnonzero(np.asarray(selected, dtype=bool))[:k].astype(np.int64)


def stripes(num_docs, wgs):
    """[(first doc, end doc)] per workgroup: contiguous runs of whole 128-row chunks, ceil(chunks / wgs) each."""
    words = (num_docs + 31) // 32 if num_docs > 0 else 0
    chunks = (words + 3) // 4
    per = -(-chunks // wgs)
    out = []
    for g in range(wgs):
        c0 = min(per * g, chunks)
        c1 = min(c0 + per, chunks)
        out.append((min(c0 * CHUNK_ROWS, max(num_docs, 0)), min(c1 * CHUNK_ROWS, max(num_docs, 0))))
    return out


def stripe_counts(selected, k, wgs):
    """What pgx_select_first_count writes: every stripe's selected rows, saturated at k."""
    sel = np.asarray(selected, dtype=bool)
    return np.array([min(k, int(sel[a:b].sum())) for a, b in stripes(len(sel), wgs)], np.int32)


def merge_unordered(lists, size):
    """SelectionOperatorUtils.mergeWithoutOrdering / reduceWithoutOrdering: the lists in order, their rows in order,
    until `size` rows."""
    out = []
    for lst in lists:
        for row in lst:
            if len(out) >= size:
                return out
            out.append(row)
    return out


def pulled(oseg, tree, p):
    """BReusableFilteredDocIdSetOperator under MSelectionOnlyOperator: next() on the filter's root iterator p times, or
    until its end.  Returns (docIds, numEntriesScannedInFilter at that moment)."""
    s = O.build_filter(oseg, tree)
    it = s.iterator()
    docs = []
    for _ in range(p):
        d = it.next()
        if d == O.EOF:
            break
        docs.append(int(d))
    return docs, int(s.entries())


def _phys(oseg, leaf):
    col = oseg.columns[leaf["column"]]
    if col.has_inverted and leaf["op"] != "RANGE":
        return "sorted" if col.is_sorted else "bitmap"
    return "scan"


def _has_scan(oseg, tree):
    if tree["op"] in ("AND", "OR"):
        return any(_has_scan(oseg, c) for c in tree["children"])
    return _phys(oseg, tree) == "scan"


def classify(tree, oseg):
    """"a" | "b" | "d" | None, by the rule of select_only_class (pgx_select.cpp): no scan leaf; the whole filter one scan
    leaf on a single-value column; a root AND of leaves with at least one sorted / bitmap leaf; anything else."""
    if tree is None or not _has_scan(oseg, tree):
        return "a"
    if tree["op"] not in ("AND", "OR"):
        return None if oseg.columns[tree["column"]].mv_ids is not None else "b"
    if tree["op"] != "AND" or any(c["op"] in ("AND", "OR") for c in tree["children"]):
        return None
    return "d" if any(_phys(oseg, c) != "scan" for c in tree["children"]) else None


def early_entries(cls, docs, p, num_docs, full_entries):
    """numEntriesScannedInFilter after p pulls, in closed form.  docs: the first <= p matching docIds; full_entries: the
    full run's number."""
    if cls == "a":
        return 0
    if cls == "b":
        return docs[p - 1] + 1 if len(docs) >= p else num_docs
    if cls == "d":
        return full_entries
    raise ValueError(cls)


def bind(L):
    """Set the prototypes of the first-K launchers on the loaded libpgx.so; returns (count, first)."""
    ct = L.pgx_launch_select_first_count
    ct.restype = C.c_int
    ct.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    fi = L.pgx_launch_select_first
    fi.restype = C.c_int
    fi.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                   C.c_void_p]
    return ct, fi
