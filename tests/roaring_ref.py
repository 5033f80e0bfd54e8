"""Numpy model of the bitmap inverted-index kernels (pinot_amd/csrc: pgx_roaring_expand, pgx_roaring_program and its
_wide / _seg / _wave forms), the ctypes mirrors of their descriptors (pgx_jit_abi.h JRDesc / JRProg) and the launcher
prototypes.  A test segment is a list of doc arrays, one per bitmap; its .bitmap.inv is assembled here (the big-endian
offset header, then pinot_amd.segment.roaring_serialize of every bitmap), so every container's alignment is known."""
import ctypes as C
import struct

import numpy as np

from pinot_amd.segment import roaring_serialize

MAX_RPROG, MAX_RLEAVES = 24, 8          # PGX_J_MAX_RPROG, PGX_J_MAX_RLEAVES
LEAF, AND, OR, NOT = 0, 1, 2, 3         # RProgOp
CHUNK_WORDS = 2048                      # mask words of one 65536-doc chunk


class JRDesc(C.Structure):
    _fields_ = [("mask", C.c_void_p), ("inv", C.c_void_p), ("ids", C.c_void_p), ("nb", C.c_int), ("nchunks", C.c_int)]


class JRProg(C.Structure):
    _fields_ = [("mask", C.c_void_p), ("nchunks", C.c_int), ("num_docs", C.c_int), ("nops", C.c_int),
                ("op", C.c_int8 * MAX_RPROG), ("arg", C.c_int16 * MAX_RPROG), ("ldesc", C.c_int16 * MAX_RLEAVES)]


assert C.sizeof(JRDesc) == 32 and C.sizeof(JRProg) == 112


def bind(L):
    """(expand, program, wave): expand(descs, npairs, maxchunks, stream); program(progs, descs, nprogs, maxchunks,
    maxleaves, stream) with maxleaves 0 the stack kernel, 1..8 the wide one, -1..-8 the per-segment walk;
    wave(progs, descs, nprogs, maxchunks, nslots, stream)."""
    ex = L.pgx_launch_roaring
    ex.restype = C.c_int
    ex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    pr = L.pgx_launch_roaring_program
    pr.restype = C.c_int
    pr.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    wv = L.pgx_launch_roaring_program_wave
    wv.restype = C.c_int
    wv.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return ex, pr, wv


class Seg:
    """One segment's inverted index: bitmap i holds the docs bitmaps[i] (all below num_docs)."""

    def __init__(self, num_docs, bitmaps):
        self.num_docs = num_docs
        self.nchunks = (num_docs + 65535) >> 16
        self.bitmaps = [np.unique(np.asarray(b, np.int64)) for b in bitmaps]
        assert all(len(b) == 0 or (b[0] >= 0 and b[-1] < num_docs) for b in self.bitmaps)
        blobs = [roaring_serialize(b) for b in self.bitmaps]
        offs = [4 * (len(blobs) + 1)]
        for b in blobs:
            offs.append(offs[-1] + len(b))
        self.offs = offs
        self.inv = struct.pack(">%di" % len(offs), *offs) + b"".join(blobs)

    def containers(self, i):
        """[(key, cardinality, byte offset of the container inside the .bitmap.inv)] of bitmap i."""
        base = self.offs[i]
        n = struct.unpack_from("<i", self.inv, base + 4)[0]
        out = []
        for c in range(n):
            key, cm1 = struct.unpack_from("<HH", self.inv, base + 8 + 4 * c)
            out.append((key, cm1 + 1, base + struct.unpack_from("<i", self.inv, base + 8 + 4 * n + 4 * c)[0]))
        return out

    def leaf_bits(self, ids):
        bits = np.zeros(self.nchunks << 16, bool)
        for i in ids:
            bits[self.bitmaps[i]] = True
        return bits


def pack_bits(bits):
    """bool per doc -> mask words: bit (d & 31) of word d >> 5."""
    return np.packbits(bits, bitorder="little").view(np.uint32)


def is_leaf(t):
    return isinstance(t, (list, tuple))


def wave_slots(prog):
    """Mask slots of the wave kernel for a program: a leaf followed by OR joins the top operand's slot while that
    operand is still an OR of leaves, a leaf followed by NOT, AND is cleared out of it (which ends that state), every
    other leaf takes a new slot.  Guards the slot counts the tests state, which size the kernel's LDS."""
    pure, ns, i = [], 0, 0
    while i < len(prog):
        t = prog[i]
        if is_leaf(t):
            top = bool(pure) and pure[-1]
            if top and i + 1 < len(prog) and prog[i + 1] == OR:
                i += 1
            elif top and i + 2 < len(prog) and prog[i + 1] == NOT and prog[i + 2] == AND:
                pure[-1] = False
                i += 2
            else:
                pure.append(True)
                ns += 1
        elif t == NOT:
            pure[-1] = False
        else:
            pure.pop()
            pure[-1] = False
        i += 1
    return ns


def evaluate(seg, prog):
    """The mask words of a postfix program over seg: a list whose items are a leaf (a list of bitmap ids; empty: the
    empty leaf) or AND / OR / NOT.  NOT flips inside [0, num_docs)."""
    inside = np.arange(seg.nchunks << 16) < seg.num_docs
    st = []
    for t in prog:
        if is_leaf(t):
            st.append(seg.leaf_bits(t))
        elif t == NOT:
            st.append(~st.pop() & inside)
        else:
            b, a = st.pop(), st.pop()
            st.append(a & b if t == AND else a | b)
    assert len(st) == 1
    return pack_bits(st[0])
