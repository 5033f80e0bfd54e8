"""Reference model of the combine-stage kernels (pinot_amd/csrc/pgx_trim.hip, pgx_merge.hip) in plain numpy and Python
integers: the trim key of every TrimKind, the top-k selection with its threshold / tie / candidate accounting, the
TrimState layout, merge_mix and a home-slot search, and the plain versions of the merge, join, pack and dense reduce.
Also the ctypes prototypes of the launchers libpgx.so exports for these kernels, and the generators of the trim cases
the GPU tests run.  A helper, not a test: nothing here touches a GPU (tests/test_combine_ref.py checks the model and
the generators' premises, tests/test_gpu_combine_kernels.py the kernels against the model)."""
import collections
import ctypes as C
import math
import types
import zlib

import numpy as np

from tests.narrow_ref import INVALID_VALUE, M64, SIGN, ordered_f64  # noqa: F401  (re-exported)

# ---------------------------------------------------------------------------------------------------------------------
# constants of pgx_trim.hip / pgx_merge.hip
# ---------------------------------------------------------------------------------------------------------------------
TK_COUNT, TK_SUM, TK_MIN, TK_MAX, TK_AVG, TK_SUMF, TK_AVGF = range(7)
DIGIT = 11               # kTrimDigit
BINS = 1 << DIGIT        # kTrimBins
PASSES = 6               # kTrimPasses
MAX_FNS = 8              # kTrimMaxFns
TIE_CAP = 2048           # kTieCap
CAND_LDS = 2048          # kCandLds
CAND_FLUSH = CAND_LDS - 256   # a workgroup's LDS list is flushed mid-range once it holds more than this
EMPTY = M64              # kMergeEmpty
COMPACT_TILE = 4096      # slots per workgroup tile of pgx_group_compact
OP_ADD, OP_ADDF, OP_MIN, OP_MAX = range(4)   # PlaneOp

# TrimState field offsets (documented in pgx_trim.hip, written by pgx_result::device_trim)
ST_PREFIX, ST_MASK, ST_K, ST_SHIFT, ST_DONE, ST_NSEL, ST_NTIE, ST_KMIN, ST_KMAX, ST_HIST = 0, 8, 16, 24, 28, 32, 40, \
    48, 56, 64
ST_NCAND = ST_HIST + 4 * BINS
STATE_BYTES = ST_NCAND + 8


# ---------------------------------------------------------------------------------------------------------------------
# ctypes prototypes
# ---------------------------------------------------------------------------------------------------------------------
def bind(L):
    """Set the prototypes of the combine-stage launchers on the loaded libpgx.so; returns them as a namespace.  Also
    asserts pgx_trim_state_bytes() against the layout above."""
    P, I, I64, U64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64

    def proto(name, args, res=C.c_int):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
        return f

    ns = types.SimpleNamespace(
        trim=proto("pgx_launch_trim", [P, I64, I64, P, P, I, P, P, P, I64, I, P, P, P, I64, P]),
        state_bytes=proto("pgx_trim_state_bytes", [], C.c_size_t),
        gather=proto("pgx_launch_group_gather", [P, P, I64, I, P, I64, P, P]),
        merge=proto("pgx_launch_group_merge", [P, P, I64, I64, I64, P, P, U64, I, U64, P, P]),
        compact=proto("pgx_launch_group_compact", [P, P, U64, I, P, P, I64, P, P]),
        join=proto("pgx_launch_join", [P, I64, P, P, I64, I64, P, P, U64, P, I64, I, P, P]),
        pack=proto("pgx_launch_group_pack", [P, P, I64, I64, I, P, P]),
        gather_keys=proto("pgx_launch_gather_keys", [P, P, P, I64, I, P, P]),
        dense_reduce=proto("pgx_launch_dense_reduce", [P, P, U64, I, U64, P]))
    assert ns.state_bytes() == STATE_BYTES, (ns.state_bytes(), STATE_BYTES)
    return ns


# ---------------------------------------------------------------------------------------------------------------------
# TrimState images
# ---------------------------------------------------------------------------------------------------------------------
def state_init(nf, k):
    """The nf state blocks as the caller prepares them: k = groups wanted, kmin = all ones, the rest zero."""
    img = np.zeros(nf * STATE_BYTES, dtype=np.uint8)
    for f in range(nf):
        img[f * STATE_BYTES + ST_K:f * STATE_BYTES + ST_K + 8] = np.array([k], dtype=np.int64).view(np.uint8)
        img[f * STATE_BYTES + ST_KMIN:f * STATE_BYTES + ST_KMIN + 8] = 0xFF
    return img


def state_read(img, f):
    """Fields of function slot f of a state image (uint8 array) as Python ints; hist as a uint32 array."""
    b = np.ascontiguousarray(img[f * STATE_BYTES:(f + 1) * STATE_BYTES])

    def u64(o):
        return int(b[o:o + 8].view(np.uint64)[0])

    def i32(o):
        return int(b[o:o + 4].view(np.int32)[0])

    return dict(prefix=u64(ST_PREFIX), mask=u64(ST_MASK), k=int(b[ST_K:ST_K + 8].view(np.int64)[0]),
                shift=i32(ST_SHIFT), done=i32(ST_DONE), n_sel=u64(ST_NSEL), n_tie=u64(ST_NTIE), kmin=u64(ST_KMIN),
                kmax=u64(ST_KMAX), hist=b[ST_HIST:ST_NCAND].view(np.uint32).copy(), n_cand=u64(ST_NCAND))


# ---------------------------------------------------------------------------------------------------------------------
# trim keys
# ---------------------------------------------------------------------------------------------------------------------
def ordered_f64_bits(b):
    """Vectorised narrow_ref.ordered_f64 on the doubles' bits (uint64 array)."""
    b = np.asarray(b, dtype=np.uint64)
    return np.where(b & np.uint64(SIGN), ~b, b | np.uint64(SIGN))


def ordered_f64_inv(key):
    """Bits of the double whose ordered key is `key` (uint64 array)."""
    key = np.asarray(key, dtype=np.uint64)
    return np.where(key & np.uint64(SIGN), key & np.uint64(SIGN - 1), ~key)


def trim_key(kind, count, value):
    """trim_key of pgx_trim.hip for every group: count = plane 0, value = the function's value plane (uint64 arrays
    of the planes' bits).  Larger key = better group."""
    count = np.asarray(count, dtype=np.uint64)
    value = np.asarray(value, dtype=np.uint64)
    if kind == TK_COUNT:
        return count.copy()
    if kind == TK_SUM:
        return value ^ np.uint64(SIGN)
    if kind == TK_MIN:
        return ~value
    if kind == TK_MAX:
        return value.copy()
    if kind == TK_SUMF:
        return ordered_f64_bits(value)
    assert kind in (TK_AVG, TK_AVGF), kind
    s = value.view(np.float64) if kind == TK_AVGF else value.view(np.int64).astype(np.float64)
    c = count.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        d = np.where(count != 0, s / np.where(count != 0, c, 1.0), 0.0)
    return ordered_f64_bits(np.ascontiguousarray(d).view(np.uint64))


def value_for_key(kind, key):
    """The value plane bits that give `key` under kind COUNT (the count plane itself) / SUM / MIN / MAX / SUMF."""
    key = np.asarray(key, dtype=np.uint64)
    if kind in (TK_COUNT, TK_MAX):
        return key.copy()
    if kind == TK_SUM:
        return key ^ np.uint64(SIGN)
    if kind == TK_MIN:
        return ~key
    assert kind == TK_SUMF, kind
    return ordered_f64_inv(key)


# ---------------------------------------------------------------------------------------------------------------------
# the selection
# ---------------------------------------------------------------------------------------------------------------------
TrimRef = collections.namedtuple("TrimRef", "thr above n_eq ties kept hb n_cand")


def trim_ref(keys, k, krange=None):
    """Top-k of `keys` (uint64 array), largest first.  thr: the k-th largest key; above: the indices with key > thr;
    n_eq: how many keys equal thr; ties = k - len(above), the threshold ties that are kept; kept: the sorted multiset
    of kept keys.  With fewer than k keys every group is kept and thr is None (above = every index, n_eq = ties = 0).
    hb: the varying bits of min ^ max (of krange = (kmin, kmax) when the launch is seeded with a range).  n_cand: the
    first digit's candidate count: keys >= thr with the bits below max(hb - 11, 0) cleared; 0 when hb <= 11, where the
    threshold is complete after one digit and the candidate kernel returns; None when thr is."""
    keys = np.asarray(keys, dtype=np.uint64)
    n = len(keys)
    if krange is None:
        krange = (int(keys.min()), int(keys.max())) if n else (M64, 0)
    hb = (krange[0] ^ krange[1]).bit_length() if krange[0] <= krange[1] else 0
    if n < k:
        return TrimRef(None, np.arange(n, dtype=np.int64), 0, 0, np.sort(keys), hb, None)
    srt = np.sort(keys)
    thr = int(srt[n - k])
    above = np.flatnonzero(keys > np.uint64(thr)).astype(np.int64)
    n_eq = int((keys == np.uint64(thr)).sum())
    n_cand = 0
    if hb > DIGIT:
        n_cand = int((keys >= np.uint64(thr & ~((1 << (hb - DIGIT)) - 1))).sum())
    return TrimRef(thr, above, n_eq, k - len(above), srt[n - k:], hb, n_cand)


# ---------------------------------------------------------------------------------------------------------------------
# merge_mix and the home-slot search
# ---------------------------------------------------------------------------------------------------------------------
def merge_mix(x):
    x &= M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def merge_mix_np(x):
    x = np.asarray(x, dtype=np.uint64).copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return x


def home_slot(key, cap):
    return merge_mix(key) & (cap - 1)


def keys_homed_at(cap, slot, count, start=1):
    """The first `count` keys >= start (below 2^63) whose home slot in a table of `cap` slots is `slot`."""
    assert cap & (cap - 1) == 0 and 0 <= slot < cap
    found, at, step = [], start, max(65536, 4 * cap)
    while len(found) < count:
        cand = np.arange(at, at + step, dtype=np.uint64)
        hit = cand[(merge_mix_np(cand) & np.uint64(cap - 1)) == np.uint64(slot)]
        found.extend(int(x) for x in hit[:count - len(found)])
        at += step
    assert at < SIGN
    return found


# ---------------------------------------------------------------------------------------------------------------------
# merge, compact, join, pack, dense reduce
# ---------------------------------------------------------------------------------------------------------------------
def ops_pack(ops):
    """PlaneOp per plane -> the launchers' 2-bits-per-plane word."""
    w = 0
    for p, op in enumerate(ops):
        w |= op << (2 * p)
    return w


def table_init(cap, ops):
    """Key and plane arrays of an empty merge table, as merge_device_groups fills them: keys all ones, min planes all
    ones, the others zero."""
    tkey = np.full(cap, EMPTY, dtype=np.uint64)
    tpl = np.zeros((len(ops), cap), dtype=np.uint64)
    for p, op in enumerate(ops):
        if op == OP_MIN:
            tpl[p] = M64
    return tkey, tpl


def _f64(bits):
    return float(np.uint64(bits).view(np.float64))


def _bits(x):
    return int(np.float64(x).view(np.uint64))


def group_merge_ref(keys, planes, ops):
    """key -> list of plane words of the merged groups.  keys: n ints; planes[p][i]: plane p of input i (uint64 bits).
    Integer sums are Python ints mod 2^64, ordered min / max plain unsigned min / max, f64 sums math.fsum (over the
    table's initial 0.0 and the inputs).  Also returns key -> {plane: (sum of |v|, addends)} of the f64 planes, for
    the error bound of a sum taken in another order."""
    by = collections.defaultdict(list)
    for i, k in enumerate(keys):
        by[int(k)].append(i)
    cols = [np.asarray(pl, dtype=np.uint64) for pl in planes]
    out, aux = {}, {}
    for k, ix in by.items():
        row, a = [], {}
        for p, op in enumerate(ops):
            v = [int(x) for x in cols[p][ix]]
            if op == OP_ADD:
                row.append(sum(v) & M64)
            elif op == OP_ADDF:
                f = [_f64(x) for x in v]
                row.append(_bits(math.fsum([0.0] + f)))
                a[p] = (math.fsum(abs(x) for x in f), len(f))
            elif op == OP_MIN:
                row.append(min(v))
            else:
                row.append(max(v))
        out[k], aux[k] = row, a
    return out, aux


def dense_reduce_ref(dst, src, ops):
    """dst op= src, plane by plane: dst, src of shape (nplanes, slots), uint64 bits."""
    dst, src = np.asarray(dst, dtype=np.uint64), np.asarray(src, dtype=np.uint64)
    out = np.empty_like(dst)
    for p, op in enumerate(ops):
        a, b = dst[p], src[p]
        if op == OP_ADD:
            out[p] = a + b
        elif op == OP_ADDF:
            with np.errstate(all="ignore"):
                out[p] = (a.view(np.float64) + b.view(np.float64)).view(np.uint64)
        elif op == OP_MIN:
            out[p] = np.minimum(a, b)
        else:
            out[p] = np.maximum(a, b)
    return out


def pack_ref(okey, opl, n):
    """Records (key, then the planes) of the first n groups: shape (n, 1 + nplanes)."""
    opl = np.asarray(opl, dtype=np.uint64)
    return np.concatenate([np.asarray(okey, dtype=np.uint64)[:n, None], opl[:, :n].T], axis=1)


def join_ref(keys0, keys, opl, comb, base):
    """A later pass's planes 1..3 (opl[p][i] of key keys[i]) written to comb[base .. base + 2] at the index the key
    has in the first pass (keys0); returns (the new comb, misses)."""
    at = {int(k): j for j, k in enumerate(keys0)}
    out = np.array(comb, dtype=np.uint64, copy=True)
    miss = 0
    for i, k in enumerate(keys):
        j = at.get(int(k))
        if j is None:
            miss += 1
            continue
        for p in range(3):
            out[base + p][j] = opl[1 + p][i]
    return out, miss


# ---------------------------------------------------------------------------------------------------------------------
# trim cases of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def keys_with_hb(rng, n, hb):
    """n >= 2 random keys whose smallest and largest differ in exactly the bits [0, hb): a random common part above."""
    assert 1 <= hb <= 64 and n >= 2
    low = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) << np.uint64(1)
    low |= rng.integers(0, 2, size=n, dtype=np.uint64)
    if hb < 64:
        low &= np.uint64((1 << hb) - 1)
        base = (int(rng.integers(1, 1 << 62)) >> hb) << hb  # below 2^62: kinds SUM / MIN keep room either side
        low |= np.uint64(base)
    top = np.uint64(1 << (hb - 1))
    low[0] &= ~top
    low[1] |= top
    return low


def _filler(rng, nplanes, ocap):
    """Planes of random words: what a function does not read must not matter."""
    return rng.integers(0, 1 << 63, size=(nplanes, ocap), dtype=np.uint64)


def _case(oplane, n, kinds, planes, k, grid, cap=None, ccap=0, prange=None, **premise):
    return dict(oplane=oplane, n=n, ocap=oplane.shape[1], kinds=list(kinds), planes=list(planes), k=k, grid=grid,
                cap=k if cap is None else cap, ccap=ccap, prange=prange, premise=premise)


def _one_fn(rng, keys, kind, k, grid, plane=3, nplanes=4, **kw):
    """One function of `kind` whose keys are `keys`, its value in `plane`."""
    n = len(keys)
    op = _filler(rng, nplanes, n + 3)
    op[0 if kind == TK_COUNT else plane, :n] = value_for_key(kind, keys)
    return _case(op, n, [kind], [plane], k, grid, **kw)


def case_seeded(case):
    """Whether the launcher seeds the key ranges from prange: only when every function is COUNT / SUM / MIN / MAX."""
    return case["prange"] is not None and all(k in (TK_COUNT, TK_SUM, TK_MIN, TK_MAX) for k in case["kinds"])


def case_keys(case, f):
    n = case["n"]
    return trim_key(case["kinds"][f], case["oplane"][0, :n], case["oplane"][case["planes"][f], :n])


def case_ref(case, f):
    kr = None
    if case_seeded(case):
        kr = (int(case["prange"][case["kinds"][f]]), int(case["prange"][4 + case["kinds"][f]]))
    return trim_ref(case_keys(case, f), case["k"], kr)


def range_counts(flags, grid):
    """How many of the flagged groups fall in each workgroup's contiguous range (pgx_trim_cand / pgx_trim_select over
    the planes: chunk = ceil(n / grid))."""
    n = len(flags)
    chunk = -(-n // grid) if n else 0
    return [int(flags[g * chunk:(g + 1) * chunk].sum()) for g in range(grid)]


def range_ties(case, f=0):
    keys, ref = case_keys(case, f), case_ref(case, f)
    return range_counts(keys == np.uint64(ref.thr), case["grid"])


def range_cands(case, f=0):
    keys, ref = case_keys(case, f), case_ref(case, f)
    if ref.hb <= DIGIT:
        return [0] * case["grid"]
    return range_counts(keys >= np.uint64(ref.thr & ~((1 << (ref.hb - DIGIT)) - 1)), case["grid"])


def prange_of(case, loose=0):
    """prange of a case: smallest ([kind]) and largest ([4 + kind]) trim key per kind COUNT / SUM / MIN / MAX over
    the case's functions, widened by `loose` either side."""
    pr = np.zeros(8, dtype=np.uint64)
    pr[:4] = M64
    for f, kind in enumerate(case["kinds"]):
        if kind < 4 and case["n"]:
            keys = case_keys(case, f)
            pr[kind] = min(int(pr[kind]), max(int(keys.min()) - loose, 0))
            pr[4 + kind] = max(int(pr[4 + kind]), min(int(keys.max()) + loose, M64))
    return pr


HBS = [1, 5, 11, 12, 22, 23, 34, 45, 56, 63, 64]
COUNT_CASES = sorted({(n, k, g) for n in (0, 1, 255, 256, 257) for k in (1, n - 1, n, n + 5) if k >= 1
                      for g in (1, 4)})


def _tie_case(rng, grid, n, layout, want, ccap=0):
    """layout: per range of ceil(n / grid) groups, how many sit at the threshold key; of the rest, alternately one
    above and one below it.  want: threshold ties to keep."""
    chunk = -(-n // grid)
    thr = (0x1234 << 40) | 0x777
    keys = np.empty(n, dtype=np.uint64)
    for g in range(grid):
        m = min(chunk, n - g * chunk)
        part = np.where(np.arange(m) % 2 == 0, thr + 1 + rng.integers(0, 1 << 30, size=m), thr - 1 - rng.integers(
            0, 1 << 30, size=m)).astype(np.uint64)
        at = rng.permutation(m)[:layout[g]]
        part[at] = thr
        keys[g * chunk:g * chunk + m] = part
    above = int((keys > np.uint64(thr)).sum())
    return _one_fn(rng, keys, TK_MAX, above + want, grid, ccap=ccap, thr=thr, want=want)


def _cand_case(rng, width, which):
    """The candidate-list cases: keys of `width` varying bits (22: two passes, 64: six), n = 20000."""
    n = 20000
    keys = keys_with_hb(rng, n, width)
    if which == "flush":  # one workgroup, more than CAND_FLUSH candidates before its range ends
        c = _one_fn(rng, keys, TK_MAX, 3000, 1, ccap=n)
    else:
        c = _one_fn(rng, keys, TK_MAX, 1000, 8)
        nc = case_ref(c, 0).n_cand
        c["ccap"] = {"none": 0, "all": n, "exact": nc, "short": nc - 1}[which]
    return c


def _avg_planes(rng, n):
    """count, int64 sum: some counts 0, sums of both signs, small ones and ones above 2^53 (inexact as doubles)."""
    count = rng.integers(1, 1000, size=n, dtype=np.uint64)
    count[rng.permutation(n)[:n // 16]] = 0
    s = rng.integers(-(1 << 20), 1 << 20, size=n, dtype=np.int64)
    big = rng.permutation(n)[:n // 4]
    s[big] = rng.integers(-(1 << 62), 1 << 62, size=len(big), dtype=np.int64) | 1
    return count, s.view(np.uint64)


def _f64_values(rng, n):
    """Doubles of both signs over many exponents, with -0.0, +0.0 and subnormals of both signs; no NaN, no inf."""
    v = rng.standard_normal(n) * np.exp2(rng.integers(-300, 300, size=n).astype(np.float64))
    v[0:8] = [-0.0, 0.0, 5e-324, -5e-324, 2.2e-308 / 4, -2.2e-308 / 4, 0.0, -0.0]
    v = v[rng.permutation(n)]
    assert np.isfinite(v).all()
    return np.ascontiguousarray(v).view(np.uint64)


def _side_by_side(rng, n, k, grid, kinds, **kw):
    """Functions over three value columns (planes 1 + 3c + r: sum / min / max of column c): columns 0 and 2 int64,
    column 1 f64.  kinds: list of (TrimKind, column)."""
    op = _filler(rng, 10, n + 3)
    op[0, :n], op[1, :n] = _avg_planes(rng, n)
    op[4, :n] = _f64_values(rng, n)
    op[7, :n] = rng.integers(-(1 << 40), 1 << 40, size=n, dtype=np.int64).view(np.uint64)
    role = {TK_SUM: 0, TK_AVG: 0, TK_SUMF: 0, TK_AVGF: 0, TK_MIN: 1, TK_MAX: 2, TK_COUNT: 0}
    return _case(op, n, [kd for kd, _ in kinds], [1 + 3 * c + role[kd] for kd, c in kinds], k, grid, **kw)


def trim_case(name, seed=0):
    """Build the named trim case: dict(oplane (nplanes, ocap), n, ocap, kinds, planes, k, grid, cap, ccap, prange,
    premise)."""
    rng = np.random.default_rng([seed, zlib.crc32(name.encode())])
    part = name.split("_")
    if part[0] == "hb":  # key width: TK_MAX keys with exactly hb varying bits
        return _one_fn(rng, keys_with_hb(rng, 20000, int(part[1])), TK_MAX, 1000, 8, ccap=20000, hb=int(part[1]))
    if name == "sum_signed":  # sums of both signs: SUM keys vary in all 64 bits
        s = rng.integers(-(1 << 62), 1 << 62, size=20000, dtype=np.int64)
        return _one_fn(rng, s.view(np.uint64) ^ np.uint64(SIGN), TK_SUM, 1000, 8, plane=1, ccap=20000, hb=64)
    if part[0] == "kind":
        n, k, grid = 5000, 700, 5
        kind = int(part[1])
        if kind == TK_COUNT:
            return _one_fn(rng, rng.integers(0, 1 << 20, size=n, dtype=np.uint64), kind, k, grid, ccap=n)
        if kind in (TK_SUM, TK_MIN, TK_MAX):  # the second value column's planes (1 + 3 + r)
            v = rng.integers(-(1 << 45), 1 << 45, size=n, dtype=np.int64).view(np.uint64)  # both signs
            keys = trim_key(kind, v, v if kind == TK_SUM else v ^ np.uint64(SIGN))  # MIN / MAX planes: ordered int64
            return _one_fn(rng, keys, kind, k, grid, plane=3 + kind, nplanes=7, ccap=n)
        if kind == TK_SUMF:
            return _one_fn(rng, ordered_f64_bits(_f64_values(rng, n)), kind, k, grid, plane=4, nplanes=7, ccap=n)
        op = _filler(rng, 7, n + 3)
        if kind == TK_AVG:
            op[0, :n], op[4, :n] = _avg_planes(rng, n)
        else:
            op[0, :n] = _avg_planes(rng, n)[0]
            op[4, :n] = _f64_values(rng, n)
        return _case(op, n, [kind], [4], k, grid, ccap=n)
    if name == "all_equal":
        return _one_fn(rng, np.full(5000, 0xABCDEF0123, dtype=np.uint64), TK_MAX, 1000, 4, ccap=5000)
    if part[0] == "two":  # two distinct keys, 3000 of the upper one: k inside the upper / the lower
        keys = np.where(rng.permutation(5000) < 3000, (7 << 33) | 5, (7 << 33) | 2).astype(np.uint64)
        return _one_fn(rng, keys, TK_MAX, {"upper": 1200, "lower": 3700}[part[2]], 4, ccap=5000)
    if part[0] == "tiecap":  # more threshold ties in one workgroup's range than the LDS tie list holds
        return {"g1": lambda: _tie_case(rng, 1, 6000, [5000], 2500),
                "g1w": lambda: _tie_case(rng, 1, 6000, [5000], 3500),
                "g1c": lambda: _tie_case(rng, 1, 6000, [5000], 2500, ccap=6000),
                "g3": lambda: _tie_case(rng, 3, 18000, [0, 5000, 0], 2500),
                "g3w": lambda: _tie_case(rng, 3, 18000, [0, 5000, 0], 3500),
                "g3s": lambda: _tie_case(rng, 3, 18000, [1000, 3500, 500], 3000)}[part[1]]()
    if part[0] == "cand":
        return _cand_case(rng, int(part[1][1:]), part[2])
    if part[0] == "cnt":
        n, k, grid = int(part[1][1:]), int(part[2][1:]), int(part[3][1:])
        keys = rng.integers(0, 1 << 40, size=n, dtype=np.uint64)
        return _one_fn(rng, keys, TK_MAX, k, grid, ccap=max(n, 1))
    mixed = [(TK_COUNT, 0), (TK_SUM, 0), (TK_MIN, 0), (TK_MAX, 2), (TK_AVG, 0), (TK_SUMF, 1), (TK_AVGF, 1), (TK_SUM, 2)]
    if name == "nf8":  # cap > k: the strip stride, not the number wanted
        return _side_by_side(rng, 3000, 400, 4, mixed, cap=437, ccap=3000)
    if name == "nf1":
        return _side_by_side(rng, 3000, 400, 4, mixed[3:4], cap=437, ccap=3000)
    if part[0] == "seed":
        rng = np.random.default_rng([seed, zlib.crc32(b"seed")])  # the same planes in all four
        ints = [(TK_COUNT, 0), (TK_SUM, 0), (TK_MIN, 0), (TK_MAX, 2)]
        if part[1] == "poison":  # one AVG function: the launcher must take the range pass and never read prange
            c = _side_by_side(rng, 3000, 400, 4, ints + [(TK_AVG, 0)], ccap=3000)
            c["prange"] = prange_of(c)
            c["prange"][4:] = c["prange"][:4]  # "every key equal to the smallest": a wrong threshold if read
            return c
        c = _side_by_side(rng, 3000, 400, 4, ints, ccap=3000)
        c["prange"] = {"exact": lambda: prange_of(c), "loose": lambda: prange_of(c, loose=12345),
                       "null": lambda: None}[part[1]]()
        return c
    raise KeyError(name)


TRIM_CASES = (["hb_%d" % hb for hb in HBS] + ["sum_signed"] + ["kind_%d" % kd for kd in range(7)]
              + ["all_equal", "two_keys_upper", "two_keys_lower"]
              + ["tiecap_" + v for v in ("g1", "g1w", "g1c", "g3", "g3w", "g3s")]
              + ["cand_w%d_%s" % (w, v) for w in (22, 64) for v in ("none", "all", "exact", "short", "flush")]
              + ["cnt_n%d_k%d_g%d" % c for c in COUNT_CASES]
              + ["nf8", "nf1", "seed_exact", "seed_loose", "seed_poison", "seed_null"])
