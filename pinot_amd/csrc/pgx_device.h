// Device primitives every kernel of the library shares, the library's own (.hip files and device headers include this
// file) and the query kernels generated at run time (pasted after pgx_jit_abi.h, in front of pgx_roaring_device.h and
// pgx_jit_device.h).  Builtin types only, no includes.  One definition each of: the typedef prelude and the global
// address space, the LDS-only barriers, the fixed-bit forward-index readers, the group keys' hash, the global group
// hash table, and the plane encodings and ops.  Atomics are the __hip_atomic_* builtins: they take pointers of either
// address space (the atomicCAS / atomicAdd overloads reject an address_space(1) pointer in the host pass).
#ifndef PGX_DEVICE_H_
#define PGX_DEVICE_H_

typedef unsigned int u32;
typedef unsigned long long u64;
typedef long long i64;
typedef u32 pgx_u32x4 __attribute__((ext_vector_type(4)));
typedef u32 pgx_u32x2 __attribute__((ext_vector_type(2)));
// Global (HBM) address space: pointers read out of the argument block are generic, and generic (flat) loads share
// the LDS wait counter, which would make every LDS read wait for the next tile's prefetch (and would serialise the
// roaring loads with the mask atomics).
#define PGX_G __attribute__((address_space(1)))

// LDS hand-off between the lanes of ONE wave (no workgroup barrier).
__device__ __forceinline__ void pgx_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Workgroup barrier for LDS hand-offs only: waits for this wave's LDS operations (lgkmcnt), not for its outstanding
// global loads or stores, so a prefetch (the next tile's forward index, the next container's fields) and the previous
// chunk's mask stores stay in flight across it (__syncthreads drains vmcnt).  Global memory is never communicated
// between the workgroup's threads where it is used.
__device__ __forceinline__ void pgx_lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// ---------------------------------------------------------------------------------------------------------------------
// Forward index (util/PinotDataCustomBitSet.java:122-155): row r of a B-bit column occupies bits [r*B, r*B+B) of a
// big-endian, MSB-first bit stream.
// ---------------------------------------------------------------------------------------------------------------------
// One row.  The second dword is read only when the row reaches into it (it may lie past the index).
__device__ __forceinline__ u32 pgx_fwd_value(const u32* __restrict__ fwd, int row, int bits) {
  const i64 o = (i64)row * bits;
  const PGX_G u32* w = (const PGX_G u32*)fwd + (o >> 5);
  const int s = (int)(o & 31);
  const u32 mask = bits == 32 ? 0xFFFFFFFFu : ((1u << bits) - 1u);
  const u32 hi = __builtin_bswap32(w[0]);
  if (s + bits <= 32) return (hi >> (32 - s - bits)) & mask;
  const u64 x = ((u64)hi << 32) | __builtin_bswap32(w[1]);
  return (u32)(x >> (64 - s - bits)) & mask;
}
// The same without a branch: both dwords are always read.  For rows inside the padded index only (single-value
// columns: whole tiles plus 64 bytes; the staged multi-value stream is padded past its last value), where the second
// dword of the last row is still inside.  1 <= bits <= 32.  The multi-value stream is indexed in 64 bits.
// MASKED chooses between the two forms the kernels had, the same value either way, because each costs one family:
//   false  a generic pointer and (x << s) >> (64 - bits): two 64-bit shifts, the second by a loop invariant.  With it
//          pgx_mv_group takes 152 VGPRs instead of 124 and pgx_mv_group_ordered 135 instead of 104, a wave per SIMD
//          less each.
//   true   a PGX_G pointer, shift right and mask: a subtraction and an AND more per row.  With it pgx_distinct_mark_mv
//          ran 6.4 % and 3.1 % slower (tools/bench_distinct.py, set mv, match_all and f < 10; the parent's spread 1.2 %
//          and 0.4 %), and with the PGX_G pointer alone still 2.7 % and 3.4 % (spread 2.6 % and 0.0 %).
// So the multi-value kernels of pgx_kernels.hip take MASKED, the walks over the selection bits do not.
template <bool MASKED = false>
__device__ __forceinline__ u32 pgx_fwd_value2(const u32* __restrict__ fwd, i64 row, int bits) {
  const i64 o = row * bits;
  const int s = (int)(o & 31);
  if constexpr (MASKED) {
    const PGX_G u32* w = (const PGX_G u32*)fwd + (o >> 5);
    const u64 x = ((u64)__builtin_bswap32(w[0]) << 32) | __builtin_bswap32(w[1]);
    return (u32)(x >> (64 - s - bits)) & (0xFFFFFFFFu >> (32 - bits));
  } else {
    const u32* w = fwd + (o >> 5);
    const u64 x = ((u64)__builtin_bswap32(w[0]) << 32) | __builtin_bswap32(w[1]);
    return (u32)((x << s) >> (64 - bits));
  }
}

// The 32 dictIds of one mask word's rows (rows 32 * word ...): exactly B dwords, every one read once (streaming) with
// the widest loads the dword count allows, without their natural alignment (the hardware runs in unaligned mode: right
// at every dword address), then constant-shift extraction.
template <int B>
__device__ __forceinline__ void pgx_fwd_decode32(const u32* __restrict__ gp, u32 (&v)[32]) {
  const PGX_G u32* p = (const PGX_G u32*)gp;
  u32 w[B + 1];
#pragma unroll
  for (int i = 0; i < B / 4; ++i) {
    const pgx_u32x4 q = __builtin_nontemporal_load((const PGX_G pgx_u32x4*)(p + 4 * i));
    w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
  }
  constexpr int r = B % 4, b = B - r;
  if constexpr (r >= 2) {
    const pgx_u32x2 q = __builtin_nontemporal_load((const PGX_G pgx_u32x2*)(p + b));
    w[b] = q.x; w[b + 1] = q.y;
  }
  if constexpr (r % 2 == 1) w[B - 1] = __builtin_nontemporal_load(p + B - 1);
#pragma unroll
  for (int i = 0; i < B; ++i) w[i] = __builtin_bswap32(w[i]);
  w[B] = 0;
  constexpr u32 MASK = (B == 32) ? 0xFFFFFFFFu : ((1u << (B & 31)) - 1u);
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int o = j * B, k = o >> 5, sh = o & 31;
    if (sh + B <= 32) {
      v[j] = (w[k] >> (32 - sh - B)) & MASK;
    } else {
      const u64 win = ((u64)w[k] << 32) | w[k + 1];
      v[j] = (u32)(win >> (64 - sh - B)) & MASK;
    }
  }
}

#define PGX_FWD_WIDTHS(X) \
  X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) \
  X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)

// mask word `word` of a column whose width is known at run time only (a width out of range: all zero)
__device__ __forceinline__ void pgx_fwd_decode_word(int bits, const u32* __restrict__ fwd, i64 word, u32 (&v)[32]) {
  const u32* p = fwd + word * bits;
  switch (bits) {
#define PGX_FWD_CASE(b)        \
  case b:                      \
    pgx_fwd_decode32<b>(p, v); \
    break;
    PGX_FWD_WIDTHS(PGX_FWD_CASE)
#undef PGX_FWD_CASE
    default:
#pragma unroll
      for (int j = 0; j < 32; ++j) v[j] = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Group keys of W 64-bit words (LONG_MAP / ARRAY_MAP keys, DefaultGroupKeyGenerator.java:239-246 / :268-608) and the
// global hash table they live in: open addressing, linear probing, cap a power of two, W words per slot in `keys`
// (empty: ~0; the packed key words keep <= 63 bits).  The table of a query is filled by the interpreter kernel, by the
// generated kernels' flush and by the multi-value kernels alike, and read back by pgx_find: one hash, one protocol.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 pgx_mix64(u64 x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
// the hash whose low bits are the key's home slot
template <int W>
__device__ __forceinline__ u64 pgx_key_hash(const u64 (&k)[W]) {
  if constexpr (W == 1) {
    return pgx_mix64(k[0]);
  } else if constexpr (W == 2) {
    return pgx_mix64(k[0] ^ pgx_mix64(k[1]));
  } else {
    u64 hv = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) hv = pgx_mix64(hv ^ k[w]);
    return hv;
  }
}

#define PGX_RELAXED_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// The slot of key k, claimed if the table does not hold it yet; -1 after min(cap, max_probes) occupied slots.  W = 1: a
// compare-and-swap on the key itself.  W >= 2: a state word per slot (0 empty, 1 being written, 2 published), and every
// loop iteration makes progress for every lane (no divergent spin on another lane's write).  KP / SP: generic or PGX_G
// pointers to unsigned long long / unsigned int (state is not used when W = 1).
template <int W, class KP, class SP>
__device__ __forceinline__ i64 pgx_insert(KP keys, SP state, u64 cap, const u64 (&k)[W], u64 max_probes) {
  const u64 mask = cap - 1;
  const u64 lim = cap < max_probes ? cap : max_probes;
  u64 h = pgx_key_hash<W>(k) & mask;
  u64 probes = 0;
  if constexpr (W == 1) {
    for (; probes < lim; ++probes) {
      u64 prev = ~0ull;
      __hip_atomic_compare_exchange_strong(keys + h, &prev, k[0], __ATOMIC_RELAXED, PGX_RELAXED_AGENT);
      if (prev == ~0ull || prev == k[0]) return (i64)h;
      h = (h + 1) & mask;
    }
  } else {
    while (probes < lim) {
      u32 st = 0u;
      __hip_atomic_compare_exchange_strong(state + h, &st, 1u, __ATOMIC_RELAXED, PGX_RELAXED_AGENT);
      if (st == 0u) {
#pragma unroll
        for (int w = 0; w < W; ++w) __hip_atomic_store(keys + W * h + w, k[w], PGX_RELAXED_AGENT);
        __threadfence();
        __hip_atomic_exchange(state + h, 2u, PGX_RELAXED_AGENT);
        return (i64)h;
      }
      if (st == 2u) {
        u64 t[W];  // every word is loaded before any is compared: the loads are in flight together
#pragma unroll
        for (int w = 0; w < W; ++w) t[w] = __hip_atomic_load(keys + W * h + w, PGX_RELAXED_AGENT);
        bool same = true;
#pragma unroll
        for (int w = 0; w < W; ++w) same = same && t[w] == k[w];
        if (same) return (i64)h;
        h = (h + 1) & mask;
        ++probes;
      }
      // st == 1: another lane is publishing this slot; re-read next iteration.
    }
  }
  return -1;
}

// The slot of a key an earlier launch inserted (read-only probe; -1 if absent).
template <int W, class KP, class SP>
__device__ __forceinline__ i64 pgx_find(KP keys, SP state, u64 cap, const u64 (&k)[W], u64 max_probes) {
  const u64 mask = cap - 1;
  const u64 lim = cap < max_probes ? cap : max_probes;
  u64 h = pgx_key_hash<W>(k) & mask;
  for (u64 probes = 0; probes < lim; ++probes) {
    if constexpr (W == 1) {
      const u64 t = keys[h];
      if (t == k[0]) return (i64)h;
      if (t == ~0ull) return -1;
    } else {
      if (state[h] != 2u) return -1;
      bool same = true;
#pragma unroll
      for (int w = 0; w < W; ++w) same = same && keys[W * h + w] == k[w];
      if (same) return (i64)h;
    }
    h = (h + 1) & mask;
  }
  return -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Planes.  Order-preserving encodings for MIN / MAX planes (unsigned compare == signed / IEEE compare), and the four
// plane ops (PlaneOp: 0 int64 add, 1 f64 add on the plane's bits, 2 ordered min, 3 ordered max).
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 pgx_ord_i64(i64 x) { return (u64)x ^ 0x8000000000000000ull; }
__device__ __forceinline__ u64 pgx_ord_bits(u64 b) {  // (the bits of a double)
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ u64 pgx_f64_bits(double d) { return (u64)__double_as_longlong(d); }
__device__ __forceinline__ double pgx_bits_f64(u64 b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ u64 pgx_ord_f64(double d) { return pgx_ord_bits(pgx_f64_bits(d)); }

__device__ __forceinline__ double* pgx_as_f64(u64* p) { return (double*)p; }
__device__ __forceinline__ PGX_G double* pgx_as_f64(PGX_G u64* p) { return (PGX_G double*)p; }

// *p op= enc, atomically.  P: a generic (global or LDS) or PGX_G pointer to unsigned long long.
template <class P>
__device__ __forceinline__ void pgx_plane_apply(P p, int op, u64 enc) {
  switch (op) {
    case 0: __hip_atomic_fetch_add(p, enc, PGX_RELAXED_AGENT); break;
    case 1:
#if defined(__has_extension) && __has_extension(clang_atomic_attributes)
      [[clang::atomic(fine_grained_memory, remote_memory)]]  // as atomicAdd(double*): any allocation kind
#endif
      { __hip_atomic_fetch_add(pgx_as_f64(p), pgx_bits_f64(enc), PGX_RELAXED_AGENT); }
      break;
    case 2: __hip_atomic_fetch_min(p, enc, PGX_RELAXED_AGENT); break;
    default: __hip_atomic_fetch_max(p, enc, PGX_RELAXED_AGENT); break;
  }
}
__device__ __forceinline__ u64 pgx_plane_combine(int op, u64 x, u64 y) {
  if (op == 0) return x + y;
  if (op == 1) return pgx_f64_bits(pgx_bits_f64(x) + pgx_bits_f64(y));
  if (op == 2) return x < y ? x : y;
  return x > y ? x : y;
}

#endif  // PGX_DEVICE_H_
