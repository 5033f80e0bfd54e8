// Device side of the bitmap inverted-index leaves, shared by the library kernels (pgx_roaring.hip) and the query kernels
// generated at run time (pasted after pgx_jit_abi.h and pgx_device.h -- u32, PGX_G, the LDS-only barriers -- and in
// front of pgx_jit_device.h).  Builtin types only, no includes.
//
// BitmapBasedFilterOperator (operator/filter/BitmapBasedFilterOperator.java:62-92) ORs the RoaringBitmap of every
// matching dictId (segment/index/readers/BitmapInvertedIndexReader.java:91-117); AndBlockDocIdSet / OrBlockDocIdSet
// combine bitmap leaves; NEQ / NOT_IN flip over [0, num_docs) (BitmapDocIdSet).  RoaringBitmap 0.5.10 portable format
// without run containers: cookie 12346, container count, (key, card - 1) u16 pairs, u32 offsets, then array (<= 4096
// u16 values) or bitmap (1024 u64 LE words) containers.  The doc mask of a 65536-doc chunk is 2048 words in LDS: array
// containers go in bit by bit with LDS atomics, bitmap containers word by word.  Roaring bytes are only 2-byte aligned
// inside the inverted-index file, so multi-byte fields are read as u16 pairs (the headers everywhere, and the containers
// in the workgroup kernels below; the wave kernel of pgx_roaring.hip reads containers as wide aligned granules).
#ifndef PGX_ROARING_DEVICE_H_
#define PGX_ROARING_DEVICE_H_

__device__ __forceinline__ u32 pgx_rd16(const unsigned char* p) { return *(const PGX_G unsigned short*)p; }
__device__ __forceinline__ u32 pgx_rd32(const unsigned char* p) { return pgx_rd16(p) | (pgx_rd16(p + 2) << 16); }
// Bitmap k of a descriptor: its dictId's entry of the .bitmap.inv header (BE int offsets, 4-byte aligned) locates it.
__device__ __forceinline__ const unsigned char* pgx_rbitmap(const PGX_G JRDesc* d, int k) {
  const u32 id = ((const PGX_G u32*)d->ids)[k];
  return d->inv + __builtin_bswap32(((const PGX_G u32*)d->inv)[id]);
}

// The container of `chunk` in the bitmap at base: its cardinality (0: none) and where it starts.  Keys are sorted and
// distinct, so a bitmap with a container in every chunk holds chunk c at index c: probe there first (one load for dense
// bitmaps), then binary-search the rest of the range.
__device__ __forceinline__ int pgx_rcontainer(const unsigned char* base, int chunk, const unsigned char*& ptr) {
  const int n = (int)pgx_rd32(base + 4);
  int lo = 0, hi = n - 1, found = -1;
  const int g = min(chunk, n - 1);
  if (g >= 0) {
    const int k = (int)pgx_rd16(base + 8 + 4 * g);
    if (k == chunk) found = g;
    else if (k < chunk) lo = g + 1;
    else hi = g - 1;
  }
  while (found < 0 && lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const int k = (int)pgx_rd16(base + 8 + 4 * mid);
    if (k == chunk) { found = mid; break; }
    if (k < chunk) lo = mid + 1; else hi = mid - 1;
  }
  if (found < 0) return 0;
  ptr = base + pgx_rd32(base + 8 + 4 * n + 4 * found);
  return (int)pgx_rd16(base + 8 + 4 * found + 2) + 1;
}

// Cursor over one bitmap's containers for kernels that walk a segment's chunks in order: key() / card() / ptr()
// describe the first container not yet consumed (key 1 << 30 past the last).  advance() loads the next container's
// fields at once; they are consumed at a later chunk, so the loads stay in flight while the current container is
// expanded.  The loaded words are kept as they come and taken apart in key() / card(): any arithmetic on them inside
// load() would make advance() wait for its own loads.
struct PgxRCursor {
  const unsigned char* base = nullptr;
  int n = 0, cur = 0;
  u32 kc = 0, off = 0;  // kc: key | (cardinality - 1) << 16
  __device__ __forceinline__ void load() {
    u32 k = kc, o = off;  // through locals: conditional stores to the members would put the cursor in scratch
    if (cur < n) {
      k = pgx_rd32(base + 8 + 4 * cur);
      o = pgx_rd32(base + 8 + 4 * n + 4 * cur);
    }
    kc = k, off = o;
  }
  __device__ __forceinline__ int key() const { return cur < n ? (int)(kc & 0xFFFFu) : 1 << 30; }
  __device__ __forceinline__ int card() const { return (int)(kc >> 16) + 1; }
  // first container with key >= c0: keys are strictly increasing, so key[c0] == c0 settles it
  __device__ __forceinline__ void seek(const unsigned char* bitmap, int c0) {
    base = bitmap;
    n = (int)pgx_rd32(base + 4);
    if (c0 > 0 && n > 0) {
      if (n > c0 && (int)pgx_rd16(base + 8 + 4 * c0) == c0) {
        cur = c0;
      } else {
        int lo = 0, hi = n;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if ((int)pgx_rd16(base + 8 + 4 * mid) < c0) lo = mid + 1; else hi = mid;
        }
        cur = lo;
      }
    }
    load();
  }
  __device__ __forceinline__ void advance() {
    ++cur;
    load();
  }
  __device__ __forceinline__ const unsigned char* ptr() const { return base + off; }
};

// Exclusive prefix of the array containers' cardinalities (bitmap containers count 0) over the nc found containers,
// by the workgroup's first wave, PER entries per lane: cpre[k] for every k < 64 * PER, the total in *total.  LIST: the
// bitmap containers' indices are listed in bidx, their number in *nbm.
template <int PER, bool LIST>
__device__ __forceinline__ void pgx_rcard_prefix(int lane, int nc, const int* ccard, int* cpre, int* total, int* bidx,
                                                 int* nbm) {
  int v[PER], x = 0, nb = 0;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int k = lane * PER + q;
    const bool in = k < nc;
    v[q] = (in && ccard[k] <= 4096) ? ccard[k] : 0;
    if (LIST) nb += (in && ccard[k] > 4096) ? 1 : 0;
    x += v[q];
  }
  int incl = x, binc = nb;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(incl, d, 64);
    const int z = LIST ? __shfl_up(binc, d, 64) : 0;
    if (lane >= d) {
      incl += y;
      binc += z;
    }
  }
  int e = incl - x, b = binc - nb;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int k = lane * PER + q;
    cpre[k] = e;
    e += v[q];
    if (LIST && k < nc && ccard[k] > 4096) bidx[b++] = k;
  }
  if (lane == 63) {
    *total = incl;
    if (LIST) *nbm = binc;
  }
}

// Array containers: every thread of the NT takes elements of any container, PER loads in flight before the LDS atomics
// (a loop over containers would chain one global-load latency per container).  Element e of the concatenated
// containers lies in the last container with cpre <= e (empty parts repeat cpre); its bit goes into leaf cleaf's mask.
template <int NT, int PER>
__device__ __forceinline__ void pgx_rspread(int tid, int nc, int ne, const unsigned char* const* cptr, const int* cpre,
                                            const int* cleaf, u32* lm) {
  for (int e0 = 0; e0 < ne; e0 += PER * NT) {
    u32 val[PER];
    int dst[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      // lanes past the last element load it again and OR nothing into word tid: no branch around the search, the load
      // or the atomic, so the PER loads are issued back to back, certainly consumed before the next round, and the
      // compiler never has to wait for loads still in flight (the first bitmap container's) at the head of the loop
      const int i = e0 + q * NT + tid, e = min(i, ne - 1);
      int lo = 0, hi = nc - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cpre[mid] <= e) lo = mid; else hi = mid - 1;
      }
      val[q] = pgx_rd16(cptr[lo] + 2 * (e - cpre[lo]));
      dst[q] = i < ne ? cleaf[lo] * 2048 : -1;
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const bool in = dst[q] >= 0;
      atomicOr(&lm[in ? dst[q] + (val[q] >> 5) : tid], in ? 1u << (val[q] & 31u) : 0u);
    }
  }
}

// Bitmap container c (1024 x u64 LE == 2048 x u32, bit j of word w = doc 32w + j) over the NT threads: every word's
// load issued (pgx_rwords_load), then the LDS ORs of the non-zero ones into mask m (pgx_rwords_or).
template <int NT>
__device__ __forceinline__ void pgx_rwords_load(const unsigned char* c, int tid, u32* x) {
#pragma unroll
  for (int q = 0; q < 2048 / NT; ++q) x[q] = pgx_rd32(c + 4 * (q * NT + tid));
}
template <int NT>
__device__ __forceinline__ void pgx_rwords_or(u32* m, int tid, const u32* x) {
#pragma unroll
  for (int q = 0; q < 2048 / NT; ++q)
    if (x[q]) atomicOr(&m[q * NT + tid], x[q]);
}

// NOT flips inside [0, num_docs) (BitmapDocIdSet: flip(startDocId, endDocId + 1)): the bits to keep of the mask word
// whose first doc is d.
__device__ __forceinline__ u32 pgx_rkeep(long long d, int num_docs) {
  return d >= num_docs ? 0u : (d + 32 > num_docs ? (1u << (num_docs - d)) - 1u : 0xFFFFFFFFu);
}

#define PGX_RB 256  // bitmaps per container-search batch
struct PgxRScratch {
  const unsigned char* cptr[PGX_RB];
  int ccard[PGX_RB], cpre[PGX_RB], cleaf[PGX_RB];
  int ncont, celems;
};

// The leaves of a program and the first bitmap number of each, for pgx_rexpand: NL leaves known at compile time, held
// in registers.  locate() is a select chain on purpose: indexing the arrays by a run-time leaf would put them in
// scratch memory.  (The library's wide kernel learns its leaves at run time and keeps them in LDS: PgxRLeavesLds.)
template <int NL>
struct PgxRLeavesReg {
  int desc[NL], b0[NL], total;
  __device__ __forceinline__ int leaves() const { return NL; }
  __device__ __forceinline__ void locate(int b, int& leaf, int& d, int& first) const {
    leaf = 0, d = desc[0], first = 0;
#pragma unroll
    for (int q = 1; q < NL; ++q)
      if (b >= b0[q]) { leaf = q; d = desc[q]; first = b0[q]; }
  }
};
struct PgxRLeavesLds {
  const int* desc;
  const int* b0;  // b0[nl]: all bitmaps
  int nl, total;
  __device__ __forceinline__ int leaves() const { return nl; }
  __device__ __forceinline__ void locate(int b, int& leaf, int& d, int& first) const {
    leaf = 0;
    while (b0[leaf + 1] <= b) ++leaf;  // (<= 8 leaves)
    d = desc[leaf], first = b0[leaf];
  }
};

// Builds the mask of every leaf of L for `chunk` into lm[leaf * 2048, +2048) (LDS), every leaf at once: one container
// search over ALL bitmaps of ALL leaves (a lane per bitmap, batches of PGX_RB), one pass over all their array-container
// elements, then the bitmap containers.  The dependent global-load chain is that of ONE leaf, not one per leaf.  Every
// thread of the NT-thread workgroup calls it; the caller synchronises before (lm and S reused) and after.
template <int NT, class LT>
__device__ void pgx_rexpand(const LT& L, const PGX_G JRDesc* D, int chunk, u32* lm, PgxRScratch& S) {
  const int tid = threadIdx.x;
  for (int i = tid; i < L.leaves() * 2048; i += NT) lm[i] = 0u;
  for (int b0 = 0; b0 < L.total; b0 += PGX_RB) {
    if (tid == 0) S.ncont = 0;
    pgx_lds_barrier();
    const int b = b0 + tid;
    if (tid < PGX_RB && b < L.total) {
      int leaf, d, first;
      L.locate(b, leaf, d, first);
      const unsigned char* ptr;
      const int card = pgx_rcontainer(pgx_rbitmap(D + d, b - first), chunk, ptr);
      if (card) {
        const int slot = atomicAdd(&S.ncont, 1);
        S.cptr[slot] = ptr;
        S.ccard[slot] = card;
        S.cleaf[slot] = leaf;
      }
    }
    pgx_lds_barrier();
    const int nc = S.ncont;
    if (tid < 64) pgx_rcard_prefix<PGX_RB / 64, false>(tid, nc, S.ccard, S.cpre, &S.celems, nullptr, nullptr);
    pgx_lds_barrier();
    pgx_rspread<NT, 4>(tid, nc, S.celems, S.cptr, S.cpre, S.cleaf, lm);
    for (int k = 0; k < nc; ++k) {
      if (S.ccard[k] <= 4096) continue;
      u32 x[2048 / NT];
      pgx_rwords_load<NT>(S.cptr[k], tid, x);
      pgx_rwords_or<NT>(lm + S.cleaf[k] * 2048, tid, x);
    }
    pgx_lds_barrier();
  }
}

// The generated kernels' entry: P->ldesc lists the NL leaves' descriptors in program order.
template <int NT, int NL>
__device__ void pgx_rchunk_leaves(const PGX_G JRProg* P, const PGX_G JRDesc* D, int chunk, u32* lm, PgxRScratch& S) {
  PgxRLeavesReg<NL> L;
  L.total = 0;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    L.desc[j] = P->ldesc[j];
    L.b0[j] = L.total;
    L.total += L.desc[j] >= 0 ? D[L.desc[j]].nb : 0;
  }
  pgx_rexpand<NT>(L, D, chunk, lm, S);
}

#endif  // PGX_ROARING_DEVICE_H_
