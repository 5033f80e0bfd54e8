// Direct test entry of the query kernels' run-time-position row decode (pgx_jit_device.h pgx_unpack_at /
// pgx_unpack_frac_at) against the whole-lane unpack (pgx_unpack / pgx_unpack_frac), for every bit width and every
// rows-per-lane count the query compiler uses.  tests/test_gpu_unpack_at.py drives it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_jit_abi.h"
#include "pgx_device.h"
#include "pgx_jit_device.h"

namespace {

// Lane i owns rows [i * R, i * R + R) of a B-bit forward index.  ref[i * R + q] = row q of the whole-lane unpack;
// at[i * R + q] = the single-row decode at position js[q] (a run-time value: read from memory).
template <int B, int R, bool FRAC>
__global__ void pgx_unpack_at_check(const u32* __restrict__ fwd, int n, const u32* __restrict__ js, u32* at, u32* ref) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 v[R];
  if constexpr (FRAC) {
    constexpr int RB = R * B;
    constexpr int G = RB % 32 == 0 ? 32 : (RB % 16 == 0 ? 16 : (RB % 8 == 0 ? 8 : (RB % 4 == 0 ? 4 : (RB % 2 == 0 ? 2 : 1))));
    constexpr int DL = (RB + 32 - G + 31) / 32;
    const long long o = (long long)i * RB;
    const u32 sh = (u32)(o & 31);
    u32 w[DL];
#pragma unroll
    for (int k = 0; k < DL; ++k) w[k] = fwd[(o >> 5) + k];
    pgx_unpack_frac<B, R, DL>(w, sh, v);
#pragma unroll
    for (int q = 0; q < R; ++q) ref[(long long)i * R + q] = v[q];
#pragma unroll 1
    for (int q = 0; q < R; ++q) at[(long long)i * R + q] = pgx_unpack_frac_at<B, R, DL>(w, sh, js[q]);
  } else {
    constexpr int D = R * B / 32;
    u32 w[D];
#pragma unroll
    for (int k = 0; k < D; ++k) w[k] = fwd[(long long)i * D + k];
    pgx_unpack<B, R>(w, v);
#pragma unroll
    for (int q = 0; q < R; ++q) ref[(long long)i * R + q] = v[q];
#pragma unroll 1
    for (int q = 0; q < R; ++q) at[(long long)i * R + q] = pgx_unpack_at<B, R>(w, js[q]);
  }
}

template <int B, int R>
hipError_t launch_br(bool frac, const u32* fwd, int n, const u32* js, u32* at, u32* ref, hipStream_t st) {
  const dim3 grid((n + 255) / 256), block(256);
  if (frac) {
    if constexpr (B == 32) return hipErrorInvalidValue;  // (whole dwords: never a frac column)
    else hipLaunchKernelGGL((pgx_unpack_at_check<B, R, true>), grid, block, 0, st, fwd, n, js, at, ref);
  } else {
    if constexpr ((R * B) % 32 != 0) return hipErrorInvalidValue;
    else hipLaunchKernelGGL((pgx_unpack_at_check<B, R, false>), grid, block, 0, st, fwd, n, js, at, ref);
  }
  return hipGetLastError();
}

template <int B>
hipError_t launch_b(int R, bool frac, const u32* fwd, int n, const u32* js, u32* at, u32* ref, hipStream_t st) {
  if (R == 8) return launch_br<B, 8>(frac, fwd, n, js, at, ref, st);
  if (R == 16) return launch_br<B, 16>(frac, fwd, n, js, at, ref, st);
  if (R == 32) return launch_br<B, 32>(frac, fwd, n, js, at, ref, st);
  return hipErrorInvalidValue;
}

template <int B>
hipError_t launch_from(int bits, int R, bool frac, const u32* fwd, int n, const u32* js, u32* at, u32* ref, hipStream_t st) {
  if (bits == B) return launch_b<B>(R, frac, fwd, n, js, at, ref, st);
  if constexpr (B < 32) return launch_from<B + 1>(bits, R, frac, fwd, n, js, at, ref, st);
  else return hipErrorInvalidValue;
}

}  // namespace

// fwd: n * R * bits bits of forward index (frac: plus two dwords of padding), js: R row positions in [0, R),
// at / ref: n * R words each.  Non-frac needs R * bits % 32 == 0.
extern "C" hipError_t pgx_launch_unpack_at_check(int bits, int R, int frac, const uint32_t* fwd, int n, const uint32_t* js,
                                                 uint32_t* at, uint32_t* ref, hipStream_t stream) {
  if (bits < 1 || bits > 32 || n < 1 || !fwd || !js || !at || !ref) return hipErrorInvalidValue;
  return launch_from<1>(bits, R, frac != 0, fwd, n, js, at, ref, stream);
}
