// libpgx: the boxed Java values' hashCode() in Java int arithmetic, and the union of hash-code lists.  Host only and
// free of device code: pgx_hll.cpp (the HLL code tables, pgx_hll_codes, the DISTINCTCOUNT hash tables,
// pgx_java_hash_codes), pgx_distinct.cpp (the per-group union), pgx_fasthll.cpp (the decode of a serialized estimator),
// tests/host/distinct_host_check.cpp and tests/host/fasthll_host_check.cpp share it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace pgxh {

inline int32_t hash_long(int64_t v) { return int32_t(uint32_t(uint64_t(v) ^ (uint64_t(v) >> 32))); }
inline int32_t hash_float(float f) {  // Float.hashCode: floatToIntBits (NaN canonical)
  if (f != f) return 0x7FC00000;
  int32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}
inline int32_t hash_double(double d) {  // Double.hashCode: (int)(bits ^ bits >>> 32) of doubleToLongBits
  uint64_t b = 0x7FF8000000000000ull;
  if (d == d) std::memcpy(&b, &d, 8);
  return int32_t(uint32_t(b ^ (b >> 32)));
}
// f(unit) for every UTF-16 code unit of a UTF-8 string, in order (a malformed byte decodes to U+FFFD, a supplementary
// code point to its surrogate pair)
template <typename F>
inline void utf16_units(const uint8_t* s, size_t n, F&& f) {
  for (size_t i = 0; i < n;) {
    uint32_t cp = 0xFFFDu;
    const uint8_t b = s[i];
    int more = b < 0x80 ? 0 : (b >> 5) == 6 ? 1 : (b >> 4) == 14 ? 2 : (b >> 3) == 30 ? 3 : -1;
    if (more >= 0 && i + size_t(more) < n) {
      uint32_t x = more == 0 ? b : more == 1 ? (b & 0x1Fu) : more == 2 ? (b & 0x0Fu) : (b & 0x07u);
      bool ok = true;
      for (int k = 1; k <= more; ++k) {
        ok = ok && (s[i + k] >> 6) == 2;
        x = (x << 6) | (s[i + k] & 0x3Fu);
      }
      if (ok && x <= 0x10FFFFu) {
        cp = x;
        i += size_t(more);
      }
    }
    ++i;
    if (cp >= 0x10000u) {  // a surrogate pair
      cp -= 0x10000u;
      f(0xD800u + (cp >> 10));
      f(0xDC00u + (cp & 0x3FFu));
    } else {
      f(cp);
    }
  }
}
// String.hashCode over the UTF-16 code units of a UTF-8 string
inline int32_t hash_utf8(const uint8_t* s, size_t n) {
  uint32_t h = 0;
  utf16_units(s, n, [&](uint32_t unit) { h = 31u * h + unit; });
  return int32_t(h);
}

// A FASTHLL column's value: HllUtil.convertStringToHll (startree/hll/HllUtil.java: byte = (byte)(char - 129) per UTF-16
// code unit), then HyperLogLog.Builder.build: big-endian log2m, byte count, and the RegisterSet words of six 5-bit
// registers (register i: word i / 6, shift 5 * (i % 6)).  regs: 256 bytes.  False for anything but a 180-byte
// estimator of log2m 8 (the reference throws there: addAll of another size); regs is then not written.
constexpr int kFastHllChars = 180;  // 8 header bytes and 43 register words (HllUtil.LOG2M_TO_SIZE_IN_BYTES, log2m 8)
constexpr int kFastHllRegs = 256;
inline bool fasthll_decode(const uint8_t* s, size_t n, uint8_t* regs) {
  uint8_t b[kFastHllChars];
  size_t nb = 0;
  utf16_units(s, n, [&](uint32_t unit) {
    if (nb < size_t(kFastHllChars)) b[nb] = uint8_t(unit - 129u);
    ++nb;
  });
  const auto word = [&](int at) {
    return (uint32_t(b[at]) << 24) | (uint32_t(b[at + 1]) << 16) | (uint32_t(b[at + 2]) << 8) | uint32_t(b[at + 3]);
  };
  if (nb != size_t(kFastHllChars) || word(0) != 8u || word(4) != uint32_t(kFastHllChars - 8)) return false;
  for (int i = 0; i < kFastHllRegs; ++i) regs[i] = uint8_t((word(8 + 4 * (i / 6)) >> (5 * (i % 6))) & 31u);
  return true;
}

// out[i] = hashCode of value i.  values: int32 / int64 / float / double per data_type (pgx_data_type: 0..4), or for
// STRING (4) the values' UTF-8 bytes back to back with n + 1 ascending offsets.  Returns null, or what is wrong with
// the arguments (nothing is written past the first bad value).
template <typename Out, typename F>
inline const char* hash_values(int32_t data_type, const void* values, const int32_t* string_offsets, int64_t n,
                               Out* out, F&& of_hash) {
  if (n < 0 || (n > 0 && (!values || !out))) return "bad argument";
  if (data_type < 0 || data_type > 4) return "data type";
  if (data_type == 4 && !string_offsets) return "STRING values need offsets";
  for (int64_t i = 0; i < n; ++i) {
    int32_t h;
    switch (data_type) {
      case 0: h = static_cast<const int32_t*>(values)[i]; break;
      case 1: h = hash_long(static_cast<const int64_t*>(values)[i]); break;
      case 2: h = hash_float(static_cast<const float*>(values)[i]); break;
      case 3: h = hash_double(static_cast<const double*>(values)[i]); break;
      default: {
        const int32_t a = string_offsets[i], b = string_offsets[i + 1];
        if (a < 0 || b < a) return "string offsets not ascending";
        h = hash_utf8(static_cast<const uint8_t*>(values) + a, size_t(b - a));
        break;
      }
    }
    out[i] = of_hash(h);
  }
  return nullptr;
}

inline const char* java_hash_codes(int32_t data_type, const void* values, const int32_t* string_offsets, int64_t n,
                                   int32_t* out) {
  return hash_values(data_type, values, string_offsets, n, out, [](int32_t h) { return h; });
}

// DistinctCountAggregationFunction's combine: the union of hash-code lists, ascending and unique (two values with
// equal hash codes count once, within one dictionary as well).
inline void sort_unique(std::vector<int32_t>& codes) {
  std::sort(codes.begin(), codes.end());
  codes.erase(std::unique(codes.begin(), codes.end()), codes.end());
}

}  // namespace pgxh
