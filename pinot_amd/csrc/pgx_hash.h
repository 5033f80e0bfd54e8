// libpgx: the boxed Java values' hashCode() in Java int arithmetic, and the union of hash-code lists.  Host only and
// free of device code: pgx_hll.cpp (the HLL code tables, pgx_hll_codes, the DISTINCTCOUNT hash tables,
// pgx_java_hash_codes), pgx_distinct.cpp (the per-group union) and tests/host/distinct_host_check.cpp share it.
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
// String.hashCode over the UTF-16 code units of a UTF-8 string (a malformed byte decodes to U+FFFD)
inline int32_t hash_utf8(const uint8_t* s, size_t n) {
  uint32_t h = 0;
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
      h = 31u * h + (0xD800u + (cp >> 10));
      h = 31u * h + (0xDC00u + (cp & 0x3FFu));
    } else {
      h = 31u * h + cp;
    }
  }
  return int32_t(h);
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
