// Stand-alone host check of pinot_amd/csrc/pgx_hash.h: the Java hash codes behind pgx_java_hash_codes / pgx_hll_codes
// and the sort + unique union behind pgx_result_distinct, on edge inputs.  Meant for a sanitizer build; no device, no
// library:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipinot_amd/csrc \
//       tests/host/distinct_host_check.cpp -o build/distinct_host_check && build/distinct_host_check
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "pgx_hash.h"

using namespace pgxh;

static int failures = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                               \
    }                                                           \
  } while (0)

// the arrays are heap blocks of exactly the size the call may touch, so a read or write past them is reported
template <typename T>
static std::vector<int32_t> hashes(int32_t type, const std::vector<T>& v) {
  std::vector<int32_t> out(v.size());
  CHECK(java_hash_codes(type, v.data(), nullptr, int64_t(v.size()), out.data()) == nullptr);
  return out;
}

static std::vector<int32_t> string_hashes(const std::vector<std::string>& v) {
  std::vector<uint8_t> blob;
  std::vector<int32_t> off(1, 0);
  for (const auto& s : v) {
    blob.insert(blob.end(), s.begin(), s.end());
    off.push_back(int32_t(blob.size()));
  }
  if (blob.empty()) blob.push_back(0);
  std::vector<int32_t> out(v.size());
  CHECK(java_hash_codes(4, blob.data(), off.data(), int64_t(v.size()), out.data()) == nullptr);
  return out;
}

int main() {
  const int64_t lmin = std::numeric_limits<int64_t>::min(), lmax = std::numeric_limits<int64_t>::max();
  const int32_t imin = std::numeric_limits<int32_t>::min(), imax = std::numeric_limits<int32_t>::max();
  CHECK((hashes<int32_t>(0, {0, -1, imin, imax}) == std::vector<int32_t>{0, -1, imin, imax}));
  // Long.hashCode: (int)(v ^ v >>> 32); 0 and 0x100000001 collide
  CHECK((hashes<int64_t>(1, {0, 0x0000000100000001ll, -1, lmin, lmax, 1ll << 32}) ==
         std::vector<int32_t>{0, 0, 0, imin, imin, 1}));
  const float fnan = std::numeric_limits<float>::quiet_NaN(), finf = std::numeric_limits<float>::infinity();
  float other_nan;
  const uint32_t nan_bits = 0x7FC01234u;
  std::memcpy(&other_nan, &nan_bits, 4);
  CHECK((hashes<float>(2, {0.25f, 0.75f, 0.0f, -0.0f, fnan, other_nan, finf}) ==
         std::vector<int32_t>{0x3E800000, 0x3F400000, 0, imin, 0x7FC00000, 0x7FC00000, 0x7F800000}));
  const double dnan = std::numeric_limits<double>::quiet_NaN();
  CHECK((hashes<double>(3, {0.0, -0.0, 1.0, dnan, 0.25}) ==
         std::vector<int32_t>{0, imin, 0x3FF00000, 0x7FF80000, 0x3FD00000}));
  // String.hashCode over UTF-16 units: "" 0, "a" 97, "ab" 3105, U+00E9 233, U+4E2D 20013, U+1F600 = D83D DE00
  CHECK((string_hashes({"", "a", "ab", "\t", "\xC3\xA9", "\xE4\xB8\xAD", "\xF0\x9F\x98\x80"}) ==
         std::vector<int32_t>{0, 97, 3105, 9, 233, 20013, int32_t(31u * 0xD83Du + 0xDE00u)}));
  // malformed UTF-8 decodes to U+FFFD and never reads past the value: a lead byte at the very end, a stray
  // continuation byte, a 4-byte lead cut short
  CHECK((string_hashes({"\xC3", "\x80", "\xF0\x9F", "a\xE4"}) ==
         std::vector<int32_t>{0xFFFD, 0xFFFD, int32_t(31u * 0xFFFDu + 0xFFFDu), int32_t(31u * 97u + 0xFFFDu)}));
  CHECK(string_hashes({}).empty());

  // argument refusals: nothing is read or written
  int32_t one = 0;
  const int32_t good_off[2] = {0, 1}, bad_off[3] = {0, 3, 2}, neg_off[2] = {-1, 1};
  const uint8_t bytes[4] = {'a', 'b', 'c', 'd'};
  CHECK(java_hash_codes(0, &one, nullptr, -1, &one) != nullptr);
  CHECK(java_hash_codes(5, &one, nullptr, 1, &one) != nullptr);
  CHECK(java_hash_codes(-1, &one, nullptr, 1, &one) != nullptr);
  CHECK(java_hash_codes(0, nullptr, nullptr, 1, &one) != nullptr);
  CHECK(java_hash_codes(0, &one, nullptr, 1, nullptr) != nullptr);
  CHECK(java_hash_codes(4, bytes, nullptr, 1, &one) != nullptr);
  CHECK(java_hash_codes(4, bytes, neg_off, 1, &one) != nullptr);
  int32_t two[2] = {7, 7};
  CHECK(java_hash_codes(4, bytes, bad_off, 2, two) != nullptr && two[1] == 7);
  CHECK(java_hash_codes(4, bytes, good_off, 1, &one) == nullptr && one == 97);
  CHECK(java_hash_codes(0, nullptr, nullptr, 0, nullptr) == nullptr);

  // the union of the dictionaries' lists
  std::vector<int32_t> u;
  sort_unique(u);
  CHECK(u.empty());
  u = {5};
  sort_unique(u);
  CHECK((u == std::vector<int32_t>{5}));
  u = {3, imax, 0, imin, 3, 0, 0, -1, imax};
  sort_unique(u);
  CHECK((u == std::vector<int32_t>{imin, -1, 0, 3, imax}));
  u.assign(100000, 42);
  sort_unique(u);
  CHECK((u == std::vector<int32_t>{42}));
  u.clear();
  for (int32_t i = 0; i < 50000; ++i) u.push_back(int32_t(uint32_t(i) * 2654435761u));
  for (int32_t i = 0; i < 50000; i += 2) u.push_back(int32_t(uint32_t(i) * 2654435761u));
  sort_unique(u);
  CHECK(u.size() == 50000 && std::is_sorted(u.begin(), u.end()));

  if (failures) return 1;
  std::printf("distinct_host_check OK\n");
  return 0;
}
