// Stand-alone host check of the FASTHLL decode in pinot_amd/csrc/pgx_hash.h (fasthll_decode, which
// pgx_fasthll_registers and the register images call): estimators written here as HllUtil.convertHllToString writes
// them read back register for register, and malformed, truncated and over-long values are refused without a write
// past the 180 bytes the decode keeps.  Meant for a sanitizer build; no device, no library:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipinot_amd/csrc \
//       tests/host/fasthll_host_check.cpp -o build/fasthll_host_check && build/fasthll_host_check
#include <cstdio>
#include <string>
#include <vector>

#include "pgx_hash.h"

using namespace pgxh;

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                   \
    }                                                               \
  } while (0)

static uint64_t rnd(uint64_t& s) {
  s ^= s << 13;
  s ^= s >> 7;
  s ^= s << 17;
  return s;
}

// HyperLogLog.getBytes(): log2m, 4 * words, the words big-endian (register i: word i / 6, shift 5 * (i % 6))
static std::vector<uint8_t> to_bytes(const uint8_t* regs, uint32_t log2m, uint32_t count) {
  std::vector<uint32_t> words(43, 0);
  for (int i = 0; i < 256; ++i) words[size_t(i / 6)] |= uint32_t(regs[i]) << (5 * (i % 6));
  std::vector<uint8_t> b;
  const auto put = [&](uint32_t w) {
    for (int k = 3; k >= 0; --k) b.push_back(uint8_t(w >> (8 * k)));
  };
  put(log2m);
  put(count);
  for (uint32_t w : words) put(w);
  return b;
}

// HllUtil.convertHllToString: char = (signed) byte + 129, here as UTF-8 (chars 1 .. 256: one or two bytes)
static std::string to_utf8(const std::vector<uint8_t>& bytes) {
  std::string s;
  for (uint8_t x : bytes) {
    const uint32_t ch = uint32_t(int(int8_t(x)) + 129);
    if (ch < 0x80) {
      s.push_back(char(ch));
    } else {
      s.push_back(char(0xC0 | (ch >> 6)));
      s.push_back(char(0x80 | (ch & 0x3F)));
    }
  }
  return s;
}

static bool decode(const std::string& s, uint8_t* regs) {
  // an exact-size copy, so that a read past the value's end is a heap overflow the sanitizer sees
  std::vector<uint8_t> v(s.begin(), s.end());
  return fasthll_decode(v.data(), v.size(), regs);
}

int main() {
  uint64_t s = 88172645463325252ull;
  uint8_t regs[256], got[256 + 16];
  for (int round = 0; round < 200; ++round) {
    for (int i = 0; i < 256; ++i) regs[i] = round == 0 ? 0 : round == 1 ? 31 : uint8_t(rnd(s) % 32);
    for (int i = 0; i < 256 + 16; ++i) got[i] = 0xA5;
    CHECK(decode(to_utf8(to_bytes(regs, 8, 172)), got));
    for (int i = 0; i < 256; ++i) CHECK(got[i] == regs[i]);
    for (int i = 256; i < 256 + 16; ++i) CHECK(got[i] == 0xA5);
  }
  const std::string good = to_utf8(to_bytes(regs, 8, 172));
  for (int i = 0; i < 256; ++i) got[i] = 0xA5;
  CHECK(!decode(to_utf8(to_bytes(regs, 9, 172)), got));   // another log2m
  CHECK(!decode(to_utf8(to_bytes(regs, 8, 168)), got));   // another byte count
  CHECK(!decode(std::string(), got));
  std::vector<uint8_t> shorter = to_bytes(regs, 8, 172);
  shorter.pop_back();
  CHECK(!decode(to_utf8(shorter), got));                  // 179 chars
  CHECK(!decode(good + "A", got));                        // 181 chars
  CHECK(!decode(good + good + good + good + good + good, got));  // 1,080 chars: nothing kept past the 180th
  CHECK(!decode(good.substr(0, good.size() - 1) + "\xF0\x9F\x98\x80", got));  // a surrogate pair: two units
  CHECK(!decode(std::string(180, '\xFF'), got));          // 180 malformed bytes: 180 x U+FFFD, no estimator
  // a value that ends inside a two-byte char: the lone lead byte is one U+FFFD, whatever the count then says; only
  // the read matters here (nothing past the value's end)
  std::string cut = good;
  while (!cut.empty() && (uint8_t(cut.back()) & 0xC0) != 0xC0) cut.pop_back();
  uint8_t scratch[256];
  (void)decode(cut, scratch);
  for (int i = 0; i < 256; ++i) CHECK(got[i] == 0xA5);    // a refused value writes nothing
  if (failures) return 1;
  std::printf("fasthll_host_check: ok\n");
  return 0;
}
