// Stand-alone host check of pinot_amd/csrc/pgx_sel_key.h: the layout and the packing of the sparse GROUP BY's
// directory key, and the table-size arithmetic of its refusals, on edge inputs.  Meant for a sanitizer build; no
// device, no library:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipinot_amd/csrc \
//       tests/host/sel_key_host_check.cpp -o build/sel_key_host_check && build/sel_key_host_check
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "pgx_sel_key.h"

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

// random and extreme ids pack into distinct keys, and every field reads back
static void injective(const std::vector<int64_t>& cards) {
  SelKeyLayout L;
  CHECK(sel_key_layout(cards.data(), int(cards.size()), L));
  std::set<std::vector<int64_t>> seen;
  std::set<std::pair<uint64_t, uint64_t>> keys;
  uint64_t s = 88172645463325252ull;
  for (int i = 0; i < 2000; ++i) {
    std::vector<int64_t> ids(cards.size());
    for (size_t g = 0; g < cards.size(); ++g) {
      const int64_t top = cards[g] > 0 ? cards[g] - 1 : 0;
      ids[g] = i == 0 ? 0 : i == 1 ? top : i == 2 + int(g) ? top : int64_t(rnd(s) % uint64_t(top + 1));
    }
    uint64_t k[2];
    CHECK(sel_key_pack(L, ids.data(), k));
    if (L.W == 1) CHECK(k[1] == 0);
    if (seen.insert(ids).second) CHECK(keys.insert({k[0], k[1]}).second);
    for (size_t g = 0; g < cards.size(); ++g) {  // the field, read back from the 128-bit word
      const int at = 64 * L.word[g] + L.shift[g];
      uint64_t v = at < 64 ? k[0] >> at : k[1] >> (at - 64);
      if (at < 64 && at + L.bits[g] > 64) v |= k[1] << (64 - at);
      CHECK(int64_t(v & ((uint64_t(1) << L.bits[g]) - 1)) == ids[g]);
    }
  }
}

int main() {
  CHECK(sel_key_field_bits(0) == 1 && sel_key_field_bits(1) == 1 && sel_key_field_bits(2) == 1);
  CHECK(sel_key_field_bits(3) == 2 && sel_key_field_bits(4) == 2 && sel_key_field_bits(5) == 3);
  CHECK(sel_key_field_bits(int64_t(1) << 31) == 31 && sel_key_field_bits((int64_t(1) << 31) - 1) == 31);
  SelKeyLayout L;
  const int64_t c31 = int64_t(1) << 31;
  {  // exactly 64 bits: one word; 65: two, the last field at bit 0 of word 1
    const std::vector<int64_t> a{c31, c31, 4}, b{c31, c31, 5};
    CHECK(sel_key_layout(a.data(), 3, L) && L.total_bits == 64 && L.W == 1 && L.shift[2] == 62 && L.word[2] == 0);
    CHECK(sel_key_layout(b.data(), 3, L) && L.total_bits == 65 && L.W == 2 && L.shift[2] == 62 && L.word[2] == 0);
    injective(a);
    injective(b);
  }
  {  // 128 bits fit, 129 do not
    const std::vector<int64_t> a{c31, c31, c31, c31, 16}, b{c31, c31, c31, c31, 17};
    CHECK(sel_key_layout(a.data(), 5, L) && L.total_bits == 128 && L.W == 2);
    CHECK(!sel_key_layout(b.data(), 5, L));
    injective(a);
  }
  {  // a field that straddles bit 64: 3 x 30 bits
    const std::vector<int64_t> a{int64_t(1) << 30, int64_t(1) << 30, int64_t(1) << 30};
    CHECK(sel_key_layout(a.data(), 3, L) && L.word[2] == 0 && L.shift[2] == 60 && L.W == 2);
    injective(a);
  }
  {  // sixteen one-bit columns; seventeen columns, none, and a cardinality no int32 id reaches are refused
    const std::vector<int64_t> a(16, 2), b(17, 2), c{c31 + 1};
    CHECK(sel_key_layout(a.data(), 16, L) && L.total_bits == 16 && L.W == 1);
    CHECK(!sel_key_layout(b.data(), 17, L) && !sel_key_layout(a.data(), 0, L) && !sel_key_layout(nullptr, 1, L));
    CHECK(!sel_key_layout(c.data(), 1, L));
    injective(a);
    injective({300, 300});
    injective({1, 1, 1});
  }
  {  // ids outside their field are not keys
    const std::vector<int64_t> a{300, 300};
    CHECK(sel_key_layout(a.data(), 2, L));
    uint64_t k[2];
    const int64_t neg[2] = {-1, 5}, wide[2] = {5, 512}, top[2] = {511, 511};
    CHECK(!sel_key_pack(L, neg, k) && !sel_key_pack(L, wide, k) && sel_key_pack(L, top, k) && k[0] == 0x3FFFF);
  }
  {  // the refusals' arithmetic at the largest shapes: no overflow in 64 bits
    const uint64_t groups = 131072, regs = 256, cols = 16;
    CHECK(cols * groups * regs * 4 == (uint64_t(1) << 31));
    CHECK(groups * ((uint64_t(INT32_MAX) + 31) >> 5) * 4 < (uint64_t(1) << 63));
    CHECK(groups * uint64_t(INT32_MAX) * 8 < (uint64_t(1) << 63));
  }
  if (failures) return 1;
  std::printf("sel_key_host_check: ok\n");
  return 0;
}
