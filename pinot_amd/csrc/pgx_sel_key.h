// libpgx: the key of a sparse run's group directory (SelSparseKey, pgx_internal.h), host side -- its layout from the
// group columns' global cardinalities, and the packing of one group's global ids.  Plain C++ without the device: the
// runner (pgx_hll.cpp) and tests/host/sel_key_host_check.cpp include it.  tests/sel_dir_ref.py is the numpy model.
#pragma once
#include <cstdint>

namespace pgxh {

constexpr int kSelKeyMaxCols = 16;  // pgx_internal.h kMaxGroupCols

// Field g: the column's global id in ceil(log2(cardinality)) bits, at least 1; the fields one after the other from bit
// 0 of a 128-bit word.  Field g starts at bit 64 * word[g] + shift[g]; one that straddles bit 64 continues in word 1.
struct SelKeyLayout {
  int ngcols = 0;
  int total_bits = 0;
  int W = 0;  // 64-bit words of a key: 1 for up to 64 bits, 2 for up to 128
  uint8_t shift[kSelKeyMaxCols] = {}, word[kSelKeyMaxCols] = {}, bits[kSelKeyMaxCols] = {};
};

inline int sel_key_field_bits(int64_t card) {
  int b = 1;
  while (b < 63 && (int64_t(1) << b) < card) ++b;
  return b;
}

// false: no column or more than kSelKeyMaxCols, a cardinality over 2^31 (ids are int32), or a key wider than 128 bits
inline bool sel_key_layout(const int64_t* cards, int ngcols, SelKeyLayout& L) {
  L = SelKeyLayout{};
  if (!cards || ngcols < 1 || ngcols > kSelKeyMaxCols) return false;
  int at = 0;
  for (int g = 0; g < ngcols; ++g) {
    if (cards[g] < 0 || cards[g] > (int64_t(1) << 31)) return false;
    const int b = sel_key_field_bits(cards[g]);
    if (at + b > 128) return false;
    L.shift[g] = uint8_t(at & 63);
    L.word[g] = uint8_t(at >> 6);
    L.bits[g] = uint8_t(b);
    at += b;
  }
  L.ngcols = ngcols;
  L.total_bits = at;
  L.W = at <= 64 ? 1 : 2;
  return true;
}

// key[0..1] of one group; false: an id outside its field
inline bool sel_key_pack(const SelKeyLayout& L, const int64_t* gids, uint64_t key[2]) {
  key[0] = key[1] = 0;
  for (int g = 0; g < L.ngcols; ++g) {
    const int64_t id = gids[g];
    if (id < 0 || (id >> L.bits[g]) != 0) return false;
    const uint64_t v = uint64_t(id);
    const int sh = L.shift[g];
    key[L.word[g]] |= v << sh;
    if (L.word[g] == 0 && sh + L.bits[g] > 64) key[1] |= v >> (64 - sh);
  }
  return true;
}

}  // namespace pgxh
