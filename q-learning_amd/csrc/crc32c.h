// crc32c (Castagnoli, reflected 0x82F63B78), host only: the TF bundle reader's block / tensor checksum and the snapshot
// container's small-section checksum.
#pragma once
#include <cstddef>
#include <cstdint>

namespace qlx {

inline uint32_t crc32c(const uint8_t* p, size_t n) {
  struct Table {
    uint32_t t[256];
    Table() {
      for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
        t[i] = c;
      }
    }
  };
  static const Table table;
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) c = table.t[(c ^ p[i]) & 0xFF] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

}  // namespace qlx
