// aes_tables.hpp -- the AES tables (FIPS-197 5.1.1, 5.3.2) computed at compile
// time, shared by the host cipher (aes_host.cpp) and the device kernels
// (aes_device.hpp, aes.hip).  Plain C++: no HIP here.
//
// A column of the state is one little-endian dword (row r in bits 8r..8r+7),
// which is how the bytes of a block load.  Te0[x] is the MixColumns column of
// S[x] in row 0, Td0[x] the InvMixColumns column of Si[x] in row 0; the tables
// for rows 1..3 are these rotated left by 8, 16 and 24 bits.
#pragma once

#include <cstdint>

namespace vds_ec {

struct AesTables {
  uint32_t te0[256];  // 2 S | S << 8 | S << 16 | 3 S << 24
  uint32_t td0[256];  // 14 Si | 9 Si << 8 | 13 Si << 16 | 11 Si << 24
  uint8_t sbox[256];
  uint8_t isbox[256];
};

constexpr uint32_t aes_xtime(uint32_t a) { return ((a << 1) ^ ((a & 0x80u) ? 0x11Bu : 0u)) & 0xFFu; }

constexpr uint32_t aes_gmul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 8; ++i) {
    if (b & 1u) p ^= a;
    a = aes_xtime(a);
    b >>= 1;
  }
  return p;
}

constexpr AesTables make_aes_tables() {
  AesTables t{};
  for (uint32_t x = 0; x < 256; ++x) {
    // the multiplicative inverse (0 -> 0) as x^254, then the affine map
    uint32_t inv = 1, b = x;
    for (int e = 254; e; e >>= 1) {
      if (e & 1) inv = aes_gmul(inv, b);
      b = aes_gmul(b, b);
    }
    if (x == 0) inv = 0;
    uint32_t s = inv;
    for (int i = 1; i <= 4; ++i) s ^= ((inv << i) | (inv >> (8 - i))) & 0xFFu;
    s ^= 0x63u;
    t.sbox[x] = (uint8_t)s;
    t.isbox[s] = (uint8_t)x;
  }
  for (uint32_t x = 0; x < 256; ++x) {
    const uint32_t s = t.sbox[x], si = t.isbox[x];
    t.te0[x] = aes_gmul(s, 2) | (s << 8) | (s << 16) | (aes_gmul(s, 3) << 24);
    t.td0[x] = aes_gmul(si, 14) | (aes_gmul(si, 9) << 8) | (aes_gmul(si, 13) << 16) | (aes_gmul(si, 11) << 24);
  }
  return t;
}

// pack_block_iv (dht_network_client.cpp:1101-1105, vds_ws.js:154)
constexpr uint8_t kAesBlockIv[16] = {0xa5, 0xbb, 0x9f, 0xce, 0xc2, 0xe4, 0x4b, 0x91,
                                     0xa8, 0xc9, 0x59, 0x44, 0x62, 0x55, 0x90, 0x24};
// ... as the four little-endian dwords of the block
constexpr uint32_t kAesBlockIvWords[4] = {0xce9fbba5u, 0x914be4c2u, 0x4459c9a8u, 0x24905562u};

// Rcon of the AES-256 schedule's seven S-box-and-rotate steps
constexpr uint32_t kAesRcon[7] = {0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40};

}  // namespace vds_ec
