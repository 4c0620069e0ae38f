// rsa_common.hpp -- what the device RSA public operation (rsa.hip) and the host
// one (rsa_host.cpp) share: how a big-endian magnitude maps to little-endian
// 32-bit limbs, the EMSA-PKCS1-v1_5 encoding of a SHA-256 digest limb by limb,
// the carry resolve over generate / propagate masks, and the tables of one
// launch.  Plain C++ for the host unit, __host__ __device__ under HIP.
//
// THE ARITHMETIC.  A key has L = 64 or 128 limbs and R = 2^(32 L).  A Montgomery
// product mont(a, b) = a b R^-1 mod n runs L rows; row i adds a[i] * b and then
// m * n, m = t[0] * (-n^-1) mod 2^32, and drops the limb that became zero.  A
// column is a 64-bit accumulator that takes the LOW halves of the row's two
// products in place and their HIGH halves after the one-limb shift, so a column
// grows by less than 2^34 a row and 2^41 a product and no carry moves between
// columns inside the row loop, except the carry of the dropped limb, which
// joins the column that becomes limb 0.  The columns are resolved once per
// product: every digit (a lane's limbs) passes its excess to the next, which
// leaves a generate bit (the digit overflowed) and a propagate bit (the digit
// is all ones) per digit, and rsa_carry_in turns the two masks into every
// digit's carry-in at once.  (The host has no lanes to keep apart and lets its
// carries ripple limb by limb: rsa_host.cpp.)  The product lies in [0, 2n): the
// bit above the top limb and the comparison with n decide the one conditional
// subtraction, whose borrows are resolved the same way.  The chain is x =
// mont(s, R^2), y = x, then for every bit of e below its top one y = mont(y, y)
// and, where the bit is set, y = mont(y, x), and last mont(y, 1).  Nothing here
// is secret and nothing is constant-time.
#pragma once

#include <cstdint>

#include "../../include/vds_ec.h"

#if defined(__HIP__)
#define VDS_RSA_HD __host__ __device__ inline
#else
#define VDS_RSA_HD inline
#endif

namespace vds_ec {

constexpr uint32_t kRsaMinBits = 512, kRsaMaxBits = 4096;
constexpr uint32_t kRsaDigestInfoLen = 19, kRsaEmTail = kRsaDigestInfoLen + 32;  // DigestInfo || H
constexpr uint32_t kRsaEmMin = kRsaEmTail + 11;  // 00 01, eight FF at least, 00 (RFC 8017 9.2)
static_assert(kRsaEmMin <= kRsaMinBits / 8, "the encoding fits every modulus a key may have");

// limb j of the magnitude whose big-endian bytes are p[0 .. len): zero above it
VDS_RSA_HD uint32_t rsa_be_limb(const uint8_t *p, uint64_t len, uint32_t j) {
  uint32_t v = 0;
  for (uint32_t b = 0; b < 4; ++b) {
    const uint64_t pos = 4ull * j + b;
    if (pos < len) v |= (uint32_t)p[len - 1 - pos] << (8 * b);
  }
  return v;
}

// Byte `pos`, counted from the LAST byte, of EM = 00 01 FF..FF 00 || DigestInfo
// || H for a modulus of k bytes (k >= kRsaEmMin); zero at and above k.  The
// DigestInfo is SHA-256's WITH the NULL parameter (RFC 8017 9.2 note 1).
VDS_RSA_HD uint32_t rsa_em_byte(uint32_t pos, uint32_t k, const uint8_t *h) {
  if (pos < 32) return h[31 - pos];
  if (pos < kRsaEmTail) {
    // 30 31 30 0d 06 09 60 86 48 01 65 03 04 02 01 05 00 04 20 as little-endian words from its LAST byte
    const uint32_t i = pos - 32;
    const uint64_t w = i < 8 ? 0x0304020105000420ull : i < 16 ? 0x0d06096086480165ull : 0x303130ull;
    return (uint32_t)(w >> (8 * (i & 7u))) & 0xFFu;
  }
  if (pos == kRsaEmTail) return 0x00;
  if (pos + 2 < k) return 0xFF;
  if (pos + 2 == k) return 0x01;
  return 0x00;
}

VDS_RSA_HD uint32_t rsa_em_limb(uint32_t j, uint32_t k, const uint8_t *h) {
  uint32_t v = 0;
  for (uint32_t b = 0; b < 4; ++b) v |= rsa_em_byte(4 * j + b, k, h) << (8 * b);
  return v;
}

// Digit d generates a carry (g bit d) or passes one on (p bit d; never both):
// bit d of the result is the carry INTO digit d, *out the carry out of digit
// 63.  The sum (g | p) + g ripples exactly as the carries do.
VDS_RSA_HD uint64_t rsa_carry_in(uint64_t g, uint64_t p, uint32_t *out) {
  const uint64_t x = g | p, s = x + g;
  *out = s < x ? 1u : 0u;
  return s ^ p;
}

// What vds_ec_rsa_key_prepare leaves (the device entry points check it again:
// the kernel's loops and indices rest on it)
VDS_RSA_HD bool rsa_key_sane(const vds_ec_rsa_key &k) {
  if (k.limbs != 64 && k.limbs != 128) return false;
  if (k.n_bytes < kRsaMinBits / 8 || k.n_bytes > 4 * k.limbs) return false;
  if (k.limbs == 128 && k.n_bytes <= 256) return false;
  if (!(k.n[0] & 1u) || !(k.e & 1u) || k.e < 3) return false;
  return k.n0inv * k.n[0] == 0xFFFFFFFFu;
}

// One item of a launch, in launch order: the 128-limb ones first.
struct RsaItem {
  uint64_t in;      // the big-endian input (a signature, in the verify form)
  uint64_t out;     // raw form: where the n_bytes go
  uint32_t in_len;
  uint32_t key;     // index into the launch's keys
  uint32_t index;   // the caller's index: the status / verdict byte
  uint32_t digest;  // verify form: the digest's index
};
static_assert(sizeof(RsaItem) == 32, "RsaItem");

struct RsaLaunch {
  const RsaItem *items;
  const vds_ec_rsa_key *keys;
  uint32_t count;
  const uint8_t *digests;  // verify form
  uint8_t *results;        // statuses (raw form) or verdicts
};

}  // namespace vds_ec
