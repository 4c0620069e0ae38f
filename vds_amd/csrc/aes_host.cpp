// aes_host.cpp -- AES-256-CBC with PKCS#7 padding of one message on the
// calling CPU thread.
//
// The reference packs a piece of a file into a body with two passes of this
// cipher (client::save, dht_network_client.cpp:1107-1140; save_block,
// vds_ws.js:151-161) and wraps every channel message in one
// (user_channel.cpp:229): symmetric_encrypt / symmetric_decrypt over OpenSSL's
// EVP_aes_256_cbc with its default padding (private/symmetriccrypto_p.h).  CBC
// encryption is ONE chain of dependent blocks, so a single small message (a
// channel message) is served here for the reason the body hash is (DESIGN
// 3.8); batches of bodies go to the device (aes.hip), and this file is the
// CPU restatement the device tests check against.
//
// Two implementations, picked once at first use: AES-NI (aesenc / aesdec) and
// a portable one (FIPS-197 with the Te0 / Td0 tables of aes_tables.hpp), the
// only one on other hosts.  VDS_EC_AES_HOST=portable in the environment, read
// at that first use, forces the latter (tests/test_aes_host_cpu.py runs a
// child process each way and compares them).  Both share the key schedule;
// the decrypt schedule is the equivalent inverse cipher's (FIPS-197 5.3.5:
// InvMixColumns of the middle round keys), which is also what aesdec expects.
#if defined(__x86_64__) || defined(__i386__)
#define VDS_HOST_AES_X86 1
#include <cpuid.h>
#include <immintrin.h>
#else
#define VDS_HOST_AES_X86 0
#endif

#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "aes_tables.hpp"
#include "vds_ec.h"

namespace vds_ec {
namespace {

constexpr AesTables kT = make_aes_tables();

inline uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
inline uint32_t sub_word(uint32_t w) {
  return (uint32_t)kT.sbox[w & 0xFF] | (uint32_t)kT.sbox[(w >> 8) & 0xFF] << 8 |
         (uint32_t)kT.sbox[(w >> 16) & 0xFF] << 16 | (uint32_t)kT.sbox[w >> 24] << 24;
}
inline uint32_t load32(const uint8_t *p) {
  uint32_t v;
  std::memcpy(&v, p, 4);
  return v;
}
inline void store32(uint8_t *p, uint32_t v) { std::memcpy(p, &v, 4); }

// rk: the 60 schedule words as little-endian dwords (so their bytes in memory
// are the schedule's bytes); drk: the equivalent inverse cipher's, round by round.
struct Schedule {
  alignas(16) uint32_t rk[60];
  alignas(16) uint32_t drk[60];
};

void expand(const uint8_t key[32], Schedule &s) {
  for (int i = 0; i < 8; ++i) s.rk[i] = load32(key + 4 * i);
  for (int i = 8; i < 60; ++i) {
    uint32_t t = s.rk[i - 1];
    if (i % 8 == 0)
      t = sub_word(rotl(t, 24)) ^ kAesRcon[i / 8 - 1];  // RotWord: byte 1 becomes byte 0
    else if (i % 8 == 4)
      t = sub_word(t);
    s.rk[i] = s.rk[i - 8] ^ t;
  }
  for (int r = 0; r <= 14; ++r)
    for (int c = 0; c < 4; ++c) {
      const uint32_t w = s.rk[4 * (14 - r) + c];
      s.drk[4 * r + c] = r == 0 || r == 14 ? w
                                           : kT.td0[kT.sbox[w & 0xFF]] ^ rotl(kT.td0[kT.sbox[(w >> 8) & 0xFF]], 8) ^
                                                 rotl(kT.td0[kT.sbox[(w >> 16) & 0xFF]], 16) ^
                                                 rotl(kT.td0[kT.sbox[w >> 24]], 24);
    }
}

// ------------------------------------------------------------ portable
void enc_block_portable(const uint32_t *rk, uint32_t s[4]) {
  uint32_t a0 = s[0] ^ rk[0], a1 = s[1] ^ rk[1], a2 = s[2] ^ rk[2], a3 = s[3] ^ rk[3];
  for (int r = 1; r < 14; ++r) {
    const uint32_t *k = rk + 4 * r;
    const uint32_t b0 = kT.te0[a0 & 0xFF] ^ rotl(kT.te0[(a1 >> 8) & 0xFF], 8) ^ rotl(kT.te0[(a2 >> 16) & 0xFF], 16) ^
                        rotl(kT.te0[a3 >> 24], 24) ^ k[0];
    const uint32_t b1 = kT.te0[a1 & 0xFF] ^ rotl(kT.te0[(a2 >> 8) & 0xFF], 8) ^ rotl(kT.te0[(a3 >> 16) & 0xFF], 16) ^
                        rotl(kT.te0[a0 >> 24], 24) ^ k[1];
    const uint32_t b2 = kT.te0[a2 & 0xFF] ^ rotl(kT.te0[(a3 >> 8) & 0xFF], 8) ^ rotl(kT.te0[(a0 >> 16) & 0xFF], 16) ^
                        rotl(kT.te0[a1 >> 24], 24) ^ k[2];
    const uint32_t b3 = kT.te0[a3 & 0xFF] ^ rotl(kT.te0[(a0 >> 8) & 0xFF], 8) ^ rotl(kT.te0[(a1 >> 16) & 0xFF], 16) ^
                        rotl(kT.te0[a2 >> 24], 24) ^ k[3];
    a0 = b0, a1 = b1, a2 = b2, a3 = b3;
  }
  const uint32_t *k = rk + 56;
  const uint8_t *S = kT.sbox;
  s[0] = ((uint32_t)S[a0 & 0xFF] | (uint32_t)S[(a1 >> 8) & 0xFF] << 8 | (uint32_t)S[(a2 >> 16) & 0xFF] << 16 |
          (uint32_t)S[a3 >> 24] << 24) ^ k[0];
  s[1] = ((uint32_t)S[a1 & 0xFF] | (uint32_t)S[(a2 >> 8) & 0xFF] << 8 | (uint32_t)S[(a3 >> 16) & 0xFF] << 16 |
          (uint32_t)S[a0 >> 24] << 24) ^ k[1];
  s[2] = ((uint32_t)S[a2 & 0xFF] | (uint32_t)S[(a3 >> 8) & 0xFF] << 8 | (uint32_t)S[(a0 >> 16) & 0xFF] << 16 |
          (uint32_t)S[a1 >> 24] << 24) ^ k[2];
  s[3] = ((uint32_t)S[a3 & 0xFF] | (uint32_t)S[(a0 >> 8) & 0xFF] << 8 | (uint32_t)S[(a1 >> 16) & 0xFF] << 16 |
          (uint32_t)S[a2 >> 24] << 24) ^ k[3];
}

void dec_block_portable(const uint32_t *drk, uint32_t s[4]) {
  uint32_t a0 = s[0] ^ drk[0], a1 = s[1] ^ drk[1], a2 = s[2] ^ drk[2], a3 = s[3] ^ drk[3];
  for (int r = 1; r < 14; ++r) {
    const uint32_t *k = drk + 4 * r;
    const uint32_t b0 = kT.td0[a0 & 0xFF] ^ rotl(kT.td0[(a3 >> 8) & 0xFF], 8) ^ rotl(kT.td0[(a2 >> 16) & 0xFF], 16) ^
                        rotl(kT.td0[a1 >> 24], 24) ^ k[0];
    const uint32_t b1 = kT.td0[a1 & 0xFF] ^ rotl(kT.td0[(a0 >> 8) & 0xFF], 8) ^ rotl(kT.td0[(a3 >> 16) & 0xFF], 16) ^
                        rotl(kT.td0[a2 >> 24], 24) ^ k[1];
    const uint32_t b2 = kT.td0[a2 & 0xFF] ^ rotl(kT.td0[(a1 >> 8) & 0xFF], 8) ^ rotl(kT.td0[(a0 >> 16) & 0xFF], 16) ^
                        rotl(kT.td0[a3 >> 24], 24) ^ k[2];
    const uint32_t b3 = kT.td0[a3 & 0xFF] ^ rotl(kT.td0[(a2 >> 8) & 0xFF], 8) ^ rotl(kT.td0[(a1 >> 16) & 0xFF], 16) ^
                        rotl(kT.td0[a0 >> 24], 24) ^ k[3];
    a0 = b0, a1 = b1, a2 = b2, a3 = b3;
  }
  const uint32_t *k = drk + 56;
  const uint8_t *S = kT.isbox;
  s[0] = ((uint32_t)S[a0 & 0xFF] | (uint32_t)S[(a3 >> 8) & 0xFF] << 8 | (uint32_t)S[(a2 >> 16) & 0xFF] << 16 |
          (uint32_t)S[a1 >> 24] << 24) ^ k[0];
  s[1] = ((uint32_t)S[a1 & 0xFF] | (uint32_t)S[(a0 >> 8) & 0xFF] << 8 | (uint32_t)S[(a3 >> 16) & 0xFF] << 16 |
          (uint32_t)S[a2 >> 24] << 24) ^ k[1];
  s[2] = ((uint32_t)S[a2 & 0xFF] | (uint32_t)S[(a1 >> 8) & 0xFF] << 8 | (uint32_t)S[(a0 >> 16) & 0xFF] << 16 |
          (uint32_t)S[a3 >> 24] << 24) ^ k[2];
  s[3] = ((uint32_t)S[a3 & 0xFF] | (uint32_t)S[(a2 >> 8) & 0xFF] << 8 | (uint32_t)S[(a1 >> 16) & 0xFF] << 16 |
          (uint32_t)S[a0 >> 24] << 24) ^ k[3];
}

// CBC over n whole blocks.  `chain` is the iv on entry and the last ciphertext
// block on return.  in == out is allowed (the decrypt keeps the block it
// overwrites).
void cbc_enc_portable(const Schedule &sc, uint8_t chain[16], const uint8_t *in, uint64_t n, uint8_t *out) {
  uint32_t s[4];
  for (int c = 0; c < 4; ++c) s[c] = load32(chain + 4 * c);
  for (uint64_t b = 0; b < n; ++b) {
    for (int c = 0; c < 4; ++c) s[c] ^= load32(in + 16 * b + 4 * c);
    enc_block_portable(sc.rk, s);
    for (int c = 0; c < 4; ++c) store32(out + 16 * b + 4 * c, s[c]);
  }
  for (int c = 0; c < 4; ++c) store32(chain + 4 * c, s[c]);
}

void cbc_dec_portable(const Schedule &sc, uint8_t chain[16], const uint8_t *in, uint64_t n, uint8_t *out) {
  uint32_t prev[4];
  for (int c = 0; c < 4; ++c) prev[c] = load32(chain + 4 * c);
  for (uint64_t b = 0; b < n; ++b) {
    uint32_t ct[4], s[4];
    for (int c = 0; c < 4; ++c) s[c] = ct[c] = load32(in + 16 * b + 4 * c);
    dec_block_portable(sc.drk, s);
    for (int c = 0; c < 4; ++c) {
      store32(out + 16 * b + 4 * c, s[c] ^ prev[c]);
      prev[c] = ct[c];
    }
  }
  for (int c = 0; c < 4; ++c) store32(chain + 4 * c, prev[c]);
}

#if VDS_HOST_AES_X86
// ------------------------------------------------------------ AES-NI
__attribute__((target("aes,sse2"))) void cbc_enc_aesni(const Schedule &sc, uint8_t chain[16], const uint8_t *in,
                                                       uint64_t n, uint8_t *out) {
  __m128i k[15];
  for (int r = 0; r < 15; ++r) k[r] = _mm_load_si128((const __m128i *)(sc.rk + 4 * r));
  __m128i s = _mm_loadu_si128((const __m128i *)chain);
  for (uint64_t b = 0; b < n; ++b) {
    s = _mm_xor_si128(s, _mm_loadu_si128((const __m128i *)(in + 16 * b)));
    s = _mm_xor_si128(s, k[0]);
    for (int r = 1; r < 14; ++r) s = _mm_aesenc_si128(s, k[r]);
    s = _mm_aesenclast_si128(s, k[14]);
    _mm_storeu_si128((__m128i *)(out + 16 * b), s);
  }
  _mm_storeu_si128((__m128i *)chain, s);
}

__attribute__((target("aes,sse2"))) void cbc_dec_aesni(const Schedule &sc, uint8_t chain[16], const uint8_t *in,
                                                       uint64_t n, uint8_t *out) {
  __m128i k[15];
  for (int r = 0; r < 15; ++r) k[r] = _mm_load_si128((const __m128i *)(sc.drk + 4 * r));
  __m128i prev = _mm_loadu_si128((const __m128i *)chain);
  for (uint64_t b = 0; b < n; ++b) {
    const __m128i ct = _mm_loadu_si128((const __m128i *)(in + 16 * b));
    __m128i s = _mm_xor_si128(ct, k[0]);
    for (int r = 1; r < 14; ++r) s = _mm_aesdec_si128(s, k[r]);
    s = _mm_aesdeclast_si128(s, k[14]);
    _mm_storeu_si128((__m128i *)(out + 16 * b), _mm_xor_si128(s, prev));
    prev = ct;
  }
  _mm_storeu_si128((__m128i *)chain, prev);
}

bool have_aesni() {
  unsigned a, b, c, d;
  if (!__get_cpuid(1, &a, &b, &c, &d)) return false;
  return ((c >> 25) & 1u) && ((d >> 26) & 1u);  // AES, SSE2
}
#endif  // VDS_HOST_AES_X86

using CbcFn = void (*)(const Schedule &, uint8_t *, const uint8_t *, uint64_t, uint8_t *);
struct Impl {
  CbcFn enc, dec;
};
const Impl &impl() {
  static const Impl f = [] {
#if VDS_HOST_AES_X86
    const char *e = std::getenv("VDS_EC_AES_HOST");
    if (!(e && std::strcmp(e, "portable") == 0) && have_aesni()) return Impl{cbc_enc_aesni, cbc_dec_aesni};
#endif
    return Impl{cbc_enc_portable, cbc_dec_portable};
  }();
  return f;
}

}  // namespace

void aes256_cbc_encrypt_host(const uint8_t key[32], const uint8_t iv[16], const uint8_t *in, uint64_t len,
                             uint8_t *out) {
  Schedule sc;
  expand(key, sc);
  uint8_t chain[16];
  std::memcpy(chain, iv, 16);
  const uint64_t full = len / 16;
  uint8_t last[16];  // (taken before the whole blocks are written: in may be out)
  const uint32_t rem = (uint32_t)(len - 16 * full);
  if (rem) std::memcpy(last, in + 16 * full, rem);
  std::memset(last + rem, (int)(16 - rem), 16 - rem);
  if (full) impl().enc(sc, chain, in, full, out);
  impl().enc(sc, chain, last, 1, out + 16 * full);
}

int aes256_cbc_decrypt_host(const uint8_t key[32], const uint8_t iv[16], const uint8_t *in, uint64_t len, uint8_t *out,
                            uint64_t *out_len) {
  *out_len = 0;
  if (len == 0 || len % 16) return VDS_EC_ECRYPT_LENGTH;
  Schedule sc;
  expand(key, sc);
  uint8_t chain[16];
  std::memcpy(chain, iv, 16);
  impl().dec(sc, chain, in, len / 16, out);
  const uint32_t pad = out[len - 1];
  if (pad < 1 || pad > 16) return VDS_EC_ECRYPT_PADDING;
  for (uint32_t i = 0; i < pad; ++i)
    if (out[len - 1 - i] != pad) return VDS_EC_ECRYPT_PADDING;
  *out_len = len - pad;
  return VDS_EC_OK;
}

}  // namespace vds_ec

extern "C" uint64_t vds_ec_aes256_cbc_padded_size(uint64_t len) { return (len / 16 + 1) * 16; }

extern "C" int vds_ec_block_iv(uint8_t *iv) {
  if (!iv) return VDS_EC_EINVAL;
  std::memcpy(iv, vds_ec::kAesBlockIv, 16);
  return VDS_EC_OK;
}

extern "C" int vds_ec_aes256_cbc_encrypt_host(const uint8_t *key, const uint8_t *iv, const uint8_t *in, uint64_t len,
                                              uint8_t *out) {
  if (!key || !iv || !out || (len && !in)) return VDS_EC_EINVAL;
  vds_ec::aes256_cbc_encrypt_host(key, iv, in, len, out);
  return VDS_EC_OK;
}

extern "C" int vds_ec_aes256_cbc_decrypt_host(const uint8_t *key, const uint8_t *iv, const uint8_t *in, uint64_t len,
                                              uint8_t *out, uint64_t *out_len) {
  if (!key || !iv || !out_len || (len && (!in || !out))) return VDS_EC_EINVAL;
  return vds_ec::aes256_cbc_decrypt_host(key, iv, in, len, out, out_len);
}
