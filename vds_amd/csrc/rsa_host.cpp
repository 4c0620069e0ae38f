// rsa_host.cpp -- the RSA public operation and the RSASSA-PKCS1-v1_5 / SHA-256
// verdict of one signature on the calling CPU thread, the key preparation the
// device kernel needs, the reference's key fingerprint, and the split of a
// transaction-log block into its fields.
//
// The reference checks every record of the transaction log with
// asymmetric_sign_verify::verify(hash::sha256(), key, sig, data)
// (kernel/vds_crypto/asymmetriccrypto.cpp:488-537: EVP_DigestVerify* with an
// RSA key).  A batch of records goes to the device (rsa.hip); a single one is
// served here, and this file is the CPU restatement the device tests check
// against.  Portable C++, no OpenSSL: Montgomery products in the coarsely
// integrated operand scanning form (one pass of a[i] * b, one of m * n with the
// shift, carries rippling at once), which is the sequential statement of what
// rsa_common.hpp describes for the lanes.  Public data only, nothing here is
// constant-time.
#include <cstdint>
#include <cstring>

#include "rsa_common.hpp"

namespace vds_ec {

void sha256_host(const uint8_t *data, uint64_t len, uint8_t out[32]);  // sha256_host.cpp

namespace {

constexpr uint32_t kMaxL = VDS_EC_RSA_MAX_LIMBS;

// r = a b R^-1 mod n for a, b < n; r may be a or b
void mont(const uint32_t *a, const uint32_t *b, const uint32_t *n, uint32_t n0inv, uint32_t L, uint32_t *r) {
  uint32_t t[kMaxL + 2] = {};
  for (uint32_t i = 0; i < L; ++i) {
    uint64_t c = 0;
    for (uint32_t j = 0; j < L; ++j) {
      const uint64_t x = (uint64_t)a[i] * b[j] + t[j] + c;
      t[j] = (uint32_t)x;
      c = x >> 32;
    }
    uint64_t x = (uint64_t)t[L] + c;
    t[L] = (uint32_t)x;
    t[L + 1] = (uint32_t)(x >> 32);
    const uint32_t m = t[0] * n0inv;
    c = ((uint64_t)m * n[0] + t[0]) >> 32;
    for (uint32_t j = 1; j < L; ++j) {
      x = (uint64_t)m * n[j] + t[j] + c;
      t[j - 1] = (uint32_t)x;
      c = x >> 32;
    }
    x = (uint64_t)t[L] + c;
    t[L - 1] = (uint32_t)x;
    t[L] = t[L + 1] + (uint32_t)(x >> 32);
  }
  // [0, 2n): one conditional subtraction
  bool ge = t[L] != 0;
  if (!ge) {
    ge = true;
    for (uint32_t j = L; j-- > 0;)
      if (t[j] != n[j]) {
        ge = t[j] > n[j];
        break;
      }
  }
  uint64_t bw = 0;
  for (uint32_t j = 0; j < L; ++j) {
    const uint64_t x = (uint64_t)t[j] - (ge ? n[j] : 0u) - bw;
    r[j] = (uint32_t)x;
    bw = (x >> 32) & 1u;
  }
}

// the magnitude without its leading zero bytes
void strip(const uint8_t *&p, uint64_t &len) {
  while (len && !*p) {
    ++p;
    --len;
  }
}

bool below(const uint32_t *a, const uint32_t *n, uint32_t L) {
  for (uint32_t j = L; j-- > 0;)
    if (a[j] != n[j]) return a[j] < n[j];
  return false;
}

// out = in^e mod n as limbs; in < n
void public_op(const vds_ec_rsa_key &k, const uint32_t *in, uint32_t *out) {
  const uint32_t L = k.limbs;
  uint32_t x[kMaxL], y[kMaxL], one[kMaxL] = {};
  mont(in, k.rr, k.n, k.n0inv, L, x);
  std::memcpy(y, x, sizeof(y));
  int top = 31;
  while (!((k.e >> top) & 1u)) --top;
  for (int b = top - 1; b >= 0; --b) {
    mont(y, y, k.n, k.n0inv, L, y);
    if ((k.e >> b) & 1u) mont(y, x, k.n, k.n0inv, L, y);
  }
  one[0] = 1;
  mont(y, one, k.n, k.n0inv, L, out);
}

// binary_deserializer::read_number (binary_serialize.cpp:245-262), accepting
// only what write_number (:44-66) writes
bool read_number(const uint8_t *d, uint64_t len, uint64_t &at, uint64_t &v) {
  if (at >= len) return false;
  const uint8_t first = d[at++];
  if (first < 0x80) {
    v = first;
    return true;
  }
  const uint32_t cnt = first & 0x7Fu;
  if (cnt == 0 || cnt > 8 || len - at < cnt) return false;
  if (cnt > 1 && d[at] == 0) return false;  // a longer form of a smaller number
  uint64_t r = 0;
  for (uint32_t i = 0; i < cnt; ++i) r = (r << 8) | d[at++];
  if (r > UINT64_MAX - 0x80) return false;
  v = r + 0x80;
  return true;
}

// binary_deserializer::get(const_data_buffer &) (:197-215)
bool read_buffer(const uint8_t *d, uint64_t len, uint64_t &at, uint64_t &off, uint64_t &n) {
  if (!read_number(d, len, at, n)) return false;
  if (n > 1024ull * 1024 * 1024 || n > len - at) return false;
  off = at;
  at += n;
  return true;
}

uint64_t be(const uint8_t *p, uint32_t bytes) {
  uint64_t v = 0;
  for (uint32_t i = 0; i < bytes; ++i) v = (v << 8) | p[i];
  return v;
}

}  // namespace
}  // namespace vds_ec

extern "C" {

int vds_ec_rsa_key_prepare(const uint8_t *n_be, uint64_t n_len, const uint8_t *e_be, uint64_t e_len,
                           vds_ec_rsa_key *key) {
  using namespace vds_ec;
  if (!n_be || !e_be || !key) return VDS_EC_EINVAL;
  strip(n_be, n_len);
  strip(e_be, e_len);
  if (e_len == 0 || e_len > 4 || n_len == 0 || n_len > kRsaMaxBits / 8) return VDS_EC_EINVAL;
  uint32_t top = n_be[0], bits = (uint32_t)n_len * 8;
  while (!(top & 0x80u)) {
    top <<= 1;
    --bits;
  }
  if (bits < kRsaMinBits || !(n_be[n_len - 1] & 1u)) return VDS_EC_EINVAL;
  const uint32_t e = (uint32_t)be(e_be, (uint32_t)e_len);
  if (!(e & 1u) || e < 3) return VDS_EC_EINVAL;
  vds_ec_rsa_key k;
  std::memset(&k, 0, sizeof(k));
  k.limbs = bits <= 2048 ? 64 : 128;
  k.n_bytes = (uint32_t)n_len;
  k.e = e;
  for (uint32_t j = 0; j < k.limbs; ++j) k.n[j] = rsa_be_limb(n_be, n_len, j);
  // -n^-1 mod 2^32: Newton's iteration doubles the correct low bits (3 to start with, for any odd n)
  uint32_t inv = k.n[0];
  for (int i = 0; i < 5; ++i) inv *= 2u - k.n[0] * inv;
  k.n0inv = 0u - inv;
  // R^2 mod n: 1 doubled 64 L times
  uint32_t *x = k.rr;
  x[0] = 1;
  for (uint32_t i = 0; i < 64 * k.limbs; ++i) {
    uint32_t c = 0;
    for (uint32_t j = 0; j < k.limbs; ++j) {
      const uint32_t v = x[j];
      x[j] = (v << 1) | c;
      c = v >> 31;
    }
    if (c || !below(x, k.n, k.limbs)) {
      uint64_t bw = 0;
      for (uint32_t j = 0; j < k.limbs; ++j) {
        const uint64_t d = (uint64_t)x[j] - k.n[j] - bw;
        x[j] = (uint32_t)d;
        bw = (d >> 32) & 1u;
      }
    }
  }
  *key = k;
  return VDS_EC_OK;
}

int vds_ec_rsa_fingerprint(const uint8_t *n_be, uint64_t n_len, const uint8_t *e_be, uint64_t e_len, uint8_t *out) {
  using namespace vds_ec;
  if (!n_be || !e_be || !out) return VDS_EC_EINVAL;
  strip(n_be, n_len);
  strip(e_be, e_len);
  if (!n_len || !e_len || n_len > kRsaMaxBits / 8 + 64 || e_len > kRsaMaxBits / 8 + 64) return VDS_EC_EINVAL;
  // BN_bn2hex gives whole bytes, so its first character is the top nibble: a 00 goes in front above '8'
  uint8_t rec[11 + 2 * (4 + 1 + kRsaMaxBits / 8 + 64)];
  uint64_t at = 0;
  auto put32 = [&](uint64_t v) {
    for (int s = 24; s >= 0; s -= 8) rec[at++] = (uint8_t)(v >> s);
  };
  auto put_mag = [&](const uint8_t *p, uint64_t len) {
    const bool zero = (p[0] >> 4) > 8;
    put32(len + (zero ? 1 : 0));
    if (zero) rec[at++] = 0;
    std::memcpy(rec + at, p, len);
    at += len;
  };
  put32(7);
  std::memcpy(rec + at, "ssh-rsa", 7);
  at += 7;
  put_mag(e_be, e_len);
  put_mag(n_be, n_len);
  sha256_host(rec, at, out);
  return VDS_EC_OK;
}

int vds_ec_rsa_public_host(const vds_ec_rsa_key *key, const uint8_t *in, uint64_t in_len, uint8_t *out) {
  using namespace vds_ec;
  if (!key || !in || !out || !rsa_key_sane(*key) || in_len != key->n_bytes) return VDS_EC_EINVAL;
  uint32_t s[kMaxL], r[kMaxL];
  for (uint32_t j = 0; j < key->limbs; ++j) s[j] = rsa_be_limb(in, in_len, j);
  if (!below(s, key->n, key->limbs)) return VDS_EC_EINVAL;
  public_op(*key, s, r);
  for (uint32_t pos = 0; pos < key->n_bytes; ++pos)
    out[key->n_bytes - 1 - pos] = (uint8_t)(r[pos / 4] >> (8 * (pos % 4)));
  return VDS_EC_OK;
}

int vds_ec_rsa_verify_sha256_host(const vds_ec_rsa_key *key, const uint8_t *msg, uint64_t len, const uint8_t *sig,
                                  uint64_t sig_len, uint8_t *verdict) {
  using namespace vds_ec;
  if (!key || !verdict || !rsa_key_sane(*key) || (len && !msg) || (sig_len && !sig)) return VDS_EC_EINVAL;
  *verdict = 0;
  if (sig_len != key->n_bytes) return VDS_EC_OK;
  uint32_t s[kMaxL], r[kMaxL];
  for (uint32_t j = 0; j < key->limbs; ++j) s[j] = rsa_be_limb(sig, sig_len, j);
  if (!below(s, key->n, key->limbs)) return VDS_EC_OK;
  uint8_t h[32];
  sha256_host(msg, len, h);
  public_op(*key, s, r);
  uint32_t diff = 0;
  for (uint32_t j = 0; j < key->limbs; ++j) diff |= r[j] ^ rsa_em_limb(j, key->n_bytes, h);
  *verdict = diff == 0;
  return VDS_EC_OK;
}

int vds_ec_txblock_parse(const uint8_t *data, uint64_t len, vds_ec_txblock *out) {
  using namespace vds_ec;
  if (!data || !out) return VDS_EC_EINVAL;
  vds_ec_txblock b;
  std::memset(&b, 0, sizeof(b));
  if (len < 20 || be(data, 4) != 0x31564453u) return VDS_EC_ETX_FORM;
  b.time_point = be(data + 4, 8);
  b.order_no = be(data + 12, 8);
  // system_clock::from_time_t / to_time_t give the seconds back only while they fit the clock's nanoseconds
  if (b.time_point >= (1ull << 63) / 1000000000ull) return VDS_EC_ETX_FORM;
  uint64_t at = 20;
  if (!read_buffer(data, len, at, b.key_id_off, b.key_id_len)) return VDS_EC_ETX_FORM;
  b.ancestors_off = at;
  if (!read_number(data, len, at, b.ancestors_count)) return VDS_EC_ETX_FORM;
  uint64_t prev_off = 0, prev_len = 0;
  for (uint64_t i = 0; i < b.ancestors_count; ++i) {
    uint64_t off, n;
    if (!read_buffer(data, len, at, off, n)) return VDS_EC_ETX_FORM;
    // std::set's order, each strictly above the one before: const_data_buffer::operator< (size, then bytes)
    if (i && !(prev_len < n || (prev_len == n && std::memcmp(data + prev_off, data + off, n) < 0)))
      return VDS_EC_ETX_FORM;
    prev_off = off;
    prev_len = n;
  }
  b.ancestors_len = at - b.ancestors_off;
  if (!read_buffer(data, len, at, b.messages_off, b.messages_len)) return VDS_EC_ETX_FORM;
  b.signed_len = at;
  if (!read_buffer(data, len, at, b.signature_off, b.signature_len)) return VDS_EC_ETX_FORM;
  if (at != len) return VDS_EC_ETX_FORM;
  *out = b;
  return VDS_EC_OK;
}

}  // extern "C"
