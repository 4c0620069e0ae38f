// test_rsa_host.cpp -- the host RSA routines (rsa_host.cpp) on heap buffers of
// exactly the stated lengths: key preparation, the raw operation, the verdict
// of a signature, the fingerprint and the split of a transaction-log block.
// The cases come from a text file that tests/test_rsa_host_cpp.py writes, with
// every expected value computed there by Python integers (or recorded from
// libcrypto); one record a line, fields in hex ("-" for no bytes):
//   P n e in status out        vds_ec_rsa_public_host (status as a decimal)
//   V n e msg sig verdict      vds_ec_rsa_verify_sha256_host
//   F n e fingerprint          vds_ec_rsa_fingerprint
//   K n e status               vds_ec_rsa_key_prepare alone
//   T block status signed_len  vds_ec_txblock_parse
// A stand-alone program: the Python test builds it from rsa_host.cpp and
// sha256_host.cpp with -fsanitize=address,undefined and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "vds_ec.h"

// exactly `len` heap bytes (one where len is 0, never read): a byte outside is the sanitizer's
struct Heap {
  uint8_t *p;
  uint64_t len;
  explicit Heap(const std::string &hex) {
    len = hex == "-" ? 0 : hex.size() / 2;
    p = static_cast<uint8_t *>(std::malloc(len ? len : 1));
    for (uint64_t i = 0; i < len; ++i) p[i] = (uint8_t)std::stoul(hex.substr(2 * i, 2), nullptr, 16);
  }
  explicit Heap(uint64_t n) : p(static_cast<uint8_t *>(std::malloc(n ? n : 1))), len(n) { std::memset(p, 0xA5, n ? n : 1); }
  Heap(const Heap &) = delete;
  ~Heap() { std::free(p); }
  const uint8_t *in() const { return len ? p : nullptr; }
};

static int failures = 0;
static void fail(size_t line, const char *what) {
  std::printf("FAIL line %zu: %s\n", line, what);
  ++failures;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  std::string text;
  size_t line = 0, records = 0;
  while (std::getline(f, text)) {
    ++line;
    std::istringstream s(text);
    std::string kind;
    s >> kind;
    if (kind == "T") {
      std::string blk;
      int status;
      unsigned long long signed_len;
      s >> blk >> status >> signed_len;
      Heap b(blk);
      vds_ec_txblock out;
      const int rc = vds_ec_txblock_parse(b.p, b.len, &out);
      if (rc != status || (rc == VDS_EC_OK && out.signed_len != signed_len)) fail(line, "txblock_parse");
      ++records;
      continue;
    }
    std::string nh, eh;
    s >> nh >> eh;
    Heap n(nh), e(eh);
    // the key on the heap too: prepare writes exactly one vds_ec_rsa_key
    Heap kh(sizeof(vds_ec_rsa_key));
    vds_ec_rsa_key *key = reinterpret_cast<vds_ec_rsa_key *>(kh.p);
    if (kind == "F") {
      std::string fh;
      s >> fh;
      Heap want(fh), got(32);
      if (vds_ec_rsa_fingerprint(n.p, n.len, e.p, e.len, got.p) != VDS_EC_OK || std::memcmp(got.p, want.p, 32))
        fail(line, "fingerprint");
      ++records;
      continue;
    }
    const int prc = vds_ec_rsa_key_prepare(n.p, n.len, e.p, e.len, key);
    if (kind == "K") {
      int status;
      s >> status;
      if (prc != status) fail(line, "key_prepare status");
    } else if (prc != VDS_EC_OK) {
      fail(line, "key_prepare");
    } else if (kind == "P") {
      std::string ih, oh;
      int status;
      s >> ih >> status >> oh;
      Heap in(ih), want(oh), got(key->n_bytes);
      const int rc = vds_ec_rsa_public_host(key, in.in(), in.len, got.p);
      if (rc != status) fail(line, "public_host status");
      if (rc == VDS_EC_OK && (want.len != key->n_bytes || std::memcmp(got.p, want.p, want.len))) fail(line, "public_host");
    } else if (kind == "V") {
      std::string mh, sh;
      int verdict;
      s >> mh >> sh >> verdict;
      Heap msg(mh), sig(sh);
      uint8_t v = 7;
      if (vds_ec_rsa_verify_sha256_host(key, msg.in(), msg.len, sig.in(), sig.len, &v) != VDS_EC_OK || v != verdict)
        fail(line, "verify_sha256_host");
    } else {
      fail(line, "unknown record");
    }
    ++records;
  }
  if (failures || records == 0) {
    std::printf("%d failures in %zu records\n", failures, records);
    return 1;
  }
  std::printf("rsa OK: %zu records\n", records);
  return 0;
}
