// test_deflate_host.cpp -- vds_ec_deflate_host into a heap buffer of exactly
// vds_ec_deflate_bound bytes and vds_ec_inflate_host back, over runs, periodic
// bodies and splitmix bodies at the lengths where the deflate changes its path.
// Then the length-limited code construction that host and device share
// (def_build_lengths), on counts no body of a segment's size can produce:
// Fibonacci numbers, whose unlimited tree is deeper than 15 (7 for the
// code-length alphabet).
// A stand-alone program: tests/test_deflate_host_cpp.py builds it from
// deflate_host.cpp and inflate_host.cpp with -fsanitize=address,undefined and
// runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "deflate_common.hpp"
#include "vds_ec.h"

static uint64_t splitmix(uint64_t &s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static int failures = 0;

static void round_trip(const char *what, const std::vector<uint8_t> &data) {
  const uint64_t n = data.size(), bound = vds_ec_deflate_bound(n);
  // heap buffers of exactly the sizes given: a byte outside either is the sanitizer's
  uint8_t *in = static_cast<uint8_t *>(std::malloc(n ? n : 1));
  uint8_t *z = static_cast<uint8_t *>(std::malloc(bound));
  uint8_t *back = static_cast<uint8_t *>(std::malloc(n ? n : 1));
  if (n) std::memcpy(in, data.data(), n);
  uint64_t zl = 0, bl = 0;
  int rc = vds_ec_deflate_host(n ? in : nullptr, n, z, bound, &zl);
  if (rc != VDS_EC_OK || zl > bound || zl < 11) {
    std::printf("FAIL %s n=%llu: deflate rc=%d len=%llu bound=%llu\n", what, (unsigned long long)n, rc,
                (unsigned long long)zl, (unsigned long long)bound);
    ++failures;
  } else {
    rc = vds_ec_inflate_host(z, zl, n ? back : nullptr, n, &bl);
    if (rc != VDS_EC_OK || bl != n || (n && std::memcmp(back, in, n))) {
      std::printf("FAIL %s n=%llu: inflate rc=%d len=%llu\n", what, (unsigned long long)n, rc, (unsigned long long)bl);
      ++failures;
    }
    if (bound > 11 && vds_ec_deflate_host(n ? in : nullptr, n, z, bound - 1, &zl) != VDS_EC_EINVAL) {
      std::printf("FAIL %s n=%llu: a capacity below the bound was taken\n", what, (unsigned long long)n);
      ++failures;
    }
  }
  std::free(in);
  std::free(z);
  std::free(back);
}

// lens must be a complete prefix code within maxbits, a length for exactly the counted symbols (two at least)
static void limit_case(const char *what, const std::vector<uint32_t> &freq, uint32_t maxbits, bool expect_cut) {
  static vds_ec::DeflPlan p;
  std::vector<uint8_t> lens(freq.size() + 8, 0xEE);
  std::vector<uint32_t> f(freq);
  f.resize(freq.size() + 8, 0);
  vds_ec::def_build_lengths(p, f.data(), (uint32_t)freq.size(), maxbits, lens.data());
  uint64_t kraft = 0, used = 0, longest = 0, weighted = 0;
  bool ok = true;
  for (size_t s = 0; s < freq.size(); ++s) {
    if (freq[s] && !lens[s]) ok = false;
    if (lens[s] > maxbits) ok = false;
    if (lens[s]) {
      kraft += 1ull << (maxbits - lens[s]);
      ++used;
      if (lens[s] > longest) longest = lens[s];
      weighted += (uint64_t)freq[s] * lens[s];
    }
  }
  for (size_t s = freq.size(); s < lens.size(); ++s)
    if (lens[s] != 0xEE) ok = false;
  // a rarer symbol never has the shorter code
  for (size_t a = 0; a < freq.size(); ++a)
    for (size_t b = 0; b < freq.size(); ++b)
      if (freq[a] && freq[b] && freq[a] < freq[b] && lens[a] < lens[b]) ok = false;
  if (!ok || used < 2 || kraft != (1ull << maxbits) || (expect_cut && longest != maxbits)) {
    std::printf("FAIL limit %s maxbits=%u: used=%llu kraft=%llu longest=%llu\n", what, maxbits, (unsigned long long)used,
                (unsigned long long)kraft, (unsigned long long)longest);
    ++failures;
  }
  (void)weighted;
}

static void limit_tests() {
  for (uint32_t maxbits : {15u, 7u}) {
    const uint32_t nsym = maxbits == 15u ? 286u : 19u;
    for (uint32_t k = 2; k <= (maxbits == 15u ? 19u : 12u); ++k) {  // k Fibonacci counts: k - 1 deep unlimited
      std::vector<uint32_t> f(nsym, 0);
      uint32_t a = 1, b = 1;
      for (uint32_t i = 0; i < k; ++i) {
        f[(i * 7u + 3u) % nsym] = a;
        const uint32_t t = a + b;
        a = b;
        b = t;
      }
      limit_case("fibonacci", f, maxbits, k - 1 > maxbits);
      f[(k * 7u + 3u) % nsym] = 1;  // a third count of one: the sums pass the next count, the tree is bushy, no cut
      limit_case("fibonacci+1", f, maxbits, false);
    }
    // powers of two, every symbol used with the same count, one symbol, none
    std::vector<uint32_t> f(nsym, 0);
    for (uint32_t i = 0; i < 14 && i < nsym; ++i) f[i] = 1u << (i < 13 ? i : 12);
    limit_case("powers", f, maxbits, maxbits == 7u);
    limit_case("flat", std::vector<uint32_t>(nsym, 5), maxbits, false);
    std::vector<uint32_t> one(nsym, 0);
    limit_case("none", one, maxbits, false);
    one[nsym - 1] = 3000;
    limit_case("one", one, maxbits, false);
    uint64_t s = 99;
    for (int r = 0; r < 200; ++r) {  // skewed random counts within a segment's total
      std::vector<uint32_t> g(nsym, 0);
      uint32_t total = 0;
      for (uint32_t i = 0; i < nsym && total < 3500; ++i) {
        const uint32_t v = (uint32_t)(splitmix(s) % 4 ? splitmix(s) % 3 : splitmix(s) % (1u << (splitmix(s) % 11)));
        g[i] = v;
        total += v;
      }
      limit_case("random", g, maxbits, false);
    }
  }
}

int main() {
  limit_tests();
  const uint32_t S = 3584;  // the deflate's segment
  const uint32_t lens[] = {0,     1,     2,     3,     4,     5,     63,    64,    65,    66,        67,
                           127,   128,   129,   257,   258,   259,   260,   32767, 32768, 32769,     32770,
                           65535, 65536, 65537, S - 1, S,     S + 1, 2 * S + 1, (1u << 20) + 5};
  const uint32_t periods[] = {1, 2, 3, 4, 5, 63, 64, 65, 258, 259, 32767, 32768, 32769};
  for (uint32_t n : lens) {
    std::vector<uint8_t> d(n, 0);
    round_trip("zeros", d);
    uint64_t s = 77 + n;
    for (uint32_t i = 0; i < n; ++i) d[i] = (uint8_t)splitmix(s);
    round_trip("splitmix", d);
    if (n > (1u << 17)) continue;  // (the long body: zeros and splitmix only)
    for (uint32_t per : periods) {
      if (per >= n) continue;
      std::vector<uint8_t> q(n);
      uint64_t t = 1000 + per;
      for (uint32_t i = 0; i < n; ++i) q[i] = i < per ? (uint8_t)splitmix(t) : q[i - per];
      round_trip("period", q);
    }
  }
  if (failures) return 1;
  std::printf("deflate OK\n");
  return 0;
}
