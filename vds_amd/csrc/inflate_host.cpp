// inflate_host.cpp -- vds_ec_inflate_host: one zlib stream (RFC 1950 around
// RFC 1951) inflated on the calling thread, no GPU and no zlib: the path for
// one small message, and the CPU restatement of k_inflate_batch (inflate.hip)
// that the tests pin to zlib byte for byte, status for status.  The reference's
// inflate (kernel/vds_data/private/inflate_p.h) is zlib's inflateInit /
// inflate(Z_NO_FLUSH).
//
// The statuses follow zlib's own order of events.  A step needs its bits
// before it acts: an error shows only once the bits that reveal it lie inside
// the input, and an input that ends first is VDS_EC_EINFLATE_SHORT with what
// zlib would have delivered -- every literal whose code is wholly there, every
// match whose length code, distance code and extra bits are wholly there, the
// bytes of a stored block that are there.  Past the input's end the bit reader
// delivers zeros, as zlib's bit accumulator does above its valid bits, so a
// lookup on the bits that are left finds the same entry zlib's finds, and
// "entry.bits > bits available" is the same test.
//
// The tables are the two-level ones of inflate_common.hpp, built here by one
// thread in the order the device builds them with 64 lanes.
#include "../../include/vds_ec.h"

#include <cstring>
#include <mutex>

#include "inflate_common.hpp"

namespace vds_ec {
namespace {

struct BitIn {
  const uint8_t *in;
  uint64_t len, pos = 0;  // pos: the next byte to load (it may pass len: zeros)
  uint64_t hold = 0;
  uint32_t n = 0;
  uint64_t avail;  // message bits not yet consumed
  BitIn(const uint8_t *p, uint64_t l) : in(p), len(l), avail(8 * l) {}
  void fill() {  // at least 57 bits; 8 a step, so at most 8 steps
    while (n <= 56) {
      hold |= (uint64_t)(pos < len ? in[pos] : 0) << n;
      ++pos;
      n += 8;
    }
  }
  uint32_t peek(uint32_t k) const { return (uint32_t)(hold & ((1ull << k) - 1)); }
  void drop(uint32_t k) {  // k <= avail, k <= n
    hold >>= k;
    n -= k;
    avail -= k;
  }
  // restart at the message's byte b (the stored block's bytes skipped)
  void seek(uint64_t b) {
    pos = b;
    hold = 0;
    n = 0;
    avail = 8 * (len - b);
  }
};

// zlib's inflate_table: 0, or 1 for an over-subscribed set and for an
// incomplete one (allowed only with a single code of one bit).  `codes`: the
// code-length code, which may not be incomplete, and whose empty form decodes
// every lookup as symbol 0 of one bit (zlib reads the invalid entry's val
// without looking at its op there).
int build_table(const uint8_t *lens, uint32_t n, uint32_t root, inf_entry_t *T, uint32_t cap, bool codes) {
  uint32_t count[16] = {}, first[16] = {}, next[16];
  for (uint32_t i = 0; i < n; ++i) ++count[lens[i]];
  count[0] = 0;
  int left = 1;
  uint32_t code = 0, maxl = 0, p0 = 0;
  for (uint32_t l = 1; l <= 15; ++l) {
    code = (code + count[l - 1]) << 1;
    first[l] = code;
    left = (left << 1) - (int)count[l];
    if (left < 0) return 1;
    if (count[l]) maxl = l;
    if (l <= root) p0 += count[l] << (root - l);
  }
  const uint32_t nroot = 1u << root;
  if (maxl == 0) {
    for (uint32_t i = 0; i < nroot; ++i) T[i] = codes ? inf_entry(kInfSym, 1, 0) : kInfInvalidEntry;
    return 0;
  }
  if (left > 0 && (codes || maxl != 1)) return 1;
  for (uint32_t i = 0; i < nroot; ++i) T[i] = kInfInvalidEntry;
  uint32_t off = nroot;
  if (maxl > root)
    for (uint32_t p = p0; p < nroot; ++p) {
      const uint32_t L = inf_sub_len(count, first, root, p);
      if (!L) continue;
      if (off + (1u << (L - root)) > cap) return 1;  // (cannot be: zlib's ENOUGH)
      T[inf_brev(p, root)] = inf_entry(kInfLink, L - root, off);
      off += 1u << (L - root);
    }
  std::memcpy(next, first, sizeof next);
  for (uint32_t s = 0; s < n; ++s)
    if (lens[s]) inf_fill_symbol(T, cap, root, s, lens[s], next[lens[s]]++);
  return 0;
}

// the entry of the next code, its bits the total over both levels
inline uint32_t lookup(const inf_entry_t *T, uint32_t root, uint32_t bits) {
  const uint32_t e = T[bits & ((1u << root) - 1u)];
  if (inf_kind(e) != kInfLink) return e;
  const uint32_t e2 = T[inf_val(e) + ((bits >> root) & ((1u << inf_nbits(e)) - 1u))];
  return (e2 & ~15u) | (root + inf_nbits(e2));
}

struct FixedTables {
  inf_entry_t lit[kInfFixLitCap], dist[kInfFixDistCap];
  FixedTables() {
    uint8_t lens[288];
    for (uint32_t i = 0; i < 288; ++i) lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
    build_table(lens, 288, kInfLitRoot, lit, kInfFixLitCap, false);
    for (uint32_t i = 0; i < 32; ++i) lens[i] = 5;
    build_table(lens, 32, kInfDistRoot, dist, kInfFixDistCap, false);
  }
};
const FixedTables &fixed_tables() {
  static const FixedTables t;
  return t;
}

uint32_t adler32(const uint8_t *p, uint64_t n) {
  uint32_t a = 1, b = 0;
  while (n) {
    const uint64_t k = n < 5552 ? n : 5552;
    for (uint64_t i = 0; i < k; ++i) {
      a += p[i];
      b += a;
    }
    a %= kAdlerMod;
    b %= kAdlerMod;
    p += k;
    n -= k;
  }
  return (b << 16) | a;
}

int inflate(const uint8_t *in, uint64_t len, uint8_t *out, uint64_t cap, uint64_t *out_len) {
  BitIn b(in, len);
  uint64_t pos = 0;
  auto stop = [&](int status) {
    *out_len = status == VDS_EC_EINFLATE_SHORT || status == VDS_EC_OK ? pos : 0;
    return status;
  };
  // the zlib header: CMF, FLG; a preset dictionary is Z_NEED_DICT once its id is there
  if (b.avail < 16) return stop(VDS_EC_EINFLATE_SHORT);
  b.fill();
  const uint32_t cmf = b.peek(8), flg = b.peek(16) >> 8;
  if (((cmf << 8) + flg) % 31u || (cmf & 15u) != 8u || (cmf >> 4) > 7u) return stop(VDS_EC_EINFLATE_DATA);
  b.drop(16);
  if (flg & 0x20u) return stop(b.avail < 32 ? VDS_EC_EINFLATE_SHORT : VDS_EC_EINFLATE_DATA);

  inf_entry_t lit[kInfLitCap], dist[kInfDistCap], cl[kInfClCap];
  uint8_t lens[kInfMaxSyms];
  // Every block consumes its three header bits, all inside the message, or the loop ends.
  for (;;) {
    b.fill();
    if (b.avail < 3) return stop(VDS_EC_EINFLATE_SHORT);
    const uint32_t last = b.peek(1), type = b.peek(3) >> 1;
    b.drop(3);
    const inf_entry_t *LT = nullptr, *DT = nullptr;
    if (type == 0) {
      b.drop((uint32_t)(b.avail & 7u));
      if (b.avail < 32) return stop(VDS_EC_EINFLATE_SHORT);
      b.fill();
      const uint32_t n = b.peek(16), nn = b.peek(32) >> 16;
      if (n != (~nn & 0xFFFFu)) return stop(VDS_EC_EINFLATE_DATA);
      b.drop(32);
      const uint64_t there = b.avail / 8, src = len - there;
      const uint64_t take = n < there ? n : there;
      if (pos + take > cap) return stop(VDS_EC_EINFLATE_SPACE);
      if (take) std::memcpy(out + pos, in + src, take);
      pos += take;
      b.seek(src + take);
      if (take < n) return stop(VDS_EC_EINFLATE_SHORT);
    } else if (type == 1) {
      LT = fixed_tables().lit;
      DT = fixed_tables().dist;
    } else if (type == 2) {
      if (b.avail < 14) return stop(VDS_EC_EINFLATE_SHORT);
      const uint32_t nlen = b.peek(5) + 257u, ndist = (b.peek(10) >> 5) + 1u, ncode = (b.peek(14) >> 10) + 4u;
      b.drop(14);
      if (nlen > 286u || ndist > 30u) return stop(VDS_EC_EINFLATE_DATA);
      uint8_t cll[19] = {};
      for (uint32_t i = 0; i < ncode; ++i) {
        b.fill();
        if (b.avail < 3) return stop(VDS_EC_EINFLATE_SHORT);
        cll[kInfClOrder[i]] = (uint8_t)b.peek(3);
        b.drop(3);
      }
      if (build_table(cll, 19, kInfClRoot, cl, kInfClCap, true)) return stop(VDS_EC_EINFLATE_DATA);
      // Every step consumes at least one bit inside the message and adds at least one length.
      for (uint32_t have = 0; have < nlen + ndist;) {
        b.fill();
        const uint32_t e = lookup(cl, kInfClRoot, b.peek(15)), nb = inf_nbits(e), sym = inf_val(e);
        if (nb > b.avail) return stop(VDS_EC_EINFLATE_SHORT);
        if (sym < 16u) {
          b.drop(nb);
          lens[have++] = (uint8_t)sym;
          continue;
        }
        const uint32_t x = sym == 16u ? 2u : sym == 17u ? 3u : 7u;
        if (nb + x > b.avail) return stop(VDS_EC_EINFLATE_SHORT);
        b.drop(nb);
        if (sym == 16u && have == 0) return stop(VDS_EC_EINFLATE_DATA);
        const uint8_t v = sym == 16u ? lens[have - 1] : 0;
        const uint32_t rep = (sym == 18u ? 11u : 3u) + b.peek(x);
        b.drop(x);
        if (have + rep > nlen + ndist) return stop(VDS_EC_EINFLATE_DATA);
        for (uint32_t i = 0; i < rep; ++i) lens[have++] = v;
      }
      if (lens[256] == 0) return stop(VDS_EC_EINFLATE_DATA);
      if (build_table(lens, nlen, kInfLitRoot, lit, kInfLitCap, false)) return stop(VDS_EC_EINFLATE_DATA);
      if (build_table(lens + nlen, ndist, kInfDistRoot, dist, kInfDistCap, false)) return stop(VDS_EC_EINFLATE_DATA);
      LT = lit;
      DT = dist;
    } else {
      return stop(VDS_EC_EINFLATE_DATA);
    }
    // The symbols of a compressed block.  Every iteration consumes the bits of
    // one literal/length code, at least one and all inside the message (the
    // test against avail comes before the drop), or leaves the loop.
    while (LT) {
      b.fill();
      uint32_t e = lookup(LT, kInfLitRoot, b.peek(15)), nb = inf_nbits(e);
      if (nb > b.avail) return stop(VDS_EC_EINFLATE_SHORT);
      if (inf_kind(e) == kInfInvalid || nb == 0) return stop(VDS_EC_EINFLATE_DATA);
      const uint32_t sym = inf_val(e);
      if (sym < 256u) {
        if (pos >= cap) return stop(VDS_EC_EINFLATE_SPACE);
        out[pos++] = (uint8_t)sym;
        b.drop(nb);
        continue;
      }
      if (sym == 256u) {
        b.drop(nb);
        break;
      }
      if (sym > 285u) return stop(VDS_EC_EINFLATE_DATA);
      uint32_t x = 0;
      const uint32_t lbase = inf_len_base(sym, &x);
      if (nb + x > b.avail) return stop(VDS_EC_EINFLATE_SHORT);
      b.drop(nb);
      const uint32_t L = lbase + b.peek(x);
      b.drop(x);
      b.fill();
      e = lookup(DT, kInfDistRoot, b.peek(15));
      nb = inf_nbits(e);
      if (nb > b.avail) return stop(VDS_EC_EINFLATE_SHORT);
      if (inf_kind(e) == kInfInvalid || nb == 0 || inf_val(e) >= 30u) return stop(VDS_EC_EINFLATE_DATA);
      const uint32_t dbase = inf_dist_base(inf_val(e), &x);
      if (nb + x > b.avail) return stop(VDS_EC_EINFLATE_SHORT);
      b.drop(nb);
      const uint32_t D = dbase + b.peek(x);
      b.drop(x);
      // "invalid distance too far back" -- which zlib looks for only once the match's first byte has room
      if (D > pos) return stop(pos >= cap ? VDS_EC_EINFLATE_SPACE : VDS_EC_EINFLATE_DATA);
      if (pos + L > cap) return stop(VDS_EC_EINFLATE_SPACE);
      for (uint32_t i = 0; i < L; ++i) out[pos + i] = out[pos + i - D];
      pos += L;
    }
    if (last) break;
  }
  b.drop((uint32_t)(b.avail & 7u));
  if (b.avail < 32) return stop(VDS_EC_EINFLATE_SHORT);
  b.fill();
  const uint32_t t = b.peek(32);
  const uint32_t want = (t >> 24) | ((t >> 8) & 0xFF00u) | ((t << 8) & 0xFF0000u) | (t << 24);
  if (want != adler32(out, pos)) return stop(VDS_EC_EINFLATE_DATA);
  return stop(VDS_EC_OK);
}

}  // namespace
}  // namespace vds_ec

extern "C" int vds_ec_inflate_host(const uint8_t *in, uint64_t len, uint8_t *out, uint64_t out_cap,
                                   uint64_t *out_len) {
  if (!out_len || (len && !in) || (out_cap && !out)) return VDS_EC_EINVAL;
  if (len > 0xFFFFFFFFull || out_cap > 0xFFFFFFFFull) return VDS_EC_EINVAL;
  const uintptr_t a = reinterpret_cast<uintptr_t>(in), o = reinterpret_cast<uintptr_t>(out);
  if (len && out_cap && a < o + out_cap && o < a + len) return VDS_EC_EINVAL;
  return vds_ec::inflate(in, len, out, out_cap, out_len);
}
