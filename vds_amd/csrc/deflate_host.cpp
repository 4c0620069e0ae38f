// deflate_host.cpp -- vds_ec_deflate_host: one buffer deflated into a zlib
// stream (RFC 1950 around RFC 1951) on the calling thread, no GPU and no zlib:
// the path for one small block, and the sequential statement of
// k_deflate_batch (deflate.hip), which writes the same bytes -- a block's body
// is named by its SHA-256, so two paths may not pack one block differently.
// The reference's deflate (kernel/vds_data/deflate.cpp) is zlib at its default
// level; what it needs from ours is a stream its inflate turns back into the
// data, and the tests pin that to zlib and to vds_ec_inflate_host.
//
// The algorithm is described in deflate_common.hpp, which also holds the plan
// of a dynamic block that the device runs unchanged.
#include "../../include/vds_ec.h"

#include <cstring>

#include "deflate_common.hpp"

namespace vds_ec {
namespace {

struct BitOut {
  uint8_t *out;
  uint64_t cap, pos = 0;
  uint64_t hold = 0;
  uint32_t n = 0;  // below 8 between calls
  BitOut(uint8_t *o, uint64_t c) : out(o), cap(c) {}
  void byte(uint8_t b) {
    if (pos < cap) out[pos] = b;  // (cap is at least the bound: always)
    ++pos;
  }
  void put(uint64_t v, uint32_t nb) {  // nb <= 48
    hold |= v << n;
    n += nb;
    for (; n >= 8; n -= 8, hold >>= 8) byte((uint8_t)hold);  // at most 6 steps
  }
  void align() {
    if (n) byte((uint8_t)hold);
    hold = 0;
    n = 0;
  }
};

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

struct Deflater {
  const uint8_t *in;
  uint64_t len;
  BitOut o;
  uint32_t hash[kDefHashSize];
  uint32_t tok[kDefSegment];
  uint32_t ntok = 0;
  DeflPlan p;
  uint64_t pend0 = 0, pend1 = 0;  // the pending stored run
  bool finished = false;

  Deflater(const uint8_t *i, uint64_t l, uint8_t *out, uint64_t cap) : in(i), len(l), o(out, cap) {}

  uint32_t match(uint64_t at, uint64_t from, uint32_t maxn) const {  // at most 258 steps
    uint32_t n = 0;
    while (n < maxn && in[from + n] == in[at + n]) ++n;
    return n;
  }
  void reset_segment() {
    std::memset(p.lfreq, 0, sizeof p.lfreq);
    std::memset(p.dfreq, 0, sizeof p.dfreq);
    ntok = 0;
  }
  // the pending run as stored blocks; every step writes 65535 bytes or the rest
  void flush_stored(bool final) {
    uint64_t r = pend1 - pend0, src = pend0;
    pend0 = pend1 = 0;
    if (!r && !final) return;
    do {
      const uint32_t t = (uint32_t)(r < kDefStoredMax ? r : kDefStoredMax);
      o.put(final && t == r ? 1u : 0u, 3);
      o.align();
      o.byte((uint8_t)t);
      o.byte((uint8_t)(t >> 8));
      o.byte((uint8_t)~t);
      o.byte((uint8_t)(~t >> 8));
      for (uint32_t i = 0; i < t; ++i) o.byte(in[src + i]);
      src += t;
      r -= t;
    } while (r);
    if (final) finished = true;
  }
  void end_segment(uint64_t start, uint64_t end, bool last) {
    def_plan(p);
    if ((uint64_t)p.dyn_bits + kDefStoredSlack <= 8 * (end - start)) {
      flush_stored(false);
      p.hdr[0] |= last ? 1u : 0u;
      for (uint32_t i = 0; i < p.nhdr; ++i) o.put(p.hdr[i] & 0xFFFFFFu, p.hdr[i] >> 24);
      for (uint32_t i = 0; i < ntok; ++i) {
        uint32_t nb;
        const uint64_t v = def_token_bits(p, tok[i], &nb);
        o.put(v, nb);
      }
      o.put(p.lcode[256], p.llen[256]);
      finished = last;
    } else {
      if (pend1 == pend0) pend0 = start;
      pend1 = end;
    }
    reset_segment();
  }

  uint64_t run() {
    o.byte(kDefCmf);
    o.byte(kDefFlg);
    std::memset(hash, 0, sizeof hash);
    reset_segment();
    uint64_t skip = 0, seg_start = 0;
    uint32_t mlen[kDefChunk], mdist[kDefChunk];
    for (uint64_t c = 0; c < len; c += kDefChunk) {
      const uint32_t nvalid = (uint32_t)(len - c < kDefChunk ? len - c : kDefChunk);
      for (uint32_t i = 0; i < nvalid; ++i) {
        const uint64_t at = c + i;
        mlen[i] = mdist[i] = 0;
        if (at < skip) continue;  // inside a match: nothing is chosen here
        const uint32_t maxn = (uint32_t)(len - at < kDefMaxMatch ? len - at : kDefMaxMatch);
        uint32_t l1 = 0, d1 = 0, l2 = 0;
        if (len - at >= 4) {
          uint32_t four;
          std::memcpy(&four, in + at, 4);  // (little-endian, as the device assembles it)
          const uint32_t h = hash[def_hash(four)];
          if (h && at - (h - 1) <= kDefMaxDist) {
            d1 = (uint32_t)(at - (h - 1));
            l1 = match(at, h - 1, maxn);
          }
        }
        if (at >= 1 && in[at] == in[at - 1]) l2 = match(at, at - 1, maxn);
        if (l2 >= l1 && l2 >= kDefMinMatch) {
          mlen[i] = l2;
          mdist[i] = 1;
        } else if (l1 >= kDefMinMatch) {
          mlen[i] = l1;
          mdist[i] = d1;
        }
      }
      for (uint32_t i = 0; i < nvalid; ++i) {
        const uint64_t at = c + i;
        if (len - at < 4) continue;
        uint32_t four;
        std::memcpy(&four, in + at, 4);
        uint32_t &slot = hash[def_hash(four)];
        if (slot < at + 1) slot = (uint32_t)(at + 1);
      }
      uint64_t pr = skip > c ? skip - c : 0;
      while (pr < nvalid) {  // a step takes a position or more
        if (mlen[pr] >= kDefMinMatch) {
          uint32_t eb, ev;
          tok[ntok++] = def_match_token(mlen[pr], mdist[pr]);
          ++p.lfreq[def_len_sym(mlen[pr], &eb, &ev)];
          ++p.dfreq[def_dist_sym(mdist[pr], &eb, &ev)];
          pr += mlen[pr];
        } else {
          tok[ntok++] = in[c + pr];
          ++p.lfreq[in[c + pr]];
          ++pr;
        }
      }
      skip = c + pr;
      const bool last = c + kDefChunk >= len;
      if ((c / kDefChunk + 1) % kDefSegChunks == 0 || last) {
        end_segment(seg_start, skip, last);
        seg_start = skip;
      }
    }
    if (!finished) flush_stored(true);
    o.align();
    const uint32_t ad = adler32(in, len);
    o.byte((uint8_t)(ad >> 24));
    o.byte((uint8_t)(ad >> 16));
    o.byte((uint8_t)(ad >> 8));
    o.byte((uint8_t)ad);
    return o.pos;
  }
};

}  // namespace
}  // namespace vds_ec

extern "C" uint64_t vds_ec_deflate_bound(uint64_t len) { return vds_ec::def_bound(len); }

extern "C" int vds_ec_deflate_host(const uint8_t *in, uint64_t len, uint8_t *out, uint64_t out_cap, uint64_t *out_len) {
  if (!out_len || (len && !in) || !out) return VDS_EC_EINVAL;
  if (len > 0xFFFFFFFFull || vds_ec::def_bound(len) > 0xFFFFFFFFull || out_cap < vds_ec::def_bound(len)) return VDS_EC_EINVAL;
  const uintptr_t a = reinterpret_cast<uintptr_t>(in), o = reinterpret_cast<uintptr_t>(out);
  if (len && a < o + out_cap && o < a + len) return VDS_EC_EINVAL;
  vds_ec::Deflater *d = new vds_ec::Deflater(in, len, out, out_cap);
  *out_len = d->run();
  delete d;
  return VDS_EC_OK;
}
