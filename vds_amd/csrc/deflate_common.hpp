// deflate_common.hpp -- what the device deflate (deflate.hip) and the host one
// (deflate_host.cpp) share, so that both write the same bytes: the constants of
// the match finder, the token word, the length / distance symbols, and the
// whole plan of one dynamic block (code lengths, codes, header) as one
// sequential routine over a DeflPlan, which the host runs on its stack and the
// device runs with one lane on LDS.  Plain C++ for the host unit,
// __host__ __device__ under HIP.
//
// THE ALGORITHM (deflate_host.cpp is its sequential statement).
//   match finding   The input is walked in chunks of 64 positions.  Position p
//       hashes its 4 bytes (none where fewer than 4 are left) and reads the
//       table: the candidate is the highest position with that hash in an
//       EARLIER chunk, because a chunk's positions -- all of them, those inside
//       a match too -- enter the table only after every position of the chunk
//       has read it; where two share a slot the higher one stays.  p - 1 is a
//       second candidate.  A candidate's length is the bytes that agree, at
//       most 258 and at most to the input's end; a candidate farther than
//       32768 is none.  Distance 1 wins a tie.
//   selection       Greedy: a match of 4 or more is taken where the walk
//       stands, else a literal; a match may run past its chunk, and the
//       positions it covers in later chunks emit nothing.
//   segments        kDefSegChunks chunks make a segment, and a segment becomes
//       one dynamic block when that is smaller by kDefStoredSlack bits than its
//       input bytes, else its input joins the pending stored run, which is
//       written (blocks of at most 65535 bytes) before the next dynamic block
//       and at the end.  The slack pays for the stored header that may follow
//       a dynamic block and for the padding before the Adler-32, so no output
//       is longer than the all-stored form, vds_ec_deflate_bound.
//   code lengths    Huffman by the two-queue method over the symbols sorted by
//       (count, symbol), lengths above the limit cut to it and the Kraft sum
//       repaired in whole units; at least two codes a tree, as zlib has it.
#pragma once

#include <cstdint>

#include "inflate_common.hpp"

#if defined(__HIP__)
#define VDS_DEF_HD __host__ __device__ inline
#else
#define VDS_DEF_HD inline
#endif

namespace vds_ec {

constexpr uint32_t kDefHashBits = 12, kDefHashSize = 1u << kDefHashBits;
constexpr uint32_t kDefChunk = 64, kDefSegChunks = 56, kDefSegment = kDefChunk * kDefSegChunks;
constexpr uint32_t kDefMinMatch = 4, kDefMaxMatch = 258, kDefMaxDist = 32768;
constexpr uint32_t kDefStoredMax = 65535, kDefStoredSlack = 64;
constexpr uint32_t kDefLitSyms = 286, kDefDistSyms = 30, kDefClSyms = 19;
constexpr uint32_t kDefHdrMax = 1 + kDefClSyms + kDefLitSyms + kDefDistSyms;
constexpr uint8_t kDefCmf = 0x78, kDefFlg = 0x01;  // CM 8, window 32 KiB; FLEVEL 0, no dictionary, FCHECK
static_assert((kDefCmf * 256u + kDefFlg) % 31u == 0, "FCHECK");
static_assert(kDefSegment + 3u < (1u << 14), "a count fits the two 7-bit passes of the sort and 16 bits");

VDS_INF_HD uint32_t def_hash(uint32_t four) { return (four * 2654435761u) >> (32u - kDefHashBits); }

// a token: a literal is its byte; a match has bit 31, length - 3 in bits 16..23, distance - 1 in bits 0..14
VDS_INF_HD uint32_t def_match_token(uint32_t len, uint32_t dist) { return 0x80000000u | ((len - 3u) << 16) | (dist - 1u); }

// the symbol of a length 3..258 / a distance 1..32768, its extra bits and their value (RFC 1951 3.2.5)
VDS_INF_HD uint32_t def_len_sym(uint32_t len, uint32_t *ebits, uint32_t *eval) {
  const uint32_t l = len - 3u;
  *ebits = 0;
  *eval = 0;
  if (l < 8u) return 257u + l;
  if (len == 258u) return 285u;
  const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2u;
  *ebits = e;
  *eval = l & ((1u << e) - 1u);
  return 261u + 4u * e + ((l >> e) - 4u);
}
VDS_INF_HD uint32_t def_dist_sym(uint32_t dist, uint32_t *ebits, uint32_t *eval) {
  const uint32_t d = dist - 1u;
  *ebits = 0;
  *eval = 0;
  if (d < 4u) return d;
  const uint32_t t = 31u - (uint32_t)__builtin_clz(d), e = t - 1u;
  *ebits = e;
  *eval = d & ((1u << e) - 1u);
  return 2u * t + ((d >> e) & 1u);
}
VDS_INF_HD uint32_t def_len_extra(uint32_t sym) { return sym < 265u || sym == 285u ? 0u : (sym - 261u) >> 2; }
VDS_INF_HD uint32_t def_dist_extra(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }

// vds_ec_deflate_bound: the all-stored form
VDS_INF_HD uint64_t def_bound(uint64_t len) {
  const uint64_t blocks = len ? (len + kDefStoredMax - 1u) / kDefStoredMax : 1u;
  return 2u + len + 5u * blocks + 4u;
}

// One segment's histograms in, its dynamic block's codes and header out.
struct DeflPlan {
  uint32_t lfreq[288], dfreq[32];  // the histograms (the end-of-block symbol is added by def_plan)
  uint32_t clfreq[20];
  uint32_t hdr[kDefHdrMax];  // the header's items, in order: bits in 0..23, their number in 24..31
  uint32_t nhdr, dyn_bits;   // dyn_bits: the whole block, header and end-of-block included
  uint16_t lcode[288], dcode[32], clcode[20];  // bit-reversed: ready to be written least significant bit first
  uint8_t llen[288], dlen[32], cllen[20];
  // work
  uint16_t fw[288], a[288], b[288], bucket[128], w[576], par[576], cls[320];
};

// Code lengths of at most maxbits for the n symbols counted in freq.  Every
// loop is bounded by n (at most 286), by the 128 buckets or by maxbits, except
// the two repairs: the first lowers E by at least one a step from at most n,
// the second raises it by at least one a step from above -2^maxbits.
VDS_DEF_HD void def_build_lengths(DeflPlan &p, const uint32_t *freq, uint32_t n, uint32_t maxbits, uint8_t *lens) {
  uint32_t m = 0;
  for (uint32_t s = 0; s < n; ++s) {
    p.fw[s] = (uint16_t)freq[s];
    lens[s] = 0;
    if (freq[s]) ++m;
  }
  for (uint32_t s = 0; m < 2u && s < n; ++s)  // at least two codes: the lowest unused symbols count once
    if (!p.fw[s]) {
      p.fw[s] = 1;
      ++m;
    }
  uint32_t k = 0;
  for (uint32_t s = 0; s < n; ++s)
    if (p.fw[s]) p.a[k++] = (uint16_t)s;
  // stable radix sort by count, 7 bits a pass: ascending (count, symbol)
  for (uint32_t pass = 0; pass < 2u; ++pass) {
    uint16_t *src = pass ? p.b : p.a, *dst = pass ? p.a : p.b;
    const uint32_t sh = 7u * pass;
    for (uint32_t i = 0; i < 128u; ++i) p.bucket[i] = 0;
    for (uint32_t i = 0; i < m; ++i) ++p.bucket[(p.fw[src[i]] >> sh) & 127u];
    uint32_t at = 0;
    for (uint32_t i = 0; i < 128u; ++i) {
      const uint32_t c = p.bucket[i];
      p.bucket[i] = (uint16_t)at;
      at += c;
    }
    for (uint32_t i = 0; i < m; ++i) dst[p.bucket[(p.fw[src[i]] >> sh) & 127u]++] = src[i];
  }
  // two queues: the leaves 0 .. m-1 in order, the inner nodes m .. 2m-2 as they are made; a leaf wins a tie
  for (uint32_t i = 0; i < m; ++i) p.w[i] = p.fw[p.a[i]];
  uint32_t li = 0, ni = m;
  for (k = m; k < 2u * m - 1u; ++k) {
    uint32_t x, y;
    if (li < m && (ni >= k || p.w[li] <= p.w[ni])) x = li++; else x = ni++;
    if (li < m && (ni >= k || p.w[li] <= p.w[ni])) y = li++; else y = ni++;
    p.w[k] = (uint16_t)(p.w[x] + p.w[y]);
    p.par[x] = (uint16_t)k;
    p.par[y] = (uint16_t)k;
  }
  // depths in place of the parents, root first (a parent's index is above its children's)
  p.par[2u * m - 2u] = 0;
  for (uint32_t node = 2u * m - 2u; node-- > 0u;) p.par[node] = (uint16_t)(p.par[p.par[node]] + 1u);
  // the leaves a length, cut at maxbits; E: the Kraft sum's excess in units of 2^-maxbits
  for (uint32_t i = 0; i <= maxbits; ++i) p.bucket[i] = 0;
  int32_t E = -(int32_t)(1u << maxbits);
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t d = p.par[i] < maxbits ? p.par[i] : maxbits;
    ++p.bucket[d];
    E += (int32_t)(1u << (maxbits - d));
  }
  while (E > 0) {  // lengthen the longest code below the limit (there is one: the sum is above 1)
    uint32_t bits = maxbits - 1u;
    while (bits > 0u && !p.bucket[bits]) --bits;
    if (bits == 0u) break;
    --p.bucket[bits];
    ++p.bucket[bits + 1u];
    E -= (int32_t)(1u << (maxbits - bits - 1u));
  }
  while (E < 0) {  // shorten the code that gives back the most without passing 1 (the longest length's unit divides -E)
    uint32_t bits = 2u;
    while (bits <= maxbits && !(p.bucket[bits] && (int32_t)(1u << (maxbits - bits)) <= -E)) ++bits;
    if (bits > maxbits) break;
    --p.bucket[bits];
    ++p.bucket[bits - 1u];
    E += (int32_t)(1u << (maxbits - bits));
  }
  // the rarest symbols get the longest codes
  uint32_t i = 0;
  for (uint32_t bits = maxbits; bits >= 1u; --bits)
    for (uint32_t c = p.bucket[bits]; c; --c) lens[p.a[i++]] = (uint8_t)bits;
}

// canonical codes (RFC 1951 3.2.2), bit-reversed
VDS_DEF_HD void def_build_codes(DeflPlan &p, const uint8_t *lens, uint32_t n, uint16_t *codes) {
  for (uint32_t i = 0; i < 32u; ++i) p.bucket[i] = 0;
  for (uint32_t s = 0; s < n; ++s) ++p.bucket[lens[s]];
  p.bucket[0] = 0;
  uint32_t code = 0;
  for (uint32_t l = 1; l <= 15u; ++l) {
    code = (code + p.bucket[l - 1u]) << 1;
    p.bucket[16u + l] = (uint16_t)code;
  }
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t l = lens[s];
    codes[s] = l ? (uint16_t)inf_brev(p.bucket[16u + l]++, l) : (uint16_t)0;
  }
}

VDS_DEF_HD uint32_t def_cl_order(uint32_t i) {
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return order[i];
}

// The dynamic block of the segment whose tokens lfreq and dfreq count.  The
// final-block bit (bit 0 of hdr[0]) is left 0 for the writer.
VDS_DEF_HD void def_plan(DeflPlan &p) {
  p.lfreq[256] = 1;
  def_build_lengths(p, p.lfreq, kDefLitSyms, 15, p.llen);
  def_build_codes(p, p.llen, kDefLitSyms, p.lcode);
  def_build_lengths(p, p.dfreq, kDefDistSyms, 15, p.dlen);
  def_build_codes(p, p.dlen, kDefDistSyms, p.dcode);
  uint32_t nlen = kDefLitSyms, ndist = kDefDistSyms;
  while (nlen > 257u && !p.llen[nlen - 1u]) --nlen;
  while (ndist > 1u && !p.dlen[ndist - 1u]) --ndist;
  // the lengths of both codes as one sequence, run-length coded: 16 repeats the
  // length before 3..6 times, 17 is 3..10 zeros, 18 is 11..138 zeros.  A step
  // consumes a whole run, so at most nlen + ndist steps and as many items.
  const uint32_t total = nlen + ndist;
  for (uint32_t i = 0; i < kDefClSyms; ++i) p.clfreq[i] = 0;
  uint32_t ncls = 0;
  for (uint32_t i = 0; i < total;) {
    const uint32_t v = i < nlen ? p.llen[i] : p.dlen[i - nlen];
    uint32_t run = 1;
    while (i + run < total && (i + run < nlen ? p.llen[i + run] : p.dlen[i + run - nlen]) == v) ++run;
    i += run;
    if (v == 0u) {
      while (run >= 11u) {
        const uint32_t t = run < 138u ? run : 138u;
        p.cls[ncls++] = (uint16_t)(18u | ((t - 11u) << 8));
        ++p.clfreq[18];
        run -= t;
      }
      if (run >= 3u) {
        p.cls[ncls++] = (uint16_t)(17u | ((run - 3u) << 8));
        ++p.clfreq[17];
        run = 0;
      }
    } else {
      p.cls[ncls++] = (uint16_t)v;
      ++p.clfreq[v];
      --run;
      while (run >= 3u) {
        const uint32_t t = run < 6u ? run : 6u;
        p.cls[ncls++] = (uint16_t)(16u | ((t - 3u) << 8));
        ++p.clfreq[16];
        run -= t;
      }
    }
    for (; run; --run) {
      p.cls[ncls++] = (uint16_t)v;
      ++p.clfreq[v];
    }
  }
  def_build_lengths(p, p.clfreq, kDefClSyms, 7, p.cllen);
  def_build_codes(p, p.cllen, kDefClSyms, p.clcode);
  uint32_t ncode = kDefClSyms;
  while (ncode > 4u && !p.cllen[def_cl_order(ncode - 1u)]) --ncode;
  uint32_t bits = 17u + 3u * ncode;
  p.hdr[0] = (2u << 1) | ((nlen - 257u) << 3) | ((ndist - 1u) << 8) | ((ncode - 4u) << 13) | (17u << 24);
  for (uint32_t i = 0; i < ncode; ++i) p.hdr[1u + i] = p.cllen[def_cl_order(i)] | (3u << 24);
  for (uint32_t i = 0; i < ncls; ++i) {
    const uint32_t sym = p.cls[i] & 0xFFu, ev = p.cls[i] >> 8;
    const uint32_t eb = sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u;
    const uint32_t l = p.cllen[sym];
    p.hdr[1u + ncode + i] = p.clcode[sym] | (ev << l) | ((l + eb) << 24);
    bits += l + eb;
  }
  p.nhdr = 1u + ncode + ncls;
  for (uint32_t s = 0; s < kDefLitSyms; ++s) bits += p.lfreq[s] * (p.llen[s] + def_len_extra(s));
  for (uint32_t s = 0; s < kDefDistSyms; ++s) bits += p.dfreq[s] * (p.dlen[s] + def_dist_extra(s));
  p.dyn_bits = bits;
}

// a token's bits and their number (at most 48) under the plan's codes
VDS_DEF_HD uint64_t def_token_bits(const DeflPlan &p, uint32_t tok, uint32_t *nbits) {
  if (!(tok & 0x80000000u)) {
    *nbits = p.llen[tok];
    return p.lcode[tok];
  }
  uint32_t leb, lev, deb, dev;
  const uint32_t ls = def_len_sym(((tok >> 16) & 0xFFu) + 3u, &leb, &lev);
  const uint32_t ds = def_dist_sym((tok & 0x7FFFu) + 1u, &deb, &dev);
  const uint32_t ll = p.llen[ls], dl = p.dlen[ds];
  uint64_t v = p.lcode[ls] | ((uint64_t)lev << ll);
  v |= ((uint64_t)p.dcode[ds] | ((uint64_t)dev << dl)) << (ll + leb);
  *nbits = ll + leb + dl + deb;
  return v;
}

}  // namespace vds_ec
