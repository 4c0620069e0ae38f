// inflate_common.hpp -- what the device inflate (inflate.hip) and the host one
// (inflate_host.cpp) share: the two-level decoding table's entry, the rule that
// sizes a second-level table, the fill of one symbol's entries, and the
// length / distance bases.  Plain C++ for the host unit, __host__ __device__
// under HIP.
//
// A table decodes a canonical Huffman code read least significant bit first
// (RFC 1951 3.2.2).  The first level is indexed by the next `root` bits.  A
// code of at most `root` bits owns every first-level entry whose low bits are
// its bit-reversed code.  The codes longer than `root` bits that share their
// first `root` bits p own one second-level table of 2^(L_p - root) entries,
// L_p the longest of them, indexed by the bits behind the first `root`; the
// first-level entry of p links to it.  This is zlib's layout (inftrees.c), so
// its bounds hold: 852 entries for 286 literal/length symbols at root 9, 592
// for 30 distance symbols at root 6.  An entry is 16 bits.
#pragma once

#include <cstdint>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define VDS_INF_HD __host__ __device__ __forceinline__
#else
#define VDS_INF_HD inline
#endif

namespace vds_ec {

constexpr uint32_t kInfLitRoot = 9, kInfDistRoot = 6, kInfClRoot = 7;
constexpr uint32_t kInfLitCap = 852, kInfDistCap = 592, kInfClCap = 128;
constexpr uint32_t kInfFixLitCap = 512, kInfFixDistCap = 64;
constexpr uint32_t kInfMaxSyms = 320;  // 288 literal/length + 32 distance lengths of one block
constexpr uint32_t kAdlerMod = 65521u;

// entry: bits 0..3 the bits this level consumes (a link: the bits that index
// its second-level table), bits 4..5 the kind, bits 6..15 the symbol (at most
// 287) or, in a link, the second-level table's first entry (below 852)
typedef uint16_t inf_entry_t;
constexpr uint32_t kInfSym = 0, kInfLink = 1, kInfInvalid = 2;
VDS_INF_HD inf_entry_t inf_entry(uint32_t kind, uint32_t nbits, uint32_t val) {
  return (inf_entry_t)(nbits | (kind << 4) | (val << 6));
}
VDS_INF_HD uint32_t inf_nbits(uint32_t e) { return e & 15u; }
VDS_INF_HD uint32_t inf_kind(uint32_t e) { return (e >> 4) & 3u; }
VDS_INF_HD uint32_t inf_val(uint32_t e) { return e >> 6; }
// zlib's entry for a code that does not exist: one bit, then "invalid code"
constexpr inf_entry_t kInfInvalidEntry = 1u | (kInfInvalid << 4);

// the low `len` bits of `code`, reversed (len in 1..15)
VDS_INF_HD uint32_t inf_brev(uint32_t code, uint32_t len) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < 15u; ++i)
    if (i < len) r |= ((code >> i) & 1u) << (len - 1u - i);
  return r;
}

// L_p of the first `root` bits p (most significant bit first) of a code whose
// lengths occur count[l] times and start at the canonical code first[l]: the
// longest length above root with a code in p, 0 if there is none.  In
// left-aligned 15-bit terms the codes of length l are the range
// [first[l] << (15 - l), (first[l] + count[l]) << (15 - l)) and p is
// [p << (15 - root), (p + 1) << (15 - root)).
template <typename Arr>
VDS_INF_HD uint32_t inf_sub_len(const Arr &count, const Arr &first, uint32_t root, uint32_t p) {
  const uint32_t s = 15u - root, lo_p = p << s, hi_p = (p + 1u) << s;
  uint32_t L = 0;
  for (uint32_t l = root + 1u; l <= 15u; ++l) {
    const uint32_t c = count[l];
    if (!c) continue;
    const uint32_t lo = first[l] << (15u - l), hi = (first[l] + c) << (15u - l);
    if (lo < hi_p && hi > lo_p) L = l;
  }
  return L;
}

// Every entry of symbol `sym`, whose code is the `len` bits of `code`: in the
// first level, or in the second-level table its first-level entry links to
// (written before this is called).  No entry at or past `cap` is written.
VDS_INF_HD void inf_fill_symbol(inf_entry_t *T, uint32_t cap, uint32_t root, uint32_t sym, uint32_t len, uint32_t code) {
  const uint32_t rc = inf_brev(code, len);
  if (len <= root) {
    const inf_entry_t e = inf_entry(kInfSym, len, sym);
    for (uint32_t i = rc; i < (1u << root); i += 1u << len) T[i] = e;  // at most 2^(root - 1) entries
    return;
  }
  const uint32_t link = T[rc & ((1u << root) - 1u)];
  if (inf_kind(link) != kInfLink) return;  // (cannot be: the allocation covers every long code)
  const uint32_t sub = inf_val(link), sb = inf_nbits(link), l2 = len - root;
  const inf_entry_t e = inf_entry(kInfSym, l2, sym);
  for (uint32_t i = rc >> root; i < (1u << sb); i += 1u << l2)  // at most 2^5 entries
    if (sub + i < cap) T[sub + i] = e;
}

// length symbol 257..285 -> base and extra bits; distance symbol 0..29 likewise (RFC 1951 3.2.5)
VDS_INF_HD uint32_t inf_len_base(uint32_t sym, uint32_t *extra) {
  if (sym < 265u) {
    *extra = 0;
    return sym - 254u;
  }
  if (sym == 285u) {
    *extra = 0;
    return 258u;
  }
  const uint32_t e = (sym - 261u) >> 2;
  *extra = e;
  return ((4u + ((sym - 265u) & 3u)) << e) + 3u;
}
VDS_INF_HD uint32_t inf_dist_base(uint32_t sym, uint32_t *extra) {
  if (sym < 4u) {
    *extra = 0;
    return sym + 1u;
  }
  const uint32_t e = (sym >> 1) - 1u;
  *extra = e;
  return ((2u + (sym & 1u)) << e) + 1u;
}

// the order in which a dynamic block stores the code-length code's lengths
constexpr uint8_t kInfClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

}  // namespace vds_ec
