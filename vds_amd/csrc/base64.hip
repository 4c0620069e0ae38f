// base64.hip -- the wire text of the upload and download loops on the device.
//
// The websocket "upload" carries its body as base64 (websocket_api.cpp:141-155
// -> base64::to_bytes, encoding.cpp:181-247) and "download" answers in base64
// (base64::from_bytes, encoding.cpp:138-174).  The text crosses PCIe into the
// staging anyway, so it is decoded in front of the batched save_temp and
// encoded behind the batched restore, where the bytes already are.
//
// k_b64_decode_batch: `count` texts of different lengths in one launch, ONE
// WAVE PER MESSAGE.  Per message the result is what vds_ec_base64_decode
// (vds_ec_wire.cpp) gives, the reference's quirks included: the output size is
// len/4*3 minus the '=' among the LAST TWO characters; characters are consumed
// in order; the first '=' met, wherever it stands, ends the decode and emits
// one or two bytes of the running 32-bit accumulator (never reset between
// quanta, so an '=' at an odd place draws on the characters before it); any
// other character outside the alphabet met before it is an error; the bytes
// the host code leaves unwritten are zero.  "Where is the first event" is the
// only sequential question: a step takes 16 characters a lane (kB64DecStep =
// 1024 characters a wave), a ballot of the lanes that saw a character outside
// the alphabet gives the first event, the lanes before it store their 12 bytes,
// and the event is finished by the wave (no atomics, no LDS, no second launch).
// A text of many MiB walked by one wave is slow -- accepted: the shape that
// matters is bodies of up to 64 KiB by the thousand, longest first.
//
// k_b64_encode_batch: `count` inputs of different lengths, tiled over the whole
// batch (kB64EncTile input bytes a wave, 12 a lane a step); nothing is
// sequential, so long inputs are split across waves.
// k_b64_encode_batch<true>: the same behind verdict bytes (the download
// loop's check): a message whose gate bytes are not all zero gets no character
// written and VDS_EC_ECORRUPT in its status slot.
//
// Both take texts, inputs and outputs at any byte address: only the aligned
// 4-byte words holding at least one input byte are read, and only the output's
// own bytes are written (a lane's piece that is not dword-aligned goes out as
// head and tail bytes round realigned dwords, a partial piece as bytes).  The fast path is a 16-byte aligned text and a 4-byte aligned
// output, which the host form always produces.  Characters map to sextets (and
// back) with compares and selects; bytes are packed with v_perm_b32.
#include <hip/hip_runtime.h>

#include "../../include/vds_ec.h"
#include "ec_internal.hpp"

namespace vds_ec {

namespace {

// (the addresses come from the tables as integers: global pointers made from
// them keep the loads and stores global_* rather than flat_*)
typedef const __attribute__((address_space(1))) uint32_t *gptr_u32;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4 *gptr_u128;
typedef __attribute__((address_space(1))) uint32_t *gptr_w32;
typedef __attribute__((address_space(1))) uint8_t *gptr_w8;
typedef __attribute__((address_space(1))) int32_t *gptr_wi32;

// character -> sextet, 0xFF for anything outside the alphabet ('=' included)
__device__ __forceinline__ uint32_t sextet(uint32_t c) {
  uint32_t s = 0xFFu;
  s = c - 'A' < 26u ? c - 'A' : s;
  s = c - 'a' < 26u ? c - 'a' + 26u : s;
  s = c - '0' < 10u ? c - '0' + 52u : s;
  s = c == '+' ? 62u : s;
  s = c == '/' ? 63u : s;
  return s;
}

// four characters (first in the low byte) -> the quantum's 24 bits; bit i of
// *bad set when character i is outside the alphabet
__device__ __forceinline__ uint32_t quantum(uint32_t w, uint32_t *bad) {
  const uint32_t s0 = sextet(w & 0xFFu), s1 = sextet((w >> 8) & 0xFFu), s2 = sextet((w >> 16) & 0xFFu),
                 s3 = sextet(w >> 24);
  *bad = (s0 >> 7) | ((s1 >> 7) << 1) | ((s2 >> 7) << 2) | ((s3 >> 7) << 3);
  return ((s0 & 63u) << 18) | ((s1 & 63u) << 12) | ((s2 & 63u) << 6) | (s3 & 63u);
}

// the byte at address a, from its aligned word
__device__ __forceinline__ uint32_t byte_at(uint64_t a) {
  return (*reinterpret_cast<gptr_u32>(a & ~3ull) >> (8u * (uint32_t)(a & 3u))) & 0xFFu;
}

// A lane's 16 characters of step `it`: characters c0 .. c0 + 15, c0 = 1024 it +
// 16 lane, of a text of len (a multiple of 4) characters at p + sh (p 4-byte
// aligned, sh < 4).  Characters past the end come back as anything.
__device__ __forceinline__ u32x4 load_chars(uint64_t text, gptr_u32 p, uint32_t sh, uint32_t len, uint64_t c0) {
  u32x4 w = {0u, 0u, 0u, 0u};
  if ((text & 15u) == 0 && c0 + 16u <= len) {
    w = *reinterpret_cast<gptr_u128>(text + c0);
  } else if (c0 < len) {
    // aligned words at byte offsets < lim hold a character of the text
    const uint64_t lim = (uint64_t)len + sh;
    const uint64_t q = c0 / 4;
    uint32_t raw[5];
#pragma unroll
    for (int i = 0; i < 4; ++i) raw[i] = 4 * (q + i) < lim ? p[q + i] : 0u;
    raw[4] = sh && 4 * (q + 4) < lim ? p[q + 4] : 0u;
    const uint32_t sel = 0x03020100u + 0x01010101u * sh;
    w.x = __builtin_amdgcn_perm(raw[1], raw[0], sel);
    w.y = __builtin_amdgcn_perm(raw[2], raw[1], sel);
    w.z = __builtin_amdgcn_perm(raw[3], raw[2], sel);
    w.w = __builtin_amdgcn_perm(raw[4], raw[3], sel);
  }
  return w;
}

// The first nb bytes of w[0..NW) to address a.  A whole run goes out as dwords:
// at once when a is 4-byte aligned, else its head up to the next aligned
// address and its tail as bytes and the NW - 1 dwords between them realigned
// with v_perm_b32.  A partial run (a message's last lane, the lane of the
// first event) goes out as bytes.
template <int NW>
__device__ __forceinline__ void store_run(uint64_t a, const uint32_t (&w)[NW], uint32_t nb) {
  const uint32_t mis = (uint32_t)(a & 3u);
  if (nb == 4u * NW && mis == 0) {
    const gptr_w32 d = reinterpret_cast<gptr_w32>(a);
#pragma unroll
    for (int i = 0; i < NW; ++i) d[i] = w[i];
  } else if (nb == 4u * NW) {
    const uint32_t h = 4u - mis;  // head bytes; the tail is mis bytes
    const gptr_w8 b = reinterpret_cast<gptr_w8>(a);
    const gptr_w32 d = reinterpret_cast<gptr_w32>(a + h);
    const uint32_t sel = 0x03020100u + 0x01010101u * h;
#pragma unroll
    for (uint32_t i = 0; i < 3; ++i)
      if (i < h) b[i] = (uint8_t)(w[0] >> (8 * i));
#pragma unroll
    for (int i = 0; i + 1 < NW; ++i) d[i] = __builtin_amdgcn_perm(w[i + 1], w[i], sel);
#pragma unroll
    for (uint32_t i = 0; i < 3; ++i)
      if (i < mis) b[h + 4 * (NW - 1) + i] = (uint8_t)(w[NW - 1] >> (8 * (h + i)));
  } else {
    const gptr_w8 b = reinterpret_cast<gptr_w8>(a);
#pragma unroll
    for (int i = 0; i < 4 * NW; ++i)
      if ((uint32_t)i < nb) b[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
  }
}

// MASKED (texts still under their websocket mask, websocket.cpp:162-171):
// masks[blockIdx.x] beside msgs[blockIdx.x], the four mask bytes of the text's
// characters 0..3 in a little-endian word; character j is byte j of the text
// ^ mask byte j & 3.  Everything the kernel looks at is unmasked first.  A
// lane's 16 characters start at a multiple of 16, so once load_chars has
// realigned them every dword of the 16 takes the same word.  Unmasked, `masks`
// is not read and the kernel is the one it was before the mask existed.
// (a: the character's address, j: its index in the text modulo 4)
template <bool MASKED>
__device__ __forceinline__ uint32_t char_at(uint64_t a, uint32_t j, uint32_t mk) {
  const uint32_t c = byte_at(a);
  if constexpr (MASKED) return c ^ ((mk >> (8u * (j & 3u))) & 0xFFu);
  return c;
}

template <bool MASKED>
__global__ __launch_bounds__(64) void k_b64_decode_batch(const B64DecMsg *msgs, const uint32_t *masks) {
  const B64DecMsg m = msgs[blockIdx.x];
  uint32_t mk = 0;
  if constexpr (MASKED) mk = masks[blockIdx.x];
  const uint32_t lane = threadIdx.x;
  const uint32_t len = m.len;
  const gptr_wi32 status = reinterpret_cast<gptr_wi32>(m.status);
  if (len % 4) {
    if (lane == 0) *status = VDS_EC_EB64_LENGTH;
    return;
  }
  if (len == 0) {
    if (lane == 0) *status = VDS_EC_OK;
    return;
  }
  // the '=' among the last two characters against the size the caller declared
  const uint32_t padding =
      char_at<MASKED>(m.text + len - 1, len - 1, mk) != '='   ? 0u
      : char_at<MASKED>(m.text + len - 2, len - 2, mk) != '=' ? 1u
                                                              : 2u;
  if (len / 4 * 3 - padding != m.size) {
    if (lane == 0) *status = VDS_EC_EINVAL;
    return;
  }
  const uint32_t sh = (uint32_t)(m.text & 3u);
  const gptr_u32 p = reinterpret_cast<gptr_u32>(m.text - sh);
  const uint32_t steps = (len - 1) / kB64DecStep + 1;
  u32x4 nx = load_chars(m.text, p, sh, len, 16u * lane);
  for (uint32_t it = 0; it < steps; ++it) {
    u32x4 w = nx;
    if constexpr (MASKED) w ^= mk;
    const uint64_t c0 = (uint64_t)it * kB64DecStep + 16u * lane;
    if (it + 1 < steps) nx = load_chars(m.text, p, sh, len, c0 + kB64DecStep);
    uint32_t b[4], t[4];
    t[0] = quantum(w.x, &b[0]);
    t[1] = quantum(w.y, &b[1]);
    t[2] = quantum(w.z, &b[2]);
    t[3] = quantum(w.w, &b[3]);
    // the lane's characters inside the text: 0, 4, 8, 12 or 16
    const uint32_t valid = c0 < len ? (uint32_t)min((uint64_t)16, len - c0) : 0u;
    const uint32_t bad = (b[0] | (b[1] << 4) | (b[2] << 8) | (b[3] << 12)) & ((1u << valid) - 1u);
    uint32_t o[3];
    o[0] = __builtin_amdgcn_perm(t[1], t[0], 0x06000102u);
    o[1] = __builtin_amdgcn_perm(t[2], t[1], 0x05060001u);
    o[2] = __builtin_amdgcn_perm(t[3], t[2], 0x04050600u);
    const uint64_t dst = m.out + (uint64_t)(c0 / 4) * 3;
    const unsigned long long events = __ballot(bad != 0);
    if (events == 0) {
      store_run(dst, o, valid / 4 * 3);
      continue;
    }
    // The first event: character e of lane fl.  The lanes before it hold whole
    // quanta of the alphabet; lane fl its quanta before the event's.
    const uint32_t fl = (uint32_t)__builtin_ctzll(events);
    const uint32_t e = (uint32_t)__shfl((int)(__builtin_ctz(bad | 0x10000u)), (int)fl);
    const uint32_t pos = it * kB64DecStep + 16u * fl + e;
    if (char_at<MASKED>(m.text + pos, pos, mk) != '=') {
      if (lane == 0) *status = VDS_EC_EB64_CHAR;
      return;
    }
    if (padding == 0) {
      if (lane == 0) *status = VDS_EC_EB64_PADDING;
      return;
    }
    store_run(dst, o, lane < fl ? 12u : lane == fl ? e / 4 * 3 : 0u);
    // the accumulator after this step's shift: the three characters before
    // the '=' (of the alphabet; nothing before the text) reach bits 8..23
    uint32_t temp = 0;
#pragma unroll
    for (uint32_t j = 1; j <= 3; ++j)
      if (pos >= j) temp |= (sextet(char_at<MASKED>(m.text + pos - j, pos - j, mk)) & 63u) << (6u * j);
    const uint32_t off = pos / 4 * 3;
    const gptr_w8 out = reinterpret_cast<gptr_w8>(m.out);
    if (lane == 0) {
      if (padding == 1) {
        out[off] = (uint8_t)(temp >> 16);
        out[off + 1] = (uint8_t)(temp >> 8);
      } else {
        out[off] = (uint8_t)(temp >> 10);
      }
    }
    // what the host code leaves unwritten is zero
    for (uint64_t i = (uint64_t)off + 3 - padding + lane; i < m.size; i += 64) out[i] = 0;
    break;
  }
  if (lane == 0) *status = VDS_EC_OK;
}

// sextet -> character
__device__ __forceinline__ uint32_t b64_char(uint32_t s) {
  uint32_t d = 65u;  // 'A' - 0
  d = s >= 26u ? 71u : d;               // 'a' - 26
  d = s >= 52u ? (uint32_t)-4 : d;      // '0' - 52
  d = s == 62u ? (uint32_t)-19 : d;     // '+' - 62
  d = s == 63u ? (uint32_t)-16 : d;     // '/' - 63
  return (s + d) & 0xFFu;
}

// 24 bits -> four characters, first in the low byte
__device__ __forceinline__ uint32_t b64_chars(uint32_t t) {
  return b64_char((t >> 18) & 63u) | (b64_char((t >> 12) & 63u) << 8) | (b64_char((t >> 6) & 63u) << 16) |
         (b64_char(t & 63u) << 24);
}

// GATED (the download loop's last launch): gates[tl.msg] beside msgs[tl.msg].
// Before it writes anything a wave ORs its message's ngate gate bytes (64 a
// step, then one ballot over the wave); with any of them non-zero no tile of
// the message writes a character.  The wave of the message's tile 0 -- every
// message has one, an empty message too -- writes the status.  The gate bytes
// come from an earlier launch on the same stream: stream order is all the
// ordering needed.  Ungated, `gates` is not read and the kernel is the one it
// was before the gate existed.
template <bool GATED>
__global__ __launch_bounds__(256) void k_b64_encode_batch(const B64EncMsg *msgs, const B64EncTile *tiles,
                                                          uint32_t ntiles, const B64EncGate *gates) {
  const uint32_t wv = blockIdx.x * 4u + threadIdx.x / 64u;
  if (wv >= ntiles) return;  // (wave-uniform: every lane of a wave that goes on takes part in the ballot)
  const uint32_t lane = threadIdx.x % 64u;
  const B64EncTile tl = tiles[wv];
  if constexpr (GATED) {
    const B64EncGate g = gates[tl.msg];
    uint32_t any = 0;
    for (uint32_t i = lane; i < g.ngate; i += 64u) any |= byte_at(g.gate + i);
    const bool shut = __ballot(any != 0) != 0ull;
    if (tl.tile == 0 && lane == 0) *reinterpret_cast<gptr_wi32>(g.status) = shut ? VDS_EC_ECORRUPT : VDS_EC_OK;
    if (shut) return;
  }
  const B64EncMsg m = msgs[tl.msg];
  const uint64_t len = m.len;
  const uint32_t sh = (uint32_t)(m.in & 3u);
  const gptr_u32 p = reinterpret_cast<gptr_u32>(m.in - sh);
  const uint64_t lim = len + sh;  // aligned words at byte offsets < lim hold an input byte
  const uint32_t sel = 0x03020100u + 0x01010101u * sh;
  const uint64_t t0 = (uint64_t)tl.tile * kB64EncTile;
#pragma unroll 2
  for (uint32_t it = 0; it < kB64EncTile / 768u; ++it) {
    const uint64_t b0 = t0 + it * 768u + 12u * lane;  // the lane's 12 bytes
    if (b0 >= len) break;
    const uint32_t valid = (uint32_t)min((uint64_t)12, len - b0);
    const uint64_t q = b0 / 4;
    uint32_t raw[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) raw[i] = 4 * (q + i) < lim ? p[q + i] : 0u;
    raw[3] = sh && 4 * (q + 3) < lim ? p[q + 3] : 0u;
    uint32_t d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      d[i] = __builtin_amdgcn_perm(raw[i + 1], raw[i], sel);
      const int c = (int)valid - 4 * i;  // input bytes left at this word: those past the end count as zero
      if (c < 4) d[i] = c <= 0 ? 0u : d[i] & (0xFFFFFFFFu >> (8 * (4 - c)));
    }
    uint32_t ch[4];
    ch[0] = b64_chars(__builtin_amdgcn_perm(0u, d[0], 0x0c000102u));
    ch[1] = b64_chars(__builtin_amdgcn_perm(d[1], d[0], 0x0c030405u));
    ch[2] = b64_chars(__builtin_amdgcn_perm(d[2], d[1], 0x0c020304u));
    ch[3] = b64_chars(__builtin_amdgcn_perm(0u, d[2], 0x0c010203u));
    // the last group of an input of 3 g + 1 or 3 g + 2 bytes ends in '='
    const uint32_t groups = (valid + 2u) / 3u;
    if (valid % 3u) {
      const uint32_t pad = valid % 3u == 1u ? 0x3D3D0000u : 0x3D000000u;
      const uint32_t keep = valid % 3u == 1u ? 0x0000FFFFu : 0x00FFFFFFu;
#pragma unroll
      for (uint32_t g = 0; g < 4; ++g)
        if (g + 1 == groups) ch[g] = (ch[g] & keep) | pad;
    }
    store_run(m.out + b0 / 3 * 4, ch, 4u * groups);
  }
}

// The first nb <= 4 NW bytes of w[0..NW) to address a, any nb: the head up to
// the next aligned address and the tail as bytes, the dwords between them
// realigned with v_perm_b32.
template <int NW>
__device__ __forceinline__ void store_any(uint64_t a, const uint32_t (&w)[NW], uint32_t nb) {
  const uint32_t h = min((uint32_t)(-a) & 3u, nb);  // head bytes
  const gptr_w8 b = reinterpret_cast<gptr_w8>(a);
#pragma unroll
  for (uint32_t i = 0; i < 3; ++i)
    if (i < h) b[i] = (uint8_t)(w[0] >> (8 * i));
  const uint32_t nd = (nb - h) / 4;  // whole dwords behind the head
  const gptr_w32 d = reinterpret_cast<gptr_w32>(a + h);
  const uint32_t sel = 0x03020100u + 0x01010101u * h;
  uint32_t tw = 0;  // the dword behind them, of which the tail is the low bytes
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const uint32_t v = __builtin_amdgcn_perm(i + 1 < NW ? w[i + 1] : 0u, w[i], sel);
    if ((uint32_t)i < nd) d[i] = v;
    if ((uint32_t)i == nd) tw = v;
  }
  const uint32_t t0 = h + 4 * nd;
#pragma unroll
  for (uint32_t i = 0; i < 3; ++i)
    if (t0 + i < nb) b[t0 + i] = (uint8_t)(tw >> (8 * i));
}

// The 44 characters of a 32-byte digest at any address d (base64::from_bytes:
// ten groups of three bytes, then two bytes and one '='), first character in
// the low byte of ch[0].  Reads the aligned words holding a digest byte.
__device__ __forceinline__ void digest_chars(uint64_t dg, uint32_t (&ch)[11]) {
  const uint32_t sh = (uint32_t)(dg & 3u);
  const gptr_u32 p = reinterpret_cast<gptr_u32>(dg - sh);
  const uint32_t sel = 0x03020100u + 0x01010101u * sh;
  uint32_t raw[9], d[9];
#pragma unroll
  for (int i = 0; i < 8; ++i) raw[i] = p[i];
  raw[8] = sh ? p[8] : 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) d[i] = __builtin_amdgcn_perm(raw[i + 1], raw[i], sel);
  d[8] = 0u;
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    const int i = 3 * g, c = 4 * g;
    ch[c] = b64_chars(__builtin_amdgcn_perm(0u, d[i], 0x0c000102u));
    ch[c + 1] = b64_chars(__builtin_amdgcn_perm(d[i + 1], d[i], 0x0c030405u));
    ch[c + 2] = b64_chars(__builtin_amdgcn_perm(d[i + 2], d[i + 1], 0x0c020304u));
    if (g < 2) ch[c + 3] = b64_chars(__builtin_amdgcn_perm(0u, d[i + 2], 0x0c010203u));
  }
  ch[10] = (ch[10] & 0x00FFFFFFu) | 0x3D000000u;  // bytes 30, 31 and one '='
}

// k_ws_upload_answer_batch: the "upload" answers of `count` messages as
// websocket frames (vds_ec_ws_frame_header + vds_ec_upload_response_json), ONE
// WAVE PER MESSAGE.  Every name is 44 characters, so with the frame header and
// the digits of the id (m.head) and of the replica size (m.tail) given, every
// piece has its place: lane i < n writes "<name i>" and the comma behind it
// (none behind the last), lane n the head, ],"hash":"<body hash> and the tail.
// A lane encodes one digest and waits for no other.
__global__ __launch_bounds__(256) void k_ws_upload_answer_batch(const WsAnsMsg *msgs, uint32_t count) {
  const uint32_t wv = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + threadIdx.x / 64u);
  if (wv >= count) return;
  const uint32_t lane = threadIdx.x % 64u;
  const WsAnsMsg *m = msgs + wv;
  const uint32_t n = m->n, hl = m->head_len;
  const uint64_t out = m->out;
  for (uint32_t i = lane; i <= n; i += 64u) {
    uint32_t ch[11];
    if (i < n) {
      digest_chars(m->rdig + 32ull * i, ch);
      uint32_t w[12];
      w[0] = '"' | (ch[0] << 8);
#pragma unroll
      for (int j = 1; j < 11; ++j) w[j] = (ch[j - 1] >> 24) | (ch[j] << 8);
      w[11] = (ch[10] >> 24) | ('"' << 8) | (',' << 16);
      store_any(out + hl + 47ull * i, w, i + 1 < n ? 47u : 46u);
    } else {
      uint32_t hw[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) hw[j] = m->head[j];
      store_any(out, hw, hl);
      digest_chars(m->ddig, ch);
      uint32_t w[22];
      w[0] = 0x68222C5Du;  // ],"h
      w[1] = 0x22687361u;  // ash"
      w[2] = 0x0000223Au | (ch[0] << 16);  // :"
#pragma unroll
      for (int j = 1; j < 11; ++j) w[2 + j] = (ch[j - 1] >> 16) | (ch[j] << 16);
      w[13] = (ch[10] >> 16) | (m->tail[0] << 16);
#pragma unroll
      for (int j = 0; j < 8; ++j) w[14 + j] = (m->tail[j] >> 16) | (m->tail[j + 1] << 16);
      store_any(out + hl + (n ? 47ull * n - 1 : 0), w, 54u + m->tail_len);
    }
  }
}

}  // namespace

hipError_t launch_b64_decode_batch(const B64DecMsg *msgs, uint32_t count, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_b64_decode_batch<false>, dim3(count), dim3(64), 0, s, msgs,
                     static_cast<const uint32_t *>(nullptr));
  return hipGetLastError();
}

hipError_t launch_b64_decode_masked_batch(const B64DecMsg *msgs, const uint32_t *masks, uint32_t count,
                                          hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_b64_decode_batch<true>, dim3(count), dim3(64), 0, s, msgs, masks);
  return hipGetLastError();
}

hipError_t launch_ws_upload_answer_batch(const WsAnsMsg *msgs, uint32_t count, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ws_upload_answer_batch, dim3((count + 3) / 4), dim3(256), 0, s, msgs, count);
  return hipGetLastError();
}

hipError_t launch_b64_encode_batch(const B64EncMsg *msgs, const B64EncTile *tiles, uint32_t ntiles, hipStream_t s) {
  if (ntiles == 0) return hipSuccess;
  hipLaunchKernelGGL(k_b64_encode_batch<false>, dim3((ntiles + 3) / 4), dim3(256), 0, s, msgs, tiles, ntiles,
                     static_cast<const B64EncGate *>(nullptr));
  return hipGetLastError();
}

hipError_t launch_b64_encode_gated_batch(const B64EncMsg *msgs, const B64EncGate *gates, const B64EncTile *tiles,
                                         uint32_t ntiles, hipStream_t s) {
  if (ntiles == 0) return hipSuccess;
  hipLaunchKernelGGL(k_b64_encode_batch<true>, dim3((ntiles + 3) / 4), dim3(256), 0, s, msgs, tiles, ntiles, gates);
  return hipGetLastError();
}

}  // namespace vds_ec
