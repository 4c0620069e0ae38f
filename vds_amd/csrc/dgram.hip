// dgram.hip -- the node-to-node datagram layer on the device.
//
// A replica crosses between nodes as a sync_replica_data message
// (sync_process.cpp:184-191, messages/sync_messages.h:311-330) that
// dht_datagram_protocol::prepare_to_send (impl/dht_datagram_protocol.cpp:335-541)
// cuts into datagrams of at most mtu bytes, each signed with HMAC-SHA256 under
// the session key; the receiver verifies every datagram (:130-141) and
// stitches the payloads together (:544-769).  Three kernels, one lane per
// message or datagram:
//   k_hmac_sha256_batch  HMAC of messages of different lengths, optionally
//                        compared with expected bytes (verdict 0 / 1);
//   k_dgram_seal         header, payload slice and MAC of one datagram, from
//                        its message's descriptor;
//   k_dgram_open         MAC over len - 32 bytes against the last 32, one
//                        verdict byte, and the payload copied to where the
//                        message is assembled ONLY when the datagram verified
//                        (by the whole wave, datagram after datagram; the
//                        one-lane-per-datagram copy it is measured against is
//                        kept as k_dgram_open<false>, VDS_EC_DGRAM_COPY=lane).
//
// A lane sees its MAC input as a stream of bytes: up to 9 header bytes it
// holds in registers, then runs of bytes that live in memory at any alignment
// (the route blob, the payload).  Each 64-byte block of the stream is
// assembled as the hash kernels do it -- aligned dwords, one v_perm_b32 per
// big-endian word -- masked at the runs' ends; only aligned dwords holding at
// least one byte of a run are read.  The seal lane stores the very words it
// hashes, so it reads its slice once.  The key pads are not hashed here: the
// host supplies each session's two midstates (HmacKeyState, ec_internal.hpp).
#include <hip/hip_runtime.h>

#include "ec_internal.hpp"
#include "sha256_device.hpp"

// -DVDS_DGRAM_STORE_X4=0: the seal stores whole blocks dword by dword even into
// 16-byte aligned slots (the A/B of DESIGN.md 6; see 3.10).
#ifndef VDS_DGRAM_STORE_X4
#define VDS_DGRAM_STORE_X4 1
#endif

namespace vds_ec {

namespace {

typedef const __attribute__((address_space(1))) uint32_t *gptr_u32;
typedef const __attribute__((address_space(1))) uint8_t *gptr_u8;
typedef __attribute__((address_space(1))) uint32_t *gptr_w32;
typedef __attribute__((address_space(1))) uint8_t *gptr_w8;

// Stream bytes [lo, hi) live in memory; p is the aligned dword that holds
// stream byte 0 (were it there), sh that byte's place in it: dword q of p
// holds stream bytes 4 q - sh .. 4 q - sh + 3.
struct Seg {
  gptr_u32 p;
  uint32_t sel;
  int32_t sh, lo, hi;
};

__device__ __forceinline__ Seg make_seg(uint64_t addr_of_lo, int32_t lo, int32_t hi) {
  Seg s;
  if (hi <= lo) {
    s.p = nullptr;
    s.sel = 0;
    s.sh = s.lo = s.hi = 0;
    return s;
  }
  const uint64_t v = addr_of_lo - (uint64_t)lo;
  const uint32_t sh = (uint32_t)(v & 3u);
  s.p = reinterpret_cast<gptr_u32>(v - sh);
  s.sel = (sh + 3u) | ((sh + 2u) << 8) | ((sh + 1u) << 16) | (sh << 24);
  s.sh = (int32_t)sh;
  s.lo = lo;
  s.hi = hi;
  return s;
}

// Stream block blk lies wholly inside the run, and so do the 17 aligned dwords its words are made of.
__device__ __forceinline__ bool seg_whole(const Seg &s, int32_t blk) {
  const int32_t b0 = 64 * blk;
  return s.hi > s.lo && s.lo <= b0 && b0 + 68 <= s.hi + s.sh;
}

// OR the run's bytes of stream block blk into the big-endian words w.
__device__ __forceinline__ void seg_block(const Seg &s, int32_t blk, uint32_t (&w)[16]) {
  const int32_t b0 = 64 * blk;
  if (s.hi <= s.lo || s.hi <= b0 || s.lo >= b0 + 64) return;
  const gptr_u32 q = s.p + 16 * blk;
  uint32_t raw[17];
  if (seg_whole(s, blk)) {
#pragma unroll
    for (int i = 0; i <= 16; ++i) raw[i] = q[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] |= __builtin_amdgcn_perm(raw[i + 1], raw[i], s.sel);
    return;
  }
#pragma unroll
  for (int i = 0; i <= 16; ++i) {
    const int32_t a = b0 + 4 * i - s.sh;  // the dword's first stream byte
    raw[i] = (a + 3 >= s.lo && a < s.hi) ? q[i] : 0u;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int32_t chi = s.hi - (b0 + 4 * i), clo = s.lo - (b0 + 4 * i);
    uint32_t mk = 0xFFFFFFFFu;
    if (chi < 4) mk = chi <= 0 ? 0u : ~(0xFFFFFFFFu >> (8 * chi));
    if (clo > 0) mk = clo >= 4 ? 0u : mk & (0xFFFFFFFFu >> (8 * clo));
    w[i] |= __builtin_amdgcn_perm(raw[i + 1], raw[i], s.sel) & mk;
  }
}

__device__ __forceinline__ uint32_t bswap(uint32_t v) { return __builtin_amdgcn_perm(0u, v, 0x00010203u); }

// Stream bytes 64 blk .. of the n-byte stream (big-endian words w) to out + 64 blk ..:
// a whole block into a 16-byte aligned slot as four 16-byte stores (the lanes
// of a wave write to different datagrams: one 64-byte line a lane), else dwords
// when out is 4-byte aligned, bytes for a last partial word or otherwise.
__device__ __forceinline__ void store_block(uint64_t out, int32_t blk, const uint32_t (&w)[16], int32_t n) {
  const uint64_t o = out + 64ull * (uint32_t)blk;
  const int32_t c = n - 64 * blk;  // bytes of the stream from this block on
  if (VDS_DGRAM_STORE_X4 && (out & 15u) == 0 && c >= 64) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) u32x4 *gptr_w128;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4 v;
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = bswap(w[4 * i + t]);
      reinterpret_cast<gptr_w128>(o)[i] = v;
    }
  } else if ((out & 3u) == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int32_t ci = c - 4 * i;
      if (ci >= 4) {
        reinterpret_cast<gptr_w32>(o)[i] = bswap(w[i]);
      } else {
#pragma unroll
        for (int t = 0; t < 3; ++t)
          if (t < ci) reinterpret_cast<gptr_w8>(o)[4 * i + t] = (uint8_t)(w[i] >> (24 - 8 * t));
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (4 * i + t < c) reinterpret_cast<gptr_w8>(o)[4 * i + t] = (uint8_t)(w[i] >> (24 - 8 * t));
  }
}

__device__ __forceinline__ void store_mac(uint64_t at, const uint32_t (&h)[8]) {
  if ((at & 3u) == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) reinterpret_cast<gptr_w32>(at)[i] = bswap(h[i]);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int t = 0; t < 4; ++t) reinterpret_cast<gptr_w8>(at)[4 * i + t] = (uint8_t)(h[i] >> (24 - 8 * t));
  }
}

// HMAC of the n-byte stream hw (its first words; bytes past the header zero),
// R, P under key state ks; STORE: the stream's bytes also go to out.
template <bool STORE>
__device__ __forceinline__ void hmac_stream(const HmacKeyState *ks, const uint32_t (&hw)[3], const Seg &R,
                                            const Seg &P, int32_t n, uint64_t out, uint32_t (&mac)[8]) {
  const gptr_u32 kp = reinterpret_cast<gptr_u32>(reinterpret_cast<uint64_t>(ks));
  uint32_t h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = kp[i];
  const int32_t nblk = (n + 8) / 64 + 1;
  const uint64_t bits = (64ull + (uint32_t)n) * 8;
  for (int32_t blk = 0; blk < nblk; ++blk) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = 0u;
    if (blk == 0) {
      w[0] = hw[0];
      w[1] = hw[1];
      w[2] = hw[2];
    }
    seg_block(R, blk, w);
    seg_block(P, blk, w);
    if constexpr (STORE) store_block(out, blk, w, n);
    const int32_t c = n - 64 * blk;  // stream bytes from this block on
    if (c < 64) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int32_t ci = c - 4 * i;
        if (ci >= 0 && ci < 4) w[i] |= 0x80u << (24 - 8 * ci);
      }
      if (blk + 1 == nblk) {
        w[14] = (uint32_t)(bits >> 32);
        w[15] = (uint32_t)bits;
      }
    }
    sha256_compress(h, w);
  }
  // outer: the second pad's state, then the 32-byte inner digest (one block)
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    w[i] = h[i];
    mac[i] = kp[8 + i];
  }
  w[8] = 0x80000000u;
#pragma unroll
  for (int i = 9; i < 15; ++i) w[i] = 0u;
  w[15] = (64u + 32u) * 8u;
  sha256_compress(mac, w);
}

// mac against the 32 bytes at e (any alignment; read as the message is)
__device__ __forceinline__ uint32_t mac_differs(const uint32_t (&mac)[8], uint64_t e) {
  const uint32_t esh = (uint32_t)(e & 3u);
  const gptr_u32 ep = reinterpret_cast<gptr_u32>(e - esh);
  const uint32_t esel = (esh + 3u) | ((esh + 2u) << 8) | ((esh + 1u) << 16) | (esh << 24);
  uint32_t raw[9];
#pragma unroll
  for (int i = 0; i < 8; ++i) raw[i] = ep[i];
  raw[8] = esh ? ep[8] : 0u;
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= mac[i] ^ __builtin_amdgcn_perm(raw[i + 1], raw[i], esel);
  return diff;
}

// cnt bytes from src to dst, any alignments: bytes up to dst's first aligned
// dword, then aligned dword stores assembled from aligned dword loads (only
// dwords holding a source byte), then the last bytes.
__device__ __forceinline__ void copy_bytes(uint64_t dst, uint64_t src, uint32_t cnt) {
  uint32_t head = (uint32_t)((4u - (dst & 3u)) & 3u);
  if (head > cnt) head = cnt;
  for (uint32_t i = 0; i < head; ++i) reinterpret_cast<gptr_w8>(dst)[i] = reinterpret_cast<gptr_u8>(src)[i];
  dst += head;
  src += head;
  cnt -= head;
  const uint32_t nd = cnt / 4;
  const gptr_w32 d = reinterpret_cast<gptr_w32>(dst);
  const uint32_t sh = (uint32_t)(src & 3u);
  const gptr_u32 p = reinterpret_cast<gptr_u32>(src - sh);
  if (sh == 0) {
    for (uint32_t i = 0; i < nd; ++i) d[i] = p[i];
  } else if (nd) {
    const uint32_t sel = sh | ((sh + 1u) << 8) | ((sh + 2u) << 16) | ((sh + 3u) << 24);
    uint32_t cur = p[0];
    for (uint32_t i = 0; i < nd; ++i) {
      const uint32_t nxt = p[i + 1];  // holds source byte 4 i + 3
      d[i] = __builtin_amdgcn_perm(nxt, cur, sel);
      cur = nxt;
    }
  }
  for (uint32_t i = 4 * nd; i < cnt; ++i) reinterpret_cast<gptr_w8>(dst)[i] = reinterpret_cast<gptr_u8>(src)[i];
}

__global__ __launch_bounds__(64) void k_hmac_sha256_batch(HmacBatchLaunch L) {
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  if (j >= L.count) return;
  const HmacLane ln = L.lanes[j];
  const uint32_t hw[3] = {0u, 0u, 0u};
  const Seg none = make_seg(0, 0, 0);
  const Seg P = make_seg(ln.src, 0, (int32_t)ln.len);
  uint32_t mac[8];
  hmac_stream<false>(L.keys + ln.session, hw, none, P, (int32_t)ln.len, 0, mac);
  if (L.macs) store_mac(L.macs + 32ull * ln.index, mac);
  if (L.expected)
    reinterpret_cast<gptr_w8>(L.verdicts)[ln.index] = mac_differs(mac, L.expected + 32ull * ln.index) ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_dgram_seal(DgramSealLaunch L) {
  const uint32_t wv = blockIdx.x;
  const uint32_t j = wv * 64u + threadIdx.x;
  if (j >= L.lanes) return;
  uint32_t lo = L.wave_msg[wv], hi = L.wave_msg[wv + 1];
  while (lo < hi) {  // the last message whose first lane is <= j
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (L.msgs[mid].first <= j)
      lo = mid;
    else
      hi = mid - 1;
  }
  const DgramSealMsg m = L.msgs[lo];
  const uint32_t d = j - m.first;
  const uint32_t r = m.route_len;
  const uint32_t kind = r == 0 ? 1u : r == 32 ? 3u : 5u;  // direct, routed, proxied (single; +1: split)
  const bool single = 37ull + r + m.len < m.mtu;
  uint32_t hdr, b0, poff, plen;
  if (d == 0) {
    hdr = single ? 5u : 9u;
    b0 = ((single ? kind : kind + 1u) << 5) | m.type;
    poff = 0;
    plen = single ? m.len : m.mtu - (41u + r);
  } else {
    const uint32_t c0 = m.mtu - (41u + r), per = m.mtu - 37u;
    const uint64_t at = c0 + (uint64_t)(d - 1) * per;
    if (single || at >= m.len) return;  // (no such datagram: the host's lane count says otherwise)
    hdr = 5u;
    b0 = 0x03u;
    poff = (uint32_t)at;
    plen = m.len - poff < per ? m.len - poff : per;
  }
  const uint32_t idx = m.index0 + d;
  uint32_t hw[3];
  hw[0] = (b0 << 24) | (idx >> 8);
  hw[1] = (idx << 24) | (hdr == 9u ? m.len >> 8 : 0u);
  hw[2] = hdr == 9u ? m.len << 24 : 0u;
  const uint32_t rl = d == 0 ? r : 0u;
  const int32_t n = (int32_t)(hdr + rl + plen);
  const Seg R = make_seg(m.route, (int32_t)hdr, (int32_t)(hdr + rl));
  const Seg P = make_seg(m.msg + poff, (int32_t)(hdr + rl), n);
  const uint64_t out = m.out + (uint64_t)d * m.pitch;
  uint32_t mac[8];
  hmac_stream<true>(L.keys + m.session, hw, R, P, n, out, mac);
  store_mac(out + (uint32_t)n, mac);
}

// The same copy by the whole wave (cnt, dst and src wave-uniform): lane l
// stores the bytes before dst's first aligned dword and the last ones, and the
// dwords l, l + 64, ... in between, so a wave's stores are contiguous.
__device__ __forceinline__ void copy_bytes_wave(uint64_t dst, uint64_t src, uint32_t cnt, uint32_t lane) {
  uint32_t head = (uint32_t)((4u - (dst & 3u)) & 3u);
  if (head > cnt) head = cnt;
  if (lane < head) reinterpret_cast<gptr_w8>(dst)[lane] = reinterpret_cast<gptr_u8>(src)[lane];
  dst += head;
  src += head;
  cnt -= head;
  const uint32_t nd = cnt / 4;
  const gptr_w32 d = reinterpret_cast<gptr_w32>(dst);
  const uint32_t sh = (uint32_t)(src & 3u);
  const gptr_u32 p = reinterpret_cast<gptr_u32>(src - sh);
  const uint32_t sel = sh | ((sh + 1u) << 8) | ((sh + 2u) << 16) | ((sh + 3u) << 24);
  for (uint32_t i = lane; i < nd; i += 64u) {
    const uint32_t cur = p[i];
    const uint32_t nxt = sh ? p[i + 1] : 0u;  // holds source byte 4 i + 3 when sh != 0
    d[i] = sh ? __builtin_amdgcn_perm(nxt, cur, sel) : cur;
  }
  const uint32_t t = 4 * nd + lane;
  if (t < cnt) reinterpret_cast<gptr_w8>(dst)[t] = reinterpret_cast<gptr_u8>(src)[t];
}

__device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t lane) { return __builtin_amdgcn_readlane(v, lane); }

// WAVE: the payloads of a wave's verified datagrams are copied one after the
// other by all 64 lanes (no lane leaves before that); else each lane copies
// its own.
template <bool WAVE>
__global__ __launch_bounds__(64) void k_dgram_open(DgramOpenLaunch L) {
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  HmacLane ln{};
  if (j < L.count) ln = L.lanes[j];
  uint32_t todo = 0;  // payload bytes this lane's datagram has for its destination
  if (j < L.count) {
    const gptr_w8 verdict = reinterpret_cast<gptr_w8>(L.verdicts) + ln.index;
    if (ln.len < 33u) {
      *verdict = 2;
    } else {
      const int32_t n = (int32_t)(ln.len - 32u);
      const uint32_t hw[3] = {0u, 0u, 0u};
      const Seg none = make_seg(0, 0, 0);
      const Seg P = make_seg(ln.src, 0, n);
      uint32_t mac[8];
      hmac_stream<false>(L.keys + ln.session, hw, none, P, n, 0, mac);
      const uint32_t diff = mac_differs(mac, ln.src + (uint32_t)n);
      *verdict = diff ? 1 : 0;
      // unauthenticated bytes never reach a message buffer
      if (!diff && ln.dst && ln.hdr_len < (uint32_t)n) todo = (uint32_t)n - ln.hdr_len;
    }
  }
  if constexpr (!WAVE) {
    if (todo) copy_bytes(ln.dst, ln.src + ln.hdr_len, todo);
  } else {
    const uint64_t from = ln.src + ln.hdr_len;
    for (uint64_t pending = __ballot(todo != 0); pending; pending &= pending - 1) {
      const uint32_t l = (uint32_t)__builtin_ctzll(pending);
      const uint64_t dst = (uint64_t)bcast((uint32_t)(ln.dst >> 32), l) << 32 | bcast((uint32_t)ln.dst, l);
      const uint64_t src = (uint64_t)bcast((uint32_t)(from >> 32), l) << 32 | bcast((uint32_t)from, l);
      copy_bytes_wave(dst, src, bcast(todo, l), threadIdx.x);
    }
  }
}

}  // namespace

hipError_t launch_hmac_sha256_batch(const HmacBatchLaunch &b, hipStream_t s) {
  if (b.count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_hmac_sha256_batch, dim3((b.count + 63) / 64), dim3(64), 0, s, b);
  return hipGetLastError();
}

hipError_t launch_dgram_seal(const DgramSealLaunch &b, hipStream_t s) {
  if (b.lanes == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dgram_seal, dim3((b.lanes + 63) / 64), dim3(64), 0, s, b);
  return hipGetLastError();
}

hipError_t launch_dgram_open(const DgramOpenLaunch &b, hipStream_t s, bool lane_copy) {
  if (b.count == 0) return hipSuccess;
  if (lane_copy)
    hipLaunchKernelGGL(k_dgram_open<false>, dim3((b.count + 63) / 64), dim3(64), 0, s, b);
  else
    hipLaunchKernelGGL(k_dgram_open<true>, dim3((b.count + 63) / 64), dim3(64), 0, s, b);
  return hipGetLastError();
}

}  // namespace vds_ec
