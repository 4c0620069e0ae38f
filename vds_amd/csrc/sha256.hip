// sha256.hip -- SHA-256 (FIPS 180-4) of replica buffers on the device.
//
// The reference names every replica by the SHA-256 of its bytes:
// save_temp and save_data (dht_network_client.cpp:79, :593) call
// hash::signature(hash::sha256(), replica), i.e. OpenSSL EVP_sha256
// (kernel/vds_crypto/hash.cpp:21-29, 91-101).  After a GPU encode the replica
// bytes are already in HBM, so hashing them there replaces n CPU passes over
// the replicas.
//
// SHA-256 is a sequential chain over 64-byte blocks, so one lane hashes one
// message; a launch hashes many messages (every replica of every object of a
// batch) side by side.  Replicas are 2 T + 2 bytes long, so a message may
// start at any byte: each lane reads aligned dwords and assembles the
// big-endian message words with one v_perm_b32 each.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/vds_ec.h"
#include "ec_internal.hpp"
#include "sha256_device.hpp"

namespace vds_ec {

namespace {

// Message j = base + j * stride (len bytes) -> digest at digests + 32 j.
// ALIGNED (base and stride multiples of 16, e.g. the replica layouts of the
// batched encodes): whole blocks as four 16-byte loads per lane, the next
// block's loads issued before this block's 64 rounds (each lane walks its
// own message: without the prefetch every block waited out a full memory
// latency).  Otherwise aligned dwords and one v_perm_b32 per word.
template <bool ALIGNED>
__global__ __launch_bounds__(64) void k_sha256(const uint8_t *base, uint64_t len, uint64_t stride, uint32_t count,
                                               uint8_t *digests) {
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  if (j >= count) return;
  const uint8_t *m = base + (uint64_t)j * stride;
  uint32_t h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = kSha256H0[i];

  // Whole blocks from aligned dwords: block b needs dwords 16 b .. 16 b + 16
  // of p (17 with the misalignment), all inside the message while
  // 64 b + 68 <= len + sh.  (ALIGNED: sh = 0 and 64 b + 64 <= len.)
  const uint32_t sh = ALIGNED ? 0u : (uint32_t)((uintptr_t)m & 3u);
  const uint32_t *p = reinterpret_cast<const uint32_t *>(m - sh);
  // big-endian word of message bytes 4i..4i+3 = bytes sh+3, sh+2, sh+1, sh of (p[i+1]:p[i])
  const uint32_t sel = (sh + 3u) | ((sh + 2u) << 8) | ((sh + 1u) << 16) | (sh << 24);
  uint64_t nfast;
  if constexpr (ALIGNED) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 *q = reinterpret_cast<const u32x4 *>(m);
    nfast = len / 64;
    u32x4 nx[4];
    if (nfast) {
#pragma unroll
      for (int i = 0; i < 4; ++i) nx[i] = q[i];
    }
    for (uint64_t blk = 0; blk < nfast; ++blk) {
      uint32_t w[16];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) w[4 * i + t] = __builtin_amdgcn_perm(0u, nx[i][t], 0x00010203u);
      if (blk + 1 < nfast) {
#pragma unroll
        for (int i = 0; i < 4; ++i) nx[i] = q[4 * (blk + 1) + i];
      }
      sha256_compress(h, w);
    }
  } else {
    nfast = len + sh >= 68 ? (len + sh - 68) / 64 + 1 : 0;
    uint32_t carry = nfast ? p[0] : 0u;
    for (uint64_t blk = 0; blk < nfast; ++blk) {
      const uint32_t *q = p + 16 * blk;
      uint32_t raw[17];
      raw[0] = carry;
#pragma unroll
      for (int i = 1; i <= 16; ++i) raw[i] = q[i];
      carry = raw[16];
      uint32_t w[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) w[i] = __builtin_amdgcn_perm(raw[i + 1], raw[i], sel);
      sha256_compress(h, w);
    }
  }

  // The rest (< 132 bytes) the same way, from the aligned dwords that hold at
  // least one message byte (never past the dword of the last byte), then
  // bytes >= rem masked off, 0x80 after them, and the 64-bit big-endian bit
  // length in the last block.
  const uint64_t rem = len - 64 * nfast;
  const uint32_t nb = (uint32_t)((rem + 9 + 63) / 64);
  const uint64_t bits = len * 8;
  const uint64_t lim = len + sh;  // aligned byte offsets < lim hold message bytes
  for (uint32_t blk = 0; blk < nb; ++blk) {
    const uint64_t q0 = 16 * (nfast + blk);
    uint32_t raw[17];
#pragma unroll
    for (int i = 0; i <= 16; ++i) raw[i] = 4 * (q0 + i) < lim ? p[q0 + i] : 0u;
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t c = (int64_t)rem - (int64_t)(64 * blk + 4 * i);  // message bytes left at this word
      uint32_t v = __builtin_amdgcn_perm(raw[i + 1], raw[i], sel);
      if (c < 4) v = c <= 0 ? 0u : v & ~(0xFFFFFFFFu >> (8 * c));
      if (c >= 0 && c < 4) v |= 0x80u << (24 - 8 * c);
      w[i] = v;
    }
    if (blk + 1 == nb) {
      w[14] = (uint32_t)(bits >> 32);
      w[15] = (uint32_t)bits;
    }
    sha256_compress(h, w);
  }
  uint8_t *dg = digests + 32ull * j;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) dg[4 * i + t] = (uint8_t)(h[i] >> (24 - 8 * t));
}

// (the batch kernel's tables, whichever launch struct its instance takes)
__device__ __forceinline__ const ShaBatchLaunch &tables(const ShaBatchLaunch &l) { return l; }
__device__ __forceinline__ const ShaBatchLaunch &tables(const ShaBatchCheckLaunch &l) { return l.b; }
__device__ __forceinline__ const ShaBatchLaunch &tables(const ShaBatchGatedLaunch &l) { return l.c.b; }
__device__ __forceinline__ const ShaBatchCheck *checks_of(const ShaBatchCheckLaunch &l) { return l.checks; }
__device__ __forceinline__ const ShaBatchCheck *checks_of(const ShaBatchGatedLaunch &l) { return l.c.checks; }

// Messages of different lengths, one lane each: lane j finds its group between
// its wave's two wave_group entries (ShaBatchLaunch, ec_internal.hpp), then
// walks its own message with its own length and alignment -- aligned dwords
// and one v_perm_b32 per word as k_sha256<false>, and the next block's 17
// dwords issued before this block's 64 rounds (the lanes of a wave sit in
// different messages, so nothing else hides the latency).  A wave runs as long
// as its longest chain; the host orders the lanes by length.  Only aligned
// dwords holding at least one message byte are read; a message of length 0
// reads nothing (its pointer may be null).
//
// CHECK (the repair and download loops: the catalogue holds the name every
// replica must have): after its last compression, when only h[8] is live, the
// lane also compares its digest with its group's expected bytes and writes a
// verdict byte (ShaBatchCheck, ec_internal.hpp); the expected bytes are read
// as the message is, from the aligned dwords holding at least one of them.
//
// GATED (the unpack chain's name check, every group one message): the length
// and a status come from device arrays (ShaBatchGate, ec_internal.hpp); the
// lane hashes only where the status lets it and writes the final status, and
// a length of 0 where that is not VDS_EC_OK.
template <bool CHECK, bool GATED = false>
__global__ __launch_bounds__(64) void k_sha256_batch(
    std::conditional_t<GATED, ShaBatchGatedLaunch, std::conditional_t<CHECK, ShaBatchCheckLaunch, ShaBatchLaunch>>
        launch) {
  const ShaBatchLaunch &b = tables(launch);
  const uint32_t wv = blockIdx.x;
  const uint32_t j = wv * 64u + threadIdx.x;
  uint32_t lo = b.wave_group[wv], hi = b.wave_group[wv + 1];
  while (lo < hi) {  // the last group whose first lane is <= j
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (b.spans[mid].first <= j)
      lo = mid;
    else
      hi = mid - 1;
  }
  const ShaBatchSpan sp = b.spans[lo];
  const uint32_t idx = j - sp.first;
  if (idx >= sp.m) return;  // a lane between two groups, or past the last one
  const ShaBatchGroup g = b.groups[lo];
  uint64_t len = g.len;
  if constexpr (GATED) {
    const ShaBatchGate gt = launch.gates[lo];
    const int32_t st = *reinterpret_cast<const __attribute__((address_space(1))) int32_t *>(gt.status);
    if (st != VDS_EC_OK && st != VDS_EC_EINFLATE_SHORT) {
      *reinterpret_cast<__attribute__((address_space(1))) uint32_t *>(gt.len) = 0u;
      return;
    }
    len = min(len, (uint64_t)*reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(gt.len));
  }
  // (the addresses come from the tables as integers: global pointers made
  // from them keep the loads and stores global_* rather than flat_*)
  typedef const __attribute__((address_space(1))) uint64_t *gptr_u64;
  typedef const __attribute__((address_space(1))) uint32_t *gptr_u32;
  typedef __attribute__((address_space(1))) uint8_t *gptr_u8;
  uint64_t m = 0;
  if (len) m = g.pitch == kShaBatchPtrTable ? reinterpret_cast<gptr_u64>(g.msg)[idx] : g.msg + (uint64_t)idx * g.pitch;
  uint32_t h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = kSha256H0[i];

  // Whole blocks: block blk needs dwords 16 blk .. 16 blk + 16 of p, all
  // holding message bytes while 64 blk + 68 <= len + sh.
  const uint32_t sh = (uint32_t)(m & 3u);
  const gptr_u32 p = reinterpret_cast<gptr_u32>(m - sh);
  const uint32_t sel = (sh + 3u) | ((sh + 2u) << 8) | ((sh + 1u) << 16) | (sh << 24);
  const uint64_t nfast = len + sh >= 68 ? (len + sh - 68) / 64 + 1 : 0;
  // nx = the block's 16 dwords, top = the one after them.  (Loading the 16 from
  // the block's own first dword, not from the second with the first carried
  // over: with a 64-byte aligned message -- replicas in aligned slots -- each
  // lane's loads then stay inside one 64-byte segment.)
  uint32_t nx[16], top = 0u;
  if (nfast) {
#pragma unroll
    for (int i = 0; i < 16; ++i) nx[i] = p[i];
    top = p[16];
  }
  for (uint64_t blk = 0; blk < nfast; ++blk) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 15; ++i) w[i] = __builtin_amdgcn_perm(nx[i + 1], nx[i], sel);
    w[15] = __builtin_amdgcn_perm(top, nx[15], sel);
    if (blk + 1 < nfast) {  // dwords 16 (blk + 1) .. + 16: inside the message, as above
      const gptr_u32 q = p + 16 * (blk + 1);
#pragma unroll
      for (int i = 0; i < 16; ++i) nx[i] = q[i];
      top = q[16];
    }
    sha256_compress(h, w);
  }

  // The rest (< 132 bytes) and the padding as k_sha256 does; with len == 0 no
  // dword holds a message byte whatever the pointer is.
  const uint64_t rem = len - 64 * nfast;
  const uint32_t nb = (uint32_t)((rem + 9 + 63) / 64);
  const uint64_t bits = len * 8;
  const uint64_t lim = len ? len + sh : 0;  // aligned byte offsets < lim hold message bytes
  for (uint32_t blk = 0; blk < nb; ++blk) {
    const uint64_t q0 = 16 * (nfast + blk);
    uint32_t raw[17];
#pragma unroll
    for (int i = 0; i <= 16; ++i) raw[i] = 4 * (q0 + i) < lim ? p[q0 + i] : 0u;
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t c = (int64_t)rem - (int64_t)(64 * blk + 4 * i);  // message bytes left at this word
      uint32_t v = __builtin_amdgcn_perm(raw[i + 1], raw[i], sel);
      if (c < 4) v = c <= 0 ? 0u : v & ~(0xFFFFFFFFu >> (8 * c));
      if (c >= 0 && c < 4) v |= 0x80u << (24 - 8 * c);
      w[i] = v;
    }
    if (blk + 1 == nb) {
      w[14] = (uint32_t)(bits >> 32);
      w[15] = (uint32_t)bits;
    }
    sha256_compress(h, w);
  }
  if (!CHECK || g.digests) {
    const gptr_u8 dg = reinterpret_cast<gptr_u8>(g.digests + 32ull * idx);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int t = 0; t < 4; ++t) dg[4 * i + t] = (uint8_t)(h[i] >> (24 - 8 * t));
  }
  if constexpr (CHECK) {
    const ShaBatchCheck c = checks_of(launch)[lo];
    if (c.expected == 0) return;
    // expected byte 4i..4i+3 big-endian = word i of the digest: dwords 0..7 of
    // ep hold expected bytes whatever esh is, dword 8 only when esh != 0
    const uint64_t e = c.expected + 32ull * idx;
    const uint32_t esh = (uint32_t)(e & 3u);
    const gptr_u32 ep = reinterpret_cast<gptr_u32>(e - esh);
    const uint32_t esel = (esh + 3u) | ((esh + 2u) << 8) | ((esh + 1u) << 16) | (esh << 24);
    uint32_t raw[9];
#pragma unroll
    for (int i = 0; i < 8; ++i) raw[i] = ep[i];
    raw[8] = esh ? ep[8] : 0u;
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) diff |= h[i] ^ __builtin_amdgcn_perm(raw[i + 1], raw[i], esel);
    if constexpr (GATED) {
      const ShaBatchGate gt = launch.gates[lo];
      *reinterpret_cast<__attribute__((address_space(1))) int32_t *>(gt.status) = diff ? VDS_EC_ECORRUPT : VDS_EC_OK;
      if (diff) *reinterpret_cast<__attribute__((address_space(1))) uint32_t *>(gt.len) = 0u;
    } else {
      reinterpret_cast<gptr_u8>(c.verdicts)[idx] = diff ? 1 : 0;
    }
  }
}


}  // namespace

hipError_t launch_sha256_batch(const ShaBatchLaunch &b, hipStream_t s) {
  if (b.waves == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sha256_batch<false>, dim3(b.waves), dim3(64), 0, s, b);
  return hipGetLastError();
}

hipError_t launch_sha256_check_batch(const ShaBatchCheckLaunch &c, hipStream_t s) {
  if (c.b.waves == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sha256_batch<true>, dim3(c.b.waves), dim3(64), 0, s, c);
  return hipGetLastError();
}

hipError_t launch_sha256_gated_batch(const ShaBatchGatedLaunch &g, hipStream_t s) {
  if (g.c.b.waves == 0) return hipSuccess;
  hipLaunchKernelGGL((k_sha256_batch<true, true>), dim3(g.c.b.waves), dim3(64), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_sha256(const uint8_t *base, uint64_t len, uint64_t stride, uint32_t count, uint8_t *digests,
                         hipStream_t s) {
  if (count == 0) return hipSuccess;
  if ((((uintptr_t)base | stride) & 15u) == 0)
    hipLaunchKernelGGL(k_sha256<true>, dim3((count + 63) / 64), dim3(64), 0, s, base, len, stride, count, digests);
  else
    hipLaunchKernelGGL(k_sha256<false>, dim3((count + 63) / 64), dim3(64), 0, s, base, len, stride, count, digests);
  return hipGetLastError();
}

}  // namespace vds_ec
