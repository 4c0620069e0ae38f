// aes.hip -- AES-256-CBC with PKCS#7 padding for batches of messages on the
// device: the cipher of the reference's file blocks (client::save / restore,
// dht_network_client.cpp:1101-1320; save_block, vds_ws.js:151-161) and channel
// messages, OpenSSL's EVP_aes_256_cbc with its default padding there.
//
// k_aes256_cbc_encrypt_batch: CBC encryption is one chain of dependent blocks
// a message, so the parallelism is the batch.  ONE QUAD PER CHAIN, 16 chains a
// wave: lane c of a quad holds column c of the state in one VGPR and its
// column of the 15 round keys in 15.  A round is four Te0 lookups a lane, on
// its own byte 0 and on bytes 1, 2, 3 of the columns of lanes c+1, c+2, c+3
// (three quad-perm DPP moves), the rows' rotations one v_alignbit_b32 each; no
// LDS exchange and no barrier after the table fill.  The quad expands its own
// key (aes_device.hpp).  A lane reads and writes its own dword of every block,
// so a quad reads and writes 16 contiguous bytes; the next block's dword is
// loaded before this block's rounds.  The last block is the message's tail and
// the padding bytes (a whole block of 0x10 when the length is a multiple of
// 16).  A quad stops after its own last block: a wave runs as long as its
// longest chain, and the host orders the chains longest first.
// k_aes256_cbc_encrypt_batch_lane is the one-lane-a-chain form, kept for the
// A/B behind VDS_EC_AES_ENC=lane.  k_aes256_cbc_encrypt_batch<true>
// is the gated instance (the pack chain's last launch: the lengths are the
// deflate's, on the device); <false> compiles to the instructions the kernel
// had before it was a template (profiles/deflate_batch/README.md).
//
// k_aes256_cbc_decrypt_batch: CBC decryption has no chain (block i needs
// ciphertext blocks i and i - 1), so the batch is tiled: a workgroup of
// kAesDecThreads lanes takes kAesDecTile bytes of one message, one lane a
// 16-byte block a step, so a wave reads contiguous memory.  The workgroup's
// first quad expands the key and stores the equivalent inverse cipher's
// schedule in LDS; every lane reads its round keys from there (one broadcast
// read a round).  A tile's first block XORs with the block before it in the
// message -- the previous tile's last -- or, in tile 0, with the iv.  The lane
// that owns the message's last block checks the padding and stores out_len and
// status; a message whose length is 0 or no multiple of 16 has one tile, which
// stores its status and does nothing else.
//
// Inputs and outputs at any byte address: only aligned words holding at least
// one byte of the message are read, only the output's own bytes written.  The
// fast path is 16-byte aligned messages (4-byte aligned for the encrypt).
#include <hip/hip_runtime.h>

#include "aes_device.hpp"

namespace vds_ec {

namespace {

// The lane's dword of the padded message at byte offset off (a multiple of 4):
// message bytes below len, the pad byte from there on.  p = the message's
// aligned base, sh its misalignment, lim = len + sh (0 for an empty message:
// nothing is read), padw = the pad byte four times.
__device__ __forceinline__ uint32_t padded_word(aes_gptr_u32 p, uint32_t sh, uint64_t lim, uint32_t len,
                                                uint32_t padw, uint64_t off) {
  const uint64_t q = off / 4;
  const uint32_t lo = 4 * q < lim ? p[q] : 0u;
  const uint32_t hi = sh && 4 * (q + 1) < lim ? p[q + 1] : 0u;
  uint32_t v = __builtin_amdgcn_perm(hi, lo, 0x03020100u + 0x01010101u * sh);
  const int64_t rem = (int64_t)len - (int64_t)off;  // message bytes from off on
  if (rem < 4) v = rem <= 0 ? padw : (v & (0xFFFFFFFFu >> (8 * (4 - (int)rem)))) | (padw << (8 * (int)rem));
  return v;
}

// kGated: the chain's length is min(m.len, lens[m.idx]) (device uint32_t: the
// deflate's out_lens in the pack chain; the host ordered the chains by m.len,
// the upper bound), and out_lens[m.idx] receives what it encrypts to.
template <bool kGated>
__global__ __launch_bounds__(64) void k_aes256_cbc_encrypt_batch(const AesEncMsg *msgs, uint32_t count, uint64_t keys,
                                                                 uint64_t ivs, uint64_t lens, uint64_t out_lens) {
  __shared__ uint32_t te0[256];
  for (uint32_t i = threadIdx.x; i < 256u; i += 64u) te0[i] = kAesDev.te0[i];
  __syncthreads();
  const uint32_t q = blockIdx.x * kAesEncChainsPerWave + threadIdx.x / 4u;
  const uint32_t c = threadIdx.x & 3u;
  if (q >= count) return;  // (a whole quad)
  const AesEncMsg m = msgs[q];
  const aes_gptr_u32 kp = reinterpret_cast<aes_gptr_u32>(keys + 32ull * m.idx);
  uint32_t rk[15];
  aes256_expand_quad(te0, c, kp[c], kp[4u + c], rk);
  uint32_t st = c == 0 ? kAesBlockIvWords[0] : c == 1 ? kAesBlockIvWords[1] : c == 2 ? kAesBlockIvWords[2]
                                                                                     : kAesBlockIvWords[3];
  if (ivs) st = aes_get_word(ivs + 16ull * m.idx + 4u * c);

  uint32_t len = m.len;
  if constexpr (kGated) {
    len = min(len, reinterpret_cast<aes_gptr_u32>(lens)[m.idx]);
    if (c == 0) reinterpret_cast<aes_gptr_w32>(out_lens)[m.idx] = (len / 16u + 1u) * 16u;
  }
  const uint32_t sh = (uint32_t)(m.in & 3u);
  const aes_gptr_u32 p = reinterpret_cast<aes_gptr_u32>(m.in - sh);
  const uint64_t lim = len ? (uint64_t)len + sh : 0;
  const uint32_t padw = 0x01010101u * (16u - len % 16u);
  const uint32_t nblk = len / 16u + 1u;
  uint32_t nx = padded_word(p, sh, lim, len, padw, 4u * c);
  for (uint32_t b = 0; b < nblk; ++b) {
    uint32_t x = st ^ nx ^ rk[0];
    if (b + 1 < nblk) nx = padded_word(p, sh, lim, len, padw, 16ull * (b + 1) + 4u * c);
#pragma unroll
    for (int r = 1; r < 14; ++r) {
      const uint32_t x1 = quad<kQuadNext1>(x), x2 = quad<kQuadNext2>(x), x3 = quad<kQuadNext3>(x);
      x = te0[x & 0xFFu] ^ aes_rotl(te0[(x1 >> 8) & 0xFFu], 8) ^ aes_rotl(te0[(x2 >> 16) & 0xFFu], 16) ^
          aes_rotl(te0[x3 >> 24], 24) ^ rk[r];
    }
    const uint32_t x1 = quad<kQuadNext1>(x), x2 = quad<kQuadNext2>(x), x3 = quad<kQuadNext3>(x);
    st = (((te0[x & 0xFFu] >> 8) & 0xFFu) | (te0[(x1 >> 8) & 0xFFu] & 0xFF00u) | (te0[(x2 >> 16) & 0xFFu] & 0xFF0000u) |
          ((te0[x3 >> 24] << 8) & 0xFF000000u)) ^ rk[14];
    aes_put_word(m.out + 16ull * b + 4u * c, st);
  }
}

// The A/B arm of the quad form (VDS_EC_AES_ENC=lane): ONE LANE PER CHAIN, 64
// chains a wave.  The lane holds the whole state (four columns) and all 60
// schedule words, expands its own key, and does a round's 16 lookups itself;
// nothing crosses lanes.  Same table, same order of chains, same bytes.
__global__ __launch_bounds__(64) void k_aes256_cbc_encrypt_batch_lane(const AesEncMsg *msgs, uint32_t count,
                                                                      uint64_t keys, uint64_t ivs) {
  __shared__ uint32_t te0[256];
  for (uint32_t i = threadIdx.x; i < 256u; i += 64u) te0[i] = kAesDev.te0[i];
  __syncthreads();
  const uint32_t q = blockIdx.x * 64u + threadIdx.x;
  if (q >= count) return;
  const AesEncMsg m = msgs[q];
  const aes_gptr_u32 kp = reinterpret_cast<aes_gptr_u32>(keys + 32ull * m.idx);
  uint32_t rk[60];
#pragma unroll
  for (int i = 0; i < 8; ++i) rk[i] = kp[i];
#pragma unroll
  for (int i = 8; i < 60; ++i) {
    uint32_t t = rk[i - 1];
    if (i % 8 == 0)
      t = aes_sub_word(te0, aes_rotl(t, 24)) ^ kAesRcon[i / 8 - 1];
    else if (i % 8 == 4)
      t = aes_sub_word(te0, t);
    rk[i] = rk[i - 8] ^ t;
  }
  uint32_t st[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) st[c] = ivs ? aes_get_word(ivs + 16ull * m.idx + 4u * c) : kAesBlockIvWords[c];

  const uint32_t len = m.len;
  const uint32_t sh = (uint32_t)(m.in & 3u);
  const aes_gptr_u32 p = reinterpret_cast<aes_gptr_u32>(m.in - sh);
  const uint64_t lim = len ? (uint64_t)len + sh : 0;
  const uint32_t padw = 0x01010101u * (16u - len % 16u);
  const uint32_t nblk = len / 16u + 1u;
  uint32_t nx[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) nx[c] = padded_word(p, sh, lim, len, padw, 4u * c);
  for (uint32_t b = 0; b < nblk; ++b) {
    uint32_t a0 = st[0] ^ nx[0] ^ rk[0], a1 = st[1] ^ nx[1] ^ rk[1], a2 = st[2] ^ nx[2] ^ rk[2],
             a3 = st[3] ^ nx[3] ^ rk[3];
    if (b + 1 < nblk) {
#pragma unroll
      for (int c = 0; c < 4; ++c) nx[c] = padded_word(p, sh, lim, len, padw, 16ull * (b + 1) + 4u * c);
    }
#pragma unroll
    for (int r = 1; r < 14; ++r) {
      const uint32_t n0 = te0[a0 & 0xFFu] ^ aes_rotl(te0[(a1 >> 8) & 0xFFu], 8) ^ aes_rotl(te0[(a2 >> 16) & 0xFFu], 16) ^
                          aes_rotl(te0[a3 >> 24], 24) ^ rk[4 * r];
      const uint32_t n1 = te0[a1 & 0xFFu] ^ aes_rotl(te0[(a2 >> 8) & 0xFFu], 8) ^ aes_rotl(te0[(a3 >> 16) & 0xFFu], 16) ^
                          aes_rotl(te0[a0 >> 24], 24) ^ rk[4 * r + 1];
      const uint32_t n2 = te0[a2 & 0xFFu] ^ aes_rotl(te0[(a3 >> 8) & 0xFFu], 8) ^ aes_rotl(te0[(a0 >> 16) & 0xFFu], 16) ^
                          aes_rotl(te0[a1 >> 24], 24) ^ rk[4 * r + 2];
      const uint32_t n3 = te0[a3 & 0xFFu] ^ aes_rotl(te0[(a0 >> 8) & 0xFFu], 8) ^ aes_rotl(te0[(a1 >> 16) & 0xFFu], 16) ^
                          aes_rotl(te0[a2 >> 24], 24) ^ rk[4 * r + 3];
      a0 = n0, a1 = n1, a2 = n2, a3 = n3;
    }
    st[0] = (((te0[a0 & 0xFFu] >> 8) & 0xFFu) | (te0[(a1 >> 8) & 0xFFu] & 0xFF00u) | (te0[(a2 >> 16) & 0xFFu] & 0xFF0000u) |
             ((te0[a3 >> 24] << 8) & 0xFF000000u)) ^ rk[56];
    st[1] = (((te0[a1 & 0xFFu] >> 8) & 0xFFu) | (te0[(a2 >> 8) & 0xFFu] & 0xFF00u) | (te0[(a3 >> 16) & 0xFFu] & 0xFF0000u) |
             ((te0[a0 >> 24] << 8) & 0xFF000000u)) ^ rk[57];
    st[2] = (((te0[a2 & 0xFFu] >> 8) & 0xFFu) | (te0[(a3 >> 8) & 0xFFu] & 0xFF00u) | (te0[(a0 >> 16) & 0xFFu] & 0xFF0000u) |
             ((te0[a1 >> 24] << 8) & 0xFF000000u)) ^ rk[58];
    st[3] = (((te0[a3 & 0xFFu] >> 8) & 0xFFu) | (te0[(a0 >> 8) & 0xFFu] & 0xFF00u) | (te0[(a1 >> 16) & 0xFFu] & 0xFF0000u) |
             ((te0[a2 >> 24] << 8) & 0xFF000000u)) ^ rk[59];
    const uint64_t dst = m.out + 16ull * b;
    if ((dst & 15u) == 0) {
      *reinterpret_cast<aes_gptr_w128>(dst) = aes_u32x4{st[0], st[1], st[2], st[3]};
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) aes_put_word(dst + 4u * c, st[c]);
    }
  }
}

// the 16 bytes at address a, all of them the caller's
__device__ __forceinline__ aes_u32x4 load_block(uint64_t a) {
  if ((a & 15u) == 0) return *reinterpret_cast<aes_gptr_u128>(a);
  const uint32_t sh = (uint32_t)(a & 3u);
  const aes_gptr_u32 p = reinterpret_cast<aes_gptr_u32>(a - sh);
  uint32_t raw[5];
#pragma unroll
  for (int i = 0; i < 4; ++i) raw[i] = p[i];
  raw[4] = sh ? p[4] : 0u;
  const uint32_t sel = 0x03020100u + 0x01010101u * sh;
  aes_u32x4 w;
  w.x = __builtin_amdgcn_perm(raw[1], raw[0], sel);
  w.y = __builtin_amdgcn_perm(raw[2], raw[1], sel);
  w.z = __builtin_amdgcn_perm(raw[3], raw[2], sel);
  w.w = __builtin_amdgcn_perm(raw[4], raw[3], sel);
  return w;
}

__global__ __launch_bounds__(kAesDecThreads) void k_aes256_cbc_decrypt_batch(AesDecLaunch l) {
  __shared__ uint32_t te0[256];
  __shared__ uint32_t td0[256];
  __shared__ uint8_t isb[256];
  __shared__ aes_u32x4 drk[15];
  const uint32_t tid = threadIdx.x;
  const AesDecTile tl = l.tiles[blockIdx.x];
  const AesDecMsg m = l.msgs[tl.msg];
  const uint32_t len = m.len;
  if (len == 0 || len % 16u) {  // (the whole workgroup: its one tile)
    if (tid == 0) {
      reinterpret_cast<aes_gptr_wi32>(l.statuses)[tl.msg] = VDS_EC_ECRYPT_LENGTH;
      reinterpret_cast<aes_gptr_w32>(l.out_lens)[tl.msg] = 0u;
    }
    return;
  }
  te0[tid] = kAesDev.te0[tid];
  td0[tid] = kAesDev.td0[tid];
  isb[tid] = kAesDev.isbox[tid];
  __syncthreads();
  if (tid < 4u) {
    const aes_gptr_u32 kp = reinterpret_cast<aes_gptr_u32>(l.keys + 32ull * tl.msg);
    uint32_t rk[15];
    aes256_expand_quad(te0, tid, kp[tid], kp[4u + tid], rk);
    uint32_t *d = reinterpret_cast<uint32_t *>(drk);
#pragma unroll
    for (int r = 0; r < 15; ++r) d[4 * r + tid] = r == 0 || r == 14 ? rk[14 - r] : aes_inv_mix(te0, td0, rk[14 - r]);
  }
  __syncthreads();

  const uint32_t nblk = len / 16u;
  const uint32_t b0 = tl.tile * (kAesDecTile / 16u);
  const uint32_t b1 = min(b0 + kAesDecTile / 16u, nblk);
  for (uint32_t b = b0 + tid; b < b1; b += kAesDecThreads) {
    const aes_u32x4 ct = load_block(m.in + 16ull * b);
    aes_u32x4 prev;
    if (b)
      prev = load_block(m.in + 16ull * (b - 1));
    else if (l.ivs)
      prev = load_block(l.ivs + 16ull * tl.msg);
    else
      prev = aes_u32x4{kAesBlockIvWords[0], kAesBlockIvWords[1], kAesBlockIvWords[2], kAesBlockIvWords[3]};
    aes_u32x4 k = drk[0];
    uint32_t a0 = ct.x ^ k.x, a1 = ct.y ^ k.y, a2 = ct.z ^ k.z, a3 = ct.w ^ k.w;
#pragma unroll
    for (int r = 1; r < 14; ++r) {
      k = drk[r];
      const uint32_t n0 = td0[a0 & 0xFFu] ^ aes_rotl(td0[(a3 >> 8) & 0xFFu], 8) ^ aes_rotl(td0[(a2 >> 16) & 0xFFu], 16) ^
                          aes_rotl(td0[a1 >> 24], 24) ^ k.x;
      const uint32_t n1 = td0[a1 & 0xFFu] ^ aes_rotl(td0[(a0 >> 8) & 0xFFu], 8) ^ aes_rotl(td0[(a3 >> 16) & 0xFFu], 16) ^
                          aes_rotl(td0[a2 >> 24], 24) ^ k.y;
      const uint32_t n2 = td0[a2 & 0xFFu] ^ aes_rotl(td0[(a1 >> 8) & 0xFFu], 8) ^ aes_rotl(td0[(a0 >> 16) & 0xFFu], 16) ^
                          aes_rotl(td0[a3 >> 24], 24) ^ k.z;
      const uint32_t n3 = td0[a3 & 0xFFu] ^ aes_rotl(td0[(a2 >> 8) & 0xFFu], 8) ^ aes_rotl(td0[(a1 >> 16) & 0xFFu], 16) ^
                          aes_rotl(td0[a0 >> 24], 24) ^ k.w;
      a0 = n0, a1 = n1, a2 = n2, a3 = n3;
    }
    k = drk[14];
    uint32_t o[4];
    o[0] = ((uint32_t)isb[a0 & 0xFFu] | (uint32_t)isb[(a3 >> 8) & 0xFFu] << 8 | (uint32_t)isb[(a2 >> 16) & 0xFFu] << 16 |
            (uint32_t)isb[a1 >> 24] << 24) ^ k.x ^ prev.x;
    o[1] = ((uint32_t)isb[a1 & 0xFFu] | (uint32_t)isb[(a0 >> 8) & 0xFFu] << 8 | (uint32_t)isb[(a3 >> 16) & 0xFFu] << 16 |
            (uint32_t)isb[a2 >> 24] << 24) ^ k.y ^ prev.y;
    o[2] = ((uint32_t)isb[a2 & 0xFFu] | (uint32_t)isb[(a1 >> 8) & 0xFFu] << 8 | (uint32_t)isb[(a0 >> 16) & 0xFFu] << 16 |
            (uint32_t)isb[a3 >> 24] << 24) ^ k.z ^ prev.z;
    o[3] = ((uint32_t)isb[a3 & 0xFFu] | (uint32_t)isb[(a2 >> 8) & 0xFFu] << 8 | (uint32_t)isb[(a1 >> 16) & 0xFFu] << 16 |
            (uint32_t)isb[a0 >> 24] << 24) ^ k.w ^ prev.w;
    const uint64_t dst = m.out + 16ull * b;
    if ((dst & 15u) == 0) {
      *reinterpret_cast<aes_gptr_w128>(dst) = aes_u32x4{o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) aes_put_word(dst + 4u * i, o[i]);
    }
    if (b + 1 == nblk) {  // PKCS#7: the last byte n in 1..16 and the last n bytes all n
      const uint32_t pad = o[3] >> 24;
      bool ok = pad >= 1u && pad <= 16u;
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (16u - j <= pad && ((o[j / 4] >> (8 * (j % 4))) & 0xFFu) != pad) ok = false;
      reinterpret_cast<aes_gptr_wi32>(l.statuses)[tl.msg] = ok ? VDS_EC_OK : VDS_EC_ECRYPT_PADDING;
      reinterpret_cast<aes_gptr_w32>(l.out_lens)[tl.msg] = ok ? len - pad : 0u;
    }
  }
}

}  // namespace

hipError_t launch_aes_encrypt_batch(const AesEncMsg *msgs, uint32_t count, const uint8_t *keys, const uint8_t *ivs,
                                    hipStream_t s, bool lane_chain) {
  if (count == 0) return hipSuccess;
  if (lane_chain) {
    hipLaunchKernelGGL(k_aes256_cbc_encrypt_batch_lane, dim3((count + 63u) / 64u), dim3(64), 0, s, msgs, count,
                       reinterpret_cast<uint64_t>(keys), reinterpret_cast<uint64_t>(ivs));
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_aes256_cbc_encrypt_batch<false>, dim3((count + kAesEncChainsPerWave - 1) / kAesEncChainsPerWave),
                     dim3(64), 0, s, msgs, count, reinterpret_cast<uint64_t>(keys), reinterpret_cast<uint64_t>(ivs),
                     uint64_t(0), uint64_t(0));
  return hipGetLastError();
}

hipError_t launch_aes_encrypt_gated_batch(const AesEncMsg *msgs, uint32_t count, const uint8_t *keys,
                                          const uint8_t *ivs, const uint32_t *lens, uint32_t *out_lens, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_aes256_cbc_encrypt_batch<true>, dim3((count + kAesEncChainsPerWave - 1) / kAesEncChainsPerWave),
                     dim3(64), 0, s, msgs, count, reinterpret_cast<uint64_t>(keys), reinterpret_cast<uint64_t>(ivs),
                     reinterpret_cast<uint64_t>(lens), reinterpret_cast<uint64_t>(out_lens));
  return hipGetLastError();
}

hipError_t launch_aes_decrypt_batch(const AesDecLaunch &l, hipStream_t s) {
  if (l.ntiles == 0) return hipSuccess;
  hipLaunchKernelGGL(k_aes256_cbc_decrypt_batch, dim3(l.ntiles), dim3(kAesDecThreads), 0, s, l);
  return hipGetLastError();
}

}  // namespace vds_ec
