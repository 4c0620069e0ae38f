// aes_device.hpp -- the AES-256 pieces shared by aes.hip's two kernels: the
// tables as __constant__ data and their LDS copies, the key schedule computed
// by a quad (lane c of the quad holds column c of every round key), and the
// helpers that read and write bytes at any address.  Internal linkage.
//
// A column of the state is one little-endian dword, as the bytes load: no
// byte swap anywhere (aes_tables.hpp).  The tables for rows 1..3 are Te0 / Td0
// rotated with one v_alignbit_b32 each: three VALU ops a lane a round against
// 3 KiB more LDS a workgroup for the rotated copies.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vds_ec.h"
#include "aes_tables.hpp"
#include "ec_internal.hpp"

namespace vds_ec {
namespace {

__constant__ AesTables kAesDev = make_aes_tables();

typedef const __attribute__((address_space(1))) uint32_t *aes_gptr_u32;
typedef uint32_t aes_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) aes_u32x4 *aes_gptr_u128;
typedef __attribute__((address_space(1))) aes_u32x4 *aes_gptr_w128;
typedef __attribute__((address_space(1))) uint32_t *aes_gptr_w32;
typedef __attribute__((address_space(1))) int32_t *aes_gptr_wi32;
typedef __attribute__((address_space(1))) uint8_t *aes_gptr_w8;

__device__ __forceinline__ uint32_t aes_rotl(uint32_t x, uint32_t n) { return __builtin_amdgcn_alignbit(x, x, 32u - n); }

// quad_perm controls: lane c of a quad reads lane (c + d) % 4, or a fixed lane
constexpr int kQuadNext1 = 0x39;  // [1,2,3,0]
constexpr int kQuadNext2 = 0x4E;  // [2,3,0,1]
constexpr int kQuadNext3 = 0x93;  // [3,0,1,2]
constexpr int kQuadLane3 = 0xFF;  // [3,3,3,3]
constexpr int kQuadShr1 = 0x90;   // [0,0,1,2]
constexpr int kQuadShr2 = 0x40;   // [0,0,0,1]
template <int CTRL>
__device__ __forceinline__ uint32_t quad(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, false);
}

// SubWord through Te0, whose bytes 1 and 2 are S[x]
__device__ __forceinline__ uint32_t aes_sub_word(const uint32_t *te0, uint32_t w) {
  return ((te0[w & 0xFFu] >> 8) & 0xFFu) | (te0[(w >> 8) & 0xFFu] & 0xFF00u) | (te0[(w >> 16) & 0xFFu] & 0xFF0000u) |
         ((te0[w >> 24] << 8) & 0xFF000000u);
}

// The AES-256 schedule by a quad whose four lanes are all active: k0, k1 =
// the lane's columns of the key's two halves (key words c and 4 + c); rk[r] =
// the lane's column of round key r.  w[4r + c] = w[4r - 8 + c] ^ w[4r + c - 1]
// unrolls, inside a round key, to a prefix XOR over the quad's lanes 0..c of
// round key r - 2, XOR g = f(w[4r - 1]), lane 3's column of round key r - 1.
__device__ __forceinline__ void aes256_expand_quad(const uint32_t *te0, uint32_t c, uint32_t k0, uint32_t k1,
                                                   uint32_t (&rk)[15]) {
  rk[0] = k0;
  rk[1] = k1;
#pragma unroll
  for (int r = 2; r < 15; ++r) {
    const uint32_t last = quad<kQuadLane3>(rk[r - 1]);
    const uint32_t g = r % 2 == 0 ? aes_sub_word(te0, aes_rotl(last, 24)) ^ kAesRcon[r / 2 - 1] : aes_sub_word(te0, last);
    uint32_t p = rk[r - 2];
    const uint32_t t1 = quad<kQuadShr1>(p);
    p ^= c >= 1 ? t1 : 0u;
    const uint32_t t2 = quad<kQuadShr2>(p);
    p ^= c >= 2 ? t2 : 0u;
    rk[r] = p ^ g;
  }
}

// InvMixColumns of a round key column: Td0[S[x]] per byte (the equivalent inverse cipher's schedule)
__device__ __forceinline__ uint32_t aes_inv_mix(const uint32_t *te0, const uint32_t *td0, uint32_t w) {
  const uint32_t s = aes_sub_word(te0, w);
  return td0[s & 0xFFu] ^ aes_rotl(td0[(s >> 8) & 0xFFu], 8) ^ aes_rotl(td0[(s >> 16) & 0xFFu], 16) ^
         aes_rotl(td0[s >> 24], 24);
}

// The four bytes at address a (all of them the caller's), from the one or two aligned words holding them
__device__ __forceinline__ uint32_t aes_get_word(uint64_t a) {
  const uint32_t sh = (uint32_t)(a & 3u);
  const aes_gptr_u32 p = reinterpret_cast<aes_gptr_u32>(a - sh);
  const uint32_t lo = p[0], hi = sh ? p[1] : 0u;
  return __builtin_amdgcn_perm(hi, lo, 0x03020100u + 0x01010101u * sh);
}

// Four bytes to address a, and no other byte
__device__ __forceinline__ void aes_put_word(uint64_t a, uint32_t v) {
  if ((a & 3u) == 0) {
    *reinterpret_cast<aes_gptr_w32>(a) = v;
  } else {
    const aes_gptr_w8 b = reinterpret_cast<aes_gptr_w8>(a);
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = (uint8_t)(v >> (8 * i));
  }
}

}  // namespace
}  // namespace vds_ec
