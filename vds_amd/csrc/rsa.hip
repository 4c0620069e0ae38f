// rsa.hip -- the RSA public operation s^e mod n for a ragged batch, and the
// RSASSA-PKCS1-v1_5 / SHA-256 verdict built on it (the transaction log's
// asymmetric_sign_verify::verify, asymmetriccrypto.cpp:488-537).
//
// ONE WAVE AN ITEM.  Lane l holds limbs K l .. K l + K - 1 of every operand, K =
// 1 for a 64-limb key and 2 for a 128-limb one, so an operand is K registers a
// lane and a Montgomery product (rsa_common.hpp has the arithmetic) keeps a, b,
// n and K 64-bit columns in registers: nothing spills and nothing touches LDS.
// A row reads its multiplicand limb with v_readlane (the row index is uniform),
// multiplies, takes the quotient digit from lane 0 the same way, multiplies
// again and moves every column one lane down (__shfl_down).  The columns are
// resolved across the lanes once per product from two __ballot masks; the
// conditional subtraction takes two more for the comparison and two for the
// borrows.  e's bits are uniform, so the chain branches on them.  Both limb
// counts are one kernel (the key's count picks the instance, uniformly), so a
// call that mixes keys is still one launch; the host puts the 128-limb items
// first.
//
// The raw form stores the result; the verify form compares it in registers
// with the encoding of the item's digest (rsa_em_limb) and stores one byte.
#include <hip/hip_runtime.h>

#include "ec_internal.hpp"
#include "rsa_common.hpp"

namespace vds_ec {

namespace {

__device__ __forceinline__ uint32_t lane_bcast(uint32_t v, int lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

// x >= y over the wave's digits (lane 63 the most significant)
template <int K>
__device__ __forceinline__ bool wave_ge(const uint32_t (&x)[K], const uint32_t (&y)[K]) {
  bool gt = false, eq = true;
#pragma unroll
  for (int j = K - 1; j >= 0; --j) {
    gt = gt || (eq && x[j] > y[j]);
    eq = eq && x[j] == y[j];
  }
  const uint64_t ne = ~__ballot(eq), g = __ballot(gt);
  return ne == 0 || ((g >> (63 - __clzll((long long)ne))) & 1u);
}

// r = a b R^-1 mod n for a, b < n (r may be a or b)
template <int K>
__device__ __forceinline__ void mont(const uint32_t (&a)[K], const uint32_t (&b)[K], const uint32_t (&n)[K],
                                     uint32_t n0inv, uint32_t lane, uint32_t (&r)[K]) {
  uint64_t acc[K];
#pragma unroll
  for (int j = 0; j < K; ++j) acc[j] = 0;
  for (int src = 0; src < 64; ++src) {
#pragma unroll
    for (int w = 0; w < K; ++w) {
      const uint32_t ai = lane_bcast(a[w], src);
      uint64_t p[K], q[K];
#pragma unroll
      for (int j = 0; j < K; ++j) p[j] = (uint64_t)ai * b[j];
      acc[0] += (uint32_t)p[0];
      const uint32_t m = lane_bcast((uint32_t)acc[0] * n0inv, 0);
#pragma unroll
      for (int j = 0; j < K; ++j) q[j] = (uint64_t)m * n[j];
      acc[0] += (uint32_t)q[0];
#pragma unroll
      for (int j = 1; j < K; ++j) acc[j] += (uint64_t)(uint32_t)p[j] + (uint32_t)q[j];
      // one limb down: lane 0's column 0 is zero in its low half now, and its high half joins the new column 0
      const uint64_t low = acc[0];
      uint64_t in = __shfl_down(low, 1);
      if (lane == 63) in = 0;
#pragma unroll
      for (int j = 0; j + 1 < K; ++j) acc[j] = acc[j + 1];
      acc[K - 1] = in;
      if (lane == 0) acc[0] += low >> 32;
#pragma unroll
      for (int j = 0; j < K; ++j) acc[j] += (p[j] >> 32) + (q[j] >> 32);
    }
  }
  // the columns resolved: inside the lane, the lane's excess to the next lane, then the masks
  uint32_t d[K];
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    c += acc[j];
    d[j] = (uint32_t)c;
    c >>= 32;
  }
  const uint32_t excess = (uint32_t)c;  // < 2^10
  uint32_t cin = __shfl_up(excess, 1);
  if (lane == 0) cin = 0;
  bool ones = true;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint64_t x = (uint64_t)d[j] + cin;
    d[j] = (uint32_t)x;
    cin = (uint32_t)(x >> 32);
    ones = ones && d[j] == 0xFFFFFFFFu;
  }
  uint32_t over;
  const uint64_t carries = rsa_carry_in(__ballot(cin != 0), __ballot(ones), &over);
  const uint32_t top = lane_bcast(excess, 63) + over;  // the bit above the top limb
  cin = (uint32_t)(carries >> lane) & 1u;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint64_t x = (uint64_t)d[j] + cin;
    d[j] = (uint32_t)x;
    cin = (uint32_t)(x >> 32);
  }
  // [0, 2n): the one conditional subtraction
  if (top != 0 || wave_ge<K>(d, n)) {
    uint32_t bw = 0;
    bool zero = true;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const uint64_t x = (uint64_t)d[j] - n[j] - bw;
      d[j] = (uint32_t)x;
      bw = (uint32_t)(x >> 32) & 1u;
      zero = zero && d[j] == 0;
    }
    const uint64_t borrows = rsa_carry_in(__ballot(bw != 0), __ballot(zero), &over);
    bw = (uint32_t)(borrows >> lane) & 1u;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const uint64_t x = (uint64_t)d[j] - bw;
      d[j] = (uint32_t)x;
      bw = (uint32_t)(x >> 32) & 1u;
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j) r[j] = d[j];
}

template <int K, bool VERIFY>
__device__ __forceinline__ void rsa_item(const RsaLaunch &L, const RsaItem &it, const vds_ec_rsa_key *key,
                                         uint32_t lane) {
  const uint32_t nb = key->n_bytes, e = key->e, n0inv = key->n0inv;
  uint8_t *res = L.results + it.index;
  const uint8_t bad = VERIFY ? 0 : (uint8_t)VDS_EC_EINVAL;
  if (it.in_len != nb) {
    if (lane == 0) *res = bad;
    return;
  }
  uint32_t n[K], x[K], y[K];
  const uint8_t *in = reinterpret_cast<const uint8_t *>(it.in);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    n[j] = key->n[K * lane + j];
    y[j] = key->rr[K * lane + j];
    x[j] = rsa_be_limb(in, nb, K * lane + j);
  }
  if (wave_ge<K>(x, n)) {
    if (lane == 0) *res = bad;
    return;
  }
  mont<K>(x, y, n, n0inv, lane, x);  // s R
#pragma unroll
  for (int j = 0; j < K; ++j) y[j] = x[j];
  for (int b = 30 - __clz((int)e); b >= 0; --b) {
    mont<K>(y, y, n, n0inv, lane, y);
    if ((e >> b) & 1u) mont<K>(y, x, n, n0inv, lane, y);
  }
#pragma unroll
  for (int j = 0; j < K; ++j) x[j] = (lane == 0 && j == 0) ? 1u : 0u;
  mont<K>(y, x, n, n0inv, lane, y);
  if constexpr (VERIFY) {
    const uint8_t *h = L.digests + 32ull * it.digest;
    bool same = true;
#pragma unroll
    for (int j = 0; j < K; ++j) same = same && y[j] == rsa_em_limb(K * lane + j, nb, h);
    const uint64_t differ = __ballot(!same);
    if (lane == 0) *res = differ == 0 ? 1 : 0;
  } else {
    uint8_t *out = reinterpret_cast<uint8_t *>(it.out);
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
      for (uint32_t b = 0; b < 4; ++b) {
        const uint32_t pos = 4u * (K * lane + j) + b;
        if (pos < nb) out[nb - 1 - pos] = (uint8_t)(y[j] >> (8 * b));
      }
    if (lane == 0) *res = 0;
  }
}

template <bool VERIFY>
__global__ __launch_bounds__(64) void k_rsa_public(RsaLaunch L) {
  if (blockIdx.x >= L.count) return;
  const RsaItem it = L.items[blockIdx.x];
  const vds_ec_rsa_key *key = L.keys + it.key;
  const uint32_t lane = threadIdx.x;
  if (key->limbs == 128)
    rsa_item<2, VERIFY>(L, it, key, lane);
  else
    rsa_item<1, VERIFY>(L, it, key, lane);
}

}  // namespace

namespace api {  // (declared in api_rsa_batch.cpp, their one caller)

hipError_t launch_rsa_public(const RsaLaunch &l, hipStream_t s) {
  if (l.count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rsa_public<false>, dim3(l.count), dim3(64), 0, s, l);
  return hipGetLastError();
}

hipError_t launch_rsa_verify(const RsaLaunch &l, hipStream_t s) {
  if (l.count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rsa_public<true>, dim3(l.count), dim3(64), 0, s, l);
  return hipGetLastError();
}

}  // namespace api
}  // namespace vds_ec
