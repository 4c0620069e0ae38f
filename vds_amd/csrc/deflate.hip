// deflate.hip -- buffers of a batch deflated into zlib streams (RFC 1950 around
// RFC 1951) in one launch: the third step of the reference's client::save
// (dht_network_client.cpp:1107-1140; kernel/vds_data/deflate.cpp is zlib's
// deflate), the mirror of inflate.hip.  The algorithm is the library's own and
// is stated in deflate_common.hpp; deflate_host.cpp is its sequential form, and
// this kernel writes the same bytes.
//
// k_deflate_batch: ONE WAVE PER MESSAGE, a workgroup is one wave; the host
// orders the messages longest first.  What is the same in every lane -- the
// walk's position, the pending stored run, the output position, the bits
// carried between two writes -- comes out of ballots and v_readfirstlane_b32,
// so it lives in SGPRs and branches on it are scalar.  The 64 lanes:
//   match finding  a lane a position of the chunk: it hashes its four bytes,
//             reads the table in LDS, and measures its two candidates (the
//             table's and position - 1) byte by byte against the input in HBM;
//             lanes inside a match that an earlier chunk took measure nothing.
//             After a barrier the chunk's positions enter the table with an LDS
//             max-atomic, so the highest position of a slot stays whatever the
//             order of the lanes.
//   selection      the ballot of the lanes that hold a match is walked from
//             the first free position: the next set bit is the next match, the
//             lanes before it are literals, its length (one cross-lane read)
//             says where the walk goes on; at most 16 steps a chunk.  A lane
//             that holds a token stores it at the segment's count plus the
//             tokens below it (a prefix popcount) and counts its symbols with
//             LDS atomics.
//   the plan       one lane runs def_plan (deflate_common.hpp) on the
//             histograms: the host's code, so the host's trees.
//   emission       a lane a token (or a header item): code and extra bits, at
//             most 48; a wave prefix sum of the bit counts; the bits are ORed
//             into a staging area in LDS (atomics: two lanes may share a
//             dword); whole bytes leave for the output, the last bits stay.
//   stored         all lanes copy the run's bytes from the input.
//   Adler-32       every lane sums the byte it reads as a position of a chunk,
//             s1 as a plain sum and s2 as a sum of (position mod 65521) * byte,
//             combined once at the end as in inflate.hip.
//
// WHERE TOKENS WAIT between a segment's two passes: in LDS.  A segment is 56
// chunks, so at most 3584 tokens of 4 bytes.  LDS a workgroup: the table
// 16384 + the tokens 14336 + the plan 8660 + staging 400 = 39780 bytes, four
// workgroups (waves) a CU of 160 KiB (163840 / 39780 = 4.1), one a SIMD; 64
// chunks a segment would be 41828 bytes and three.  No device scratch at all.
//
// Input and output at any byte address: the input is read byte by byte (only
// bytes of the message), the output written byte by byte, every store behind a
// test against the capacity.  Nothing else is written but out_lens[idx].
#include <hip/hip_runtime.h>

#include "../../include/vds_ec.h"
#include "deflate_common.hpp"
#include "ec_internal.hpp"

namespace vds_ec {

namespace {

typedef const __attribute__((address_space(1))) uint8_t *def_gptr_u8;
typedef __attribute__((address_space(1))) uint8_t *def_gptr_w8;
typedef __attribute__((address_space(1))) uint32_t *def_gptr_w32;

constexpr uint32_t kDefStageWords = 100;  // 7 carried bits + 64 * 48: 97 dwords

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

struct DefLds {
  uint32_t hash[kDefHashSize];
  uint32_t tok[kDefSegment];
  DeflPlan plan;
  uint32_t stage[kDefStageWords];
};
static_assert(sizeof(DefLds) <= 40960, "four workgroups a CU");

// bits a .. b-1 (a < 64, a <= b <= 64)
__device__ __forceinline__ uint64_t bit_range(uint32_t a, uint32_t b) {
  const uint64_t hi = b >= 64u ? ~0ull : (1ull << b) - 1ull;
  return hi & ~((1ull << a) - 1ull);
}

struct DefWave {
  DefLds &m;
  uint32_t lane;
  def_gptr_u8 in;
  def_gptr_w8 out;
  uint32_t len, cap;
  uint32_t opos, cbits;    // bytes written; bits (below 8) waiting in stage[0]
  uint32_t pend0, pend1;   // the pending stored run
  uint32_t ntok;
  bool finished;
  uint64_t ad_a, ad_b;

  __device__ __forceinline__ void store(uint32_t at, uint32_t b) {
    if (at < cap) out[at] = (uint8_t)b;  // (cap is at least the bound: always)
  }

  // Every lane's nb bits of v (nb <= 48, 0: none), in lane order, behind the
  // carried bits; the whole bytes are written, the rest is carried.
  __device__ __forceinline__ void emit(uint64_t v, uint32_t nb) {
    uint32_t incl = nb;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d) incl += t;
    }
    const uint32_t total = cbits + uni((uint32_t)__shfl((int)incl, 63));
    if (nb) {
      const uint32_t off = cbits + incl - nb, w = off >> 5, sh = off & 31u;
      const uint32_t lo = (uint32_t)(v << sh);
      const uint64_t hi = v >> (32u - sh);
      if (lo) atomicOr(&m.stage[w], lo);
      if ((uint32_t)hi) atomicOr(&m.stage[w + 1u], (uint32_t)hi);
      if ((uint32_t)(hi >> 32)) atomicOr(&m.stage[w + 2u], (uint32_t)(hi >> 32));
    }
    __syncthreads();
    const uint32_t nbytes = total >> 3, rem = total & 7u;
    for (uint32_t i = lane; i < nbytes; i += 64u) store(opos + i, (m.stage[i >> 2] >> (8u * (i & 3u))) & 0xFFu);  // at most 7 steps
    const uint32_t carry = rem ? uni((m.stage[nbytes >> 2] >> (8u * (nbytes & 3u))) & 0xFFu) : 0u;
    __syncthreads();
    for (uint32_t i = lane; i < ((total + 31u) >> 5); i += 64u) m.stage[i] = 0u;  // at most 2 steps
    __syncthreads();
    if (lane == 0) m.stage[0] = carry;
    __syncthreads();
    opos += nbytes;
    cbits = rem;
  }
  __device__ __forceinline__ void align() {
    if (cbits) {
      if (lane == 0) {
        store(opos, m.stage[0] & 0xFFu);
        m.stage[0] = 0u;
      }
      __syncthreads();
      ++opos;
      cbits = 0;
    }
  }
  // the pending run as stored blocks; every step writes 65535 bytes or the rest
  __device__ __forceinline__ void flush_stored(bool final) {
    uint32_t r = pend1 - pend0, src = pend0;
    pend0 = pend1 = 0;
    if (!r && !final) return;
    do {
      const uint32_t t = r < kDefStoredMax ? r : kDefStoredMax;
      emit(final && t == r ? 1u : 0u, lane == 0 ? 3u : 0u);
      align();
      const uint32_t word = t | ((~t & 0xFFFFu) << 16);
      if (lane < 4u) store(opos + lane, (word >> (8u * lane)) & 0xFFu);
      opos += 4u;
      for (uint32_t i = lane; i < t; i += 64u) store(opos + i, in[src + i]);  // 64 bytes a step
      opos += t;
      src += t;
      r -= t;
    } while (r);
    if (final) finished = true;
  }
  __device__ __forceinline__ void reset_segment() {
    for (uint32_t i = lane; i < 288u; i += 64u) m.plan.lfreq[i] = 0u;
    if (lane < 32u) m.plan.dfreq[lane] = 0u;
    ntok = 0;
    __syncthreads();
  }
  __device__ __forceinline__ void end_segment(uint32_t start, uint32_t end, bool last) {
    __syncthreads();
    if (lane == 0) def_plan(m.plan);
    __syncthreads();
    const uint32_t dyn = uni(m.plan.dyn_bits);
    if ((uint64_t)dyn + kDefStoredSlack <= 8ull * (end - start)) {
      flush_stored(false);
      const uint32_t nhdr = uni(m.plan.nhdr);
      for (uint32_t base = 0; base < nhdr; base += 64u) {  // at most 6 steps
        const uint32_t i = base + lane;
        uint32_t e = i < nhdr ? m.plan.hdr[i] : 0u;
        if (i == 0u && last) e |= 1u;
        emit(e & 0xFFFFFFu, e >> 24);
      }
      for (uint32_t base = 0; base <= ntok; base += 64u) {  // the tokens, then the end-of-block code: at most 57 steps
        const uint32_t i = base + lane;
        uint64_t v = 0;
        uint32_t nb = 0;
        if (i < ntok) {
          v = def_token_bits(m.plan, m.tok[i], &nb);
        } else if (i == ntok) {
          v = m.plan.lcode[256];
          nb = m.plan.llen[256];
        }
        emit(v, nb);
      }
      finished = last;
    } else {
      if (pend1 == pend0) pend0 = start;
      pend1 = end;
    }
    reset_segment();
  }

  __device__ __forceinline__ uint32_t match(uint32_t at, uint32_t from, uint32_t maxn) const {  // at most 258 steps
    uint32_t n = 0;
    while (n < maxn && in[from + n] == in[at + n]) ++n;
    return n;
  }

  __device__ __forceinline__ uint32_t run() {
    if (lane < 2u) store(lane, lane == 0 ? kDefCmf : kDefFlg);
    opos = 2;
    for (uint32_t i = lane; i < kDefHashSize; i += 64u) m.hash[i] = 0u;
    for (uint32_t i = lane; i < kDefStageWords; i += 64u) m.stage[i] = 0u;
    reset_segment();
    uint32_t skip = 0, seg_start = 0, chunks = 0;
    const uint64_t below = (1ull << lane) - 1ull;
    // A chunk a step: len / 64 steps, rounded up (c cannot wrap: the bound of len is below 2^32).
    for (uint32_t c = 0; c < len; c += kDefChunk) {
      const uint32_t nvalid = len - c < kDefChunk ? len - c : kDefChunk;
      const uint32_t at = c + lane;
      const bool valid = lane < nvalid;
      const bool hashes = valid && len - at >= 4u;
      uint32_t b0 = 0, slot = 0, ml = 0, md = 0;
      if (valid) {
        b0 = in[at];
        ad_a += b0;
        ad_b += (uint64_t)(at % kAdlerMod) * b0;
      }
      if (hashes) slot = def_hash(b0 | ((uint32_t)in[at + 1u] << 8) | ((uint32_t)in[at + 2u] << 16) | ((uint32_t)in[at + 3u] << 24));
      if (valid && at >= skip) {
        const uint32_t maxn = len - at < kDefMaxMatch ? len - at : kDefMaxMatch;
        uint32_t l1 = 0, d1 = 0, l2 = 0;
        if (hashes) {
          const uint32_t h = m.hash[slot];
          if (h && at - (h - 1u) <= kDefMaxDist) {
            d1 = at - (h - 1u);
            l1 = match(at, h - 1u, maxn);
          }
        }
        if (at >= 1u && in[at - 1u] == b0) l2 = match(at, at - 1u, maxn);
        if (l2 >= l1 && l2 >= kDefMinMatch) {
          ml = l2;
          md = 1;
        } else if (l1 >= kDefMinMatch) {
          ml = l1;
          md = d1;
        }
      }
      __syncthreads();  // every lane has read the table
      if (hashes) atomicMax(&m.hash[slot], at + 1u);
      __syncthreads();
      // the greedy walk; a step takes a match of at least 4 positions or ends the chunk: at most 16 steps
      const uint64_t mask = __ballot(ml >= kDefMinMatch);
      uint32_t pr = skip > c ? skip - c : 0u;
      uint64_t taken = 0;
      while (pr < nvalid) {
        const uint64_t rest = mask >> pr;
        if (!rest) {
          taken |= bit_range(pr, nvalid);
          pr = nvalid;
          break;
        }
        const uint32_t nx = pr + (uint32_t)__builtin_ctzll(rest);
        taken |= bit_range(pr, nx + 1u);
        pr = nx + uni((uint32_t)__shfl((int)ml, (int)nx));
      }
      skip = c + pr;
      if ((taken >> lane) & 1ull) {
        const uint32_t i = ntok + (uint32_t)__popcll(taken & below);
        if (ml >= kDefMinMatch) {
          uint32_t eb, ev;
          m.tok[i] = def_match_token(ml, md);
          atomicAdd(&m.plan.lfreq[def_len_sym(ml, &eb, &ev)], 1u);
          atomicAdd(&m.plan.dfreq[def_dist_sym(md, &eb, &ev)], 1u);
        } else {
          m.tok[i] = b0;
          atomicAdd(&m.plan.lfreq[b0], 1u);
        }
      }
      ntok += (uint32_t)__popcll(taken);
      const bool last = len - c <= kDefChunk;
      if (++chunks == kDefSegChunks || last) {
        end_segment(seg_start, skip, last);
        seg_start = skip;
        chunks = 0;
      }
    }
    if (!finished) flush_stored(true);
    align();
    uint32_t a = (uint32_t)(ad_a % kAdlerMod), b = (uint32_t)(ad_b % kAdlerMod);
#pragma unroll
    for (int d = 32; d; d >>= 1) {  // (64 values below 65521: no overflow)
      a += (uint32_t)__shfl_xor((int)a, d);
      b += (uint32_t)__shfl_xor((int)b, d);
    }
    a = uni(a) % kAdlerMod;
    b = uni(b) % kAdlerMod;
    const uint32_t nm = len % kAdlerMod;
    const uint32_t s1 = (1u + a) % kAdlerMod;
    const uint32_t s2 = (uint32_t)((nm + (uint64_t)nm * a + kAdlerMod - b) % kAdlerMod);
    const uint32_t ad = (s2 << 16) | s1;
    if (lane < 4u) store(opos + lane, (ad >> (8u * (3u - lane))) & 0xFFu);
    opos += 4u;
    return opos;
  }
};

__global__ __launch_bounds__(64) void k_deflate_batch(const InflateMsg *msgs, uint64_t out_lens) {
  __shared__ DefLds m;
  const InflateMsg msg = msgs[blockIdx.x];
  DefWave w{m};
  w.lane = threadIdx.x;
  w.in = reinterpret_cast<def_gptr_u8>(msg.in);
  w.out = reinterpret_cast<def_gptr_w8>(msg.out);
  w.len = msg.len;
  w.cap = msg.cap;
  w.opos = w.cbits = 0;
  w.pend0 = w.pend1 = 0;
  w.ntok = 0;
  w.finished = false;
  w.ad_a = w.ad_b = 0;
  const uint32_t n = w.run();
  if (w.lane == 0) reinterpret_cast<def_gptr_w32>(out_lens)[msg.idx] = n;
}

}  // namespace

hipError_t launch_deflate_batch(const InflateMsg *msgs, uint32_t count, uint32_t *out_lens, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_deflate_batch, dim3(count), dim3(64), 0, s, msgs, reinterpret_cast<uint64_t>(out_lens));
  return hipGetLastError();
}

}  // namespace vds_ec
