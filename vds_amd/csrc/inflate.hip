// inflate.hip -- zlib streams (RFC 1950 around RFC 1951) of a batch inflated in
// one launch: the second step of the reference's client::restore
// (dht_network_client.cpp:1297-1316; kernel/vds_data/private/inflate_p.h is
// zlib's inflate), between the batched decrypt and the name check.
//
// k_inflate_batch: ONE WAVE PER STREAM, a workgroup is one wave.  A stream is
// a serial chain (a symbol's place in the input is known only once the symbol
// before it is decoded), so the parallelism is the batch, as for the CBC
// encrypt; the host orders the streams longest input first.  What is serial by
// nature -- the bit buffer, the block state, the symbol decode, the output
// position -- is the same in every lane (made so with v_readfirstlane_b32 at
// the LDS and input reads it comes from, so it lives in SGPRs and branches on
// it are scalar).  Everything around it uses the 64 lanes:
//   input     64 aligned dwords a load, one a lane; the bit buffer refills from
//             them with v_readlane_b32, 32 bits a step.  Only aligned dwords
//             holding at least one message byte are read; the bytes of the
//             last one behind the message are masked to zero, and past the end
//             the reader delivers zeros while `avail` -- the message bits not
//             yet consumed -- says how many of the bits are real.
//   tables    two-level lookup tables in LDS (inflate_common.hpp), built for
//             every dynamic block: the lengths are counted with LDS atomics,
//             the canonical first codes and the completeness check are 15
//             steps, a symbol's rank among those of its length comes from 15
//             ballots a 64 symbols, the second-level tables are sized a lane a
//             prefix and placed by a wave scan, and then each symbol's lane
//             fills its own replicated entries.  The fixed tables are built
//             the same way once a workgroup.
//   literals  gathered in one VGPR (lane i holds the i-th pending byte) and
//             stored 64 at a time, or when a match or the block's end needs
//             them in memory.
//   matches   all lanes copy: byte i of the match is byte i mod D of the D
//             bytes before it, all of them written before the match began, so
//             an overlapping copy (D < L, distance 1 runs included) is as
//             parallel as any other.
//   stored    all lanes copy the block's bytes from the input.
//   Adler-32  every lane sums the bytes it stores, s1 as a plain sum and s2 as
//             a sum of (position mod 65521) * byte; the two are combined once
//             at the stream's end: s2 = n + n * sum(b) - sum(i * b_i).
//
// THE WINDOW is the stream's own output in HBM: a match reads back what the
// wave stored.  LDS then holds tables only (under 5 KiB a wave), so the waves a
// CU holds are bounded by its wave slots and not by a 32 KiB ring a wave (which
// would give 4 a CU); the decode is a chain of dependent LDS and SALU steps, and
// other waves are what hides it.  What makes a lane's load see the byte another
// lane of the same wave stored an instruction earlier: a wave's vector memory
// instructions are issued and reach its CU's L1 in program order, so at
// wavefront scope the memory model needs no cache action and no wait; what is
// left is the compiler, and wave_fence() -- a wavefront-scope acq_rel fence,
// which emits no instruction -- sits between the stores and the loads so that
// it may not move one across the other.  The same lane's store-then-load is
// ordinary program order.
//
// Statuses as vds_ec.h says; the order of events is zlib's, restated on one CPU
// thread by inflate_host.cpp, which the tests pin to zlib.
#include <hip/hip_runtime.h>

#include "../../include/vds_ec.h"
#include "ec_internal.hpp"
#include "inflate_common.hpp"

namespace vds_ec {

namespace {

typedef const __attribute__((address_space(1))) uint32_t *inf_gptr_u32;
typedef const __attribute__((address_space(1))) int32_t *inf_gptr_i32;
typedef const __attribute__((address_space(1))) uint8_t *inf_gptr_u8;
typedef __attribute__((address_space(1))) uint8_t *inf_gptr_w8;
typedef __attribute__((address_space(1))) uint32_t *inf_gptr_w32;
typedef __attribute__((address_space(1))) int32_t *inf_gptr_wi32;

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// zlib's inflate_table by 64 lanes (all of them call it, with the same
// arguments): 0, or 1 for an over-subscribed set and for an incomplete one
// (allowed only with a single code of one bit; never for the code-length code,
// `codes`, whose empty form decodes every lookup as symbol 0 of one bit).
// lens, T, cnt, first: LDS.  Every loop is bounded by a constant: n <= 320.
__device__ __forceinline__ int build_table(const uint8_t *lens, uint32_t n, uint32_t root, inf_entry_t *T, uint32_t cap,
                                           bool codes, uint32_t *cnt, uint32_t *first, uint32_t lane) {
  if (lane < 16u) cnt[lane] = 0u;
  __syncthreads();
  for (uint32_t i = lane; i < n; i += 64u) {
    const uint32_t l = lens[i];
    if (l) atomicAdd(&cnt[l], 1u);
  }
  __syncthreads();
  int left = 1;
  uint32_t code = 0, prev = 0, maxl = 0, p0 = 0;
  uint32_t run[16];
#pragma unroll
  for (uint32_t l = 1; l <= 15u; ++l) {
    const uint32_t c = uni(cnt[l]);
    code = (code + prev) << 1;
    prev = c;
    run[l] = code;
    if (lane == 0) first[l] = code;
    left = (left << 1) - (int)c;
    if (left < 0) return 1;
    if (c) maxl = l;
    if (l <= root) p0 += c << (root - l);
  }
  const uint32_t nroot = 1u << root;
  if (maxl == 0 || !(left > 0 && (codes || maxl != 1u))) {
    const inf_entry_t e0 = maxl == 0 && codes ? inf_entry(kInfSym, 1, 0) : kInfInvalidEntry;
    for (uint32_t i = lane; i < nroot; i += 64u) T[i] = e0;
  }
  __syncthreads();
  if (maxl == 0) return 0;
  if (left > 0 && (codes || maxl != 1u)) return 1;
  if (maxl > root) {
    // the second-level tables: lane's prefixes p = lane * per .. + per - 1
    const uint32_t per = nroot / 64u;
    uint32_t Ls[8], mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
      const uint32_t p = lane * per + j;
      Ls[j] = j < per && p >= p0 ? inf_sub_len(cnt, first, root, p) : 0u;
      if (Ls[j]) mine += 1u << (Ls[j] - root);
    }
    uint32_t incl = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d) incl += t;
    }
    const uint32_t total = uni((uint32_t)__shfl((int)incl, 63));
    if (nroot + total > cap) return 1;  // (cannot be: zlib's ENOUGH)
    uint32_t off = nroot + incl - mine;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j)
      if (Ls[j]) {
        T[inf_brev(lane * per + j, root)] = inf_entry(kInfLink, Ls[j] - root, off);
        off += 1u << (Ls[j] - root);
      }
    __syncthreads();
  }
  // ranks in symbol order, 64 symbols a step (at most 5 steps), then the entries
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t base = 0; base < n; base += 64u) {
    const uint32_t sym = base + lane;
    const uint32_t l = sym < n ? lens[sym] : 0u;
    uint32_t code_of = 0;
#pragma unroll
    for (uint32_t ll = 1; ll <= 15u; ++ll) {
      const uint64_t mask = __ballot(l == ll);
      if (l == ll) code_of = run[ll] + (uint32_t)__popcll(mask & below);
      run[ll] += (uint32_t)__popcll(mask);
    }
    if (l) inf_fill_symbol(T, cap, root, sym, l, code_of);
  }
  __syncthreads();
  return 0;
}

// the entry of the next code, its bits the total over both levels
__device__ __forceinline__ uint32_t lookup(const inf_entry_t *T, uint32_t root, uint32_t bits) {
  const uint32_t e = uni(T[bits & ((1u << root) - 1u)]);
  if (inf_kind(e) != kInfLink) return e;
  const uint32_t e2 = uni(T[inf_val(e) + ((bits >> root) & ((1u << inf_nbits(e)) - 1u))]);
  return (e2 & ~15u) | (root + inf_nbits(e2));
}

struct Lds {
  inf_entry_t fixlit[kInfFixLitCap], fixdist[kInfFixDistCap], lit[kInfLitCap], dist[kInfDistCap], cl[kInfClCap];
  uint32_t cnt[16], first[16];
  uint8_t lens[kInfMaxSyms], cll[32];
};

struct Wave {
  uint32_t lane;
  // the input: aligned base, misalignment, length; 64 dwords from cbase on, one a lane; the bit buffer
  inf_gptr_u32 p;
  uint64_t in, lim;
  uint32_t sh, len, chunk, cbase, widx;
  uint64_t hold, avail;
  uint32_t n;
  // the output: pos bytes stored, nlit literals pending (lane i holds the i-th)
  uint64_t out;
  uint32_t cap, pos, nlit, litbuf;
  uint64_t ad_a, ad_b;

  __device__ __forceinline__ void load_chunk(uint32_t base) {
    cbase = base;
    const uint64_t b = 4ull * ((uint64_t)base + lane);
    uint32_t v = 0;
    if (b < lim) {  // the dword holds a message byte
      v = p[base + lane];
      if (b + 4u > lim) v &= (1u << (8u * (uint32_t)(lim - b))) - 1u;
    }
    chunk = v;
  }
  __device__ __forceinline__ uint32_t next_dword() {
    if (widx - cbase >= 64u) load_chunk(widx);
    const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)chunk, (int)(widx - cbase));
    ++widx;
    return v;
  }
  // (re)start at the message's byte b
  __device__ __forceinline__ void seek(uint32_t b) {
    const uint64_t a = (uint64_t)sh + b;
    widx = (uint32_t)(a >> 2);
    load_chunk(widx);
    const uint32_t s = 8u * (uint32_t)(a & 3u);
    hold = next_dword() >> s;
    n = 32u - s;
    avail = 8ull * (len - b);
  }
  __device__ __forceinline__ void fill() {  // at least 33 bits, one step
    if (n <= 32u) {
      hold |= (uint64_t)next_dword() << n;
      n += 32u;
    }
  }
  __device__ __forceinline__ uint32_t peek(uint32_t k) const { return (uint32_t)hold & (uint32_t)((1ull << k) - 1ull); }
  __device__ __forceinline__ void drop(uint32_t k) {  // k <= avail, k <= n
    hold >>= k;
    n -= k;
    avail -= k;
  }

  __device__ __forceinline__ void adler(uint32_t byte, uint32_t i) {
    ad_a += byte;
    ad_b += (uint64_t)(i % kAdlerMod) * byte;
  }
  __device__ __forceinline__ void flush() {
    if (nlit) {
      if (lane < nlit) {
        const uint32_t b = litbuf & 0xFFu;
        reinterpret_cast<inf_gptr_w8>(out)[pos + lane] = (uint8_t)b;
        adler(b, pos + lane);
      }
      pos += nlit;
      nlit = 0;
    }
  }
  __device__ __forceinline__ void literal(uint32_t sym) {
    if (lane == nlit) litbuf = sym;
    if (++nlit == 64u) flush();
  }
  // D <= pos, pos + L <= cap, nothing pending.  At most 5 steps (L <= 258).
  __device__ __forceinline__ void copy_match(uint32_t D, uint32_t L) {
    wave_fence();  // the stores before this, by any lane, and the loads below
    const inf_gptr_w8 o = reinterpret_cast<inf_gptr_w8>(out);
    for (uint32_t i = lane; i < L; i += 64u) {
      const uint32_t from = D >= L ? i : i % D;  // < D: a byte from before the match
      const uint32_t b = o[pos - D + from];
      o[pos + i] = (uint8_t)b;
      adler(b, pos + i);
    }
    pos += L;
  }
  // the message's bytes src .. src + take - 1 (all inside it), pos + take <=
  // cap.  Every step consumes 64 input bytes, or the last ones.
  __device__ __forceinline__ void copy_stored(uint32_t src, uint32_t take) {
    const inf_gptr_u8 s = reinterpret_cast<inf_gptr_u8>(in);
    const inf_gptr_w8 o = reinterpret_cast<inf_gptr_w8>(out);
    for (uint32_t i = lane; i < take; i += 64u) {
      const uint32_t b = s[src + i];
      o[pos + i] = (uint8_t)b;
      adler(b, pos + i);
    }
    pos += take;
  }

  __device__ __forceinline__ int run(Lds &m) {
    seek(0);
    fill();
    if (avail < 16u) return VDS_EC_EINFLATE_SHORT;
    const uint32_t cmf = peek(8), flg = peek(16) >> 8;
    if (((cmf << 8) + flg) % 31u || (cmf & 15u) != 8u || (cmf >> 4) > 7u) return VDS_EC_EINFLATE_DATA;
    drop(16);
    if (flg & 0x20u) return avail < 32u ? VDS_EC_EINFLATE_SHORT : VDS_EC_EINFLATE_DATA;
    // TERMINATION.  Every block consumes its three header bits, every code
    // length its code, every symbol of a compressed block its literal/length
    // code, every step of a stored copy its bytes: each at least one bit, all
    // inside the message, because the test against `avail` -- the message bits
    // not yet consumed -- stands before every drop, and a step that finds too
    // few returns.  avail only falls, so the loops below end after at most 8 *
    // len iterations in all; every other loop (fill, the table builds, a
    // match's copy, the repeats of a code length) is bounded by a constant.
    for (;;) {
      fill();
      if (avail < 3u) return VDS_EC_EINFLATE_SHORT;
      const uint32_t last = peek(1), type = peek(3) >> 1;
      drop(3);
      const inf_entry_t *LT = nullptr, *DT = nullptr;
      if (type == 0u) {
        drop((uint32_t)avail & 7u);
        if (avail < 32u) return VDS_EC_EINFLATE_SHORT;
        fill();
        const uint32_t w = (uint32_t)hold, cnt = w & 0xFFFFu;
        if (cnt != (~(w >> 16) & 0xFFFFu)) return VDS_EC_EINFLATE_DATA;
        drop(32);
        const uint32_t there = (uint32_t)(avail >> 3), src = len - there;
        const uint32_t take = cnt < there ? cnt : there;
        flush();
        if ((uint64_t)pos + take > cap) return VDS_EC_EINFLATE_SPACE;
        copy_stored(src, take);
        seek(src + take);
        if (take < cnt) return VDS_EC_EINFLATE_SHORT;
      } else if (type == 1u) {
        LT = m.fixlit;
        DT = m.fixdist;
      } else if (type == 2u) {
        if (avail < 14u) return VDS_EC_EINFLATE_SHORT;
        const uint32_t nlen = peek(5) + 257u, ndist = (peek(10) >> 5) + 1u, ncode = (peek(14) >> 10) + 4u;
        drop(14);
        if (nlen > 286u || ndist > 30u) return VDS_EC_EINFLATE_DATA;
        if (lane < 32u) m.cll[lane] = 0;
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < 19u; ++i)
          if (i < ncode) {
            fill();
            if (avail < 3u) return VDS_EC_EINFLATE_SHORT;
            if (lane == 0) m.cll[kInfClOrder[i]] = (uint8_t)peek(3);
            drop(3);
          }
        if (build_table(m.cll, 19, kInfClRoot, m.cl, kInfClCap, true, m.cnt, m.first, lane)) return VDS_EC_EINFLATE_DATA;
        const uint32_t total = nlen + ndist;
        uint32_t before = 0;  // the length before this one
        for (uint32_t have = 0; have < total;) {  // (a step: at least one bit consumed, at least one length added)
          fill();
          const uint32_t e = lookup(m.cl, kInfClRoot, (uint32_t)hold), nb = inf_nbits(e), sym = inf_val(e);
          if (nb > avail) return VDS_EC_EINFLATE_SHORT;
          if (sym < 16u) {
            drop(nb);
            if (lane == 0) m.lens[have] = (uint8_t)sym;
            ++have;
            before = sym;
            continue;
          }
          const uint32_t x = sym == 16u ? 2u : sym == 17u ? 3u : 7u;
          if (nb + x > avail) return VDS_EC_EINFLATE_SHORT;
          drop(nb);
          if (sym == 16u && have == 0) return VDS_EC_EINFLATE_DATA;
          const uint32_t v = sym == 16u ? before : 0u;
          const uint32_t rep = (sym == 18u ? 11u : 3u) + peek(x);
          drop(x);
          if (have + rep > total) return VDS_EC_EINFLATE_DATA;
          for (uint32_t i = lane; i < rep; i += 64u) m.lens[have + i] = (uint8_t)v;  // rep <= 138
          have += rep;
          before = v;
        }
        __syncthreads();
        if (uni(m.lens[256]) == 0u) return VDS_EC_EINFLATE_DATA;
        if (build_table(m.lens, nlen, kInfLitRoot, m.lit, kInfLitCap, false, m.cnt, m.first, lane))
          return VDS_EC_EINFLATE_DATA;
        if (build_table(m.lens + nlen, ndist, kInfDistRoot, m.dist, kInfDistCap, false, m.cnt, m.first, lane))
          return VDS_EC_EINFLATE_DATA;
        LT = m.lit;
        DT = m.dist;
      } else {
        return VDS_EC_EINFLATE_DATA;
      }
      while (LT) {  // (a step: the bits of one literal/length code consumed, or the loop left)
        fill();
        uint32_t e = lookup(LT, kInfLitRoot, (uint32_t)hold), nb = inf_nbits(e);
        if (nb > avail) return VDS_EC_EINFLATE_SHORT;
        if (inf_kind(e) == kInfInvalid || nb == 0) return VDS_EC_EINFLATE_DATA;
        const uint32_t sym = inf_val(e);
        if (sym < 256u) {
          if (pos + nlit >= cap) return VDS_EC_EINFLATE_SPACE;
          literal(sym);
          drop(nb);
          continue;
        }
        if (sym == 256u) {
          drop(nb);
          break;
        }
        if (sym > 285u) return VDS_EC_EINFLATE_DATA;
        uint32_t x = 0;
        const uint32_t lbase = inf_len_base(sym, &x);
        if (nb + x > avail) return VDS_EC_EINFLATE_SHORT;
        drop(nb);
        const uint32_t L = lbase + peek(x);
        drop(x);
        fill();
        e = lookup(DT, kInfDistRoot, (uint32_t)hold);
        nb = inf_nbits(e);
        if (nb > avail) return VDS_EC_EINFLATE_SHORT;
        if (inf_kind(e) == kInfInvalid || nb == 0 || inf_val(e) >= 30u) return VDS_EC_EINFLATE_DATA;
        const uint32_t dbase = inf_dist_base(inf_val(e), &x);
        if (nb + x > avail) return VDS_EC_EINFLATE_SHORT;
        drop(nb);
        const uint32_t D = dbase + peek(x);
        drop(x);
        // "invalid distance too far back": an error, not a read -- which zlib looks for only once the
        // match's first byte has room
        if (D > pos + nlit) return pos + nlit >= cap ? VDS_EC_EINFLATE_SPACE : VDS_EC_EINFLATE_DATA;
        if ((uint64_t)pos + nlit + L > cap) return VDS_EC_EINFLATE_SPACE;
        flush();
        copy_match(D, L);
      }
      if (last) break;
    }
    flush();
    drop((uint32_t)avail & 7u);
    if (avail < 32u) return VDS_EC_EINFLATE_SHORT;
    fill();
    const uint32_t t = (uint32_t)hold;
    const uint32_t want = (t >> 24) | ((t >> 8) & 0xFF00u) | ((t << 8) & 0xFF0000u) | (t << 24);
    uint32_t a = (uint32_t)(ad_a % kAdlerMod), b = (uint32_t)(ad_b % kAdlerMod);
#pragma unroll
    for (int d = 32; d; d >>= 1) {  // (64 values below 65521: no overflow)
      a += (uint32_t)__shfl_xor((int)a, d);
      b += (uint32_t)__shfl_xor((int)b, d);
    }
    a = uni(a) % kAdlerMod;
    b = uni(b) % kAdlerMod;
    const uint32_t nm = pos % kAdlerMod;
    const uint32_t s1 = (1u + a) % kAdlerMod;
    const uint32_t s2 = (uint32_t)((nm + (uint64_t)nm * a + kAdlerMod - b) % kAdlerMod);
    return want == ((s2 << 16) | s1) ? VDS_EC_OK : VDS_EC_EINFLATE_DATA;
  }
};

__global__ __launch_bounds__(64) void k_inflate_batch(InflateLaunch l) {
  __shared__ Lds m;
  const uint32_t lane = threadIdx.x;
  const InflateMsg msg = l.msgs[blockIdx.x];
  const inf_gptr_wi32 st_out = reinterpret_cast<inf_gptr_wi32>(l.statuses) + msg.idx;
  const inf_gptr_w32 len_out = reinterpret_cast<inf_gptr_w32>(l.out_lens) + msg.idx;
  uint32_t len = msg.len;
  if (l.gate) {  // (the whole workgroup)
    const int32_t g = (int32_t)uni((uint32_t)reinterpret_cast<inf_gptr_i32>(l.gate)[msg.idx]);
    if (g != VDS_EC_OK) {
      if (lane == 0) {
        *st_out = g;
        *len_out = 0u;
      }
      return;
    }
  }
  if (l.in_lens) len = min(len, uni(reinterpret_cast<inf_gptr_u32>(l.in_lens)[msg.idx]));

  for (uint32_t i = lane; i < 288u; i += 64u) m.lens[i] = i < 144u ? 8 : i < 256u ? 9 : i < 280u ? 7 : 8;
  build_table(m.lens, 288, kInfLitRoot, m.fixlit, kInfFixLitCap, false, m.cnt, m.first, lane);
  if (lane < 32u) m.lens[lane] = 5;
  build_table(m.lens, 32, kInfDistRoot, m.fixdist, kInfFixDistCap, false, m.cnt, m.first, lane);

  Wave w;
  w.lane = lane;
  w.in = msg.in;
  w.sh = (uint32_t)(msg.in & 3u);
  w.p = reinterpret_cast<inf_gptr_u32>(msg.in - w.sh);
  w.len = len;
  w.lim = len ? (uint64_t)len + w.sh : 0;
  w.chunk = w.cbase = w.widx = 0;
  w.hold = 0;
  w.n = 0;
  w.avail = 0;
  w.out = msg.out;
  w.cap = msg.cap;
  w.pos = w.nlit = w.litbuf = 0;
  w.ad_a = w.ad_b = 0;
  const int st = w.run(m);
  if (st == VDS_EC_EINFLATE_SHORT) w.flush();  // what was delivered is valid
  if (lane == 0) {
    *st_out = st;
    *len_out = st == VDS_EC_OK || st == VDS_EC_EINFLATE_SHORT ? w.pos : 0u;
  }
}

}  // namespace

hipError_t launch_inflate_batch(const InflateLaunch &l, hipStream_t s) {
  if (l.count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_inflate_batch, dim3(l.count), dim3(64), 0, s, l);
  return hipGetLastError();
}

}  // namespace vds_ec
