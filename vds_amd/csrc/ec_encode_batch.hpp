// ec_encode_batch.hpp -- k_encode_batch<K,N>: the bit-sliced encode of
// ec_encode.hpp over a batch of objects of different sizes, every stripe of
// every object in one launch (vds_ec_encode16_batch_device).
//
// The transposes, the LDS layout, the Taylor steps and the pair / quad
// evaluation are ec_encode.hpp's, unchanged.  What differs is where a tile's
// cells come from and where its replica cells go: each of a tile's sixteen
// 128-stripe groups is (object, group of that object) from a device table
// (EncBatchTile), and the object's input, size and replica addresses come
// from its descriptor (EncBatchObj).  The last group of an object has v <= 128
// valid stripes and its last stripe may be partial: loads beyond the object's
// last byte are not issued (the missing bytes are zero, chunk.h:251-268) and
// stores beyond cell T-1 are masked, so no generic launch is needed for tails
// or trailers, and no byte outside [in, in + size) and the replicas' own L
// bytes is touched.
//
// This header defines VDS_ENC_BATCH before it includes ec_encode.hpp: the
// evaluation code's store_rep() then forwards to store_replica_batch() below,
// and everything ec_encode.hpp declares lands in the inline namespace
// vds_ec::enc_batch, so the translation units of the uniform kernels and of
// the batch kernels never hold two definitions of one entity.
#pragma once

#define VDS_ENC_BATCH 1

#include "ec_device.hpp"

namespace vds_ec {
inline namespace enc_batch {

// The kernel's arguments: `fa` first (offset 0), because the evaluation code
// fetches its replica "pointers" from FastEncodeArgs::outs in the kernarg
// segment (rep_ptr).  In batch mode outs[r] holds the replica id r itself.
struct EncodeBatchArgs {
  FastEncodeArgs fa;  // total_tiles and outs[r] = r; the other fields unused
  const EncBatchObj *objs;
  const EncBatchTile *tiles;
  uint32_t trailer;  // 1: write each object's BE16 trailer (size mod 2k) after cell T-1
};

typedef const __attribute__((address_space(4))) EncodeBatchArgs *BatchKernarg;
__device__ __forceinline__ BatchKernarg batch_kernarg() {
  return (BatchKernarg)__builtin_amdgcn_kernarg_segment_ptr();
}

// Where the current tile's sixteen groups store, worked out once per tile
// from the tables (publish_info) and kept in the first kInfoBytes of
// the workgroup's LDS, 32 bytes a group:
//   dwords 0-1  out     the object's replica base, or its pointer table
//   dwords 2-3  pitch   bytes between its replicas, or kEncBatchPtrTable
//   dwords 4-5  off     256 q: the group's offset in every replica
//   dword  6    v       valid stripes of the group (0: an unused group)
//   dword  7    trl     the object's trailer as stored (big-endian) when this
//                       is its last group and trailers are written, else bit 31
// then, 16 bytes a group, where the NEXT tile's groups load (the prefetch):
//   dwords 0-1  src     the group's first input byte
//   dword  2    nb      the group's bytes inside the object (0 .. 256 k)
// The sixty-odd replica stores of a tile each need all of the store info.
// Read from the tables by scalar loads at every use, the compiler hoists and
// keeps them: 1200-2200 SGPR spills at 106 SGPRs (and 25-30 for the loads
// alone).  From LDS they are 32 uniform ds_read_b128 a replica, and live only
// as long as one group's stores.
constexpr int kStoreInfoBytes = 16 * 32;
constexpr int kInfoBytes = kStoreInfoBytes + 16 * 16;
constexpr uint32_t kNoTrailer = 0x80000000u;

__device__ __forceinline__ uint32_t *batch_lds() {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  return lds;
}

__device__ __forceinline__ uint64_t uniform64(uint32_t lo, uint32_t hi) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)lo) |
         (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)hi) << 32;
}

// Replica `rep` (its id, as rep_ptr returns it in batch mode) of the current
// tile's sixteen groups.  Word j of lane s holds the cells of stripes 2s and
// 2s + 1 of group j (ec_encode.hpp, map 3): the dword goes out when both are
// below the group's v valid stripes, its low half when only the first is,
// nothing otherwise.  Lane 0 of an object's last group also writes the
// object's trailer.  v, the addresses and the trailer are wave-uniform
// (readfirstlane), so only the two store masks diverge, and only in an
// object's last group.
template <bool ROT>
__device__ __forceinline__ void store_replica_batch(const Plane16 &acc, uint8_t *rep, int lane, const BitMasks &bm) {
  uint32_t rows[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) rows[j] = acc.p[j ^ 8];  // word bit j <-> cell bit j^8 (BE)
  transpose16x2<ROT>(rows, bm);
  const uint64_t r = (uint64_t)rep;
  lds_u32x4 *info = (lds_u32x4 *)batch_lds();
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const u32x4 a = info[2 * j], b = info[2 * j + 1];
    const uint32_t v = (uint32_t)__builtin_amdgcn_readfirstlane((int)b.z);
    if (v == 0) continue;  // an unused group of the batch's last tile
    const uint64_t out = uniform64(a.x, a.y), pitch = uniform64(a.z, a.w), off = uniform64(b.x, b.y);
    const uint32_t trl = (uint32_t)__builtin_amdgcn_readfirstlane((int)b.w);
    uint8_t *base = (pitch == kEncBatchPtrTable ? s_ld(reinterpret_cast<uint8_t *const *>(out) + r)
                                                : reinterpret_cast<uint8_t *>(out) + r * pitch) +
                    off;
    uint8_t *p = base + 4 * lane;
    if ((uint32_t)(2 * lane + 1) < v)
      g_st<1>(p, rows[j]);
    else if ((uint32_t)(2 * lane) < v)
      *(gmem<uint16_t> *)p = (uint16_t)rows[j];
    if (trl != kNoTrailer && lane == 0) *(gmem<uint16_t> *)(base + 2 * v) = (uint16_t)trl;
  }
}

}  // namespace enc_batch
}  // namespace vds_ec

#include "ec_encode.hpp"

namespace vds_ec {
inline namespace enc_batch {

// Tile `tile`'s store info (STORE) or load info into LDS: the waves share the
// sixteen groups, each reads its groups' table entries and descriptors with
// scalar loads and lane 0 writes the entry.  The caller's barriers order it
// against the stores and loads that read it.
template <int K, int WV, bool STORE>
__device__ __forceinline__ void publish_info(uint32_t tile, int wave, int lane) {
  constexpr uint64_t B = 2 * K, G = 128 * B;
  const BatchKernarg ka = batch_kernarg();
  const EncBatchTile *tl = ka->tiles + tile;
  const uint32_t trailer = ka->trailer;
  lds_v4 *info = (lds_v4 *)batch_lds();
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (wave != j % WV) continue;
    const uint32_t q = s_ld(&tl->q[j]);
    const EncBatchObj *d = ka->objs + s_ld(&tl->obj[j]);
    const uint64_t size = s_ld(&d->size);
    if constexpr (!STORE) {
      const uint64_t g0 = (uint64_t)q * G, src = (uint64_t)s_ld(&d->in) + g0;
      const uint32_t nb = size <= g0 ? 0u : (size - g0 < G ? (uint32_t)(size - g0) : (uint32_t)G);
      if (lane == 0) info[kStoreInfoBytes / 16 + j] = u32x4{(uint32_t)src, (uint32_t)(src >> 32), nb, 0u};
      continue;
    }
    const uint64_t out = s_ld(&d->out), pitch = s_ld(&d->pitch);
    const uint64_t T = (size + B - 1) / B, t0 = 128ull * q, off = 2 * t0;
    const uint32_t v = T <= t0 ? 0u : (T - t0 < 128 ? (uint32_t)(T - t0) : 128u);
    const uint32_t pad = (uint32_t)(size % B);
    const uint32_t trl = (trailer && v && t0 + v == T) ? ((pad >> 8) | ((pad & 0xFFu) << 8)) : kNoTrailer;
    if (lane == 0) {
      info[2 * j] = u32x4{(uint32_t)out, (uint32_t)(out >> 32), (uint32_t)pitch, (uint32_t)(pitch >> 32)};
      info[2 * j + 1] = u32x4{(uint32_t)off, (uint32_t)(off >> 32), v, trl};
    }
  }
}

// The first `valid` (1..15) bytes at src (4-byte aligned) as a zero-padded
// chunk: whole dwords, then the last dword's bytes one by one, so nothing
// beyond the object's last byte is read.
__device__ __forceinline__ u32x4 load_chunk_partial(const uint8_t *src, uint32_t valid) {
  uint32_t w[4] = {0, 0, 0, 0};
  const uint32_t nd = valid >> 2, nb = valid & 3;
#pragma unroll
  for (uint32_t i = 0; i < 3; ++i)
    if (i < nd) w[i] = *(const gmem<uint32_t> *)(src + 4 * i);
  uint32_t t = 0;
#pragma unroll
  for (uint32_t b = 0; b < 3; ++b)
    if (b < nb) t |= (uint32_t)(*(const gmem<uint8_t> *)(src + 4 * nd + b)) << (8 * b);
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i)
    if (i == nd) w[i] = t;
  return u32x4{w[0], w[1], w[2], w[3]};
}

// The 16-byte pair loads of encode_load16, per group as the load info in LDS
// says: a lane's chunk is loaded when it lies inside the object, assembled
// from its valid bytes when it straddles the object's end (one lane per
// object), and zero -- not loaded -- beyond it.
template <int K>
__device__ __forceinline__ void encode_load_batch(u32x4 (&V)[16], int set, int p) {
  constexpr uint32_t B = 2 * K;
  lds_u32x4 *info = (lds_u32x4 *)batch_lds() + kStoreInfoBytes / 16;
  const uint32_t lane_off = (uint32_t)(2 * set + (p & 1)) * B + 16u * (uint32_t)(p >> 1);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const u32x4 g = info[j];
    const uint32_t nb = g.z;
    const uint8_t *src = reinterpret_cast<const uint8_t *>(((uint64_t)g.y << 32 | g.x) + lane_off);
    u32x4 v = {0, 0, 0, 0};
    if (lane_off + 16 <= nb)
      v = g_ld<2, u32x4>(src);
    else if (lane_off < nb)
      v = load_chunk_partial(src, nb - lane_off);
    V[j] = v;
  }
}

// k_encode_bs's tile loop with the table-driven loads; the stores are
// store_replica_batch's through store_rep.  QUAD as k_encode_bs (the
// two-level split; else the one-level split).  LDS: the store info, then the
// planes (kInfoBytes keeps their bank alignment).
template <int K, int N, int RPW, int WV, bool QUAD>
__global__ __launch_bounds__((EncodeShape<K, N, RPW, WV>::kThreads), (EncodeShape<K, N, RPW, WV>::kWavesPerSimd))
void k_encode_batch(EncodeBatchArgs a) {
  using S = EncodeShape<K, N, RPW, WV>;
  static_assert(S::kMap == 3 && K >= 16, "batch mode: the pair-load shapes with a split mode");
  static_assert(kInfoBytes % 128 == 0, "the planes keep their banks");
  uint32_t *lds = batch_lds() + kInfoBytes / 4;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tset = wave * S::kSetsPerWave + lane / S::kLanesPerSet;
  const int tp = lane % S::kLanesPerSet;
  uint32_t *t_planes = lds + tset * S::kSetWords + S::cell_off(4 * tp);
  uint32_t *my_set = lds + lane * S::kSetWords;
  const BitMasks bm = bit_masks();
  u32x4 V[16];
  const bool par = (lane & 1) != 0;
  const TileRange tr = tile_range(a.fa.total_tiles);
  uint32_t tile = tr.first;
  const uint32_t t_end = tr.end, t_step = tr.step;
  if (tile < t_end) {
    publish_info<K, WV, false>(tile, wave, lane);
    publish_info<K, WV, true>(tile, wave, lane);
    __syncthreads();
    encode_load_batch<K>(V, tset, tp);
    // the first tile's stores with zero planes, under the same masks (see the
    // entry of k_encode_bs; the trailers they write are the final ones)
    if constexpr (QUAD)
      quad_zero_dispatch<K, N, RPW, WV, true, 0>(wave, a.fa, TilePos{tile, 0}, lane, bm);
    else
      pair_zero_dispatch<K, N, RPW, WV, true, 0>(wave, a.fa, TilePos{tile, 0}, lane, bm);
    __syncthreads();
  }
  for (; tile < t_end; tile += t_step) {
    // this tile's store info and the next tile's load info (their previous
    // readers are done: the barrier that ends a tile)
    const uint32_t next = tile + t_step;
    publish_info<K, WV, true>(tile, wave, lane);
    if (next < t_end) publish_info<K, WV, false>(next, wave, lane);
    uint32_t R[2][32];
    constexpr bool kPrio = 2 * (S::kLdsBytes + kInfoBytes) <= 160 * 1024;
    if constexpr (kPrio) __builtin_amdgcn_s_setprio(1);
    encode_unpack16(V, R, par);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      transpose32<enc_rot(K)>(R[g], bm);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int b0 = 16 * h + 4 * (m ^ 2);
          *reinterpret_cast<uint4 *>(t_planes + (2 * g + h) * 16 + 4 * m) =
              make_uint4(R[g][b0], R[g][b0 + 1], R[g][b0 + 2], R[g][b0 + 3]);
        }
    }
    if constexpr (kPrio) __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    if (next < t_end) encode_load_batch<K>(V, tset, tp);
    taylor_lds<K, N, RPW, WV>(wave, my_set);
    __syncthreads();
    if constexpr (QUAD) {
      quad_twist_lds<K, N, RPW, WV>(wave, my_set);
      __syncthreads();
      quad_taylor_lds<K, N, RPW, WV>(wave, my_set);
      __syncthreads();
      quad_dispatch<K, N, RPW, WV, true, 0>(wave, my_set, a.fa, TilePos{tile, 0}, lane, bm);
    } else {
      pair_dispatch<K, N, RPW, WV, true, 0>(wave, my_set, a.fa, TilePos{tile, 0}, lane, bm);
    }
    __syncthreads();
  }
}

template <int K, int N, int RPW, int WV, bool QUAD>
static hipError_t launch_encode_batch_shape(const EncBatchLaunch &b, hipStream_t s) {
  using S = EncodeShape<K, N, RPW, WV>;
  EncodeBatchArgs a{};
  a.fa.total_tiles = b.total_tiles;
  for (int r = 0; r < N; ++r) a.fa.outs[r] = reinterpret_cast<uint8_t *>((uintptr_t)r);
  a.objs = b.objs;
  a.tiles = b.tiles;
  a.trailer = b.trailer;
  const int lds = S::kLdsBytes + kInfoBytes;
  hipError_t e = ensure_lds_attr(&k_encode_batch<K, N, RPW, WV, QUAD>, lds);
  if (e != hipSuccess) return e;
  const int blocks_per_cu = (160 * 1024) / lds;
  int grid = 256 * (blocks_per_cu > 0 ? blocks_per_cu : 1);
  if ((uint32_t)grid > b.total_tiles) grid = (int)b.total_tiles;
  if (grid == 0) return hipSuccess;
  hipLaunchKernelGGL((k_encode_batch<K, N, RPW, WV, QUAD>), dim3(grid), dim3(S::kThreads), lds, s, a);
  return hipGetLastError();
}

}  // namespace enc_batch
}  // namespace vds_ec
