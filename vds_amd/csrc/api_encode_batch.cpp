// api_encode_batch.cpp -- vds_ec_encode16_batch_device / _path: one bit-sliced
// launch over a batch of objects of different sizes (k_encode_batch,
// ec_encode_batch.hpp), planned on the host.
// (api_internal.hpp lists the host runtime's translation units.)
#include "api_internal.hpp"

namespace vds_ec {
namespace api {

EncBatchScratch &enc_batch_scratch() {
  thread_local EncBatchScratch sc;
  return sc;
}

// The one pass: validate every object, classify it, sum the eligible objects'
// groups.  Shared by the dispatch and the path query, so the two cannot
// disagree; it dereferences the host arrays only, never a device pointer.
// An object rides the shared launch when (k, n) is a batch shape, replicas
// is 0..n-1, its input is 4-byte aligned (the pair loads' condition, as
// encode_device's fast path), its replica pointers are 2-byte aligned and
// its size is non-zero.
int plan_encode_batch(uint32_t k, const uint16_t *replicas, uint32_t n, uint32_t count, const uint8_t *const *ins,
                      const uint64_t *sizes, uint8_t *const *outs, unsigned flags, EncBatchScratch &sc) {
  sc.objs.clear();
  sc.ptrs.clear();
  sc.rest.clear();
  sc.groups = 0;
  if (k == 0 || (flags & VDS_EC_F_CELLS) || count >= (1u << 30)) return VDS_EC_EINVAL;
  if ((n && !replicas) || (count && (!ins || !sizes || (n && !outs)))) return VDS_EC_EINVAL;
  const uint64_t B = 2ull * k;
  bool shape = has_encode_batch(k, n);
  for (uint32_t i = 0; shape && i < n; ++i) shape = replicas[i] == i;
  // (2^40: the groups of one object and 256 q stay far inside 32 and 64 bits)
  constexpr uint64_t kMaxFastSize = 1ull << 40;
  for (uint32_t o = 0; o < count; ++o) {
    const uint64_t size = sizes[o];
    if (size && !ins[o]) return VDS_EC_EINVAL;
    if ((flags & VDS_EC_F_NO_TRAILER) && size % B) return VDS_EC_EINVAL;
    uint8_t *const *po = outs + (uint64_t)o * n;
    uintptr_t bits = 0;
    for (uint32_t i = 0; i < n; ++i) {
      if (!po[i]) return VDS_EC_EINVAL;
      bits |= reinterpret_cast<uintptr_t>(po[i]);
    }
    if (!shape || size == 0 || size > kMaxFastSize || (reinterpret_cast<uintptr_t>(ins[o]) & 3) || (bits & 1)) {
      sc.rest.push_back(o);
      continue;
    }
    EncBatchObj d{};
    d.in = ins[o];
    d.size = size;
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(po[0]);
    const uint64_t pitch = reinterpret_cast<uintptr_t>(po[1]) - p0;  // (n >= 20; may wrap: checked below)
    bool spaced = pitch != kEncBatchPtrTable;
    for (uint32_t i = 2; spaced && i < n; ++i) spaced = reinterpret_cast<uintptr_t>(po[i]) == p0 + i * pitch;
    if (spaced) {
      d.out = p0;
      d.pitch = pitch;
    } else {
      d.out = sc.ptrs.size() * sizeof(uint8_t *);  // offset for now: the table's address is known with the slot
      d.pitch = kEncBatchPtrTable;
      sc.ptrs.insert(sc.ptrs.end(), po, po + n);
    }
    sc.objs.push_back(d);
    const uint64_t T = (size + B - 1) / B;
    sc.groups += (T + 127) / 128;
  }
  if ((sc.groups + 15) / 16 > 0xFFFFFFFFull) {  // more tiles than the kernel counts: every object on its own
    sc.objs.clear();
    sc.ptrs.clear();
    sc.groups = 0;
    sc.rest.resize(count);
    for (uint32_t o = 0; o < count; ++o) sc.rest[o] = o;
  }
  return VDS_EC_OK;
}

namespace {

// The tables in one ring slot: descriptors (the batch's empty object last),
// pointer tables, tiles.  Tiles are filled in stripe order, object after
// object, and the kernel walks them with tile_range as the uniform kernel
// does; nothing is reordered.
int launch_planned(uint32_t k, uint32_t n, unsigned flags, const EncBatchScratch &sc, hipStream_t s) {
  const size_t ne = sc.objs.size();
  const uint64_t ntiles = (sc.groups + 15) / 16;
  const size_t o_ptrs = (ne + 1) * sizeof(EncBatchObj);
  const size_t o_tiles = (o_ptrs + sc.ptrs.size() * sizeof(uint8_t *) + 127) & ~size_t(127);
  const size_t bytes = o_tiles + ntiles * sizeof(EncBatchTile);
  ParamSlot *slot = nullptr;
  hipError_t e = param_acquire_n(1, &bytes, &slot);
  if (e != hipSuccess) return hip_status(e);
  EncBatchObj *objs = reinterpret_cast<EncBatchObj *>(slot->h);
  EncBatchTile *tiles = reinterpret_cast<EncBatchTile *>(slot->h + o_tiles);
  const uint64_t B = 2ull * k;
  uint64_t g = 0;
  for (size_t i = 0; i < ne; ++i) {
    EncBatchObj d = sc.objs[i];
    if (d.pitch == kEncBatchPtrTable) d.out += reinterpret_cast<uintptr_t>(slot->d + o_ptrs);
    objs[i] = d;
    const uint32_t ng = (uint32_t)(((d.size + B - 1) / B + 127) / 128);
    for (uint32_t q = 0; q < ng; ++q, ++g) {
      EncBatchTile &t = tiles[g >> 4];
      t.obj[g & 15] = (uint32_t)i;
      t.q[g & 15] = q;
    }
  }
  objs[ne] = EncBatchObj{};  // the empty object
  for (; g & 15; ++g) {
    EncBatchTile &t = tiles[g >> 4];
    t.obj[g & 15] = (uint32_t)ne;
    t.q[g & 15] = 0;
  }
  if (!sc.ptrs.empty()) std::memcpy(slot->h + o_ptrs, sc.ptrs.data(), sc.ptrs.size() * sizeof(uint8_t *));
  e = param_commit(slot, bytes, s);
  if (e == hipSuccess) {
    EncBatchLaunch b{};
    b.objs = reinterpret_cast<const EncBatchObj *>(slot->d);
    b.tiles = reinterpret_cast<const EncBatchTile *>(slot->d + o_tiles);
    b.total_tiles = (uint32_t)ntiles;
    b.trailer = (flags & VDS_EC_F_NO_TRAILER) ? 0u : 1u;
    e = launch_encode_batch(k, n, b, s);
  }
  const hipError_t re = param_release(slot, s);  // (its event follows whatever was enqueued)
  return hip_status(e != hipSuccess ? e : re);
}

}  // namespace

int encode_batch_run(uint32_t k, const uint16_t *replicas, uint32_t n, uint32_t count, const uint8_t *const *ins,
                     const uint64_t *sizes, uint8_t *const *outs, unsigned flags, const EncBatchScratch &sc,
                     hipStream_t s) {
  int rc;
  if (n == 0 || count == 0) return VDS_EC_OK;
  if (!sc.objs.empty() && (rc = launch_planned(k, n, flags, sc, s))) return rc;
  for (const uint32_t o : sc.rest) {
    rc = encode_device(2, k, replicas, n, ins[o], sizes[o], 0, 1, outs + (uint64_t)o * n, 0, flags, s);
    if (rc) return rc;
  }
  return VDS_EC_OK;
}

int encode_batch_device(uint32_t k, const uint16_t *replicas, uint32_t n, uint32_t count, const uint8_t *const *ins,
                        const uint64_t *sizes, uint8_t *const *outs, unsigned flags, hipStream_t s) {
  EncBatchScratch &sc = enc_batch_scratch();
  int rc = plan_encode_batch(k, replicas, n, count, ins, sizes, outs, flags, sc);
  if (rc) return rc;
  if ((rc = device_ready())) return rc;
  return encode_batch_run(k, replicas, n, count, ins, sizes, outs, flags, sc, s);
}

int encode_batch_path(uint32_t k, const uint16_t *replicas, uint32_t n, uint32_t count, const uint8_t *const *ins,
                      const uint64_t *sizes, uint8_t *const *outs, unsigned flags, uint32_t *fast_objects) {
  EncBatchScratch &sc = enc_batch_scratch();
  const int rc = plan_encode_batch(k, replicas, n, count, ins, sizes, outs, flags, sc);
  const uint32_t fast = rc ? 0u : (uint32_t)sc.objs.size();
  if (fast_objects) *fast_objects = fast;
  return fast ? 2 : 1;
}

}  // namespace api
}  // namespace vds_ec

extern "C" {

int vds_ec_encode16_batch_device(uint16_t k, const uint16_t *replicas, uint32_t n, uint32_t count,
                                 const uint8_t *const *ins, const uint64_t *sizes, uint8_t *const *outs,
                                 unsigned flags, void *stream) {
  return vds_ec::api::encode_batch_device(k, replicas, n, count, ins, sizes, outs, flags,
                                          vds_ec::api::as_stream(stream));
}

int vds_ec_encode16_batch_path(uint16_t k, const uint16_t *replicas, uint32_t n, uint32_t count,
                               const uint8_t *const *ins, const uint64_t *sizes, uint8_t *const *outs,
                               unsigned flags, uint32_t *fast_objects) {
  return vds_ec::api::encode_batch_path(k, replicas, n, count, ins, sizes, outs, flags, fast_objects);
}

}  // extern "C"
