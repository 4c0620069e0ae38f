// api_block_batch.cpp -- file blocks packed and unpacked on the device:
// batched AES-256-CBC (vds_ec_aes256_cbc_encrypt_batch_device /
// _decrypt_batch_device: aes.hip's two launches, planned on the host), the
// reference's client::save for a batch of blocks as four launches
// (vds_ec_block_pack_batch_device: id = SHA-256(data), key =
// SHA-256(AES(id, data)), crypted = AES(key, deflate(data));
// dht_network_client.cpp:1107-1140, vds_ws.js:151-161), client::restore the
// same way as three (vds_ec_block_unpack_batch_device: decrypt, inflate --
// inflate.hip through api_inflate_batch.cpp -- and the gated name check;
// dht_network_client.cpp:1297-1316), and the host forms through pinned staging
// (vds_ec_block_pack_host_batch, vds_ec_aes256_cbc_decrypt_host_batch,
// vds_ec_block_unpack_host_batch).  The pack with the deflate on the device
// too is five launches (vds_ec_block_pack_deflate_batch_device: hash, encrypt,
// hash, deflate -- deflate.hip through api_deflate_batch.cpp -- and the encrypt
// gated by the deflated lengths; vds_ec_aes256_cbc_encrypt_gated_batch_device
// is that last launch on its own).
// (api_internal.hpp lists the host runtime's translation units.)
#include "api_internal.hpp"

namespace vds_ec {
namespace api {

namespace {

inline uint64_t padded_size(uint64_t len) { return (len / 16 + 1) * 16; }

// [a, a + la) and [b, b + lb) share a byte
inline bool overlap(const void *a, uint64_t la, const void *b, uint64_t lb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return la && lb && x < y + lb && y < x + la;
}

// The arguments of one cipher launch, checked before the device is looked for.
// out_span(len): the bytes the launch may write at outs[o].
template <typename Span>
int check_cipher_args(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, const uint8_t *keys,
                      uint8_t *const *outs, Span out_span) {
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  if (!ins || !lens || !keys || !outs || (reinterpret_cast<uintptr_t>(keys) & 3u)) return VDS_EC_EINVAL;
  for (uint32_t o = 0; o < count; ++o) {
    if (lens[o] > 0xFFFFFFFFull || (lens[o] && !ins[o])) return VDS_EC_EINVAL;
    const uint64_t w = out_span(lens[o]);
    if ((w && !outs[o]) || overlap(ins[o], lens[o], outs[o], w)) return VDS_EC_EINVAL;
  }
  return VDS_EC_OK;
}

struct AesScratch {
  std::vector<uint32_t> key, order, bucket;
};
AesScratch &aes_scratch() {
  thread_local AesScratch sc;
  return sc;
}

// One quad walks one chain, so the chains go longest first (by blocks, the
// padding block included): a wave holds 16 chains of one length or nearly, and
// the long ones start at once.  Equal keys keep the caller's order.  A
// counting sort where the block counts are small against the batch (16,384
// bodies of up to 4097 blocks), else a comparison sort.  Then the table in one
// ring slot and the launch.  (Validated; the device is ready.)
// dev_lens: the gated form (launch_aes_encrypt_gated_batch) -- lens are then the upper bounds.
int enqueue_encrypt(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, const uint8_t *keys,
                    const uint8_t *ivs, uint8_t *const *outs, hipStream_t s, const uint32_t *dev_lens = nullptr,
                    uint32_t *dev_out_lens = nullptr) {
  AesScratch &sc = aes_scratch();
  sc.key.resize(count);
  sc.order.resize(count);
  uint32_t kmax = 0;
  for (uint32_t o = 0; o < count; ++o) {
    sc.key[o] = (uint32_t)(lens[o] / 16 + 1);
    kmax = std::max(kmax, sc.key[o]);
  }
  if (kmax <= 4ull * count + 4096) {
    sc.bucket.assign((size_t)kmax + 2, 0);
    for (uint32_t o = 0; o < count; ++o) ++sc.bucket[kmax - sc.key[o] + 1];
    for (size_t b = 1; b < sc.bucket.size(); ++b) sc.bucket[b] += sc.bucket[b - 1];
    for (uint32_t o = 0; o < count; ++o) sc.order[sc.bucket[kmax - sc.key[o]]++] = o;
  } else {
    for (uint32_t o = 0; o < count; ++o) sc.order[o] = o;
    std::stable_sort(sc.order.begin(), sc.order.end(), [&](uint32_t a, uint32_t b) { return sc.key[a] > sc.key[b]; });
  }
  const size_t bytes = (size_t)count * sizeof(AesEncMsg);
  ParamSlot *slot = nullptr;
  hipError_t e = param_acquire_n(1, &bytes, &slot);
  if (e != hipSuccess) return hip_status(e);
  AesEncMsg *t = reinterpret_cast<AesEncMsg *>(slot->h);
  for (uint32_t j = 0; j < count; ++j) {
    const uint32_t o = sc.order[j];
    t[j] = AesEncMsg{reinterpret_cast<uintptr_t>(ins[o]), reinterpret_cast<uintptr_t>(outs[o]), (uint32_t)lens[o], o};
  }
  e = param_commit(slot, bytes, s);
  if (e == hipSuccess && dev_lens) {
    e = launch_aes_encrypt_gated_batch(reinterpret_cast<const AesEncMsg *>(slot->d), count, keys, ivs, dev_lens,
                                       dev_out_lens, s);
  } else if (e == hipSuccess) {
    // (read per call: VDS_EC_AES_ENC=lane runs the one-lane-a-chain kernel, the A/B arm of DESIGN 3.8b)
    const char *arm = std::getenv("VDS_EC_AES_ENC");
    e = launch_aes_encrypt_batch(reinterpret_cast<const AesEncMsg *>(slot->d), count, keys, ivs, s,
                                 arm && std::strcmp(arm, "lane") == 0);
  }
  const hipError_t re = param_release(slot, s);  // (its event follows whatever was enqueued)
  return hip_status(e != hipSuccess ? e : re);
}

// The tiles of a decrypt launch: a message of len bytes has one a kAesDecTile
// bytes, and at least one (which writes its status).
inline uint64_t dec_tiles(uint64_t len) {
  if (len == 0 || len % 16) return 1;
  return (len + kAesDecTile - 1) / kAesDecTile;
}

int enqueue_decrypt(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, const uint8_t *keys,
                    const uint8_t *ivs, uint8_t *const *outs, uint32_t *out_lens, int32_t *statuses, uint64_t ntiles,
                    hipStream_t s) {
  // the messages, then a tile table over all of them, in one ring slot
  const size_t o_tiles = ((size_t)count * sizeof(AesDecMsg) + 15) & ~size_t(15);
  const size_t bytes = o_tiles + ntiles * sizeof(AesDecTile);
  ParamSlot *slot = nullptr;
  hipError_t e = param_acquire_n(1, &bytes, &slot);
  if (e != hipSuccess) return hip_status(e);
  AesDecMsg *msgs = reinterpret_cast<AesDecMsg *>(slot->h);
  AesDecTile *tiles = reinterpret_cast<AesDecTile *>(slot->h + o_tiles);
  size_t t = 0;
  for (uint32_t o = 0; o < count; ++o) {
    msgs[o] = AesDecMsg{reinterpret_cast<uintptr_t>(ins[o]), reinterpret_cast<uintptr_t>(outs[o]), (uint32_t)lens[o], 0};
    const uint32_t nt = (uint32_t)dec_tiles(lens[o]);
    for (uint32_t i = 0; i < nt; ++i) tiles[t++] = AesDecTile{o, i};
  }
  e = param_commit(slot, bytes, s);
  if (e == hipSuccess) {
    AesDecLaunch l{};
    l.msgs = reinterpret_cast<const AesDecMsg *>(slot->d);
    l.tiles = reinterpret_cast<const AesDecTile *>(slot->d + o_tiles);
    l.ntiles = (uint32_t)ntiles;
    l.keys = reinterpret_cast<uintptr_t>(keys);
    l.ivs = reinterpret_cast<uintptr_t>(ivs);
    l.out_lens = reinterpret_cast<uintptr_t>(out_lens);
    l.statuses = reinterpret_cast<uintptr_t>(statuses);
    e = launch_aes_decrypt_batch(l, s);
  }
  const hipError_t re = param_release(slot, s);
  return hip_status(e != hipSuccess ? e : re);
}

int check_decrypt_args(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, const uint8_t *keys,
                       uint8_t *const *outs, const void *out_lens, const void *statuses, uint64_t *ntiles) {
  int rc = check_cipher_args(count, ins, lens, keys, outs, [](uint64_t len) { return len; });
  if (rc) return rc;
  *ntiles = 0;
  if (count == 0) return VDS_EC_OK;
  if (!out_lens || !statuses || ((reinterpret_cast<uintptr_t>(out_lens) | reinterpret_cast<uintptr_t>(statuses)) & 3u))
    return VDS_EC_EINVAL;
  for (uint32_t o = 0; o < count; ++o) *ntiles += dec_tiles(lens[o]);
  return *ntiles > 0x7FFFFFFFull ? VDS_EC_EINVAL : VDS_EC_OK;  // (the launch's workgroups)
}

// The pack's intermediate ciphertext (AES(id, data), hashed into the key and
// dropped): one buffer a device for the process, grown to a power of two and
// kept.  A call holds the lock while it enqueues; the event recorded behind
// its last reader orders the next call's first writer after it on whatever
// stream that one runs, so nothing synchronises unless the buffer grows.
// Never freed, as the other contexts.
struct PackScratch {
  std::mutex mu;
  uint8_t *d = nullptr;
  size_t cap = 0;
  hipEvent_t done = nullptr;
  bool pending = false;
};
PackScratch *pack_scratch() {
  static std::mutex m;
  static std::vector<PackScratch *> per_dev;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return nullptr;
  std::lock_guard<std::mutex> g(m);
  if ((size_t)dev >= per_dev.size()) per_dev.resize(dev + 1, nullptr);
  if (!per_dev[dev]) per_dev[dev] = new PackScratch();
  return per_dev[dev];
}

int check_pack_args(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens,
                    const uint8_t *const *zipped, const uint64_t *zipped_lens, const uint8_t *ids,
                    const uint8_t *keys, uint8_t *const *crypted, bool device) {
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  if (!datas || !data_lens || !zipped || !zipped_lens || !ids || !keys || !crypted) return VDS_EC_EINVAL;
  if (device && ((reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(keys)) & 3u)) return VDS_EC_EINVAL;
  for (uint32_t o = 0; o < count; ++o) {
    if (data_lens[o] > 0xFFFFFFFFull || zipped_lens[o] > 0xFFFFFFFFull) return VDS_EC_EINVAL;
    if ((data_lens[o] && !datas[o]) || (zipped_lens[o] && !zipped[o]) || !crypted[o]) return VDS_EC_EINVAL;
    const uint64_t w = padded_size(zipped_lens[o]);
    if (overlap(datas[o], data_lens[o], crypted[o], w) || overlap(zipped[o], zipped_lens[o], crypted[o], w))
      return VDS_EC_EINVAL;
  }
  return VDS_EC_OK;
}

struct PackTables {
  std::vector<uint8_t *> tmp;
  std::vector<uint64_t> tmp_len;
};
PackTables &pack_tables() {
  thread_local PackTables t;
  return t;
}

// (validated; the device is ready)
int enqueue_pack(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens, const uint8_t *const *zipped,
                 const uint64_t *zipped_lens, uint8_t *ids, uint8_t *keys, uint8_t *const *crypted, hipStream_t s) {
  PackScratch *ps = pack_scratch();
  if (!ps) return VDS_EC_ENODEV;
  uint64_t need = 0;
  for (uint32_t o = 0; o < count; ++o) need += padded_size(data_lens[o]);
  std::lock_guard<std::mutex> g(ps->mu);
  if (!ps->done && hipEventCreateWithFlags(&ps->done, hipEventDisableTiming) != hipSuccess) return VDS_EC_ENODEV;
  if (need > ps->cap) {
    if (ps->pending) (void)hipEventSynchronize(ps->done);
    ps->pending = false;
    if (ps->d) (void)hipFree(ps->d);
    ps->d = nullptr;
    ps->cap = 0;
    size_t cap = 1u << 20;
    while (cap < need) cap *= 2;
    if (hipMalloc(&ps->d, cap) != hipSuccess) return VDS_EC_ENOMEM;
    ps->cap = cap;
  }
  if (ps->pending) {
    const hipError_t e = hipStreamWaitEvent(s, ps->done, 0);
    if (e != hipSuccess) return hip_status(e);
  }
  PackTables &t = pack_tables();
  t.tmp.resize(count);
  t.tmp_len.resize(count);
  uint64_t at = 0;
  for (uint32_t o = 0; o < count; ++o) {
    t.tmp[o] = ps->d + at;
    t.tmp_len[o] = padded_size(data_lens[o]);
    at += t.tmp_len[o];
  }
  int rc = sha256_batch_device(count, datas, data_lens, ids, s);
  if (!rc) rc = enqueue_encrypt(count, datas, data_lens, ids, nullptr, t.tmp.data(), s);
  if (!rc) rc = sha256_batch_device(count, t.tmp.data(), t.tmp_len.data(), keys, s);
  // (the scratch's last reader, also when a step failed behind an earlier one's launch)
  ps->pending = hipEventRecord(ps->done, s) == hipSuccess;
  if (!ps->pending) (void)hipStreamSynchronize(s);
  if (!rc) rc = enqueue_encrypt(count, zipped, zipped_lens, keys, nullptr, crypted, s);
  return rc;
}

int check_pack_deflate_args(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens, const uint8_t *ids,
                            const uint8_t *keys, uint8_t *const *crypted, const uint64_t *crypted_caps, bool device) {
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  if (!datas || !data_lens || !ids || !keys || !crypted || !crypted_caps) return VDS_EC_EINVAL;
  if (device && ((reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(keys)) & 3u)) return VDS_EC_EINVAL;
  for (uint32_t o = 0; o < count; ++o) {
    if (data_lens[o] > 0xFFFFFFFFull || (data_lens[o] && !datas[o]) || !crypted[o]) return VDS_EC_EINVAL;
    const uint64_t w = padded_size(vds_ec_deflate_bound(data_lens[o]));
    if (w > 0xFFFFFFFFull || crypted_caps[o] < w) return VDS_EC_EINVAL;
    if (overlap(datas[o], data_lens[o], crypted[o], crypted_caps[o])) return VDS_EC_EINVAL;
  }
  return VDS_EC_OK;
}

// client::save with the deflate on the device.  Block o has one slot of the
// pack's scratch, max(padded_size(len), the deflate's bound) bytes rounded up
// to 16: first AES(id, data), which the key's hash reads and nobody after it,
// then -- behind that hash in stream order -- the deflated bytes, which the
// last encrypt reads; the deflated lengths (a uint32_t a block) follow the
// slots.  So the scratch is about one byte an input byte.  Its last reader is
// the last launch.  (Validated; the device is ready.)
int enqueue_pack_deflate(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens, uint8_t *ids,
                         uint8_t *keys, uint8_t *const *crypted, uint32_t *crypted_lens, hipStream_t s) {
  PackScratch *ps = pack_scratch();
  if (!ps) return VDS_EC_ENODEV;
  auto slot_size = [](uint64_t len) {
    return (std::max<uint64_t>(padded_size(len), vds_ec_deflate_bound(len)) + 15) & ~15ull;
  };
  uint64_t slots_b = 0;
  for (uint32_t o = 0; o < count; ++o) slots_b += slot_size(data_lens[o]);
  const uint64_t need = slots_b + 4ull * count;
  std::lock_guard<std::mutex> g(ps->mu);
  if (!ps->done && hipEventCreateWithFlags(&ps->done, hipEventDisableTiming) != hipSuccess) return VDS_EC_ENODEV;
  if (need > ps->cap) {
    if (ps->pending) (void)hipEventSynchronize(ps->done);
    ps->pending = false;
    if (ps->d) (void)hipFree(ps->d);
    ps->d = nullptr;
    ps->cap = 0;
    size_t cap = 1u << 20;
    while (cap < need) cap *= 2;
    if (hipMalloc(&ps->d, cap) != hipSuccess) return VDS_EC_ENOMEM;
    ps->cap = cap;
  }
  if (ps->pending) {
    const hipError_t e = hipStreamWaitEvent(s, ps->done, 0);
    if (e != hipSuccess) return hip_status(e);
  }
  PackTables &t = pack_tables();
  t.tmp.resize(count);
  t.tmp_len.resize(count);
  thread_local std::vector<uint64_t> zip_caps;
  zip_caps.resize(count);
  uint64_t at = 0;
  for (uint32_t o = 0; o < count; ++o) {
    t.tmp[o] = ps->d + at;
    t.tmp_len[o] = padded_size(data_lens[o]);
    zip_caps[o] = vds_ec_deflate_bound(data_lens[o]);
    at += slot_size(data_lens[o]);
  }
  uint32_t *zip_lens = reinterpret_cast<uint32_t *>(ps->d + slots_b);
  int rc = sha256_batch_device(count, datas, data_lens, ids, s);
  if (!rc) rc = enqueue_encrypt(count, datas, data_lens, ids, nullptr, t.tmp.data(), s);
  if (!rc) rc = sha256_batch_device(count, t.tmp.data(), t.tmp_len.data(), keys, s);
  if (!rc) rc = enqueue_deflate(count, datas, data_lens, t.tmp.data(), zip_caps.data(), zip_lens, s);
  if (!rc) rc = enqueue_encrypt(count, t.tmp.data(), zip_caps.data(), keys, nullptr, crypted, s, zip_lens, crypted_lens);
  // (the scratch's last reader, also when a step failed behind an earlier one's launch)
  ps->pending = hipEventRecord(ps->done, s) == hipSuccess;
  if (!ps->pending) (void)hipStreamSynchronize(s);
  return rc;
}

int check_unpack_args(uint32_t count, const uint8_t *const *crypted, const uint64_t *crypted_lens,
                      const uint8_t *keys, const uint8_t *ids, uint8_t *const *outs, const uint64_t *out_caps,
                      const void *out_lens, const void *statuses, bool device, uint64_t *ntiles) {
  int rc = check_inflate_args(count, crypted, crypted_lens, outs, out_caps);
  if (rc) return rc;
  *ntiles = 0;
  if (count == 0) return VDS_EC_OK;
  if (!keys || !ids || !out_lens || !statuses) return VDS_EC_EINVAL;
  if (device && ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(out_lens) |
                  reinterpret_cast<uintptr_t>(statuses)) & 3u))
    return VDS_EC_EINVAL;
  for (uint32_t o = 0; o < count; ++o) *ntiles += dec_tiles(crypted_lens[o]);
  return *ntiles > 0x7FFFFFFFull ? VDS_EC_EINVAL : VDS_EC_OK;  // (the decrypt launch's workgroups)
}

// client::restore for a batch: decrypt into the pack's scratch (the
// plaintexts at 16-byte aligned offsets, then a length and a status a block),
// inflate from there under those lengths and statuses, name check under the
// inflate's.  The scratch's last reader is the inflate.  (Validated; the
// device is ready.)
int enqueue_unpack(uint32_t count, const uint8_t *const *crypted, const uint64_t *crypted_lens, const uint8_t *keys,
                   const uint8_t *ids, uint8_t *const *outs, const uint64_t *out_caps, uint32_t *out_lens,
                   int32_t *statuses, uint64_t ntiles, hipStream_t s) {
  PackScratch *ps = pack_scratch();
  if (!ps) return VDS_EC_ENODEV;
  uint64_t plain_b = 0;
  for (uint32_t o = 0; o < count; ++o) plain_b += (crypted_lens[o] + 15) & ~15ull;
  const uint64_t need = plain_b + 8ull * count;
  std::lock_guard<std::mutex> g(ps->mu);
  if (!ps->done && hipEventCreateWithFlags(&ps->done, hipEventDisableTiming) != hipSuccess) return VDS_EC_ENODEV;
  if (need > ps->cap) {
    if (ps->pending) (void)hipEventSynchronize(ps->done);
    ps->pending = false;
    if (ps->d) (void)hipFree(ps->d);
    ps->d = nullptr;
    ps->cap = 0;
    size_t cap = 1u << 20;
    while (cap < need) cap *= 2;
    if (hipMalloc(&ps->d, cap) != hipSuccess) return VDS_EC_ENOMEM;
    ps->cap = cap;
  }
  if (ps->pending) {
    const hipError_t e = hipStreamWaitEvent(s, ps->done, 0);
    if (e != hipSuccess) return hip_status(e);
  }
  PackTables &t = pack_tables();
  t.tmp.resize(count);
  uint64_t at = 0;
  for (uint32_t o = 0; o < count; ++o) {
    t.tmp[o] = ps->d + at;
    at += (crypted_lens[o] + 15) & ~15ull;
  }
  uint32_t *plain_lens = reinterpret_cast<uint32_t *>(ps->d + plain_b);
  int32_t *plain_st = reinterpret_cast<int32_t *>(ps->d + plain_b + 4ull * count);
  int rc = enqueue_decrypt(count, crypted, crypted_lens, keys, nullptr, t.tmp.data(), plain_lens, plain_st, ntiles, s);
  if (!rc)
    rc = enqueue_inflate(count, t.tmp.data(), crypted_lens, outs, out_caps, out_lens, statuses, plain_lens, plain_st, s);
  // (the scratch's last reader, also when a step failed behind an earlier one's launch)
  ps->pending = hipEventRecord(ps->done, s) == hipSuccess;
  if (!ps->pending) (void)hipStreamSynchronize(s);
  if (!rc) rc = sha256_gated_batch_device(count, outs, out_caps, ids, out_lens, statuses, s);
  return rc;
}

}  // namespace

int block_unpack_batch_device(uint32_t count, const uint8_t *const *crypted, const uint64_t *crypted_lens,
                              const uint8_t *keys, const uint8_t *ids, uint8_t *const *outs, const uint64_t *out_caps,
                              uint32_t *out_lens, int32_t *statuses, hipStream_t s) {
  uint64_t ntiles = 0;
  int rc = check_unpack_args(count, crypted, crypted_lens, keys, ids, outs, out_caps, out_lens, statuses, true, &ntiles);
  if (rc || count == 0) return rc;
  if ((rc = device_ready())) return rc;
  return enqueue_unpack(count, crypted, crypted_lens, keys, ids, outs, out_caps, out_lens, statuses, ntiles, s);
}

int block_unpack_host_batch(uint32_t count, const uint8_t *const *crypted, const uint64_t *crypted_lens,
                            const uint8_t *keys, const uint8_t *ids, uint8_t *const *outs, const uint64_t *out_caps,
                            uint64_t *out_lens, int32_t *statuses, uint32_t *failed) {
  uint64_t all_tiles = 0;
  int rc = check_unpack_args(count, crypted, crypted_lens, keys, ids, outs, out_caps, out_lens, statuses, false,
                             &all_tiles);
  if (rc) return rc;
  if (failed) *failed = 0;
  if (count == 0) return VDS_EC_OK;
  if ((rc = device_ready())) return rc;
  SaveTempStage *st = save_temp_stage();
  if (!st) return VDS_EC_ENODEV;
  std::vector<uint64_t> c_off, o_off;
  std::vector<const uint8_t *> d_crypted;
  std::vector<uint8_t *> d_outs;
  std::vector<Copy> parts;
  uint32_t bad = 0;
  for (uint32_t o0 = 0; o0 < count;) {
    // The group: blocks o0 .. o1-1, at most 64 MiB each way.  Ciphertexts at
    // 16-byte aligned offsets of the input staging, then the keys and the ids;
    // in the output staging the outputs' capacities at 16-byte aligned
    // offsets, then the lengths and the statuses.
    c_off.clear();
    o_off.clear();
    uint64_t ct_b = 0, out_b = 0, ntiles = 0;
    uint32_t o1 = o0;
    while (o1 < count && o1 - o0 < kSaveTempGroupObjects) {
      const uint64_t ca = (ct_b + 15) & ~15ull, oa = (out_b + 15) & ~15ull;
      if (o1 > o0 && (ca + crypted_lens[o1] > kSaveTempGroupBytes || oa + out_caps[o1] > kSaveTempGroupBytes)) break;
      c_off.push_back(ca);
      o_off.push_back(oa);
      ct_b = ca + crypted_lens[o1];
      out_b = oa + out_caps[o1];
      ntiles += dec_tiles(crypted_lens[o1]);
      ++o1;
    }
    const uint32_t cnt = o1 - o0;
    const uint64_t key_off = (ct_b + 15) & ~15ull, id_off = key_off + 32ull * cnt, in_b = id_off + 32ull * cnt;
    const uint64_t len_off = (out_b + 15) & ~15ull, st_off = len_off + 4ull * cnt, back_b = st_off + 4ull * cnt;
    if ((rc = st->reserve(in_b, back_b))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j) parts.push_back({st->h_in + c_off[j], crypted[o0 + j], crypted_lens[o0 + j]});
    parts.push_back({st->h_in + key_off, keys + 32ull * o0, 32ull * cnt});
    parts.push_back({st->h_in + id_off, ids + 32ull * o0, 32ull * cnt});
    parallel_copy(parts);
    hipError_t e = hipMemcpyAsync(st->d_in, st->h_in, in_b, hipMemcpyHostToDevice, st->stream);
    if (e != hipSuccess) return hip_status(e);
    auto drained = [&](int r) {
      (void)hipStreamSynchronize(st->stream);
      return r;
    };
    d_crypted.resize(cnt);
    d_outs.resize(cnt);
    for (uint32_t j = 0; j < cnt; ++j) {
      d_crypted[j] = st->d_in + c_off[j];
      d_outs[j] = st->d_out + o_off[j];
    }
    rc = enqueue_unpack(cnt, d_crypted.data(), crypted_lens + o0, st->d_in + key_off, st->d_in + id_off, d_outs.data(),
                        out_caps + o0, reinterpret_cast<uint32_t *>(st->d_out + len_off),
                        reinterpret_cast<int32_t *>(st->d_out + st_off), ntiles, st->stream);
    if (rc) return drained(rc);
    // lengths and statuses first: only what was unpacked comes back
    e = hipMemcpyAsync(st->h_out + len_off, st->d_out + len_off, back_b - len_off, hipMemcpyDeviceToHost, st->stream);
    if (e != hipSuccess) return drained(hip_status(e));
    if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    const uint32_t *dl = reinterpret_cast<const uint32_t *>(st->h_out + len_off);
    const int32_t *ds = reinterpret_cast<const int32_t *>(st->h_out + st_off);
    uint64_t hi = 0;
    for (uint32_t j = 0; j < cnt; ++j)
      if (ds[j] == VDS_EC_OK) hi = std::max<uint64_t>(hi, o_off[j] + dl[j]);
    if (hi) {
      e = hipMemcpyAsync(st->h_out, st->d_out, hi, hipMemcpyDeviceToHost, st->stream);
      if (e != hipSuccess) return drained(hip_status(e));
      if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    }
    // a block whose status is non-zero has nothing scattered
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t o = o0 + j;
      statuses[o] = ds[j];
      out_lens[o] = ds[j] ? 0 : dl[j];
      if (ds[j]) {
        ++bad;
        continue;
      }
      parts.push_back({outs[o], st->h_out + o_off[j], dl[j]});
    }
    parallel_copy(parts);
    o0 = o1;
  }
  if (failed) *failed = bad;
  return VDS_EC_OK;
}

int aes_encrypt_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, const uint8_t *keys,
                             const uint8_t *ivs, uint8_t *const *outs, hipStream_t s) {
  int rc = check_cipher_args(count, ins, lens, keys, outs, padded_size);
  if (rc || count == 0) return rc;
  if ((rc = device_ready())) return rc;
  return enqueue_encrypt(count, ins, lens, keys, ivs, outs, s);
}

int aes_decrypt_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, const uint8_t *keys,
                             const uint8_t *ivs, uint8_t *const *outs, uint32_t *out_lens, int32_t *statuses,
                             hipStream_t s) {
  uint64_t ntiles = 0;
  int rc = check_decrypt_args(count, ins, lens, keys, outs, out_lens, statuses, &ntiles);
  if (rc || count == 0) return rc;
  if ((rc = device_ready())) return rc;
  return enqueue_decrypt(count, ins, lens, keys, ivs, outs, out_lens, statuses, ntiles, s);
}

int block_pack_batch_device(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens,
                            const uint8_t *const *zipped, const uint64_t *zipped_lens, uint8_t *ids, uint8_t *keys,
                            uint8_t *const *crypted, hipStream_t s) {
  int rc = check_pack_args(count, datas, data_lens, zipped, zipped_lens, ids, keys, crypted, true);
  if (rc || count == 0) return rc;
  if ((rc = device_ready())) return rc;
  return enqueue_pack(count, datas, data_lens, zipped, zipped_lens, ids, keys, crypted, s);
}

int block_pack_host_batch(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens,
                          const uint8_t *const *zipped, const uint64_t *zipped_lens, uint8_t *ids, uint8_t *keys,
                          uint8_t *const *crypted, uint64_t *crypted_sizes) {
  int rc = check_pack_args(count, datas, data_lens, zipped, zipped_lens, ids, keys, crypted, false);
  if (rc || count == 0) return rc;
  if ((rc = device_ready())) return rc;
  SaveTempStage *st = save_temp_stage();
  if (!st) return VDS_EC_ENODEV;
  std::vector<uint64_t> d_off, z_off, c_off;
  std::vector<const uint8_t *> d_datas, d_zipped;
  std::vector<uint8_t *> d_crypted;
  std::vector<Copy> parts;
  for (uint32_t o0 = 0; o0 < count;) {
    // The group: blocks o0 .. o1-1.  Data and deflated bytes at 16-byte
    // aligned offsets of the input staging; in the output staging the bodies
    // (whole cipher blocks, so 16-byte aligned back to back), the ids, the keys.
    d_off.clear();
    z_off.clear();
    c_off.clear();
    uint64_t in_b = 0, out_b = 0;
    uint32_t o1 = o0;
    while (o1 < count && o1 - o0 < kSaveTempGroupObjects) {
      const uint64_t da = (in_b + 15) & ~15ull;
      const uint64_t za = (da + data_lens[o1] + 15) & ~15ull;
      if (o1 > o0 && za + zipped_lens[o1] > kSaveTempGroupBytes) break;
      d_off.push_back(da);
      z_off.push_back(za);
      in_b = za + zipped_lens[o1];
      c_off.push_back(out_b);
      out_b += padded_size(zipped_lens[o1]);
      ++o1;
    }
    const uint32_t cnt = o1 - o0;
    const uint64_t id_off = out_b, key_off = id_off + 32ull * cnt, back_b = key_off + 32ull * cnt;
    if ((rc = st->reserve(std::max<uint64_t>(in_b, 64), back_b))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j) {
      parts.push_back({st->h_in + d_off[j], datas[o0 + j], data_lens[o0 + j]});
      parts.push_back({st->h_in + z_off[j], zipped[o0 + j], zipped_lens[o0 + j]});
    }
    parallel_copy(parts);
    hipError_t e = in_b ? hipMemcpyAsync(st->d_in, st->h_in, in_b, hipMemcpyHostToDevice, st->stream) : hipSuccess;
    if (e != hipSuccess) return hip_status(e);
    // (an error after the first enqueue drains the stream before returning:
    // the next call on this thread reuses the buffers)
    auto drained = [&](int r) {
      (void)hipStreamSynchronize(st->stream);
      return r;
    };
    d_datas.resize(cnt);
    d_zipped.resize(cnt);
    d_crypted.resize(cnt);
    for (uint32_t j = 0; j < cnt; ++j) {
      d_datas[j] = st->d_in + d_off[j];
      d_zipped[j] = st->d_in + z_off[j];
      d_crypted[j] = st->d_out + c_off[j];
    }
    rc = enqueue_pack(cnt, d_datas.data(), data_lens + o0, d_zipped.data(), zipped_lens + o0, st->d_out + id_off,
                      st->d_out + key_off, d_crypted.data(), st->stream);
    if (rc) return drained(rc);
    e = hipMemcpyAsync(st->h_out, st->d_out, back_b, hipMemcpyDeviceToHost, st->stream);
    if (e != hipSuccess) return drained(hip_status(e));
    if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint64_t w = padded_size(zipped_lens[o0 + j]);
      parts.push_back({crypted[o0 + j], st->h_out + c_off[j], w});
      if (crypted_sizes) crypted_sizes[o0 + j] = w;
    }
    parts.push_back({ids + 32ull * o0, st->h_out + id_off, 32ull * cnt});
    parts.push_back({keys + 32ull * o0, st->h_out + key_off, 32ull * cnt});
    parallel_copy(parts);
    o0 = o1;
  }
  return VDS_EC_OK;
}

int aes_encrypt_gated_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *max_lens,
                                   const uint32_t *lens, const uint8_t *keys, const uint8_t *ivs, uint8_t *const *outs,
                                   uint32_t *out_lens, hipStream_t s) {
  int rc = check_cipher_args(count, ins, max_lens, keys, outs, padded_size);
  if (rc || count == 0) return rc;
  if (!lens || !out_lens || ((reinterpret_cast<uintptr_t>(lens) | reinterpret_cast<uintptr_t>(out_lens)) & 3u))
    return VDS_EC_EINVAL;
  if ((rc = device_ready())) return rc;
  return enqueue_encrypt(count, ins, max_lens, keys, ivs, outs, s, lens, out_lens);
}

int block_pack_deflate_batch_device(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens,
                                    uint8_t *ids, uint8_t *keys, uint8_t *const *crypted, const uint64_t *crypted_caps,
                                    uint32_t *crypted_lens, hipStream_t s) {
  int rc = check_pack_deflate_args(count, datas, data_lens, ids, keys, crypted, crypted_caps, true);
  if (rc || count == 0) return rc;
  if (!crypted_lens || (reinterpret_cast<uintptr_t>(crypted_lens) & 3u)) return VDS_EC_EINVAL;
  if ((rc = device_ready())) return rc;
  return enqueue_pack_deflate(count, datas, data_lens, ids, keys, crypted, crypted_lens, s);
}

int block_pack_deflate_host_batch(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens, uint8_t *ids,
                                  uint8_t *keys, uint8_t *const *crypted, const uint64_t *crypted_caps,
                                  uint64_t *crypted_sizes) {
  int rc = check_pack_deflate_args(count, datas, data_lens, ids, keys, crypted, crypted_caps, false);
  if (rc) return rc;
  if (count && !crypted_sizes) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  if ((rc = device_ready())) return rc;
  SaveTempStage *st = save_temp_stage();
  if (!st) return VDS_EC_ENODEV;
  std::vector<uint64_t> d_off, c_off;
  std::vector<const uint8_t *> d_datas;
  std::vector<uint8_t *> d_crypted;
  std::vector<Copy> parts;
  for (uint32_t o0 = 0; o0 < count;) {
    // The group: blocks o0 .. o1-1, at most 64 MiB each way.  Data at 16-byte
    // aligned offsets of the input staging; in the output staging the bodies'
    // capacities (whole cipher blocks: back to back), the ids, the keys, the
    // bodies' sizes.
    d_off.clear();
    c_off.clear();
    uint64_t in_b = 0, out_b = 0;
    uint32_t o1 = o0;
    while (o1 < count && o1 - o0 < kSaveTempGroupObjects) {
      const uint64_t da = (in_b + 15) & ~15ull, w = padded_size(vds_ec_deflate_bound(data_lens[o1]));
      if (o1 > o0 && (da + data_lens[o1] > kSaveTempGroupBytes || out_b + w > kSaveTempGroupBytes)) break;
      d_off.push_back(da);
      in_b = da + data_lens[o1];
      c_off.push_back(out_b);
      out_b += w;
      ++o1;
    }
    const uint32_t cnt = o1 - o0;
    const uint64_t id_off = out_b, key_off = id_off + 32ull * cnt, len_off = key_off + 32ull * cnt,
                   back_b = len_off + 4ull * cnt;
    if ((rc = st->reserve(std::max<uint64_t>(in_b, 64), back_b))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j) parts.push_back({st->h_in + d_off[j], datas[o0 + j], data_lens[o0 + j]});
    parallel_copy(parts);
    hipError_t e = in_b ? hipMemcpyAsync(st->d_in, st->h_in, in_b, hipMemcpyHostToDevice, st->stream) : hipSuccess;
    if (e != hipSuccess) return hip_status(e);
    auto drained = [&](int r) {
      (void)hipStreamSynchronize(st->stream);
      return r;
    };
    d_datas.resize(cnt);
    d_crypted.resize(cnt);
    for (uint32_t j = 0; j < cnt; ++j) {
      d_datas[j] = st->d_in + d_off[j];
      d_crypted[j] = st->d_out + c_off[j];
    }
    rc = enqueue_pack_deflate(cnt, d_datas.data(), data_lens + o0, st->d_out + id_off, st->d_out + key_off,
                              d_crypted.data(), reinterpret_cast<uint32_t *>(st->d_out + len_off), st->stream);
    if (rc) return drained(rc);
    // ids, keys and sizes first: only the bodies' own bytes come back
    e = hipMemcpyAsync(st->h_out + id_off, st->d_out + id_off, back_b - id_off, hipMemcpyDeviceToHost, st->stream);
    if (e != hipSuccess) return drained(hip_status(e));
    if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    const uint32_t *dl = reinterpret_cast<const uint32_t *>(st->h_out + len_off);
    uint64_t hi = 0;
    for (uint32_t j = 0; j < cnt; ++j) {
      if (dl[j] > crypted_caps[o0 + j]) return VDS_EC_EHIP;  // (cannot be: the stored form is the bound)
      hi = std::max<uint64_t>(hi, c_off[j] + dl[j]);
    }
    e = hipMemcpyAsync(st->h_out, st->d_out, hi, hipMemcpyDeviceToHost, st->stream);
    if (e != hipSuccess) return drained(hip_status(e));
    if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j) {
      parts.push_back({crypted[o0 + j], st->h_out + c_off[j], dl[j]});
      crypted_sizes[o0 + j] = dl[j];
    }
    parts.push_back({ids + 32ull * o0, st->h_out + id_off, 32ull * cnt});
    parts.push_back({keys + 32ull * o0, st->h_out + key_off, 32ull * cnt});
    parallel_copy(parts);
    o0 = o1;
  }
  return VDS_EC_OK;
}

int aes_decrypt_host_batch(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, const uint8_t *keys,
                           const uint8_t *ivs, uint8_t *const *outs, uint64_t *out_lens, int32_t *statuses,
                           uint32_t *failed) {
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count && (!ins || !lens || !keys || !outs || !out_lens || !statuses)) return VDS_EC_EINVAL;
  for (uint32_t o = 0; o < count; ++o) {
    if (lens[o] > 0xFFFFFFFFull || (lens[o] && (!ins[o] || !outs[o]))) return VDS_EC_EINVAL;
    if (overlap(ins[o], lens[o], outs[o], lens[o])) return VDS_EC_EINVAL;
  }
  if (failed) *failed = 0;
  if (count == 0) return VDS_EC_OK;
  int rc = device_ready();
  if (rc) return rc;
  SaveTempStage *st = save_temp_stage();
  if (!st) return VDS_EC_ENODEV;
  std::vector<uint32_t> idx;  // the group's messages (a length that is 0 or no multiple of 16 gets no device work)
  std::vector<uint64_t> off, glens;
  std::vector<const uint8_t *> d_ins;
  std::vector<uint8_t *> d_outs;
  std::vector<Copy> parts;
  uint32_t bad = 0;
  for (uint32_t o0 = 0; o0 < count;) {
    // The group: messages o0 .. o1-1.  Ciphertexts at 16-byte aligned offsets
    // of the input staging (whole blocks: back to back), then the keys and the
    // ivs; the plaintexts at the same offsets of the output staging, then the
    // lengths and the statuses.
    idx.clear();
    off.clear();
    glens.clear();
    uint64_t ct_b = 0;
    uint32_t o1 = o0;
    while (o1 < count && idx.size() < kSaveTempGroupObjects) {
      const uint64_t len = lens[o1];
      if (len == 0 || len % 16) {
        statuses[o1] = VDS_EC_ECRYPT_LENGTH;
        out_lens[o1++] = 0;
        ++bad;
        continue;
      }
      if (!idx.empty() && ct_b + len > kSaveTempGroupBytes) break;
      idx.push_back(o1);
      off.push_back(ct_b);
      glens.push_back(len);
      ct_b += len;
      ++o1;
    }
    const uint32_t cnt = (uint32_t)idx.size();
    if (cnt == 0) {
      o0 = o1;
      continue;
    }
    const uint64_t key_off = ct_b, iv_off = key_off + 32ull * cnt, in_b = iv_off + (ivs ? 16ull * cnt : 0);
    const uint64_t len_off = ct_b, st_off = len_off + 4ull * cnt, back_b = st_off + 4ull * cnt;
    if ((rc = st->reserve(in_b, back_b))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j) {
      parts.push_back({st->h_in + off[j], ins[idx[j]], glens[j]});
      parts.push_back({st->h_in + key_off + 32ull * j, keys + 32ull * idx[j], 32});
      if (ivs) parts.push_back({st->h_in + iv_off + 16ull * j, ivs + 16ull * idx[j], 16});
    }
    parallel_copy(parts);
    hipError_t e = hipMemcpyAsync(st->d_in, st->h_in, in_b, hipMemcpyHostToDevice, st->stream);
    if (e != hipSuccess) return hip_status(e);
    auto drained = [&](int r) {
      (void)hipStreamSynchronize(st->stream);
      return r;
    };
    d_ins.resize(cnt);
    d_outs.resize(cnt);
    uint64_t ntiles = 0;
    for (uint32_t j = 0; j < cnt; ++j) {
      d_ins[j] = st->d_in + off[j];
      d_outs[j] = st->d_out + off[j];
      ntiles += dec_tiles(glens[j]);
    }
    rc = enqueue_decrypt(cnt, d_ins.data(), glens.data(), st->d_in + key_off, ivs ? st->d_in + iv_off : nullptr,
                         d_outs.data(), reinterpret_cast<uint32_t *>(st->d_out + len_off),
                         reinterpret_cast<int32_t *>(st->d_out + st_off), ntiles, st->stream);
    if (rc) return drained(rc);
    e = hipMemcpyAsync(st->h_out, st->d_out, back_b, hipMemcpyDeviceToHost, st->stream);
    if (e != hipSuccess) return drained(hip_status(e));
    if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    // a message whose status is non-zero has nothing scattered
    parts.clear();
    const uint32_t *dl = reinterpret_cast<const uint32_t *>(st->h_out + len_off);
    const int32_t *ds = reinterpret_cast<const int32_t *>(st->h_out + st_off);
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t o = idx[j];
      statuses[o] = ds[j];
      out_lens[o] = ds[j] ? 0 : dl[j];
      if (ds[j]) {
        ++bad;
        continue;
      }
      parts.push_back({outs[o], st->h_out + off[j], dl[j]});
    }
    parallel_copy(parts);
    o0 = o1;
  }
  if (failed) *failed = bad;
  return VDS_EC_OK;
}

}  // namespace api
}  // namespace vds_ec

extern "C" {

int vds_ec_aes256_cbc_encrypt_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                           const uint8_t *keys, const uint8_t *ivs, uint8_t *const *outs,
                                           void *stream) {
  return vds_ec::api::aes_encrypt_batch_device(count, ins, lens, keys, ivs, outs, vds_ec::api::as_stream(stream));
}

int vds_ec_aes256_cbc_decrypt_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                           const uint8_t *keys, const uint8_t *ivs, uint8_t *const *outs,
                                           uint32_t *out_lens, int32_t *statuses, void *stream) {
  return vds_ec::api::aes_decrypt_batch_device(count, ins, lens, keys, ivs, outs, out_lens, statuses,
                                               vds_ec::api::as_stream(stream));
}

int vds_ec_block_pack_batch_device(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens,
                                   const uint8_t *const *zipped, const uint64_t *zipped_lens, uint8_t *ids,
                                   uint8_t *keys, uint8_t *const *crypted, void *stream) {
  return vds_ec::api::block_pack_batch_device(count, datas, data_lens, zipped, zipped_lens, ids, keys, crypted,
                                              vds_ec::api::as_stream(stream));
}

int vds_ec_block_pack_host_batch(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens,
                                 const uint8_t *const *zipped, const uint64_t *zipped_lens, uint8_t *ids,
                                 uint8_t *keys, uint8_t *const *crypted, uint64_t *crypted_sizes) {
  return vds_ec::api::block_pack_host_batch(count, datas, data_lens, zipped, zipped_lens, ids, keys, crypted,
                                            crypted_sizes);
}

int vds_ec_aes256_cbc_encrypt_gated_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *max_lens,
                                                 const uint32_t *lens, const uint8_t *keys, const uint8_t *ivs,
                                                 uint8_t *const *outs, uint32_t *out_lens, void *stream) {
  return vds_ec::api::aes_encrypt_gated_batch_device(count, ins, max_lens, lens, keys, ivs, outs, out_lens,
                                                     vds_ec::api::as_stream(stream));
}

int vds_ec_block_pack_deflate_batch_device(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens,
                                           uint8_t *ids, uint8_t *keys, uint8_t *const *crypted,
                                           const uint64_t *crypted_caps, uint32_t *crypted_lens, void *stream) {
  return vds_ec::api::block_pack_deflate_batch_device(count, datas, data_lens, ids, keys, crypted, crypted_caps,
                                                      crypted_lens, vds_ec::api::as_stream(stream));
}

int vds_ec_block_pack_deflate_host_batch(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens,
                                         uint8_t *ids, uint8_t *keys, uint8_t *const *crypted,
                                         const uint64_t *crypted_caps, uint64_t *crypted_sizes) {
  return vds_ec::api::block_pack_deflate_host_batch(count, datas, data_lens, ids, keys, crypted, crypted_caps,
                                                    crypted_sizes);
}

int vds_ec_aes256_cbc_decrypt_host_batch(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                         const uint8_t *keys, const uint8_t *ivs, uint8_t *const *outs,
                                         uint64_t *out_lens, int32_t *statuses, uint32_t *failed) {
  return vds_ec::api::aes_decrypt_host_batch(count, ins, lens, keys, ivs, outs, out_lens, statuses, failed);
}

int vds_ec_block_unpack_batch_device(uint32_t count, const uint8_t *const *crypted, const uint64_t *crypted_lens,
                                     const uint8_t *keys, const uint8_t *ids, uint8_t *const *outs,
                                     const uint64_t *out_caps, uint32_t *out_lens, int32_t *statuses, void *stream) {
  return vds_ec::api::block_unpack_batch_device(count, crypted, crypted_lens, keys, ids, outs, out_caps, out_lens,
                                                statuses, vds_ec::api::as_stream(stream));
}

int vds_ec_block_unpack_host_batch(uint32_t count, const uint8_t *const *crypted, const uint64_t *crypted_lens,
                                   const uint8_t *keys, const uint8_t *ids, uint8_t *const *outs,
                                   const uint64_t *out_caps, uint64_t *out_lens, int32_t *statuses, uint32_t *failed) {
  return vds_ec::api::block_unpack_host_batch(count, crypted, crypted_lens, keys, ids, outs, out_caps, out_lens,
                                              statuses, failed);
}

}  // extern "C"
