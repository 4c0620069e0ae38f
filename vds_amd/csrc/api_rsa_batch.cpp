// api_rsa_batch.cpp -- RSA signatures of a batch verified on the device
// (rsa.hip's one launch, planned on the host): the raw public operation, the
// verdicts from digests, the verdicts from messages (the batched SHA-256 in
// front), and apply_message's check of a drained batch of transaction-log
// blocks through pinned staging (vds_ec_txblock_validate_host_batch).
// One of the host runtime's translation units (api_internal.hpp has what they
// share: the parameter ring, the staging, sha256_batch_device).
#include "api_internal.hpp"
#include "rsa_common.hpp"

namespace vds_ec {
namespace api {

// the RSA public operation of a batch (rsa.hip): the raw form and the verify form
hipError_t launch_rsa_public(const RsaLaunch &l, hipStream_t s);
hipError_t launch_rsa_verify(const RsaLaunch &l, hipStream_t s);

namespace {

// Everything the three device forms reject for the call, before anything is
// enqueued and before the device is looked for.  outs: the raw form's.
int check_rsa_args(uint32_t count, const uint8_t *const *ins, const uint64_t *in_lens, const uint32_t *key_idx,
                   const vds_ec_rsa_key *keys, uint32_t nkeys, uint8_t *const *outs, bool raw, const void *results) {
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  if (!ins || !in_lens || !key_idx || !keys || !results || (raw && !outs)) return VDS_EC_EINVAL;
  for (uint32_t j = 0; j < nkeys; ++j)
    if (!rsa_key_sane(keys[j])) return VDS_EC_EINVAL;
  for (uint32_t o = 0; o < count; ++o) {
    if (key_idx[o] >= nkeys || (in_lens[o] && !ins[o]) || (raw && !outs[o])) return VDS_EC_EINVAL;
  }
  return VDS_EC_OK;
}

// The table (the 128-limb items first: a wave of those runs four times as long)
// and the keys in one ring slot, and the launch.  digest_of: the verify form's
// digest index per item, null for the item's own.  (Validated; the device is
// ready.)
int enqueue_rsa(bool verify, uint32_t count, const uint8_t *const *ins, const uint64_t *in_lens,
                const uint32_t *key_idx, const vds_ec_rsa_key *keys, uint32_t nkeys, uint8_t *const *outs,
                const uint32_t *digest_of, const uint8_t *digests, uint8_t *results, hipStream_t s) {
  const size_t items_b = (size_t)count * sizeof(RsaItem), bytes = items_b + (size_t)nkeys * sizeof(vds_ec_rsa_key);
  ParamSlot *slot = nullptr;
  hipError_t e = param_acquire_n(1, &bytes, &slot);
  if (e != hipSuccess) return hip_status(e);
  RsaItem *t = reinterpret_cast<RsaItem *>(slot->h);
  uint32_t at = 0;
  for (uint32_t limbs = 128; limbs >= 64; limbs /= 2)
    for (uint32_t o = 0; o < count; ++o) {
      if (keys[key_idx[o]].limbs != limbs) continue;
      t[at++] = RsaItem{reinterpret_cast<uintptr_t>(ins[o]), outs ? reinterpret_cast<uintptr_t>(outs[o]) : 0,
                        (uint32_t)std::min<uint64_t>(in_lens[o], 0xFFFFFFFFull), key_idx[o], o,
                        digest_of ? digest_of[o] : o};
    }
  std::memcpy(slot->h + items_b, keys, (size_t)nkeys * sizeof(vds_ec_rsa_key));
  e = param_commit(slot, bytes, s);
  if (e == hipSuccess) {
    RsaLaunch l{};
    l.items = reinterpret_cast<const RsaItem *>(slot->d);
    l.keys = reinterpret_cast<const vds_ec_rsa_key *>(slot->d + items_b);
    l.count = at;
    l.digests = digests;
    l.results = results;
    e = verify ? launch_rsa_verify(l, s) : launch_rsa_public(l, s);
  }
  const hipError_t re = param_release(slot, s);  // (its event follows whatever was enqueued)
  return hip_status(e != hipSuccess ? e : re);
}

// The digests of vds_ec_rsa_verify_sha256_batch_device when the caller wants
// none: one buffer a device for the process, grown to a power of two and kept,
// under the rules of the pack's scratch (api_block_batch.cpp) -- a call holds
// the lock while it enqueues, and the event behind its last reader orders the
// next call's first writer after it on whatever stream that one runs.
struct DigestScratch {
  std::mutex mu;
  uint8_t *d = nullptr;
  size_t cap = 0;
  hipEvent_t done = nullptr;
  bool pending = false;
};
DigestScratch *digest_scratch() {
  static std::mutex m;
  static std::vector<DigestScratch *> per_dev;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return nullptr;
  std::lock_guard<std::mutex> g(m);
  if ((size_t)dev >= per_dev.size()) per_dev.resize(dev + 1, nullptr);
  if (!per_dev[dev]) per_dev[dev] = new DigestScratch();
  return per_dev[dev];
}

struct TxScratch {
  std::vector<vds_ec_txblock> parsed;
  std::vector<uint64_t> off, sha_len, sig_len;
  std::vector<const uint8_t *> sha_msg, sig;
  std::vector<uint32_t> key, digest_of, who, who_key;  // who: the group's checked blocks, by position
};
TxScratch &tx_scratch() {
  thread_local TxScratch t;
  return t;
}

}  // namespace

int rsa_public_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *in_lens,
                            const uint32_t *key_idx, const vds_ec_rsa_key *keys, uint32_t nkeys, uint8_t *const *outs,
                            uint8_t *statuses, hipStream_t s) {
  int rc = check_rsa_args(count, ins, in_lens, key_idx, keys, nkeys, outs, true, statuses);
  if (rc || count == 0) return rc;
  if ((rc = device_ready())) return rc;
  return enqueue_rsa(false, count, ins, in_lens, key_idx, keys, nkeys, outs, nullptr, nullptr, statuses, s);
}

int rsa_verify_digest_batch_device(uint32_t count, const uint8_t *digests, const uint8_t *const *sigs,
                                   const uint64_t *sig_lens, const uint32_t *key_idx, const vds_ec_rsa_key *keys,
                                   uint32_t nkeys, uint8_t *verdicts, hipStream_t s) {
  int rc = check_rsa_args(count, sigs, sig_lens, key_idx, keys, nkeys, nullptr, false, verdicts);
  if (rc || count == 0) return rc;
  if (!digests) return VDS_EC_EINVAL;
  if ((rc = device_ready())) return rc;
  return enqueue_rsa(true, count, sigs, sig_lens, key_idx, keys, nkeys, nullptr, nullptr, digests, verdicts, s);
}

int rsa_verify_sha256_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens,
                                   const uint8_t *const *sigs, const uint64_t *sig_lens, const uint32_t *key_idx,
                                   const vds_ec_rsa_key *keys, uint32_t nkeys, uint8_t *verdicts, uint8_t *digests,
                                   hipStream_t s) {
  int rc = check_rsa_args(count, sigs, sig_lens, key_idx, keys, nkeys, nullptr, false, verdicts);
  if (rc || count == 0) return rc;
  if (!msgs || !lens) return VDS_EC_EINVAL;
  for (uint32_t o = 0; o < count; ++o)
    if (lens[o] && !msgs[o]) return VDS_EC_EINVAL;
  if ((rc = device_ready())) return rc;
  if (digests) {
    if ((rc = sha256_batch_device(count, msgs, lens, digests, s))) return rc;
    return enqueue_rsa(true, count, sigs, sig_lens, key_idx, keys, nkeys, nullptr, nullptr, digests, verdicts, s);
  }
  DigestScratch *ds = digest_scratch();
  if (!ds) return VDS_EC_ENODEV;
  const size_t need = 32ull * count;
  std::lock_guard<std::mutex> g(ds->mu);
  if (!ds->done && hipEventCreateWithFlags(&ds->done, hipEventDisableTiming) != hipSuccess) return VDS_EC_ENODEV;
  if (need > ds->cap) {
    if (ds->pending) (void)hipEventSynchronize(ds->done);
    ds->pending = false;
    if (ds->d) (void)hipFree(ds->d);
    ds->d = nullptr;
    ds->cap = 0;
    size_t cap = 64u << 10;
    while (cap < need) cap *= 2;
    if (hipMalloc(&ds->d, cap) != hipSuccess) return VDS_EC_ENOMEM;
    ds->cap = cap;
  }
  if (ds->pending) {
    const hipError_t e = hipStreamWaitEvent(s, ds->done, 0);
    if (e != hipSuccess) return hip_status(e);
  }
  rc = sha256_batch_device(count, msgs, lens, ds->d, s);
  if (!rc) rc = enqueue_rsa(true, count, sigs, sig_lens, key_idx, keys, nkeys, nullptr, nullptr, ds->d, verdicts, s);
  // (the scratch's last reader, also when the second step failed behind the first one's launch)
  ds->pending = hipEventRecord(ds->done, s) == hipSuccess;
  if (!ds->pending) (void)hipStreamSynchronize(s);
  return rc;
}

int txblock_validate_host_batch(uint32_t count, const uint8_t *const *blocks, const uint64_t *lens,
                                const vds_ec_rsa_key *keys, const uint8_t *fingerprints, uint32_t nkeys, uint8_t *ids,
                                uint8_t *verdicts, int32_t *statuses) {
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  if (!blocks || !lens || !ids || !verdicts || !statuses || (nkeys && (!keys || !fingerprints))) return VDS_EC_EINVAL;
  for (uint32_t j = 0; j < nkeys; ++j)
    if (!rsa_key_sane(keys[j])) return VDS_EC_EINVAL;
  for (uint32_t o = 0; o < count; ++o)
    if (lens[o] > 0xFFFFFFFFull || (lens[o] && !blocks[o])) return VDS_EC_EINVAL;
  // the host's share: the split of every block and the writer's key
  TxScratch &t = tx_scratch();
  t.parsed.resize(count);
  t.key.resize(count);
  for (uint32_t o = 0; o < count; ++o) {
    verdicts[o] = 0;
    statuses[o] = lens[o] ? vds_ec_txblock_parse(blocks[o], lens[o], &t.parsed[o]) : VDS_EC_ETX_FORM;
    if (statuses[o]) continue;
    const vds_ec_txblock &b = t.parsed[o];
    uint32_t j = 0;
    const uint8_t *id = blocks[o] + b.key_id_off;
    while (j < nkeys && !(b.key_id_len == 32 && !std::memcmp(id, fingerprints + 32ull * j, 32))) ++j;
    if (j == nkeys) statuses[o] = VDS_EC_ETX_KEY;
    t.key[o] = j;
  }
  int rc = device_ready();
  if (rc) return rc;
  SaveTempStage *st = save_temp_stage();
  if (!st) return VDS_EC_ENODEV;
  std::vector<Copy> parts;
  for (uint32_t o0 = 0; o0 < count;) {
    // The group: blocks o0 .. o1-1, at most 64 MiB, at 16-byte aligned offsets
    // of the input staging; in the output staging the ids, the prefix digests
    // and the verdict bytes.
    t.off.clear();
    uint64_t in_b = 0;
    uint32_t o1 = o0;
    while (o1 < count && o1 - o0 < kSaveTempGroupObjects) {
      const uint64_t a = (in_b + 15) & ~15ull;
      if (o1 > o0 && a + lens[o1] > kSaveTempGroupBytes) break;
      t.off.push_back(a);
      in_b = a + lens[o1];
      ++o1;
    }
    const uint32_t cnt = o1 - o0;
    const uint64_t ver_off = 64ull * cnt, back_b = ver_off + cnt;
    if ((rc = st->reserve(std::max<uint64_t>(in_b, 64), back_b))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j) parts.push_back({st->h_in + t.off[j], blocks[o0 + j], lens[o0 + j]});
    parallel_copy(parts);
    hipError_t e = in_b ? hipMemcpyAsync(st->d_in, st->h_in, in_b, hipMemcpyHostToDevice, st->stream) : hipSuccess;
    if (e != hipSuccess) return hip_status(e);
    // (an error after the first enqueue drains the stream before returning:
    // the next call on this thread reuses the buffers)
    auto drained = [&](int r) {
      (void)hipStreamSynchronize(st->stream);
      return r;
    };
    // one SHA-256 launch: the blocks whole (the ids), then their signed prefixes
    t.sha_msg.assign(2ull * cnt, nullptr);
    t.sha_len.assign(2ull * cnt, 0);
    t.sig.clear();
    t.sig_len.clear();
    t.digest_of.clear();
    t.who.clear();
    t.who_key.clear();
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t o = o0 + j;
      t.sha_msg[j] = st->d_in + t.off[j];
      t.sha_len[j] = lens[o];
      if (statuses[o]) continue;
      t.sha_msg[cnt + j] = st->d_in + t.off[j];
      t.sha_len[cnt + j] = t.parsed[o].signed_len;
      t.sig.push_back(st->d_in + t.off[j] + t.parsed[o].signature_off);
      t.sig_len.push_back(t.parsed[o].signature_len);
      t.digest_of.push_back(cnt + j);
      t.who.push_back(j);
      t.who_key.push_back(t.key[o]);
    }
    rc = sha256_batch_device(2 * cnt, t.sha_msg.data(), t.sha_len.data(), st->d_out, st->stream);
    if (rc) return drained(rc);
    // verdict bytes by position in `who`: only the blocks that are checked have one
    const uint32_t nv = (uint32_t)t.who.size();
    if (nv) {
      rc = enqueue_rsa(true, nv, t.sig.data(), t.sig_len.data(), t.who_key.data(), keys, nkeys, nullptr,
                       t.digest_of.data(), st->d_out, st->d_out + ver_off, st->stream);
      if (rc) return drained(rc);
    }
    e = hipMemcpyAsync(st->h_out, st->d_out, ver_off + nv, hipMemcpyDeviceToHost, st->stream);
    if (e != hipSuccess) return drained(hip_status(e));
    if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    std::memcpy(ids + 32ull * o0, st->h_out, 32ull * cnt);
    for (uint32_t v = 0; v < nv; ++v) verdicts[o0 + t.who[v]] = st->h_out[ver_off + v];
    o0 = o1;
  }
  return VDS_EC_OK;
}

}  // namespace api
}  // namespace vds_ec

extern "C" {

int vds_ec_rsa_public_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *in_lens,
                                   const uint32_t *key_idx, const vds_ec_rsa_key *keys, uint32_t nkeys,
                                   uint8_t *const *outs, uint8_t *statuses, void *stream) {
  return vds_ec::api::rsa_public_batch_device(count, ins, in_lens, key_idx, keys, nkeys, outs, statuses,
                                              vds_ec::api::as_stream(stream));
}

int vds_ec_rsa_verify_digest_batch_device(uint32_t count, const uint8_t *digests, const uint8_t *const *sigs,
                                          const uint64_t *sig_lens, const uint32_t *key_idx,
                                          const vds_ec_rsa_key *keys, uint32_t nkeys, uint8_t *verdicts,
                                          void *stream) {
  return vds_ec::api::rsa_verify_digest_batch_device(count, digests, sigs, sig_lens, key_idx, keys, nkeys, verdicts,
                                                     vds_ec::api::as_stream(stream));
}

int vds_ec_rsa_verify_sha256_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens,
                                          const uint8_t *const *sigs, const uint64_t *sig_lens,
                                          const uint32_t *key_idx, const vds_ec_rsa_key *keys, uint32_t nkeys,
                                          uint8_t *verdicts, uint8_t *digests, void *stream) {
  return vds_ec::api::rsa_verify_sha256_batch_device(count, msgs, lens, sigs, sig_lens, key_idx, keys, nkeys,
                                                     verdicts, digests, vds_ec::api::as_stream(stream));
}

int vds_ec_txblock_validate_host_batch(uint32_t count, const uint8_t *const *blocks, const uint64_t *lens,
                                       const vds_ec_rsa_key *keys, const uint8_t *fingerprints, uint32_t nkeys,
                                       uint8_t *ids, uint8_t *verdicts, int32_t *statuses) {
  return vds_ec::api::txblock_validate_host_batch(count, blocks, lens, keys, fingerprints, nkeys, ids, verdicts,
                                                  statuses);
}

}  // extern "C"
