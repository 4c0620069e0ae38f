// api_upload_batch.cpp -- the base64 wire text of the upload and download
// loops on the device (vds_ec_base64_decode_batch_device /
// _encode_batch_device: base64.hip's two launches, planned on the host), and
// the batched upload from text (vds_ec_upload16_host_batch): the websocket
// "upload" bodies (websocket_api.cpp:141-155) decoded in front of the batched
// save_temp (api_save_temp_batch.cpp), so that the host never walks a text
// character by character.
// (api_internal.hpp lists the host runtime's translation units.)
#include "api_internal.hpp"

namespace vds_ec {
namespace api {

namespace {

// What a text of len characters decodes to must be one of len/4*3 - p, p = 0, 1, 2 (0 when len % 4)
bool decoded_size_legal(uint64_t len, uint64_t size) {
  if (len % 4) return size == 0;
  const uint64_t q = len / 4 * 3;
  return size <= q && q - size <= 2;
}

// vds_ec_base64_decoded_size of a host text whose length is a multiple of 4
uint64_t decoded_size(const char *t, uint64_t len) {
  uint64_t p = 0;
  if (len > 0 && t[len - 1] == '=') p = len > 1 && t[len - 2] == '=' ? 2 : 1;
  return len / 4 * 3 - p;
}

}  // namespace

B64DecScratch &b64_dec_scratch() {
  thread_local B64DecScratch sc;
  return sc;
}

// One wave walks one message, so the messages go longest first (by steps of
// the kernel): the long walks set the launch's critical path and start at
// once.  Equal keys keep the caller's order.  A counting sort where the steps
// are few against the batch (the upload loop: 16,384 texts of up to 86
// steps), else a comparison sort.  Then the table in one ring slot and the
// launch.  With masks (one word a message, beside msgs) the table of masks
// follows the messages' in the slot, in the same order, and the launch is the
// masked instance.
int launch_decode(B64DecScratch &sc, hipStream_t s) {
  const size_t nm = sc.msgs.size();
  if (nm == 0) return VDS_EC_OK;
  const bool masked = !sc.masks.empty();
  sc.key.resize(nm);
  sc.order.resize(nm);
  uint32_t kmax = 0;
  for (size_t j = 0; j < nm; ++j) {
    sc.key[j] = sc.msgs[j].len / kB64DecStep;
    kmax = std::max(kmax, sc.key[j]);
  }
  if (kmax <= 4 * nm + 4096) {
    sc.bucket.assign((size_t)kmax + 2, 0);
    for (size_t j = 0; j < nm; ++j) ++sc.bucket[kmax - sc.key[j] + 1];
    for (size_t b = 1; b < sc.bucket.size(); ++b) sc.bucket[b] += sc.bucket[b - 1];
    for (size_t j = 0; j < nm; ++j) sc.order[sc.bucket[kmax - sc.key[j]]++] = (uint32_t)j;
  } else {
    for (size_t j = 0; j < nm; ++j) sc.order[j] = (uint32_t)j;
    std::stable_sort(sc.order.begin(), sc.order.end(),
                     [&](uint32_t a, uint32_t b) { return sc.msgs[a].len > sc.msgs[b].len; });
  }
  const size_t o_masks = nm * sizeof(B64DecMsg);
  const size_t bytes = o_masks + (masked ? nm * sizeof(uint32_t) : 0);
  ParamSlot *slot = nullptr;
  hipError_t e = param_acquire_n(1, &bytes, &slot);
  if (e != hipSuccess) return hip_status(e);
  B64DecMsg *t = reinterpret_cast<B64DecMsg *>(slot->h);
  for (size_t j = 0; j < nm; ++j) t[j] = sc.msgs[sc.order[j]];
  if (masked) {
    uint32_t *mk = reinterpret_cast<uint32_t *>(slot->h + o_masks);
    for (size_t j = 0; j < nm; ++j) mk[j] = sc.masks[sc.order[j]];
  }
  e = param_commit(slot, bytes, s);
  if (e == hipSuccess)
    e = masked ? launch_b64_decode_masked_batch(reinterpret_cast<const B64DecMsg *>(slot->d),
                                                reinterpret_cast<const uint32_t *>(slot->d + o_masks), (uint32_t)nm, s)
               : launch_b64_decode_batch(reinterpret_cast<const B64DecMsg *>(slot->d), (uint32_t)nm, s);
  const hipError_t re = param_release(slot, s);  // (its event follows whatever was enqueued)
  return hip_status(e != hipSuccess ? e : re);
}

int base64_decode_batch_device(uint32_t count, const char *const *texts, const uint64_t *text_lens,
                               const uint8_t *masks, bool masked, uint8_t *const *outs, const uint64_t *out_sizes,
                               int32_t *statuses, hipStream_t s) {
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count && (!texts || !text_lens || !outs || !out_sizes || !statuses || (masked && !masks))) return VDS_EC_EINVAL;
  for (uint32_t o = 0; o < count; ++o) {
    if (text_lens[o] > 0xFFFFFFFFull || !decoded_size_legal(text_lens[o], out_sizes[o])) return VDS_EC_EINVAL;
    if ((text_lens[o] && !texts[o]) || (out_sizes[o] && !outs[o])) return VDS_EC_EINVAL;
  }
  if (count == 0) return VDS_EC_OK;
  const int rc = device_ready();
  if (rc) return rc;
  B64DecScratch &sc = b64_dec_scratch();
  sc.msgs.resize(count);
  for (uint32_t o = 0; o < count; ++o)
    sc.msgs[o] = B64DecMsg{reinterpret_cast<uintptr_t>(texts[o]), reinterpret_cast<uintptr_t>(outs[o]),
                           reinterpret_cast<uintptr_t>(statuses + o), (uint32_t)text_lens[o], (uint32_t)out_sizes[o]};
  sc.masks.clear();
  if (masked) {
    sc.masks.resize(count);
    std::memcpy(sc.masks.data(), masks, 4ull * count);  // (bytes 0..3 of a mask: a little-endian word)
  }
  return launch_decode(sc, s);
}

int base64_encode_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, char *const *outs,
                               hipStream_t s) {
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count && (!ins || !lens || !outs)) return VDS_EC_EINVAL;
  uint64_t ntiles = 0;
  for (uint32_t o = 0; o < count; ++o) {
    if (lens[o] > 0xFFFFFFFFull || (lens[o] && (!ins[o] || !outs[o]))) return VDS_EC_EINVAL;
    ntiles += (lens[o] + kB64EncTile - 1) / kB64EncTile;
  }
  if (ntiles > 0x7FFFFFFFull) return VDS_EC_EINVAL;  // (the launch's waves)
  if (count == 0) return VDS_EC_OK;
  const int rc = device_ready();
  if (rc) return rc;
  if (ntiles == 0) return VDS_EC_OK;  // (every input empty: no character to write)
  // the messages, then a tile table over all of them, in one ring slot
  const size_t o_tiles = ((size_t)count * sizeof(B64EncMsg) + 15) & ~size_t(15);
  const size_t bytes = o_tiles + ntiles * sizeof(B64EncTile);
  ParamSlot *slot = nullptr;
  hipError_t e = param_acquire_n(1, &bytes, &slot);
  if (e != hipSuccess) return hip_status(e);
  B64EncMsg *msgs = reinterpret_cast<B64EncMsg *>(slot->h);
  B64EncTile *tiles = reinterpret_cast<B64EncTile *>(slot->h + o_tiles);
  size_t t = 0;
  for (uint32_t o = 0; o < count; ++o) {
    msgs[o] = B64EncMsg{reinterpret_cast<uintptr_t>(ins[o]), reinterpret_cast<uintptr_t>(outs[o]), lens[o]};
    const uint32_t nt = (uint32_t)((lens[o] + kB64EncTile - 1) / kB64EncTile);
    for (uint32_t i = 0; i < nt; ++i) tiles[t++] = B64EncTile{o, i};
  }
  e = param_commit(slot, bytes, s);
  if (e == hipSuccess)
    e = launch_b64_encode_batch(reinterpret_cast<const B64EncMsg *>(slot->d),
                                reinterpret_cast<const B64EncTile *>(slot->d + o_tiles), (uint32_t)ntiles, s);
  const hipError_t re = param_release(slot, s);
  return hip_status(e != hipSuccess ? e : re);
}

int upload_host_batch(uint32_t k, uint32_t n, uint32_t count, const char *const *texts, const uint64_t *text_lens,
                      uint8_t *const *outs, uint8_t *replica_digests, uint8_t *data_digests, uint32_t *replica_sizes,
                      uint8_t *const *bodies, uint64_t *body_sizes, int32_t *statuses, uint32_t *failed) {
  // save_temp's checks and the decode's, every message before any transfer
  if (k == 0 || n > 65536u || count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count && (!texts || !text_lens || !statuses || (n && (!outs || !replica_digests)))) return VDS_EC_EINVAL;
  if ((uint64_t)count * ((uint64_t)n + 64) > 0xFFFFFFFFull) return VDS_EC_EINVAL;
  for (uint32_t o = 0; o < count; ++o) {
    if (text_lens[o] > 0xFFFFFFFFull || (text_lens[o] && !texts[o])) return VDS_EC_EINVAL;
    if (bodies && text_lens[o] >= 4 && text_lens[o] % 4 == 0 && !bodies[o]) return VDS_EC_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
      if (!outs[(uint64_t)o * n + i]) return VDS_EC_EINVAL;
  }
  if (failed) *failed = 0;
  if (count == 0) return VDS_EC_OK;
  int rc = device_ready();
  if (rc) return rc;
  SaveTempStage *st = save_temp_stage();
  if (!st) return VDS_EC_ENODEV;
  B64DecScratch &sc = b64_dec_scratch();
  std::vector<uint32_t> idx;  // the group's messages (a text whose length is no multiple of 4 gets no device work)
  std::vector<uint64_t> in_off, body_off, out_off, L, size;
  std::vector<const uint8_t *> d_ins;
  std::vector<uint8_t *> d_outs;
  std::vector<Copy> parts;
  uint32_t bad = 0;
  for (uint32_t o0 = 0; o0 < count;) {
    // The group: messages o0 .. o1-1.  Texts at 16-byte aligned offsets of the
    // input staging; in the output staging the replicas back to back, the
    // names, the body hashes, the statuses, then the bodies at 16-byte
    // aligned offsets (copied back only when the caller asks for them).
    // Sizes come from the host texts, so nothing waits for the decode.
    idx.clear();
    in_off.clear();
    body_off.clear();
    out_off.clear();
    L.clear();
    size.clear();
    uint64_t in_b = 0, rep_b = 0, body_b = 0;
    uint32_t o1 = o0;
    while (o1 < count && idx.size() < kSaveTempGroupObjects) {
      const uint64_t len = text_lens[o1];
      if (len % 4) {
        statuses[o1++] = VDS_EC_EB64_LENGTH;
        ++bad;
        continue;
      }
      const uint64_t at = (in_b + 15) & ~15ull;
      if (!idx.empty() && at + len > kSaveTempGroupBytes) break;
      idx.push_back(o1);
      in_off.push_back(at);
      in_b = at + len;
      size.push_back(decoded_size(texts[o1], len));
      body_off.push_back(body_b);
      body_b = (body_b + size.back() + 15) & ~15ull;
      L.push_back(vds_ec_replica_size(2, k, size.back(), 0));
      out_off.push_back(rep_b);
      rep_b += L.back() * n;
      ++o1;
    }
    const uint32_t cnt = (uint32_t)idx.size();
    if (cnt == 0) {
      o0 = o1;
      continue;
    }
    const uint64_t rd_off = (rep_b + 15) & ~15ull;
    const uint64_t dd_off = rd_off + 32ull * cnt * n;
    const uint64_t st_off = dd_off + (data_digests ? 32ull * cnt : 0);
    const uint64_t bd_off = (st_off + 4ull * cnt + 15) & ~15ull;
    const uint64_t back_b = bodies ? bd_off + body_b : st_off + 4ull * cnt;  // what is copied back
    if ((rc = st->reserve(std::max<uint64_t>(in_b, 64), bd_off + std::max<uint64_t>(body_b, 16)))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j)
      if (text_lens[idx[j]])
        parts.push_back({st->h_in + in_off[j], reinterpret_cast<const uint8_t *>(texts[idx[j]]), text_lens[idx[j]]});
    parallel_copy(parts);
    hipError_t e = in_b ? hipMemcpyAsync(st->d_in, st->h_in, in_b, hipMemcpyHostToDevice, st->stream) : hipSuccess;
    if (e != hipSuccess) return hip_status(e);
    // (an error after the first enqueue drains the stream before returning:
    // the next call on this thread reuses the buffers)
    auto drained = [&](int r) {
      (void)hipStreamSynchronize(st->stream);
      return r;
    };
    sc.msgs.resize(cnt);
    d_ins.resize(cnt);
    d_outs.resize((size_t)cnt * n);
    for (uint32_t j = 0; j < cnt; ++j) {
      d_ins[j] = st->d_out + bd_off + body_off[j];
      sc.msgs[j] = B64DecMsg{reinterpret_cast<uintptr_t>(st->d_in + in_off[j]), reinterpret_cast<uintptr_t>(d_ins[j]),
                             reinterpret_cast<uintptr_t>(st->d_out + st_off + 4ull * j), (uint32_t)text_lens[idx[j]],
                             (uint32_t)size[j]};
      for (uint32_t i = 0; i < n; ++i) d_outs[(size_t)j * n + i] = st->d_out + out_off[j] + i * L[j];
    }
    sc.masks.clear();
    if ((rc = launch_decode(sc, st->stream))) return drained(rc);
    rc = save_temp_batch_device(k, n, cnt, d_ins.data(), size.data(), d_outs.data(), st->d_out + rd_off,
                                data_digests ? st->d_out + dd_off : nullptr, st->stream);
    if (rc) return drained(rc);
    e = hipMemcpyAsync(st->h_out, st->d_out, back_b, hipMemcpyDeviceToHost, st->stream);
    if (e != hipSuccess) return drained(hip_status(e));
    if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    // a message whose status is non-zero has none of its outputs scattered
    parts.clear();
    const int32_t *dst = reinterpret_cast<const int32_t *>(st->h_out + st_off);
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t o = idx[j];
      statuses[o] = dst[j];
      if (dst[j]) {
        ++bad;
        continue;
      }
      for (uint32_t i = 0; i < n; ++i)
        parts.push_back({outs[(uint64_t)o * n + i], st->h_out + out_off[j] + i * L[j], L[j]});
      if (n) parts.push_back({replica_digests + 32ull * o * n, st->h_out + rd_off + 32ull * j * n, 32ull * n});
      if (data_digests) parts.push_back({data_digests + 32ull * o, st->h_out + dd_off + 32ull * j, 32});
      if (bodies && size[j]) parts.push_back({bodies[o], st->h_out + bd_off + body_off[j], size[j]});
      if (replica_sizes) replica_sizes[o] = (uint32_t)L[j];
      if (body_sizes) body_sizes[o] = size[j];
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

int vds_ec_base64_decode_batch_device(uint32_t count, const char *const *texts, const uint64_t *text_lens,
                                      uint8_t *const *outs, const uint64_t *out_sizes, int32_t *statuses,
                                      void *stream) {
  return vds_ec::api::base64_decode_batch_device(count, texts, text_lens, nullptr, false, outs, out_sizes, statuses,
                                                 vds_ec::api::as_stream(stream));
}

int vds_ec_base64_decode_masked_batch_device(uint32_t count, const char *const *texts, const uint64_t *text_lens,
                                             const uint8_t *masks, uint8_t *const *outs, const uint64_t *out_sizes,
                                             int32_t *statuses, void *stream) {
  return vds_ec::api::base64_decode_batch_device(count, texts, text_lens, masks, true, outs, out_sizes, statuses,
                                                 vds_ec::api::as_stream(stream));
}

int vds_ec_base64_encode_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                      char *const *outs, void *stream) {
  return vds_ec::api::base64_encode_batch_device(count, ins, lens, outs, vds_ec::api::as_stream(stream));
}

int vds_ec_upload16_host_batch(uint16_t k, uint32_t n, uint32_t count, const char *const *texts,
                               const uint64_t *text_lens, uint8_t *const *outs, uint8_t *replica_digests,
                               uint8_t *data_digests, uint32_t *replica_sizes, uint8_t *const *bodies,
                               uint64_t *body_sizes, int32_t *statuses, uint32_t *failed) {
  return vds_ec::api::upload_host_batch(k, n, count, texts, text_lens, outs, replica_digests, data_digests,
                                        replica_sizes, bodies, body_sizes, statuses, failed);
}

}  // extern "C"
