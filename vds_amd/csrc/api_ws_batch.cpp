// api_ws_batch.cpp -- the websocket frame round the upload and download loops
// (kernel/vds_http/websocket.cpp:45-257; the envelope of websocket_api.cpp:
// 30-49, :97-104, :141-155, :772-782): the "upload" answers written as frames
// on the device (vds_ec_ws_upload_answer_batch_device), the batched upload
// from frames to answer frames (vds_ec_ws_upload16_host_batch: the bodies
// cross PCIe still masked and are unmasked inside the decode), and the
// download loop answering in frames (vds_ec_ws_download16_host_batch).  The
// frame and envelope arithmetic itself is host code in vds_ec_wire.cpp.
// (api_internal.hpp lists the host runtime's translation units.)
#include "api_internal.hpp"

#include <string>

namespace vds_ec {
namespace api {

namespace {

// s as little-endian words into w[0..nw), zero behind its end
void pack_words(const std::string &s, uint32_t *w, size_t nw) {
  std::memset(w, 0, 4 * nw);
  std::memcpy(w, s.data(), std::min(s.size(), 4 * nw));
}

std::string id_text(int id) { return std::to_string((uint64_t)(int64_t)id); }

// the descriptor of one answer: everything but the addresses
void fill_answer(WsAnsMsg &m, int id, uint32_t n, uint32_t replica_size) {
  uint64_t flen = 0;
  uint32_t hl = 0;
  vds_ec_ws_upload_answer_size(id, n, replica_size, &flen, &hl);
  uint8_t h[10];
  vds_ec_ws_frame_header(flen - hl, 0, h, &hl);
  const std::string head =
      std::string(reinterpret_cast<const char *>(h), hl) + "{\"id\":\"" + id_text(id) + "\",\"result\":{\"replicas\":[";
  const std::string tail = "\",\"replica_size\":\"" + std::to_string((uint64_t)replica_size) + "\"}}";
  m.n = n;
  m.head_len = (uint32_t)head.size();
  m.tail_len = (uint32_t)tail.size();
  m.reserved = 0;
  pack_words(head, m.head, 16);
  pack_words(tail, m.tail, 9);
  std::memset(m.pad, 0, sizeof(m.pad));
}

size_t error_answer_len(int id, int status) {
  size_t l = 0;
  vds_ec_ws_error_answer(id, status, nullptr, 0, &l);
  return l;
}

}  // namespace

int ws_upload_answer_batch_device(uint32_t count, const int32_t *ids, uint32_t n, const uint8_t *replica_digests,
                                  const uint8_t *data_digests, const uint32_t *replica_sizes, uint8_t *const *outs,
                                  hipStream_t s) {
  if (n > 65536u || count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count && (!ids || !data_digests || !replica_sizes || !outs || (n && !replica_digests))) return VDS_EC_EINVAL;
  for (uint32_t o = 0; o < count; ++o)
    if (!outs[o]) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  const int rc = device_ready();
  if (rc) return rc;
  const size_t bytes = (size_t)count * sizeof(WsAnsMsg);
  ParamSlot *slot = nullptr;
  hipError_t e = param_acquire_n(1, &bytes, &slot);
  if (e != hipSuccess) return hip_status(e);
  WsAnsMsg *t = reinterpret_cast<WsAnsMsg *>(slot->h);
  for (uint32_t o = 0; o < count; ++o) {
    fill_answer(t[o], ids[o], n, replica_sizes[o]);
    t[o].out = reinterpret_cast<uintptr_t>(outs[o]);
    t[o].rdig = reinterpret_cast<uintptr_t>(replica_digests) + 32ull * o * n;
    t[o].ddig = reinterpret_cast<uintptr_t>(data_digests) + 32ull * o;
  }
  e = param_commit(slot, bytes, s);
  if (e == hipSuccess) e = launch_ws_upload_answer_batch(reinterpret_cast<const WsAnsMsg *>(slot->d), count, s);
  const hipError_t re = param_release(slot, s);
  return hip_status(e != hipSuccess ? e : re);
}

int ws_upload_host_batch(uint32_t k, uint32_t n, uint32_t count, const uint8_t *const *frames,
                         const uint64_t *frame_lens, uint8_t *const *outs, uint8_t *replica_digests,
                         uint8_t *data_digests, uint32_t *replica_sizes, uint8_t *answers, uint64_t answers_bytes,
                         uint64_t *answer_offs, uint64_t *answer_lens, int32_t *statuses, uint32_t *failed) {
  if (k == 0 || n > 65536u || count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count && (!frames || !frame_lens || !statuses || !answers || !answer_offs || !answer_lens ||
                (n && (!outs || !replica_digests))))
    return VDS_EC_EINVAL;
  if ((uint64_t)count * ((uint64_t)n + 64) > 0xFFFFFFFFull) return VDS_EC_EINVAL;
  // Every frame before any transfer: the header, the request, the sizes that
  // follow from them and the answers' places.
  struct Req {
    int32_t status, id;
    uint32_t mask;  // the frame's, rotated to the body's first character
    const uint8_t *body;
    uint64_t len, size, L, ok_len, slot;
  };
  std::vector<Req> rq(count);
  uint64_t ans_b = 0;
  for (uint32_t o = 0; o < count; ++o) {
    Req &r = rq[o];
    r = Req{};
    if (frame_lens[o] && !frames[o]) return VDS_EC_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
      if (!outs[(uint64_t)o * n + i]) return VDS_EC_EINVAL;
    answer_offs[o] = ans_b;
    answer_lens[o] = 0;
    vds_ec_ws_frame fr;
    r.status = vds_ec_ws_frame_parse(frames[o], frame_lens[o], &fr);
    if (r.status) continue;
    if (fr.payload_len > frame_lens[o] - fr.header_len) {
      r.status = VDS_EC_EWS_SHORT;
      continue;
    }
    if (fr.opcode == 9) {
      r.status = VDS_EC_EWS_PING;
      continue;
    }
    const uint8_t *payload = frames[o] + fr.header_len;
    uint64_t off = 0;
    r.status = vds_ec_ws_upload_request(payload, fr.payload_len, fr.masked ? fr.mask : nullptr, &r.id, &off, &r.len,
                                        &r.size);
    if (r.status) continue;
    if (r.len > 0xFFFFFFFFull) return VDS_EC_EINVAL;
    r.body = payload + off;
    for (uint32_t j = 0; j < 4; ++j) r.mask |= (uint32_t)fr.mask[(off + j) & 3] << (8 * j);
    r.L = vds_ec_replica_size(2, k, r.size, 0);
    if (r.L > 0xFFFFFFFFull) return VDS_EC_EINVAL;
    vds_ec_ws_upload_answer_size(r.id, n, (uint32_t)r.L, &r.ok_len, nullptr);
    r.slot = std::max<uint64_t>(r.ok_len, error_answer_len(r.id, VDS_EC_EB64_CHAR));
    ans_b += r.slot;
  }
  if (ans_b > answers_bytes) return VDS_EC_EINVAL;
  if (failed) *failed = 0;
  if (count == 0) return VDS_EC_OK;
  // (a batch with no device work needs no device; else nothing is written without one)
  uint32_t bad = 0, work = 0;
  for (uint32_t o = 0; o < count; ++o) work += rq[o].status == VDS_EC_OK;
  int rc = work ? device_ready() : VDS_EC_OK;
  if (rc) return rc;
  SaveTempStage *st = work ? save_temp_stage() : nullptr;
  if (work && !st) return VDS_EC_ENODEV;
  for (uint32_t o = 0; o < count; ++o)
    if (rq[o].status) {
      statuses[o] = rq[o].status;
      ++bad;
    }
  if (work == 0) {
    if (failed) *failed = bad;
    return VDS_EC_OK;
  }
  B64DecScratch &sc = b64_dec_scratch();
  std::vector<uint32_t> idx, rsz;
  std::vector<int32_t> gid;
  std::vector<uint64_t> in_off, body_off, out_off, size;
  std::vector<const uint8_t *> d_ins;
  std::vector<uint8_t *> d_outs, d_ans;
  std::vector<Copy> parts;
  for (uint32_t o0 = 0; o0 < count;) {
    // The group: the messages with device work among o0 .. o1-1.  BODIES (not
    // payloads) at 16-byte aligned offsets of the input staging, still masked;
    // in the output staging the replicas back to back, the names, the body
    // hashes, the statuses, the answer frames spaced as in the caller's slab
    // -- all copied back at once --, then the bodies, which stay on the device.
    idx.clear();
    in_off.clear();
    body_off.clear();
    out_off.clear();
    size.clear();
    uint64_t in_b = 0, rep_b = 0, body_b = 0;
    uint32_t o1 = o0;
    while (o1 < count && idx.size() < kSaveTempGroupObjects) {
      const Req &r = rq[o1];
      if (r.status) {
        ++o1;
        continue;
      }
      if (r.len % 4) {  // (no device work, as vds_ec_upload16_host_batch; its slot takes the error answer)
        statuses[o1] = VDS_EC_EB64_LENGTH;
        ++bad;
        size_t l = 0;
        vds_ec_ws_error_answer(r.id, VDS_EC_EB64_LENGTH, answers + answer_offs[o1], r.slot, &l);
        answer_lens[o1++] = l;
        continue;
      }
      const uint64_t at = (in_b + 15) & ~15ull;
      if (!idx.empty() && at + r.len > kSaveTempGroupBytes) break;
      idx.push_back(o1);
      in_off.push_back(at);
      in_b = at + r.len;
      size.push_back(r.size);
      body_off.push_back(body_b);
      body_b = (body_b + r.size + 15) & ~15ull;
      out_off.push_back(rep_b);
      rep_b += r.L * n;
      ++o1;
    }
    const uint32_t cnt = (uint32_t)idx.size();
    if (cnt == 0) {
      o0 = o1;
      continue;
    }
    const uint64_t a0 = answer_offs[idx[0]];  // the group's answers: one run of the caller's slab
    const uint64_t a_b = answer_offs[idx[cnt - 1]] + rq[idx[cnt - 1]].slot - a0;
    const uint64_t rd_off = (rep_b + 15) & ~15ull;
    const uint64_t dd_off = rd_off + 32ull * cnt * n;
    const uint64_t st_off = dd_off + 32ull * cnt;
    const uint64_t an_off = (st_off + 4ull * cnt + 15) & ~15ull;
    const uint64_t back_b = an_off + a_b;  // what is copied back
    const uint64_t bd_off = (back_b + 15) & ~15ull;
    if ((rc = st->reserve(std::max<uint64_t>(in_b, 64), bd_off + std::max<uint64_t>(body_b, 16)))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j)
      if (rq[idx[j]].len) parts.push_back({st->h_in + in_off[j], rq[idx[j]].body, rq[idx[j]].len});
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
    sc.masks.resize(cnt);
    d_ins.resize(cnt);
    d_outs.resize((size_t)cnt * n);
    d_ans.resize(cnt);
    gid.resize(cnt);
    rsz.resize(cnt);
    for (uint32_t j = 0; j < cnt; ++j) {
      const Req &r = rq[idx[j]];
      d_ins[j] = st->d_out + bd_off + body_off[j];
      sc.msgs[j] = B64DecMsg{reinterpret_cast<uintptr_t>(st->d_in + in_off[j]), reinterpret_cast<uintptr_t>(d_ins[j]),
                             reinterpret_cast<uintptr_t>(st->d_out + st_off + 4ull * j), (uint32_t)r.len,
                             (uint32_t)r.size};
      sc.masks[j] = r.mask;
      for (uint32_t i = 0; i < n; ++i) d_outs[(size_t)j * n + i] = st->d_out + out_off[j] + i * r.L;
      d_ans[j] = st->d_out + an_off + (answer_offs[idx[j]] - a0);
      gid[j] = r.id;
      rsz[j] = (uint32_t)r.L;
    }
    rc = launch_decode(sc, st->stream);
    sc.masks.clear();
    if (rc) return drained(rc);
    rc = save_temp_batch_device(k, n, cnt, d_ins.data(), size.data(), d_outs.data(), st->d_out + rd_off,
                                st->d_out + dd_off, st->stream);
    if (rc) return drained(rc);
    rc = ws_upload_answer_batch_device(cnt, gid.data(), n, st->d_out + rd_off, st->d_out + dd_off, rsz.data(),
                                       d_ans.data(), st->stream);
    if (rc) return drained(rc);
    e = hipMemcpyAsync(st->h_out, st->d_out, back_b, hipMemcpyDeviceToHost, st->stream);
    if (e != hipSuccess) return drained(hip_status(e));
    if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    // a message whose status is non-zero has none of its outputs scattered,
    // and the error answer in its slot
    parts.clear();
    const int32_t *dst = reinterpret_cast<const int32_t *>(st->h_out + st_off);
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t o = idx[j];
      const Req &r = rq[o];
      statuses[o] = dst[j];
      if (dst[j]) {
        ++bad;
        size_t l = 0;
        vds_ec_ws_error_answer(r.id, dst[j], answers + answer_offs[o], r.slot, &l);
        answer_lens[o] = l;
        continue;
      }
      for (uint32_t i = 0; i < n; ++i)
        parts.push_back({outs[(uint64_t)o * n + i], st->h_out + out_off[j] + i * r.L, r.L});
      if (n) parts.push_back({replica_digests + 32ull * o * n, st->h_out + rd_off + 32ull * j * n, 32ull * n});
      if (data_digests) parts.push_back({data_digests + 32ull * o, st->h_out + dd_off + 32ull * j, 32});
      parts.push_back({answers + answer_offs[o], st->h_out + an_off + (answer_offs[o] - a0), r.ok_len});
      answer_lens[o] = r.ok_len;
      if (replica_sizes) replica_sizes[o] = (uint32_t)r.L;
    }
    parallel_copy(parts);
    o0 = o1;
  }
  if (failed) *failed = bad;
  return VDS_EC_OK;
}

int ws_download_host_batch(uint32_t k, uint32_t count, const int32_t *ids, const uint16_t *nodes,
                           const uint8_t *const *chunks, const uint64_t *chunk_sizes, const uint8_t *survivor_names,
                           const uint16_t *witness_ids, const uint8_t *witness_names, uint8_t *slab,
                           uint64_t slab_bytes, uint64_t *frame_offs, uint64_t *frame_lens, int32_t *statuses,
                           uint8_t *survivor_verdicts, uint32_t *failed) {
  if (k == 0 || count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count && (!ids || !chunks || !chunk_sizes || !slab || !frame_offs || !frame_lens || !statuses))
    return VDS_EC_EINVAL;
  // The slots, from the trailers (download_host_batch validates the rest, and
  // decides `usable` as here): the text's place in its frame is known before
  // anything runs, so the text is copied once, from the staging to its frame.
  std::vector<char *> texts(count);
  std::vector<uint64_t> caps(count), ok_len(count), slot(count);
  uint64_t at = 0;
  for (uint32_t o = 0; o < count; ++o) {
    const uint64_t cs = chunk_sizes[o];
    const uint8_t *c0 = chunks[(uint64_t)o * k];
    if (cs < 2 || (cs - 2) % 2 || !c0) return VDS_EC_EINVAL;
    const uint16_t pad = (uint16_t)((c0[cs - 2] << 8) | c0[cs - 1]);
    bool ok = true;
    const uint64_t E = restored_len(2, k, cs, pad, 0, &ok);
    const bool usable = ok && !(witness_ids && pad > 2 * k);
    if (usable && E > 0xFFFFFFFFull) return VDS_EC_EINVAL;
    slot[o] = error_answer_len(ids[o], VDS_EC_ERESTORE);
    uint64_t t_off = 0;
    ok_len[o] = caps[o] = 0;
    if (usable) {
      vds_ec_ws_download_answer_layout(ids[o], E, &ok_len[o], nullptr, &t_off);
      caps[o] = (E + 2) / 3 * 4;
      slot[o] = std::max(slot[o], ok_len[o]);
    }
    if (slot[o] > slab_bytes || at > slab_bytes - slot[o]) return VDS_EC_EINVAL;
    frame_offs[o] = at;
    texts[o] = reinterpret_cast<char *>(slab + at + t_off);
    at += slot[o];
  }
  const int rc = download_host_batch(k, count, nodes, chunks, chunk_sizes, survivor_names, witness_ids, witness_names,
                                     texts.data(), caps.data(), statuses, survivor_verdicts, failed);
  if (rc) return rc;
  for (uint32_t o = 0; o < count; ++o) {
    uint8_t *f = slab + frame_offs[o];
    if (statuses[o]) {
      size_t l = 0;
      vds_ec_ws_error_answer(ids[o], statuses[o], f, slot[o], &l);
      frame_lens[o] = l;
      continue;
    }
    // header + {"id":"N","result":" in front of the text, "} behind it
    uint8_t h[10];
    uint32_t hl = 0;
    const uint64_t t_off = reinterpret_cast<uint8_t *>(texts[o]) - f;
    const std::string front = "{\"id\":\"" + id_text(ids[o]) + "\",\"result\":\"";
    hl = (uint32_t)(t_off - front.size());
    vds_ec_ws_frame_header(ok_len[o] - hl, 0, h, &hl);
    std::memcpy(f, h, hl);
    std::memcpy(f + hl, front.data(), front.size());
    std::memcpy(f + t_off + caps[o], "\"}", 2);
    frame_lens[o] = ok_len[o];
  }
  return VDS_EC_OK;
}

}  // namespace api
}  // namespace vds_ec

extern "C" {

int vds_ec_ws_upload_answer_batch_device(uint32_t count, const int32_t *ids, uint32_t n,
                                         const uint8_t *replica_digests, const uint8_t *data_digests,
                                         const uint32_t *replica_sizes, uint8_t *const *outs, void *stream) {
  return vds_ec::api::ws_upload_answer_batch_device(count, ids, n, replica_digests, data_digests, replica_sizes, outs,
                                                    vds_ec::api::as_stream(stream));
}

int vds_ec_ws_upload16_host_batch(uint16_t k, uint32_t n, uint32_t count, const uint8_t *const *frames,
                                  const uint64_t *frame_lens, uint8_t *const *outs, uint8_t *replica_digests,
                                  uint8_t *data_digests, uint32_t *replica_sizes, uint8_t *answers,
                                  uint64_t answers_bytes, uint64_t *answer_offs, uint64_t *answer_lens,
                                  int32_t *statuses, uint32_t *failed) {
  return vds_ec::api::ws_upload_host_batch(k, n, count, frames, frame_lens, outs, replica_digests, data_digests,
                                           replica_sizes, answers, answers_bytes, answer_offs, answer_lens, statuses,
                                           failed);
}

int vds_ec_ws_download16_host_batch(uint16_t k, uint32_t count, const int32_t *ids, const uint16_t *nodes,
                                    const uint8_t *const *chunks, const uint64_t *chunk_sizes,
                                    const uint8_t *survivor_names, const uint16_t *witness_ids,
                                    const uint8_t *witness_names, uint8_t *slab, uint64_t slab_bytes,
                                    uint64_t *frame_offs, uint64_t *frame_lens, int32_t *statuses,
                                    uint8_t *survivor_verdicts, uint32_t *failed) {
  return vds_ec::api::ws_download_host_batch(k, count, ids, nodes, chunks, chunk_sizes, survivor_names, witness_ids,
                                             witness_names, slab, slab_bytes, frame_offs, frame_lens, statuses,
                                             survivor_verdicts, failed);
}

}  // extern "C"
