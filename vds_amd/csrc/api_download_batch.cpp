// api_download_batch.cpp -- the download loop for a batch in one call
// (vds_ec_download16_batch_device / _host_batch): websocket_api.cpp:191-210 ->
// _client::restore_async (dht_network_client.cpp:851-901) -> the base64 answer
// (websocket_api.cpp:772-782).  The reference decodes the replica files
// without hashing them; here the names the request carries
// (websocket_api.cpp:193) are checked on the device first -- every survivor's,
// or one regenerated replica's (a witness: the code is MDS, so any changed
// cell of any survivor changes it) -- and the base64 encode behind the restore
// reads the verdicts (k_b64_encode_batch<true>, base64.hip): an object that
// fails the check never becomes text.
// (api_internal.hpp lists the host runtime's translation units.)
#include "api_internal.hpp"

namespace vds_ec {
namespace api {

namespace {

inline uint64_t enc_tiles(uint64_t len) { return std::max<uint64_t>(1, (len + kB64EncTile - 1) / kB64EncTile); }

// The gated launch over validated messages (the device is ready): message o's
// gate is gate_of(o), ngate_of(o) bytes.  Messages, gates and the tile table
// (a tile 0 for every message) in one ring slot.
template <typename GateOf, typename NGateOf>
int gated_encode(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, char *const *outs, GateOf gate_of,
                 NGateOf ngate_of, int32_t *statuses, uint64_t ntiles, hipStream_t s) {
  const size_t o_gates = ((size_t)count * sizeof(B64EncMsg) + 15) & ~size_t(15);
  const size_t o_tiles = (o_gates + (size_t)count * sizeof(B64EncGate) + 15) & ~size_t(15);
  const size_t bytes = o_tiles + ntiles * sizeof(B64EncTile);
  ParamSlot *slot = nullptr;
  hipError_t e = param_acquire_n(1, &bytes, &slot);
  if (e != hipSuccess) return hip_status(e);
  B64EncMsg *msgs = reinterpret_cast<B64EncMsg *>(slot->h);
  B64EncGate *gates = reinterpret_cast<B64EncGate *>(slot->h + o_gates);
  B64EncTile *tiles = reinterpret_cast<B64EncTile *>(slot->h + o_tiles);
  size_t t = 0;
  for (uint32_t o = 0; o < count; ++o) {
    msgs[o] = B64EncMsg{reinterpret_cast<uintptr_t>(ins[o]), reinterpret_cast<uintptr_t>(outs[o]), lens[o]};
    gates[o] = B64EncGate{reinterpret_cast<uintptr_t>(gate_of(o)), reinterpret_cast<uintptr_t>(statuses + o),
                          ngate_of(o), 0};
    const uint32_t nt = (uint32_t)enc_tiles(lens[o]);
    for (uint32_t i = 0; i < nt; ++i) tiles[t++] = B64EncTile{o, i};
  }
  e = param_commit(slot, bytes, s);
  if (e == hipSuccess)
    e = launch_b64_encode_gated_batch(reinterpret_cast<const B64EncMsg *>(slot->d),
                                      reinterpret_cast<const B64EncGate *>(slot->d + o_gates),
                                      reinterpret_cast<const B64EncTile *>(slot->d + o_tiles), (uint32_t)ntiles, s);
  const hipError_t re = param_release(slot, s);  // (its event follows whatever was enqueued)
  return hip_status(e != hipSuccess ? e : re);
}

// Per-thread tables of the download calls, reused from call to call.
struct DownloadScratch {
  std::vector<uint64_t> lens;        // the restored sizes E
  std::vector<const uint8_t *> exp;  // survivor mode: each object's k names
  std::vector<uint8_t *> ver;        // ... and its k verdict bytes
};
DownloadScratch &download_scratch() {
  thread_local DownloadScratch sc;
  return sc;
}

}  // namespace

int base64_encode_gated_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                     char *const *outs, const uint8_t *const *gates, const uint32_t *ngates,
                                     int32_t *statuses, hipStream_t s) {
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count && (!ins || !lens || !outs || !gates || !ngates || !statuses)) return VDS_EC_EINVAL;
  uint64_t ntiles = 0;
  for (uint32_t o = 0; o < count; ++o) {
    if (lens[o] > 0xFFFFFFFFull || (lens[o] && (!ins[o] || !outs[o]))) return VDS_EC_EINVAL;
    if (ngates[o] && !gates[o]) return VDS_EC_EINVAL;
    ntiles += enc_tiles(lens[o]);
  }
  if (ntiles > 0x7FFFFFFFull) return VDS_EC_EINVAL;  // (the launch's waves)
  if (count == 0) return VDS_EC_OK;
  const int rc = device_ready();
  if (rc) return rc;
  return gated_encode(
      count, ins, lens, outs, [&](uint32_t o) { return gates[o]; }, [&](uint32_t o) { return ngates[o]; }, statuses,
      ntiles, s);
}

int download_batch_device(uint32_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                          const uint64_t *chunk_sizes, const uint16_t *paddings, const uint8_t *survivor_names,
                          const uint16_t *witness_ids, const uint8_t *witness_names, uint8_t *const *witness_outs,
                          uint8_t *const *objects, char *const *texts, uint8_t *verdicts, int32_t *statuses,
                          hipStream_t s) {
  if (k == 0) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (!nodes || !chunks || !chunk_sizes || !paddings || !objects || !texts || !verdicts || !statuses)
    return VDS_EC_EINVAL;
  // exactly one check: every survivor's name, or the witness triple
  const bool wit = witness_ids || witness_names || witness_outs;
  if (wit == (survivor_names != nullptr)) return VDS_EC_EINVAL;
  if (wit && (!witness_ids || !witness_names || !witness_outs)) return VDS_EC_EINVAL;
  // the hash launch's lanes: a group of k survivors, or of one witness, an object
  if ((uint64_t)count * ((wit ? 1ull : k) + 64) > 0xFFFFFFFFull) return VDS_EC_EINVAL;
  // Every object as vds_ec_restore16_batch_device checks it, as the name
  // check does and, with a witness, as vds_ec_repair16_batch_device does;
  // then the encode's own limits.  Nothing has been enqueued yet.
  DownloadScratch &sc = download_scratch();
  sc.lens.resize(count);
  uint64_t ntiles = 0;
  for (uint32_t o = 0; o < count; ++o) {
    const uint16_t *nd = nodes + (uint64_t)o * k;
    const uint8_t *const *ch = chunks + (uint64_t)o * k;
    const uint64_t cs = chunk_sizes[o];
    if (wit && (cs < 2 || (cs - 2) % 2 || !witness_outs[o])) return VDS_EC_EINVAL;  // cells + BE16 trailer
    for (uint32_t j = 0; j < k; ++j)
      if (!ch[j] && (wit || cs)) return VDS_EC_EINVAL;
    bool ok = true;
    const uint64_t E = restored_len(2, k, cs, paddings[o], 0, &ok);
    if (!ok) return VDS_EC_ERESTORE;
    if (E > 0xFFFFFFFFull || (E && (!objects[o] || !texts[o]))) return VDS_EC_EINVAL;
    if ((wit || E) && !ids_distinct(k, nd)) return VDS_EC_ESINGULAR;
    if (wit)
      for (uint32_t j = 0; j < k; ++j)
        if (nd[j] == witness_ids[o]) return VDS_EC_EINVAL;  // a survivor is no witness
    sc.lens[o] = E;
    ntiles += enc_tiles(E);
  }
  if (ntiles > 0x7FFFFFFFull) return VDS_EC_EINVAL;  // (the encode launch's waves)
  int rc = device_ready();
  if (rc) return rc;
  // 1. the check
  if (wit) {
    // the repair call's two launches with ntargets = 1; the witness's own name
    // is compared inside the hash launch and stored nowhere (check only)
    if ((rc = regenerate_batch_device(k, count, nodes, chunks, chunk_sizes, 1, witness_ids, witness_outs, s)))
      return rc;
    rc = sha256_check_batch_device(count, witness_outs, chunk_sizes, witness_names, nullptr, verdicts, s);
  } else {
    // vds_ec_sha256_check_batch_device's launch over the count*k survivors,
    // planned as one group of k messages an object (one length, names and
    // verdicts contiguous): 1/k of the descriptors for the host to order
    sc.exp.resize(count);
    sc.ver.resize(count);
    for (uint32_t o = 0; o < count; ++o) {
      sc.exp[o] = survivor_names + 32ull * k * o;
      sc.ver[o] = verdicts + (uint64_t)k * o;
    }
    rc = sha256_check_groups_device(count, k, chunks, chunk_sizes, sc.exp.data(), sc.ver.data(), s);
  }
  if (rc) return rc;
  // 2. the restore
  if ((rc = restore_batch_device(k, count, nodes, chunks, chunk_sizes, paddings, objects, 0, s))) return rc;
  // 3. the encode, behind the verdicts
  const uint32_t ngate = wit ? 1u : k;
  return gated_encode(
      count, objects, sc.lens.data(), texts, [&](uint32_t o) { return verdicts + (uint64_t)o * ngate; },
      [&](uint32_t) { return ngate; }, statuses, ntiles, s);
}

int download_host_batch(uint32_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                        const uint64_t *chunk_sizes, const uint8_t *survivor_names, const uint16_t *witness_ids,
                        const uint8_t *witness_names, char *const *texts, uint64_t *text_lens, int32_t *statuses,
                        uint8_t *survivor_verdicts, uint32_t *failed) {
  if (k == 0) return VDS_EC_EINVAL;
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count && (!nodes || !chunks || !chunk_sizes || !survivor_names || !texts || !text_lens || !statuses ||
                !survivor_verdicts))
    return VDS_EC_EINVAL;
  if ((witness_ids == nullptr) != (witness_names == nullptr)) return VDS_EC_EINVAL;
  const bool wit = witness_ids != nullptr;
  // Every object before any transfer.  The host has the trailers: the first
  // chunk's gives the padding (chunk.h:408).  An object whose trailer has no
  // answer -- restore's "Fatal error", or, with a witness, above 2k, where the
  // witness is unspecified -- gets no restore: `usable` is 0 and it goes to
  // the locating pass.
  std::vector<uint64_t> E(count), need(count);
  std::vector<uint16_t> pad(count);
  std::vector<uint8_t> usable(count);
  for (uint32_t o = 0; o < count; ++o) {
    const uint64_t cs = chunk_sizes[o];
    const uint16_t *nd = nodes + (uint64_t)o * k;
    if (cs < 2 || (cs - 2) % 2) return VDS_EC_EINVAL;
    for (uint32_t j = 0; j < k; ++j)
      if (!chunks[(uint64_t)o * k + j]) return VDS_EC_EINVAL;
    if (!ids_distinct(k, nd)) return VDS_EC_ESINGULAR;
    if (wit)
      for (uint32_t j = 0; j < k; ++j)
        if (nd[j] == witness_ids[o]) return VDS_EC_EINVAL;
    const uint8_t *c0 = chunks[(uint64_t)o * k];
    pad[o] = (uint16_t)((c0[cs - 2] << 8) | c0[cs - 1]);
    bool ok = true;
    E[o] = restored_len(2, k, cs, pad[o], 0, &ok);
    usable[o] = ok && !(wit && pad[o] > 2 * k);
    need[o] = 0;
    if (!usable[o]) continue;
    if (E[o] > 0xFFFFFFFFull) return VDS_EC_EINVAL;
    need[o] = (E[o] + 2) / 3 * 4;
    if (text_lens[o] < need[o] || (need[o] && !texts[o])) return VDS_EC_EINVAL;
  }
  if (failed) *failed = 0;
  if (count == 0) return VDS_EC_OK;
  int rc = device_ready();
  if (rc) return rc;
  SaveTempStage *st = save_temp_stage();
  if (!st) return VDS_EC_ENODEV;
  std::vector<uint32_t> use, rest, locate;  // the group's usable objects, the others, those to locate a failure in
  std::vector<uint64_t> in_off, t_off, ob_off, wo_off, csz, lens;
  std::vector<uint16_t> nd, pd, wid;
  std::vector<const uint8_t *> d_chunks, d_exp;
  std::vector<uint8_t *> d_objs, d_wouts, d_ver;
  std::vector<char *> d_texts;
  std::vector<Copy> parts;
  uint32_t bad = 0;
  for (uint32_t o0 = 0; o0 < count;) {
    // The group: objects o0 .. o1-1, each object's k survivors back to back
    // from a 16-byte aligned offset of the input staging, then the survivors'
    // names -- the usable objects' first -- and the witnesses' names.  In the
    // output staging the texts at 16-byte aligned offsets, the statuses and
    // (survivor mode) the gate, all copied back at once; behind them the
    // witness gate, the locating pass's verdicts, the restored objects and
    // the witnesses, which stay on the device.
    in_off.clear();
    use.clear();
    rest.clear();
    uint64_t in_b = 0;
    uint32_t o1 = o0;
    while (o1 < count && o1 - o0 < kSaveTempGroupObjects) {
      const uint64_t at = (in_b + 15) & ~15ull;
      const uint64_t sb = chunk_sizes[o1] * k;
      if (o1 > o0 && at + sb > kSaveTempGroupBytes) break;
      in_off.push_back(at);
      in_b = at + sb;
      (usable[o1] ? use : rest).push_back(o1);
      ++o1;
    }
    const uint32_t cnt = o1 - o0, nu = (uint32_t)use.size();
    const uint64_t sn_off = (in_b + 15) & ~15ull;
    const uint64_t wn_off = sn_off + 32ull * k * cnt;
    in_b = wn_off + (wit ? 32ull * nu : 0);
    t_off.resize(nu);
    ob_off.resize(nu);
    wo_off.resize(nu);
    uint64_t out_b = 0;
    for (uint32_t u = 0; u < nu; ++u) {
      t_off[u] = out_b;
      out_b = (out_b + need[use[u]] + 15) & ~15ull;
    }
    const uint64_t st_off = out_b;
    const uint64_t gv_off = st_off + 4ull * nu;
    const uint64_t back_b = wit ? gv_off : gv_off + (uint64_t)nu * k;  // what is copied back
    const uint64_t lv_off = (gv_off + (wit ? nu : (uint64_t)nu * k) + 15) & ~15ull;
    out_b = (lv_off + (uint64_t)cnt * k + 15) & ~15ull;
    for (uint32_t u = 0; u < nu; ++u) {
      ob_off[u] = out_b;
      out_b = (out_b + E[use[u]] + 15) & ~15ull;
    }
    for (uint32_t u = 0; wit && u < nu; ++u) {
      wo_off[u] = out_b;
      out_b = (out_b + chunk_sizes[use[u]] + 15) & ~15ull;
    }
    if ((rc = st->reserve(in_b, std::max<uint64_t>(out_b, 16)))) return rc;
    // position of an object's names among the staged ones: usable objects first
    auto names_at = [&](uint32_t pos) { return sn_off + 32ull * k * pos; };
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j)
      for (uint32_t c = 0; c < k; ++c)
        parts.push_back({st->h_in + in_off[j] + c * chunk_sizes[o0 + j], chunks[(uint64_t)(o0 + j) * k + c],
                         chunk_sizes[o0 + j]});
    for (uint32_t u = 0; u < nu; ++u) {
      parts.push_back({st->h_in + names_at(u), survivor_names + 32ull * k * use[u], 32ull * k});
      if (wit) parts.push_back({st->h_in + wn_off + 32ull * u, witness_names + 32ull * use[u], 32});
    }
    for (uint32_t r = 0; r < rest.size(); ++r)
      parts.push_back({st->h_in + names_at(nu + r), survivor_names + 32ull * k * rest[r], 32ull * k});
    parallel_copy(parts);
    hipError_t e = hipMemcpyAsync(st->d_in, st->h_in, in_b, hipMemcpyHostToDevice, st->stream);
    if (e != hipSuccess) return hip_status(e);
    // (an error after the first enqueue drains the stream before returning:
    // the next call on this thread reuses the buffers)
    auto drained = [&](int r) {
      (void)hipStreamSynchronize(st->stream);
      return r;
    };
    auto survivors_of = [&](uint32_t o) {
      for (uint32_t c = 0; c < k; ++c) d_chunks.push_back(st->d_in + in_off[o - o0] + c * chunk_sizes[o]);
    };
    if (nu) {
      d_chunks.clear();
      nd.resize((size_t)nu * k);
      csz.resize(nu);
      pd.resize(nu);
      wid.resize(nu);
      d_objs.resize(nu);
      d_wouts.resize(nu);
      d_texts.resize(nu);
      for (uint32_t u = 0; u < nu; ++u) {
        const uint32_t o = use[u];
        survivors_of(o);
        std::memcpy(nd.data() + (size_t)u * k, nodes + (uint64_t)o * k, sizeof(uint16_t) * k);
        csz[u] = chunk_sizes[o];
        pd[u] = pad[o];
        if (wit) wid[u] = witness_ids[o];
        d_objs[u] = st->d_out + ob_off[u];
        d_wouts[u] = wit ? st->d_out + wo_off[u] : nullptr;
        d_texts[u] = reinterpret_cast<char *>(st->d_out + t_off[u]);
      }
      rc = download_batch_device(k, nu, nd.data(), d_chunks.data(), csz.data(), pd.data(),
                                 wit ? nullptr : st->d_in + sn_off, wit ? wid.data() : nullptr,
                                 wit ? st->d_in + wn_off : nullptr, wit ? d_wouts.data() : nullptr, d_objs.data(),
                                 d_texts.data(), st->d_out + gv_off, reinterpret_cast<int32_t *>(st->d_out + st_off),
                                 st->stream);
      if (rc) return drained(rc);
      e = hipMemcpyAsync(st->h_out, st->d_out, back_b, hipMemcpyDeviceToHost, st->stream);
      if (e != hipSuccess) return drained(hip_status(e));
      if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    }
    // an object whose status is non-zero has no text scattered
    parts.clear();
    locate.clear();
    const int32_t *dst = reinterpret_cast<const int32_t *>(st->h_out + st_off);
    for (uint32_t u = 0; u < nu; ++u) {
      const uint32_t o = use[u];
      statuses[o] = dst[u];
      uint8_t *sv = survivor_verdicts + (uint64_t)o * k;
      if (wit)
        std::memset(sv, 0, k);
      else
        std::memcpy(sv, st->h_out + gv_off + (uint64_t)u * k, k);  // survivor mode: the gate itself
      if (dst[u]) {
        ++bad;
        text_lens[o] = 0;
        if (wit) locate.push_back(u);
        continue;
      }
      if (need[o]) parts.push_back({reinterpret_cast<uint8_t *>(texts[o]), st->h_out + t_off[u], need[o]});
      text_lens[o] = need[o];
    }
    for (uint32_t r = 0; r < rest.size(); ++r) {
      statuses[rest[r]] = wit ? VDS_EC_ECORRUPT : VDS_EC_ERESTORE;
      text_lens[rest[r]] = 0;
      ++bad;
      locate.push_back(nu + r);
    }
    parallel_copy(parts);
    if (!locate.empty()) {
      // The locating pass: the survivors are still on the device, and one
      // more hash launch over the failed objects' survivors alone says which
      // file is rotten.
      const uint32_t nl = (uint32_t)locate.size();
      d_chunks.clear();
      lens.resize(nl);
      d_exp.resize(nl);
      d_ver.resize(nl);
      for (uint32_t f = 0; f < nl; ++f) {
        const uint32_t o = locate[f] < nu ? use[locate[f]] : rest[locate[f] - nu];
        survivors_of(o);
        lens[f] = chunk_sizes[o];
        d_exp[f] = st->d_in + names_at(locate[f]);
        d_ver[f] = st->d_out + lv_off + (uint64_t)f * k;
      }
      rc = sha256_check_groups_device(nl, k, d_chunks.data(), lens.data(), d_exp.data(), d_ver.data(), st->stream);
      if (rc) return drained(rc);
      e = hipMemcpyAsync(st->h_out + lv_off, st->d_out + lv_off, (uint64_t)nl * k, hipMemcpyDeviceToHost,
                         st->stream);
      if (e != hipSuccess) return drained(hip_status(e));
      if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
      for (uint32_t f = 0; f < nl; ++f) {
        const uint32_t o = locate[f] < nu ? use[locate[f]] : rest[locate[f] - nu];
        std::memcpy(survivor_verdicts + (uint64_t)o * k, st->h_out + lv_off + (uint64_t)f * k, k);
      }
    }
    o0 = o1;
  }
  if (failed) *failed = bad;
  return VDS_EC_OK;
}

}  // namespace api
}  // namespace vds_ec

extern "C" {

int vds_ec_base64_encode_gated_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                            char *const *outs, const uint8_t *const *gates, const uint32_t *ngates,
                                            int32_t *statuses, void *stream) {
  return vds_ec::api::base64_encode_gated_batch_device(count, ins, lens, outs, gates, ngates, statuses,
                                                       vds_ec::api::as_stream(stream));
}

int vds_ec_download16_batch_device(uint16_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                                   const uint64_t *chunk_sizes, const uint16_t *paddings,
                                   const uint8_t *survivor_names, const uint16_t *witness_ids,
                                   const uint8_t *witness_names, uint8_t *const *witness_outs,
                                   uint8_t *const *objects, char *const *texts, uint8_t *verdicts, int32_t *statuses,
                                   void *stream) {
  return vds_ec::api::download_batch_device(k, count, nodes, chunks, chunk_sizes, paddings, survivor_names,
                                            witness_ids, witness_names, witness_outs, objects, texts, verdicts,
                                            statuses, vds_ec::api::as_stream(stream));
}

int vds_ec_download16_host_batch(uint16_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                                 const uint64_t *chunk_sizes, const uint8_t *survivor_names,
                                 const uint16_t *witness_ids, const uint8_t *witness_names, char *const *texts,
                                 uint64_t *text_lens, int32_t *statuses, uint8_t *survivor_verdicts,
                                 uint32_t *failed) {
  return vds_ec::api::download_host_batch(k, count, nodes, chunks, chunk_sizes, survivor_names, witness_ids,
                                          witness_names, texts, text_lens, statuses, survivor_verdicts, failed);
}

}  // extern "C"
