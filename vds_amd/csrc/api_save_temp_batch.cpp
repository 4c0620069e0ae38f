// api_save_temp_batch.cpp -- vds_ec_sha256_batch_device, and the batched
// save_temp built on it (vds_ec_save_temp16_batch_device / _host_batch): the
// upload loop's encode AND names for a batch of bodies of different sizes.
// save_temp and save_data name every replica by its SHA-256
// (dht_network_client.cpp:77-79, :591-593) and upload_data hashes the body
// (server_api.cpp:16); here every hash of a call rides ONE k_sha256_batch
// launch (sha256.hip), planned on the host.  The repair loop's batch
// (vds_ec_repair16_batch_device / _host_batch: regenerate, name and check the
// lost replicas; sync_process.cpp:313-335) and vds_ec_sha256_check_batch_device
// ride the same launch in its check mode.
// (api_internal.hpp lists the host runtime's translation units.)
#include "api_internal.hpp"

namespace vds_ec {
namespace api {

namespace {

// The message groups of one call before they are ordered (pointer-table
// addresses still as offsets into `ptrs`).  Kept per thread, so a caller's
// loop allocates nothing after its first call.
struct ShaBatchScratch {
  std::vector<ShaBatchGroup> groups;
  std::vector<uint32_t> m;
  std::vector<const uint8_t *> ptrs;
  std::vector<uint32_t> key, order, bucket;
  std::vector<uint16_t> ids;  // 0..n-1, save_temp's replicas
  // check mode (k_sha256_batch<true>): checks[g] beside groups[g]
  bool check = false;
  std::vector<ShaBatchCheck> checks;
  // gated mode (k_sha256_batch<true, true>): gates[g] beside groups[g] and checks[g]
  bool gated = false;
  std::vector<ShaBatchGate> gates;
  void clear(bool check_mode = false, bool gated_mode = false) {
    groups.clear();
    m.clear();
    ptrs.clear();
    checks.clear();
    gates.clear();
    check = check_mode;
    gated = gated_mode;
  }
  void add(uint64_t msg, uint64_t pitch, uint64_t len, uint8_t *digests, uint32_t cnt,
           const uint8_t *expected = nullptr, uint8_t *verdicts = nullptr) {
    groups.push_back(ShaBatchGroup{msg, pitch, len, reinterpret_cast<uint64_t>(digests)});
    m.push_back(cnt);
    if (check) checks.push_back(ShaBatchCheck{reinterpret_cast<uint64_t>(expected), reinterpret_cast<uint64_t>(verdicts)});
  }
  // m messages through pointers p[0..m): one descriptor when they are equally spaced, else a pointer table
  void add_ptrs(const uint8_t *const *p, uint32_t cnt, uint64_t len, uint8_t *digests,
                const uint8_t *expected = nullptr, uint8_t *verdicts = nullptr) {
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(p[0]);
    const uint64_t pitch = cnt > 1 ? reinterpret_cast<uintptr_t>(p[1]) - p0 : 0;
    bool spaced = pitch != kShaBatchPtrTable;
    for (uint32_t i = 2; spaced && i < cnt; ++i) spaced = reinterpret_cast<uintptr_t>(p[i]) == p0 + i * pitch;
    if (spaced) {
      add(p0, pitch, len, digests, cnt, expected, verdicts);
    } else {
      add(ptrs.size() * sizeof(uint8_t *), kShaBatchPtrTable, len, digests, cnt, expected, verdicts);
      ptrs.insert(ptrs.end(), p, p + cnt);
    }
  }
};

ShaBatchScratch &sha_batch_scratch() {
  thread_local ShaBatchScratch sc;
  return sc;
}

// Lane order: a wave runs as long as its longest chain, so groups go by
// compressions (64-byte blocks, padding included), most first -- the long
// chains set the call's critical path and start at once, and a wave holds
// chains of one length or nearly.  Equal keys keep the caller's order.  A
// counting sort where the block counts are small against the batch (the
// upload loop: 16,384 objects, up to 1025 blocks), else a comparison sort.
void order_groups(ShaBatchScratch &sc) {
  const size_t ng = sc.groups.size();
  sc.key.resize(ng);
  sc.order.resize(ng);
  uint64_t kmax = 0;
  bool wide = false;
  for (size_t g = 0; g < ng; ++g) {
    const uint64_t blocks = (sc.groups[g].len + 8) / 64 + 1;
    wide = wide || blocks > 0xFFFFFFFFull;
    sc.key[g] = (uint32_t)std::min<uint64_t>(blocks, 0xFFFFFFFFull);
    kmax = std::max<uint64_t>(kmax, sc.key[g]);
  }
  if (!wide && kmax <= 4 * ng + 4096) {
    sc.bucket.assign(kmax + 2, 0);
    for (size_t g = 0; g < ng; ++g) ++sc.bucket[kmax - sc.key[g] + 1];
    for (size_t b = 1; b < sc.bucket.size(); ++b) sc.bucket[b] += sc.bucket[b - 1];
    for (size_t g = 0; g < ng; ++g) sc.order[sc.bucket[kmax - sc.key[g]]++] = (uint32_t)g;
  } else {
    for (size_t g = 0; g < ng; ++g) sc.order[g] = (uint32_t)g;
    std::stable_sort(sc.order.begin(), sc.order.end(),
                     [&](uint32_t a, uint32_t b) { return sc.groups[a].len > sc.groups[b].len; });
  }
}

// The tables in one ring slot -- groups, spans, wave_group, pointer tables --
// and the launch.  A group of whole waves (m a multiple of 64: the 64
// replicas of an object) starts on a wave boundary, so one wave is one
// object; the lanes skipped for that belong to no group.  The caller has
// bounded the lanes (sum of m plus 63 a group) below 2^32.
int launch_sha_groups(ShaBatchScratch &sc, hipStream_t s) {
  const size_t ng = sc.groups.size();
  if (ng == 0) return VDS_EC_OK;
  order_groups(sc);
  uint64_t lanes = 0;
  for (size_t i = 0; i < ng; ++i) {
    const uint32_t m = sc.m[sc.order[i]];
    if (m % 64 == 0) lanes = (lanes + 63) & ~63ull;
    lanes += m;
  }
  const uint64_t waves = (lanes + 63) / 64;
  if (waves == 0) return VDS_EC_OK;  // (groups of no messages)
  if (waves > 0x3FFFFFFull) return VDS_EC_EINVAL;
  const size_t o_spans = ng * sizeof(ShaBatchGroup);
  const size_t o_wave = o_spans + ng * sizeof(ShaBatchSpan);
  const size_t o_ptrs = (o_wave + (waves + 1) * sizeof(uint32_t) + 7) & ~size_t(7);
  const size_t o_checks = o_ptrs + sc.ptrs.size() * sizeof(uint8_t *);  // (check mode: after the pointer tables)
  const size_t o_gates = o_checks + (sc.check ? ng * sizeof(ShaBatchCheck) : 0);  // (gated mode: after the checks)
  const size_t bytes = o_gates + (sc.gated ? ng * sizeof(ShaBatchGate) : 0);
  ParamSlot *slot = nullptr;
  hipError_t e = param_acquire_n(1, &bytes, &slot);
  if (e != hipSuccess) return hip_status(e);
  ShaBatchGroup *groups = reinterpret_cast<ShaBatchGroup *>(slot->h);
  ShaBatchSpan *spans = reinterpret_cast<ShaBatchSpan *>(slot->h + o_spans);
  uint32_t *wave_group = reinterpret_cast<uint32_t *>(slot->h + o_wave);
  ShaBatchCheck *checks = reinterpret_cast<ShaBatchCheck *>(slot->h + o_checks);
  ShaBatchGate *gates = reinterpret_cast<ShaBatchGate *>(slot->h + o_gates);
  uint64_t lane = 0;
  for (size_t i = 0; i < ng; ++i) {
    const uint32_t g = sc.order[i];
    ShaBatchGroup d = sc.groups[g];
    if (d.pitch == kShaBatchPtrTable) d.msg += reinterpret_cast<uintptr_t>(slot->d + o_ptrs);
    groups[i] = d;
    if (sc.check) checks[i] = sc.checks[g];
    if (sc.gated) gates[i] = sc.gates[g];
    const uint32_t m = sc.m[g];
    if (m % 64 == 0) lane = (lane + 63) & ~63ull;
    spans[i] = ShaBatchSpan{(uint32_t)lane, m};
    lane += m;
  }
  size_t g = 0;
  for (uint64_t w = 0; w <= waves; ++w) {  // the last group whose first lane is <= 64 w
    while (g + 1 < ng && spans[g + 1].first <= 64 * w) ++g;
    wave_group[w] = (uint32_t)g;
  }
  if (!sc.ptrs.empty()) std::memcpy(slot->h + o_ptrs, sc.ptrs.data(), sc.ptrs.size() * sizeof(uint8_t *));
  e = param_commit(slot, bytes, s);
  if (e == hipSuccess) {
    ShaBatchLaunch b{};
    b.groups = reinterpret_cast<const ShaBatchGroup *>(slot->d);
    b.spans = reinterpret_cast<const ShaBatchSpan *>(slot->d + o_spans);
    b.wave_group = reinterpret_cast<const uint32_t *>(slot->d + o_wave);
    b.waves = (uint32_t)waves;
    if (sc.gated)
      e = launch_sha256_gated_batch(
          ShaBatchGatedLaunch{ShaBatchCheckLaunch{b, reinterpret_cast<const ShaBatchCheck *>(slot->d + o_checks)},
                              reinterpret_cast<const ShaBatchGate *>(slot->d + o_gates)},
          s);
    else if (sc.check)
      e = launch_sha256_check_batch(
          ShaBatchCheckLaunch{b, reinterpret_cast<const ShaBatchCheck *>(slot->d + o_checks)}, s);
    else
      e = launch_sha256_batch(b, s);
  }
  const hipError_t re = param_release(slot, s);  // (its event follows whatever was enqueued)
  return hip_status(e != hipSuccess ? e : re);
}

// save_temp's arguments, checked before the device is looked for.  (n <=
// 65536: the replicas are ids 0..n-1 of GF(2^16).  count (n + 64) < 2^32: the
// hash launch's lanes, a wave-aligned group per object and a body each.)
int check_save_temp_batch(uint32_t k, uint32_t n, uint32_t count, const void *objs, const uint64_t *sizes,
                          const void *outs, const uint8_t *replica_digests) {
  if (k == 0 || n > 65536u || count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count && (!objs || !sizes || (n && (!outs || !replica_digests)))) return VDS_EC_EINVAL;
  if ((uint64_t)count * ((uint64_t)n + 64) > 0xFFFFFFFFull) return VDS_EC_EINVAL;
  return VDS_EC_OK;
}

}  // namespace

int sha256_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens, uint8_t *digests,
                        hipStream_t s) {
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count && (!msgs || !lens || !digests)) return VDS_EC_EINVAL;
  for (uint32_t j = 0; j < count; ++j)
    if (lens[j] && !msgs[j]) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  const int rc = device_ready();
  if (rc) return rc;
  ShaBatchScratch &sc = sha_batch_scratch();
  sc.clear();
  for (uint32_t j = 0; j < count; ++j)
    sc.add(reinterpret_cast<uintptr_t>(msgs[j]), 0, lens[j], digests + 32ull * j, 1);
  return launch_sha_groups(sc, s);
}

int save_temp_batch_device(uint32_t k, uint32_t n, uint32_t count, const uint8_t *const *ins, const uint64_t *sizes,
                           uint8_t *const *outs, uint8_t *replica_digests, uint8_t *data_digests, hipStream_t s) {
  int rc = check_save_temp_batch(k, n, count, ins, sizes, outs, replica_digests);
  if (rc) return rc;
  ShaBatchScratch &sc = sha_batch_scratch();
  if (sc.ids.size() < n) {
    sc.ids.resize(n);
    for (uint32_t i = 0; i < n; ++i) sc.ids[i] = (uint16_t)i;
  }
  // the batched encode's own pass: every object validated and routed
  EncBatchScratch &enc = enc_batch_scratch();
  if ((rc = plan_encode_batch(k, sc.ids.data(), n, count, ins, sizes, outs, 0, enc))) return rc;
  if (count == 0) return VDS_EC_OK;
  if ((rc = device_ready())) return rc;
  if ((rc = encode_batch_run(k, sc.ids.data(), n, count, ins, sizes, outs, 0, enc, s))) return rc;
  // The names: object o's n replicas are one group (what the encode's plan
  // found out about their spacing is reused; the objects that took
  // encode_device are looked at here), its body another of one message.
  sc.clear();
  size_t ie = 0, ir = 0;
  for (uint32_t o = 0; o < count; ++o) {
    const bool rest = ir < enc.rest.size() && enc.rest[ir] == o;
    if (n) {
      const uint64_t L = vds_ec_replica_size(2, k, sizes[o], 0);
      uint8_t *dg = replica_digests + 32ull * o * n;
      if (rest) {
        sc.add_ptrs(outs + (uint64_t)o * n, n, L, dg);
      } else {
        const EncBatchObj &d = enc.objs[ie];
        if (d.pitch != kEncBatchPtrTable) {
          sc.add(d.out, d.pitch, L, dg, n);
        } else {
          sc.add(sc.ptrs.size() * sizeof(uint8_t *), kShaBatchPtrTable, L, dg, n);
          const uint8_t *const *t = enc.ptrs.data() + d.out / sizeof(uint8_t *);
          sc.ptrs.insert(sc.ptrs.end(), t, t + n);
        }
      }
    }
    if (rest)
      ++ir;
    else
      ++ie;
    if (data_digests) sc.add(reinterpret_cast<uintptr_t>(ins[o]), 0, sizes[o], data_digests + 32ull * o, 1);
  }
  return launch_sha_groups(sc, s);
}

// ------------------------------------------------------------ host form
SaveTempStage *save_temp_stage() {
  thread_local std::vector<SaveTempStage *> per_device;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return nullptr;
  if ((size_t)dev >= per_device.size()) per_device.resize(dev + 1, nullptr);
  if (!per_device[dev]) per_device[dev] = new SaveTempStage();
  return per_device[dev];
}

int save_temp_host_batch(uint32_t k, uint32_t n, uint32_t count, const uint8_t *const *objs, const uint64_t *sizes,
                         uint8_t *const *outs, uint8_t *replica_digests, uint8_t *data_digests,
                         uint32_t *replica_sizes) {
  int rc = check_save_temp_batch(k, n, count, objs, sizes, outs, replica_digests);
  if (rc) return rc;
  for (uint32_t o = 0; o < count; ++o) {
    if (sizes[o] && !objs[o]) return VDS_EC_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
      if (!outs[(uint64_t)o * n + i]) return VDS_EC_EINVAL;
  }
  if (count == 0) return VDS_EC_OK;
  if ((rc = device_ready())) return rc;
  SaveTempStage *st = save_temp_stage();
  if (!st) return VDS_EC_ENODEV;
  std::vector<uint64_t> in_off, out_off, L;
  std::vector<const uint8_t *> d_ins;
  std::vector<uint8_t *> d_outs;
  std::vector<Copy> parts;
  for (uint32_t o0 = 0; o0 < count;) {
    // the group: objects o0 .. o1-1, their bodies at 16-byte aligned offsets
    // of the input staging, their replicas back to back in the output
    // staging, then the names and the body hashes
    in_off.clear();
    out_off.clear();
    L.clear();
    uint64_t in_b = 0, out_b = 0;
    uint32_t o1 = o0;
    while (o1 < count && o1 - o0 < kSaveTempGroupObjects) {
      const uint64_t at = (in_b + 15) & ~15ull;
      if (o1 > o0 && at + sizes[o1] > kSaveTempGroupBytes) break;
      in_off.push_back(at);
      in_b = at + sizes[o1];
      L.push_back(vds_ec_replica_size(2, k, sizes[o1], 0));
      out_off.push_back(out_b);
      out_b += L.back() * n;
      ++o1;
    }
    const uint32_t cnt = o1 - o0;
    const uint64_t rd_off = (out_b + 15) & ~15ull;
    const uint64_t dd_off = rd_off + 32ull * cnt * n;
    out_b = dd_off + (data_digests ? 32ull * cnt : 0);
    if ((rc = st->reserve(std::max<uint64_t>(in_b, 64), out_b))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j)
      if (sizes[o0 + j]) parts.push_back({st->h_in + in_off[j], objs[o0 + j], sizes[o0 + j]});
    parallel_copy(parts);
    hipError_t e = in_b ? hipMemcpyAsync(st->d_in, st->h_in, in_b, hipMemcpyHostToDevice, st->stream) : hipSuccess;
    if (e != hipSuccess) return hip_status(e);
    // (an error after the first enqueue drains the stream before returning:
    // the next call on this thread reuses the buffers)
    auto drained = [&](int r) {
      (void)hipStreamSynchronize(st->stream);
      return r;
    };
    d_ins.resize(cnt);
    d_outs.resize((size_t)cnt * n);
    for (uint32_t j = 0; j < cnt; ++j) {
      d_ins[j] = st->d_in + in_off[j];
      for (uint32_t i = 0; i < n; ++i) d_outs[(size_t)j * n + i] = st->d_out + out_off[j] + i * L[j];
    }
    rc = save_temp_batch_device(k, n, cnt, d_ins.data(), sizes + o0, d_outs.data(), st->d_out + rd_off,
                                data_digests ? st->d_out + dd_off : nullptr, st->stream);
    if (rc) return drained(rc);
    if (out_b) e = hipMemcpyAsync(st->h_out, st->d_out, out_b, hipMemcpyDeviceToHost, st->stream);
    if (e != hipSuccess) return drained(hip_status(e));
    if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j) {
      for (uint32_t i = 0; i < n; ++i)
        parts.push_back({outs[(uint64_t)(o0 + j) * n + i], st->h_out + out_off[j] + i * L[j], L[j]});
      if (replica_sizes) replica_sizes[o0 + j] = (uint32_t)L[j];
    }
    if (n) parts.push_back({replica_digests + 32ull * o0 * n, st->h_out + rd_off, 32ull * cnt * n});
    if (data_digests) parts.push_back({data_digests + 32ull * o0, st->h_out + dd_off, 32ull * cnt});
    parallel_copy(parts);
    o0 = o1;
  }
  return VDS_EC_OK;
}

// ------------------------------------------------------------ check and repair
int sha256_check_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens,
                              const uint8_t *expected, uint8_t *digests, uint8_t *verdicts, hipStream_t s) {
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count && (!msgs || !lens || !expected || !verdicts)) return VDS_EC_EINVAL;
  for (uint32_t j = 0; j < count; ++j)
    if (lens[j] && !msgs[j]) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  const int rc = device_ready();
  if (rc) return rc;
  ShaBatchScratch &sc = sha_batch_scratch();
  sc.clear(true);
  for (uint32_t j = 0; j < count; ++j)
    sc.add(reinterpret_cast<uintptr_t>(msgs[j]), 0, lens[j], digests ? digests + 32ull * j : nullptr, 1,
           expected + 32ull * j, verdicts + j);
  return launch_sha_groups(sc, s);
}

int sha256_gated_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *caps,
                              const uint8_t *expected, uint32_t *lens_dev, int32_t *statuses, hipStream_t s) {
  ShaBatchScratch &sc = sha_batch_scratch();
  sc.clear(true, true);
  for (uint32_t j = 0; j < count; ++j) {
    // (ordered by the capacity, the length's upper bound: the length itself is on the device)
    sc.add(reinterpret_cast<uintptr_t>(msgs[j]), 0, caps[j], nullptr, 1, expected + 32ull * j, nullptr);
    sc.gates.push_back(ShaBatchGate{reinterpret_cast<uintptr_t>(lens_dev + j), reinterpret_cast<uintptr_t>(statuses + j)});
  }
  return launch_sha_groups(sc, s);
}

// Check only, group by group (the download loop's second pass, over the
// survivors of the objects that failed): group g is the m messages
// msgs[g*m + i] of lens[g] bytes each, compared with expected[g] + 32 i into
// verdicts[g] + i.  One launch.  The caller has validated the arguments and
// found the device.
int sha256_check_groups_device(uint32_t ngroups, uint32_t m, const uint8_t *const *msgs, const uint64_t *lens,
                               const uint8_t *const *expected, uint8_t *const *verdicts, hipStream_t s) {
  if (ngroups == 0 || m == 0) return VDS_EC_OK;
  if ((uint64_t)ngroups * ((uint64_t)m + 64) > 0xFFFFFFFFull) return VDS_EC_EINVAL;
  ShaBatchScratch &sc = sha_batch_scratch();
  sc.clear(true);
  for (uint32_t g = 0; g < ngroups; ++g) sc.add_ptrs(msgs + (uint64_t)g * m, m, lens[g], nullptr, expected[g], verdicts[g]);
  return launch_sha_groups(sc, s);
}

namespace {

// What the repair entry points check beyond vds_ec_regenerate16_batch_device
// (whose own first checks these repeat, so that nothing of the names is
// judged for a call that regenerate would reject outright).  *empty: the call
// has nothing to do.  (count (nt + 64) < 2^32: the hash launch's lanes, one
// group per object, wave-aligned when nt is a multiple of 64.)
int check_repair_batch(uint32_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                       const uint64_t *chunk_sizes, uint32_t nt, const uint16_t *targets, uint8_t *const *outs,
                       const uint8_t *digests, const uint8_t *expected, const uint8_t *verdicts, bool *empty) {
  *empty = false;
  if (k == 0 || (count && (!nodes || !chunks || !chunk_sizes || (nt && (!targets || !outs))))) return VDS_EC_EINVAL;
  if (count == 0 || nt == 0) {
    *empty = true;
    return VDS_EC_OK;
  }
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (!digests || (expected == nullptr) != (verdicts == nullptr)) return VDS_EC_EINVAL;
  if ((uint64_t)count * ((uint64_t)nt + 64) > 0xFFFFFFFFull) return VDS_EC_EINVAL;
  return VDS_EC_OK;
}

// The one hash launch after the regenerate: object o's nt replicas are one group.
int repair_names(uint32_t count, const uint64_t *chunk_sizes, uint32_t nt, uint8_t *const *outs, uint8_t *digests,
                 const uint8_t *expected, uint8_t *verdicts, hipStream_t s) {
  ShaBatchScratch &sc = sha_batch_scratch();
  sc.clear(expected != nullptr);
  for (uint32_t o = 0; o < count; ++o) {
    const uint64_t at = (uint64_t)o * nt;
    sc.add_ptrs(outs + at, nt, chunk_sizes[o], digests + 32 * at, expected ? expected + 32 * at : nullptr,
                verdicts ? verdicts + at : nullptr);
  }
  return launch_sha_groups(sc, s);
}

}  // namespace

int repair_batch_device(uint32_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                        const uint64_t *chunk_sizes, uint32_t nt, const uint16_t *targets, uint8_t *const *outs,
                        uint8_t *digests, const uint8_t *expected, uint8_t *verdicts, hipStream_t s) {
  bool empty;
  int rc = check_repair_batch(k, count, nodes, chunks, chunk_sizes, nt, targets, outs, digests, expected, verdicts,
                              &empty);
  if (rc || empty) return rc;
  // (every object validated, then the device looked for, then the launches)
  if ((rc = regenerate_batch_device(k, count, nodes, chunks, chunk_sizes, nt, targets, outs, s))) return rc;
  return repair_names(count, chunk_sizes, nt, outs, digests, expected, verdicts, s);
}

int repair_host_batch(uint32_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                      const uint64_t *chunk_sizes, uint32_t nt, const uint16_t *targets, uint8_t *const *outs,
                      uint8_t *digests, const uint8_t *expected, uint8_t *verdicts, uint32_t *mismatches) {
  bool empty;
  int rc = check_repair_batch(k, count, nodes, chunks, chunk_sizes, nt, targets, outs, digests, expected, verdicts,
                              &empty);
  if (rc) return rc;
  if (mismatches) *mismatches = 0;
  if (empty) return VDS_EC_OK;
  // Every object as vds_ec_regenerate16_batch_device checks it, and -- the
  // host has the trailers -- as vds_ec_regenerate16_host does: the reference
  // route restores with the first chunk's trailer p (chunk.h:408), and p > 2k
  // has no chunk_size-byte answer.
  for (uint32_t o = 0; o < count; ++o) {
    const uint64_t cs = chunk_sizes[o];
    if (cs < 2 || (cs - 2) % 2) return VDS_EC_EINVAL;
    for (uint32_t j = 0; j < k; ++j)
      if (!chunks[(uint64_t)o * k + j]) return VDS_EC_EINVAL;
    for (uint32_t i = 0; i < nt; ++i)
      if (!outs[(uint64_t)o * nt + i]) return VDS_EC_EINVAL;
    if (!ids_distinct(k, nodes + (uint64_t)o * k)) return VDS_EC_ESINGULAR;
    const uint8_t *c0 = chunks[(uint64_t)o * k];
    const uint16_t p = (uint16_t)((c0[cs - 2] << 8) | c0[cs - 1]);
    bool ok = true;
    (void)restored_len(2, k, cs, p, 0, &ok);
    if (!ok || p > 2 * k) return VDS_EC_ERESTORE;
  }
  if ((rc = device_ready())) return rc;
  SaveTempStage *st = save_temp_stage();
  if (!st) return VDS_EC_ENODEV;
  std::vector<uint64_t> in_off, out_off;
  std::vector<const uint8_t *> d_chunks;
  std::vector<uint8_t *> d_outs;
  std::vector<Copy> parts;
  uint32_t bad = 0;
  for (uint32_t o0 = 0; o0 < count;) {
    // the group: objects o0 .. o1-1, each object's k survivors back to back
    // from a 16-byte aligned offset of the input staging, then the expected
    // names; its nt replicas back to back in the output staging, then the
    // names and the verdicts
    in_off.clear();
    out_off.clear();
    uint64_t in_b = 0, out_b = 0;
    uint32_t o1 = o0;
    while (o1 < count && o1 - o0 < kSaveTempGroupObjects) {
      const uint64_t at = (in_b + 15) & ~15ull;
      const uint64_t sb = chunk_sizes[o1] * k;
      if (o1 > o0 && at + sb > kSaveTempGroupBytes) break;
      in_off.push_back(at);
      in_b = at + sb;
      out_off.push_back(out_b);
      out_b += chunk_sizes[o1] * nt;
      ++o1;
    }
    const uint32_t cnt = o1 - o0;
    const uint64_t names = (uint64_t)cnt * nt;
    const uint64_t ex_off = (in_b + 15) & ~15ull;
    if (expected) in_b = ex_off + 32 * names;
    const uint64_t dg_off = (out_b + 15) & ~15ull;
    const uint64_t vd_off = dg_off + 32 * names;
    out_b = vd_off + (expected ? names : 0);
    if ((rc = st->reserve(in_b, out_b))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j)
      for (uint32_t c = 0; c < k; ++c)
        parts.push_back({st->h_in + in_off[j] + c * chunk_sizes[o0 + j], chunks[(uint64_t)(o0 + j) * k + c],
                         chunk_sizes[o0 + j]});
    if (expected) parts.push_back({st->h_in + ex_off, expected + 32ull * o0 * nt, 32 * names});
    parallel_copy(parts);
    hipError_t e = hipMemcpyAsync(st->d_in, st->h_in, in_b, hipMemcpyHostToDevice, st->stream);
    if (e != hipSuccess) return hip_status(e);
    // (an error after the first enqueue drains the stream before returning:
    // the next call on this thread reuses the buffers)
    auto drained = [&](int r) {
      (void)hipStreamSynchronize(st->stream);
      return r;
    };
    d_chunks.resize((size_t)cnt * k);
    d_outs.resize((size_t)cnt * nt);
    for (uint32_t j = 0; j < cnt; ++j) {
      for (uint32_t c = 0; c < k; ++c) d_chunks[(size_t)j * k + c] = st->d_in + in_off[j] + c * chunk_sizes[o0 + j];
      for (uint32_t i = 0; i < nt; ++i) d_outs[(size_t)j * nt + i] = st->d_out + out_off[j] + i * chunk_sizes[o0 + j];
    }
    rc = repair_batch_device(k, cnt, nodes + (uint64_t)o0 * k, d_chunks.data(), chunk_sizes + o0, nt,
                             targets + (uint64_t)o0 * nt, d_outs.data(), st->d_out + dg_off,
                             expected ? st->d_in + ex_off : nullptr, expected ? st->d_out + vd_off : nullptr,
                             st->stream);
    if (rc) return drained(rc);
    e = hipMemcpyAsync(st->h_out, st->d_out, out_b, hipMemcpyDeviceToHost, st->stream);
    if (e != hipSuccess) return drained(hip_status(e));
    if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j)
      for (uint32_t i = 0; i < nt; ++i)
        parts.push_back({outs[(uint64_t)(o0 + j) * nt + i], st->h_out + out_off[j] + i * chunk_sizes[o0 + j],
                         chunk_sizes[o0 + j]});
    parts.push_back({digests + 32ull * o0 * nt, st->h_out + dg_off, 32 * names});
    if (expected) {
      parts.push_back({verdicts + (uint64_t)o0 * nt, st->h_out + vd_off, names});
      for (uint64_t i = 0; i < names; ++i) bad += st->h_out[vd_off + i] != 0;
    }
    parallel_copy(parts);
    o0 = o1;
  }
  if (mismatches) *mismatches = bad;
  return VDS_EC_OK;
}

}  // namespace api
}  // namespace vds_ec

extern "C" {

int vds_ec_sha256_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens, uint8_t *digests,
                               void *stream) {
  return vds_ec::api::sha256_batch_device(count, msgs, lens, digests, vds_ec::api::as_stream(stream));
}

int vds_ec_save_temp16_batch_device(uint16_t k, uint32_t n, uint32_t count, const uint8_t *const *ins,
                                    const uint64_t *sizes, uint8_t *const *outs, uint8_t *replica_digests,
                                    uint8_t *data_digests, void *stream) {
  return vds_ec::api::save_temp_batch_device(k, n, count, ins, sizes, outs, replica_digests, data_digests,
                                             vds_ec::api::as_stream(stream));
}

int vds_ec_save_temp16_host_batch(uint16_t k, uint32_t n, uint32_t count, const uint8_t *const *objs,
                                  const uint64_t *sizes, uint8_t *const *outs, uint8_t *replica_digests,
                                  uint8_t *data_digests, uint32_t *replica_sizes) {
  return vds_ec::api::save_temp_host_batch(k, n, count, objs, sizes, outs, replica_digests, data_digests,
                                           replica_sizes);
}

int vds_ec_sha256_check_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens,
                                     const uint8_t *expected, uint8_t *digests, uint8_t *verdicts, void *stream) {
  return vds_ec::api::sha256_check_batch_device(count, msgs, lens, expected, digests, verdicts,
                                                vds_ec::api::as_stream(stream));
}

int vds_ec_repair16_batch_device(uint16_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                                 const uint64_t *chunk_sizes, uint32_t ntargets, const uint16_t *targets,
                                 uint8_t *const *outs, uint8_t *digests, const uint8_t *expected, uint8_t *verdicts,
                                 void *stream) {
  return vds_ec::api::repair_batch_device(k, count, nodes, chunks, chunk_sizes, ntargets, targets, outs, digests,
                                          expected, verdicts, vds_ec::api::as_stream(stream));
}

int vds_ec_repair16_host_batch(uint16_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                               const uint64_t *chunk_sizes, uint32_t ntargets, const uint16_t *targets,
                               uint8_t *const *outs, uint8_t *digests, const uint8_t *expected, uint8_t *verdicts,
                               uint32_t *mismatches) {
  return vds_ec::api::repair_host_batch(k, count, nodes, chunks, chunk_sizes, ntargets, targets, outs, digests,
                                        expected, verdicts, mismatches);
}

}  // extern "C"
