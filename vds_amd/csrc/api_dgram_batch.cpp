// api_dgram_batch.cpp -- the node-to-node datagram layer for a batch
// (dgram.hip): vds_ec_hmac_sha256_batch_device, vds_ec_dgram_seal_batch_device,
// vds_ec_dgram_open_batch_device and the host forms built on them.
//
// dht_datagram_protocol::prepare_to_send (impl/dht_datagram_protocol.cpp:335-541)
// cuts a message into datagrams and signs each with HMAC-SHA256 under the
// session key; process_datagram (:108-193) verifies one, and
// continue_process_messages (:544-769) stitches verified payloads together.
// Here a ragged batch of messages is sealed in one launch and a drained socket
// batch opened in one launch; the planning (which datagram belongs where) is
// host arithmetic on headers, and a message is handed out only when every
// datagram that planned it verified.
// The sessions' key pads are hashed on the host, two compressions a session,
// and ride the parameter ring beside the lane tables (HmacKeyState).
// (api_internal.hpp lists the host runtime's translation units.)
#include "api_internal.hpp"

namespace vds_ec {
namespace api {

namespace {

constexpr uint32_t kKeyBytes = 32;            // the session key (udp_transport.cpp:275-276)
constexpr uint64_t kMaxHmacLen = 1ull << 30;  // the lanes count bytes in 32 bits, signed
constexpr uint64_t kMaxLanes = 1ull << 31;

void fill_keys(HmacKeyState *ks, const uint8_t *keys, uint32_t nsessions) {
  for (uint32_t s = 0; s < nsessions; ++s)
    hmac_sha256_host_midstates(keys + (size_t)kKeyBytes * s, kKeyBytes, ks[s].inner, ks[s].outer);
}

// order[] = the lanes by compressions, most first (a wave runs as long as its
// longest chain); equal counts keep the caller's order.  A counting sort where
// the block counts are small against the batch, else a comparison sort.
template <typename Len>
void order_by_blocks(uint32_t count, const Len *lens, std::vector<uint32_t> &order, std::vector<uint32_t> &bucket) {
  order.resize(count);
  uint64_t kmax = 0;
  for (uint32_t j = 0; j < count; ++j) kmax = std::max<uint64_t>(kmax, ((uint64_t)lens[j] + 8) / 64);
  if (kmax <= 4ull * count + 4096) {
    bucket.assign(kmax + 2, 0);
    for (uint32_t j = 0; j < count; ++j) ++bucket[kmax - ((uint64_t)lens[j] + 8) / 64 + 1];
    for (size_t b = 1; b < bucket.size(); ++b) bucket[b] += bucket[b - 1];
    for (uint32_t j = 0; j < count; ++j) order[bucket[kmax - ((uint64_t)lens[j] + 8) / 64]++] = j;
  } else {
    for (uint32_t j = 0; j < count; ++j) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
  }
}

struct DgramScratch {
  std::vector<uint32_t> order, bucket, counts;
};
DgramScratch &dgram_scratch() {
  thread_local DgramScratch sc;
  return sc;
}

int check_sessions(uint32_t count, const uint32_t *session_of, const uint8_t *keys, uint32_t nsessions) {
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count && (!session_of || !keys || nsessions == 0)) return VDS_EC_EINVAL;
  for (uint32_t j = 0; j < count; ++j)
    if (session_of[j] >= nsessions) return VDS_EC_EINVAL;
  return VDS_EC_OK;
}

// The ring slot of the HMAC and open launches: key states, then the lanes.
int launch_lanes(uint32_t count, uint32_t nsessions, const uint8_t *keys, hipStream_t s,
                 const std::function<void(HmacLane *)> &fill,
                 const std::function<hipError_t(const HmacKeyState *, const HmacLane *)> &launch) {
  const size_t o_lanes = (size_t)nsessions * sizeof(HmacKeyState);
  const size_t bytes = o_lanes + (size_t)count * sizeof(HmacLane);
  ParamSlot *slot = nullptr;
  hipError_t e = param_acquire_n(1, &bytes, &slot);
  if (e != hipSuccess) return hip_status(e);
  fill_keys(reinterpret_cast<HmacKeyState *>(slot->h), keys, nsessions);
  fill(reinterpret_cast<HmacLane *>(slot->h + o_lanes));
  e = param_commit(slot, bytes, s);
  if (e == hipSuccess)
    e = launch(reinterpret_cast<const HmacKeyState *>(slot->d), reinterpret_cast<const HmacLane *>(slot->d + o_lanes));
  const hipError_t re = param_release(slot, s);  // (its event follows whatever was enqueued)
  return hip_status(e != hipSuccess ? e : re);
}

}  // namespace

int hmac_sha256_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens,
                             const uint32_t *session_of, const uint8_t *keys, uint32_t nsessions, uint8_t *macs,
                             const uint8_t *expected, uint8_t *verdicts, hipStream_t s) {
  int rc = check_sessions(count, session_of, keys, nsessions);
  if (rc) return rc;
  if (count && (!msgs || !lens || (expected == nullptr) != (verdicts == nullptr) || (!macs && !expected)))
    return VDS_EC_EINVAL;
  for (uint32_t j = 0; j < count; ++j)
    if ((lens[j] && !msgs[j]) || lens[j] > kMaxHmacLen) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  if ((rc = device_ready())) return rc;
  DgramScratch &sc = dgram_scratch();
  order_by_blocks(count, lens, sc.order, sc.bucket);
  return launch_lanes(
      count, nsessions, keys, s,
      [&](HmacLane *lanes) {
        for (uint32_t i = 0; i < count; ++i) {
          const uint32_t j = sc.order[i];
          lanes[i] = HmacLane{reinterpret_cast<uintptr_t>(msgs[j]), 0, (uint32_t)lens[j], 0, session_of[j], j};
        }
      },
      [&](const HmacKeyState *ks, const HmacLane *lanes) {
        return launch_hmac_sha256_batch(
            HmacBatchLaunch{lanes, ks, count, reinterpret_cast<uintptr_t>(macs), reinterpret_cast<uintptr_t>(expected),
                            reinterpret_cast<uintptr_t>(verdicts)},
            s);
      });
}

namespace {

// Every message of a seal checked, its datagram count into counts[o]; *lanes
// their sum.  pitch == 0: each message's pitch is its own mtu (the host form).
int check_seal(uint32_t count, const uint8_t *const *msgs, const uint64_t *msg_lens, const uint8_t *types,
               const uint32_t *index0, const uint8_t *const *routes, const uint32_t *route_lens,
               const uint32_t *session_of, const uint8_t *keys, const uint32_t *mtus, uint32_t nsessions,
               const void *outs, uint64_t pitch, std::vector<uint32_t> &counts, uint64_t *lanes) {
  int rc = check_sessions(count, session_of, keys, nsessions);
  if (rc) return rc;
  if (count && (!msgs || !msg_lens || !types || !index0 || !route_lens || !mtus || !outs)) return VDS_EC_EINVAL;
  if (pitch > 0xFFFFFFFFull) return VDS_EC_EINVAL;
  counts.resize(count);
  uint64_t total = 0;
  for (uint32_t o = 0; o < count; ++o) {
    if (types[o] >= 32 || (msg_lens[o] && !msgs[o])) return VDS_EC_EINVAL;
    if (route_lens[o] && (!routes || !routes[o])) return VDS_EC_EINVAL;
    if (vds_ec_dgram_layout(mtus[o], route_lens[o], msg_lens[o], &counts[o], nullptr, nullptr)) return VDS_EC_EINVAL;
    if (pitch && pitch < mtus[o]) return VDS_EC_EINVAL;
    if ((uint64_t)index0[o] + counts[o] > (1ull << 32)) return VDS_EC_EINVAL;  // "Overflow pipeline"
    total += counts[o];
  }
  if (total >= kMaxLanes) return VDS_EC_EINVAL;
  *lanes = total;
  return VDS_EC_OK;
}

// The seal's tables in one ring slot -- key states, messages, wave_msg -- and
// the launch.  The arguments are checked and the device is ready.
int seal_run(uint32_t count, const uint8_t *const *msgs, const uint64_t *msg_lens, const uint8_t *types,
             const uint32_t *index0, const uint8_t *const *routes, const uint32_t *route_lens,
             const uint32_t *session_of, const uint8_t *keys, const uint32_t *mtus, uint32_t nsessions,
             uint8_t *const *outs, uint64_t pitch, const std::vector<uint32_t> &counts, uint64_t lanes,
             hipStream_t s) {
  if (lanes == 0) return VDS_EC_OK;
  const uint64_t waves = (lanes + 63) / 64;
  const size_t o_msgs = (size_t)nsessions * sizeof(HmacKeyState);
  const size_t o_wave = o_msgs + (size_t)count * sizeof(DgramSealMsg);
  const size_t bytes = o_wave + (waves + 1) * sizeof(uint32_t);
  ParamSlot *slot = nullptr;
  hipError_t e = param_acquire_n(1, &bytes, &slot);
  if (e != hipSuccess) return hip_status(e);
  fill_keys(reinterpret_cast<HmacKeyState *>(slot->h), keys, nsessions);
  DgramSealMsg *dm = reinterpret_cast<DgramSealMsg *>(slot->h + o_msgs);
  uint32_t *wave_msg = reinterpret_cast<uint32_t *>(slot->h + o_wave);
  uint64_t lane = 0, w = 0;
  for (uint32_t o = 0; o < count; ++o) {
    dm[o] = DgramSealMsg{reinterpret_cast<uintptr_t>(msgs[o]),
                         route_lens[o] ? reinterpret_cast<uintptr_t>(routes[o]) : 0,
                         reinterpret_cast<uintptr_t>(outs[o]),
                         (uint32_t)msg_lens[o],
                         index0[o],
                         route_lens[o],
                         mtus[o],
                         (uint32_t)(pitch ? pitch : mtus[o]),
                         session_of[o],
                         (uint32_t)lane,
                         types[o]};
    lane += counts[o];
    for (; w <= waves && 64 * w < lane; ++w) wave_msg[w] = o;  // the message that owns lane 64 w
  }
  for (; w <= waves; ++w) wave_msg[w] = count - 1;
  e = param_commit(slot, bytes, s);
  if (e == hipSuccess)
    e = launch_dgram_seal(DgramSealLaunch{reinterpret_cast<const DgramSealMsg *>(slot->d + o_msgs),
                                          reinterpret_cast<const HmacKeyState *>(slot->d),
                                          reinterpret_cast<const uint32_t *>(slot->d + o_wave), (uint32_t)lanes},
                          s);
  const hipError_t re = param_release(slot, s);
  return hip_status(e != hipSuccess ? e : re);
}

}  // namespace

int dgram_seal_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *msg_lens,
                            const uint8_t *types, const uint32_t *index0, const uint8_t *const *routes,
                            const uint32_t *route_lens, const uint32_t *session_of, const uint8_t *keys,
                            const uint32_t *mtus, uint32_t nsessions, uint8_t *const *outs, uint64_t pitch,
                            hipStream_t s) {
  DgramScratch &sc = dgram_scratch();
  uint64_t lanes = 0;
  int rc = pitch == 0 && count ? VDS_EC_EINVAL
                               : check_seal(count, msgs, msg_lens, types, index0, routes, route_lens, session_of, keys,
                                            mtus, nsessions, outs, pitch, sc.counts, &lanes);
  if (rc) return rc;
  for (uint32_t o = 0; o < count; ++o)
    if (!outs[o]) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  if ((rc = device_ready())) return rc;
  return seal_run(count, msgs, msg_lens, types, index0, routes, route_lens, session_of, keys, mtus, nsessions, outs,
                  pitch, sc.counts, lanes, s);
}

namespace {

int check_open(uint32_t count, const uint8_t *const *dgrams, const uint32_t *lens, const uint32_t *hdr_lens,
               const uint32_t *session_of, const uint8_t *keys, uint32_t nsessions, const uint8_t *verdicts) {
  int rc = check_sessions(count, session_of, keys, nsessions);
  if (rc) return rc;
  if (count && (!dgrams || !lens || !hdr_lens || !verdicts)) return VDS_EC_EINVAL;
  for (uint32_t j = 0; j < count; ++j) {
    if ((lens[j] && !dgrams[j]) || lens[j] > 65535u) return VDS_EC_EINVAL;
    if (lens[j] >= 33 && hdr_lens[j] > lens[j] - 32) return VDS_EC_EINVAL;
  }
  return VDS_EC_OK;
}

}  // namespace

int dgram_open_batch_device(uint32_t count, const uint8_t *const *dgrams, const uint32_t *lens,
                            const uint32_t *hdr_lens, const uint32_t *session_of, const uint8_t *keys,
                            uint32_t nsessions, uint8_t *const *dsts, uint8_t *verdicts, hipStream_t s) {
  int rc = check_open(count, dgrams, lens, hdr_lens, session_of, keys, nsessions, verdicts);
  if (rc) return rc;
  if (count == 0) return VDS_EC_OK;
  if ((rc = device_ready())) return rc;
  DgramScratch &sc = dgram_scratch();
  order_by_blocks(count, lens, sc.order, sc.bucket);
  return launch_lanes(
      count, nsessions, keys, s,
      [&](HmacLane *lanes) {
        for (uint32_t i = 0; i < count; ++i) {
          const uint32_t j = sc.order[i];
          lanes[i] = HmacLane{reinterpret_cast<uintptr_t>(dgrams[j]), dsts ? reinterpret_cast<uintptr_t>(dsts[j]) : 0,
                              lens[j], hdr_lens[j], session_of[j], j};
        }
      },
      [&](const HmacKeyState *ks, const HmacLane *lanes) {
        // (VDS_EC_DGRAM_COPY=lane: the one-lane-per-datagram copy, kept for the A/B of DESIGN.md 6)
        const char *mode = std::getenv("VDS_EC_DGRAM_COPY");
        return launch_dgram_open(DgramOpenLaunch{lanes, ks, count, reinterpret_cast<uintptr_t>(verdicts)}, s,
                                 mode && mode[0] == 'l');
      });
}

// ------------------------------------------------------------ host forms
int dgram_seal_host_batch(uint32_t count, const uint8_t *const *msgs, const uint64_t *msg_lens, const uint8_t *types,
                          const uint32_t *index0, const uint8_t *const *routes, const uint32_t *route_lens,
                          const uint32_t *session_of, const uint8_t *keys, const uint32_t *mtus, uint32_t nsessions,
                          uint8_t *slab, uint64_t slab_bytes, uint64_t *offsets, uint32_t *dgram_counts,
                          uint32_t *last_lens) {
  std::vector<uint32_t> counts;
  uint64_t lanes = 0;
  int rc = check_seal(count, msgs, msg_lens, types, index0, routes, route_lens, session_of, keys, mtus, nsessions,
                      slab, 0, counts, &lanes);
  if (rc) return rc;
  if (count && (!offsets || !dgram_counts || !last_lens)) return VDS_EC_EINVAL;
  // message o's datagrams lie back to back (all but its last are mtu bytes) from offsets[o]
  uint64_t need = 0;
  for (uint32_t o = 0; o < count; ++o) {
    uint32_t last = 0;
    (void)vds_ec_dgram_layout(mtus[o], route_lens[o], msg_lens[o], nullptr, nullptr, &last);
    offsets[o] = need;
    dgram_counts[o] = counts[o];
    last_lens[o] = last;
    need += (uint64_t)(counts[o] - 1) * mtus[o] + last;
  }
  if (need > slab_bytes) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  if ((rc = device_ready())) return rc;
  SaveTempStage *st = save_temp_stage();
  if (!st) return VDS_EC_ENODEV;
  std::vector<uint64_t> m_off, r_off;
  std::vector<const uint8_t *> d_msgs, d_routes;
  std::vector<uint8_t *> d_outs;
  std::vector<uint32_t> cnts;
  std::vector<Copy> parts;
  for (uint32_t o0 = 0; o0 < count;) {
    // the group: messages o0 .. o1-1 and their routes at 16-byte aligned
    // offsets of the input staging; the output staging mirrors the slab
    m_off.clear();
    r_off.clear();
    uint64_t in_b = 0, glanes = 0;
    uint32_t o1 = o0;
    while (o1 < count && o1 - o0 < kSaveTempGroupObjects) {
      const uint64_t at = (in_b + 15) & ~15ull;
      const uint64_t rt = (at + msg_lens[o1] + 15) & ~15ull;
      if (o1 > o0 && rt + route_lens[o1] > kSaveTempGroupBytes) break;
      m_off.push_back(at);
      r_off.push_back(rt);
      in_b = rt + route_lens[o1];
      glanes += counts[o1];
      ++o1;
    }
    const uint32_t cnt = o1 - o0;
    const uint64_t out0 = offsets[o0];
    const uint64_t out_b = (o1 < count ? offsets[o1] : need) - out0;
    if ((rc = st->reserve(std::max<uint64_t>(in_b, 64), std::max<uint64_t>(out_b, 64)))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j) {
      if (msg_lens[o0 + j]) parts.push_back({st->h_in + m_off[j], msgs[o0 + j], msg_lens[o0 + j]});
      if (route_lens[o0 + j]) parts.push_back({st->h_in + r_off[j], routes[o0 + j], route_lens[o0 + j]});
    }
    parallel_copy(parts);
    hipError_t e = in_b ? hipMemcpyAsync(st->d_in, st->h_in, in_b, hipMemcpyHostToDevice, st->stream) : hipSuccess;
    if (e != hipSuccess) return hip_status(e);
    auto drained = [&](int r) {
      (void)hipStreamSynchronize(st->stream);
      return r;
    };
    d_msgs.resize(cnt);
    d_routes.resize(cnt);
    d_outs.resize(cnt);
    cnts.assign(counts.begin() + o0, counts.begin() + o1);
    for (uint32_t j = 0; j < cnt; ++j) {
      d_msgs[j] = st->d_in + m_off[j];
      d_routes[j] = st->d_in + r_off[j];
      d_outs[j] = st->d_out + (offsets[o0 + j] - out0);
    }
    rc = seal_run(cnt, d_msgs.data(), msg_lens + o0, types + o0, index0 + o0, d_routes.data(), route_lens + o0,
                  session_of + o0, keys, mtus + o0, nsessions, d_outs.data(), 0, cnts, glanes, st->stream);
    if (rc) return drained(rc);
    e = hipMemcpyAsync(st->h_out, st->d_out, out_b, hipMemcpyDeviceToHost, st->stream);
    if (e != hipSuccess) return drained(hip_status(e));
    if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    parts.clear();
    parts.push_back({slab + out0, st->h_out, out_b});
    parallel_copy(parts);
    o0 = o1;
  }
  return VDS_EC_OK;
}

namespace {

inline uint32_t be32(const uint8_t *p) {
  return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}

struct OpenEntry {  // a signed datagram whose first byte names a kind, by (session, index, arrival)
  uint32_t session, index, j;
};
struct OpenPlan {  // a message found at a first datagram
  uint32_t first_part, nparts;  // its datagrams, in order: parts[first_part ..)
  uint32_t session, index0, type, hdr, route_len;
  uint64_t len;   // bytes its datagrams carry (complete: the announced size)
  int32_t status;  // as planned from the headers: OK (complete), INCOMPLETE, DATA
};

}  // namespace

int dgram_open_host_batch(uint32_t count, const uint8_t *const *dgrams, const uint32_t *lens,
                          const uint32_t *session_of, const uint8_t *keys, uint32_t nsessions, uint8_t *verdicts,
                          uint8_t *slab, uint64_t slab_bytes, vds_ec_dgram_message *messages, uint32_t *nmessages) {
  int rc = check_sessions(count, session_of, keys, nsessions);
  if (rc) return rc;
  if (!nmessages || (count && (!dgrams || !lens || !verdicts || !messages))) return VDS_EC_EINVAL;
  for (uint32_t j = 0; j < count; ++j)
    if ((lens[j] && !dgrams[j]) || lens[j] > 65535u) return VDS_EC_EINVAL;
  *nmessages = 0;
  if (count == 0) return VDS_EC_OK;

  // ---- plan from the (not yet authenticated) headers
  std::vector<OpenEntry> ent;
  for (uint32_t j = 0; j < count; ++j) {
    if (lens[j] < 33) continue;
    const uint8_t b = dgrams[j][0];
    if (b == 6 || b == 7) continue;  // MTUTest, Acknowledgment
    const uint8_t top = b & 0xE0;
    if ((top >= 0x20 && top <= 0xC0) || b == 0x03) ent.push_back({session_of[j], be32(dgrams[j] + 1), j});
  }
  std::sort(ent.begin(), ent.end(), [](const OpenEntry &a, const OpenEntry &b) {
    return a.session != b.session ? a.session < b.session : a.index != b.index ? a.index < b.index : a.j < b.j;
  });
  // the first arrival of an index wins (process_datagram, :172-186)
  auto same_index = [](const OpenEntry &a, const OpenEntry &b) { return a.session == b.session && a.index == b.index; };
  ent.erase(std::unique(ent.begin(), ent.end(), same_index), ent.end());
  auto find = [&](uint32_t session, uint32_t index) -> const OpenEntry * {
    auto before = [](const OpenEntry &a, const OpenEntry &b) {
      return a.session != b.session ? a.session < b.session : a.index < b.index;
    };
    auto it = std::lower_bound(ent.begin(), ent.end(), OpenEntry{session, index, 0}, before);
    return it != ent.end() && it->session == session && it->index == index ? &*it : nullptr;
  };
  std::vector<OpenPlan> plans;
  std::vector<uint32_t> parts;                 // datagram numbers, plan after plan
  std::vector<uint32_t> hdr_of(count, 0);      // payload offset of a planned datagram
  std::vector<uint64_t> dst_of(count, ~0ull);  // offset in its message (complete plans), else ~0
  std::vector<uint32_t> plan_of(count, ~0u);
  uint64_t slab_need = 0;
  for (const OpenEntry &en : ent) {
    const uint8_t *d = dgrams[en.j];
    const uint32_t len = lens[en.j];
    const uint8_t top = d[0] & 0xE0;
    if (d[0] == 0x03 || top < 0x20 || top > 0xC0) continue;
    OpenPlan p{};
    p.first_part = (uint32_t)parts.size();
    p.session = en.session;
    p.index0 = en.index;
    p.type = d[0] & 0x1F;
    p.status = VDS_EC_EDGRAM_DATA;
    parts.push_back(en.j);
    const bool split = top == 0x40 || top == 0x80 || top == 0xC0;
    const uint32_t fixed = split ? 9 : 5;
    const uint32_t kind = (top >> 5) - (split ? 1 : 0);  // 1 direct, 3 routed, 5 proxied
    // (the hop count sits after the target id; read only when the datagram holds it)
    bool ok = true;
    uint32_t r = kind == 1 ? 0 : 32;
    if (kind == 5) {
      if (len - 32 > fixed + 32)
        r = 33 + 32u * d[fixed + 32];
      else
        ok = false;
    }
    p.hdr = fixed + r;
    p.route_len = r;
    ok = ok && len - 32 >= p.hdr;
    if (ok && !split) {
      p.len = len - 32 - p.hdr;
      p.status = VDS_EC_OK;
    } else if (ok) {
      // the reference's size checks as written (:663, :675, :687 -- the last
      // with its fixed constant, whatever the hop count)
      const uint64_t m = be32(d + 5);
      const uint32_t c = kind == 1 ? 41 : kind == 3 ? 73 : 106;
      if (len >= c && m > len - c) {
        const uint64_t pay0 = len - 32 - p.hdr;
        uint64_t rem = m - pay0;  // (wraps, as the reference's size_t does, when the constant let a small m by)
        p.len = pay0;
        p.status = VDS_EC_EDGRAM_INCOMPLETE;
        for (uint64_t at = (uint64_t)en.index + 1; at <= 0xFFFFFFFFull; ++at) {
          const OpenEntry *c1 = find(en.session, (uint32_t)at);
          if (!c1) break;
          parts.push_back(c1->j);
          const uint32_t l1 = lens[c1->j];
          if (dgrams[c1->j][0] != 0x03 || l1 < 37 || rem < l1 - 37) {
            p.status = VDS_EC_EDGRAM_DATA;
            break;
          }
          p.len += l1 - 37;
          rem -= l1 - 37;
          if (rem == 0) {
            p.status = VDS_EC_OK;
            break;
          }
        }
      }
    }
    p.nparts = (uint32_t)parts.size() - p.first_part;
    if (p.status == VDS_EC_OK) {
      uint64_t at = 0;
      for (uint32_t i = 0; i < p.nparts; ++i) {
        const uint32_t j = parts[p.first_part + i];
        hdr_of[j] = i == 0 ? p.hdr : 5;
        dst_of[j] = at;
        plan_of[j] = (uint32_t)plans.size();
        at += lens[j] - 32 - hdr_of[j];
      }
      slab_need += p.route_len + p.len;
    }
    plans.push_back(p);
  }
  if (slab_need > slab_bytes || (slab_need && !slab)) return VDS_EC_EINVAL;

  // ---- stage, open, copy back: whole messages, then the other signed datagrams
  std::vector<uint32_t> todo;  // datagram numbers in staging order
  std::vector<uint32_t> unit;  // todo positions where a unit (a message, or one datagram) begins
  for (const OpenPlan &p : plans)
    if (p.status == VDS_EC_OK) {
      unit.push_back((uint32_t)todo.size());
      todo.insert(todo.end(), parts.begin() + p.first_part, parts.begin() + p.first_part + p.nparts);
    }
  for (uint32_t j = 0; j < count; ++j) {
    const bool service = lens[j] >= 1 && (dgrams[j][0] == 6 || dgrams[j][0] == 7);
    if (service)
      verdicts[j] = 3;
    else if (plan_of[j] == ~0u) {
      unit.push_back((uint32_t)todo.size());
      todo.push_back(j);
    }
  }
  unit.push_back((uint32_t)todo.size());
  uint32_t nmsg = 0;
  uint64_t slab_at = 0;
  if (!todo.empty()) {
    if ((rc = device_ready())) return rc;
    SaveTempStage *st = save_temp_stage();
    if (!st) return VDS_EC_ENODEV;
    std::vector<uint64_t> in_off;
    std::vector<const uint8_t *> d_dg;
    std::vector<uint8_t *> d_dst;
    std::vector<uint32_t> g_len, g_hdr, g_ses;
    std::vector<Copy> cps;
    for (size_t u0 = 0; u0 + 1 < unit.size();) {
      uint64_t in_b = 0, asm_b = 0;
      size_t u1 = u0;
      in_off.clear();
      std::vector<uint64_t> asm_off;  // per datagram of the group: its payload's place in the assembly area, or ~0
      while (u1 + 1 < unit.size()) {
        uint64_t ub = 0;
        for (uint32_t t = unit[u1]; t < unit[u1 + 1]; ++t) ub += ((uint64_t)lens[todo[t]] + 3) & ~3ull;
        if (u1 > u0 && (in_b + ub > kSaveTempGroupBytes || unit[u1 + 1] - unit[u0] > (1u << 22))) break;
        for (uint32_t t = unit[u1]; t < unit[u1 + 1]; ++t) {
          const uint32_t j = todo[t];
          in_off.push_back(in_b);
          in_b += ((uint64_t)lens[j] + 3) & ~3ull;
          if (dst_of[j] != ~0ull) {
            asm_off.push_back(asm_b);
            asm_b += lens[j] - 32 - hdr_of[j];
          } else {
            asm_off.push_back(~0ull);
          }
        }
        ++u1;
      }
      const uint32_t t0 = unit[u0], cnt = unit[u1] - t0;
      const uint64_t vd_off = (asm_b + 15) & ~15ull;
      const uint64_t out_b = vd_off + cnt;
      if ((rc = st->reserve(std::max<uint64_t>(in_b, 64), out_b))) return rc;
      cps.clear();
      for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t j = todo[t0 + i];
        cps.push_back({st->h_in + in_off[i], dgrams[j], lens[j]});
      }
      parallel_copy(cps);
      hipError_t e = in_b ? hipMemcpyAsync(st->d_in, st->h_in, in_b, hipMemcpyHostToDevice, st->stream) : hipSuccess;
      if (e != hipSuccess) return hip_status(e);
      auto drained = [&](int r) {
        (void)hipStreamSynchronize(st->stream);
        return r;
      };
      d_dg.resize(cnt);
      d_dst.resize(cnt);
      g_len.resize(cnt);
      g_hdr.resize(cnt);
      g_ses.resize(cnt);
      for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t j = todo[t0 + i];
        d_dg[i] = st->d_in + in_off[i];
        d_dst[i] = asm_off[i] != ~0ull ? st->d_out + asm_off[i] : nullptr;
        g_len[i] = lens[j];
        g_hdr[i] = lens[j] >= 33 ? hdr_of[j] : 0;
        g_ses[i] = session_of[j];
      }
      rc = dgram_open_batch_device(cnt, d_dg.data(), g_len.data(), g_hdr.data(), g_ses.data(), keys, nsessions,
                                   d_dst.data(), st->d_out + vd_off, st->stream);
      if (rc) return drained(rc);
      e = hipMemcpyAsync(st->h_out, st->d_out, out_b, hipMemcpyDeviceToHost, st->stream);
      if (e != hipSuccess) return drained(hip_status(e));
      if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
      for (uint32_t i = 0; i < cnt; ++i) verdicts[todo[t0 + i]] = st->h_out[vd_off + i];
      // the group's whole messages: handed out only when every datagram verified
      cps.clear();
      for (uint32_t i = 0; i < cnt;) {
        const uint32_t j = todo[t0 + i];
        if (plan_of[j] == ~0u) {
          ++i;
          continue;
        }
        const OpenPlan &p = plans[plan_of[j]];
        bool good = true;
        for (uint32_t q = 0; q < p.nparts; ++q) good = good && st->h_out[vd_off + i + q] == 0;
        if (good) {
          vds_ec_dgram_message &mo = messages[plan_of[j]];
          mo.route_off = slab_at;
          mo.msg_off = slab_at + p.route_len;
          if (p.route_len) cps.push_back({slab + slab_at, dgrams[j] + (p.hdr - p.route_len), p.route_len});
          cps.push_back({slab + mo.msg_off, st->h_out + asm_off[i], p.len});
          slab_at += p.route_len + p.len;
        }
        i += p.nparts;
      }
      parallel_copy(cps);
      u0 = u1;
    }
  }
  // ---- the messages: planned status, or INCOMPLETE unless every datagram that planned it verified
  for (size_t pi = 0; pi < plans.size(); ++pi) {
    const OpenPlan &p = plans[pi];
    bool good = true;
    for (uint32_t q = 0; q < p.nparts; ++q) good = good && verdicts[parts[p.first_part + q]] == 0;
    vds_ec_dgram_message &mo = messages[pi];
    const uint64_t ro = mo.route_off, mf = mo.msg_off;
    const bool handed = good && p.status == VDS_EC_OK;
    mo = vds_ec_dgram_message{};
    mo.session = p.session;
    mo.index0 = p.index0;
    mo.dgrams = p.nparts;
    mo.type = p.type;
    mo.status = good ? p.status : VDS_EC_EDGRAM_INCOMPLETE;
    if (handed) {
      mo.route_len = p.route_len;
      mo.route_off = ro;
      mo.msg_off = mf;
      mo.msg_len = p.len;
    }
    ++nmsg;
  }
  *nmessages = nmsg;
  return VDS_EC_OK;
}

}  // namespace api
}  // namespace vds_ec

extern "C" {

int vds_ec_hmac_sha256_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens,
                                    const uint32_t *session_of, const uint8_t *keys, uint32_t nsessions,
                                    uint8_t *macs, const uint8_t *expected, uint8_t *verdicts, void *stream) {
  return vds_ec::api::hmac_sha256_batch_device(count, msgs, lens, session_of, keys, nsessions, macs, expected,
                                               verdicts, vds_ec::api::as_stream(stream));
}

int vds_ec_dgram_seal_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *msg_lens,
                                   const uint8_t *types, const uint32_t *index0, const uint8_t *const *routes,
                                   const uint32_t *route_lens, const uint32_t *session_of, const uint8_t *keys,
                                   const uint32_t *mtus, uint32_t nsessions, uint8_t *const *outs, uint64_t pitch,
                                   void *stream) {
  return vds_ec::api::dgram_seal_batch_device(count, msgs, msg_lens, types, index0, routes, route_lens, session_of,
                                              keys, mtus, nsessions, outs, pitch, vds_ec::api::as_stream(stream));
}

int vds_ec_dgram_open_batch_device(uint32_t count, const uint8_t *const *dgrams, const uint32_t *lens,
                                   const uint32_t *hdr_lens, const uint32_t *session_of, const uint8_t *keys,
                                   uint32_t nsessions, uint8_t *const *dsts, uint8_t *verdicts, void *stream) {
  return vds_ec::api::dgram_open_batch_device(count, dgrams, lens, hdr_lens, session_of, keys, nsessions, dsts,
                                              verdicts, vds_ec::api::as_stream(stream));
}

int vds_ec_dgram_seal_host_batch(uint32_t count, const uint8_t *const *msgs, const uint64_t *msg_lens,
                                 const uint8_t *types, const uint32_t *index0, const uint8_t *const *routes,
                                 const uint32_t *route_lens, const uint32_t *session_of, const uint8_t *keys,
                                 const uint32_t *mtus, uint32_t nsessions, uint8_t *slab, uint64_t slab_bytes,
                                 uint64_t *offsets, uint32_t *dgram_counts, uint32_t *last_lens) {
  return vds_ec::api::dgram_seal_host_batch(count, msgs, msg_lens, types, index0, routes, route_lens, session_of, keys,
                                            mtus, nsessions, slab, slab_bytes, offsets, dgram_counts, last_lens);
}

int vds_ec_dgram_open_host_batch(uint32_t count, const uint8_t *const *dgrams, const uint32_t *lens,
                                 const uint32_t *session_of, const uint8_t *keys, uint32_t nsessions,
                                 uint8_t *verdicts, uint8_t *slab, uint64_t slab_bytes,
                                 vds_ec_dgram_message *messages, uint32_t *nmessages) {
  return vds_ec::api::dgram_open_host_batch(count, dgrams, lens, session_of, keys, nsessions, verdicts, slab,
                                            slab_bytes, messages, nmessages);
}

}  // extern "C"
