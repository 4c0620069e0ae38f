// api_deflate_batch.cpp -- buffers of a batch deflated into zlib streams on the
// device (vds_ec_deflate_batch_device: deflate.hip's one launch, planned on the
// host) and its host form through pinned staging (vds_ec_deflate_host_batch).
// The pack chain built on it lives in api_block_batch.cpp; one message on the
// calling thread is deflate_host.cpp.
// (api_internal.hpp lists the host runtime's translation units.)
#include "api_internal.hpp"

namespace vds_ec {
namespace api {

namespace {

inline bool overlap(const void *a, uint64_t la, const void *b, uint64_t lb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return la && lb && x < y + lb && y < x + la;
}

struct DeflateScratch {
  std::vector<uint32_t> order, bucket;
};
DeflateScratch &deflate_scratch() {
  thread_local DeflateScratch sc;
  return sc;
}

}  // namespace

int check_deflate_args(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, uint8_t *const *outs,
                       const uint64_t *out_caps) {
  if (count >= (1u << 30)) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  if (!ins || !lens || !outs || !out_caps) return VDS_EC_EINVAL;
  for (uint32_t o = 0; o < count; ++o) {
    if (lens[o] > 0xFFFFFFFFull || out_caps[o] > 0xFFFFFFFFull) return VDS_EC_EINVAL;
    const uint64_t bound = vds_ec_deflate_bound(lens[o]);
    if (bound > 0xFFFFFFFFull || out_caps[o] < bound) return VDS_EC_EINVAL;
    if ((lens[o] && !ins[o]) || !outs[o]) return VDS_EC_EINVAL;
    if (overlap(ins[o], lens[o], outs[o], out_caps[o])) return VDS_EC_EINVAL;
  }
  return VDS_EC_OK;
}

// One wave walks one message, and a message's time goes with its length, so
// the messages go longest first, equal lengths in the caller's order: a
// counting sort on the length in 64-byte units (the kernel's chunk) where those
// are few against the batch, else a comparison sort.  Then the table in one
// ring slot and the launch.  (Validated; the device is ready.)
int enqueue_deflate(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, uint8_t *const *outs,
                    const uint64_t *out_caps, uint32_t *out_lens, hipStream_t s) {
  DeflateScratch &sc = deflate_scratch();
  sc.order.resize(count);
  uint64_t kmax = 0;
  for (uint32_t o = 0; o < count; ++o) kmax = std::max<uint64_t>(kmax, lens[o] / 64);
  if (kmax <= 4ull * count + 4096) {
    sc.bucket.assign((size_t)kmax + 2, 0);
    for (uint32_t o = 0; o < count; ++o) ++sc.bucket[kmax - lens[o] / 64 + 1];
    for (size_t b = 1; b < sc.bucket.size(); ++b) sc.bucket[b] += sc.bucket[b - 1];
    for (uint32_t o = 0; o < count; ++o) sc.order[sc.bucket[kmax - lens[o] / 64]++] = o;
  } else {
    for (uint32_t o = 0; o < count; ++o) sc.order[o] = o;
    std::stable_sort(sc.order.begin(), sc.order.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
  }
  const size_t bytes = (size_t)count * sizeof(InflateMsg);
  ParamSlot *slot = nullptr;
  hipError_t e = param_acquire_n(1, &bytes, &slot);
  if (e != hipSuccess) return hip_status(e);
  InflateMsg *t = reinterpret_cast<InflateMsg *>(slot->h);
  for (uint32_t j = 0; j < count; ++j) {
    const uint32_t o = sc.order[j];
    t[j] = InflateMsg{reinterpret_cast<uintptr_t>(ins[o]), reinterpret_cast<uintptr_t>(outs[o]), (uint32_t)lens[o],
                      (uint32_t)out_caps[o], o, 0};
  }
  e = param_commit(slot, bytes, s);
  if (e == hipSuccess) e = launch_deflate_batch(reinterpret_cast<const InflateMsg *>(slot->d), count, out_lens, s);
  const hipError_t re = param_release(slot, s);  // (its event follows whatever was enqueued)
  return hip_status(e != hipSuccess ? e : re);
}

int deflate_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, uint8_t *const *outs,
                         const uint64_t *out_caps, uint32_t *out_lens, hipStream_t s) {
  int rc = check_deflate_args(count, ins, lens, outs, out_caps);
  if (rc || count == 0) return rc;
  if (!out_lens || (reinterpret_cast<uintptr_t>(out_lens) & 3u)) return VDS_EC_EINVAL;
  if ((rc = device_ready())) return rc;
  return enqueue_deflate(count, ins, lens, outs, out_caps, out_lens, s);
}

int deflate_host_batch(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, uint8_t *const *outs,
                       const uint64_t *out_caps, uint64_t *out_lens) {
  int rc = check_deflate_args(count, ins, lens, outs, out_caps);
  if (rc) return rc;
  if (count && !out_lens) return VDS_EC_EINVAL;
  if (count == 0) return VDS_EC_OK;
  if ((rc = device_ready())) return rc;
  SaveTempStage *st = save_temp_stage();
  if (!st) return VDS_EC_ENODEV;
  std::vector<uint64_t> i_off, o_off, bounds;
  std::vector<const uint8_t *> d_ins;
  std::vector<uint8_t *> d_outs;
  std::vector<Copy> parts;
  for (uint32_t o0 = 0; o0 < count;) {
    // The group: messages o0 .. o1-1, at most 64 MiB each way.  Inputs at
    // 16-byte aligned offsets of the input staging; in the output staging the
    // outputs' bounds at 16-byte aligned offsets, then the lengths.
    i_off.clear();
    o_off.clear();
    bounds.clear();
    uint64_t in_b = 0, out_b = 0;
    uint32_t o1 = o0;
    while (o1 < count && o1 - o0 < kSaveTempGroupObjects) {
      const uint64_t ia = (in_b + 15) & ~15ull, oa = (out_b + 15) & ~15ull, bound = vds_ec_deflate_bound(lens[o1]);
      if (o1 > o0 && (ia + lens[o1] > kSaveTempGroupBytes || oa + bound > kSaveTempGroupBytes)) break;
      i_off.push_back(ia);
      o_off.push_back(oa);
      bounds.push_back(bound);
      in_b = ia + lens[o1];
      out_b = oa + bound;
      ++o1;
    }
    const uint32_t cnt = o1 - o0;
    const uint64_t len_off = (out_b + 15) & ~15ull, back_b = len_off + 4ull * cnt;
    if ((rc = st->reserve(std::max<uint64_t>(in_b, 64), back_b))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j) parts.push_back({st->h_in + i_off[j], ins[o0 + j], lens[o0 + j]});
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
    d_outs.resize(cnt);
    for (uint32_t j = 0; j < cnt; ++j) {
      d_ins[j] = st->d_in + i_off[j];
      d_outs[j] = st->d_out + o_off[j];
    }
    rc = enqueue_deflate(cnt, d_ins.data(), lens + o0, d_outs.data(), bounds.data(),
                         reinterpret_cast<uint32_t *>(st->d_out + len_off), st->stream);
    if (rc) return drained(rc);
    // the lengths first: only what was written comes back
    e = hipMemcpyAsync(st->h_out + len_off, st->d_out + len_off, back_b - len_off, hipMemcpyDeviceToHost, st->stream);
    if (e != hipSuccess) return drained(hip_status(e));
    if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    const uint32_t *dl = reinterpret_cast<const uint32_t *>(st->h_out + len_off);
    uint64_t hi = 0;
    for (uint32_t j = 0; j < cnt; ++j) {
      if (dl[j] > bounds[j]) return VDS_EC_EHIP;  // (cannot be: the stored form is the bound)
      hi = std::max<uint64_t>(hi, o_off[j] + dl[j]);
    }
    e = hipMemcpyAsync(st->h_out, st->d_out, hi, hipMemcpyDeviceToHost, st->stream);
    if (e != hipSuccess) return drained(hip_status(e));
    if ((rc = hip_status(hipStreamSynchronize(st->stream)))) return rc;
    parts.clear();
    for (uint32_t j = 0; j < cnt; ++j) {
      out_lens[o0 + j] = dl[j];
      parts.push_back({outs[o0 + j], st->h_out + o_off[j], dl[j]});
    }
    parallel_copy(parts);
    o0 = o1;
  }
  return VDS_EC_OK;
}

}  // namespace api
}  // namespace vds_ec

extern "C" {

int vds_ec_deflate_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, uint8_t *const *outs,
                                const uint64_t *out_caps, uint32_t *out_lens, void *stream) {
  return vds_ec::api::deflate_batch_device(count, ins, lens, outs, out_caps, out_lens, vds_ec::api::as_stream(stream));
}

int vds_ec_deflate_host_batch(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, uint8_t *const *outs,
                              const uint64_t *out_caps, uint64_t *out_lens) {
  return vds_ec::api::deflate_host_batch(count, ins, lens, outs, out_caps, out_lens);
}

}  // extern "C"
