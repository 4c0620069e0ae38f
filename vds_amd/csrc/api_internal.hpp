// api_internal.hpp -- host runtime internals shared by the C ABI's
// translation units (internal to libvds_ec.so):
//   vds_ec_api.cpp      argument validation, host field arithmetic and the
//                       inverse, encode / restore / regenerate dispatch, host
//                       staging contexts, the C ABI itself;
//   api_param_ring.cpp  the stream-ordered parameter ring;
//   api_batch.cpp       batched per-object-survivor restore / regenerate
//                       planning (routes, erased-set plans, tiles);
//   api_encode_batch.cpp  batched encode of objects of different sizes
//                       (planning, tables, the one shared launch);
//   api_save_temp_batch.cpp  SHA-256 over messages of different lengths and
//                       the batched save_temp built on it (device and host);
//                       its check mode and the batched repair (regenerate,
//                       name, check);
//   api_upload_batch.cpp  base64 wire text decoded and encoded on the device,
//                       and the batched upload from text (decode, save_temp);
//   api_ws_batch.cpp    websocket frames: the upload loop from frames to answer
//                       frames, the download loop answering in frames;
//   api_download_batch.cpp  the download loop in one call: the name check
//                       (survivors or a witness), the batched restore and the
//                       gated base64 encode (device and host);
//   api_dgram_batch.cpp  the node-to-node datagram layer: batched HMAC-SHA256,
//                       sealing and opening of datagrams (device and host);
//   api_block_batch.cpp  file blocks: batched AES-256-CBC, the pack of a batch
//                       of blocks (hash, encrypt, hash, encrypt), the unpack
//                       (decrypt, inflate, name check) and the host forms;
//   api_inflate_batch.cpp  zlib streams of a batch inflated on the device, and
//                       the host form;
//   api_deflate_batch.cpp  buffers of a batch deflated on the device, and the
//                       host form;
//   api_host_batch.cpp  caller-pinned slabs, the multi-GPU host batches and
//                       the stripe-range split.
#pragma once

#include "../../include/vds_ec.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <climits>
#include <condition_variable>
#include <cstdint>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <sched.h>
#include <shared_mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "ec_internal.hpp"
#include "gf_common.hpp"

namespace vds_ec {
namespace api {

struct HostCtx;
struct RestorePlan;

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// ------------------------------------------------- host field arithmetic
// log / antilog tables for the host's k x k and M x M work (gf.h:193-253's
// tables; the kernels never use them).  Built once, 384 KiB.
struct Gf16Tables {
  uint16_t log[65536];
  uint16_t exp[2 * 65535];
  Gf16Tables() {
    uint32_t v = 1;
    for (uint32_t l = 0; l < 65535; ++l) {
      exp[l] = exp[l + 65535] = (uint16_t)v;
      log[v] = (uint16_t)l;
      v = gf16_mul(v, 2);
    }
    log[0] = 0;
  }
};

// ------------------------------------------------ stream-ordered parameters
// Kernel parameters too large for the kernel arguments (k > 32 inverses, k >
// 64 chunk tables, regenerate coefficients beyond kInlineCoef) ride a
// per-device ring of pinned host + device slots, so the *_device entry points
// enqueue without synchronising.  A slot's bytes are written on the host,
// copied with hipMemcpyAsync on the caller's stream, and an event recorded
// after the kernels that read them; a slot is reused only once its event has
// completed, and hipEventSynchronize blocks only when the ring has wrapped
// round inside the GPU's queue.  (The round-1 version copied a std::vector
// on the caller's stack with hipMemcpyAsync and freed a hipMallocAsync
// buffer in a destructor: the copy could read the vector after it was gone
// -- the likely cause of that round's fault)  Growing a slot
// allocates, which synchronises; slots only grow.
struct ParamSlot {
  uint8_t *h = nullptr, *d = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  hipEvent_t copied = nullptr;  // the host -> device copy on the ring's copy stream
  bool pending = false;  // its event guards the device copy's readers
  bool busy = false;     // acquired, not yet released
  uint64_t stamp = 0;    // when last acquired (ParamRing::clock)
};

// --------------------------------------------------------- restore core
// Optional layout facts the host path knows: chunks contiguous at a pitch,
// and a device copy of a large inverse already staged.
struct ChunkLayout {
  const uint8_t *base = nullptr;
  uint64_t pitch = 0;
  const uint16_t *matrix_dev = nullptr;
};

struct Copy {
  uint8_t *dst;
  const uint8_t *src;
  size_t len;
};

// ---------------------------------------------- caller-pinned host memory
// Buffers the caller allocated with vds_ec_host_alloc or registered with
// vds_ec_host_register (page-locked, mapped, portable across devices).  A
// host batch whose group of objects (or replicas) lies in one such range as
// one contiguous slab skips the staging copies: the H2D DMA reads the
// caller's bytes, and the push kernel writes the results straight into the
// caller's pages.  Lookups are per group, not per object.
constexpr int kPinnedMaxDev = 64;
struct PinnedRange {
  uint64_t bytes;
  bool owned;  // vds_ec_host_alloc (freed by vds_ec_host_free) vs registered
  // the device address of the range's first byte, per device: resolved on
  // each device the first time a host batch there uses the range (a mapped
  // host range need not have the same address on every device)
  uint8_t *dev[kPinnedMaxDev] = {};
};
struct PinnedRegistry {
  std::mutex mu;
  std::map<uintptr_t, PinnedRange> ranges;  // by start address
};

// Per (thread, device) staging of the host form: pinned and device buffers
// for one group each way, and a stream.  Kept across calls (hipHostMalloc of
// tens of MiB costs more than the group it feeds); never freed, as the other
// host contexts (at process exit it would race the HIP runtime's teardown).
struct SaveTempStage {
  hipStream_t stream = nullptr;
  uint8_t *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;
  size_t in_cap = 0, out_cap = 0;
  int reserve(size_t in_b, size_t out_b) {
    if (!stream && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return VDS_EC_ENODEV;
    if (in_b > in_cap) {
      if (h_in) (void)hipHostFree(h_in);
      if (d_in) (void)hipFree(d_in);
      h_in = d_in = nullptr;
      in_cap = 0;
      if (hipHostMalloc(&h_in, in_b, 0) != hipSuccess || hipMalloc(&d_in, in_b) != hipSuccess) return VDS_EC_ENOMEM;
      in_cap = in_b;
    }
    if (out_b > out_cap) {
      if (h_out) (void)hipHostFree(h_out);
      if (d_out) (void)hipFree(d_out);
      h_out = d_out = nullptr;
      out_cap = 0;
      if (hipHostMalloc(&h_out, out_b, 0) != hipSuccess || hipMalloc(&d_out, out_b) != hipSuccess)
        return VDS_EC_ENOMEM;
      out_cap = out_b;
    }
    return VDS_EC_OK;
  }
};

SaveTempStage *save_temp_stage();
// a group's bound: api_host_batch.cpp's 64 MiB of input, and a count that keeps its tables small
constexpr uint64_t kSaveTempGroupBytes = 64ull << 20;
constexpr uint32_t kSaveTempGroupObjects = 1u << 16;

int hip_status(hipError_t e);
int device_ready();
int inverse16(uint32_t k, const uint16_t *nodes, uint16_t *out);
bool restore_path_override_bs();
bool syn_solve(uint32_t k, uint32_t n, SynRestoreArgs &sa);
int encode_device(unsigned cb, uint32_t k, const uint16_t *replicas, uint32_t n, const uint8_t *in,
                  uint64_t size, uint64_t in_stride, uint32_t count, uint8_t *const *outs,
                  uint64_t out_stride, unsigned flags, hipStream_t s);
int encode_batch_device(uint32_t k, const uint16_t *replicas, uint32_t n, uint32_t count, const uint8_t *const *ins,
                        const uint64_t *sizes, uint8_t *const *outs, unsigned flags, hipStream_t s);
int encode_batch_path(uint32_t k, const uint16_t *replicas, uint32_t n, uint32_t count, const uint8_t *const *ins,
                      const uint64_t *sizes, uint8_t *const *outs, unsigned flags, uint32_t *fast_objects);
// What plan_encode_batch's one pass over the objects leaves: the eligible
// objects' descriptors in the caller's order (table addresses still as offsets
// into `ptrs`), the others' indices in ascending order, and the eligible
// objects' groups summed.  Kept per thread, so a caller's loop allocates
// nothing after its first call.
struct EncBatchScratch {
  std::vector<EncBatchObj> objs;
  std::vector<uint8_t *> ptrs;  // replica pointer tables of the objects whose replicas are not equally spaced
  std::vector<uint32_t> rest;   // the objects that take encode_device, one call each
  uint64_t groups = 0;
};
EncBatchScratch &enc_batch_scratch();
int plan_encode_batch(uint32_t k, const uint16_t *replicas, uint32_t n, uint32_t count, const uint8_t *const *ins,
                      const uint64_t *sizes, uint8_t *const *outs, unsigned flags, EncBatchScratch &sc);
// Enqueue what the plan describes (the device is ready): the shared launch, then the rest one call each.
int encode_batch_run(uint32_t k, const uint16_t *replicas, uint32_t n, uint32_t count, const uint8_t *const *ins,
                     const uint64_t *sizes, uint8_t *const *outs, unsigned flags, const EncBatchScratch &sc,
                     hipStream_t s);
int sha256_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens, uint8_t *digests,
                        hipStream_t s);
int save_temp_batch_device(uint32_t k, uint32_t n, uint32_t count, const uint8_t *const *ins, const uint64_t *sizes,
                           uint8_t *const *outs, uint8_t *replica_digests, uint8_t *data_digests, hipStream_t s);
int save_temp_host_batch(uint32_t k, uint32_t n, uint32_t count, const uint8_t *const *objs, const uint64_t *sizes,
                         uint8_t *const *outs, uint8_t *replica_digests, uint8_t *data_digests,
                         uint32_t *replica_sizes);
int sha256_check_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens,
                              const uint8_t *expected, uint8_t *digests, uint8_t *verdicts, hipStream_t s);
// The unpack chain's name check (k_sha256_batch<true, true>): message j, whose
// length and status exist only on the device (lens_dev[j] <= caps[j], statuses
// [j]), hashed and compared with expected + 32 j where its status lets it.
// The caller has validated the arguments and found the device.
int sha256_gated_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *caps,
                              const uint8_t *expected, uint32_t *lens_dev, int32_t *statuses, hipStream_t s);
// zlib streams inflated (api_inflate_batch.cpp, inflate.hip).  enqueue_inflate:
// validated arguments, the device ready; in_lens / gate: the unpack chain's
// device arrays (InflateLaunch), or null.
int check_inflate_args(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, uint8_t *const *outs,
                       const uint64_t *out_caps);
int enqueue_inflate(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, uint8_t *const *outs,
                    const uint64_t *out_caps, uint32_t *out_lens, int32_t *statuses, const uint32_t *in_lens,
                    const int32_t *gate, hipStream_t s);
// Buffers deflated (api_deflate_batch.cpp, deflate.hip).  check_deflate_args:
// everything vds_ec_deflate_batch_device rejects but out_lens.  enqueue_deflate:
// validated arguments, the device ready.
int check_deflate_args(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, uint8_t *const *outs,
                       const uint64_t *out_caps);
int enqueue_deflate(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, uint8_t *const *outs,
                    const uint64_t *out_caps, uint32_t *out_lens, hipStream_t s);
int repair_batch_device(uint32_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                        const uint64_t *chunk_sizes, uint32_t nt, const uint16_t *targets, uint8_t *const *outs,
                        uint8_t *digests, const uint8_t *expected, uint8_t *verdicts, hipStream_t s);
int repair_host_batch(uint32_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                      const uint64_t *chunk_sizes, uint32_t nt, const uint16_t *targets, uint8_t *const *outs,
                      uint8_t *digests, const uint8_t *expected, uint8_t *verdicts, uint32_t *mismatches);
// base64 wire text on the device (api_upload_batch.cpp, base64.hip)
// The messages of one decode launch before they are ordered (masks: empty, or
// one little-endian word of four mask bytes a message).  Kept per thread, so a
// caller's loop allocates nothing after its first call.
struct B64DecScratch {
  std::vector<B64DecMsg> msgs;
  std::vector<uint32_t> masks;
  std::vector<uint32_t> key, order, bucket;
};
B64DecScratch &b64_dec_scratch();
int launch_decode(B64DecScratch &sc, hipStream_t s);
int base64_decode_batch_device(uint32_t count, const char *const *texts, const uint64_t *text_lens,
                               const uint8_t *masks, bool masked, uint8_t *const *outs, const uint64_t *out_sizes,
                               int32_t *statuses, hipStream_t s);
// websocket frames in, answer frames out (api_ws_batch.cpp)
int ws_upload_answer_batch_device(uint32_t count, const int32_t *ids, uint32_t n, const uint8_t *replica_digests,
                                  const uint8_t *data_digests, const uint32_t *replica_sizes, uint8_t *const *outs,
                                  hipStream_t s);
int ws_upload_host_batch(uint32_t k, uint32_t n, uint32_t count, const uint8_t *const *frames,
                         const uint64_t *frame_lens, uint8_t *const *outs, uint8_t *replica_digests,
                         uint8_t *data_digests, uint32_t *replica_sizes, uint8_t *answers, uint64_t answers_bytes,
                         uint64_t *answer_offs, uint64_t *answer_lens, int32_t *statuses, uint32_t *failed);
int ws_download_host_batch(uint32_t k, uint32_t count, const int32_t *ids, const uint16_t *nodes,
                           const uint8_t *const *chunks, const uint64_t *chunk_sizes, const uint8_t *survivor_names,
                           const uint16_t *witness_ids, const uint8_t *witness_names, uint8_t *slab,
                           uint64_t slab_bytes, uint64_t *frame_offs, uint64_t *frame_lens, int32_t *statuses,
                           uint8_t *survivor_verdicts, uint32_t *failed);
int base64_encode_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens, char *const *outs,
                               hipStream_t s);
int upload_host_batch(uint32_t k, uint32_t n, uint32_t count, const char *const *texts, const uint64_t *text_lens,
                      uint8_t *const *outs, uint8_t *replica_digests, uint8_t *data_digests, uint32_t *replica_sizes,
                      uint8_t *const *bodies, uint64_t *body_sizes, int32_t *statuses, uint32_t *failed);
// the download loop (api_download_batch.cpp): check, restore, gated base64 encode
int sha256_check_groups_device(uint32_t ngroups, uint32_t m, const uint8_t *const *msgs, const uint64_t *lens,
                               const uint8_t *const *expected, uint8_t *const *verdicts, hipStream_t s);
int base64_encode_gated_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                     char *const *outs, const uint8_t *const *gates, const uint32_t *ngates,
                                     int32_t *statuses, hipStream_t s);
int download_batch_device(uint32_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                          const uint64_t *chunk_sizes, const uint16_t *paddings, const uint8_t *survivor_names,
                          const uint16_t *witness_ids, const uint8_t *witness_names, uint8_t *const *witness_outs,
                          uint8_t *const *objects, char *const *texts, uint8_t *verdicts, int32_t *statuses,
                          hipStream_t s);
int download_host_batch(uint32_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                        const uint64_t *chunk_sizes, const uint8_t *survivor_names, const uint16_t *witness_ids,
                        const uint8_t *witness_names, char *const *texts, uint64_t *text_lens, int32_t *statuses,
                        uint8_t *survivor_verdicts, uint32_t *failed);
// the node-to-node datagram layer (api_dgram_batch.cpp, dgram.hip)
int hmac_sha256_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens,
                             const uint32_t *session_of, const uint8_t *keys, uint32_t nsessions, uint8_t *macs,
                             const uint8_t *expected, uint8_t *verdicts, hipStream_t s);
int dgram_seal_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *msg_lens,
                            const uint8_t *types, const uint32_t *index0, const uint8_t *const *routes,
                            const uint32_t *route_lens, const uint32_t *session_of, const uint8_t *keys,
                            const uint32_t *mtus, uint32_t nsessions, uint8_t *const *outs, uint64_t pitch,
                            hipStream_t s);
int dgram_open_batch_device(uint32_t count, const uint8_t *const *dgrams, const uint32_t *lens,
                            const uint32_t *hdr_lens, const uint32_t *session_of, const uint8_t *keys,
                            uint32_t nsessions, uint8_t *const *dsts, uint8_t *verdicts, hipStream_t s);
int dgram_seal_host_batch(uint32_t count, const uint8_t *const *msgs, const uint64_t *msg_lens, const uint8_t *types,
                          const uint32_t *index0, const uint8_t *const *routes, const uint32_t *route_lens,
                          const uint32_t *session_of, const uint8_t *keys, const uint32_t *mtus, uint32_t nsessions,
                          uint8_t *slab, uint64_t slab_bytes, uint64_t *offsets, uint32_t *dgram_counts,
                          uint32_t *last_lens);
int dgram_open_host_batch(uint32_t count, const uint8_t *const *dgrams, const uint32_t *lens,
                          const uint32_t *session_of, const uint8_t *keys, uint32_t nsessions, uint8_t *verdicts,
                          uint8_t *slab, uint64_t slab_bytes, vds_ec_dgram_message *messages, uint32_t *nmessages);
hipError_t param_acquire_n(int cnt, const size_t *bytes, ParamSlot **out);
hipError_t param_commit(ParamSlot *sl, size_t bytes, hipStream_t s);
hipError_t param_release(ParamSlot *sl, hipStream_t s);
hipError_t param_stage(const std::vector<uint8_t> &blob, hipStream_t s, const uint8_t **dev, ParamSlot **out);
int restore_device(unsigned cb, uint32_t k, const uint16_t *nodes, const uint16_t *matrix, const uint8_t *const *chunks,
                   uint64_t chunk_size, uint64_t chunk_stride, uint64_t out_len, uint32_t count,
                   uint8_t *out, uint64_t out_stride, unsigned flags, hipStream_t s,
                   const ChunkLayout &layout = ChunkLayout());
uint64_t restored_len(unsigned cb, uint32_t k, uint64_t chunk_size, uint16_t padding, unsigned flags,
                      bool *ok);
void parallel_copy(const std::vector<Copy> &parts_in);
extern std::atomic<uint64_t> g_host_ctx_created;
int regenerate_device(unsigned cb, uint32_t k, const uint16_t *nodes, const uint8_t *const *chunks,
                      uint64_t chunk_size, uint64_t chunk_stride, uint32_t count, const uint16_t *targets,
                      uint32_t nt, uint8_t *const *outs, uint64_t out_stride, hipStream_t s);
bool ids_distinct(uint32_t k, const uint16_t *nd);
int restore_batch_device(uint32_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                         const uint64_t *chunk_sizes, const uint16_t *paddings, uint8_t *const *outs, unsigned flags,
                         hipStream_t s);
int regenerate_batch_device(uint32_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                            const uint64_t *chunk_sizes, uint32_t nt, const uint16_t *targets, uint8_t *const *outs,
                            hipStream_t s);
PinnedRegistry &pinned_registry();
int encode_host_batch(uint32_t k, const uint16_t *replicas, uint32_t n, const uint8_t *const *objs,
                      const uint64_t *sizes, uint32_t count, uint8_t *const *outs, unsigned flags, int max_devices);
int restore_host_batch(uint32_t k, const uint16_t *nodes, const uint8_t *const *chunks, const uint64_t *chunk_sizes,
                       uint32_t count, uint8_t *const *outs, uint64_t *out_sizes, unsigned flags, int max_devices);
int encode_range(uint32_t k, const uint16_t *replicas, uint32_t n, const uint8_t *in, uint64_t size, uint64_t t0,
                 uint64_t t1, uint8_t *const *outs, unsigned flags, hipStream_t s);
int range_restore_len(uint32_t k, uint64_t chunk_size, uint16_t padding, unsigned flags, uint64_t *E, uint64_t *nst);
int restore_range(uint32_t k, const uint16_t *nodes, const uint16_t *matrix, const uint8_t *const *chunks,
                  uint64_t t0, uint64_t t1, uint64_t E, uint8_t *out, unsigned flags, hipStream_t s);
int encode_host_split(uint32_t k, const uint16_t *replicas, uint32_t n, const uint8_t *data, uint64_t size,
                      uint8_t *const *outs, unsigned flags, int max_devices, uint32_t parts);
int restore_host_split(uint32_t k, const uint16_t *nodes, const uint8_t *const *chunks, uint64_t chunk_size,
                       uint8_t *out, uint64_t *out_size, unsigned flags, int max_devices, uint32_t parts);const Gf16Tables &gf16_tables();

inline uint32_t gf16_mul_fast(uint32_t a, uint32_t b) {
  if (!a || !b) return 0;
  const Gf16Tables &t = gf16_tables();
  return t.exp[t.log[a] + t.log[b]];
}

inline uint32_t gf16_inv_fast(uint32_t a) {
  if (!a) return 0;
  const Gf16Tables &t = gf16_tables();
  return t.exp[65535 - t.log[a]];
}

template <typename T>
size_t blob_append(std::vector<uint8_t> &blob, const T *p, size_t n) {
  const size_t off = (blob.size() + 15) & ~size_t(15);
  blob.resize(off + sizeof(T) * n);
  std::memcpy(blob.data() + off, p, sizeof(T) * n);
  return off;
}

template <typename Id>
int check_restore_args(uint32_t k, const Id *nodes, const uint8_t *const *chunks, uint64_t chunk_size) {
  if (k == 0 || !nodes || !chunks) return VDS_EC_EINVAL;
  for (uint32_t j = 0; j < k; ++j)
    if (!chunks[j] && chunk_size) return VDS_EC_EINVAL;
  return VDS_EC_OK;
}

}  // namespace api
}  // namespace vds_ec
