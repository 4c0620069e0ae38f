/*
 * vds_ec.h -- C ABI of the MI355X-native object-chunk erasure codec.
 *
 * This is the boundary that replaces the CPU arithmetic of lboss75/vds
 * kernel/vds_data (chunk.h, gf.h, chunk_storage.cpp).  The reference's codec
 * is header-only C++ templates; the drop-in headers in vds_amd/include/vds_data/
 * keep that exact template API and forward the uint8_t / uint16_t
 * instantiations to the entry points below (see INTEGRATION.md for the
 * binding).  Plain pointers, sizes and int status codes only.
 *
 * Terminology (reference): an object of S bytes is cut into stripes of
 * k cells; a "replica" (horcrux) with id r holds, per stripe, the evaluation
 * at r of the polynomial whose coefficients are the stripe's cells
 * (chunk.h:245-281), followed by a 2-byte big-endian trailer S mod (k*cell).
 * Any k distinct replicas restore the object (chunk.h:290-444).
 *
 * Memory: *_device entry points take device pointers and enqueue work on the
 * given hipStream_t (NULL = the current device's null stream) without
 * synchronising; parameters too large for the kernel arguments (k > 32
 * inverses, k > 64 chunk tables) are staged stream-ordered through a pinned
 * ring (growing it, on first use of a larger size, allocates).  *_host entry points take host pointers, stage through
 * pinned buffers on the current device and return when the result is in host
 * memory.  Every entry point fails with VDS_EC_ENODEV if no GPU is usable --
 * there is no CPU fallback.
 */
#ifndef VDS_EC_H_
#define VDS_EC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ----------------------------------------------------------- status codes */
#define VDS_EC_OK 0
#define VDS_EC_EINVAL (-1)    /* bad argument (k == 0, null pointer, size)     */
#define VDS_EC_ENODEV (-2)    /* no usable GPU / HIP runtime error at init    */
#define VDS_EC_ENOMEM (-3)    /* device or pinned allocation failed           */
#define VDS_EC_ESINGULAR (-4) /* replica ids not distinct: V not invertible   */
#define VDS_EC_ERESTORE (-5)  /* "Fatal error at chunk_restore::restore"      */
#define VDS_EC_EHIP (-6)      /* HIP runtime error during a launch / copy     */
/* base64::to_bytes failures (encoding.cpp:181-247), by the reference's text: */
#define VDS_EC_EB64_LENGTH (-7)  /* "Non-Valid base64!" (length % 4 != 0)      */
#define VDS_EC_EB64_PADDING (-8) /* "Invalid Padding in Base 64!"              */
#define VDS_EC_EB64_CHAR (-9)    /* "Non-Valid Character in Base 64!"          */
/* a replica's bytes do not hash to its name (read_data, dht_network_client.cpp:952-960): */
#define VDS_EC_ECORRUPT (-10)    /* "Data is corrupted"                        */
/* the datagram layer (dht_datagram_protocol.cpp:130-141, :544-769), by the reference's text: */
#define VDS_EC_EDGRAM_SIGNATURE (-11)  /* "Invalid signature"                   */
#define VDS_EC_EDGRAM_DATA (-12)       /* "Invalid data"                        */
#define VDS_EC_EDGRAM_INCOMPLETE (-13) /* a message whose datagrams are not all present and verified */
/* websocket frames (vds_ec_ws_*) */
#define VDS_EC_EWS_SHORT (-14) /* the frame's header (or, in a batch, the frame) is not all there yet */
#define VDS_EC_EWS_FRAME (-15) /* "Not implemented" (an opcode other than text, binary and ping)   */
#define VDS_EC_EWS_FORM (-16)  /* not the fast form of "upload": the caller's own parser decides     */
#define VDS_EC_EWS_PING (-17)  /* a ping met in a batch: no device work, the caller sends its pong   */
/* AES-256-CBC decryption (symmetric_decrypt, private/symmetriccrypto_p.h); the reference reports both
 * as "EVP_CipherFinal_ex failed": */
#define VDS_EC_ECRYPT_LENGTH (-18)  /* a ciphertext of 0 bytes or not a multiple of 16 (OpenSSL: "wrong final block length") */
#define VDS_EC_ECRYPT_PADDING (-19) /* last byte not in 1..16, or the last n bytes not all n (OpenSSL: "bad decrypt")       */
/* inflate (kernel/vds_data/private/inflate_p.h: zlib's inflate); the reference reports the first as
 * "inflate failed" and the second not at all: */
#define VDS_EC_EINFLATE_DATA (-20)  /* what zlib answers Z_DATA_ERROR or Z_NEED_DICT to                     */
#define VDS_EC_EINFLATE_SHORT (-21) /* the input ends before the stream does; what it held has been delivered */
#define VDS_EC_EINFLATE_SPACE (-22) /* the plaintext would pass the output's capacity                        */
/* transaction-log blocks (vds_ec_txblock_*) */
#define VDS_EC_ETX_FORM (-23) /* not the canonical form of a block: the caller's own parser decides         */
#define VDS_EC_ETX_KEY (-24)  /* the writer's key id matches none of the given keys: the caller looks it up */

/* ----------------------------------------------------------------- flags */
/* write_padding = false in chunk_generator::write (chunk.h:79,273-278):
 * no trailer; the caller guarantees size % (k*cell) == 0.                  */
#define VDS_EC_F_NO_TRAILER 0x1u
/* Cell-array form (test path, chunk.h:206-224 and chunk.h:383-400): data is
 * an array of native-endian cells, no trailer, restore is not trimmed.     */
#define VDS_EC_F_CELLS 0x2u

#define VDS_EC_MAX_K 65535u

const char *vds_ec_strerror(int status);
int vds_ec_version(void);
/* Host staging contexts (pinned + device buffers and a stream per calling
 * thread and device) created so far, and how many of them sit idle in the
 * pool that exited threads return theirs to (diagnostics; host only).      */
int vds_ec_host_ctx_stats(uint64_t *created, uint64_t *pooled);
/* Number of HIP devices usable by the library (0 on a machine with none). */
int vds_ec_device_count(int *count);

/* Bytes chunk_generator<cell>::write appends for one replica
 * (chunk.h:248 expected_size + chunk.h:274 trailer).  cell_bytes = 1 | 2. */
uint64_t vds_ec_replica_size(unsigned cell_bytes, unsigned k, uint64_t size, unsigned flags);
/* Bytes chunk_restore<cell>::restore returns for replicas of replica_size
 * bytes with trailer `padding` (chunk.h:415-419).                           */
uint64_t vds_ec_restored_size(unsigned cell_bytes, unsigned k, uint64_t replica_size, uint16_t padding);

/* ---------------------------------------------------- field / matrix helpers
 * Replace gf_math<uint16_t>() / gf_math<uint8_t>() (gf.h:131-253),
 * chunk<cell>::generate_multipliers (chunk.h:183-194) and the
 * chunk_restore<cell> constructor (chunk.h:290-375).  Host-only, no GPU.   */
int vds_ec_gf16_tables(uint16_t *value2log, uint16_t *log2value); /* 65536 each */
int vds_ec_gf8_tables(uint8_t *value2log, uint8_t *log2value);    /* 256 each   */
int vds_ec_multipliers16(uint16_t k, uint16_t node, uint16_t *out);
int vds_ec_multipliers8(uint8_t k, uint8_t node, uint8_t *out);
/* out = V^{-1} (k*k, row-major) for V[i][c] = nodes[i]^c.  Returns
 * VDS_EC_ESINGULAR when two nodes coincide (the reference computes garbage
 * there: its validation is vds_assert, compiled out).        */
int vds_ec_inverse16(uint16_t k, const uint16_t *nodes, uint16_t *out);
int vds_ec_inverse8(uint8_t k, const uint8_t *nodes, uint8_t *out);

/* -------------------------------------------------------- device entry points
 * Encode `count` objects of `size` bytes each: object o at in + o*in_stride.
 * For each of the n replica ids, replica r_i of object o is written at
 * outs[i] + o*out_stride (outs is a HOST array of n device pointers) and
 * occupies vds_ec_replica_size(...) bytes.  Replaces n calls of
 * chunk_generator<uint16_t>(k, r_i).write(s, data, size) per object
 * (chunk.h:245-281; caller loops dht_network_client.cpp:75-77, :589-591).  */
int vds_ec_encode16_device(uint16_t k, const uint16_t *replicas, uint32_t n, const uint8_t *in,
                           uint64_t size, uint64_t in_stride, uint32_t count, uint8_t *const *outs,
                           uint64_t out_stride, unsigned flags, void *stream);
int vds_ec_encode8_device(uint8_t k, const uint8_t *replicas, uint32_t n, const uint8_t *in,
                          uint64_t size, uint64_t in_stride, uint32_t count, uint8_t *const *outs,
                          uint64_t out_stride, unsigned flags, void *stream);

/* Encode a batch of objects of DIFFERENT sizes -- the shape of the upload
 * loop: the web client deflates and encrypts each 64 KiB piece before
 * `upload`, so the bodies save_temp encodes (dht_network_client.cpp:62-107)
 * almost never have the same length.  Object o is sizes[o] bytes at ins[o];
 * replica replicas[i] of object o is written to outs[o*n + i] and occupies
 * vds_ec_replica_size(2, k, sizes[o], flags) bytes (ins, sizes, outs: HOST
 * arrays of `count` device pointers, `count` sizes and count*n device
 * pointers).  Bytes equal vds_ec_encode16_device called once per object,
 * zero-length objects (trailer only) and VDS_EC_F_NO_TRAILER included.
 * Every object with a non-zero size, a 4-byte aligned input and 2-byte
 * aligned replica pointers shares ONE bit-sliced launch when (k, n) is
 * (16,20), (32,40) or (32,64) and replicas is 0..n-1 -- whole groups, ragged
 * tails, partial last stripes and trailers alike; every other object takes
 * vds_ec_encode16_device's route, one call each, on the same stream.  Byte
 * API only: VDS_EC_F_CELLS is VDS_EC_EINVAL.  Every object is validated
 * before anything is enqueued, and before the device is looked for (null
 * pointers where a length is non-zero, k == 0, count >= 2^30,
 * VDS_EC_F_NO_TRAILER with a size that is not a multiple of 2k:
 * VDS_EC_EINVAL).  Nothing synchronises; the launch's tables ride the pinned
 * parameter ring.  Only bytes [ins[o], ins[o] + sizes[o]) are read and only
 * the replicas' own bytes are written.                                       */
int vds_ec_encode16_batch_device(uint16_t k, const uint16_t *replicas, uint32_t n, uint32_t count,
                                 const uint8_t *const *ins, const uint64_t *sizes, uint8_t *const *outs,
                                 unsigned flags, void *stream);
/* The route vds_ec_encode16_batch_device takes for these arguments (host only,
 * nothing is dereferenced but the host arrays; the planning is shared with
 * the call itself): 2 when at least one object rides the shared bit-sliced
 * launch, else 1 (invalid arguments too).  *fast_objects (may be NULL)
 * receives the number of objects that ride it.                               */
int vds_ec_encode16_batch_path(uint16_t k, const uint16_t *replicas, uint32_t n, uint32_t count,
                               const uint8_t *const *ins, const uint64_t *sizes, uint8_t *const *outs,
                               unsigned flags, uint32_t *fast_objects);

/* Restore `count` objects from k replicas each: replica j (id nodes[j]) of
 * object o at chunks[j] + o*chunk_stride (chunks: HOST array of k device
 * pointers), chunk_size bytes each (trailer included).  The restored object
 * o is written at out + o*out_stride; its size (identical for all objects,
 * taken from the trailer of object 0's first chunk ON THE HOST -- so the
 * caller passes it in `padding`) is vds_ec_restored_size(...).  Replaces
 * chunk_restore<uint16_t>(k, nodes).restore(chunks) (chunk.h:290-444;
 * caller dht_network_client.cpp:887-888).                                   */
int vds_ec_restore16_device(uint16_t k, const uint16_t *nodes, const uint8_t *const *chunks,
                            uint64_t chunk_size, uint64_t chunk_stride, uint16_t padding,
                            uint32_t count, uint8_t *out, uint64_t out_stride, unsigned flags,
                            void *stream);
int vds_ec_restore8_device(uint8_t k, const uint8_t *nodes, const uint8_t *const *chunks,
                           uint64_t chunk_size, uint64_t chunk_stride, uint16_t padding,
                           uint32_t count, uint8_t *out, uint64_t out_stride, unsigned flags,
                           void *stream);

/* Regenerate lost replicas from k survivors without materialising the object
 * (SURVEY.md 8(f) row 3).  The reference's repair restores the object and
 * re-encodes it (sync_process.cpp:313-335 -> restore_async + save_data,
 * dht_network_client.cpp:582-658); replica t is P(t) stripe by stripe, so one
 * pass over the survivors yields it directly.  Survivor j (id nodes[j]) of
 * object o at chunks[j] + o*chunk_stride (HOST array of k device pointers,
 * chunk_size bytes = cells + BE16 trailer); replica targets[i] of object o is
 * written to outs[i] + o*out_stride (chunk_size bytes, trailer included).
 * Bytes equal chunk_generator(k, t).write(restore(...)) -- the reference's
 * route, restored object trimmed to E bytes, last stripe zero-padded, trailer
 * E mod 2k -- for ANY survivors, codeword or not, whose first chunk's trailer
 * p is at most 2k.  For p > 2k that route has no chunk_size-byte answer (it
 * fails, or re-encodes to chunk_size + 2 bytes): the *_host forms return
 * VDS_EC_ERESTORE, the device forms leave those objects' replicas unspecified. */
int vds_ec_regenerate16_device(uint16_t k, const uint16_t *nodes, const uint8_t *const *chunks, uint64_t chunk_size,
                               uint64_t chunk_stride, uint32_t count, const uint16_t *targets, uint32_t ntargets,
                               uint8_t *const *outs, uint64_t out_stride, void *stream);

/* Batched restore / regenerate with a survivor set, size and output PER
 * OBJECT -- the shape of the download and repair loops (restore_async takes
 * the first k replicas found for each object, dht_network_client.cpp:851-901;
 * sync_process repairs object by object, sync_process.cpp:313-335).  Object
 * o's survivor j (replica id nodes[o*k + j]) is at chunks[o*k + j] (HOST
 * array of count*k device pointers), chunk_sizes[o] bytes (trailer included);
 * paddings[o] is its trailer value (the caller has it: the chunks came from
 * files or sockets).  Restore writes vds_ec_restored_size(2, k,
 * chunk_sizes[o], paddings[o]) bytes to outs[o].  Regenerate writes replica
 * targets[o*nt + i] (chunk_sizes[o] bytes, trailer included) to
 * outs[o*nt + i].  Objects whose survivors lie within the syndrome kernel's
 * points (k in {16, 32}, ids < k + k/4) share ONE launch, those with other
 * ids below 256 (same k) one runtime-coefficient launch; the rest take one
 * launch each.  Every object is validated before anything is enqueued
 * (pointers, lengths, distinct ids: VDS_EC_ESINGULAR otherwise); nothing
 * synchronises.  count < 2^30 (VDS_EC_EINVAL otherwise).  Regenerate bytes as
 * vds_ec_regenerate16_device.  To regenerate, name (save_data,
 * sync_process.cpp:313-335) and check the replicas in one call, use
 * vds_ec_repair16_batch_device below.                                         */
int vds_ec_restore16_batch_device(uint16_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                                  const uint64_t *chunk_sizes, const uint16_t *paddings, uint8_t *const *outs,
                                  unsigned flags, void *stream);
int vds_ec_regenerate16_batch_device(uint16_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                                     const uint64_t *chunk_sizes, uint32_t ntargets, const uint16_t *targets,
                                     uint8_t *const *outs, void *stream);

/* ---------------------------------------------------------- host entry points
 * Same operations on host memory (pinned staging, H2D -> kernel -> D2H on
 * the calling thread's current device).  outs: n host buffers of
 * vds_ec_replica_size(...) bytes.  This is what chunk_generator::write and
 * chunk_storage::generate_replica (chunk_storage.cpp:41-60) call.            */
int vds_ec_encode16_host(uint16_t k, const uint16_t *replicas, uint32_t n, const uint8_t *data,
                         uint64_t size, uint8_t *const *outs, unsigned flags);
int vds_ec_encode8_host(uint8_t k, const uint8_t *replicas, uint32_t n, const uint8_t *data,
                        uint64_t size, uint8_t *const *outs, unsigned flags);
/* chunks: k host buffers of chunk_size bytes; out must hold chunk_size*k
 * bytes (the most the reference's loop can produce: (chunk_size-2)*k for a
 * well-formed trailer, more when the trailer is corrupt); *out_size
 * receives the restored length (chunk.h:402-444, chunk_storage.cpp:62-86). */
int vds_ec_restore16_host(uint16_t k, const uint16_t *nodes, const uint8_t *const *chunks,
                          uint64_t chunk_size, uint8_t *out, uint64_t *out_size, unsigned flags);
int vds_ec_restore8_host(uint8_t k, const uint8_t *nodes, const uint8_t *const *chunks,
                         uint64_t chunk_size, uint8_t *out, uint64_t *out_size, unsigned flags);

/* Host-memory form of vds_ec_regenerate16_device: chunks are k host buffers
 * of chunk_size bytes, outs ntargets host buffers of chunk_size bytes.      */
int vds_ec_regenerate16_host(uint16_t k, const uint16_t *nodes, const uint8_t *const *chunks, uint64_t chunk_size,
                             const uint16_t *targets, uint32_t ntargets, uint8_t *const *outs);

/* Batched host-memory encode across every visible GPU (one host thread,
 * pinned ring and stream pair per device; object o -> device o % devices).
 * objs[o] has sizes[o] bytes; replica i of object o goes to outs[o*n + i].
 * This is the save_temp / save_data formulation.    */
int vds_ec_encode16_host_batch(uint16_t k, const uint16_t *replicas, uint32_t n,
                               const uint8_t *const *objs, const uint64_t *sizes, uint32_t count,
                               uint8_t *const *outs, unsigned flags, int max_devices);

/* Batched host-memory restore across every visible GPU (the restore side of
 * the batch above; chunk_storage::restore_data, chunk_storage.cpp:62-85, per
 * object).  Object o is restored from the k host chunks chunks[o*k + j] of
 * chunk_sizes[o] bytes holding replicas nodes[o*k + j]; on entry out_sizes[o]
 * is the capacity of outs[o], on success the restored length (trailer-trimmed
 * as vds_ec_restore16_host).  Every object is validated before any transfer. */
int vds_ec_restore16_host_batch(uint16_t k, const uint16_t *nodes, const uint8_t *const *chunks,
                                const uint64_t *chunk_sizes, uint32_t count, uint8_t *const *outs, uint64_t *out_sizes,
                                unsigned flags, int max_devices);

/* Caller-owned pinned memory for the host batches (the
 * path starts and ends in host memory).  vds_ec_host_alloc returns
 * page-locked, device-mapped memory usable from every device;
 * vds_ec_host_register pins (and maps) a caller's existing range for as long
 * as it stays registered.  When a host batch group's objects -- or replicas,
 * survivors, restored objects -- lie back to back in one such range (the
 * slab layouts: objects [count][size], replicas [count][n][L], survivors
 * [count][k][chunk_size], restored objects [count][E]), the H2D DMA reads the
 * caller's bytes and the results are written into the caller's pages by the
 * device: no staging copies in host memory.  Anything else is staged as
 * before.  Free / unregister only when no call using the range is running. */
int vds_ec_host_alloc(uint64_t bytes, void **ptr);
int vds_ec_host_free(void *ptr);
int vds_ec_host_register(void *ptr, uint64_t bytes);
int vds_ec_host_unregister(void *ptr);

/* ---------------------------------------------------- stripe-range split
 * One object split by stripe range [t0, t1), e.g. over GPUs.
 * Cell t of every replica depends on stripe t alone, so the ranges are
 * independent.  encode: in = the whole object (device, size bytes); writes
 * replica bytes [2 t0, 2 t1) of outs[i] (whole replica buffers), and the
 * trailer with the range that ends at T = ceil(size / 2k).  t0 < t1 <= T
 * (T == 0: the range [0, 0), trailer only).  restore: chunks = the whole
 * survivor buffers, padding = their trailer value; writes object bytes
 * [2k t0, min(2k t1, E)) of out for t1 <= ceil(E / 2k) (E =
 * vds_ec_restored_size).  Byte API only (no VDS_EC_F_CELLS).                */
int vds_ec_encode16_range_device(uint16_t k, const uint16_t *replicas, uint32_t n, const uint8_t *in, uint64_t size,
                                 uint64_t t0, uint64_t t1, uint8_t *const *outs, unsigned flags, void *stream);
int vds_ec_restore16_range_device(uint16_t k, const uint16_t *nodes, const uint8_t *const *chunks, uint64_t chunk_size,
                                  uint16_t padding, uint64_t t0, uint64_t t1, uint8_t *out, unsigned flags,
                                  void *stream);
/* One host object over several GPUs: its stripes in `parts` ranges of whole
 * 2048-stripe tiles (0 = one per device), range r on device r % devices, each
 * with its own PCIe link.  Same arguments and results as
 * vds_ec_encode16_host / vds_ec_restore16_host (out_size: capacity in,
 * restored length out).                                                     */
int vds_ec_encode16_host_split(uint16_t k, const uint16_t *replicas, uint32_t n, const uint8_t *data, uint64_t size,
                               uint8_t *const *outs, unsigned flags, int max_devices, uint32_t parts);
int vds_ec_restore16_host_split(uint16_t k, const uint16_t *nodes, const uint8_t *const *chunks, uint64_t chunk_size,
                                uint8_t *out, uint64_t *out_size, unsigned flags, int max_devices, uint32_t parts);

/* ---------------------------------------------------------- replica names
 * The reference names each replica by SHA-256 of its bytes (save_temp /
 * save_data: dht_network_client.cpp:79, :593 -> hash::signature(sha256),
 * kernel/vds_crypto/hash.cpp:91-101, OpenSSL EVP_sha256).  Digests of count
 * device messages of len bytes at base + j*stride (any alignment) go to
 * digests + 32*j (device memory).                                             */
int vds_ec_sha256_device(const uint8_t *base, uint64_t len, uint64_t stride, uint32_t count, uint8_t *digests,
                         void *stream);
/* SHA-256 of messages of DIFFERENT lengths in ONE launch -- the names of a
 * ragged upload batch, whose replicas differ in length from object to object:
 * message j is lens[j] bytes at msgs[j] (msgs, lens: HOST arrays of `count`
 * device pointers and lengths; any alignment; lens[j] == 0 allows msgs[j] ==
 * NULL), digest j goes to digests + 32*j (device).  One lane per message;
 * the launch's tables ride the pinned parameter ring, the lanes are ordered by
 * length on the host (a wave runs as long as its longest message) and every
 * digest still lands at the caller's index.  Every argument is validated
 * before anything is enqueued and before the device is looked for (null
 * arrays, a null message with a non-zero length, count >= 2^30:
 * VDS_EC_EINVAL); count == 0 is VDS_EC_OK.  Nothing synchronises.  Only the
 * aligned 4-byte words holding at least one message byte are read (none for
 * an empty message) and only the digests' own bytes are written.             */
int vds_ec_sha256_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens,
                               uint8_t *digests, void *stream);
/* SHA-256 of ONE host message on the calling thread (no GPU): upload_data's
 * body hash (server_api.cpp:16) is a single chain of dependent compressions,
 * ~3 us a block in one GPU lane, so vds_ec_save_temp16_host computes it here
 * while the device encodes and names the replicas.  x86 SHA extensions when
 * the CPU has them, else portable code (FIPS 180-4 6.2).                     */
int vds_ec_sha256_host(const uint8_t *data, uint64_t len, uint8_t *digest);
/* vds_ec_encode16_host plus the SHA-256 of every replica, computed on the
 * device before the copy-back: digests receives n*32 bytes (host).          */
int vds_ec_encode16_hash_host(uint16_t k, const uint16_t *replicas, uint32_t n, const uint8_t *data, uint64_t size,
                              uint8_t *const *outs, uint8_t *digests, unsigned flags);

/* Content-addressed storage path of a replica from its SHA-256 name (host,
 * no GPU): base64 (standard alphabet, '=' padding, encoding.cpp:136-174) with
 * '+' -> '#' and '/' -> '_', split as chars [0,10) "/" [10,20) "/" [20,44)
 * (dht_network_client.cpp:483-505, :632-653).  out receives count
 * NUL-terminated paths of VDS_EC_PATH_BYTES bytes each.                     */
#define VDS_EC_PATH_BYTES 48
int vds_ec_replica_paths(const uint8_t *digests, uint32_t count, char *out);

/* ------------------------------------------- upload path
 * The live upload: websocket "upload" with a base64 body
 * (websocket_api.cpp:141-155) -> server_api::upload_data (server_api.cpp:12-30:
 * data hash = SHA-256 of the body) -> _client::save_temp
 * (dht_network_client.cpp:62-107: replicas 0..n-1 written, each named by its
 * SHA-256 and kept as <root>/tmp/<tmp name>) -> the JSON answer
 * (websocket_api.cpp:467-485).  Host code except vds_ec_save_temp16_host,
 * which runs the encode and every hash on the current device.              */
/* base64::to_bytes with its quirks (see vds_ec_wire.cpp); *out_len receives
 * vds_ec_base64_decoded_size(in, len) bytes written to out.                 */
size_t vds_ec_base64_decoded_size(const char *in, size_t len);
int vds_ec_base64_decode(const char *in, size_t len, uint8_t *out, size_t *out_len);
/* base64::from_bytes; out == NULL queries the length (excluding the NUL). */
int vds_ec_base64_encode(const uint8_t *in, size_t len, char *out, size_t cap, size_t *out_len);
/* save_temp's tmp-file names: base64 of each digest with '+' -> '#' and
 * '/' -> '_' (dht_network_client.cpp:91-95), NUL-terminated, 45 bytes each. */
#define VDS_EC_NAME_BYTES 45
int vds_ec_tmp_names(const uint8_t *digests, uint32_t count, char *out);
/* The "upload" answer {"id":..,"result":{"replicas":[..],"hash":..,
 * "replica_size":..}} exactly as json_writer serialises it; out == NULL
 * queries the length (excluding the NUL).                                   */
int vds_ec_upload_response_json(int id, const uint8_t *replica_digests, uint32_t n, const uint8_t *data_digest,
                                 uint32_t replica_size, char *out, size_t cap, size_t *out_len);
/* save_temp + upload_data's hashing: replicas 0..n-1 of the body (host,
 * size bytes) into outs (n host buffers of vds_ec_replica_size bytes), their
 * SHA-256 names into replica_digests (n*32 host bytes) -- encode and names on
 * the device --, the body's SHA-256 into data_digest (32 host bytes),
 * computed on the calling thread meanwhile (vds_ec_sha256_host).            */
int vds_ec_save_temp16_host(uint16_t k, uint32_t n, const uint8_t *data, uint64_t size, uint8_t *const *outs,
                            uint8_t *replica_digests, uint8_t *data_digest, uint32_t *replica_size);

/* save_temp / save_data for a BATCH of bodies of different sizes (the upload
 * loop: dht_network_client.cpp:62-107, :582-658): vds_ec_encode16_batch_device
 * with replicas 0..n-1 and trailers -- the same planning, the same bytes, the
 * objects that route to vds_ec_encode16_device included --, then replica i of
 * object o named at replica_digests + 32*(o*n + i) (device, count*n*32 bytes)
 * and, when data_digests != NULL, the body's SHA-256 (upload_data,
 * server_api.cpp:16) at data_digests + 32*o (device).  ins, sizes, outs: HOST
 * arrays as vds_ec_encode16_batch_device takes them.  Every hash of the call,
 * whatever route an object's encode took, rides ONE vds_ec_sha256_batch_device
 * style launch after the encode; the body chains, the longest, come first in
 * its block order.  Every argument is validated before anything is enqueued
 * and before the device is looked for (null arrays with count > 0, null
 * replica_digests with count*n > 0, a null pointer where a length is
 * non-zero, k == 0, n > 65536, count >= 2^30, count*(n + 64) >= 2^32:
 * VDS_EC_EINVAL); count == 0 is VDS_EC_OK.  Nothing synchronises.  Only the
 * replicas' and the digests' own bytes are written.                          */
int vds_ec_save_temp16_batch_device(uint16_t k, uint32_t n, uint32_t count, const uint8_t *const *ins,
                                    const uint64_t *sizes, uint8_t *const *outs, uint8_t *replica_digests,
                                    uint8_t *data_digests, void *stream);
/* The same from and to host memory on the calling thread's current device:
 * bodies objs[o] (sizes[o] bytes), replicas to outs[o*n + i]
 * (vds_ec_replica_size(2, k, sizes[o], 0) bytes each), names to
 * replica_digests (count*n*32 host bytes), body hashes to data_digests
 * (count*32 host bytes; may be NULL), replica_sizes[o] (may be NULL) =
 * vds_ec_replica_size(2, k, sizes[o], 0).  Works through groups of at most
 * 64 MiB of bodies: gathered into pinned staging, one copy to the device, the
 * batch call above, one copy back of replicas and digests, scattered to the
 * caller's buffers.  One device; validation as above.                       */
int vds_ec_save_temp16_host_batch(uint16_t k, uint32_t n, uint32_t count, const uint8_t *const *objs,
                                  const uint64_t *sizes, uint8_t *const *outs, uint8_t *replica_digests,
                                  uint8_t *data_digests, uint32_t *replica_sizes);

/* ------------------------------------------- wire text on the device
 * The bodies of "upload" arrive as base64 and "download" answers in base64
 * (websocket_api.cpp:141-155, :193); vds_ec_base64_decode / _encode above walk
 * one text a character at a time on the calling thread, which costs more than
 * everything save_temp does after it.  These decode and encode a BATCH of
 * texts of different lengths in ONE launch each.
 * Decode: text o is text_lens[o] characters at texts[o], its bytes go to
 * outs[o] (texts, text_lens, outs, out_sizes: HOST arrays of `count`; the
 * texts and outputs are device memory, any alignment -- the fast path is a
 * 16-byte aligned text and a 4-byte aligned output).  out_sizes[o] is what
 * vds_ec_base64_decoded_size gives for the text: the caller had the text in
 * host memory before copying it over, and needs that size to allocate.
 * statuses[o] (device, `count` int32_t) receives what vds_ec_base64_decode
 * returns for the text -- VDS_EC_OK, VDS_EC_EB64_LENGTH, VDS_EC_EB64_PADDING,
 * VDS_EC_EB64_CHAR, quirks as there: the first '=' ends the decode, the bytes
 * it leaves unwritten are zero -- or VDS_EC_EINVAL when out_sizes[o] disagrees
 * with the '=' among the text's last two characters (its output untouched).
 * With VDS_EC_OK all out_sizes[o] bytes equal the host function's; with any
 * other status the contents of the output are unspecified; either way no byte
 * outside [outs[o], outs[o] + out_sizes[o]) is written, and only the aligned
 * 4-byte words holding a character of a text are read.  Every status is
 * written by the launch.  One wave walks one message (a text of many MiB is
 * slow; the shape that matters is bodies of up to 64 KiB by the thousand); the
 * descriptors ride the pinned parameter ring, longest message first.
 * Every argument is validated before anything is enqueued and before the
 * device is looked for (null arrays with count > 0, a null text or output
 * where a length is non-zero, count >= 2^30, text_lens[o] >= 2^32,
 * out_sizes[o] not one of len/4*3 - p for p = 0, 1, 2 or non-zero when
 * len % 4 != 0: VDS_EC_EINVAL); count == 0 is VDS_EC_OK.  Nothing
 * synchronises.                                                              */
int vds_ec_base64_decode_batch_device(uint32_t count, const char *const *texts, const uint64_t *text_lens,
                                      uint8_t *const *outs, const uint64_t *out_sizes, int32_t *statuses,
                                      void *stream);
/* Encode (base64::from_bytes: standard alphabet, '=' padding, no NUL): input o
 * is lens[o] bytes at ins[o], outs[o] receives (lens[o] + 2) / 3 * 4
 * characters; same conventions (HOST arrays of device pointers, any alignment,
 * only the outputs' own bytes written; lens[o] >= 2^32 or more than 2^31 - 1
 * tiles of 6 KiB over the batch: VDS_EC_EINVAL).  Tiled over the whole batch,
 * so a long input is split across waves.  In the download loop it follows
 * vds_ec_restore16_batch_device on the same stream.                          */
int vds_ec_base64_encode_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                      char *const *outs, void *stream);
/* vds_ec_save_temp16_host_batch fed with TEXTS: text o (host, text_lens[o]
 * characters of base64) is decoded on the device and its body encoded and
 * named as there.  statuses[o] (host, required) receives the text's
 * vds_ec_base64_decode status.  A message whose status is non-zero has none of
 * its outputs written -- replicas outs[o*n + i], names, body hash,
 * replica_sizes[o], bodies[o], body_sizes[o] --; *failed counts them; the call
 * itself returns VDS_EC_OK.  bodies (when non-NULL: count host buffers of
 * vds_ec_base64_decoded_size bytes) receive the decoded bodies, body_sizes
 * their sizes.  replica_sizes, bodies, body_sizes, data_digests and failed may
 * be NULL.  Works through groups of at most 64 MiB of text: texts gathered at
 * 16-byte aligned offsets of pinned staging, one copy to the device, the
 * decode launch into 16-byte aligned bodies, vds_ec_save_temp16_batch_device
 * on those, one copy back of replicas, names, body hashes, statuses and (when
 * asked for) bodies, scattered to the caller.  Sizes come from the host texts,
 * so nothing waits for the decode; a text whose length is no multiple of 4
 * gets no device work.  One device (the calling thread's current one);
 * validation as the decode's and save_temp's, every message before any
 * transfer.                                                                  */
int vds_ec_upload16_host_batch(uint16_t k, uint32_t n, uint32_t count, const char *const *texts,
                               const uint64_t *text_lens, uint8_t *const *outs, uint8_t *replica_digests,
                               uint8_t *data_digests, uint32_t *replica_sizes, uint8_t *const *bodies,
                               uint64_t *body_sizes, int32_t *statuses, uint32_t *failed);

/* ------------------------------------------- repair loop and the name check
 * As vds_ec_sha256_batch_device, and message j's digest compared with
 * expected + 32*j (device, any alignment): verdicts[j] = 0 equal / 1
 * different (device, count bytes).  digests may be NULL (check only: no digest
 * is written).  Validation as vds_ec_sha256_batch_device, and null expected or
 * verdicts with count > 0: VDS_EC_EINVAL.  Nothing synchronises.  The
 * comparison rides the hash launch (each lane compares its own state words
 * after its last block), so a check costs no copy-back of digests and no host
 * loop.
 * The download loop: the request carries every replica's name
 * (websocket_api.cpp:193), restore_async reads the replica files by name
 * (dht_network_client.cpp:873) and decodes them WITHOUT hashing them -- the
 * hash check of read_data (:952-960, "Data is corrupted") is not on that path.
 * This call over the k survivors of every object (digests == NULL), enqueued
 * beside vds_ec_restore16_batch_device, is that missing check.               */
int vds_ec_sha256_check_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens,
                                     const uint8_t *expected, uint8_t *digests, uint8_t *verdicts, void *stream);

/* The repair loop (sync_process.cpp:313-335 -> restore_async -> save_data,
 * dht_network_client.cpp:582-658) for a batch: vds_ec_regenerate16_batch_device
 * (same arguments, same planning, same bytes, every route), then ONE hash
 * launch naming replica targets[o*nt + i] of object o at digests +
 * 32*(o*nt + i) (device, count*nt*32 bytes) and, when expected != NULL,
 * comparing it with expected + 32*(o*nt + i) (device; the names the catalogue
 * holds, chunk_replica_data_dbo.replica_hash) into verdicts[o*nt + i] (device,
 * count*nt bytes: 0 equal, 1 different).  With expected == NULL verdicts must
 * be NULL too and nothing is compared.
 * What the check covers: EVERY CELL OF EVERY SURVIVOR and the FIRST survivor's
 * trailer.  The code is MDS: changing any cell of any of the k survivors
 * changes that stripe's cell in every other replica, so every regenerated
 * replica's name then differs from the catalogue's and every verdict of the
 * object is 1 -- without hashing the survivors themselves.  The reference
 * route reads no trailer but the first survivor's (chunk.h:408), so a wrong
 * trailer on survivor 2..k leaves every regenerated replica, and every
 * verdict, unchanged.
 * Every argument is validated before anything is enqueued and before the
 * device is looked for: the checks of vds_ec_regenerate16_batch_device
 * (VDS_EC_ESINGULAR for repeated ids included), and null digests with
 * count*ntargets > 0, expected and verdicts not both NULL or both non-NULL,
 * count*(ntargets + 64) >= 2^32 (the hash launch's lanes): VDS_EC_EINVAL.
 * count == 0 or ntargets == 0 is VDS_EC_OK.  Nothing synchronises.  Only the
 * replicas', digests' and verdicts' own bytes are written.                   */
int vds_ec_repair16_batch_device(uint16_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                                 const uint64_t *chunk_sizes, uint32_t ntargets, const uint16_t *targets,
                                 uint8_t *const *outs, uint8_t *digests, const uint8_t *expected,
                                 uint8_t *verdicts, void *stream);
/* The same from and to host memory on the calling thread's current device:
 * survivors chunks[o*k + j] (chunk_sizes[o] host bytes), replicas to
 * outs[o*nt + i] (chunk_sizes[o] bytes), names to digests (count*nt*32 host
 * bytes), expected (host, may be NULL) against them into verdicts (count*nt
 * host bytes); *mismatches (may be NULL) receives the number of non-zero
 * verdicts, 0 when expected is NULL.  Works through groups of at most 64 MiB
 * of survivor bytes (a larger object is a group of its own): gathered into
 * pinned staging with the expected names, one copy to the device, the call
 * above, one copy back of replicas, names and verdicts, scattered to the
 * caller.  Validation as above, every object before any transfer; and, the
 * host having the trailers, an object whose first chunk's trailer exceeds 2k
 * fails the whole call with VDS_EC_ERESTORE as vds_ec_regenerate16_host does. */
int vds_ec_repair16_host_batch(uint16_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                               const uint64_t *chunk_sizes, uint32_t ntargets, const uint16_t *targets,
                               uint8_t *const *outs, uint8_t *digests, const uint8_t *expected,
                               uint8_t *verdicts, uint32_t *mismatches);

/* ------------------------------------------------------------ download loop
 * vds_ec_base64_encode_batch_device behind a gate: message o also carries
 * gates[o] (device, ngates[o] verdict bytes of an earlier launch on the same
 * stream, any alignment; ngates[o] == 0: ungated, gates[o] not read) and the
 * status slot statuses + o (device, `count` int32_t).  A wave ORs the
 * message's gate bytes before it writes anything; with any of them non-zero
 * NO character of the message is written and its status is VDS_EC_ECORRUPT,
 * else the text is the ungated call's and the status VDS_EC_OK.  Every status
 * is written by the launch, a message of length 0 included.  Conventions and
 * validation as the ungated call's (every message counts at least one tile),
 * and null gates, ngates or statuses with count > 0, a null gates[o] where
 * ngates[o] != 0: VDS_EC_EINVAL.  Nothing synchronises; stream order is the
 * only ordering between the launch that wrote the gate bytes and this one.   */
int vds_ec_base64_encode_gated_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                            char *const *outs, const uint8_t *const *gates, const uint32_t *ngates,
                                            int32_t *statuses, void *stream);
/* The download loop (websocket_api.cpp:191-210 -> restore_async,
 * dht_network_client.cpp:851-901 -> the base64 answer, websocket_api.cpp:772-782)
 * for a batch, CHECKED: on the one stream, in this order,
 *   1. the check of the names the request carries (websocket_api.cpp:193),
 *   2. vds_ec_restore16_batch_device into objects[o] (same arguments, same
 *      planning, same bytes, every route),
 *   3. one gated encode of object o's E = vds_ec_restored_size(2, k,
 *      chunk_sizes[o], paddings[o]) bytes into (E + 2) / 3 * 4 characters at
 *      texts[o] (device, any alignment), gated by the object's verdict bytes:
 *      statuses[o] (device, `count` int32_t) is VDS_EC_OK and the text is
 *      written, or VDS_EC_ECORRUPT and no character of it is.
 * HOST arrays of device pointers, as vds_ec_restore16_batch_device takes them.
 * Exactly one check is given (both or neither: VDS_EC_EINVAL):
 *   SURVIVOR MODE, survivor_names != NULL (device, count*k*32 bytes, the name
 *   of survivor chunks[o*k + j] at 32*(o*k + j)):
 *   vds_ec_sha256_check_batch_device's launch over the count*k survivors
 *   (check only; planned as one group an object, 1/k of the descriptors);
 *   verdicts (device) holds count*k bytes, object o's gate is its k bytes.
 *   Covers EVERY BYTE OF EVERY SURVIVOR, trailers included -- stricter than
 *   the reference's route, which reads the first survivor's trailer only.
 *   WITNESS MODE, witness_ids (HOST, count ids), witness_names (device,
 *   count*32) and witness_outs (HOST array of count device buffers of
 *   chunk_sizes[o] bytes) all given: replica witness_ids[o] of object o -- one
 *   that is not among its survivors -- is regenerated into witness_outs[o] and
 *   its name compared with witness_names + 32*o, the two launches of
 *   vds_ec_repair16_batch_device with ntargets = 1 (the witness's digest is
 *   compared inside the hash launch and stored nowhere); verdicts holds count
 *   bytes, object o's gate is its one byte.  Covers EVERY CELL OF EVERY
 *   SURVIVOR and the FIRST survivor's trailer: the code is MDS, so changing
 *   any cell of any of the k survivors changes that stripe's cell in every
 *   other replica, the witness included -- at 1/k of the hashing.  The
 *   reference route reads no trailer but the first survivor's (chunk.h:408),
 *   so a wrong trailer on survivor 2..k leaves the witness, the verdict and
 *   the restored object unchanged.  Of a partial last stripe the route keeps
 *   the object's own bytes only (chunk.h:415-419): a changed cell there whose
 *   decode differs in the trimmed bytes alone regenerates the same witness
 *   and restores the same object, and passes with the exact text (survivor
 *   mode fails it: the file is not the named one).  A first trailer above 2k leaves the
 *   witness unspecified (see vds_ec_regenerate16_device); a valid upload never
 *   has one (p = S mod 2k), and the host form below handles it.
 * Every argument is validated before anything is enqueued and before the
 * device is looked for: restore's checks (VDS_EC_ERESTORE, VDS_EC_ESINGULAR
 * included), the name check's, with a witness repair's (chunk sizes of whole
 * cells and a trailer, VDS_EC_ESINGULAR whatever the size) and a witness id
 * equal to one of its object's survivor ids (VDS_EC_EINVAL); null arrays with
 * count > 0, a null objects[o] or texts[o] where E != 0, E >= 2^32,
 * count >= 2^30, count*(k + 64) >= 2^32 (survivor mode) or count*65 >= 2^32
 * (witness mode; the hash launch's lanes): VDS_EC_EINVAL.  count == 0 is VDS_EC_OK.  Nothing synchronises.
 * Only the objects', texts', witnesses', verdicts' and statuses' own bytes
 * are written.                                                               */
int vds_ec_download16_batch_device(uint16_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                                   const uint64_t *chunk_sizes, const uint16_t *paddings,
                                   const uint8_t *survivor_names, const uint16_t *witness_ids,
                                   const uint8_t *witness_names, uint8_t *const *witness_outs,
                                   uint8_t *const *objects, char *const *texts, uint8_t *verdicts, int32_t *statuses,
                                   void *stream);
/* The same from and to host memory on the calling thread's current device:
 * survivors chunks[o*k + j] (chunk_sizes[o] host bytes; whole cells and a
 * trailer), their names survivor_names (host, count*k*32, REQUIRED in both
 * modes), and, for witness mode, witness_ids and witness_names (host, count
 * ids and count*32 bytes; both NULL: survivor mode).  texts[o] (host) receives
 * the base64 text, text_lens[o] holds its capacity on entry (less than the
 * text needs: VDS_EC_EINVAL) and its length on return; statuses[o] (host,
 * count) the object's status; survivor_verdicts (host, count*k bytes) which
 * survivors' names did not match.  A failed object's text is untouched and
 * its text_lens[o] is 0; *failed (may be NULL) counts them; the call itself
 * returns VDS_EC_OK.  Paddings come from the first chunk's trailer.
 * Works through groups of at most 64 MiB of survivor bytes: survivors
 * gathered into pinned staging with the names, one copy to the device, the
 * call above, one copy back of texts and statuses (and, in survivor mode, the
 * gate, which is survivor_verdicts).  In witness mode the survivors of the
 * objects whose status came back non-zero, still on the device, get one more
 * vds_ec_sha256_check_batch_device launch, theirs alone, which LOCATES the
 * rotten file: their survivor_verdicts come from it (all zero: the names
 * match and the first trailer is wrong within 2k, or the witness's name is);
 * objects that passed get zeros.  An object whose first trailer has no answer
 * gets no restore and goes straight to that pass: above 2k in witness mode
 * (VDS_EC_ECORRUPT), restore's "Fatal error" in survivor mode
 * (VDS_EC_ERESTORE).  Validation as above, every object before any transfer.  */
int vds_ec_download16_host_batch(uint16_t k, uint32_t count, const uint16_t *nodes, const uint8_t *const *chunks,
                                 const uint64_t *chunk_sizes, const uint8_t *survivor_names,
                                 const uint16_t *witness_ids, const uint8_t *witness_names, char *const *texts,
                                 uint64_t *text_lens, int32_t *statuses, uint8_t *survivor_verdicts,
                                 uint32_t *failed);

/* ------------------------------------------------ node-to-node transport
 * A replica crosses between nodes as a sync_replica_data message
 * (sync_process.cpp:184-191, messages/sync_messages.h:311-330) that
 * dht_datagram_protocol::prepare_to_send (impl/dht_datagram_protocol.cpp:335-541)
 * cuts into datagrams of at most mtu bytes, each signed with HMAC-SHA256
 * (RFC 2104, OpenSSL's HMAC: kernel/vds_crypto/hash.cpp:218-260) under the
 * 32-byte session key (udp_transport.cpp:275-276); the receiver verifies each
 * (:130-141) and stitches the payloads together (:544-769).  These calls seal
 * and open a ragged BATCH of messages in one launch each way.  Acknowledgment,
 * resend, MTU probing, the handshake, the sockets and message dispatch stay
 * with the caller: this layer takes and returns datagram bytes.
 *
 * Wire format (integers big-endian; R = the route blob of r bytes: r = 0
 * direct, 32 the target id, 33 + 32 h target || h || h hop ids; M = the message
 * of m bytes; i0 = the message's first datagram index; type < 32):
 *   37 + r + m < mtu:  one datagram  B0 || BE32(i0) || R || M || MAC(all before),
 *                      B0 = type | 0x20 (r = 0), 0x60 (r = 32), 0xA0 (proxy);
 *   else the first is  B0 || BE32(i0) || BE32(m) || R || M[0, c0) || MAC with
 *                      B0 = type | 0x40 / 0x80 / 0xC0 and c0 = mtu - (41 + r)
 *                      (exactly mtu bytes), and continuation j = 1, 2, .. is
 *                      0x03 || BE32(i0 + j) || the next min(mtu - 37, rest)
 *                      bytes || MAC.
 *
 * HMAC-SHA256 of ONE host message on the calling thread (no GPU), any key
 * length (a key longer than 64 bytes is hashed first), on
 * vds_ec_sha256_host's compression.                                          */
int vds_ec_hmac_sha256_host(const uint8_t *key, uint64_t key_len, const uint8_t *data, uint64_t len, uint8_t *mac);
/* The sealing rules as host arithmetic (no GPU): *count datagrams, the first
 * carrying *first_payload message bytes, the last *last_len bytes long in all
 * (every other one is mtu bytes); any of the three may be NULL.  508 <= mtu <=
 * 65535, route_len one of the three forms above (h < 256), 41 + route_len <
 * mtu, msg_len < 2^32: VDS_EC_EINVAL otherwise.                              */
int vds_ec_dgram_layout(uint32_t mtu, uint32_t route_len, uint64_t msg_len, uint32_t *count, uint32_t *first_payload,
                        uint32_t *last_len);
/* binary_serializer::write_number (binary_serialize.cpp:44-66), the length
 * prefix of a serialized buffer: out receives *len <= 9 bytes.  With it a
 * caller lays out a sync_replica_data body -- object_id, the prefix, the
 * replica, owner, value_id, BE16(replica) -- around a gap of replica size and
 * points vds_ec_repair16_batch_device's outs into the gap: the replica is
 * never copied to build its message.                                         */
int vds_ec_write_number(uint64_t value, uint8_t *out, uint32_t *len);
/* HMAC-SHA256 of `count` device messages of different lengths in ONE launch,
 * one lane per message: message j is lens[j] bytes at msgs[j] (HOST arrays of
 * device pointers and lengths, any alignment, lens[j] == 0 allows NULL) under
 * key session_of[j] of keys (HOST, nsessions keys of 32 bytes; the key pads
 * are hashed on the host, once per session); MAC j goes to macs + 32*j
 * (device; may be NULL when expected is given) and, with expected (device,
 * count*32 bytes, any alignment), is compared into verdicts[j] (device; 0
 * equal, 1 different).  expected and verdicts are NULL together.  The lanes are
 * ordered by length on the host.  Every argument is validated before anything
 * is enqueued and before the device is looked for (null arrays, a null message
 * with a non-zero length, session_of[j] >= nsessions, lens[j] > 2^30,
 * count >= 2^30: VDS_EC_EINVAL); count == 0 is VDS_EC_OK.  Nothing
 * synchronises; the tables ride the pinned parameter ring.                   */
int vds_ec_hmac_sha256_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens,
                                    const uint32_t *session_of, const uint8_t *keys, uint32_t nsessions,
                                    uint8_t *macs, const uint8_t *expected, uint8_t *verdicts, void *stream);
/* Seal `count` messages, one lane per DATAGRAM: message o (msg_lens[o] device
 * bytes at msgs[o], any alignment) of type types[o], first index index0[o],
 * route blob routes[o] (route_lens[o] device bytes; routes may be NULL when
 * every length is 0), session session_of[o], at mtus[o].  Datagram d of message
 * o lands at outs[o] + d*pitch (device; pitch >= the largest mtu; 4-byte
 * aligned slots take the fast stores), its length as vds_ec_dgram_layout says.
 * All arrays HOST arrays; keys as above.  A lane reads its slice of the
 * message once and writes only its datagram's own bytes.  Validation as above,
 * and type >= 32, an mtu or route length vds_ec_dgram_layout rejects, a null
 * output, pitch below an mtu or >= 2^32, index0[o] + its datagram count past
 * 2^32 (the reference's "Overflow pipeline"), 2^31 datagrams or more:
 * VDS_EC_EINVAL, before anything is enqueued.                                */
int vds_ec_dgram_seal_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *msg_lens,
                                   const uint8_t *types, const uint32_t *index0, const uint8_t *const *routes,
                                   const uint32_t *route_lens, const uint32_t *session_of, const uint8_t *keys,
                                   const uint32_t *mtus, uint32_t nsessions, uint8_t *const *outs, uint64_t pitch,
                                   void *stream);
/* Open `count` datagrams, one lane each: datagram j (lens[j] <= 65535 device
 * bytes at dgrams[j]) is verified over lens[j] - 32 bytes against its last 32
 * under session session_of[j]; verdicts[j] (device) = 0 verified, 1 invalid
 * signature, 2 shorter than 33 bytes.  Its payload -- bytes [hdr_lens[j],
 * lens[j] - 32) -- is copied to dsts[j] (device; dsts or dsts[j] may be NULL:
 * verify only) ONLY when the datagram verified: unauthenticated bytes never
 * reach a message buffer, and only the payload's own range is written.
 * hdr_lens[j] > lens[j] - 32 (for lens[j] >= 33): VDS_EC_EINVAL; validation
 * otherwise as above.                                                        */
int vds_ec_dgram_open_batch_device(uint32_t count, const uint8_t *const *dgrams, const uint32_t *lens,
                                   const uint32_t *hdr_lens, const uint32_t *session_of, const uint8_t *keys,
                                   uint32_t nsessions, uint8_t *const *dsts, uint8_t *verdicts, void *stream);
/* The seal from and to host memory on the calling thread's current device:
 * messages, routes and keys in host memory; the datagrams of message o land
 * back to back from slab + offsets[o] (all but its last are mtus[o] bytes, so
 * datagram d starts at offsets[o] + d*mtus[o]), messages back to back;
 * dgram_counts[o] and last_lens[o] as vds_ec_dgram_layout gives them.  The slab
 * must hold the sum of the datagram lengths (VDS_EC_EINVAL otherwise).  Works
 * through groups of at most 64 MiB of message bytes staged in pinned memory:
 * one copy in, one launch, one copy out per group.  Validation as the device
 * form's, every message before any transfer.                                 */
int vds_ec_dgram_seal_host_batch(uint32_t count, const uint8_t *const *msgs, const uint64_t *msg_lens,
                                 const uint8_t *types, const uint32_t *index0, const uint8_t *const *routes,
                                 const uint32_t *route_lens, const uint32_t *session_of, const uint8_t *keys,
                                 const uint32_t *mtus, uint32_t nsessions, uint8_t *slab, uint64_t slab_bytes,
                                 uint64_t *offsets, uint32_t *dgram_counts, uint32_t *last_lens);
/* A message found by vds_ec_dgram_open_host_batch.  status VDS_EC_OK: the route
 * blob (route_len bytes: 0, 32 or 33 + 32 h) is at slab + route_off and the
 * message (msg_len bytes) at slab + msg_off.  Any other status hands out no
 * bytes (offsets and lengths zero): VDS_EC_EDGRAM_DATA where the reference
 * answers "Invalid data" from authenticated headers, VDS_EC_EDGRAM_INCOMPLETE
 * where a datagram is missing or one the message is made of did not verify.  */
typedef struct vds_ec_dgram_message {
  uint32_t session;
  uint32_t index0; /* index of its first datagram */
  uint32_t dgrams; /* datagrams it was planned from */
  uint32_t type;
  int32_t status;
  uint32_t route_len;
  uint64_t route_off;
  uint64_t msg_off;
  uint64_t msg_len;
} vds_ec_dgram_message;
/* Open the datagrams of a drained socket batch, in arrival order, each with its
 * session (host memory).  Headers are parsed on the host to plan where every
 * payload goes: per session the FIRST arrival of an index wins
 * (process_datagram, :172-186); a first datagram starts a message, which takes
 * the continuations at the following indices until the announced size is
 * reached, with the reference's checks as written (:663-:726, the fixed
 * constant of the ProxyData check at :687 included).  Then the datagrams are
 * staged in groups of at most 64 MiB, opened in one launch per group, and the
 * verdicts and assembled messages copied back.  verdicts[j] (host, count
 * bytes): 0 / 1 / 2 as the device form, 3 = service datagram (first byte 6,
 * MTUTest, or 7, Acknowledgment: unsigned, skipped).  messages (host, room for
 * `count`) receives *nmessages records ordered by (session, index0).  A message
 * is VDS_EC_OK only if EVERY datagram it is made of verified, its first
 * included, so every header field that planned it is authenticated after the
 * fact.  The slab needs no more than the sum of the datagram lengths
 * (VDS_EC_EINVAL when the planned messages do not fit).  Validation as the
 * device form's.                                                             */
int vds_ec_dgram_open_host_batch(uint32_t count, const uint8_t *const *dgrams, const uint32_t *lens,
                                 const uint32_t *session_of, const uint8_t *keys, uint32_t nsessions,
                                 uint8_t *verdicts, uint8_t *slab, uint64_t slab_bytes,
                                 vds_ec_dgram_message *messages, uint32_t *nmessages);

/* ------------------------------------------------------- websocket frames
 * What the server holds after a socket read is a websocket FRAME
 * (kernel/vds_http/websocket.cpp:45-201): a 2-, 4- or 10-byte header, a 4-byte
 * mask when the mask bit is set, and the payload XOR-masked byte by byte --
 * for "upload" the JSON text the web client's JSON.stringify produces,
 * {"id":5,"invoke":"upload","params":["<base64>"]} (web/src/store/vds_ws.js).
 * These calls take the frame and the upload / download envelope, and nothing
 * else of vds_http: no continuation frames (the reference implements none: one
 * frame is one message), no close, no pong, no handshake, no other method.
 *
 * vds_ec_ws_frame_parse: the header rules of websocket.cpp:54-109 as host
 * arithmetic (no GPU).  FIN and RSV1-3 are reported and not acted on, as
 * there.  header_len is 2 / 4 / 10 plus 4 with a mask; payload_len the 7-, 16-
 * or 64-bit big-endian length.  Returns VDS_EC_OK for opcodes 1 (text), 2
 * (binary) and 9 (ping: the caller sends its own pong), VDS_EC_EWS_FRAME for
 * every other opcode (the reference's "Not implemented", :123-144; the fields
 * are filled in all the same), VDS_EC_EWS_SHORT when len does not hold the
 * whole header: then only `need` is meaningful, the number of bytes the call
 * has to see to get further (2, then header_len).  (The reference waits for a
 * third byte before it looks at the first two; a frame of two bytes in all --
 * unmasked, empty -- is whole here.)  buf NULL with len > 0, frame NULL:
 * VDS_EC_EINVAL.                                                             */
typedef struct vds_ec_ws_frame {
  uint8_t fin, rsv1, rsv2, rsv3;
  uint8_t opcode;
  uint8_t masked;
  uint8_t mask[4]; /* zero when not masked */
  uint32_t header_len;
  uint32_t need;
  uint64_t payload_len;
} vds_ec_ws_frame;
int vds_ec_ws_frame_parse(const uint8_t *buf, size_t len, vds_ec_ws_frame *frame);
/* websocket_output::start (websocket.cpp:220-257): 0x81 (text) or 0x82
 * (binary), then the length in its 7-bit form below 126, its 16-bit form up to
 * 0xFFFF, else its 64-bit form; never masked.  out receives *len = 2, 4 or 10
 * bytes.                                                                     */
int vds_ec_ws_frame_header(uint64_t payload_len, int binary, uint8_t out[10], uint32_t *len);
/* Recognise the FAST FORM of an "upload" request in a payload of len bytes,
 * masked with mask[j & 3] at byte j (mask NULL: not masked): exactly
 *   {"id":<int>,"invoke":"upload","params":["<body>"]}
 * with <int> 0 or a decimal without leading zeros of at most 2^31 - 1 -- the
 * text JSON.stringify makes of the web client's request.  *id, the body's
 * offset and length in the payload, and *decoded_size =
 * vds_ec_base64_decoded_size of the body (0 when its length is no multiple of
 * 4) are returned.  At most the first 48 and the last 5 bytes of the payload
 * are unmasked and read -- the envelope and the body's last two characters --:
 * the body is never walked.  Anything else -- another key order, whitespace,
 * another method, an id outside the form, a missing end -- is
 * VDS_EC_EWS_FORM: "not the fast form, give it to your own parser".
 * The rule this function and the masked decode keep TOGETHER: a message that
 * comes out VDS_EC_OK of both has exactly the id, body and bytes the
 * reference's json_parser and base64::to_bytes would have produced; any other
 * status decides nothing and the caller may take its slow path.  A '"' or '\'
 * inside the body is not looked for here: it is outside the alphabet, so the
 * decode answers VDS_EC_EB64_CHAR (the reference would have ended the string
 * there, and may even have succeeded: ["QUJD","x"]).  One exception is known
 * and open: the decode, as base64::to_bytes, stops at the first '=', so a '"'
 * BEHIND an early '=' in a body whose last two characters hold a '=' again
 * (QQ=="],"x":["QQ==) is not seen and the message comes out VDS_EC_OK.  No
 * JSON.stringify of a base64 string produces such a body.      */
int vds_ec_ws_upload_request(const uint8_t *payload, uint64_t len, const uint8_t *mask, int32_t *id,
                             uint64_t *body_off, uint64_t *body_len, uint64_t *decoded_size);
/* The answer frames' arithmetic.  Upload: *frame_len = *header_len + the length
 * of vds_ec_upload_response_json(id, n names, replica_size).  Download: the
 * answer {"id":"<id>","result":"<text>"} (websocket_api.cpp:30-49, :772-782)
 * of an object of E bytes: 21 + digits + (E + 2) / 3 * 4 bytes behind the
 * header, the text at frame + *text_off.  The id is printed as
 * vds_ec_upload_response_json prints it (a negative one as its 64-bit
 * two's complement).  Any output may be NULL.                                */
int vds_ec_ws_upload_answer_size(int id, uint32_t n, uint32_t replica_size, uint64_t *frame_len,
                                 uint32_t *header_len);
int vds_ec_ws_download_answer_layout(int id, uint64_t object_size, uint64_t *frame_len, uint32_t *header_len,
                                     uint64_t *text_off);
/* What process_message answers when a method fails (websocket_api.cpp:97-104):
 * the frame header, then {"id":"<id>","error":"<vds_ec_strerror(status)>"} with
 * the message escaped as json_writer.cpp:205-240 escapes.  out == NULL queries
 * the length; cap below it: VDS_EC_EINVAL.  No NUL is written.               */
int vds_ec_ws_error_answer(int id, int status, uint8_t *out, size_t cap, size_t *out_len);
/* vds_ec_base64_decode_batch_device for texts still under their websocket
 * mask: masks (HOST, 4 bytes a text) -- character j of text o is
 * texts[o][j] ^ masks[4*o + (j & 3)], so the caller passes the frame's mask
 * rotated by (body_off & 3).  Everything the kernel looks at is unmasked
 * first: the characters a lane classifies, the two of the declared-size check,
 * the character of the first event and the three the accumulator is rebuilt
 * from.  Same kernel (a template instance), same statuses, same words read,
 * same bytes written; a mask of zero gives the unmasked call's bytes and
 * statuses.  masks NULL with count > 0: VDS_EC_EINVAL.                        */
int vds_ec_base64_decode_masked_batch_device(uint32_t count, const char *const *texts, const uint64_t *text_lens,
                                             const uint8_t *masks, uint8_t *const *outs, const uint64_t *out_sizes,
                                             int32_t *statuses, void *stream);
/* The "upload" answers of a batch as FRAMES, written on the device where the
 * names were made: frame o -- vds_ec_ws_frame_header, then the bytes of
 * vds_ec_upload_response_json(ids[o], n names at replica_digests + 32*o*n, the
 * body hash at data_digests + 32*o, replica_sizes[o]) -- at outs[o] (device,
 * any alignment, vds_ec_ws_upload_answer_size bytes).  ids, replica_sizes,
 * outs: HOST arrays; the digests device memory, any alignment, as
 * vds_ec_save_temp16_batch_device leaves them.  Every name is 44 characters, so
 * the layout is fixed but for the digits of the id and the replica size, which
 * the host puts into the descriptor: one wave a message, a lane encodes one
 * digest and waits for no other.  Only the frames' own bytes are written
 * (dwords where aligned) and only the aligned words holding a digest byte are
 * read.  The descriptors ride the pinned parameter ring.  Null arrays with
 * count > 0, null replica_digests with n > 0, a null outs[o], n > 65536,
 * count >= 2^30: VDS_EC_EINVAL, before the device is looked for; count == 0 is
 * VDS_EC_OK.  Nothing synchronises.                                          */
int vds_ec_ws_upload_answer_batch_device(uint32_t count, const int32_t *ids, uint32_t n,
                                         const uint8_t *replica_digests, const uint8_t *data_digests,
                                         const uint32_t *replica_sizes, uint8_t *const *outs, void *stream);
/* vds_ec_upload16_host_batch fed with FRAMES and answering in frames: frame o
 * is frame_lens[o] host bytes at frames[o] (one frame an entry; bytes behind
 * it are ignored).  Per frame the header is parsed and the request recognised;
 * a frame that is not all there (VDS_EC_EWS_SHORT), of another opcode
 * (VDS_EC_EWS_FRAME), a ping (VDS_EC_EWS_PING) or not the fast form
 * (VDS_EC_EWS_FORM) gets that status, no device work, no answer
 * (answer_lens[o] = 0) and none of its outputs written.  The others' BODIES
 * are gathered at 16-byte aligned offsets of pinned staging (the decode's fast
 * load path), still masked; one copy in; the masked decode,
 * vds_ec_save_temp16_batch_device and the answer launch into a device slab;
 * one copy back of replicas, names, body hashes, statuses and answer frames.
 * The host reads a payload only in memcpy and the at most 53 bytes of
 * vds_ec_ws_upload_request.  statuses[o] (host, required) is then the body's
 * vds_ec_base64_decode status; with a non-zero one none of the message's
 * outputs is written and its answer is vds_ec_ws_error_answer(id, status).
 * Answers land back to back in `answers` (host, answers_bytes): message o owns
 * a slot at answer_offs[o] of max(its upload answer, its error answer for
 * VDS_EC_EB64_CHAR, the longest) bytes, of which answer_lens[o] are written; a
 * slab too small for the slots: VDS_EC_EINVAL.  *failed counts the frames
 * whose status is not VDS_EC_OK.  replica_sizes, data_digests and failed may
 * be NULL.  A replica buffer holds vds_ec_replica_size(2, k, S, 0) bytes for
 * the body's decoded size S; payload_len / 4 * 3 is a bound on S that the
 * frame header gives.  Groups of at most 64 MiB of bodies, one device, validation as
 * vds_ec_upload16_host_batch's, every frame before any transfer.             */
int vds_ec_ws_upload16_host_batch(uint16_t k, uint32_t n, uint32_t count, const uint8_t *const *frames,
                                  const uint64_t *frame_lens, uint8_t *const *outs, uint8_t *replica_digests,
                                  uint8_t *data_digests, uint32_t *replica_sizes, uint8_t *answers,
                                  uint64_t answers_bytes, uint64_t *answer_offs, uint64_t *answer_lens,
                                  int32_t *statuses, uint32_t *failed);
/* vds_ec_download16_host_batch answering in FRAMES: ids (host, count) and a
 * caller slab.  Object o owns a slot at frame_offs[o] of max(its answer frame
 * as vds_ec_ws_download_answer_layout gives it, its error answer for
 * VDS_EC_ERESTORE) bytes, slots back to back; an object whose first trailer
 * has no answer owns the error answer's bytes only.  A passing object's slot
 * receives header + {"id":"N","result":" + the text + "} -- the text copied
 * once, from the staging straight to its place in the frame --, a failing one
 * (VDS_EC_ECORRUPT, VDS_EC_ERESTORE) its vds_ec_ws_error_answer and never a
 * character of text; frame_lens[o] is what was written.  statuses,
 * survivor_verdicts, failed, modes and validation as there; a slab too small
 * for the slots: VDS_EC_EINVAL.                                              */
int vds_ec_ws_download16_host_batch(uint16_t k, uint32_t count, const int32_t *ids, const uint16_t *nodes,
                                    const uint8_t *const *chunks, const uint64_t *chunk_sizes,
                                    const uint8_t *survivor_names, const uint16_t *witness_ids,
                                    const uint8_t *witness_names, uint8_t *slab, uint64_t slab_bytes,
                                    uint64_t *frame_offs, uint64_t *frame_lens, int32_t *statuses,
                                    uint8_t *survivor_verdicts, uint32_t *failed);

/* ------------------------------------------------ file blocks: AES-256-CBC
 * The reference turns a piece of a file into a body and back with AES-256-CBC
 * under PKCS#7 padding (client::save / restore, dht_network_client.cpp:1101-
 * 1320; save_block, web/src/store/vds_ws.js:151-161; OpenSSL's EVP default in
 * private/symmetriccrypto_p.h):
 *     id      = SHA-256(data)
 *     key     = SHA-256(AES-256-CBC(id, pack_block_iv, data))
 *     crypted = AES-256-CBC(key, pack_block_iv, deflate(data))
 * and back: decrypt under key, inflate, SHA-256 == id or "Data is corrupted".
 * The deflate is the library's own where the caller wants it
 * (vds_ec_block_pack_deflate_batch_device below: the whole chain on the
 * device) or the caller's (vds_ec_block_pack_batch_device takes the deflated
 * bytes: a deflate's output differs between implementations, and key does not
 * depend on it); the way back is vds_ec_block_unpack_batch_device below.
 * The same cipher wraps every channel
 * message under its own key and iv (user_channel.cpp:229).
 *
 * vds_ec_aes256_cbc_padded_size: what len bytes encrypt to, (len/16 + 1) * 16.
 * vds_ec_block_iv: pack_block_iv, a5bb9fce c2e44b91 a8c95944 62559024.
 * The *_host pair: ONE message on the calling thread, no GPU (AES-NI where the
 * CPU has it, else portable code; VDS_EC_AES_HOST=portable in the environment
 * at the first call forces the latter).  Encrypt writes padded_size(len) bytes
 * at out (in == out allowed).  Decrypt writes up to len bytes at out, of which
 * the first *out_len are the plaintext, and returns VDS_EC_OK,
 * VDS_EC_ECRYPT_LENGTH (nothing written) or VDS_EC_ECRYPT_PADDING (*out_len 0). */
uint64_t vds_ec_aes256_cbc_padded_size(uint64_t len);
int vds_ec_block_iv(uint8_t iv[16]);
int vds_ec_aes256_cbc_encrypt_host(const uint8_t key[32], const uint8_t iv[16], const uint8_t *in, uint64_t len,
                                   uint8_t *out);
int vds_ec_aes256_cbc_decrypt_host(const uint8_t key[32], const uint8_t iv[16], const uint8_t *in, uint64_t len,
                                   uint8_t *out, uint64_t *out_len);

/* `count` messages of different lengths in one launch each way.  ins, lens,
 * outs: HOST arrays of device pointers and lengths, any alignment (fast path:
 * 16-byte aligned).  keys: DEVICE, count * 32 bytes, 4-byte aligned (message
 * o's key at keys + 32 o: keys are digests of a hash launch).  ivs: DEVICE,
 * count * 16 bytes, or NULL: every message under pack_block_iv.  out_lens,
 * statuses: DEVICE, 4-byte aligned.  Nothing synchronises.  Everything is
 * validated before anything is enqueued and before the device is looked for:
 * VDS_EC_EINVAL for null arrays, a null pointer with a non-zero length,
 * lens[o] >= 2^32, count >= 2^30, a message whose input and output overlap;
 * count == 0 is VDS_EC_OK.
 * Encrypt writes exactly padded_size(lens[o]) bytes at outs[o].
 * Decrypt writes at most lens[o] bytes at outs[o], of which the first
 * out_lens[o] are the plaintext; every statuses[o] (VDS_EC_OK,
 * VDS_EC_ECRYPT_LENGTH, VDS_EC_ECRYPT_PADDING) and out_lens[o] is written by
 * the launch, a bad status with out_len 0 and unspecified contents; a length
 * that is 0 or no multiple of 16 gets its status and no other work.        */
int vds_ec_aes256_cbc_encrypt_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                           const uint8_t *keys, const uint8_t *ivs, uint8_t *const *outs,
                                           void *stream);
int vds_ec_aes256_cbc_decrypt_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                           const uint8_t *keys, const uint8_t *ivs, uint8_t *const *outs,
                                           uint32_t *out_lens, int32_t *statuses, void *stream);

/* client::save for `count` blocks on device pointers: four launches on the
 * stream, no host step between them -- SHA-256 of datas into ids, encrypt
 * datas under ids into library scratch, SHA-256 of that into keys, encrypt
 * zipped under keys into crypted[o] (padded_size(zipped_lens[o]) bytes, which
 * may be handed to vds_ec_save_temp16_batch_device as body o).  ids, keys:
 * DEVICE, count * 32 bytes each, 4-byte aligned.  zipped[o] is the caller's
 * deflate of datas[o]; the call does not look inside it.  Validation as above
 * (a crypted[o] overlapping datas[o] or zipped[o] included).               */
int vds_ec_block_pack_batch_device(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens,
                                   const uint8_t *const *zipped, const uint64_t *zipped_lens, uint8_t *ids,
                                   uint8_t *keys, uint8_t *const *crypted, void *stream);
/* The same on HOST pointers (ids, keys host too): gathered into pinned staging
 * at 16-byte aligned offsets, one copy in, the device form, one copy back,
 * scattered; groups of at most 64 MiB; the calling thread's current device;
 * every block validated before any transfer.  crypted_sizes (may be NULL)
 * receives padded_size(zipped_lens[o]).                                    */
int vds_ec_block_pack_host_batch(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens,
                                 const uint8_t *const *zipped, const uint64_t *zipped_lens, uint8_t *ids,
                                 uint8_t *keys, uint8_t *const *crypted, uint64_t *crypted_sizes);
/* vds_ec_aes256_cbc_decrypt_batch_device on HOST pointers, staged the same
 * way (keys, ivs host; ivs NULL: pack_block_iv).  outs[o] must hold lens[o]
 * bytes; a message whose status is not VDS_EC_OK has out_lens[o] 0 and its
 * output untouched; *failed (may be NULL) counts them.                      */
int vds_ec_aes256_cbc_decrypt_host_batch(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                         const uint8_t *keys, const uint8_t *ivs, uint8_t *const *outs,
                                         uint64_t *out_lens, int32_t *statuses, uint32_t *failed);

/* ------------------------------------------------------ file blocks: inflate
 * The reference's inflate (kernel/vds_data/inflate.h, private/inflate_p.h) is
 * zlib's: a zlib header, deflate blocks, an Adler-32 trailer (pako.deflate in
 * the web client writes the same).  Statuses, of one message:
 *   VDS_EC_OK              the stream ended and its Adler-32 matches; bytes
 *                          behind the stream's end are ignored; out_len = the
 *                          plaintext's length.
 *   VDS_EC_EINFLATE_DATA   zlib's Z_DATA_ERROR or Z_NEED_DICT: a bad header
 *                          (method, window, check, preset dictionary), block
 *                          type 3, a stored length that is not its complement's,
 *                          too many length or distance symbols, an invalid set
 *                          of code lengths, a repeat with no length before it,
 *                          no end-of-block code, an invalid literal/length or
 *                          distance code, a distance reaching before the
 *                          output's start, a wrong Adler-32.  out_len 0,
 *                          contents unspecified.
 *   VDS_EC_EINFLATE_SHORT  the input ends before the stream does.  out_len =
 *                          what zlib delivers for that input, and those bytes
 *                          are valid: every literal whose code lies wholly
 *                          inside the input, every match whose length code,
 *                          distance code and extra bits lie wholly inside it,
 *                          the bytes of a stored block that are there.  An
 *                          error shows only once the bits that reveal it are
 *                          inside the input.  An input of length 0 is SHORT.
 *   VDS_EC_EINFLATE_SPACE  the next literal, match or stored run would pass
 *                          out_cap.  out_len 0, contents unspecified.  As in
 *                          zlib, a full output comes before the match's own
 *                          error: a distance reaching before the output's
 *                          start is SPACE where out_cap bytes are out already.
 * No byte is written at or past out + out_cap, whatever the stream says.
 *
 * vds_ec_inflate_host: ONE message on the calling thread, no GPU, no zlib.
 * VDS_EC_EINVAL for a null out_len, a null pointer with a non-zero size, a
 * size >= 2^32, input and output overlapping.                               */
int vds_ec_inflate_host(const uint8_t *in, uint64_t len, uint8_t *out, uint64_t out_cap, uint64_t *out_len);
/* `count` streams in one launch, one wave a stream.  ins, lens, outs,
 * out_caps: HOST arrays of device pointers and sizes, any alignment.
 * out_lens, statuses: DEVICE, 4-byte aligned, every one of them written by
 * the launch.  Nothing synchronises.  Everything is validated before anything
 * is enqueued and before the device is looked for: VDS_EC_EINVAL for null
 * arrays, a null pointer with a non-zero size, lens[o] or out_caps[o] >= 2^32,
 * count >= 2^30, a message whose input and output overlap; count == 0 is
 * VDS_EC_OK.                                                                */
int vds_ec_inflate_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                uint8_t *const *outs, const uint64_t *out_caps, uint32_t *out_lens,
                                int32_t *statuses, void *stream);
/* The same on HOST pointers (out_lens, statuses host too), staged through
 * pinned buffers in groups of at most 64 MiB each way.  A message whose status
 * is not VDS_EC_OK (VDS_EC_EINFLATE_SHORT included) has out_lens[o] 0 and its
 * output untouched; *failed (may be NULL) counts them.                      */
int vds_ec_inflate_host_batch(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                              uint8_t *const *outs, const uint64_t *out_caps, uint64_t *out_lens,
                              int32_t *statuses, uint32_t *failed);
/* client::restore (dht_network_client.cpp:1297-1316) for `count` blocks on
 * device pointers: three launches on the stream, no host step and no
 * synchronisation between them -- decrypt crypted[o] under keys + 32 o and
 * pack_block_iv into library scratch, inflate from there into outs[o], SHA-256
 * of the inflated bytes compared with ids + 32 o.  keys: DEVICE, 4-byte
 * aligned; ids: DEVICE, any alignment; the rest as the inflate's.
 * statuses[o] is the first step that failed: VDS_EC_ECRYPT_LENGTH /
 * VDS_EC_ECRYPT_PADDING, VDS_EC_EINFLATE_DATA / VDS_EC_EINFLATE_SPACE,
 * VDS_EC_ECORRUPT where the digest differs from the id, else VDS_EC_OK.  A
 * stream that ends short goes on to the hash, as in the reference, and is OK
 * only if its bytes hash to the id.  out_lens[o] is 0 for every status but OK. */
int vds_ec_block_unpack_batch_device(uint32_t count, const uint8_t *const *crypted, const uint64_t *crypted_lens,
                                     const uint8_t *keys, const uint8_t *ids, uint8_t *const *outs,
                                     const uint64_t *out_caps, uint32_t *out_lens, int32_t *statuses, void *stream);
/* The same on HOST pointers (keys, ids, out_lens, statuses host too), staged
 * as above.  A block whose status is not VDS_EC_OK has its output untouched;
 * *failed (may be NULL) counts them.                                        */
int vds_ec_block_unpack_host_batch(uint32_t count, const uint8_t *const *crypted, const uint64_t *crypted_lens,
                                   const uint8_t *keys, const uint8_t *ids, uint8_t *const *outs,
                                   const uint64_t *out_caps, uint64_t *out_lens, int32_t *statuses, uint32_t *failed);

/* ------------------------------------------------------ file blocks: deflate
 * The reference's deflate (kernel/vds_data/deflate.cpp) is zlib at its default
 * level; what its inflate needs is a zlib stream that gives the data back.
 * The library's own compressor writes one: header 78 01 (CM 8, window 32 KiB,
 * no preset dictionary), dynamic-Huffman and stored blocks, the Adler-32.  Its
 * bytes differ from zlib's, and they are THE SAME on the device and on the
 * host for the same input: a body is named by its SHA-256, so two paths must
 * not pack one block differently.  There are no per-message failures.
 *
 * vds_ec_deflate_bound: the size of the all-stored form,
 * 2 + len + 5 * max(1, ceil(len / 65535)) + 4; no output is longer.
 * vds_ec_deflate_host: ONE message on the calling thread, no GPU, no zlib.
 * VDS_EC_EINVAL for a null out or out_len, a null in with a non-zero len, a
 * bound >= 2^32, out_cap below the bound, input and output overlapping.     */
uint64_t vds_ec_deflate_bound(uint64_t len);
int vds_ec_deflate_host(const uint8_t *in, uint64_t len, uint8_t *out, uint64_t out_cap, uint64_t *out_len);
/* `count` messages in one launch, one wave a message.  ins, lens, outs,
 * out_caps: HOST arrays of device pointers and sizes, any alignment.
 * out_lens: DEVICE, 4-byte aligned, every entry written by the launch.
 * Nothing synchronises.  Everything is validated before anything is enqueued
 * and before the device is looked for: VDS_EC_EINVAL for null arrays, a null
 * pointer, a bound >= 2^32, out_caps[o] below the bound of lens[o],
 * count >= 2^30, a message whose input and output overlap; count == 0 is
 * VDS_EC_OK.  Nothing is written outside outs[o] .. outs[o] + out_caps[o].  */
int vds_ec_deflate_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                                uint8_t *const *outs, const uint64_t *out_caps, uint32_t *out_lens, void *stream);
/* The same on HOST pointers (out_lens host too), staged through pinned
 * buffers in groups of at most 64 MiB each way.                             */
int vds_ec_deflate_host_batch(uint32_t count, const uint8_t *const *ins, const uint64_t *lens,
                              uint8_t *const *outs, const uint64_t *out_caps, uint64_t *out_lens);
/* vds_ec_aes256_cbc_encrypt_batch_device with the lengths on the device:
 * message o is the first lens[o] (DEVICE, uint32, 4-byte aligned) bytes at
 * ins[o], and lens[o] <= max_lens[o] (HOST), which orders the chains and
 * bounds what may be read and written: padded_size(lens[o]) bytes at outs[o],
 * never more than padded_size(max_lens[o]).  out_lens[o] (DEVICE, uint32,
 * 4-byte aligned) receives padded_size(lens[o]).  A lens[o] above max_lens[o]
 * is cut to it.  Validation as the encrypt's, with max_lens for lens.       */
int vds_ec_aes256_cbc_encrypt_gated_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *max_lens,
                                                 const uint32_t *lens, const uint8_t *keys, const uint8_t *ivs,
                                                 uint8_t *const *outs, uint32_t *out_lens, void *stream);
/* client::save for `count` blocks on device pointers with the deflate on the
 * device too: five launches on the stream, no host step and no
 * synchronisation between them -- SHA-256 of datas into ids, encrypt datas
 * under ids into library scratch, SHA-256 of that into keys, deflate datas
 * into library scratch, encrypt that under keys into crypted[o].
 * crypted_caps[o] >= padded_size(deflate_bound(data_lens[o])), else
 * VDS_EC_EINVAL; crypted_lens (DEVICE, uint32, 4-byte aligned) receives the
 * bodies' sizes.  vds_ec_save_temp16_batch_device takes its body sizes on the
 * host: the caller reads crypted_lens (count * 4 bytes) back before it.     */
int vds_ec_block_pack_deflate_batch_device(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens,
                                           uint8_t *ids, uint8_t *keys, uint8_t *const *crypted,
                                           const uint64_t *crypted_caps, uint32_t *crypted_lens, void *stream);
/* The same on HOST pointers (ids, keys, crypted_sizes host), staged as above. */
int vds_ec_block_pack_deflate_host_batch(uint32_t count, const uint8_t *const *datas, const uint64_t *data_lens,
                                         uint8_t *ids, uint8_t *keys, uint8_t *const *crypted,
                                         const uint64_t *crypted_caps, uint64_t *crypted_sizes);

/* ------------------------------------------------- RSA signature verification
 * The public-key check of the transaction log: asymmetric_sign_verify::verify
 * (hash::sha256(), key, sig, data) -- EVP_DigestVerify* with an RSA key
 * (kernel/vds_crypto/asymmetriccrypto.cpp:488-537), RSASSA-PKCS1-v1_5 over
 * SHA-256 -- behind transaction_block::validate (sync_process.cpp:283), the
 * signed messages inside a block (transaction_log.cpp:803, :1203) and
 * allocate_storage (websocket_api.cpp:667).  Public data only: nothing here is
 * constant-time.
 *
 * vds_ec_rsa_key: a public key ready for Montgomery arithmetic, a fixed-size
 * POD that is copied to the device as it stands.  limbs is 64 (moduli up to
 * 2048 bits) or 128; R = 2^(32 limbs).                                       */
#define VDS_EC_RSA_MAX_LIMBS 128
typedef struct vds_ec_rsa_key {
  uint32_t n[VDS_EC_RSA_MAX_LIMBS];  /* the modulus, little-endian 32-bit limbs, zero above its length */
  uint32_t rr[VDS_EC_RSA_MAX_LIMBS]; /* R^2 mod n, likewise                                            */
  uint32_t limbs;                    /* 64 or 128                                                      */
  uint32_t n_bytes;                  /* the modulus length in bytes (RSA_size): no leading zero byte   */
  uint32_t e;                        /* the public exponent, odd, >= 3                                 */
  uint32_t n0inv;                    /* -n^-1 mod 2^32                                                 */
} vds_ec_rsa_key;
/* From the big-endian magnitudes as the caller holds them (leading zero bytes
 * allowed; DER parsing stays with the caller).  VDS_EC_EINVAL for a null
 * argument, an even modulus, a modulus under 512 or over 4096 bits, an even
 * e, e < 3 or e >= 2^32.                                                      */
int vds_ec_rsa_key_prepare(const uint8_t *n_be, uint64_t n_len, const uint8_t *e_be, uint64_t e_len,
                           vds_ec_rsa_key *key);
/* asymmetric_public_key::fingerprint() (asymmetriccrypto.cpp:657-681): the
 * SHA-256 of BE32(7) "ssh-rsa" BE32(len e) e BE32(len n) n, each magnitude
 * without leading zero bytes and with one 00 in front when its top nibble is 9
 * or above (the reference's own rule: a top nibble of 8 gets none).  The
 * writer's key id of a transaction block.  VDS_EC_EINVAL for a null argument
 * or a zero magnitude.                                                        */
int vds_ec_rsa_fingerprint(const uint8_t *n_be, uint64_t n_len, const uint8_t *e_be, uint64_t e_len, uint8_t *out);
/* in^e mod n on the calling thread (no GPU, no OpenSSL): in and out are
 * key->n_bytes big-endian bytes.  VDS_EC_EINVAL for a null argument, in_len
 * other than key->n_bytes, a value >= n.                                      */
int vds_ec_rsa_public_host(const vds_ec_rsa_key *key, const uint8_t *in, uint64_t in_len, uint8_t *out);
/* The verdict of EVP_DigestVerify(SHA-256) on the calling thread: *verdict 1
 * or 0.  0 for a signature whose length is not key->n_bytes or whose value is
 * >= n; otherwise sig^e mod n is compared, whole, with
 * 00 01 FF..FF 00 || DigestInfo(SHA-256) || SHA-256(msg): nothing is parsed
 * out of the decrypted block.  VDS_EC_EINVAL for a null key or verdict, a
 * null msg or sig with a non-zero length.                                     */
int vds_ec_rsa_verify_sha256_host(const vds_ec_rsa_key *key, const uint8_t *msg, uint64_t len, const uint8_t *sig,
                                  uint64_t sig_len, uint8_t *verdict);
/* The raw operation for `count` items in one launch, one wave an item.  ins,
 * in_lens, key_idx, outs: HOST arrays (device pointers, lengths, indices into
 * keys); keys: HOST, nkeys prepared keys, copied through the pinned parameter
 * ring with the tables; items under 64- and 128-limb keys may be mixed.
 * outs[o] receives the n_bytes of item o's key; statuses (DEVICE, one byte an
 * item) 0, or (uint8_t)VDS_EC_EINVAL for an in_lens[o] that is not n_bytes or
 * a value >= n, and then outs[o] is left untouched.  Nothing synchronises.
 * Validated before anything is enqueued and before the device is looked for:
 * VDS_EC_EINVAL for null arrays or a null pointer with count > 0, key_idx[o]
 * >= nkeys, a key that vds_ec_rsa_key_prepare would not have produced, count
 * >= 2^30; count == 0 is VDS_EC_OK.  Only outs' and statuses' own bytes are
 * written.                                                                    */
int vds_ec_rsa_public_batch_device(uint32_t count, const uint8_t *const *ins, const uint64_t *in_lens,
                                   const uint32_t *key_idx, const vds_ec_rsa_key *keys, uint32_t nkeys,
                                   uint8_t *const *outs, uint8_t *statuses, void *stream);
/* vds_ec_rsa_verify_sha256_host's verdict for `count` signatures in ONE launch
 * from digests already on the device: digests + 32 o (DEVICE) is SHA-256 of
 * message o, sigs / sig_lens / key_idx HOST arrays as above, verdicts (DEVICE,
 * one byte an item) 1 or 0.  The decrypted block is compared in the kernel and
 * never stored.  Validation as above.                                         */
int vds_ec_rsa_verify_digest_batch_device(uint32_t count, const uint8_t *digests, const uint8_t *const *sigs,
                                          const uint64_t *sig_lens, const uint32_t *key_idx,
                                          const vds_ec_rsa_key *keys, uint32_t nkeys, uint8_t *verdicts, void *stream);
/* vds_ec_sha256_batch_device over msgs / lens, then the launch above: two
 * launches.  digests (DEVICE, 32 count bytes) receives the digests; null: the
 * library's own scratch holds them.  Validation as both.                      */
int vds_ec_rsa_verify_sha256_batch_device(uint32_t count, const uint8_t *const *msgs, const uint64_t *lens,
                                          const uint8_t *const *sigs, const uint64_t *sig_lens,
                                          const uint32_t *key_idx, const vds_ec_rsa_key *keys, uint32_t nkeys,
                                          uint8_t *verdicts, uint8_t *digests, void *stream);
/* A transaction-log block as transaction_block::create reads it
 * (transaction_block.cpp:11-50; binary_serialize.cpp:13-66, 245-): BE32
 * version, BE64 time, BE64 order number, the writer's key id, the set of
 * ancestors (a count, then the buffers), the messages, the signature -- every
 * buffer behind its write_number length.  Offsets are from the block's first
 * byte; a buffer's offset is that of its first byte behind the length.        */
typedef struct vds_ec_txblock {
  uint64_t time_point, order_no;
  uint64_t key_id_off, key_id_len;
  uint64_t ancestors_off, ancestors_len; /* the whole set, its count included    */
  uint64_t ancestors_count;
  uint64_t messages_off, messages_len;
  uint64_t signature_off, signature_len;
  uint64_t signed_len; /* the prefix in front of the signature's length: what validate() signs */
} vds_ec_txblock;
/* validate() (transaction_block.cpp:102-117) verifies a RE-SERIALISATION of
 * the parsed fields, so only a block whose re-serialisation is its own prefix
 * is accepted: version 0x31564453, every number in its shortest form, the
 * ancestors strictly ascending in const_data_buffer::operator< (size first,
 * then bytes), nothing behind the signature, a time that to_time_t /
 * from_time_t give back (below 2^63 / 10^9).  Anything else, truncation
 * included, is VDS_EC_ETX_FORM; VDS_EC_EINVAL for a null argument.            */
int vds_ec_txblock_parse(const uint8_t *data, uint64_t len, vds_ec_txblock *out);
/* apply_message's check for a drained batch of records, HOST memory in and
 * out: ids + 32 o = SHA-256 of block o (the record's id); statuses[o]
 * VDS_EC_OK, VDS_EC_ETX_FORM, or VDS_EC_ETX_KEY where the writer's key id is
 * none of fingerprints + 32 j (j < nkeys; the caller then walks
 * node_add_transaction); verdicts[o] the signature's verdict under keys[j]
 * where the status is VDS_EC_OK, else 0.  The blocks are staged once: one
 * SHA-256 launch gives ids and prefix digests, one launch verifies.           */
int vds_ec_txblock_validate_host_batch(uint32_t count, const uint8_t *const *blocks, const uint64_t *lens,
                                       const vds_ec_rsa_key *keys, const uint8_t *fingerprints, uint32_t nkeys,
                                       uint8_t *ids, uint8_t *verdicts, int32_t *statuses);

/* ----------------------------------------------------------------- utilities */
/* Fill `size` device bytes at dst with the splitmix64 stream of `seed`
 * (little-endian 8-byte words) -- the synthetic-object generator used by
 * bench.py and the parity tests (SURVEY.md 8(c) "Input PRNG").               */
int vds_ec_fill_splitmix_device(uint8_t *dst, uint64_t size, uint64_t seed, void *stream);

/* Which kernel path a device call with these parameters takes: 4 = the
 * survivor set's own run-time compiled kernel (vds_ec_jit_*) for the full
 * tiles, 3 = syndrome
 * restore (erasure-pattern-independent XOR programs, survivors within
 * 0..k+k/4-1) for the full tiles, 2 = bit-sliced fast path for the full tiles
 * (+ generic tail; objects under one tile whose stripes are whole 512-stripe
 * groups ride it in batches), 1 = generic path only.  The restore query takes
 * the trailer's padding and the batch's object count, as
 * vds_ec_restore16_device does (restore planning is shared with it).
 * (A -DVDS_RESTORE_PATH_BS=1 build of the library disables path 3: A/B.)  */
int vds_ec_encode16_path(uint16_t k, const uint16_t *replicas, uint32_t n, uint64_t size);
int vds_ec_restore16_path(uint16_t k, const uint16_t *nodes, uint64_t chunk_size, uint16_t padding, uint32_t count);
/* 4 = the regenerate runs the survivor set's run-time compiled kernel
 * (vds_ec_jit_*), 3 = the regenerate rides the syndrome kernel (every target
 * an erased point of a compiled (k, n)) for the full tiles, 2 = the runtime-coefficient
 * bit-sliced kernel (k in {16, 32}, at most k targets, >= 512 full stripes),
 * 1 = generic path only.                                                    */
int vds_ec_regenerate16_path(uint16_t k, const uint16_t *nodes, const uint16_t *targets, uint32_t ntargets,
                             uint64_t chunk_size);

/* ------------------------------------------- run-time compiled restore kernels
 * A restore whose survivors are k distinct points of 0..k+k/4-1 (k in {16,
 * 32}) runs k_restore_syn: fixed syndrome programs plus a runtime recovery of
 * the erased points.  For each such survivor set a device restore meets, the
 * library also generates the set's own XOR programs (the erased points below
 * k as fixed combinations of the survivors) and, from the set's second use,
 * compiles that kernel in the background (hiprtc, gfx950); later restores of
 * the set use it.  Same bytes.  Mode (vds_ec_jit_set_mode, initially from
 * VDS_EC_JIT): 0 = off (VDS_EC_JIT=0), 1 = background (default), 2 = compile
 * on the calling thread at the first use (VDS_EC_JIT=sync).
 * No counterpart in the reference (its restore is a CPU loop, chunk.h:402-444).
 *
 * vds_ec_jit_wait:    block until no compile is queued or running.
 * vds_ec_jit_build16: compile the kernel of survivor set `nodes` and return
 *                     its code object size (no device needed; EINVAL for a set
 *                     the syndrome kernel does not serve, EHIP if hiprtc fails).
 * vds_ec_jit_ready16: 1 when that set's kernel is compiled, else 0.
 * vds_ec_jit_dump16:  compile the kernel of survivor set `nodes` (regen != 0:
 *                     its fused-regenerate kernel) and write its source and
 *                     code object as dir/jit_<k>_<n>_<mask>[_regen].{hip,co}
 *                     (inspection: register use, spills; no device needed).  */
int vds_ec_jit_set_mode(int mode);
int vds_ec_jit_wait(void);
int vds_ec_jit_build16(uint16_t k, const uint16_t *nodes, uint64_t *code_bytes);
int vds_ec_jit_ready16(uint16_t k, const uint16_t *nodes);
int vds_ec_jit_dump16(uint16_t k, const uint16_t *nodes, int regen, const char *dir);

#ifdef __cplusplus
}
#endif

#endif /* VDS_EC_H_ */
