// ec_internal.hpp -- launch interface between the C ABI (vds_ec_api.cpp) and
// the kernels (ec_generic.hip, ec_encode.hip, ec_restore_bs.hip, ec_restore_syn.hip).  Internal to libvds_ec.so.
#pragma once

#ifndef __HIPCC_RTC__  // (hiprtc sees the launch structs only: vds_ec_jit.cpp)
#include <hip/hip_runtime_api.h>
#endif

#include <cstdint>

namespace vds_ec {

constexpr int kMaxLaunchReplicas = 64;  // replicas per generic encode launch
constexpr int kMaxFastK = 32;
constexpr uint32_t kTileStripes = 2048;  // 64 lanes x 32 bit-sliced slots

struct GenericEncodeArgs {
  const uint8_t *in;
  uint64_t size;       // object bytes (cell arrays: bytes too)
  uint64_t in_stride;  // bytes between objects
  uint32_t count;      // objects
  uint32_t k;
  uint32_t cell_bytes; // 1 or 2
  uint32_t flags;
  uint32_t nrep;
  uint64_t t_begin;    // first stripe handled
  uint64_t t_count;    // stripes handled (the trailer is one extra index)
  uint64_t stripes;    // total stripes T of an object
  uint32_t write_trailer;
  uint64_t out_stride;
  uint16_t nodes[kMaxLaunchReplicas];
  uint8_t *outs[kMaxLaunchReplicas];
};

constexpr int kInlineChunks = 64;   // chunk pointers carried in the kernel arguments
constexpr int kInlineMatrixK = 32;  // k*k inverse carried in the kernel arguments

// Where chunk j lives (first match): chunk_pitch != 0 -> chunk_base + j*pitch
// (contiguous staging of the host path); chunk_table != nullptr -> device
// table; otherwise chunk_ptr[j] (k <= kInlineChunks).  The inverse is inline
// (two coefficients per dword) unless matrix_dev is set.  No stream-ordered
// allocations are involved, so a launch never depends on a freed table.
struct GenericRestoreArgs {
  const uint8_t *chunk_ptr[kInlineChunks];
  const uint8_t *chunk_base;
  uint64_t chunk_pitch;
  const uint8_t *const *chunk_table;
  const uint16_t *matrix_dev;
  uint32_t matrix_inline[kInlineMatrixK * kInlineMatrixK / 2];
  uint64_t chunk_stride;
  uint32_t count;
  uint32_t k;
  uint32_t cell_bytes;
  uint32_t flags;
  uint64_t t_begin;
  uint64_t t_count;
  uint8_t *out;
  uint64_t out_stride;
  uint64_t out_len;  // bytes of the restored object (trim bound)
};

// Bit-sliced encode: the full stripes of `count` objects, F = 128
// groups_per_obj per object, as one stream of 2048-stripe tiles (k >= 8:
// tiles may straddle objects; k = 4: groups_per_obj % 16 == 0).
struct FastEncodeArgs {
  const uint8_t *in;
  uint64_t in_stride;
  uint64_t out_stride;
  uint32_t groups_per_obj;
  uint32_t total_tiles;
  // 1: also write every replica's trailer -- zero, as the launch covers every
  // stripe of objects whose size is a multiple of 2k -- at cell T (k >= 8)
  uint32_t trailer0;
  uint8_t *outs[kMaxLaunchReplicas];  // outs[r] for replica id r = 0..N-1
};

// Batched bit-sliced encode of objects of different sizes (k_encode_batch,
// ec_encode_batch.hpp): one launch over every 128-stripe group of every
// object.  Device tables, built on the host: objs[e] per object, tiles[t] per
// 2048-stripe tile.  Group j of tile t is group q[j] (stripes 128 q[j] ..) of
// object obj[j]; an object's groups are consecutive, its last one may hold
// fewer than 128 stripes and end in a partial stripe.  The unused groups of
// the batch's last tile name the batch's empty object (size 0: nothing is
// loaded or stored for it).
constexpr uint64_t kEncBatchPtrTable = ~0ull;  // EncBatchObj::pitch: `out` is a table of pointers
struct EncBatchObj {
  const uint8_t *in;  // 4-byte aligned
  uint64_t size;      // bytes; T = ceil(size / 2k) cells per replica, then the trailer
  // replica r at out + r * pitch (replica pointers equally spaced, the usual
  // case: 32 bytes an object whatever n), or, with pitch ==
  // kEncBatchPtrTable, at ((uint8_t *const *)out)[r] (a device table of n
  // pointers; any 2-byte aligned addresses)
  uint64_t out;
  uint64_t pitch;
};
struct EncBatchTile {
  uint32_t obj[16];
  uint32_t q[16];
};
struct EncBatchLaunch {
  const EncBatchObj *objs;
  const EncBatchTile *tiles;
  uint32_t total_tiles;
  uint32_t trailer;  // 1: each object's BE16 trailer (size mod 2k) is written after its cell T-1
};

// SHA-256 over messages of different lengths (k_sha256_batch, sha256.hip): one
// lane per message, one launch.  Device tables, built on the host.  A group is
// m messages of one length whose digests are contiguous -- the n replicas of
// one object, or one message (m = 1).  Groups are laid out in lane order:
// group g owns lanes spans[g].first .. + m - 1 (first ascending; lanes between
// two groups belong to nobody and do nothing).  wave_group[w] is the last group
// whose first lane is <= 64 w (waves + 1 entries, the last one for lane
// 64 waves), so a lane finds its group between two consecutive entries.
constexpr uint64_t kShaBatchPtrTable = ~0ull;  // ShaBatchGroup::pitch: `msg` is a table of pointers
struct ShaBatchGroup {
  // message i at msg + i * pitch (32 bytes a group whatever m), or, with
  // pitch == kShaBatchPtrTable, at ((const uint8_t *const *)msg)[i] (a device
  // table of m pointers); any alignment; len == 0: never dereferenced
  uint64_t msg;
  uint64_t pitch;
  uint64_t len;      // bytes of each message
  uint64_t digests;  // digest of message i at digests + 32 i
};
struct ShaBatchSpan {
  uint32_t first;  // the group's first lane
  uint32_t m;      // its messages
};
struct ShaBatchLaunch {
  const ShaBatchGroup *groups;
  const ShaBatchSpan *spans;
  const uint32_t *wave_group;
  uint32_t waves;
};
// Check mode (k_sha256_batch<true>): checks[g] beside groups[g], same order.
// A lane compares its digest with the 32 bytes at expected + 32 i and writes
// the verdict byte at verdicts + i: 0 equal, 1 different (any alignment, both).
// expected == 0: the group is not checked and no verdict byte of it is
// written.  In this mode a group whose ShaBatchGroup::digests is 0 writes no
// digest (check only).
struct ShaBatchCheck {
  uint64_t expected;
  uint64_t verdicts;
};
struct ShaBatchCheckLaunch {
  ShaBatchLaunch b;
  const ShaBatchCheck *checks;
};

// base64 wire text (base64.hip).  Decode: one wave per message, the messages
// longest first; msgs[w] is wave w's.  A step of a wave is kB64DecStep
// characters (16 a lane).
constexpr uint32_t kB64DecStep = 1024;
struct B64DecMsg {
  uint64_t text;    // len characters, any alignment
  uint64_t out;     // size bytes, any alignment
  uint64_t status;  // its int32_t status (VDS_EC_OK, VDS_EC_EB64_*, VDS_EC_EINVAL), 4-byte aligned
  uint32_t len;
  uint32_t size;    // declared: len / 4 * 3 - p, p = 0, 1, 2 (0 when len % 4)
};
// Encode: one wave per tile of kB64EncTile input bytes (8 steps of 12 bytes a
// lane), tiles[w] = wave w's message and its tile of it.
constexpr uint32_t kB64EncTile = 6144;
struct B64EncMsg {
  uint64_t in;   // len bytes, any alignment
  uint64_t out;  // (len + 2) / 3 * 4 characters, any alignment
  uint64_t len;
};
struct B64EncTile {
  uint32_t msg;
  uint32_t tile;
};
// Gated encode (k_b64_encode_batch<true>): gates[m] beside msgs[m], and every
// message has a tile 0 (a message of length 0 too).  A message whose ngate
// gate bytes are not all zero has no character written; its tile 0 writes the
// status either way.
struct B64EncGate {
  uint64_t gate;    // ngate bytes, any alignment (verdicts of an earlier launch on the stream); ngate == 0: never read
  uint64_t status;  // its int32_t status (VDS_EC_OK, VDS_EC_ECORRUPT), 4-byte aligned
  uint32_t ngate;
  uint32_t reserved;
};
// AES-256-CBC over messages of different lengths (aes.hip).  Encrypt: one QUAD
// per message (a chain), 16 chains a wave, the chains longest first; msgs[q]
// is quad q's.  Message idx's key is 32 bytes at keys + 32 idx, its iv 16 at
// ivs + 16 idx (ivs 0: pack_block_iv).
constexpr uint32_t kAesEncChainsPerWave = 16;
struct AesEncMsg {
  uint64_t in;   // len bytes, any alignment; never dereferenced when len == 0
  uint64_t out;  // (len / 16 + 1) * 16 bytes, any alignment
  uint32_t len;
  uint32_t idx;  // the message's place in the caller's order
};
// Decrypt: one workgroup of kAesDecThreads lanes per tile of kAesDecTile
// ciphertext bytes, one lane a 16-byte block a step; tiles[w] = workgroup w's
// message and its tile of it.  Every message has a tile 0 (one whose length is
// 0 or no multiple of 16 too: it writes the status and does nothing else).
constexpr uint32_t kAesDecTile = 16384;
constexpr uint32_t kAesDecThreads = 256;
struct AesDecMsg {
  uint64_t in;   // len bytes, any alignment
  uint64_t out;  // len bytes, any alignment, not overlapping in
  uint32_t len;
  uint32_t reserved;
};
struct AesDecTile {
  uint32_t msg;
  uint32_t tile;
};
struct AesDecLaunch {
  const AesDecMsg *msgs;
  const AesDecTile *tiles;
  uint32_t ntiles;
  uint64_t keys, ivs;          // as above, by message index
  uint64_t out_lens, statuses;  // uint32_t / int32_t a message
};
// Gated mode (k_sha256_batch<true, true>: the unpack chain's name check, whose
// lengths and statuses exist only on the device): gates[g] beside groups[g] and
// checks[g], every group one message.  The lane reads the message's status; if
// it is neither VDS_EC_OK nor VDS_EC_EINFLATE_SHORT it zeroes the length and
// does nothing else.  Else it hashes min(*len, ShaBatchGroup::len) bytes (the
// host planned with the upper bound), compares with the expected bytes, and
// writes VDS_EC_OK, or VDS_EC_ECORRUPT and a length of 0.  No verdict byte.
struct ShaBatchGate {
  uint64_t len;     // its uint32_t length, 4-byte aligned
  uint64_t status;  // its int32_t status, 4-byte aligned
};
struct ShaBatchGatedLaunch {
  ShaBatchCheckLaunch c;
  const ShaBatchGate *gates;
};
// zlib streams inflated (inflate.hip): one wave per stream, the streams longest
// input first; msgs[w] is wave w's.
struct InflateMsg {
  uint64_t in;   // len bytes, any alignment; never dereferenced when len == 0
  uint64_t out;  // cap bytes, any alignment, not overlapping in
  uint32_t len;
  uint32_t cap;
  uint32_t idx;  // the message's place in the caller's order
  uint32_t reserved;
};
struct InflateLaunch {
  const InflateMsg *msgs;
  uint32_t count;
  uint64_t out_lens, statuses;  // uint32_t / int32_t a message, by idx
  // The unpack chain (0: not given): message idx's input length is
  // min(in_lens[idx], len), and a message whose gate[idx] is not VDS_EC_OK
  // gets that status, out_len 0 and no other work.
  uint64_t in_lens, gate;
};
// The "upload" answer of one message as a websocket frame (base64.hip,
// k_ws_upload_answer_batch: one wave a message).  The few bytes that vary in
// length come from the host: head = the frame header and {"id":"<id>","result":
// {"replicas":[ (head_len <= 61 bytes), tail = ","replica_size":"<size>"}}
// (tail_len <= 31 bytes), both as little-endian words, zero behind their end.
struct WsAnsMsg {
  uint64_t out;   // the frame, any alignment
  uint64_t rdig;  // n digests of 32 bytes back to back, any alignment
  uint64_t ddig;  // the body's digest
  uint32_t n;
  uint32_t head_len;
  uint32_t tail_len;
  uint32_t reserved;
  uint32_t head[16];
  uint32_t tail[9];
  uint32_t pad[3];
};
static_assert(sizeof(WsAnsMsg) == 152, "WsAnsMsg layout");

// Node-to-node datagrams (dgram.hip): HMAC-SHA256 under a session key, one
// lane per message or datagram.  The key pads are hashed once per session ON
// THE HOST (two compressions, sha256_host.cpp): keys[s] holds the SHA-256
// states after the 64-byte block key ^ 0x36.. (inner) and key ^ 0x5c.. (outer),
// so a lane of n bytes costs (n + 8) / 64 + 1 inner compressions and one outer.
struct HmacKeyState {
  uint32_t inner[8];
  uint32_t outer[8];
};
// One lane of k_hmac_sha256_batch / k_dgram_open, in launch order (the host
// orders the lanes by length; `index` is the caller's position).
struct HmacLane {
  uint64_t src;      // len bytes, any alignment (len == 0: never dereferenced)
  uint64_t dst;      // open: where bytes [hdr_len, len - 32) go once verified (0: nowhere)
  uint32_t len;
  uint32_t hdr_len;  // open only; at most len - 32
  uint32_t session;  // keys[session]
  uint32_t index;    // MAC at macs + 32 index, expected + 32 index, verdict at verdicts + index
};
struct HmacBatchLaunch {
  const HmacLane *lanes;
  const HmacKeyState *keys;
  uint32_t count;
  uint64_t macs;      // 0: no MAC written (check only)
  uint64_t expected;  // 0: nothing compared, no verdict written
  uint64_t verdicts;  // 0 equal / 1 different
};
struct DgramOpenLaunch {
  const HmacLane *lanes;
  const HmacKeyState *keys;
  uint32_t count;
  uint64_t verdicts;  // 0 verified / 1 invalid signature / 2 shorter than 33 bytes
};
// One message of k_dgram_seal; its datagrams are lanes first .. first + its
// datagram count - 1 (first ascending), datagram d at out + d * pitch.
// wave_msg[w] is the message that owns lane 64 w (waves + 1 entries, the last
// for lane 64 waves), so a lane finds its message between two entries.
struct DgramSealMsg {
  uint64_t msg;    // len bytes, any alignment
  uint64_t route;  // route_len bytes, any alignment
  uint64_t out;
  uint32_t len;
  uint32_t index0;
  uint32_t route_len;
  uint32_t mtu;
  uint32_t pitch;
  uint32_t session;
  uint32_t first;
  uint32_t type;
};
struct DgramSealLaunch {
  const DgramSealMsg *msgs;
  const HmacKeyState *keys;
  const uint32_t *wave_msg;
  uint32_t lanes;
};

// Bit-sliced runtime-coefficient restore over 512-stripe groups: the first
// groups_per_obj groups of every object as one stream of 4-group tiles.
struct FastRestoreArgs {
  const uint8_t *chunks[kMaxFastK];
  uint64_t chunk_stride;
  uint8_t *out;
  uint64_t out_stride;
  uint32_t groups_per_obj;
  uint32_t total_tiles;
  // k x k inverse, row-major, two coefficients per dword (low half = even
  // column) so the wave-uniform reads are scalar s_load_dword.
  uint32_t matrix2[kMaxFastK * kMaxFastK / 2];
  // regenerate mode (k_restore_bs<..., true>): output m < nt is replica
  // bytes (cells in stripe order) at regen[m] + o * out_stride, the matrix
  // rows are V_targets V_S^{-1} (rows nt.. zero)
  uint8_t *regen[kMaxFastK];
  uint32_t nt;
};

// Erasure-pattern-independent restore (k_restore_syn<K,N>): survivors are K
// distinct points of 0..N-1 (N - K == K / 4).  Syndromes and the fixed
// interpolation are compile-time XOR programs; only the M x M solve
// c_E = R * S (R = W_E^{-1}) is runtime.
struct SynRestoreArgs {
  const uint8_t *chunks[kMaxFastK];  // chunk j holds point point[j]
  uint8_t point[kMaxFastK];
  uint8_t erased[kMaxFastK / 4];     // the M erased points
  uint64_t chunk_stride;
  uint8_t *out;
  uint64_t out_stride;
  uint32_t tiles_per_obj;
  uint32_t total_tiles;
  // R = W_E^{-1} as bit selections: byte (b & 3) of solve_sel[i][b >> 2] has
  // bit j set iff bit b of R[i][j] is set (row i = erased[i], M <= 8)
  uint32_t solve_sel[kMaxFastK / 4][4];
  // regenerate mode (k_restore_syn<..., true>): the recovered point erased[w]
  // is written as replica bytes to regen[w] + o * regen_stride (nullptr: not
  // requested); the interpolation is skipped
  uint8_t *regen[kMaxFastK / 4];
  uint64_t regen_stride;
  // batch mode (launch_restore_syn_batch): everything per object from tables
  const struct SynBatchObj *objs;
  const struct SynBatchPlan *plans;
  const struct SynBatchTile *tiles;
};

constexpr int kInlineCoef = 512;  // regenerate coefficients carried in the kernel arguments

// Generic regenerate (any k, any targets): replica targets[i] of object o is
// sum_j coef[i][j] * chunk_j cell by cell (coef = V_targets V_S^{-1}, nt x k
// row-major), for cells [t_begin, t_begin + t_count), then the trailer (cell
// index T) copied from chunk 0 -- the bytes restore + re-encode would give
// (sync_process.cpp:313-335 -> chunk.h:402-444 then chunk.h:245-281).
struct RegenArgs {
  const uint8_t *chunk_ptr[kInlineChunks];
  const uint8_t *const *chunk_table;  // used when k > kInlineChunks
  uint64_t chunk_stride;
  const uint16_t *coef_dev;           // used when nt * k > kInlineCoef
  uint32_t coef_inline[kInlineCoef / 2];
  uint32_t count;
  uint32_t k;
  uint32_t cell_bytes;
  uint32_t nt;
  uint64_t t_begin;
  uint64_t t_count;
  uint64_t T;
  uint8_t *outs[kMaxLaunchReplicas];
  uint64_t out_stride;
};

// Batched k_restore_syn (per-object survivor sets, sizes and outputs; one
// launch over every tile of every object).  Device tables, built on the host:
// objs[o] per object (its survivors in its plan's point order), plans[p] per
// distinct erased set, tiles[t] per tile.  A tile is two halves of
// kHalfStripes stripes; each half is a stripe range of any object of the
// tile's plan, so small objects (the live 64 KiB ones: 1024 stripes at
// k = 32) pair up instead of filling half a tile each.
constexpr uint32_t kHalfStripes = kTileStripes / 2;
// Runtime-coefficient batch mode (k_restore_syn<..., RT>): survivor sets
// outside the syndrome kernel's points -- the live n = 64 shape losing more
// than k/4 of replicas 0..k+k/4-1, where restore_async's first k found reach
// ids past k+k/4-1 (dht_network_client.cpp:851-901).  Slot j < K of an object
// holds point j when that replica survives, else one of its survivors beyond
// point K-1 ("borrowed" slot: point j itself is erased).  Output row m is a
// combination of the K slots with the coefficients coef[m][0..K): restore:
// the value at the erased point epoint[m] < K (then the fixed interpolation
// from points 0..K-1 gives the object); regenerate: replica epoint[m].  The
// rows are Lagrange over the slots' points, computed on the device
// (launch_rt_coefs) from spoint / epoint.
struct SynBatchRt {
  // ne x K, row-major, slot order (device); coefficient c as the spread word
  // (c & 0xFF) | (c >> 8) << 16, the form the RT walk builds its masks from
  const uint32_t *coef;
  uint64_t borrowed;          // bit j: slot j holds a survivor beyond K-1
  uint32_t ne;                // rows
  uint32_t mode;              // restore, k = 32: 1 = RT2 rows (kRt2MaxRows, below), else 0
  uint8_t epoint[kMaxFastK];  // point of output row m
  uint8_t spoint[kMaxFastK];  // point held by slot j
};
// RT2 (restore, k = 32, every survivor below 2k, at most kRt2MaxRows erased
// points below k): with A the survivors below k, E the erased points and b_j
// the survivor borrowed into slot e_j, P = P0 + Z Q where P0 interpolates the
// values on U = {0..k-1} with zeros at E (so P0(b) is the PERM program's
// permuted sum), Z = prod_{a in A} (X + a) and deg Q < |E|.  Then
//   P(e_m) = sum_j c[m][j] r_j,  r_j = y_(b_j) + P0(b_j),
//   c[m][j] = Z(e_m) prod_{i != j} (e_m + b_i) / (Z(b_j) prod_{i != j} (b_j + b_i)):
// |E| fixed PERM evaluations and |E|^2 runtime products instead of RT's
// |E| k.  coef holds c (row m, column j < ne) in RT's spread form.
// (two groups of r_j through the free LDS slots K..K+7 of the k = 32 kernel;
// above ~12 rows the |E|^2 products cost more than RT's |E| k)
constexpr uint32_t kRt2MaxRows = 12;
struct SynBatchObj {
  const uint8_t *chunks[kMaxFastK];  // survivor j = the chunk of plan point j (K used); RT: of slot j
  uint8_t *out;                      // restore: the object's bytes
  uint8_t *regen[kMaxFastK / 4];     // regenerate: replica erased[w] (nullptr: not requested); RT: of row w
  uint64_t out_len;                  // restore: E bytes to write
  uint64_t chunk_len;                // L = 2 T + 2 bytes of every survivor (and regenerated replica)
  uint32_t plan;                     // its plan (the regenerate tail reads it)
  uint32_t first;                    // plan position (RT: slot) of the caller's chunk 0 (whose trailer restore reads)
  SynBatchRt rt;                     // RT mode only
};
// SMALL batch mode (small-M syndromes, restore_syn.hpp): the survivors lie in
// A = {0..K+MS-1} (MS <= kSmallMaxM), so the MS checks over A and an MS x MS
// solve give the erased points; the rows recovered are erased[0..nrec).
constexpr int kSmallMaxM = 2;
struct SynBatchPlan {
  uint8_t erased[kMaxFastK / 4];  // SMALL: A's MS erased points ascending, then the syndrome slots
  uint8_t point[kMaxFastK];       // the survivors' points, ascending
  union {
    uint32_t solve_sel[kMaxFastK / 4][4];  // as SynRestoreArgs::solve_sel
    // SMALL: bit b of small_mask[m][j][i] = bit i of R[m][j] x^b (R = W_E^{-1}):
    // output plane i of recovered row m is the XOR over j, b of syndrome j's
    // plane b where the bit is set
    uint16_t small_mask[kSmallMaxM][kSmallMaxM][16];
  };
  uint32_t nrec;  // SMALL: rows recovered (restore: erased points below K; regenerate: MS; 0 = none)
  uint32_t cls;   // MULTI: the plan's phase 2 (kClsSyn, kClsSmall1, kClsSmall2, kClsPerm; restore_syn.hpp)
};
struct SynBatchTile {
  uint32_t obj[2];      // object of each half (an unused half: the batch's empty object)
  uint32_t stripe0[2];  // its first stripe
  uint32_t plan;        // (RT: unused)
  uint32_t trailer;     // regenerate: bit h = half h also copies its object's trailer cell
  uint32_t nm;          // RT: rows of the tile = max ne over its halves
  uint32_t mode;        // RT: SynBatchRt::mode of both halves (the host never pairs two modes); else kTileDual or 0
};
// mode of a syndrome-route tile whose halves are objects of different
// plans (plan = half 0's; half 1's from its object: restore_syn.hpp kDual)
constexpr uint32_t kTileDual = 2;

// Reference-route tail of a regenerate.  The reference repairs a replica by
// restoring the object -- trimmed to E bytes (chunk.h:415-419, 437-438) --
// and re-encoding it: the last stripe zero-padded past E, trailer E mod 2k
// (chunk.h:251-275; sync_process.cpp:313-335 -> dht_network_client.cpp:582-658).
// The main regenerate kernels write P(t) of the untrimmed decode.  The two
// agree on every cell but the last, and there only when the survivors are
// not one codeword (a codeword's decode is already zero past E).  These
// kernels rewrite, after the main ones on the same stream, the last cell and
// the trailer of every target replica as the reference route writes them:
// with p = the trailer of the caller's first survivor (the one restore reads,
// chunk.h:408) and 0 < p < 2k, the decoded last stripe keeps bytes [0, p)
// only.  p == 0 or p == 2k trim nothing (trailer 0 for both: E mod 2k).
// p > 2k leaves the replica as the main kernels wrote it: the reference's
// route either fails ("Fatal error", p > 4k) or writes a replica 2 bytes
// longer than its survivors, so there is no chunk_size-byte answer; the host
// entry points reject such survivors (VDS_EC_ERESTORE).
struct RegenTailArgs {  // one survivor set, `count` objects at strides, any k
  const uint8_t *chunk_ptr[kInlineChunks];
  const uint8_t *const *chunk_table;  // used when k > kInlineChunks
  uint64_t chunk_stride;
  const uint16_t *matrix_dev;  // V_S^{-1} (k x k row-major) when k > kInlineMatrixK
  uint32_t matrix_inline[kInlineMatrixK * kInlineMatrixK / 2];
  uint64_t chunk_size;  // L = 2 T + 2
  uint32_t k, count, nt;
  uint16_t targets[kMaxLaunchReplicas];
  uint8_t *outs[kMaxLaunchReplicas];
  uint64_t out_stride;
};
#ifndef __HIPCC_RTC__
hipError_t launch_regen_tail(const RegenTailArgs &a, hipStream_t s);
// The batched k_restore_syn regenerate's objects objs[0..count) (device
// tables of the batch launch; survivor points from their plans, targets the
// plans' erased points with regen[w] set): the last stripe interpolated on
// the device, one wave per object (k <= 64).
hipError_t launch_regen_tail_batch(uint32_t k, uint32_t m, const SynBatchObj *objs, const SynBatchPlan *plans,
                                   uint32_t count, hipStream_t s);
// The same for RT objects (survivor points rt.spoint, targets rt.epoint[0..ne)).
hipError_t launch_regen_tail_rt(uint32_t k, const SynBatchObj *objs, uint32_t count, hipStream_t s);
// RT coefficient rows of objs[0..count) (one wave per object, k <= 64): row m,
// column j = l_j(epoint[m]), the Lagrange basis polynomial of slot j over the
// slots' points spoint evaluated at epoint[m] -- the unique polynomial through
// the k survivors, evaluated where it is needed.
hipError_t launch_rt_coefs(uint32_t k, const SynBatchObj *objs, uint32_t count, hipStream_t s);
// Batched RT restore / regenerate: a.objs / a.tiles / a.total_tiles set (every
// object's rt filled, its coef rows computed); regenerate rows ne <= n - k.
hipError_t launch_restore_rt_batch(uint32_t k, uint32_t n, const SynRestoreArgs &a, hipStream_t s, bool regen);

hipError_t launch_encode_generic(const GenericEncodeArgs &a, hipStream_t s);
bool has_restore_syn(uint32_t k, uint32_t n);
// W[j][a] = v_a a^j of the syndrome map for (k, n); nullptr if not compiled.
const uint16_t *restore_syn_weights(uint32_t k, uint32_t n);
hipError_t launch_restore_syn(uint32_t k, uint32_t n, const SynRestoreArgs &a, hipStream_t s, bool regen = false);
// The run-time compiled restore kernel of a's survivor set (vds_ec_jit.cpp) on
// the current device, or nullptr (disabled, not compiled yet -- then queued --
// or failed): a.point[0..k) set by the plan.
hipFunction_t jit_restore_function(uint32_t k, uint32_t n, const SynRestoreArgs &a, bool regen = false);
// the set's kernel is loaded and the module is enabled (path queries)
bool jit_ready(uint32_t k, uint32_t n, const SynRestoreArgs &a, bool regen);
bool jit_enabled();  // mode != 0 (vds_ec_jit_set_mode)
hipError_t launch_restore_syn_jit(hipFunction_t fn, uint32_t k, uint32_t n, const SynRestoreArgs &a, hipStream_t s);
// a.objs / a.plans / a.tiles / a.total_tiles set; the other fields unused
hipError_t launch_restore_syn_batch(uint32_t k, uint32_t n, const SynRestoreArgs &a, hipStream_t s, bool regen);
// SMALL batch mode over the points 0..k+ms-1 (ms = 1, 2; k = 16, 32): tables as
// launch_restore_syn_batch, plans with small_mask / nrec.
bool has_restore_small(uint32_t k, uint32_t ms);
// W[j][a] = v_a a^j of the ms checks over A = {0..k+ms-1}; nullptr if not compiled.
const uint16_t *restore_small_weights(uint32_t k, uint32_t ms);
hipError_t launch_restore_small_batch(uint32_t k, uint32_t ms, const SynRestoreArgs &a, hipStream_t s, bool regen);
// PERM batch regenerate (k = 16, 32): survivors exactly 0..k-1, one target
// t = erased[0] of each plan in k..2k-1.
hipError_t launch_regen_perm_batch(uint32_t k, const SynRestoreArgs &a, hipStream_t s);
// MULTI: one launch over tiles of every class, each plan's cls choosing its
// phase 2 (k = 16, 32).
hipError_t launch_restore_multi_batch(uint32_t k, const SynRestoreArgs &a, hipStream_t s, bool regen);
hipError_t launch_regen_generic(const RegenArgs &a, hipStream_t s);
hipError_t launch_restore_generic(const GenericRestoreArgs &a, hipStream_t s);
// Returns hipErrorNotSupported when no bit-sliced instantiation exists for (k, n).
hipError_t launch_encode_fast(uint32_t k, uint32_t n, const FastEncodeArgs &a, hipStream_t s);
bool has_encode_fast(uint32_t k, uint32_t n);
// The batch kernel's shapes: (16,20), (32,40), (32,64).  The launch returns
// hipErrorNotSupported for any other (a missing kernel is an error).
bool has_encode_batch(uint32_t k, uint32_t n);
hipError_t launch_encode_batch(uint32_t k, uint32_t n, const EncBatchLaunch &b, hipStream_t s);
// SHA-256 of one message on the calling CPU thread (sha256_host.cpp)
void sha256_host(const uint8_t *data, uint64_t len, uint8_t out[32]);
hipError_t launch_restore_fast(uint32_t k, const FastRestoreArgs &a, hipStream_t s, bool regen = false);
bool has_restore_fast(uint32_t k);
// SHA-256 of count messages of len bytes at base + j * stride -> digests + 32 j (sha256.hip).
hipError_t launch_sha256(const uint8_t *base, uint64_t len, uint64_t stride, uint32_t count, uint8_t *digests,
                         hipStream_t s);
// SHA-256 of every message of b's groups, each digest at its group's address (sha256.hip).
hipError_t launch_sha256_batch(const ShaBatchLaunch &b, hipStream_t s);
// The same, and every group's check (ShaBatchCheck) in the same launch.
hipError_t launch_sha256_check_batch(const ShaBatchCheckLaunch &c, hipStream_t s);
// HMAC-SHA256 of every lane's message; sealing and opening of datagrams (dgram.hip).
hipError_t launch_hmac_sha256_batch(const HmacBatchLaunch &b, hipStream_t s);
hipError_t launch_dgram_seal(const DgramSealLaunch &b, hipStream_t s);
// lane_copy: each lane copies its own payload (the A/B arm), else the wave copies them one after the other
hipError_t launch_dgram_open(const DgramOpenLaunch &b, hipStream_t s, bool lane_copy = false);
// The SHA-256 compression of sha256_host.cpp over nblocks 64-byte blocks, and
// HMAC-SHA256 on the calling thread: the states after the two key pad blocks
// (any key length; a key longer than 64 bytes is hashed first), and a whole MAC.
void sha256_host_blocks(uint32_t h[8], const uint8_t *p, size_t nblocks);
void hmac_sha256_host_midstates(const uint8_t *key, size_t key_len, uint32_t inner[8], uint32_t outer[8]);
void hmac_sha256_host(const uint8_t *key, size_t key_len, const uint8_t *data, uint64_t len, uint8_t mac[32]);
// base64 -> bytes of msgs[0..count) (device table), every status written (base64.hip).
hipError_t launch_b64_decode_batch(const B64DecMsg *msgs, uint32_t count, hipStream_t s);
// The same for texts under their websocket masks: masks[w] beside msgs[w].
hipError_t launch_b64_decode_masked_batch(const B64DecMsg *msgs, const uint32_t *masks, uint32_t count,
                                          hipStream_t s);
// The "upload" answer frames of msgs[0..count) (device table).
hipError_t launch_ws_upload_answer_batch(const WsAnsMsg *msgs, uint32_t count, hipStream_t s);
// bytes -> base64 over tiles[0..ntiles) of msgs (device tables).
hipError_t launch_b64_encode_batch(const B64EncMsg *msgs, const B64EncTile *tiles, uint32_t ntiles, hipStream_t s);
// The same behind gates[0..) (beside msgs); every message's status written by its tile 0.
hipError_t launch_b64_encode_gated_batch(const B64EncMsg *msgs, const B64EncGate *gates, const B64EncTile *tiles,
                                         uint32_t ntiles, hipStream_t s);
// AES-256-CBC (aes.hip): the chains msgs[0..count) (device table, longest first), keys / ivs by
// AesEncMsg::idx; lane_chain: one lane a chain instead of one quad (the A/B arm).  And the tiled decrypt.
hipError_t launch_aes_encrypt_batch(const AesEncMsg *msgs, uint32_t count, const uint8_t *keys, const uint8_t *ivs,
                                    hipStream_t s, bool lane_chain = false);
// The gated encrypt: chain idx is the first min(lens[idx], AesEncMsg::len) bytes (lens: device, the host
// ordered by the upper bound AesEncMsg::len), and out_lens[idx] (device) receives what they encrypt to.
hipError_t launch_aes_encrypt_gated_batch(const AesEncMsg *msgs, uint32_t count, const uint8_t *keys,
                                          const uint8_t *ivs, const uint32_t *lens, uint32_t *out_lens, hipStream_t s);
hipError_t launch_aes_decrypt_batch(const AesDecLaunch &l, hipStream_t s);
// The gated name check of the unpack chain (sha256.hip), and the inflate of a batch (inflate.hip).
hipError_t launch_sha256_gated_batch(const ShaBatchGatedLaunch &g, hipStream_t s);
hipError_t launch_inflate_batch(const InflateLaunch &l, hipStream_t s);
// The deflate of a batch (deflate.hip): one wave a message, msgs (device table, longest first) in the
// inflate's layout with cap at least the deflate's bound; out_lens: uint32_t a message, by idx.
hipError_t launch_deflate_batch(const InflateMsg *msgs, uint32_t count, uint32_t *out_lens, hipStream_t s);
// One message on the calling CPU thread (aes_host.cpp); the decrypt returns its status.
void aes256_cbc_encrypt_host(const uint8_t key[32], const uint8_t iv[16], const uint8_t *in, uint64_t len,
                             uint8_t *out);
int aes256_cbc_decrypt_host(const uint8_t key[32], const uint8_t iv[16], const uint8_t *in, uint64_t len, uint8_t *out,
                            uint64_t *out_len);
hipError_t launch_fill_splitmix(uint8_t *dst, uint64_t size, uint64_t seed, hipStream_t s);
// Device -> mapped pinned host copy by a kernel (dst: the device view of the
// host buffer; both 16-byte aligned).
hipError_t launch_push(uint8_t *dst_host_dev, const uint8_t *src, uint64_t bytes, hipStream_t s);

#endif  // __HIPCC_RTC__

}  // namespace vds_ec
