// vds_ec_wire.cpp -- the byte formats on either side of the codec on the live
// upload path, host code:
//
//   websocket "upload" -> base64 body (websocket_api.cpp:141-155,
//   base64::to_bytes, encoding.cpp:181-247) -> server_api::upload_data
//   (server_api.cpp:12-30: data hash = SHA-256 of the body) -> save_temp
//   (dht_network_client.cpp:62-107: every replica written, hashed, and kept
//   in <root>/tmp/<base64 of its hash, '+' -> '#', '/' -> '_'>) -> the JSON
//   answer {"replicas":[...],"hash":...,"replica_size":...}
//   (websocket_api.cpp:467-485, serialised by json_writer.cpp).
//
// The arithmetic in between (encode + the SHA-256 of every replica and of the
// body) runs on the GPU: vds_ec_save_temp16_host (vds_ec_api.cpp).
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/vds_ec.h"

namespace {

const char kB64[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";

// base64::from_bytes (encoding.cpp:138-174): standard alphabet, '=' padding.
std::string b64(const uint8_t *d, size_t len) {
  std::string s;
  s.reserve((len + 2) / 3 * 4);
  for (; len > 2; len -= 3, d += 3) {
    const uint32_t t = (uint32_t(d[0]) << 16) | (uint32_t(d[1]) << 8) | d[2];
    s += kB64[(t >> 18) & 63];
    s += kB64[(t >> 12) & 63];
    s += kB64[(t >> 6) & 63];
    s += kB64[t & 63];
  }
  if (len == 1) {
    const uint32_t t = uint32_t(d[0]) << 16;
    s += kB64[(t >> 18) & 63];
    s += kB64[(t >> 12) & 63];
    s += "==";
  } else if (len == 2) {
    const uint32_t t = (uint32_t(d[0]) << 16) | (uint32_t(d[1]) << 8);
    s += kB64[(t >> 18) & 63];
    s += kB64[(t >> 12) & 63];
    s += kB64[(t >> 6) & 63];
    s += '=';
  }
  return s;
}

int copy_out(const std::string &s, char *out, size_t cap, size_t *out_len) {
  if (out_len) *out_len = s.size();
  if (!out) return VDS_EC_OK;  // size query
  if (cap < s.size() + 1) return VDS_EC_EINVAL;
  std::memcpy(out, s.data(), s.size());
  out[s.size()] = 0;
  return VDS_EC_OK;
}

// json_object::add_property(name, int) stores std::to_string of the value as
// vds_ec_upload_response_json prints it: a negative id as its 64-bit two's
// complement.
std::string id_text(int id) { return std::to_string((uint64_t)(int64_t)id); }

// json_writer::write_string's escapes (json_writer.cpp:205-240), without the quotes
std::string json_escaped(const char *s) {
  static const char kHex[] = "0123456789abcdef";
  std::string o;
  for (; *s; ++s) {
    const unsigned char ch = (unsigned char)*s;
    switch (ch) {
      case '\\': o += "\\\\"; break;
      case '"': o += "\\\""; break;
      case '\n': o += "\\n"; break;
      case '\r': o += "\\r"; break;
      case '\b': o += "\\b"; break;
      case '\t': o += "\\t"; break;
      case '\f': o += "\\f"; break;
      default:
        if (ch >= 0x20 && ch < 0x7F) {
          o += (char)ch;
        } else {
          o += "\\u00";
          o += kHex[ch >> 4];
          o += kHex[ch & 15];
        }
    }
  }
  return o;
}

uint32_t ws_header(uint64_t payload_len, bool binary, uint8_t out[10]) {
  out[0] = binary ? 0x82 : 0x81;
  if (payload_len < 126) {
    out[1] = (uint8_t)payload_len;
    return 2;
  }
  if (payload_len <= 0xFFFF) {
    out[1] = 126;
    out[2] = (uint8_t)(payload_len >> 8);
    out[3] = (uint8_t)payload_len;
    return 4;
  }
  out[1] = 127;
  for (int i = 0; i < 8; ++i) out[2 + i] = (uint8_t)(payload_len >> (56 - 8 * i));
  return 10;
}

const char kUpReqHead[] = "{\"id\":";
const char kUpReqMid[] = ",\"invoke\":\"upload\",\"params\":[\"";
const char kUpReqTail[] = "\"]}";
const char kAnsHead[] = "{\"id\":\"";
const char kUpAnsMid[] = "\",\"result\":{\"replicas\":[";
const char kUpAnsHash[] = "],\"hash\":\"";
const char kUpAnsSize[] = "\",\"replica_size\":\"";
const char kUpAnsTail[] = "\"}}";
const char kDownAnsMid[] = "\",\"result\":\"";
const char kErrAnsMid[] = "\",\"error\":\"";
const char kAnsTail[] = "\"}";
template <size_t N>
constexpr size_t lit(const char (&)[N]) {
  return N - 1;
}

}  // namespace

extern "C" {

int vds_ec_ws_frame_parse(const uint8_t *buf, size_t len, vds_ec_ws_frame *frame) {
  if ((len && !buf) || !frame) return VDS_EC_EINVAL;
  std::memset(frame, 0, sizeof(*frame));
  if (len < 2) {
    frame->need = 2;
    return VDS_EC_EWS_SHORT;
  }
  const bool masked = (buf[1] & 0x80) != 0;
  const uint32_t l7 = buf[1] & 0x7F;
  const uint32_t off = l7 == 126 ? 4 : l7 == 127 ? 10 : 2;
  const uint32_t hdr = off + (masked ? 4 : 0);
  if (len < hdr) {
    frame->need = hdr;
    return VDS_EC_EWS_SHORT;
  }
  frame->fin = (buf[0] & 0x80) != 0;
  frame->rsv1 = (buf[0] & 0x40) != 0;
  frame->rsv2 = (buf[0] & 0x20) != 0;
  frame->rsv3 = (buf[0] & 0x10) != 0;
  frame->opcode = buf[0] & 0x0F;
  frame->masked = masked;
  frame->header_len = frame->need = hdr;
  uint64_t pl = l7;
  if (l7 == 126) {
    pl = (uint64_t)buf[2] << 8 | buf[3];
  } else if (l7 == 127) {
    pl = 0;
    for (int i = 0; i < 8; ++i) pl = pl << 8 | buf[2 + i];
  }
  frame->payload_len = pl;
  if (masked) std::memcpy(frame->mask, buf + off, 4);
  return frame->opcode == 1 || frame->opcode == 2 || frame->opcode == 9 ? VDS_EC_OK : VDS_EC_EWS_FRAME;
}

int vds_ec_ws_frame_header(uint64_t payload_len, int binary, uint8_t out[10], uint32_t *len) {
  if (!out || !len) return VDS_EC_EINVAL;
  *len = ws_header(payload_len, binary != 0, out);
  return VDS_EC_OK;
}

int vds_ec_ws_upload_request(const uint8_t *payload, uint64_t len, const uint8_t *mask, int32_t *id,
                             uint64_t *body_off, uint64_t *body_len, uint64_t *decoded_size) {
  if ((len && !payload) || !id || !body_off || !body_len || !decoded_size) return VDS_EC_EINVAL;
  const uint8_t zero[4] = {0, 0, 0, 0};
  const uint8_t *mk = mask ? mask : zero;
  // the envelope's front: 6 + at most 10 digits + 30 = 46 bytes, and two more
  uint8_t head[48];
  const size_t nh = (size_t)(len < sizeof(head) ? len : sizeof(head));
  for (size_t j = 0; j < nh; ++j) head[j] = payload[j] ^ mk[j & 3];
  size_t at = lit(kUpReqHead);
  if (nh < at + 1 || std::memcmp(head, kUpReqHead, at)) return VDS_EC_EWS_FORM;
  uint64_t v = 0;
  size_t nd = 0;
  while (at + nd < nh && nd < 11 && head[at + nd] >= '0' && head[at + nd] <= '9') v = v * 10 + (head[at + nd++] - '0');
  if (nd == 0 || nd > 10 || (nd > 1 && head[at] == '0') || v > 0x7FFFFFFFull) return VDS_EC_EWS_FORM;
  at += nd;
  if (nh < at + lit(kUpReqMid) || std::memcmp(head + at, kUpReqMid, lit(kUpReqMid))) return VDS_EC_EWS_FORM;
  at += lit(kUpReqMid);
  if (len < at + lit(kUpReqTail)) return VDS_EC_EWS_FORM;
  // the envelope's end and the body's last two characters
  const uint64_t blen = len - at - lit(kUpReqTail);
  uint8_t tail[5];
  for (uint64_t j = len - 5; j < len; ++j) tail[j - (len - 5)] = payload[j] ^ mk[j & 3];  // (len >= 40)
  if (std::memcmp(tail + 2, kUpReqTail, lit(kUpReqTail))) return VDS_EC_EWS_FORM;
  uint64_t size = 0;
  if (blen && blen % 4 == 0) size = blen / 4 * 3 - (tail[1] != '=' ? 0 : tail[0] != '=' ? 1 : 2);
  *id = (int32_t)v;
  *body_off = at;
  *body_len = blen;
  *decoded_size = size;
  return VDS_EC_OK;
}

int vds_ec_ws_upload_answer_size(int id, uint32_t n, uint32_t replica_size, uint64_t *frame_len,
                                 uint32_t *header_len) {
  const uint64_t json = lit(kAnsHead) + id_text(id).size() + lit(kUpAnsMid) + 46ull * n + (n ? n - 1 : 0) +
                        lit(kUpAnsHash) + 44 + lit(kUpAnsSize) + std::to_string((uint64_t)replica_size).size() +
                        lit(kUpAnsTail);
  uint8_t h[10];
  const uint32_t hl = ws_header(json, false, h);
  if (frame_len) *frame_len = hl + json;
  if (header_len) *header_len = hl;
  return VDS_EC_OK;
}

int vds_ec_ws_download_answer_layout(int id, uint64_t object_size, uint64_t *frame_len, uint32_t *header_len,
                                     uint64_t *text_off) {
  if (object_size > 0xFFFFFFFFFFFFFF00ull / 2) return VDS_EC_EINVAL;
  const uint64_t front = lit(kAnsHead) + id_text(id).size() + lit(kDownAnsMid);
  const uint64_t json = front + (object_size + 2) / 3 * 4 + lit(kAnsTail);
  uint8_t h[10];
  const uint32_t hl = ws_header(json, false, h);
  if (frame_len) *frame_len = hl + json;
  if (header_len) *header_len = hl;
  if (text_off) *text_off = hl + front;
  return VDS_EC_OK;
}

int vds_ec_ws_error_answer(int id, int status, uint8_t *out, size_t cap, size_t *out_len) {
  const std::string json = kAnsHead + id_text(id) + kErrAnsMid + json_escaped(vds_ec_strerror(status)) + kAnsTail;
  uint8_t h[10];
  const uint32_t hl = ws_header(json.size(), false, h);
  if (out_len) *out_len = hl + json.size();
  if (!out) return VDS_EC_OK;  // size query
  if (cap < hl + json.size()) return VDS_EC_EINVAL;
  std::memcpy(out, h, hl);
  std::memcpy(out + hl, json.data(), json.size());
  return VDS_EC_OK;
}

size_t vds_ec_base64_decoded_size(const char *in, size_t len) {
  if (!in || len % 4) return 0;
  size_t padding = 0;
  if (len > 0 && in[len - 1] == '=') {
    ++padding;
    if (len > 1 && in[len - 2] == '=') ++padding;
  }
  return len / 4 * 3 - padding;
}

// base64::to_bytes (encoding.cpp:181-247), quirks kept: the output length is
// (len/4)*3 minus the '=' among the LAST TWO characters; the first '=' met
// ends the decode (whatever follows it) and emits one or two bytes by that
// trailing count; a '=' when the string does not end in one is "Invalid
// Padding"; any other character outside the alphabet (bytes >= 0x80
// included) is "Non-Valid Character".  Bytes of the output the reference
// leaves unwritten on such an early '=' (uninitialised malloc memory there)
// are zero here.
int vds_ec_base64_decode(const char *in, size_t len, uint8_t *out, size_t *out_len) {
  if ((len && !in) || !out_len) return VDS_EC_EINVAL;
  if (len % 4) return VDS_EC_EB64_LENGTH;
  const size_t size = vds_ec_base64_decoded_size(in, len);
  size_t padding = len / 4 * 3 - size;
  if (size && !out) return VDS_EC_EINVAL;
  if (size) std::memset(out, 0, size);
  uint32_t temp = 0;
  size_t offset = 0;
  int quantum = 0;
  for (size_t i = 0; i < len; ++i) {
    const char ch = in[i];
    temp <<= 6;
    if (ch >= 'A' && ch <= 'Z') {
      temp |= uint32_t(ch - 'A');
    } else if (ch >= 'a' && ch <= 'z') {
      temp |= uint32_t(ch - 'a' + 26);
    } else if (ch >= '0' && ch <= '9') {
      temp |= uint32_t(ch - '0' + 52);
    } else if (ch == '+') {
      temp |= 62u;
    } else if (ch == '/') {
      temp |= 63u;
    } else if (ch == '=') {
      if (padding == 1) {
        out[offset++] = uint8_t(temp >> 16);
        out[offset] = uint8_t(temp >> 8);
      } else if (padding == 2) {
        out[offset] = uint8_t(temp >> 10);
      } else {
        return VDS_EC_EB64_PADDING;
      }
      *out_len = size;
      return VDS_EC_OK;
    } else {
      return VDS_EC_EB64_CHAR;
    }
    if (++quantum == 4) {
      out[offset++] = uint8_t(temp >> 16);
      out[offset++] = uint8_t(temp >> 8);
      out[offset++] = uint8_t(temp);
      quantum = 0;
    }
  }
  *out_len = size;
  return VDS_EC_OK;
}

int vds_ec_base64_encode(const uint8_t *in, size_t len, char *out, size_t cap, size_t *out_len) {
  if (len && !in) return VDS_EC_EINVAL;
  return copy_out(b64(in, len), out, cap, out_len);
}

// save_temp's tmp-file names (dht_network_client.cpp:91-95): base64 of the
// replica's SHA-256 with '+' -> '#' and '/' -> '_', unsplit (the storage
// paths of save_data split it, vds_ec_replica_paths).  count names of
// VDS_EC_NAME_BYTES (44 characters + NUL) each.
int vds_ec_tmp_names(const uint8_t *digests, uint32_t count, char *out) {
  if (count && (!digests || !out)) return VDS_EC_EINVAL;
  for (uint32_t i = 0; i < count; ++i) {
    std::string s = b64(digests + 32ull * i, 32);
    for (char &c : s) c = c == '+' ? '#' : c == '/' ? '_' : c;
    std::memcpy(out + (size_t)VDS_EC_NAME_BYTES * i, s.c_str(), s.size() + 1);
  }
  return VDS_EC_OK;
}

// The websocket answer to "upload": process_message's {"id": id} with the
// "result" object websocket_api::upload adds (websocket_api.cpp:120-121,
// 472-482), as json_writer writes it: no whitespace, every primitive a
// quoted string (json_primitive holds text, json_writer.cpp:20-41), numbers
// included (json_object::add_property(name, uint64_t) stores to_string).
int vds_ec_upload_response_json(int id, const uint8_t *replica_digests, uint32_t n, const uint8_t *data_digest,
                                 uint32_t replica_size, char *out, size_t cap, size_t *out_len) {
  if ((n && !replica_digests) || !data_digest) return VDS_EC_EINVAL;
  std::string s = "{\"id\":\"" + std::to_string((uint64_t)(int64_t)id) + "\",\"result\":{\"replicas\":[";
  for (uint32_t i = 0; i < n; ++i) {
    if (i) s += ',';
    s += '"' + b64(replica_digests + 32ull * i, 32) + '"';
  }
  s += "],\"hash\":\"" + b64(data_digest, 32) + "\",\"replica_size\":\"" + std::to_string((uint64_t)replica_size) +
       "\"}}";
  return copy_out(s, out, cap, out_len);
}

// How prepare_to_send cuts a message (impl/dht_datagram_protocol.cpp:335-541):
// total = 1 + 4 + route + message + 32; below the mtu it is one datagram, else
// the first carries BE32(size) too and is exactly mtu bytes, and each
// continuation carries up to mtu - 37 bytes.
int vds_ec_dgram_layout(uint32_t mtu, uint32_t route_len, uint64_t msg_len, uint32_t *count, uint32_t *first_payload,
                        uint32_t *last_len) {
  if (mtu < 508 || mtu > 65535 || msg_len > 0xFFFFFFFFull) return VDS_EC_EINVAL;
  const bool proxy = route_len >= 33 && (route_len - 33) % 32 == 0 && (route_len - 33) / 32 < 256;
  const bool route_ok = route_len == 0 || route_len == 32 || proxy;
  if (!route_ok || 41ull + route_len >= mtu) return VDS_EC_EINVAL;
  uint32_t n = 1, c0 = (uint32_t)msg_len, last = 0;
  if (37ull + route_len + msg_len < mtu) {
    last = 37 + route_len + (uint32_t)msg_len;
  } else {
    c0 = mtu - (41 + route_len);
    const uint64_t per = mtu - 37, rest = msg_len - c0;
    n = 1 + (uint32_t)((rest + per - 1) / per);
    last = 37 + (uint32_t)(rest - (uint64_t)(n - 2) * per);
  }
  if (count) *count = n;
  if (first_payload) *first_payload = c0;
  if (last_len) *last_len = last;
  return VDS_EC_OK;
}

// binary_serializer::write_number (binary_serialize.cpp:44-66): one byte below
// 128, else 0x80 | n and the n big-endian bytes of value - 128.
int vds_ec_write_number(uint64_t value, uint8_t *out, uint32_t *len) {
  if (!out || !len) return VDS_EC_EINVAL;
  if (value < 128) {
    out[0] = (uint8_t)value;
    *len = 1;
    return VDS_EC_OK;
  }
  value -= 128;
  uint8_t data[8];
  int index = 0;
  do {
    data[index++] = (uint8_t)(value & 0xFF);
    value >>= 8;
  } while (value != 0);
  uint32_t at = 0;
  out[at++] = (uint8_t)(0x80 | index);
  while (index > 0) out[at++] = data[--index];
  *len = at;
  return VDS_EC_OK;
}

}  // extern "C"
