"""Host side of the websocket layer (vds_ec_ws_*): the frame header rules, the
recogniser of the "upload" request's fast form, the answers' arithmetic and
the error answer, against Python restatements (struct, plain string building,
XOR), and the argument validation of the device and host-batch entry points,
which runs before anything is enqueued and before the device is looked for.
No GPU: the device pointers are fabricated integers, nothing dereferences them."""
import base64
import ctypes as C
import os
import re
import struct

import numpy as np

from vds_amd import _lib, chunk

K, N = 32, 64
DEV = 0x7F0000000000  # fabricated device addresses
I32P, U32P = _lib.i32p, _lib.u32p


# ------------------------------------------------------------- restatements
def frame_header(payload_len, opcode=1, fin=1, rsv=0, mask=None):
    b0 = (fin << 7) | (rsv << 4) | opcode
    mb = 0x80 if mask is not None else 0
    if payload_len < 126:
        h = struct.pack(">BB", b0, mb | payload_len)
    elif payload_len <= 0xFFFF:
        h = struct.pack(">BBH", b0, mb | 126, payload_len)
    else:
        h = struct.pack(">BBQ", b0, mb | 127, payload_len)
    return h + (bytes(mask) if mask is not None else b"")


def xor_mask(payload, mask):
    p = np.frombuffer(bytes(payload), dtype=np.uint8)
    return (p ^ np.resize(np.frombuffer(bytes(mask), dtype=np.uint8), p.size)).tobytes() if p.size else b""


def id_text(i):
    return str(i % (1 << 64))


def upload_json_len(i, n, rs):
    return len('{"id":"%s","result":{"replicas":[' % id_text(i)) + 46 * n + max(n - 1, 0) + \
        len('],"hash":"') + 44 + len('","replica_size":"%d"}}' % rs)


def answer_frame(json_bytes):
    return frame_header(len(json_bytes)) + json_bytes


def error_frame(i, message):
    return answer_frame(('{"id":"%s","error":"%s"}' % (id_text(i), message)).encode())


def request(i, body, head='{"id":%s,"invoke":"upload","params":["', tail='"]}'):
    return (head % i).encode() + body + tail.encode()


def _no_device(lib):
    cnt = C.c_int(0)
    assert lib.vds_ec_device_count(C.byref(cnt)) == 0
    return cnt.value == 0


# ------------------------------------------------------------- frame header
PAYLOAD_LENS = (0, 125, 126, 65535, 65536)


def test_frame_parse_lengths_masks_and_truncations(vds_lib):
    for pl in PAYLOAD_LENS:
        for mask in (None, b"\x00\x00\x00\x00", b"\x12\xfe\x00\x7f"):
            h = frame_header(pl, mask=mask)
            rc, f = chunk.ws_frame_parse(h + b"xyz")
            assert rc == _lib.OK
            assert (f["fin"], f["rsv1"], f["rsv2"], f["rsv3"], f["opcode"]) == (1, 0, 0, 0, 1)
            assert f["masked"] == (mask is not None) and f["mask"] == (mask or bytes(4))
            assert f["header_len"] == len(h) == f["need"] and f["payload_len"] == pl
            assert len(h) == (2 if pl < 126 else 4 if pl < 65536 else 10) + (4 if mask is not None else 0)
            # every truncation of the header: how many bytes are needed
            for cut in range(len(h)):
                rc, f = chunk.ws_frame_parse(h[:cut])
                assert rc == _lib.EWS_SHORT, (pl, mask, cut)
                assert f["need"] == (2 if cut < 2 else len(h)), (pl, mask, cut)
            assert chunk.ws_frame_parse(h)[0] == _lib.OK


def test_frame_parse_opcodes_fin_and_rsv(vds_lib):
    for op in range(16):
        rc, f = chunk.ws_frame_parse(frame_header(5, opcode=op, mask=b"abcd") + b"12345")
        assert rc == (_lib.OK if op in (1, 2, 9) else _lib.EWS_FRAME), op
        assert f["opcode"] == op and f["payload_len"] == 5 and f["header_len"] == 6
    # FIN = 0 and the RSV bits are reported and not rejected
    for fin in (0, 1):
        for rsv in range(8):
            rc, f = chunk.ws_frame_parse(frame_header(300, opcode=2, fin=fin, rsv=rsv))
            assert rc == _lib.OK
            assert (f["fin"], f["rsv1"], f["rsv2"], f["rsv3"]) == (fin, rsv >> 2 & 1, rsv >> 1 & 1, rsv & 1)
            assert f["payload_len"] == 300 and f["header_len"] == 4
    assert vds_lib.vds_ec_ws_frame_parse(None, 3, C.byref(_lib.WsFrame())) == _lib.EINVAL
    assert vds_lib.vds_ec_ws_frame_parse(b"\x81\x00", 2, None) == _lib.EINVAL
    assert _lib.strerror(_lib.EWS_FRAME) == "Not implemented"


def test_frame_header_build(vds_lib):
    for pl in PAYLOAD_LENS + (1, 127, 65534, 1 << 32, (1 << 63) + 5):
        for binary in (False, True):
            assert chunk.ws_frame_header(pl, binary) == frame_header(pl, opcode=2 if binary else 1), pl
    n = C.c_uint32(0)
    assert vds_lib.vds_ec_ws_frame_header(5, 0, None, C.byref(n)) == _lib.EINVAL


# --------------------------------------------------------------- recogniser
BODY = base64.b64encode(bytes(range(7, 107)))  # 136 characters, ends in "=="
ACCEPTED = [  # (payload, id, body)
    (request(0, BODY), 0, BODY),
    (request(7, BODY), 7, BODY),
    (request(2147483647, BODY), 2147483647, BODY),
    (request(5, b""), 5, b""),
    (request(5, b"QUJD"), 5, b"QUJD"),
    (request(5, b"QUI="), 5, b"QUI="),
    (request(5, b"QQ=="), 5, b"QQ=="),
    (request(12, base64.b64encode(bytes(300))), 12, base64.b64encode(bytes(300))),
    (request(12, base64.b64encode(bytes(301))), 12, base64.b64encode(bytes(301))),
    (request(12, base64.b64encode(bytes(302))), 12, base64.b64encode(bytes(302))),
    (request(3, b"QUJ"), 3, b"QUJ"),              # a length the decode rejects: still the fast form
    (request(3, b'QU"D'), 3, b'QU"D'),            # a '"' in the body is the decode's to catch
    (request(3, b"=" * 8), 3, b"=" * 8),
]
REJECTED = [
    request(2147483648, BODY), request("01", BODY), request(-1, BODY), request("", BODY), request("1.0", BODY),
    request("99999999999", BODY), request('"5"', BODY),
    b'{"invoke":"upload","id":5,"params":["' + BODY + b'"]}',         # key order
    b'{"id": 5,"invoke":"upload","params":["' + BODY + b'"]}',        # whitespace
    b'{"id":5,"invoke": "upload","params":["' + BODY + b'"]}',
    b' {"id":5,"invoke":"upload","params":["' + BODY + b'"]}',
    b'{"id":5,"invoke":"download","params":["' + BODY + b'"]}',       # another method
    b'{"id":5,"invoke":"upload","params":["' + BODY,                  # the end missing
    b'{"id":5,"invoke":"upload","params":["' + BODY + b'"]',
    b'{"id":5,"invoke":"upload","params":["' + BODY + b'"] }',
    b'{"id":5,"invoke":"upload","params":["' + BODY + b'"]}\n',
    b'{"id":5,"invoke":"upload","params":["',
    b'{"id":5,"invoke":"upload","params":["]}',
    b'{"id":5,"invoke":"upload","params":[]}',
    b'{"id":5,"invoke":"upload"}', b'{"id":5', b'{"id":', b"{", b"",
]


def masks_for(payload):
    """zero, random, and one that makes masked bytes look like '"' (the byte the
    payload has most often at offset 0 mod 4 turns into '"', and so on)."""
    rng = np.random.default_rng(len(payload))
    quote = bytes((max(set(payload[j::4]) or {0}, key=payload[j::4].count) ^ 0x22) for j in range(4))
    return (None, bytes(4), bytes(rng.integers(0, 256, 4, dtype=np.uint8)), quote)


def test_upload_request_table(vds_lib):
    for payload, rid, body in ACCEPTED:
        for mask in masks_for(payload):
            sent = payload if mask is None else xor_mask(payload, mask)
            rc, got_id, off, ln, size = chunk.ws_upload_request(sent, mask)
            assert rc == _lib.OK, (payload[:50], mask)
            assert got_id == rid and payload[off:off + ln] == body and ln == len(body)
            want = 0 if len(body) % 4 or not body else len(body) // 4 * 3 - (2 if body.endswith(b"==") else
                                                                              1 if body.endswith(b"=") else 0)
            assert size == want == vds_lib.vds_ec_base64_decoded_size(body, len(body)), (body[-8:], mask)
    for payload in REJECTED:
        for mask in masks_for(payload):
            sent = payload if mask is None else xor_mask(payload, mask)
            assert chunk.ws_upload_request(sent, mask)[0] == _lib.EWS_FORM, (payload[:60], mask)
    # an accepted payload read under the wrong mask is not the fast form
    assert chunk.ws_upload_request(xor_mask(ACCEPTED[0][0], b"\x01\x02\x03\x04"), bytes(4))[0] == _lib.EWS_FORM


def test_upload_request_reads_the_envelope_only(vds_lib):
    """Bytes 48 .. len-6 of the payload do not matter: the body is never walked."""
    payload = bytearray(request(2147483647, BODY))
    want = chunk.ws_upload_request(bytes(payload))
    payload[48:len(payload) - 5] = b"\x00" * (len(payload) - 53)
    assert chunk.ws_upload_request(bytes(payload)) == want


# ------------------------------------------------------- answers' arithmetic
def test_answer_sizes(vds_lib):
    d = bytes(range(32))
    for rid in (0, 7, 2147483647, -1):
        for rs in (2, 2050, 4294967295):
            for n in (0, 1, 2, 63, 64, 65, 1391, 1392, 1393, 1394, 1395):
                json_len = upload_json_len(rid, n, rs)
                hl = 2 if json_len < 126 else 4 if json_len <= 0xFFFF else 10
                assert chunk.ws_upload_answer_size(rid, n, rs) == (hl + json_len, hl), (rid, n, rs)
            # ... and the restatement is the library's own serialiser's length
            assert upload_json_len(rid, 3, rs) == len(chunk.upload_response_json(rid, [d] * 3, d, rs))
    # the 16-bit form's last n and the 64-bit form's first
    sizes = [chunk.ws_upload_answer_size(5, n, 2050) for n in range(1380, 1400)]
    assert {h for _, h in sizes} == {4, 10}
    # download: 21 + d + T behind the header, at the header-form boundaries
    for rid, E, json_len, hl in ((5, 75, 122, 2), (5, 76, 126, 4), (10, 49134, 65535, 4), (10, 49135, 65539, 10),
                                 (5, 0, 22, 2), (-1, 1, 45, 2), (2147483647, 3, 35, 2)):
        digits = len(id_text(rid))
        assert json_len == 21 + digits + (E + 2) // 3 * 4
        assert chunk.ws_download_answer_layout(rid, E) == (hl + json_len, hl, hl + 19 + digits), (rid, E)


def test_error_answer(vds_lib):
    for rid in (0, 7, 2147483647, -1):
        for status in (_lib.EB64_LENGTH, _lib.EB64_PADDING, _lib.EB64_CHAR, _lib.ECORRUPT, _lib.ERESTORE):
            assert chunk.ws_error_answer(rid, status) == error_frame(rid, _lib.strerror(status)), (rid, status)
    assert chunk.ws_error_answer(5, _lib.ECORRUPT) == b'\x81\x26{"id":"5","error":"Data is corrupted"}'
    ln = C.c_size_t(0)
    buf = C.create_string_buffer(64)
    assert vds_lib.vds_ec_ws_error_answer(5, _lib.ECORRUPT, buf, 39, C.byref(ln)) == _lib.EINVAL
    assert ln.value == 40 and buf.raw == bytes(64)


# ------------------------------------------------------- argument validation
LENS = [88, 4, 0, 1024, 8]
SIZES = [66, 1, 0, 767, 4]


def _mdec(lib, lens=LENS, sizes=SIZES, texts=None, outs=None, statuses=DEV, count=None, null=()):
    tp = np.asarray([DEV + (1 << 20) * (i + 1) for i in range(len(lens))] if texts is None else texts, dtype=np.uint64)
    op = np.asarray([DEV + (1 << 20) * (i + 100) for i in range(len(lens))] if outs is None else outs,
                    dtype=np.uint64)
    tl, os_ = np.asarray(lens, dtype=np.uint64), np.asarray(sizes, dtype=np.uint64)
    mk = np.zeros(4 * max(1, len(lens)), dtype=np.uint8)
    return lib.vds_ec_base64_decode_masked_batch_device(
        len(lens) if count is None else count, None if "texts" in null else tp.ctypes.data_as(_lib.vpp),
        None if "lens" in null else tl.ctypes.data_as(_lib.u64p), None if "masks" in null else mk.ctypes.data,
        None if "outs" in null else op.ctypes.data_as(_lib.vpp),
        None if "sizes" in null else os_.ctypes.data_as(_lib.u64p), statuses, None)


def _ans(lib, count=5, n=N, null=(), outs=None):
    ids = np.arange(count, dtype=np.int32)
    rs = np.full(count, 2050, dtype=np.uint32)
    op = np.asarray([DEV + 4096 * i for i in range(1, count + 1)] if outs is None else outs, dtype=np.uint64)
    return lib.vds_ec_ws_upload_answer_batch_device(
        count, None if "ids" in null else ids.ctypes.data_as(I32P), n, None if "rd" in null else DEV + (1 << 30),
        None if "dd" in null else DEV + (2 << 30), None if "rs" in null else rs.ctypes.data_as(U32P),
        None if "outs" in null else op.ctypes.data_as(_lib.vpp), None)


class WsUpload:
    """Real host buffers for one call of vds_ec_ws_upload16_host_batch."""

    def __init__(self, frames, k=K, n=N):
        self.k, self.n, self.frames, self.count = k, n, frames, len(frames)
        self.lens = np.asarray([len(f) for f in frames] or [0], dtype=np.uint64)
        self.fp = (C.c_char_p * max(1, self.count))(*frames)
        self.outs = [np.zeros(4096, dtype=np.uint8) for _ in range(self.count * n)]
        self.op = (C.c_void_p * max(1, self.count * n))(*[o.ctypes.data for o in self.outs])
        self.rd = np.zeros(max(1, 32 * self.count * n), dtype=np.uint8)
        self.st = np.zeros(max(1, self.count), dtype=np.int32)
        self.ans = np.zeros(max(1, self.count) * 4096, dtype=np.uint8)
        self.ao = np.zeros(max(1, self.count), dtype=np.uint64)
        self.al = np.zeros(max(1, self.count), dtype=np.uint64)
        self.failed = C.c_uint32(99)

    def call(self, lib, count=None, k=None, n=None, null=(), fp=None, op=None, ans_bytes=None):
        return lib.vds_ec_ws_upload16_host_batch(
            self.k if k is None else k, self.n if n is None else n, self.count if count is None else count,
            None if "frames" in null else C.cast(self.fp if fp is None else fp, _lib.vpp),
            None if "lens" in null else self.lens.ctypes.data_as(_lib.u64p),
            None if "outs" in null else (self.op if op is None else op),
            None if "rd" in null else self.rd.ctypes.data, None, None,
            None if "answers" in null else self.ans.ctypes.data, self.ans.size if ans_bytes is None else ans_bytes,
            None if "offs" in null else self.ao.ctypes.data_as(_lib.u64p),
            None if "alens" in null else self.al.ctypes.data_as(_lib.u64p),
            None if "statuses" in null else self.st.ctypes.data_as(I32P), C.byref(self.failed))


def upload_frame(rid, body_bytes, mask=b"\x31\x41\x59\x26"):
    payload = request(rid, base64.b64encode(body_bytes))
    return frame_header(len(payload), mask=mask) + (xor_mask(payload, mask) if mask is not None else payload)


def test_device_entry_points_invalid_arguments(vds_lib):
    for null in ("texts", "lens", "outs", "sizes", "masks"):
        assert _mdec(vds_lib, null=(null,)) == _lib.EINVAL, null
    assert _mdec(vds_lib, statuses=None) == _lib.EINVAL
    assert _mdec(vds_lib, count=1 << 30) == _lib.EINVAL
    assert _mdec(vds_lib, lens=[8, 88], sizes=[6, 67]) == _lib.EINVAL
    assert _mdec(vds_lib, lens=[1 << 32], sizes=[(1 << 30) * 3]) == _lib.EINVAL
    assert _mdec(vds_lib, texts=[0, 1, 2, 3, 4]) == _lib.EINVAL
    for null in ("ids", "rd", "dd", "rs", "outs"):
        assert _ans(vds_lib, null=(null,)) == _lib.EINVAL, null
    assert _ans(vds_lib, n=65537) == _lib.EINVAL
    assert _ans(vds_lib, count=5, outs=[DEV, DEV + 4096, 0, DEV + 8192, DEV + 12288]) == _lib.EINVAL


def test_ws_upload_invalid_arguments(vds_lib):
    body = bytes(range(200))
    u = WsUpload([upload_frame(i, body[:s]) for i, s in enumerate((0, 1, 2, 3, 100, 200))])
    for null in ("frames", "lens", "outs", "rd", "statuses", "answers", "offs", "alens"):
        assert u.call(vds_lib, null=(null,)) == _lib.EINVAL, null
    assert u.call(vds_lib, k=0) == _lib.EINVAL
    assert u.call(vds_lib, n=65537) == _lib.EINVAL
    assert u.call(vds_lib, count=1 << 30) == _lib.EINVAL
    assert u.call(vds_lib, count=(1 << 32) // (N + 64) + 1) == _lib.EINVAL
    fp = (C.c_char_p * u.count)(*(u.frames[:4] + [None] + u.frames[5:]))
    assert u.call(vds_lib, fp=fp) == _lib.EINVAL
    op = (C.c_void_p * (u.count * N))(*[o.ctypes.data for o in u.outs])
    op[3 * N + 7] = None
    assert u.call(vds_lib, op=op) == _lib.EINVAL
    # a slab too small for the answers' slots
    need = sum(chunk.ws_upload_answer_size(i, N, chunk.replica_size(K, s))[0]
               for i, s in enumerate((0, 1, 2, 3, 100, 200)))
    assert u.call(vds_lib, ans_bytes=need - 1) == _lib.EINVAL
    assert (u.st == 0).all() and not u.rd.any() and not u.ans.any(), "a rejected call wrote something"


def test_ws_download_invalid_arguments(vds_lib):
    k, cs = 4, 10
    chunks = [np.zeros(cs, dtype=np.uint8) for _ in range(2 * k)]
    cp = (C.c_void_p * (2 * k))(*[c.ctypes.data for c in chunks])
    ids = np.asarray([5, 6], dtype=np.int32)
    nodes = np.asarray(list(range(k)) * 2, dtype=np.uint16)
    csz = np.asarray([cs, cs], dtype=np.uint64)
    names = np.zeros(2 * k * 32, dtype=np.uint8)
    slab = np.zeros(4096, dtype=np.uint8)
    fo, fl = np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    st, sv = np.zeros(2, dtype=np.int32), np.zeros(2 * k, dtype=np.uint8)

    def call(null=(), count=2, kk=k, slab_bytes=slab.size, nd=nodes, sizes=csz):
        return vds_lib.vds_ec_ws_download16_host_batch(
            kk, count, None if "ids" in null else ids.ctypes.data_as(I32P),
            None if "nodes" in null else nd.ctypes.data_as(_lib.u16p), None if "chunks" in null else cp,
            None if "sizes" in null else sizes.ctypes.data_as(_lib.u64p),
            None if "names" in null else names.ctypes.data, None, None, None if "slab" in null else slab.ctypes.data,
            slab_bytes, None if "offs" in null else fo.ctypes.data_as(_lib.u64p),
            None if "lens" in null else fl.ctypes.data_as(_lib.u64p),
            None if "statuses" in null else st.ctypes.data_as(I32P), None if "sv" in null else sv.ctypes.data, None)

    for null in ("ids", "nodes", "chunks", "sizes", "names", "slab", "offs", "lens", "statuses", "sv"):
        assert call(null=(null,)) == _lib.EINVAL, null
    assert call(kk=0) == _lib.EINVAL
    assert call(count=1 << 30) == _lib.EINVAL
    assert call(sizes=np.asarray([cs, 1], dtype=np.uint64)) == _lib.EINVAL
    assert call(sizes=np.asarray([cs, 9], dtype=np.uint64)) == _lib.EINVAL
    assert call(nd=np.asarray([0, 1, 2, 3, 0, 1, 1, 3], dtype=np.uint16)) == _lib.ESINGULAR
    assert call(slab_bytes=60) == _lib.EINVAL  # two slots need more
    assert not slab.any() and not st.any()


def test_empty_batches_are_ok(vds_lib):
    assert vds_lib.vds_ec_base64_decode_masked_batch_device(0, None, None, None, None, None, None, None) == _lib.OK
    assert vds_lib.vds_ec_ws_upload_answer_batch_device(0, None, N, None, None, None, None, None) == _lib.OK
    failed = C.c_uint32(7)
    assert vds_lib.vds_ec_ws_upload16_host_batch(K, N, 0, None, None, None, None, None, None, None, 0, None, None,
                                                 None, C.byref(failed)) == _lib.OK
    assert failed.value == 0
    failed = C.c_uint32(7)
    assert vds_lib.vds_ec_ws_download16_host_batch(K, 0, None, None, None, None, None, None, None, None, 0, None,
                                                   None, None, None, C.byref(failed)) == _lib.OK
    assert failed.value == 0


def test_frames_without_device_work_need_no_device(vds_lib):
    """A ping, another opcode, a short frame and a payload that is not the fast
    form are answered from the host alone: their statuses, no answer."""
    slow = b'{"id": 5,"invoke":"upload","params":["QUJD"]}'
    whole = upload_frame(5, b"abc")
    u = WsUpload([frame_header(4, opcode=9, mask=b"abcd") + b"ping", frame_header(2, opcode=8) + b"\x03\xe8",
                  frame_header(len(slow)) + slow, whole[:-1], whole[:3], b"\x81"])
    assert u.call(vds_lib) == _lib.OK
    assert list(u.st) == [_lib.EWS_PING, _lib.EWS_FRAME, _lib.EWS_FORM, _lib.EWS_SHORT, _lib.EWS_SHORT,
                          _lib.EWS_SHORT]
    assert u.failed.value == 6 and not u.al.any() and not u.ans.any() and not u.rd.any()
    assert not any(o.any() for o in u.outs)


def test_valid_calls_need_a_device(vds_lib):
    """Validation comes first, the device check second (where a GPU is present
    this test has nothing to assert and the GPU suite covers the calls)."""
    if not _no_device(vds_lib):
        return
    assert _mdec(vds_lib) == _lib.ENODEV
    assert _ans(vds_lib) == _lib.ENODEV
    body = bytes(range(200))
    u = WsUpload([upload_frame(i, body[:s]) for i, s in enumerate((0, 1, 100))] +
                 [frame_header(0, opcode=9), upload_frame(9, b"x")[:-1]])
    assert u.call(vds_lib) == _lib.ENODEV
    assert (u.st == 0).all() and not u.ans.any(), "written without a device"


def test_header_entry_points_are_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "vds_ec.h")).read(), flags=re.S)
    names = re.findall(r"\b(vds_ec_ws_\w+|vds_ec_base64_decode_masked_batch_device)\s*\(", text)
    assert len(set(names)) == 10, names
    for name in names:
        assert name in _lib.SIGNATURES, name
    for code in ("EWS_SHORT", "EWS_FRAME", "EWS_FORM", "EWS_PING"):
        value = int(re.search(r"#define VDS_EC_%s \((-\d+)\)" % code, text).group(1))
        assert getattr(_lib, code) == value
        assert _lib.strerror(value) != _lib.strerror(-999), code
