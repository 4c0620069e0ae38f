"""The websocket layer on the device (base64.hip's masked decode instance and
k_ws_upload_answer_batch) and the two host forms built on it
(vds_ec_ws_upload16_host_batch, vds_ec_ws_download16_host_batch).

Expected values come from Python restatements (struct, plain string building,
XOR with numpy) and from the library's existing host functions on the UNMASKED
inputs: vds_ec_base64_decode, vds_ec_upload_response_json,
vds_ec_upload16_host_batch, vds_ec_download16_host_batch.  Every device output
is compared whole and between guard bytes; statuses start as a sentinel."""
import base64
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

from test_ws_cpu import error_frame, frame_header, request, xor_mask

pytestmark = pytest.mark.gpu

FILL = 0x5A
SENTINEL = 0x5A5A5A5A
GUARD = 16
EINVAL, EB64_LENGTH, EB64_PADDING, EB64_CHAR, ECORRUPT = -1, -7, -8, -9, -10


def _host_decode(lib, t: bytes):
    """(status, bytes) of vds_ec_base64_decode: the checker."""
    size = lib.vds_ec_base64_decoded_size(t, len(t))
    out = np.zeros(max(size, 1), dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib.vds_ec_base64_decode(t, len(t), out.ctypes.data, C.byref(n))
    return rc, out[:size]


def _place(lens, mods, align, lead):
    """Offsets of pieces of `lens` bytes, piece i at mods[i] modulo `align`, at least `lead` bytes apart."""
    offs, pos = [], 0
    for ln, m in zip(lens, mods):
        pos = (pos + align - 1) // align * align + align * ((lead + align - 1) // align) + m
        offs.append(pos)
        pos += ln
    return offs, pos + lead + align


def _text_mask(frame_mask: bytes, rot: int) -> bytes:
    """What the caller passes for a body at payload offset rot mod 4."""
    return bytes(frame_mask[(rot + j) & 3] for j in range(4))


def _run_masked(torch, lib, texts, masks, text_mods, out_mods, declared=None, also_unmasked=False):
    """One masked decode launch: text i (unmasked: texts[i]) lies on the device
    under masks[i] at text_mods[i] mod 16, foreign bytes in the gaps, its output
    at out_mods[i] mod 4 between guard bytes.  Statuses and outputs against the
    host decode of the UNMASKED text; declared[i] replaces the size passed (the
    message must come back EINVAL, its output untouched).  Returns (statuses,
    outputs)."""
    from vds_amd import chunk
    count = len(texts)
    sizes = [lib.vds_ec_base64_decoded_size(t, len(t)) for t in texts]
    passed = list(sizes)
    for i, s in (declared or {}).items():
        passed[i] = s
    sent = [xor_mask(t, m) for t, m in zip(texts, masks)]
    t_offs, t_total = _place([len(t) for t in texts], text_mods, 16, 16)
    buf = np.empty(t_total, dtype=np.uint8)
    buf[0::2], buf[1::2] = ord("="), ord("A")
    for s, off in zip(sent, t_offs):
        buf[off:off + len(s)] = np.frombuffer(s, dtype=np.uint8)
    d_text = torch.from_numpy(buf).cuda()
    assert d_text.data_ptr() % 16 == 0
    o_offs, o_total = _place(passed, out_mods, 4, GUARD)
    want = np.full(o_total, FILL, dtype=np.uint8)
    must = np.ones(o_total, dtype=bool)
    want_st = np.zeros(count, dtype=np.int32)
    for i, t in enumerate(texts):
        if declared and i in declared:
            want_st[i] = EINVAL
            continue
        rc, ref = _host_decode(lib, t)
        want_st[i] = rc
        if rc == 0:
            want[o_offs[i]:o_offs[i] + sizes[i]] = ref
        else:
            must[o_offs[i]:o_offs[i] + sizes[i]] = False
    tptrs = [d_text.data_ptr() + off for off in t_offs]
    tlens = [len(t) for t in texts]

    def launch(masked):
        d_out = torch.full((o_total,), FILL, dtype=torch.uint8, device="cuda")
        assert d_out.data_ptr() % 4 == 0
        d_st = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
        optrs = [d_out.data_ptr() + o for o in o_offs]
        if masked:
            chunk.base64_decode_masked_batch_device(tptrs, tlens, b"".join(masks), optrs, passed, d_st)
        else:
            chunk.base64_decode_batch_device(tptrs, tlens, optrs, passed, d_st)
        torch.cuda.synchronize()
        return d_st.cpu().numpy(), d_out.cpu().numpy()

    st, got = launch(True)
    bad = np.flatnonzero(st != want_st)
    assert bad.size == 0, ("status", int(bad[0]), texts[bad[0]][:64], masks[bad[0]], int(st[bad[0]]),
                           int(want_st[bad[0]]))
    wrong = np.flatnonzero((got != want) & must)
    if wrong.size:
        at = int(wrong[0])
        i = int(np.searchsorted(np.asarray(o_offs), at, side="right")) - 1
        raise AssertionError(("bytes", at, "message", i, "offset in it", at - o_offs[max(i, 0)], len(texts[i]),
                              masks[i], text_mods[i], out_mods[i], int(got[at]), int(want[at])))
    if also_unmasked:  # (every mask is zero: the unmasked call on the same device bytes)
        st0, got0 = launch(False)
        assert np.array_equal(st0, st) and np.array_equal(got0, got)
    return st, [got[o:o + s] for o, s in zip(o_offs, passed)]


def _most_frequent(t: bytes) -> int:
    return max(set(t), key=t.count) if t else ord("A")


LENGTHS = (0, 4, 8, 12, 16, 20, 60, 64, 68, 1020, 1024, 1028, 2044, 2048, 2052)
TEXT_MOD16 = (0, 1, 2, 3, 4, 7, 8, 15)


def test_masked_decode_every_length_and_alignment(gpu, vds_lib):
    import torch
    rng = random.Random(11)
    for kind in ("zero", "random", "equals"):
        texts, masks, tmods, omods = [], [], [], []
        for ln in LENGTHS:
            for tm in TEXT_MOD16:
                for om in range(4):
                    for rot in range(4):
                        p = (tm + om + rot) % 3 if ln else 0
                        t = base64.b64encode(rng.randbytes(ln // 4 * 3 - p))
                        assert len(t) == ln
                        if kind == "zero":
                            fm = bytes(4)
                        elif kind == "random":
                            fm = rng.randbytes(4)
                        else:  # a kernel that classified before unmasking would see '=' everywhere
                            fm = bytes([_most_frequent(t) ^ ord("=")] * 4)
                        texts.append(t)
                        masks.append(_text_mask(fm, rot))
                        tmods.append(tm)
                        omods.append(om)
        st, outs = _run_masked(torch, vds_lib, texts, masks, tmods, omods, also_unmasked=kind == "zero")
        assert not st.any()
        for t, o in zip(texts, outs):
            assert o.tobytes() == base64.b64decode(t)


def test_first_event_under_a_mask(gpu, vds_lib):
    import torch
    rng = random.Random(12)
    span = 2052
    forms = [base64.b64encode(rng.randbytes(span // 4 * 3 - p)) for p in (0, 1, 2)]
    assert [len(f) for f in forms] == [span] * 3
    spots = (0, 1, 15, 16, 17, 1023, 1024, 1025, span - 3, span - 2, span - 1)
    texts, masks, tmods, omods = [], [], [], []
    for f in forms:  # '=' without (p = 0: an error) and with one or two trailing '='
        for pos in spots:
            for ch in (b"*", b"=", b'"', b"\\"):
                t = f[:pos] + ch + f[pos + 1:]
                for tm in (1, 3):
                    for fm in (rng.randbytes(4), bytes([_most_frequent(t) ^ ord("=")] * 4),
                               bytes(c ^ ord("=") for c in t[max(pos - 3, 0):max(pos - 3, 0) + 4])):
                        texts.append(t)
                        masks.append(_text_mask(fm, pos & 3))
                        tmods.append(tm + 4 * (len(texts) % 4))
                        omods.append(len(texts) % 4)
    st, _ = _run_masked(torch, vds_lib, texts, masks, tmods, omods)
    assert set(st.tolist()) == {0, EB64_PADDING, EB64_CHAR}
    by_text = {t: int(s) for t, s in zip(texts, st)}
    assert by_text[forms[0][:16] + b"=" + forms[0][17:]] == EB64_PADDING
    assert by_text[forms[1][:1024] + b"=" + forms[1][1025:]] == 0  # two accumulator bytes, then zeros
    assert by_text[forms[2][:1] + b"=" + forms[2][2:]] == 0
    assert by_text[forms[2][:1025] + b'"' + forms[2][1026:]] == EB64_CHAR


def test_declared_size_mismatch_under_a_mask(gpu, vds_lib):
    """The '=' among the last two characters are counted on the UNMASKED text:
    a mask that turns them into '=' while masked (or hides real ones) must not
    move the verdict."""
    import torch
    rng = random.Random(13)
    texts, masks, tmods, omods, declared = [], [], [], [], {}
    for ln in (4, 8, 1024, 2052):
        for p in (0, 1, 2):
            t = base64.b64encode(rng.randbytes(ln // 4 * 3 - p))
            a, b = (ln - 2) & 3, (ln - 1) & 3
            looks = bytearray(rng.randbytes(4))
            looks[a], looks[b] = t[-2] ^ ord("="), t[-1] ^ ord("=")   # masked, the last two are "=="
            hides = bytearray(rng.randbytes(4))
            hides[a], hides[b] = 0x11, 0x13                            # masked, neither is '='
            for mk in (bytes(looks), bytes(hides)):
                for q in (0, 1, 2):
                    if q != p:
                        declared[len(texts)] = ln // 4 * 3 - q
                    texts.append(t)
                    masks.append(mk)
                    tmods.append((len(texts) * 5) % 16)
                    omods.append(len(texts) % 4)
    st, outs = _run_masked(torch, vds_lib, texts, masks, tmods, omods, declared=declared)
    for i, t in enumerate(texts):
        if i in declared:
            assert st[i] == EINVAL and (outs[i] == FILL).all()
        else:
            assert st[i] == 0 and outs[i].tobytes() == base64.b64decode(t)


def _upload_json(lib, rid, digests: bytes, n, data_digest: bytes, rs):
    ln = C.c_size_t(0)
    assert lib.vds_ec_upload_response_json(rid, digests, n, data_digest, rs, None, 0, C.byref(ln)) == 0
    out = C.create_string_buffer(ln.value + 1)
    assert lib.vds_ec_upload_response_json(rid, digests, n, data_digest, rs, out, ln.value + 1, C.byref(ln)) == 0
    return out.raw[:ln.value]


def test_upload_answer_kernel(gpu, vds_lib):
    import torch
    from vds_amd import chunk
    count = 130  # more than one wave and workgroup
    big = next(n for n in range(1, 3000) if chunk.ws_upload_answer_size(0, n, 2)[0] > 65535 + 4)
    assert 1300 < big < 1500
    ids = [(0, 7, 2147483647, -1)[o % 4] for o in range(count)]
    rsz = [(2, 2050, 4294967295)[(o // 4) % 3] for o in range(count)]
    rng = np.random.default_rng(14)
    for n in (1, 2, 63, 64, 65, big):
        rd = rng.integers(0, 256, 32 * n * count, dtype=np.uint8)
        dd = rng.integers(0, 256, 32 * count, dtype=np.uint8)
        lead = n % 4  # (the digests at every address mod 4 over the calls)
        d_rd = torch.from_numpy(np.concatenate([np.zeros(lead, dtype=np.uint8), rd])).cuda()
        d_dd = torch.from_numpy(np.concatenate([np.zeros(3 - lead, dtype=np.uint8), dd])).cuda()
        want_frames = []
        for o in range(count):
            js = _upload_json(vds_lib, ids[o], rd[32 * n * o:32 * n * (o + 1)].tobytes(), n,
                              dd[32 * o:32 * o + 32].tobytes(), rsz[o])
            want_frames.append(chunk.ws_frame_header(len(js)) + js)
            assert len(want_frames[-1]) == chunk.ws_upload_answer_size(ids[o], n, rsz[o])[0]
            assert len(want_frames[-1]) - len(js) == (10 if n == big else 4)
        offs, total = _place([len(f) for f in want_frames], [(o // 2) % 4 for o in range(count)], 4, GUARD)
        want = np.full(total, FILL, dtype=np.uint8)
        for f, off in zip(want_frames, offs):
            want[off:off + len(f)] = np.frombuffer(f, dtype=np.uint8)
        d_out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        assert d_out.data_ptr() % 4 == 0
        chunk.ws_upload_answer_batch_device(ids, n, d_rd.data_ptr() + lead, d_dd.data_ptr() + 3 - lead, rsz,
                                            [d_out.data_ptr() + o for o in offs])
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        wrong = np.flatnonzero(got != want)
        if wrong.size:
            at = int(wrong[0])
            o = int(np.searchsorted(np.asarray(offs), at, side="right")) - 1
            raise AssertionError(("n", n, "byte", at, "message", o, "offset in it", at - offs[max(o, 0)],
                                  "of", len(want_frames[o]), int(got[at]), int(want[at])))


SLOW = b'{"id": 5,"invoke":"upload","params":["QUJDRA=="]}'  # valid JSON, not the fast form


def _ws_upload_cases(rng):
    """(frames, per frame: None for a member without device work, else (id, body text))."""
    frames, members = [], []

    def add(rid, text, mask, opcode=1):
        payload = request(rid, text)
        frames.append(frame_header(len(payload), opcode=opcode, mask=mask) +
                      (xor_mask(payload, mask) if mask is not None else payload))
        members.append((rid, text))
        return frames[-1]

    rid = 0
    for rep in range(3):
        for size in (0, 1, 2, 3, 57, 100):
            f = add(rid, base64.b64encode(rng.randbytes(size)), rng.randbytes(4))
            assert (f[1] & 0x7F < 126) == (size <= 57)  # 2-byte headers (the 100-byte body's payload: 177 bytes)
            rid = (7, 2147483647, 0, 31337)[len(frames) % 4]
    sizes = [48000] * 4 + [57 * 1024] * 2 + [65536] * 8
    for i, size in enumerate(sizes):
        mask = None if i in (1, 9) else rng.randbytes(4)  # two unmasked
        f = add((5, 2147483647, 31337)[i % 3], base64.b64encode(rng.randbytes(size)), mask, opcode=1 + i % 2)
        assert f[1] & 0x7F == (126 if size == 48000 else 127)
    # one of each, mixed in
    good = base64.b64encode(rng.randbytes(300))
    add(41, good[:100] + b'"' + good[101:], rng.randbytes(4))        # a stray '"' in the body
    add(42, good[:-2], rng.randbytes(4))                             # a length that is no multiple of 4
    add(43, good[:50] + b"=" + good[51:], rng.randbytes(4))          # wrong padding
    for at, fr in ((3, frame_header(4, opcode=9, mask=b"abcd") + b"ping"),
                   (17, frame_header(2, opcode=8, mask=b"abcd") + b"\x03\xe8"),
                   (29, frame_header(len(SLOW), mask=bytes(4)) + SLOW)):
        frames.insert(at, fr)
        members.insert(at, None)
    return frames, members


@pytest.mark.parametrize("k,n", [(32, 64), (16, 20)])
def test_ws_upload_host_batch(gpu, vds_lib, k, n):
    from vds_amd import _lib, chunk
    frames, members = _ws_upload_cases(random.Random(15))
    count = len(frames)
    assert 38 <= count <= 44
    work = [o for o in range(count) if members[o] is not None]
    # the existing batched upload on the unmasked bodies
    ref = chunk.upload_batch([members[o][0] for o in work], [members[o][1] for o in work], k=k, n=n)
    ref = dict(zip(work, ref))
    assert sum(isinstance(r, str) for r in ref.values()) == 3
    Ls = [chunk.replica_size(k, len(members[o][1]) // 4 * 3) if members[o] else 8 for o in range(count)]
    outs = [np.full(GUARD + L + GUARD, FILL, dtype=np.uint8) for L in Ls for _ in range(n)]
    op = (C.c_void_p * (count * n))(*[b.ctypes.data + GUARD for b in outs])
    rd = np.full(32 * count * n + GUARD, FILL, dtype=np.uint8)
    dd = np.full(32 * count + GUARD, FILL, dtype=np.uint8)
    rs = np.full(count + 1, SENTINEL, dtype=np.uint32)
    st = np.full(count + 1, SENTINEL, dtype=np.int32)
    # the answers as the restatement lays them out: slots back to back
    want_ans, slots = [], []
    for o in range(count):
        if members[o] is None:
            want_ans.append(b"")
            slots.append(0)
            continue
        rid, text = members[o]
        r = ref[o]
        size = vds_lib.vds_ec_base64_decoded_size(text, len(text))
        ok_len = chunk.ws_upload_answer_size(rid, n, chunk.replica_size(k, size))[0]
        slots.append(max(ok_len, len(error_frame(rid, _lib.strerror(EB64_CHAR)))))
        if isinstance(r, str):
            want_ans.append(error_frame(rid, r))
        else:
            js = r["json"].encode()
            want_ans.append(frame_header(len(js)) + js)
            assert len(want_ans[-1]) == ok_len
    total = sum(slots)
    ans = np.full(total + GUARD, FILL, dtype=np.uint8)
    ao = np.full(count, 1 << 60, dtype=np.uint64)
    al = np.full(count, 1 << 60, dtype=np.uint64)
    fl = np.asarray([len(f) for f in frames], dtype=np.uint64)
    fp = (C.c_char_p * count)(*frames)
    failed = C.c_uint32(12345)
    _lib.check(vds_lib.vds_ec_ws_upload16_host_batch(
        k, n, count, C.cast(fp, _lib.vpp), fl.ctypes.data_as(_lib.u64p), op, rd.ctypes.data, dd.ctypes.data,
        rs.ctypes.data_as(_lib.u32p), ans.ctypes.data, total, ao.ctypes.data_as(_lib.u64p),
        al.ctypes.data_as(_lib.u64p), st.ctypes.data_as(_lib.i32p), C.byref(failed)), "ws_upload16_host_batch")
    assert st[count] == SENTINEL and rs[count] == SENTINEL
    assert (rd[32 * count * n:] == FILL).all() and (dd[32 * count:] == FILL).all() and (ans[total:] == FILL).all()
    want_st = {3: _lib.EWS_PING, 17: _lib.EWS_FRAME, 29: _lib.EWS_FORM}
    pos = 0
    for o in range(count):
        mine = outs[o * n:(o + 1) * n]
        assert ao[o] == pos, o
        slot = ans[pos:pos + slots[o]]
        pos += slots[o]
        r = ref.get(o)
        if r is None or isinstance(r, str):
            # no output written: replicas, names, hash, replica size
            assert all((b == FILL).all() for b in mine), o
            assert (rd[32 * o * n:32 * (o + 1) * n] == FILL).all() and (dd[32 * o:32 * o + 32] == FILL).all(), o
            assert rs[o] == SENTINEL, o
            if r is None:
                assert st[o] == want_st[o] and al[o] == 0, (o, st[o])
                continue
            assert _lib.strerror(int(st[o])) == r, (o, st[o], r)
        else:
            assert st[o] == 0, (o, st[o])
            L = len(r["replicas"][0])
            assert rs[o] == L
            for b, want in zip(mine, r["replicas"]):
                assert (b[:GUARD] == FILL).all() and (b[GUARD + L:] == FILL).all(), (o, "guard bytes written")
                assert np.array_equal(b[GUARD:GUARD + L], want[:L]), o
            assert rd[32 * o * n:32 * (o + 1) * n].tobytes() == b"".join(r["replica_digests"]), o
            assert dd[32 * o:32 * o + 32].tobytes() == r["data_hash"], o
        assert al[o] == len(want_ans[o]), (o, al[o], len(want_ans[o]))
        assert slot[:al[o]].tobytes() == want_ans[o], (o, slot[:64].tobytes(), want_ans[o][:64])
        assert (slot[al[o]:] == FILL).all(), (o, "answer slot written behind the answer")
    assert pos == total
    assert failed.value == 6
    kinds = {int(s) for s in st[:count]}
    assert kinds == {0, EB64_CHAR, EB64_LENGTH, EB64_PADDING, _lib.EWS_PING, _lib.EWS_FRAME, _lib.EWS_FORM}


_DL = {}


def _download_objects(k):
    """Per object (id, E, flipped?) at the answers' header-form boundaries; the
    replicas from the library's own batched save_temp, computed once."""
    if k in _DL:
        return _DL[k]
    from vds_amd import chunk
    spec = [(5, 75), (5, 76), (10, 49134), (10, 49135), (2147483647, 0), (-1, 30001), (7, 1000)]
    rng = random.Random(16)
    bodies = [rng.randbytes(E) for _, E in spec]
    n = k + 8
    saved = chunk.save_temp_batch(k, n, bodies)
    objs = []
    for (rid, E), body, (reps, names, _, L) in zip(spec, bodies, saved):
        surv = [np.ascontiguousarray(np.asarray(reps[r][:L], dtype=np.uint8)) for r in range(8, n)]
        wit = np.asarray(reps[0][:L], dtype=np.uint8)
        objs.append({"id": rid, "E": E, "body": body, "nodes": list(range(8, n)), "surv": surv,
                     "names": [hashlib.sha256(c.tobytes()).digest() for c in surv], "wid": 0,
                     "wname": hashlib.sha256(wit.tobytes()).digest()})
    flipped = 5
    bad = objs[flipped]["surv"][11].copy()
    bad[77] ^= 0x10
    objs[flipped]["surv"][11] = bad
    _DL[k] = (objs, flipped)
    return _DL[k]


@pytest.mark.parametrize("mode", ["survivor", "witness"])
def test_ws_download_host_batch(gpu, vds_lib, mode):
    from vds_amd import _lib, chunk
    k = 32
    objs, flipped = _download_objects(k)
    count = len(objs)
    wit = mode == "witness"
    # the existing download loop, then the restatement round its texts
    ref = chunk.download_batch(k, [dict(zip(ob["nodes"], ob["surv"])) for ob in objs], [ob["names"] for ob in objs],
                               [(ob["wid"], ob["wname"]) for ob in objs] if wit else None)
    want, slots = [], []
    for o, (ob, (text, status, _)) in enumerate(zip(objs, ref)):
        rid, E = ob["id"], ob["E"]
        assert (status != 0) == (o == flipped)
        T = (E + 2) // 3 * 4
        digits = len(str(rid % (1 << 64)))
        ok = frame_header(21 + digits + T) + ('{"id":"%d","result":"' % (rid % (1 << 64))).encode() + \
            base64.b64encode(ob["body"]) + b'"}'
        if E in (75, 76, 49134, 49135):
            assert len(ok) - (21 + digits + T) == {75: 2, 76: 4, 49134: 4, 49135: 10}[E]
        if status == 0:
            assert text.encode() == base64.b64encode(ob["body"])
            want.append(ok)
        else:
            assert status == ECORRUPT
            want.append(error_frame(rid, "Data is corrupted"))
        slots.append(max(len(ok), len(error_frame(rid, _lib.strerror(_lib.ERESTORE)))))
    assert len(want[0]) == 124 and len(want[1]) == 130 and len(want[2]) == 65539 and len(want[3]) == 65549
    total = sum(slots)
    slab = np.full(GUARD + total + GUARD, FILL, dtype=np.uint8)
    nd = np.asarray([ob["nodes"] for ob in objs], dtype=np.uint16).reshape(-1)
    cs = np.asarray([ob["surv"][0].size for ob in objs], dtype=np.uint64)
    cp = (C.c_void_p * (count * k))(*[c.ctypes.data for ob in objs for c in ob["surv"]])
    sn = np.frombuffer(b"".join(x for ob in objs for x in ob["names"]), dtype=np.uint8).copy()
    wi = np.asarray([ob["wid"] for ob in objs], dtype=np.uint16)
    wn = np.frombuffer(b"".join(ob["wname"] for ob in objs), dtype=np.uint8).copy()
    ids = np.asarray([ob["id"] for ob in objs], dtype=np.int32)
    fo = np.full(count, 1 << 60, dtype=np.uint64)
    fl = np.full(count, 1 << 60, dtype=np.uint64)
    st = np.full(count, SENTINEL, dtype=np.int32)
    sv = np.full(count * k + 8, FILL, dtype=np.uint8)
    failed = C.c_uint32(12345)
    _lib.check(vds_lib.vds_ec_ws_download16_host_batch(
        k, count, ids.ctypes.data_as(_lib.i32p), nd.ctypes.data_as(_lib.u16p), cp, cs.ctypes.data_as(_lib.u64p),
        sn.ctypes.data, wi.ctypes.data_as(_lib.u16p) if wit else None, wn.ctypes.data if wit else None,
        slab.ctypes.data + GUARD, total, fo.ctypes.data_as(_lib.u64p), fl.ctypes.data_as(_lib.u64p),
        st.ctypes.data_as(_lib.i32p), sv.ctypes.data, C.byref(failed)), "ws_download16_host_batch")
    assert (slab[:GUARD] == FILL).all() and (slab[GUARD + total:] == FILL).all(), "guard bytes written"
    assert (sv[count * k:] == FILL).all() and failed.value == 1
    pos = 0
    for o in range(count):
        assert fo[o] == pos and fl[o] == len(want[o]), (o, fo[o], fl[o], len(want[o]))
        slot = slab[GUARD + pos:GUARD + pos + slots[o]]
        assert slot[:fl[o]].tobytes() == want[o], (o, slot[:48].tobytes(), want[o][:48])
        # behind the frame the slot keeps its guard bytes: a corrupt object's text region above all
        assert (slot[fl[o]:] == FILL).all(), o
        assert st[o] == ref[o][1] and sv[o * k:(o + 1) * k].tolist() == ref[o][2], o
        pos += slots[o]
    assert slots[flipped] - int(fl[flipped]) > 39000  # (the text it never got: 40,004 characters)
