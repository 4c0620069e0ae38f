"""The download loop for a ragged batch in one call, checked
(vds_ec_download16_batch_device / _host_batch: the name check over the
survivors or over one regenerated witness, the batched restore, the gated
base64 encode; websocket_api.cpp:191-210 -> restore_async,
dht_network_client.cpp:851-901 -> websocket_api.cpp:772-782) and the gated
encode alone.  Replicas and objects from the oracle (chunk.h:245-281,
chunk.h:402-444), texts against Python's base64.b64encode, names from hashlib.
Bit-exact; an object that fails its check must not become text."""
import base64
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle_ctypes as O

SEED = 0x7664730000000000
pytestmark = pytest.mark.gpu
GUARD = 61      # guard bytes either side (odd: what lies between them is unaligned)
FILL = 0x5A     # sentinel of every output buffer
ST_FILL = 0x5A5A5A5A
SHAPES = [(16, 20), (32, 64), (3, 5)]
MODES = ["survivor", "witness"]
_CACHE = {}


def _survivors(rng, k, n, i):
    """The survivor ids of object i and a witness (a lost replica's id).
    (16,20): ids below k + k/4, the syndrome route, and the last object with
    an id >= 256, one launch of its own; (32,64): even objects lose so many of
    the first replicas that the survivors reach ids >= 40 (the
    runtime-coefficient route), odd ones stay below 40; (3,5): the generic
    route.  Odd objects hold their survivors in permuted order."""
    if (k, n) == (32, 64) and i % 2 == 0:
        gone = set(rng.choice(40, int(rng.integers(9, 12)), replace=False).tolist())
        nd = [r for r in range(n) if r not in gone][:k]
        assert max(nd) >= 40
    else:
        pool = k + k // 4 if k >= 4 else n
        gone = set(rng.choice(pool, pool - k, replace=False).tolist())
        nd = [r for r in range(pool) if r not in gone]
    witness = min(gone)
    if i % 2:
        nd = [int(x) for x in rng.permutation(nd)]
    return nd, witness


def _batch(k, n):
    """One batch per shape, computed once and never changed: per object the
    body, its survivors' ids and bytes (oracle), their names, a witness's id,
    bytes and name, and the text the answer must carry."""
    if (k, n) in _CACHE:
        return _CACHE[(k, n)]
    rng = np.random.default_rng(7000 + 100 * k + n)
    sizes = [0, 1, 2 * k * 9 + 1, 2048 * k + 1] + ([65536] if k == 32 else [])
    if (k, n) == (16, 20):
        sizes.append(2 * k * 5 + 3)  # the object with an id >= 256
    objs = []
    for i, size in enumerate(sizes):
        body = O.splitmix(SEED + 9000 + 100 * k + i, size)
        nd, wid = _survivors(rng, k, n, i)
        if (k, n) == (16, 20) and i == len(sizes) - 1:
            nd[5] = 300
        surv = [O.encode(k, r, body) for r in nd]
        wit = O.encode(k, wid, body)
        objs.append({"size": size, "body": body, "nodes": nd, "surv": surv, "wid": wid, "wit": wit,
                     "names": [hashlib.sha256(c.tobytes()).digest() for c in surv],
                     "wname": hashlib.sha256(wit.tobytes()).digest(),
                     "text": base64.b64encode(body.tobytes()), "pad": size % (2 * k)})
    # the oracle's own restore gives the bodies back (the texts are the reference route's)
    for ob in objs:
        got = O.restore(k, ob["nodes"], ob["surv"])
        assert got is not None and np.array_equal(got, ob["body"])
    _CACHE[(k, n)] = objs
    return objs


def _replaced(objs, o, j, chunk):
    """The batch's survivors with survivor j of object o replaced (the batch itself stays as it is)."""
    surv = [list(ob["surv"]) for ob in objs]
    surv[o][j] = chunk
    return surv


def _flip(chunk, at, bit=0x10):
    c = chunk.copy()
    c[at] ^= bit
    return c


def _trailer(chunk):
    return (int(chunk[-2]) << 8) | int(chunk[-1])


def _with_trailer(chunk, p):
    c = chunk.copy()
    c[-2], c[-1] = p >> 8, p & 0xFF
    return c


class _Slots:
    """Buffers of the given sizes in one device allocation filled with FILL,
    each between GUARD-byte bands, so at unaligned addresses."""

    def __init__(self, torch, sizes):
        self.sizes, self.off, pos = list(sizes), [], GUARD
        for s in self.sizes:
            self.off.append(pos)
            pos += s + GUARD
        self.buf = torch.full((pos + 3,), FILL, dtype=torch.uint8, device="cuda")
        self.ptrs = [self.buf.data_ptr() + o for o in self.off]

    def read(self):
        """(contents per slot, True when no byte outside the slots changed)"""
        got = self.buf.cpu().numpy()
        mask = np.ones(got.size, dtype=bool)
        for o, s in zip(self.off, self.sizes):
            mask[o:o + s] = False
        return [got[o:o + s] for o, s in zip(self.off, self.sizes)], bool((got[mask] == FILL).all())


def _device_call(torch, chunk, k, objs, surv, mode, stream=None):
    """One vds_ec_download16_batch_device call on the survivors `surv` (host
    arrays): (statuses, texts as the buffers hold them, verdicts, witnesses)."""
    from vds_amd import _lib
    count = len(objs)
    keep = [[torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in row] for row in surv]
    csz = [row[0].size for row in surv]
    # restore reads the FIRST survivor's trailer (chunk.h:408): the caller passes what that file says
    pads = [_trailer(row[0]) for row in surv]
    texts = _Slots(torch, [len(ob["text"]) for ob in objs])
    bodies = _Slots(torch, [_lib.lib().vds_ec_restored_size(2, k, L, p) for L, p in zip(csz, pads)])
    wouts = _Slots(torch, csz)
    nver = count * (k if mode == "survivor" else 1)
    ver = _Slots(torch, [nver])
    st = torch.full((count,), ST_FILL, dtype=torch.int32, device="cuda")
    if mode == "survivor":
        raw = b"\x00" + b"".join(x for ob in objs for x in ob["names"])
    else:
        raw = b"\x00" + b"".join(ob["wname"] for ob in objs)
    names = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()  # (the names at an odd address)
    torch.cuda.synchronize()
    kw = {"survivor_names": names.data_ptr() + 1} if mode == "survivor" else {
        "witness_ids": [ob["wid"] for ob in objs], "witness_names": names.data_ptr() + 1, "witness_outs": wouts.ptrs}
    chunk.download_batch_device(k, [ob["nodes"] for ob in objs], [[c.data_ptr() for c in row] for row in keep], csz,
                                pads, bodies.ptrs, texts.ptrs, ver.ptrs[0], st, stream=stream, **kw)
    torch.cuda.synchronize()
    got_t, ok_t = texts.read()
    got_w, ok_w = wouts.read()
    got_v, ok_v = ver.read()
    assert ok_t and ok_w and ok_v and bodies.read()[1], "guard bytes written"
    return st.cpu().numpy().tolist(), got_t, got_v[0], got_w


def _host_call(k, objs, surv, mode, slack=0):
    """vds_ec_download16_host_batch through the C ABI: (statuses, texts as the
    buffers hold them, text_lens, survivor verdicts, failed)."""
    from vds_amd import _lib
    count = len(objs)
    surv = [[np.ascontiguousarray(c) for c in row] for row in surv]
    nd = np.asarray([ob["nodes"] for ob in objs], dtype=np.uint16).reshape(-1)
    cs = np.asarray([row[0].size for row in surv], dtype=np.uint64)
    cp = (C.c_void_p * (count * k))(*[c.ctypes.data for row in surv for c in row])
    sn = np.frombuffer(b"".join(x for ob in objs for x in ob["names"]), dtype=np.uint8).copy()
    wi = np.asarray([ob["wid"] for ob in objs], dtype=np.uint16)
    wn = np.frombuffer(b"".join(ob["wname"] for ob in objs), dtype=np.uint8).copy()
    need = [len(ob["text"]) for ob in objs]
    # the capacity a caller gives: what the first survivor's trailer, as the file holds it, asks for
    caps = [max(t, (_lib.lib().vds_ec_restored_size(2, k, row[0].size, _trailer(row[0])) + 2) // 3 * 4) + slack
            for t, row in zip(need, surv)]
    bufs = [np.full(GUARD + c + GUARD, FILL, dtype=np.uint8) for c in caps]
    tp = (C.c_void_p * count)(*[b.ctypes.data + GUARD for b in bufs])
    tl = np.asarray(caps, dtype=np.uint64)
    st = np.full(count, ST_FILL, dtype=np.int32)
    sv = np.full(count * k + 8, FILL, dtype=np.uint8)
    failed = C.c_uint32(12345)
    wit = mode == "witness"
    _lib.check(_lib.lib().vds_ec_download16_host_batch(
        k, count, nd.ctypes.data_as(_lib.u16p), cp, cs.ctypes.data_as(_lib.u64p), sn.ctypes.data,
        wi.ctypes.data_as(_lib.u16p) if wit else None, wn.ctypes.data if wit else None, tp,
        tl.ctypes.data_as(_lib.u64p), st.ctypes.data_as(C.POINTER(C.c_int32)), sv.ctypes.data, C.byref(failed)),
        "download16_host_batch")
    for b, t in zip(bufs, need):
        assert (b[:GUARD] == FILL).all() and (b[GUARD + t:] == FILL).all(), "guard bytes written"
    assert (sv[count * k:] == FILL).all()
    return (st.tolist(), [b[GUARD:GUARD + t] for b, t in zip(bufs, need)], tl.tolist(),
            sv[:count * k].reshape(count, k).tolist(), failed.value)


def _check_texts(objs, statuses, texts, bad=()):
    """Objects in `bad` failed and hold the sentinel; every other text is exact."""
    from vds_amd import _lib
    for o, ob in enumerate(objs):
        if o in bad:
            assert statuses[o] == _lib.ECORRUPT, (o, statuses)
            assert (texts[o] == FILL).all(), (o, "a corrupt object became text")
        else:
            assert statuses[o] == 0, (o, statuses)
            assert texts[o].tobytes() == ob["text"], (o, ob["size"])


# ------------------------------------------------------------- clean batches
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,n", SHAPES)
def test_clean_batch_device(gpu, k, n, mode):
    """Every route, every size (the empty object too: its status is written
    over the sentinel): status 0, text = b64encode(object), verdicts 0, the
    witness the oracle's replica, no guard byte changed."""
    import torch
    from vds_amd import chunk
    objs = _batch(k, n)
    stream = torch.cuda.Stream() if (k, n) == (32, 64) else None
    st, texts, ver, wouts = _device_call(torch, chunk, k, objs, [ob["surv"] for ob in objs], mode, stream)
    assert objs[0]["size"] == 0 and st[0] == 0
    _check_texts(objs, st, texts)
    assert (ver == 0).all()
    if mode == "witness":
        for o, ob in enumerate(objs):
            assert np.array_equal(wouts[o], ob["wit"]), o


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,n", SHAPES)
def test_clean_batch_host(gpu, k, n, mode):
    from vds_amd import chunk
    objs = _batch(k, n)
    st, texts, tl, sv, failed = _host_call(k, objs, [ob["surv"] for ob in objs], mode, slack=5 if n == 20 else 0)
    _check_texts(objs, st, texts)
    assert tl == [len(ob["text"]) for ob in objs] and failed == 0
    assert sv == [[0] * k] * len(objs)
    # the Python mirror: the same call from {id: bytes} mappings
    res = chunk.download_batch(k, [dict(zip(ob["nodes"], ob["surv"])) for ob in objs],
                               [ob["names"] for ob in objs],
                               [(ob["wid"], ob["wname"]) for ob in objs] if mode == "witness" else None)
    assert [r[0].encode() for r in res] == [ob["text"] for ob in objs]
    assert all(r[1] == 0 and r[2] == [0] * k for r in res)


# ---------------------------------------------------------------- corruption
def _corruptions(k, objs):
    """(what, object, survivor, its bytes): one bit of a cell of survivor 0; one
    bit of a cell of a middle survivor; the first survivor's trailer changed,
    staying <= 2k (p + 1: one byte more of the last stripe).  None of them in
    the empty object."""
    big = max(range(len(objs)), key=lambda o: objs[o]["size"])
    mid = 2
    a = objs[big]["surv"][0]
    b = objs[mid]["surv"][k // 2]
    p = objs[3]["pad"]
    q = p + 1
    assert 0 < p and q < 2 * k
    return [("cell of survivor 0", big, 0, _flip(a, 2 * ((a.size - 2) // 4) + 1)),
            ("cell of a middle survivor", mid, k // 2, _flip(b, 2 * 3, 0x01)),
            ("first trailer", 3, 0, _with_trailer(objs[3]["surv"][0], q))]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,n", [(16, 20), (32, 64), (3, 5)])
def test_corrupt_object_never_becomes_text(gpu, k, n, mode):
    """One object of the batch corrupted at a time: its status is
    VDS_EC_ECORRUPT and its text buffer still holds the sentinel, every other
    object's text is exact -- device form and host form; the host form's
    survivor_verdicts mark exactly the corrupted survivor and *failed counts
    the object."""
    import torch
    from vds_amd import chunk
    objs = _batch(k, n)
    for what, o, j, c in _corruptions(k, objs):
        surv = _replaced(objs, o, j, c)
        st, texts, ver, _ = _device_call(torch, chunk, k, objs, surv, mode)
        _check_texts(objs, st, texts, bad=(o,))
        if mode == "survivor":
            assert np.flatnonzero(ver).tolist() == [o * k + j], what
        else:
            assert np.flatnonzero(ver).tolist() == [o], what
        st, texts, tl, sv, failed = _host_call(k, objs, surv, mode)
        _check_texts(objs, st, texts, bad=(o,))
        assert failed == 1 and tl[o] == 0, what
        assert tl == [0 if i == o else len(ob["text"]) for i, ob in enumerate(objs)]
        want = [[0] * k for _ in objs]
        want[o][j] = 1
        assert sv == want, (what, mode)


def test_two_corrupt_objects_host(gpu):
    """Two objects of one batch corrupt, witness mode: both located by the one
    second launch, *failed == 2."""
    k, n = 32, 64
    objs = _batch(k, n)
    surv = _replaced(objs, 2, k - 1, _flip(objs[2]["surv"][k - 1], 0))
    surv[4][7] = _flip(objs[4]["surv"][7], 2 * 1000)
    st, texts, tl, sv, failed = _host_call(k, objs, surv, "witness")
    _check_texts(objs, st, texts, bad=(2, 4))
    want = [[0] * k for _ in objs]
    want[2][k - 1] = want[4][7] = 1
    assert sv == want and failed == 2


def test_trimmed_bytes_of_a_partial_last_stripe(gpu):
    """The other documented difference.  The object of one byte is one partial
    stripe: the reference route decodes it and keeps byte 0 only
    (chunk.h:415-419, 437-438).  A survivor's cell changed so that the decode
    differs in the trimmed bytes alone restores the SAME object (the oracle
    says so below) and regenerates the same witness: witness mode passes it,
    with the exact text; survivor mode, which hashes the files, fails it."""
    import torch
    from vds_amd import chunk
    k, n = 32, 64
    objs = _batch(k, n)
    o = 1
    assert objs[o]["size"] == 1
    surv = _replaced(objs, o, k - 1, _flip(objs[o]["surv"][k - 1], 0))
    ref = O.restore(k, objs[o]["nodes"], surv[o])
    assert ref is not None and np.array_equal(ref, objs[o]["body"])
    assert np.array_equal(O.encode(k, objs[o]["wid"], ref), objs[o]["wit"])
    st, texts, ver, _ = _device_call(torch, chunk, k, objs, surv, "witness")
    _check_texts(objs, st, texts)
    st, texts, ver, _ = _device_call(torch, chunk, k, objs, surv, "survivor")
    _check_texts(objs, st, texts, bad=(o,))
    assert np.flatnonzero(ver).tolist() == [o * k + k - 1]


def test_wrong_trailer_on_a_later_survivor(gpu):
    """The documented difference between the modes.  Survivor mode covers every
    byte of every survivor, trailers included: a wrong trailer on survivor 3
    fails the object and verdict 3 is set.  Witness mode covers every cell of
    every survivor and the FIRST survivor's trailer, as the reference route
    reads no other (chunk.h:408): the object passes, with the reference
    route's exact text."""
    import torch
    from vds_amd import chunk
    k, n = 32, 64
    objs = _batch(k, n)
    o = 2
    surv = _replaced(objs, o, 3, _with_trailer(objs[o]["surv"][3], 0x1234))
    ref = O.restore(k, objs[o]["nodes"], surv[o])
    assert ref is not None and base64.b64encode(ref.tobytes()) == objs[o]["text"]
    st, texts, ver, _ = _device_call(torch, chunk, k, objs, surv, "survivor")
    _check_texts(objs, st, texts, bad=(o,))
    assert np.flatnonzero(ver).tolist() == [o * k + 3]
    st, texts, ver, _ = _device_call(torch, chunk, k, objs, surv, "witness")
    _check_texts(objs, st, texts)
    assert (ver == 0).all()
    st, texts, tl, sv, failed = _host_call(k, objs, surv, "survivor")
    _check_texts(objs, st, texts, bad=(o,))
    assert failed == 1 and np.flatnonzero(np.asarray(sv).reshape(-1)).tolist() == [o * k + 3]
    st, texts, tl, sv, failed = _host_call(k, objs, surv, "witness")
    _check_texts(objs, st, texts)
    assert failed == 0 and sv == [[0] * k] * len(objs)


# ------------------------------------------------------- gate reduction width
@pytest.mark.parametrize("k,n", [(3, 5), (32, 64), (16, 20)])
def test_corrupt_last_survivor_gates(gpu, k, n):
    """Survivor mode: the gate is the object's k verdict bytes, and the LAST of
    them alone must shut it -- at k = 3, at k = 32, and for the (16,20)
    batch's object with an id >= 256 (one launch of its own for the restore)."""
    import torch
    from vds_amd import chunk
    objs = _batch(k, n)
    o = len(objs) - 1
    if n == 20:
        assert max(objs[o]["nodes"]) >= 256
    surv = _replaced(objs, o, k - 1, _flip(objs[o]["surv"][k - 1], 0, 0x80))
    st, texts, ver, _ = _device_call(torch, chunk, k, objs, surv, "survivor")
    _check_texts(objs, st, texts, bad=(o,))
    assert np.flatnonzero(ver).tolist() == [o * k + k - 1]


def test_gated_encode_alone_seventy_gate_bytes(gpu):
    """The gated launch itself: a gate of 70 bytes with only byte 69 set (past
    one wave of gate bytes) writes no character and sets the status; of a gate
    of 64 bytes with byte 63 set neither tile of a two-tile message is written;
    clean gates, an ungated message (its gate never read) and an empty message
    are written, and every status is set."""
    import torch
    from vds_amd import _lib, chunk
    rng = np.random.default_rng(70)
    lens = [1000, 1000, 0, 7000, 7000, 11, 0]
    ngates = [70, 70, 0, 64, 64, 0, 3]
    hot = {0: 69, 3: 63, 6: 2}
    msgs = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
    ins = _Slots(torch, lens)
    for p, m in zip(ins.off, msgs):
        ins.buf[p:p + m.size] = torch.from_numpy(m).cuda()
    gates = _Slots(torch, ngates)
    for p, g in zip(gates.off, ngates):
        gates.buf[p:p + g] = 0
    for m, b in hot.items():
        gates.buf[gates.off[m] + b] = 1 if m else 0x80
    outs = _Slots(torch, [(n + 2) // 3 * 4 for n in lens])
    st = torch.full((len(lens),), ST_FILL, dtype=torch.int32, device="cuda")
    gp = [0 if g == 0 else p for p, g in zip(gates.ptrs, ngates)]
    chunk.base64_encode_gated_batch_device(ins.ptrs, lens, outs.ptrs, gp, ngates, st)
    torch.cuda.synchronize()
    texts, clean = outs.read()
    assert clean, "guard bytes written"
    status = st.cpu().numpy().tolist()
    for m in range(len(lens)):
        if m in hot:
            assert status[m] == _lib.ECORRUPT and (texts[m] == FILL).all(), m
        else:
            assert status[m] == 0 and texts[m].tobytes() == base64.b64encode(msgs[m].tobytes()), m
