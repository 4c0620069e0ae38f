"""The batched upload from text (vds_ec_upload16_host_batch, chunk.upload_batch):
websocket "upload" bodies (base64) decoded on the device in front of the
batched save_temp.  Checked against the already-tested routes --
chunk.save_temp_batch of the decoded bodies, chunk.upload -- and hashlib."""
import base64
import ctypes as C
import hashlib
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(32, 64), (16, 20)]
FILL = 0x5A
EB64_LENGTH, EB64_PADDING, EB64_CHAR = -7, -8, -9
MALFORMED = {3: (b"QUJDR", EB64_LENGTH, "Non-Valid base64!"),
             7: (b"QU=DQUJD", EB64_PADDING, "Invalid Padding in Base 64!"),
             11: (b"QUJDQU*D", EB64_CHAR, "Non-Valid Character in Base 64!")}


def _bodies(k, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, s, dtype=np.uint8)
            for s in (0, 1, 2, 3, 63, 64, 65, 2 * k - 1, 2 * k, 2 * k + 1, 4097, 65499, 65536)]


_WANT = {}


def _want(k, n):
    """chunk.save_temp_batch of the bodies: computed once, shared, left unchanged."""
    from vds_amd import chunk
    if (k, n) not in _WANT:
        bodies = _bodies(k, 10 * k + n)
        _WANT[k, n] = (bodies, chunk.save_temp_batch(k, n, bodies))
    return _WANT[k, n]


@pytest.mark.parametrize("k,n", SHAPES)
def test_upload_batch_against_existing_routes(gpu, k, n):
    from vds_amd import chunk
    bodies, want = _want(k, n)
    texts = [base64.b64encode(b.tobytes()).decode() for b in bodies]
    ids = list(range(100, 100 + len(bodies)))
    got = chunk.upload_batch(ids, texts, k, n, bodies=True)
    assert len(got) == len(bodies)
    for body, res, (w_reps, w_names, w_hash, w_rsize) in zip(bodies, got, want):
        assert res["data_hash"] == w_hash == hashlib.sha256(body.tobytes()).digest(), body.size
        assert res["replica_digests"] == w_names, body.size
        assert res["tmp_names"] == chunk.tmp_names(w_names)
        assert json.loads(res["json"])["result"]["replica_size"] == str(w_rsize), body.size
        for r in range(n):
            assert res["replicas"][r].size == w_rsize
            assert np.array_equal(res["replicas"][r], w_reps[r]), (body.size, r)
            assert res["replica_digests"][r] == hashlib.sha256(res["replicas"][r].tobytes()).digest(), (body.size, r)
        assert res["body"] == body.tobytes(), body.size
    for j in (5, 11):
        assert got[j]["json"] == chunk.upload(ids[j], texts[j], k, n)["json"]
    # without the bodies the rest is the same
    lean = chunk.upload_batch(ids, texts, k, n)
    assert [r["json"] for r in lean] == [r["json"] for r in got] and "body" not in lean[0]


class RawUpload:
    """vds_ec_upload16_host_batch on buffers of the test's own, every one
    filled with FILL (and 8 bytes longer than what it must receive)."""

    def __init__(self, lib, k, n, texts, body_hashes=True):
        from vds_amd import _lib, chunk
        count = len(texts)
        self.sizes = [lib.vds_ec_base64_decoded_size(t, len(t)) for t in texts]
        self.L = [chunk.replica_size(k, s) for s in self.sizes]
        self.outs = [[np.full(self.L[o] + 8, FILL, dtype=np.uint8) for _ in range(n)] for o in range(count)]
        self.bufs = [np.full(self.sizes[o] + 8, FILL, dtype=np.uint8) for o in range(count)]
        self.rd = np.full((count * n, 32), FILL, dtype=np.uint8)
        self.dd = np.full((count, 32), FILL, dtype=np.uint8)
        self.rs = np.full(count, 0x5A5A5A5A, dtype=np.uint32)
        self.bs = np.full(count, 0x5A5A5A5A, dtype=np.uint64)
        self.st = np.full(count, 0x5A5A5A5A, dtype=np.int32)
        failed = C.c_uint32(99)
        tp = (C.c_char_p * count)(*texts)
        tl = np.asarray([len(t) for t in texts], dtype=np.uint64)
        op = (C.c_void_p * (count * n))(*[o.ctypes.data for os_ in self.outs for o in os_])
        bp = (C.c_void_p * count)(*[b.ctypes.data for b in self.bufs])
        self.rc = lib.vds_ec_upload16_host_batch(
            k, n, count, C.cast(tp, _lib.vpp), tl.ctypes.data_as(_lib.u64p), op, self.rd.ctypes.data,
            self.dd.ctypes.data if body_hashes else None, self.rs.ctypes.data_as(C.POINTER(C.c_uint32)), bp,
            self.bs.ctypes.data_as(_lib.u64p), self.st.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(failed))
        self.failed = failed.value


@pytest.mark.parametrize("k,n", SHAPES)
def test_malformed_members(gpu, vds_lib, k, n):
    """The same batch with one member of each error: their statuses and
    `failed` are right, their output buffers keep the fill, every other
    message is as before."""
    from vds_amd import chunk
    bodies, want = _want(k, n)
    texts = [base64.b64encode(b.tobytes()) for b in bodies]
    for at in sorted(MALFORMED):
        texts.insert(at, MALFORMED[at][0])
    ok = [i for i in range(len(texts)) if i not in MALFORMED]  # the batch's index of well-formed message j
    u = RawUpload(vds_lib, k, n, texts)
    assert u.rc == 0 and u.failed == len(MALFORMED)
    for o, (_, status, _) in MALFORMED.items():
        assert u.st[o] == status, o
        assert all((x == FILL).all() for x in u.outs[o]) and (u.bufs[o] == FILL).all(), o
        assert (u.rd[o * n:(o + 1) * n] == FILL).all() and (u.dd[o] == FILL).all(), o
        assert u.rs[o] == 0x5A5A5A5A and u.bs[o] == 0x5A5A5A5A, o
    for o, body, (w_reps, w_names, w_hash, w_rsize) in zip(ok, bodies, want):
        assert u.st[o] == 0 and u.rs[o] == w_rsize and u.bs[o] == body.size, o
        assert bytes(u.dd[o]) == w_hash and [bytes(x) for x in u.rd[o * n:(o + 1) * n]] == w_names, o
        assert np.array_equal(u.bufs[o][:body.size], body) and (u.bufs[o][body.size:] == FILL).all(), o
        for r in range(n):
            assert np.array_equal(u.outs[o][r][:w_rsize], w_reps[r]) and (u.outs[o][r][w_rsize:] == FILL).all(), (o, r)
    # and through the Python form: the reference's error text
    got = chunk.upload_batch(list(range(len(texts))), texts, k, n)
    for o, (_, _, message) in MALFORMED.items():
        assert got[o] == message
    assert all(isinstance(got[o], dict) for o in ok)


def test_beyond_one_staging_group(gpu, vds_lib):
    """Three texts of 24 MiB + 5 bytes of body each (32 MiB + 8 characters):
    more than one 64 MiB staging group.  Replicas and names against
    vds_ec_save_temp16_host_batch of the bodies, the bodies against the input;
    neither side hashes the bodies here (one lane walks a body's chain, over a
    second for each of these; the body hashes are checked at the live sizes
    above)."""
    from vds_amd import chunk
    k, n = 16, 20
    rng = np.random.default_rng(24)
    bodies = [rng.integers(0, 256, (24 << 20) + 5, dtype=np.uint8) for _ in range(3)]
    u = RawUpload(vds_lib, k, n, [base64.b64encode(b.tobytes()) for b in bodies], body_hashes=False)
    assert u.rc == 0 and u.failed == 0 and not u.st.any()
    L = chunk.replica_size(k, bodies[0].size)
    w_outs = [np.empty(L, dtype=np.uint8) for _ in range(3 * n)]
    w_rd = np.empty((3 * n, 32), dtype=np.uint8)
    ip = (C.c_void_p * 3)(*[b.ctypes.data for b in bodies])
    op = (C.c_void_p * (3 * n))(*[o.ctypes.data for o in w_outs])
    sz = np.asarray([b.size for b in bodies], dtype=np.uint64)
    assert vds_lib.vds_ec_save_temp16_host_batch(k, n, 3, ip, sz.ctypes.data_as(C.POINTER(C.c_uint64)), op,
                                                 w_rd.ctypes.data, None, None) == 0
    assert np.array_equal(u.rd, w_rd) and (u.dd == FILL).all()
    for o, body in enumerate(bodies):
        assert u.bs[o] == body.size and u.rs[o] == L
        assert np.array_equal(u.bufs[o][:body.size], body) and (u.bufs[o][body.size:] == FILL).all(), o
        for r in range(n):
            assert np.array_equal(u.outs[o][r][:L], w_outs[o * n + r]) and (u.outs[o][r][L:] == FILL).all(), (o, r)
