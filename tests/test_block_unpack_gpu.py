"""client::restore for a batch of blocks in one call (vds_ec_block_unpack_batch_device
and _host_batch): decrypt, inflate, name check, no host step between them.

The checkers: Python's zlib and hashlib, and the library's host cipher
(pinned against OpenSSL's recorded answers by tests/test_aes_host_cpu.py).
Bit-exact, status for status."""
import collections
import ctypes as C
import hashlib
import zlib

import numpy as np
import pytest

import aes_kats as A
import inflate_cases as K

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0x5A
SENTINEL = 0x5A5A5A5A


def _reference(lib, crypted, key, ident, cap):
    """(status, data) as the reference's restore would have it, step by step"""
    st, plain = A.host_decrypt(lib, key, A.block_iv(), crypted)
    if st:
        return st, b""
    zst, out = K.expected(plain)
    if zst == K.EINFLATE_DATA:
        return zst, b""
    if len(out) > cap:
        return K.EINFLATE_SPACE, b""
    return (0, out) if hashlib.sha256(out).digest() == ident else (K.ECORRUPT, b"")


def _device_unpack(torch, blocks):
    """blocks = [(crypted, key, id, cap)] through the device form -> [(status, data)]; every status and
    length written, nothing outside the capacities touched"""
    from vds_amd import chunk
    count = len(blocks)
    c_offs, pos = [], 0
    for c, _, _, _ in blocks:
        c_offs.append(pos)
        pos += (len(c) + 15) // 16 * 16 + 16
    buf = np.full(pos + 16, 0xA5, dtype=np.uint8)
    for (c, _, _, _), off in zip(blocks, c_offs):
        buf[off:off + len(c)] = np.frombuffer(c, dtype=np.uint8)
    o_offs, pos = [], GUARD
    for i, (_, _, _, cap) in enumerate(blocks):
        o_offs.append(pos + i % 4)
        pos += cap + GUARD + 4
    d_in = torch.from_numpy(buf).cuda()
    d_keys = torch.from_numpy(np.frombuffer(b"".join(b[1] for b in blocks), dtype=np.uint8).copy()).cuda()
    # the ids at an odd address: they are any bytes of the caller's
    d_ids = torch.from_numpy(np.frombuffer(b"\x00" + b"".join(b[2] for b in blocks), dtype=np.uint8).copy()).cuda()
    d_out = torch.full((pos,), FILL, dtype=torch.uint8, device="cuda")
    d_len = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    d_st = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    chunk.block_unpack_batch_device([d_in.data_ptr() + o for o in c_offs], [len(b[0]) for b in blocks], d_keys,
                                    d_ids.data_ptr() + 1, [d_out.data_ptr() + o for o in o_offs],
                                    [b[3] for b in blocks], d_len, d_st)
    torch.cuda.synchronize()
    got, lens, sts = d_out.cpu().numpy(), d_len.cpu().numpy().view(np.uint32), d_st.cpu().numpy()
    res = []
    inside = np.zeros(got.size, dtype=bool)
    for i, b in enumerate(blocks):
        assert int(sts[i]) != SENTINEL and int(lens[i]) != SENTINEL, i
        assert sts[i] == 0 or lens[i] == 0, i
        res.append((int(sts[i]), got[o_offs[i]:o_offs[i] + int(lens[i])].tobytes()))
        inside[o_offs[i]:o_offs[i] + b[3]] = True
    assert (got[~inside] == FILL).all(), "a byte outside the capacities was written"
    return res


@pytest.fixture(scope="module")
def packed(gpu):
    from vds_amd import chunk
    datas = [K.text(n, 300 + i) if i % 3 else K.splitmix(n, 300 + i)
             for i, n in enumerate((0, 1, 100, 5000, 65536, 70001, 33, 4097, 20000, 15, 16, 17))]
    zipped = [zlib.compress(d, 6) for d in datas]
    return datas, zipped, chunk.block_pack_host_batch(datas, zipped)


def test_pack_then_unpack(gpu, vds_lib, packed):
    import torch
    from vds_amd import chunk
    datas, zipped, res = packed
    blocks = [(c, k, i, len(d) + (o % 3)) for o, (d, (i, k, c)) in enumerate(zip(datas, res))]
    assert _device_unpack(torch, blocks) == [(0, d) for d in datas]
    ids, keys, crypted = ([r[j] for r in res] for j in range(3))
    assert chunk.block_unpack_host_batch(crypted, keys, ids, [b[3] for b in blocks]) == [(d, 0) for d in datas]
    assert chunk.block_unpack_host_batch([], [], [], []) == []
    # what the parent's route gives for the same bodies
    assert chunk.block_unpack_batch(crypted, keys, ids) == datas


def _failure_batch(lib, packed):
    """[(crypted, key, id, cap, expected status)]: one block per failure, good blocks between them"""
    datas, zipped, res = packed
    iv = A.block_iv()
    sha = lambda b: hashlib.sha256(b).digest()

    def good(o):
        return (res[o][2], res[o][1], res[o][0], len(datas[o]), 0)

    flipped = bytearray(res[3][2])
    flipped[-3] ^= 0x40
    half = zipped[8][:len(zipped[8]) // 2]
    delivered = K.expected(half)
    assert delivered[0] == K.EINFLATE_SHORT and len(delivered[1]) > 1000
    key = res[8][1]
    return [
        good(4),
        (res[2][2][:17], res[2][1], res[2][0], 100, K.ECRYPT_LENGTH),                 # a ciphertext of length 17
        good(0),
        (bytes(flipped), res[3][1], res[3][0], 5000, K.ECRYPT_PADDING),               # a flipped last cipher block
        (A.host_encrypt(lib, key, iv, b"not a zlib stream at all, only text"), key, res[8][0], 20000,
         K.EINFLATE_DATA),
        good(5),
        (A.host_encrypt(lib, key, iv, half), key, res[8][0], 20000, K.ECORRUPT),      # a truncated stream
        # ... which is OK where what it delivers is what the id names, as in the reference
        (A.host_encrypt(lib, key, iv, half), key, sha(delivered[1]), 20000, 0),
        (res[7][2], res[7][1], sha(b"another block"), 4097, K.ECORRUPT),              # a valid stream, the wrong id
        (res[7][2], res[7][1], res[7][0], 4096, K.EINFLATE_SPACE),                    # a too-small cap
        good(7),
        (b"", res[1][1], res[1][0], 8, K.ECRYPT_LENGTH),
        good(1),
    ]


def test_one_block_per_failure(gpu, vds_lib, packed):
    import torch
    batch = _failure_batch(vds_lib, packed)
    want = [_reference(vds_lib, c, k, i, cap) for c, k, i, cap, _ in batch]
    assert [w[0] for w in want] == [b[4] for b in batch]  # each is the failure it is meant to be
    assert _device_unpack(torch, [b[:4] for b in batch]) == want


def test_forms_no_compressor_emits(gpu, vds_lib):
    """64 streams of tests/inflate_forms.py -- table shapes up to 15 bits, degenerate sets, refused headers,
    truncated streams -- as block bodies: the inflate reached through the decrypt's gate and lengths, the
    bytes behind each message PKCS#7 padding.  A stream that ends short goes on to the hash."""
    import torch
    import inflate_forms as F
    iv = A.block_iv()
    sha = lambda b: hashlib.sha256(b).digest()
    shapes = F.table_shapes()
    cases = F.degenerate() + shapes[:14] + shapes[14::11][:30]
    short = [c for c in F.prefixes() if c[3] == K.EINFLATE_SHORT and len(c[4]) > 10][::97][:6]
    assert len(short) == 6
    blocks, want = [], []
    for i, (name, s, cap, st, out) in enumerate((cases + short)[:64]):
        key = K.splitmix(32, 900 + i)
        named = i % 2 == 0  # of the short ones: the id names what was delivered, or something else
        ident = sha(out) if st == 0 or (st == K.EINFLATE_SHORT and named) else sha(b"not this")
        blocks.append((A.host_encrypt(vds_lib, key, iv, s), key, ident, cap))
        want.append((K.EINFLATE_DATA, b"") if st == K.EINFLATE_DATA else (0, out) if st == 0 or named else (K.ECORRUPT, b""))
    assert len(blocks) == 64 and len({len(b[0]) - len(c[1]) for b, c in zip(blocks, cases + short)}) >= 8
    assert [_reference(vds_lib, *b) for b in blocks] == want
    assert collections.Counter(w[0] for w in want) == {0: 53, K.EINFLATE_DATA: 8, K.ECORRUPT: 3}
    assert _device_unpack(torch, blocks) == want


def test_host_form_leaves_failed_outputs_untouched(gpu, vds_lib, packed):
    from vds_amd import chunk
    batch = _failure_batch(vds_lib, packed)
    want = [_reference(vds_lib, c, k, i, cap) for c, k, i, cap, _ in batch]
    got = chunk.block_unpack_host_batch(*[[b[j] for b in batch] for j in range(4)])
    assert got == [(None, st) if st else (d, 0) for st, d in want]
    # straight through the C ABI: untouched outputs and the count
    n = len(batch)
    ins = [np.frombuffer(b[0], dtype=np.uint8).copy() if b[0] else np.zeros(1, dtype=np.uint8) for b in batch]
    outs = [np.full(max(1, b[3]), 0xC3, dtype=np.uint8) for b in batch]
    keys = np.frombuffer(b"".join(b[1] for b in batch), dtype=np.uint8).copy()
    ids = np.frombuffer(b"".join(b[2] for b in batch), dtype=np.uint8).copy()
    ln, cp = (C.c_uint64 * n)(*[len(b[0]) for b in batch]), (C.c_uint64 * n)(*[b[3] for b in batch])
    ol, st, failed = (C.c_uint64 * n)(), (C.c_int32 * n)(), C.c_uint32(77)
    rc = vds_lib.vds_ec_block_unpack_host_batch(n, (C.c_void_p * n)(*[a.ctypes.data for a in ins]), ln,
                                                keys.ctypes.data, ids.ctypes.data,
                                                (C.c_void_p * n)(*[a.ctypes.data for a in outs]), cp, ol, st,
                                                C.byref(failed))
    assert rc == 0 and failed.value == sum(1 for w in want if w[0])
    for i, (code, data) in enumerate(want):
        assert st[i] == code, i
        if code:
            assert ol[i] == 0 and (outs[i] == 0xC3).all(), i
        else:
            assert ol[i] == len(data) and outs[i][:len(data)].tobytes() == data, i
