"""File blocks packed and unpacked on the device (vds_ec_block_pack_batch_device
/ _host_batch, vds_ec_aes256_cbc_decrypt_host_batch, chunk.block_pack_batch /
block_unpack_batch): client::save and restore of the reference
(dht_network_client.cpp:1101-1320) for batches of blocks.

References: OpenSSL's recorded pack records (tests/golden/aes_cbc_kats.json)
and the three-line host composition of vds_ec_sha256_host and
vds_ec_aes256_cbc_encrypt_host.  Bit-exact."""
import hashlib
import random
import zlib

import numpy as np
import pytest

import aes_kats as K

pytestmark = pytest.mark.gpu

FILL = 0x5A
GUARD = 32


def _host_pack(lib, data: bytes, zipped: bytes):
    """client::save as three lines of host calls."""
    bid = np.zeros(32, dtype=np.uint8)
    assert lib.vds_ec_sha256_host(data, len(data), bid.ctypes.data) == 0
    c1 = K.host_encrypt(lib, bid.tobytes(), K.block_iv(), data)
    key = np.zeros(32, dtype=np.uint8)
    assert lib.vds_ec_sha256_host(c1, len(c1), key.ctypes.data) == 0
    return bid.tobytes(), key.tobytes(), K.host_encrypt(lib, key.tobytes(), K.block_iv(), zipped)


def _device_pack(torch, datas, zipped):
    """vds_ec_block_pack_batch_device over datas / zipped laid out back to back at odd offsets; the
    outputs between guards.  Returns [(id, key, crypted)] and the device tensors (kept alive)."""
    from vds_amd import chunk
    count = len(datas)

    def lay(pieces, step):
        offs, pos = [], 0
        for i, p in enumerate(pieces):
            pos = (pos + 15) // 16 * 16 + (i * step) % 16
            offs.append(pos)
            pos += len(p)
        buf = np.full(pos + 16, 0xA5, dtype=np.uint8)
        for p, off in zip(pieces, offs):
            buf[off:off + len(p)] = np.frombuffer(p, dtype=np.uint8)
        return torch.from_numpy(buf).cuda(), offs

    d_data, d_offs = lay(datas, 1)
    d_zip, z_offs = lay(zipped, 3)
    sizes = [len(z) // 16 * 16 + 16 for z in zipped]
    c_offs, pos = [], 0
    for i, s in enumerate(sizes):
        pos = (pos + 15) // 16 * 16 + GUARD + (i * 5) % 16
        c_offs.append(pos)
        pos += s
    d_out = torch.full((pos + GUARD + 16,), FILL, dtype=torch.uint8, device="cuda")
    d_ids = torch.full((max(1, count) * 32 + 16,), FILL, dtype=torch.uint8, device="cuda")
    d_keys = torch.full((max(1, count) * 32 + 16,), FILL, dtype=torch.uint8, device="cuda")
    chunk.block_pack_batch_device([d_data.data_ptr() + o for o in d_offs], [len(d) for d in datas],
                                  [d_zip.data_ptr() + o for o in z_offs], [len(z) for z in zipped], d_ids, d_keys,
                                  [d_out.data_ptr() + o for o in c_offs])
    torch.cuda.synchronize()
    out, ids, keys = d_out.cpu().numpy(), d_ids.cpu().numpy(), d_keys.cpu().numpy()
    mask = np.ones(out.size, dtype=bool)
    for o, s in zip(c_offs, sizes):
        mask[o:o + s] = False
    assert (out[mask] == FILL).all() and (ids[32 * count:] == FILL).all() and (keys[32 * count:] == FILL).all()
    res = [(ids[32 * i:32 * i + 32].tobytes(), keys[32 * i:32 * i + 32].tobytes(),
            out[c_offs[i]:c_offs[i] + sizes[i]].tobytes()) for i in range(count)]
    return res, (d_out, c_offs, sizes, d_ids, d_keys)


def _ragged(rng, count, top):
    """Blocks of 0 .. top bytes, compressible (words from a small alphabet) so the deflate is a real one."""
    sizes = [0, 1, 15, 16, 17, top] + [rng.randrange(top + 1) for _ in range(count - 6)]
    words = [rng.randbytes(rng.randrange(1, 12)) for _ in range(64)]
    blocks = []
    for n in sizes:
        b = bytearray()
        while len(b) < n:
            b += rng.choice(words)
        blocks.append(bytes(b[:n]))
    return blocks


@pytest.fixture(scope="module")
def ragged():
    rng = random.Random(21)
    datas = _ragged(rng, 33, 70000)
    return datas, [zlib.compress(d, 6) for d in datas]


def test_device_pack_fixture_records(gpu, vds_lib):
    import torch
    recs = K.kats()["pack"]
    datas = [K.sm(r["data_seed"], r["data_len"]) for r in recs]
    zipped = [K.sm(r["zipped_seed"], r["zipped_len"]) for r in recs]
    res, _ = _device_pack(torch, datas, zipped)
    for r, (bid, key, crypted) in zip(recs, res):
        assert bid.hex() == r["id"], r["data_len"]
        assert key.hex() == r["key"], r["data_len"]
        assert K.matches(r, "crypted", crypted), r["data_len"]


def test_device_pack_equals_host_composition(gpu, vds_lib, ragged):
    import torch
    datas, zipped = ragged
    assert len(datas) == 33 and min(map(len, datas)) == 0 and max(map(len, datas)) == 70000
    res, _ = _device_pack(torch, datas, zipped)
    for i, (d, z) in enumerate(zip(datas, zipped)):
        assert res[i] == _host_pack(vds_lib, d, z), (i, len(d), len(z))
    # a second call reuses the library's scratch: same answers
    res2, _ = _device_pack(torch, datas[::-1], zipped[::-1])
    assert res2 == res[::-1]


def test_host_batch_equals_device_form(gpu, vds_lib, ragged):
    import torch
    from vds_amd import chunk
    datas, zipped = ragged
    res, _ = _device_pack(torch, datas, zipped)
    assert chunk.block_pack_host_batch(datas, zipped) == res
    assert chunk.block_pack_host_batch([], []) == []
    # and the decrypt host batch gives the deflated bytes back
    back = chunk.aes256_cbc_decrypt_host_batch([c for _, _, c in res], [k for _, k, _ in res])
    assert back == [(z, 0) for z in zipped]


def test_pack_save_restore_unpack_on_device_pointers(gpu, vds_lib):
    """pack -> save_temp16 -> four replicas lost -> restore16 -> decrypt -> inflate -> name check, the
    bodies never leaving device memory between the calls (k = 16, n = 20, three blocks)."""
    import torch
    from vds_amd import chunk
    k, n = 16, 20
    rng = random.Random(22)
    datas = _ragged(rng, 6, 30000)[3:]
    datas = [datas[2], rng.randbytes(5000) * 3, datas[1]]
    zipped = [zlib.compress(d, 6) for d in datas]
    _, (d_out, c_offs, sizes, d_ids, d_keys) = _device_pack(torch, datas, zipped)
    count = len(datas)
    bodies = [d_out.data_ptr() + o for o in c_offs]
    Ls = [chunk.replica_size(k, s) for s in sizes]
    reps = [[torch.full((L,), FILL, dtype=torch.uint8, device="cuda") for _ in range(n)] for L in Ls]
    names = torch.zeros(count * n * 32, dtype=torch.uint8, device="cuda")
    chunk.save_temp_batch_device(k, n, bodies, sizes, [[r.data_ptr() for r in row] for row in reps], names)
    lost = [(0, 5, 17, 19), (1, 2, 3, 4), (16, 17, 18, 19)]
    nodes = [[r for r in range(n) if r not in lo] for lo in lost]
    restored = [torch.full((L * k + 64,), FILL, dtype=torch.uint8, device="cuda") for L in Ls]
    chunk.restore_batch_device(k, nodes, [[reps[o][r].data_ptr() for r in nodes[o]] for o in range(count)], Ls,
                               [s % (2 * k) for s in sizes], [r.data_ptr() for r in restored])
    plain = [torch.full((s + 64,), FILL, dtype=torch.uint8, device="cuda") for s in sizes]
    d_len = torch.full((count,), -1, dtype=torch.int32, device="cuda")
    d_st = torch.full((count,), -1, dtype=torch.int32, device="cuda")
    chunk.aes256_cbc_decrypt_batch_device([r.data_ptr() for r in restored], sizes, d_keys,
                                          [p.data_ptr() for p in plain], d_len, d_st)
    torch.cuda.synchronize()
    assert d_st.cpu().tolist() == [0] * count
    assert d_len.cpu().tolist() == [len(z) for z in zipped]
    inflated = []
    for o in range(count):
        got = plain[o].cpu().numpy()
        assert (got[sizes[o]:] == FILL).all()
        assert got[:len(zipped[o])].tobytes() == zipped[o]
        inflated.append(zlib.decompress(got[:len(zipped[o])].tobytes()))
    assert inflated == datas
    # the inflated bytes back on the device hash to the ids the pack wrote
    d_inf = [torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() for b in inflated]
    verdicts = torch.full((count,), 7, dtype=torch.uint8, device="cuda")
    chunk.sha256_check_batch_device([t.data_ptr() for t in d_inf], [len(b) for b in inflated], d_ids, verdicts)
    torch.cuda.synchronize()
    assert verdicts.cpu().tolist() == [0] * count
    assert d_ids.cpu().numpy()[:32 * count].tobytes() == b"".join(hashlib.sha256(d).digest() for d in datas)


def test_block_pack_and_unpack_batch(gpu, vds_lib, ragged):
    from vds_amd import chunk, VdsEcError
    datas = ragged[0][:12]
    packed = chunk.block_pack_batch(datas)
    for d, (bid, key, crypted) in zip(datas, packed):
        assert (bid, key, crypted) == _host_pack(vds_lib, d, zlib.compress(d, 6))
    ids, keys, crypted = ([p[i] for p in packed] for i in range(3))
    assert chunk.block_unpack_batch(crypted, keys, ids) == datas
    # a flipped byte in crypted: the status the host function gives for that same tampered input
    raised = set()
    for at in (-1, -17, 0, 40):
        bad = list(crypted)
        b = bytearray(bad[5])
        b[at] ^= 0x01
        bad[5] = bytes(b)
        st, plain = K.host_decrypt(vds_lib, keys[5], K.block_iv(), bad[5])
        with pytest.raises(VdsEcError) as e:
            chunk.block_unpack_batch(bad, keys, ids)
        # (where the padding still holds, the damage shows in the inflate or in the name)
        assert e.value.status == (st if st else K.ECORRUPT), at
        raised.add(e.value.status)
    assert K.ECORRUPT in raised
    bad = list(crypted)
    bad[3] = bad[3][:-5]
    with pytest.raises(VdsEcError) as e:
        chunk.block_unpack_batch(bad, keys, ids)
    assert e.value.status == K.ECRYPT_LENGTH == K.host_decrypt(vds_lib, keys[3], K.block_iv(), bad[3])[0]
    # a wrong id
    wrong = list(ids)
    wrong[6] = hashlib.sha256(b"another block").digest()
    with pytest.raises(VdsEcError) as e:
        chunk.block_unpack_batch(crypted, keys, wrong)
    assert e.value.status == K.ECORRUPT


def test_host_batches_split_into_groups(gpu, vds_lib):
    """More blocks than one staging group holds (65,536 a group): the second group's blocks land in
    the caller's arrays at their own places, for the pack and for the decrypt."""
    import ctypes as C
    from vds_amd import _lib
    count = 65536 + 7
    rng = np.random.default_rng(23)
    dl = rng.integers(0, 4, count).astype(np.uint64)
    zl = rng.integers(0, 18, count).astype(np.uint64)
    data = rng.integers(0, 256, int(dl.sum()) + 1, dtype=np.uint8)
    zipped = rng.integers(0, 256, int(zl.sum()) + 1, dtype=np.uint8)
    d_off = np.concatenate(([0], np.cumsum(dl)[:-1])).astype(np.uint64)
    z_off = np.concatenate(([0], np.cumsum(zl)[:-1])).astype(np.uint64)
    crypted = np.full(32 * count, FILL, dtype=np.uint8)
    ids = np.zeros((count, 32), dtype=np.uint8)
    keys = np.zeros((count, 32), dtype=np.uint8)
    cs = np.zeros(count, dtype=np.uint64)
    dp = (np.uint64(data.ctypes.data) + d_off).astype(np.uint64)
    zp = (np.uint64(zipped.ctypes.data) + z_off).astype(np.uint64)
    cp = (np.uint64(crypted.ctypes.data) + np.arange(count, dtype=np.uint64) * np.uint64(32)).astype(np.uint64)
    vpp, u64p = _lib.vpp, _lib.u64p
    assert vds_lib.vds_ec_block_pack_host_batch(count, dp.ctypes.data_as(vpp), dl.ctypes.data_as(u64p),
                                                zp.ctypes.data_as(vpp), zl.ctypes.data_as(u64p), ids.ctypes.data,
                                                keys.ctypes.data, cp.ctypes.data_as(vpp), cs.ctypes.data_as(u64p)) == 0
    assert np.array_equal(cs, (zl // 16 + 1) * 16)
    slots = crypted.reshape(count, 32)
    assert (slots[cs == 16, 16:] == FILL).all()

    def piece(buf, off, ln, i):
        return buf[int(off[i]):int(off[i] + ln[i])].tobytes()

    for i in range(count):
        assert ids[i].tobytes() == hashlib.sha256(piece(data, d_off, dl, i)).digest(), i
    sample = [0, 1, 65534, 65535, 65536, 65537, count - 1] + [int(x) for x in rng.integers(0, count, 60)]
    for i in sample:
        want = _host_pack(vds_lib, piece(data, d_off, dl, i), piece(zipped, z_off, zl, i))
        assert (ids[i].tobytes(), keys[i].tobytes(), slots[i, :int(cs[i])].tobytes()) == want, i
    # back: one length made bad and one body damaged, on either side of the group border
    lens = cs.copy()
    lens[5] = 0
    slots[65536 + 3, int(cs[65536 + 3]) - 1] ^= 0x55
    plain = np.full(32 * count, FILL, dtype=np.uint8)
    pp = (np.uint64(plain.ctypes.data) + np.arange(count, dtype=np.uint64) * np.uint64(32)).astype(np.uint64)
    ol = np.full(count, 99, dtype=np.uint64)
    st = np.full(count, 99, dtype=np.int32)
    failed = C.c_uint32(99)
    assert vds_lib.vds_ec_aes256_cbc_decrypt_host_batch(count, cp.ctypes.data_as(vpp), lens.ctypes.data_as(u64p),
                                                        keys.ctypes.data, None, pp.ctypes.data_as(vpp),
                                                        ol.ctypes.data_as(u64p), st.ctypes.data_as(_lib.i32p),
                                                        C.byref(failed)) == 0
    dst, dpt = K.host_decrypt(vds_lib, keys[65536 + 3].tobytes(), K.block_iv(), slots[65536 + 3, :int(cs[65536 + 3])].tobytes())
    want_st = np.zeros(count, dtype=np.int32)
    want_st[5], want_st[65536 + 3] = K.ECRYPT_LENGTH, dst
    assert np.array_equal(st, want_st) and failed.value == int((want_st != 0).sum())
    good = want_st == 0
    good[65536 + 3] = False  # (damaged: whatever the host function says of it, checked on its own)
    assert np.array_equal(ol[good], zl[good]) and ol[5] == 0 and ol[65536 + 3] == len(dpt)
    pslots = plain.reshape(count, 32)
    for i in np.flatnonzero(good):
        n = int(zl[i])
        assert pslots[i, :n].tobytes() == piece(zipped, z_off, zl, i) and (pslots[i, n:] == FILL).all(), i
    assert (pslots[5] == FILL).all()
    if dst:
        assert (pslots[65536 + 3] == FILL).all()
    else:
        assert pslots[65536 + 3, :len(dpt)].tobytes() == dpt
