"""File blocks packed with the deflate on the device
(vds_ec_block_pack_deflate_batch_device / _host_batch) and its last launch on
its own (vds_ec_aes256_cbc_encrypt_gated_batch_device): client::save of the
reference (dht_network_client.cpp:1107-1140) in five launches.

References: vds_ec_aes256_cbc_encrypt_host, vds_ec_deflate_host (pinned to zlib
by tests/test_deflate_host_cpu.py) and vds_ec_block_pack_batch_device (pinned to
OpenSSL's records by tests/test_block_pack_gpu.py).  Bit-exact."""
import hashlib
import random

import numpy as np
import pytest

import inflate_cases as K

pytestmark = pytest.mark.gpu

FILL = 0x5A
GUARD = 64
SENTINEL = 0x5A5A5A5A


def _padded(n):
    return n // 16 * 16 + 16


def _lay(torch, pieces, step):
    """pieces back to back in one device buffer, piece i at (i * step) modulo 16, foreign bytes between"""
    offs, pos = [], 0
    for i, p in enumerate(pieces):
        pos = (pos + 15) // 16 * 16 + 16 + (i * step) % 16
        offs.append(pos)
        pos += len(p)
    buf = np.full(pos + 32, 0xA5, dtype=np.uint8)
    for p, off in zip(pieces, offs):
        buf[off:off + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return torch.from_numpy(buf).cuda(), offs


def _slots(torch, caps, step):
    """one output buffer with GUARD bytes around every capacity"""
    offs, pos = [], 0
    for i, c in enumerate(caps):
        pos = (pos + 15) // 16 * 16 + GUARD + (i * step) % 16
        offs.append(pos)
        pos += c
    return torch.full((pos + GUARD + 16,), FILL, dtype=torch.uint8, device="cuda"), offs


def test_gated_encrypt(gpu, vds_lib):
    """device lengths below their max_lens: the host's ciphertext, out_lens, nothing past padded_size(len)"""
    import torch
    from vds_amd import chunk
    lens = [0, 1, 15, 16, 17, 4097, 31, 32, 1000]
    maxs = [5, 16, 16, 40, 33, 5000, 31, 4096, 1001]
    rng = random.Random(31)
    msgs = [rng.randbytes(m) for m in maxs]
    keys = [rng.randbytes(32) for _ in lens]
    d_in, i_offs = _lay(torch, msgs, 3)
    d_out, o_offs = _slots(torch, [_padded(m) for m in maxs], 5)
    d_keys = torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).cuda()
    d_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    d_ol = torch.full((len(lens),), SENTINEL, dtype=torch.int32, device="cuda")
    chunk.aes256_cbc_encrypt_gated_batch_device([d_in.data_ptr() + o for o in i_offs], maxs, d_lens, d_keys,
                                                [d_out.data_ptr() + o for o in o_offs], d_ol)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert d_ol.cpu().tolist() == [_padded(n) for n in lens]
    inside = np.zeros(got.size, dtype=bool)
    for i, n in enumerate(lens):
        want = chunk.aes256_cbc_encrypt_host(keys[i], msgs[i][:n])
        assert got[o_offs[i]:o_offs[i] + len(want)].tobytes() == want, i
        inside[o_offs[i]:o_offs[i] + _padded(n)] = True
    assert (got[~inside] == FILL).all(), "a byte past padded_size(len) was written"


def _bodies():
    rng = random.Random(32)
    words = [rng.randbytes(rng.randrange(1, 12)) for _ in range(64)]

    def wordy(n):
        b = bytearray()
        while len(b) < n:
            b += rng.choice(words)
        return bytes(b[:n])

    return [b"", wordy(1), wordy(15), wordy(16), wordy(3583), wordy(3585), wordy(70000), K.splitmix(5000, 3),
            K.text(65536, 1), bytes(20000), K.splitmix(66000, 4), wordy(33)]


def _pack(torch, datas):
    """the fused pack over datas at odd offsets -> [(id, key, crypted)], and what stays on the device"""
    from vds_amd import chunk
    count = len(datas)
    caps = [_padded(chunk.deflate_bound(len(d))) for d in datas]
    d_data, d_offs = _lay(torch, datas, 1)
    d_out, c_offs = _slots(torch, caps, 5)
    d_ids = torch.full((count * 32 + 16,), FILL, dtype=torch.uint8, device="cuda")
    d_keys = torch.full((count * 32 + 16,), FILL, dtype=torch.uint8, device="cuda")
    d_cl = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    chunk.block_pack_deflate_batch_device([d_data.data_ptr() + o for o in d_offs], [len(d) for d in datas], d_ids,
                                          d_keys, [d_out.data_ptr() + o for o in c_offs], caps, d_cl)
    torch.cuda.synchronize()
    out, ids, keys, cl = d_out.cpu().numpy(), d_ids.cpu().numpy(), d_keys.cpu().numpy(), d_cl.cpu().tolist()
    inside = np.zeros(out.size, dtype=bool)
    for o, c in zip(c_offs, caps):
        inside[o:o + c] = True
    assert (out[~inside] == FILL).all() and (ids[32 * count:] == FILL).all() and (keys[32 * count:] == FILL).all()
    res = [(ids[32 * i:32 * i + 32].tobytes(), keys[32 * i:32 * i + 32].tobytes(),
            out[c_offs[i]:c_offs[i] + cl[i]].tobytes()) for i in range(count)]
    return res, (d_out, c_offs, cl, d_ids, d_keys, out, caps)


def test_fused_pack(gpu, vds_lib):
    """ids and keys as vds_ec_block_pack_batch_device writes them, crypted = AES(key, deflate_host(data)),
    crypted_lens right, nothing written past a body's size; the host form gives the same"""
    import torch
    from vds_amd import chunk
    datas = _bodies()
    res, (d_out, c_offs, cl, _, _, out, caps) = _pack(torch, datas)
    zipped = [chunk.deflate_host(d) for d in datas]
    # the pack that takes the deflated bytes from the caller, on the same blocks
    count = len(datas)
    d_data, d_offs = _lay(torch, datas, 1)
    d_zip, z_offs = _lay(torch, zipped, 3)
    d_ref, r_offs = _slots(torch, [_padded(len(z)) for z in zipped], 0)
    d_ids = torch.zeros(count * 32, dtype=torch.uint8, device="cuda")
    d_keys = torch.zeros(count * 32, dtype=torch.uint8, device="cuda")
    chunk.block_pack_batch_device([d_data.data_ptr() + o for o in d_offs], [len(d) for d in datas],
                                  [d_zip.data_ptr() + o for o in z_offs], [len(z) for z in zipped], d_ids, d_keys,
                                  [d_ref.data_ptr() + o for o in r_offs])
    torch.cuda.synchronize()
    ids, keys = d_ids.cpu().numpy(), d_keys.cpu().numpy()
    for i, (d, z) in enumerate(zip(datas, zipped)):
        bid, key, crypted = res[i]
        assert bid == ids[32 * i:32 * i + 32].tobytes() == hashlib.sha256(d).digest(), i
        assert key == keys[32 * i:32 * i + 32].tobytes(), i
        assert cl[i] == _padded(len(z)), i
        assert crypted == chunk.aes256_cbc_encrypt_host(key, z), i
        assert (out[c_offs[i] + cl[i]:c_offs[i] + caps[i]] == FILL).all(), i
    assert chunk.block_pack_deflate_host_batch(datas) == res
    assert chunk.block_pack_deflate_host_batch([]) == []
    # a second call reuses the library's scratch: same answers
    res2, _ = _pack(torch, datas[::-1])
    assert res2 == res[::-1]


def test_round_trip_through_unpack(gpu, vds_lib):
    """vds_ec_block_unpack_batch_device gives every block back with status OK: a body of length 0 and
    stored ones (splitmix) among them"""
    import torch
    from vds_amd import chunk
    datas = _bodies()
    count = len(datas)
    _, (d_out, c_offs, cl, d_ids, d_keys, _, _) = _pack(torch, datas)
    d_back, b_offs = _slots(torch, [len(d) for d in datas], 1)
    d_len = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    d_st = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    chunk.block_unpack_batch_device([d_out.data_ptr() + o for o in c_offs], cl, d_keys, d_ids,
                                    [d_back.data_ptr() + o for o in b_offs], [len(d) for d in datas], d_len, d_st)
    torch.cuda.synchronize()
    assert d_st.cpu().tolist() == [0] * count
    assert d_len.cpu().tolist() == [len(d) for d in datas]
    got = d_back.cpu().numpy()
    for d, off in zip(datas, b_offs):
        assert got[off:off + len(d)].tobytes() == d


def test_pack_save_restore_unpack_on_device_pointers(gpu, vds_lib):
    """fused pack -> crypted_lens read back (count * 4 bytes) -> save_temp16 -> four replicas lost ->
    restore16 -> unpack, k = 16 and n = 20, the bodies never leaving device memory"""
    import torch
    from vds_amd import chunk
    k, n = 16, 20
    datas = [K.text(30000, 41), b"", K.splitmix(9000, 42), K.text(4096, 43) * 3]
    count = len(datas)
    _, (d_out, c_offs, sizes, d_ids, d_keys, _, _) = _pack(torch, datas)
    bodies = [d_out.data_ptr() + o for o in c_offs]
    Ls = [chunk.replica_size(k, s) for s in sizes]
    reps = [[torch.full((L,), FILL, dtype=torch.uint8, device="cuda") for _ in range(n)] for L in Ls]
    names = torch.zeros(count * n * 32, dtype=torch.uint8, device="cuda")
    chunk.save_temp_batch_device(k, n, bodies, sizes, [[r.data_ptr() for r in row] for row in reps], names)
    lost = [(0, 5, 17, 19), (1, 2, 3, 4), (16, 17, 18, 19), (0, 1, 18, 19)]
    nodes = [[r for r in range(n) if r not in lo] for lo in lost]
    restored = [torch.full((L * k + 64,), FILL, dtype=torch.uint8, device="cuda") for L in Ls]
    chunk.restore_batch_device(k, nodes, [[reps[o][r].data_ptr() for r in nodes[o]] for o in range(count)], Ls,
                               [s % (2 * k) for s in sizes], [r.data_ptr() for r in restored])
    back = [torch.full((len(d) + 64,), FILL, dtype=torch.uint8, device="cuda") for d in datas]
    d_len = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    d_st = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    chunk.block_unpack_batch_device([r.data_ptr() for r in restored], sizes, d_keys, d_ids,
                                    [b.data_ptr() for b in back], [len(d) for d in datas], d_len, d_st)
    torch.cuda.synchronize()
    assert d_st.cpu().tolist() == [0] * count
    assert d_len.cpu().tolist() == [len(d) for d in datas]
    for d, b in zip(datas, back):
        got = b.cpu().numpy()
        assert got[:len(d)].tobytes() == d and (got[len(d):] == FILL).all()
