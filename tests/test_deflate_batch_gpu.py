"""Buffers of a ragged batch deflated in one launch
(vds_ec_deflate_batch_device, deflate.hip) against vds_ec_deflate_host, the
sequential statement of the same algorithm, which tests/test_deflate_host_cpu.py
pins to zlib: the kernel's bytes and out_lens equal the host's, bit for bit,
over the bodies of tests/deflate_cases.py.

Layout as in tests/test_inflate_batch_gpu.py: every input of a launch lies in
ONE device buffer with foreign bytes (0xA5) between the messages, every output
in ONE buffer with at least 64 guard bytes (0x5A) before and behind its
capacity, out_lens starts as a sentinel, and every byte outside the capacities
is checked untouched."""
import ctypes as C

import numpy as np
import pytest

import deflate_cases as D
import inflate_cases as K

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0x5A
SENTINEL = 0x5A5A5A5A


def _place(sizes, mods, lead):
    """Offsets of pieces of `sizes` bytes, piece i at mods[i] modulo 16, at least `lead` bytes apart."""
    offs, pos = [], 0
    for n, m in zip(sizes, mods):
        pos = (pos + 15) // 16 * 16 + 16 * ((lead + 15) // 16) + m
        offs.append(pos)
        pos += n
    return offs, pos + lead + 16


_HOST = {}


def _host(data):
    """vds_ec_deflate_host of a body, computed once"""
    from vds_amd import chunk
    if data not in _HOST:
        _HOST[data] = chunk.deflate_host(data)
    return _HOST[data]


def _run(torch, datas, in_mod=lambda i: 0, out_mod=lambda i: 0, extra_cap=lambda i: 0):
    """One launch over `datas`: every out_len and every byte against the host's, every byte outside the
    capacities untouched.  Returns the device buffers for a second step."""
    from vds_amd import chunk
    count = len(datas)
    caps = [chunk.deflate_bound(len(d)) + extra_cap(i) for i, d in enumerate(datas)]
    i_offs, i_total = _place([len(d) for d in datas], [in_mod(i) for i in range(count)], 16)
    o_offs, o_total = _place(caps, [out_mod(i) for i in range(count)], GUARD)
    buf = np.full(i_total, 0xA5, dtype=np.uint8)
    for d, off in zip(datas, i_offs):
        buf[off:off + len(d)] = np.frombuffer(d, dtype=np.uint8)
    d_in = torch.from_numpy(buf).cuda()
    d_out = torch.full((o_total,), FILL, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    d_len = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    chunk.deflate_batch_device([d_in.data_ptr() + o for o in i_offs], [len(d) for d in datas],
                               [d_out.data_ptr() + o for o in o_offs], caps, d_len)
    torch.cuda.synchronize()
    got, lens = d_out.cpu().numpy(), d_len.cpu().numpy().view(np.uint32)
    inside = np.zeros(o_total, dtype=bool)
    for i, d in enumerate(datas):
        want = _host(d)
        assert int(lens[i]) == len(want), ("out_len of message", i, "of", count, "length", len(d))
        assert got[o_offs[i]:o_offs[i] + len(want)].tobytes() == want, ("bytes of message", i, "length", len(d))
        inside[o_offs[i]:o_offs[i] + caps[i]] = True
    assert (got[~inside] == FILL).all(), "a byte outside the capacities was written"
    return d_out, o_offs, lens, caps


def test_every_case_equals_the_host(gpu):
    import torch
    _run(torch, [d for _, d in D.cases()], extra_cap=lambda i: (0, 1, 37)[i % 3])


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_alignment(gpu, shift):
    """input and output pointers at every offset 0..3 (all 16 pairs over four launches), on the short cases"""
    import torch
    _run(torch, [d for _, d in D.short_cases()], in_mod=lambda i: i % 4, out_mod=lambda i: (i // 4 + shift) % 4)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_batch_counts(gpu, count):
    """lengths mixed so that the longest-first order differs from the caller's"""
    import torch
    datas = []
    for i in range(count):
        n = (i * 7919) % 3001 if i % 5 else (i * 131) % 17
        datas.append(K.text(n, 100 + i) if i % 3 else K.splitmix(n, 100 + i))
    lens = [len(d) for d in datas]
    assert count == 1 or lens != sorted(lens, reverse=True)
    _run(torch, datas, in_mod=lambda i: (3 * i) % 4, out_mod=lambda i: i % 4)


def test_web_client_bodies_and_back(gpu):
    """64 text bodies of 64 KiB; then the device's own streams through vds_ec_inflate_batch_device"""
    import torch
    from vds_amd import chunk
    datas = [K.text(65536, 200 + i) for i in range(64)] + [b"", K.splitmix(70000, 9), bytes(70000)]
    d_z, z_offs, z_lens, _ = _run(torch, datas)
    count = len(datas)
    o_offs, o_total = _place([len(d) for d in datas], [0] * count, GUARD)
    d_out = torch.full((o_total,), FILL, dtype=torch.uint8, device="cuda")
    d_len = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    d_st = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    chunk.inflate_batch_device([d_z.data_ptr() + o for o in z_offs], [int(n) for n in z_lens],
                               [d_out.data_ptr() + o for o in o_offs], [len(d) for d in datas], d_len, d_st)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (d_st.cpu().numpy() == 0).all()
    assert d_len.cpu().numpy().tolist() == [len(d) for d in datas]
    for d, off in zip(datas, o_offs):
        assert got[off:off + len(d)].tobytes() == d


def test_host_batch(gpu):
    """vds_ec_deflate_host_batch: the device's bytes on host pointers, through the wrapper and straight
    through the C ABI with guard bytes behind every capacity"""
    from vds_amd import _lib, chunk
    datas = [d for _, d in D.short_cases()] + [K.text(65536, 5), K.splitmix(65537, 6)]
    assert chunk.deflate_host_batch(datas) == [_host(d) for d in datas]
    assert chunk.deflate_host_batch([]) == []
    lib = _lib.lib()
    n = len(datas)
    ins = [np.frombuffer(d, dtype=np.uint8).copy() if d else np.zeros(1, dtype=np.uint8) for d in datas]
    caps = [chunk.deflate_bound(len(d)) for d in datas]
    outs = [np.full(c + 16, 0xC3, dtype=np.uint8) for c in caps]
    ln, cp, ol = (C.c_uint64 * n)(*[len(d) for d in datas]), (C.c_uint64 * n)(*caps), (C.c_uint64 * n)()
    rc = lib.vds_ec_deflate_host_batch(n, (C.c_void_p * n)(*[a.ctypes.data for a in ins]), ln,
                                       (C.c_void_p * n)(*[a.ctypes.data for a in outs]), cp, ol)
    assert rc == 0
    for i, d in enumerate(datas):
        want = _host(d)
        assert ol[i] == len(want) and outs[i][:len(want)].tobytes() == want, i
        assert (outs[i][caps[i]:] == 0xC3).all(), i
