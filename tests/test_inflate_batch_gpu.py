"""zlib streams of a ragged batch inflated in one launch
(vds_ec_inflate_batch_device, inflate.hip) against Python's zlib -- the library
the reference links -- over the streams of tests/inflate_cases.py.  Status,
length and bytes; bit-exact.

Layout: every input of a launch lies in ONE device buffer with foreign bytes
(0xA5) between the streams, every output in ONE buffer with at least 64 guard
bytes (0x5A) before and behind it, and the statuses and lengths start as a
sentinel, so that one the launch did not write shows."""
import zlib

import numpy as np
import pytest

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


def _run(torch, cases, in_mod=lambda i: 0, out_mod=lambda i: 0):
    """One launch over cases = [(stream, cap, status, bytes)]: every status and out_len against the case's,
    the delivered bytes of every OK and SHORT stream against its own, nothing checked inside a failed
    stream's capacity, and every byte outside the capacities untouched."""
    from vds_amd import chunk
    count = len(cases)
    streams, caps = [c[0] for c in cases], [c[1] for c in cases]
    i_offs, i_total = _place([len(s) for s in streams], [in_mod(i) for i in range(count)], 16)
    o_offs, o_total = _place(caps, [out_mod(i) for i in range(count)], GUARD)
    buf = np.full(i_total, 0xA5, dtype=np.uint8)
    for s, off in zip(streams, i_offs):
        buf[off:off + len(s)] = np.frombuffer(s, dtype=np.uint8)
    d_in = torch.from_numpy(buf).cuda()
    d_out = torch.full((o_total,), FILL, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    d_len = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    d_st = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    chunk.inflate_batch_device([d_in.data_ptr() + o for o in i_offs], [len(s) for s in streams],
                               [d_out.data_ptr() + o for o in o_offs], caps, d_len, d_st)
    torch.cuda.synchronize()
    got, lens, sts = d_out.cpu().numpy(), d_len.cpu().numpy().view(np.uint32), d_st.cpu().numpy()
    inside = np.zeros(o_total, dtype=bool)
    for i, (s, cap, st, out) in enumerate(cases):
        assert (int(sts[i]), int(lens[i])) == (st, len(out)), ("stream", i, "of", count, "length", len(s), "cap", cap)
        assert got[o_offs[i]:o_offs[i] + len(out)].tobytes() == out, ("bytes of stream", i, "length", len(s))
        inside[o_offs[i]:o_offs[i] + cap] = True
    assert (got[~inside] == FILL).all(), "a byte outside the capacities was written"


def _case(stream, cap=None):
    st, out = K.expected(stream)
    return (stream, K.mutation_cap(stream) if cap is None else cap, st, out)


@pytest.fixture(scope="module")
def valid():
    return K.valid_cases()


def test_valid_streams_exact_and_short_caps(gpu, valid):
    import torch
    cases = []
    for name, s, data in valid:
        cases.append((s, len(data), 0, data))
        cases.append((s + b"\x00tail", len(data) + 7, 0, data))
        if data:
            cases.append((s, len(data) - 1, K.EINFLATE_SPACE, b""))
    _run(torch, cases)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_alignment(gpu, valid, shift):
    """input and output pointers at every offset 0..3 (all 16 pairs over four launches), on the short cases"""
    import torch
    cases = [(s, len(d), 0, d) for _, s, d in valid if len(d) <= 5000]
    cases += [_case(s) for _, s in K.failures()]
    cases += [_case(p[0]) for p in K.prefixes(K.prefix_streams()[1][1])[::7]]
    _run(torch, cases, in_mod=lambda i: i % 4, out_mod=lambda i: (i // 4 + shift) % 4)


def test_failures(gpu):
    import torch
    cases = [_case(s) for _, s in K.failures()]
    assert all(c[2] == K.EINFLATE_DATA for c in cases)
    _run(torch, cases)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_prefixes(gpu, kind):
    """every prefix of one stream as one batch of a few hundred messages"""
    import torch
    name, s = K.prefix_streams()[kind]
    cases = [(p, K.mutation_cap(s), st, out) for p, st, out in K.prefixes(s)]
    assert cases[0][2:] == (K.EINFLATE_SHORT, b"") and cases[-1][2] == 0
    _run(torch, cases, in_mod=lambda i: i % 4, out_mod=lambda i: (i // 4) % 4)


@pytest.mark.parametrize("kind", K.MUTATION_KINDS)
def test_mutations(gpu, kind):
    import torch
    cases = [(s, K.mutation_cap(s), st, out) for s, st, out in K.mutations(kind)]
    _run(torch, cases, in_mod=lambda i: i % 4)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_batch_counts(gpu, count):
    """lengths mixed so that the longest-first order differs from the caller's"""
    import torch
    cases = []
    for i in range(count):
        n = (i * 7919) % 3001 if i % 5 else (i * 131) % 17
        data = K.text(n, 100 + i) if i % 3 else K.splitmix(n, 100 + i)
        s = K.deflate(data, level=(0, 1, 6, 9)[i % 4])
        if i % 11 == 10:
            s = s[:len(s) // 2]
        st, out = K.expected(s)
        cases.append((s, len(data), st, out))
    lens = [len(c[0]) for c in cases]
    assert count == 1 or lens != sorted(lens, reverse=True)
    _run(torch, cases, in_mod=lambda i: (3 * i) % 4, out_mod=lambda i: i % 4)


def test_web_client_bodies(gpu):
    """64 bodies of 64 KiB as the web client makes them"""
    import torch
    datas = [K.text(65536, 200 + i) for i in range(64)]
    _run(torch, [(zlib.compress(d, 6), 65536, 0, d) for d in datas])


def test_host_batch(gpu, valid):
    """vds_ec_inflate_host_batch: the device's answers on host pointers; a failed stream has its output
    untouched and is counted"""
    import ctypes as C
    from vds_amd import chunk
    streams = [s for _, s, _ in valid] + [s for _, s in K.failures()[:4]] + [valid[3][1][:200], b""]
    caps = [len(d) for _, _, d in valid] + [4096] * 6
    caps[1] -= 1  # SPACE
    want = []
    for s, cap in zip(streams, caps):
        st, out = K.expected(s)
        want.append((None, K.EINFLATE_SPACE) if len(out) > cap else (out, 0) if st == 0 else (None, st))
    assert chunk.inflate_host_batch(streams, caps) == want
    assert {w[1] for w in want} == {0, K.EINFLATE_DATA, K.EINFLATE_SHORT, K.EINFLATE_SPACE}
    # straight through the C ABI: untouched outputs and the count
    from vds_amd import _lib
    lib = _lib.lib()
    n = len(streams)
    ins = [np.frombuffer(s, dtype=np.uint8).copy() if s else np.zeros(1, dtype=np.uint8) for s in streams]
    outs = [np.full(max(1, c), 0xC3, dtype=np.uint8) for c in caps]
    ln, cp = (C.c_uint64 * n)(*[len(s) for s in streams]), (C.c_uint64 * n)(*caps)
    ol, st, failed = (C.c_uint64 * n)(), (C.c_int32 * n)(), C.c_uint32(77)
    rc = lib.vds_ec_inflate_host_batch(n, (C.c_void_p * n)(*[a.ctypes.data for a in ins]), ln,
                                       (C.c_void_p * n)(*[a.ctypes.data for a in outs]), cp, ol, st, C.byref(failed))
    assert rc == 0 and failed.value == sum(1 for w in want if w[1])
    for i, (out, code) in enumerate(want):
        assert st[i] == code
        if code:
            assert ol[i] == 0 and (outs[i] == 0xC3).all(), i
        else:
            assert ol[i] == len(out) and outs[i][:len(out)].tobytes() == out, i
