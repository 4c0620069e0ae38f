"""vds_ec_deflate_host, the sequential statement of the device deflate, on the
CPU: every body of tests/deflate_cases.py comes back through Python's zlib --
the library the reference links -- and through vds_ec_inflate_host, no output
passes vds_ec_deflate_bound, and the sizes stay inside the bars below.  The
GPU suite pins the kernel's bytes to this function's."""
import ctypes as C
import zlib

import numpy as np
import pytest

import deflate_cases as D
import inflate_cases as K


@pytest.fixture(scope="module")
def packed(vds_lib):
    from vds_amd import chunk
    return [(name, data, chunk.deflate_host(data)) for name, data in D.cases()]


def _bound(n):
    return 2 + n + 5 * max(1, -(-n // 65535)) + 4


def test_bound(vds_lib):
    from vds_amd import chunk
    for n in (0, 1, 65534, 65535, 65536, 131070, 131071, (1 << 20) + 5, (1 << 32) - 1):
        assert chunk.deflate_bound(n) == _bound(n)


def test_round_trip_through_zlib_and_inflate_host(packed):
    from vds_amd import chunk
    for name, data, out in packed:
        d = zlib.decompressobj()
        assert d.decompress(out) == data and d.eof, name
        assert d.unused_data == b"", name
        assert out[:2] == b"\x78\x01", name
        assert chunk.inflate_host(out, len(data)) == (K.OK, data), name
        assert len(out) <= chunk.deflate_bound(len(data)), name


def test_exact_capacity_and_smaller(vds_lib, packed):
    """out_cap exactly the bound gives the same bytes (deflate_host passes exactly that); one byte less is EINVAL"""
    from vds_amd import _lib
    lib = _lib.lib()
    for name, data, out in packed[::3]:
        src = np.frombuffer(data, dtype=np.uint8).copy() if data else np.zeros(1, dtype=np.uint8)
        bound = _bound(len(data))
        buf = np.full(bound + 64, 0x5A, dtype=np.uint8)
        n = C.c_uint64(0)
        assert lib.vds_ec_deflate_host(src.ctypes.data if data else None, len(data), buf.ctypes.data, bound,
                                       C.byref(n)) == 0, name
        assert buf[:n.value].tobytes() == out and (buf[bound:] == 0x5A).all(), name
        assert lib.vds_ec_deflate_host(src.ctypes.data if data else None, len(data), buf.ctypes.data, bound - 1,
                                       C.byref(n)) == K.EINVAL, name


def test_argument_errors(vds_lib):
    from vds_amd import _lib
    lib = _lib.lib()
    src, dst, n = np.zeros(64, dtype=np.uint8), np.zeros(128, dtype=np.uint8), C.c_uint64(0)
    assert lib.vds_ec_deflate_host(src.ctypes.data, 64, dst.ctypes.data, 128, None) == K.EINVAL
    assert lib.vds_ec_deflate_host(None, 64, dst.ctypes.data, 128, C.byref(n)) == K.EINVAL
    assert lib.vds_ec_deflate_host(src.ctypes.data, 64, None, 128, C.byref(n)) == K.EINVAL
    assert lib.vds_ec_deflate_host(src.ctypes.data, 1 << 32, dst.ctypes.data, 1 << 33, C.byref(n)) == K.EINVAL
    assert lib.vds_ec_deflate_host(src.ctypes.data, (1 << 32) - 12, dst.ctypes.data, 1 << 33, C.byref(n)) == K.EINVAL
    both = np.zeros(256, dtype=np.uint8)  # input and output overlapping
    assert lib.vds_ec_deflate_host(both.ctypes.data + 100, 64, both.ctypes.data, 128, C.byref(n)) == K.EINVAL
    assert lib.vds_ec_deflate_host(None, 0, dst.ctypes.data, 11, C.byref(n)) == 0 and n.value == 11
    assert zlib.decompress(dst[:11].tobytes()) == b""
    # the batch forms reject before the device is looked for (so also without one)
    one_in, one_out = (C.c_void_p * 1)(src.ctypes.data), (C.c_void_p * 1)(dst.ctypes.data)
    ln, small, ok = (C.c_uint64 * 1)(64), (C.c_uint64 * 1)(_bound(64) - 1), (C.c_uint64 * 1)(_bound(64))
    lens = (C.c_uint32 * 1)()
    assert lib.vds_ec_deflate_batch_device(1, one_in, ln, one_out, small, lens, None) == K.EINVAL
    assert lib.vds_ec_deflate_batch_device(1, one_in, ln, one_out, ok, None, None) == K.EINVAL
    assert lib.vds_ec_deflate_batch_device(1, None, ln, one_out, ok, lens, None) == K.EINVAL
    assert lib.vds_ec_deflate_batch_device(0, None, None, None, None, None, None) == 0
    assert lib.vds_ec_deflate_host_batch(1, one_in, ln, one_out, small, (C.c_uint64 * 1)()) == K.EINVAL
    ids, keys = np.zeros(32, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
    body_cap = (C.c_uint64 * 1)((_bound(64) // 16 + 1) * 16 - 1)
    assert lib.vds_ec_block_pack_deflate_batch_device(1, one_in, ln, ids.ctypes.data, keys.ctypes.data, one_out,
                                                      body_cap, lens, None) == K.EINVAL
    assert lib.vds_ec_block_pack_deflate_batch_device(0, None, None, None, None, None, None, None, None) == 0
    assert lib.vds_ec_aes256_cbc_encrypt_gated_batch_device(1, one_in, ln, None, keys.ctypes.data, None, one_out,
                                                            lens, None) == K.EINVAL


def test_forms(packed):
    """what each content must come out as"""
    by = {name: (data, out) for name, data, out in packed}
    btype = lambda out: (out[2] >> 1) & 3
    for n in D.LENGTHS:
        data, out = by[f"splitmix-{n}"]
        assert btype(out) == 0 and len(out) == _bound(n), n  # stored, and merged into blocks of 65535
    assert len(by["zeros-65536"][1]) < 1024  # chained 258-byte matches at distance 1: a few hundred bytes
    assert btype(by["no-match-64"][1]) == 2  # a dynamic block with an empty distance tree
    assert btype(by["fibonacci-16"][1]) == 2 and btype(by["one-byte-300"][1]) == 2
    data, out = by["period32769-65537"]  # no legal match: nothing to gain
    assert len(out) == _bound(len(data))
    for p in (32767, 32768):
        data, out = by[f"period{p}-65638"]
        # Matches at the farthest distances are found and written (zlib has inflated them above).  Only
        # some: 32767 positions of random bytes pass through 4096 slots between a position and its
        # copy, so the one probe mostly meets a younger position with the same hash.
        assert len(out) < len(data), p


@pytest.mark.parametrize("n", [65536, 4096])
def test_size_against_zlib(vds_lib, n, capsys):
    """Summed over inflate_cases.text(n, 200..203), at most 1.25 x zlib level 1's size.  The bar comes from
    a model of this match finder (single probe, 12-bit table, chunks of 64, distance 1, greedy, minimum 4)
    costed at the entropy of its tokens: 1.07 x level 1 at 64 KiB, 1.13 x at 4 KiB; the margin is for the
    tree headers, whole-bit code lengths and the 15-bit limit.  The gap to level 6 is the price of one
    probe and no lazy evaluation: printed, no bar."""
    from vds_amd import chunk
    bodies = [K.text(n, 200 + i) for i in range(4)]
    ours = sum(len(chunk.deflate_host(b)) for b in bodies)
    l1 = sum(len(zlib.compress(b, 1)) for b in bodies)
    l6 = sum(len(zlib.compress(b, 6)) for b in bodies)
    with capsys.disabled():
        print(f"\ndeflate_host n={n}: {ours / (4 * n):.4f} of the input; zlib level 1 {l1 / (4 * n):.4f} "
              f"(ours / level 1 = {ours / l1:.3f}), level 6 {l6 / (4 * n):.4f} (ours / level 6 = {ours / l6:.3f})")
    assert ours <= 1.25 * l1
