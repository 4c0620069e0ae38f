"""The node-to-node datagram layer's host pieces (no GPU):
vds_ec_hmac_sha256_host against Python's hmac (OpenSSL, as the reference's
hmac::signature, kernel/vds_crypto/hash.cpp:218-260) and RFC 4231;
vds_ec_dgram_layout against a plain restatement of prepare_to_send's cutting
rules (impl/dht_datagram_protocol.cpp:335-541); vds_ec_write_number against
binary_serializer::write_number (binary_serialize.cpp:44-66); argument
validation of every new entry point, which answers before any device is looked
for; the new status texts."""
import ctypes as C
import hashlib
import hmac

import numpy as np
import pytest


# ------------------------------------------------- the sealing rules, restated
def layout(mtu, r, m):
    """(count, message bytes in the first datagram, length of the last)."""
    total = 1 + 4 + 32 + r + m
    if total < mtu:
        return 1, m, total
    c0 = mtu - (1 + 4 + 4 + 32 + r)
    count, off, last = 1, c0, 0
    while True:  # the reference's continuation loop (:490-531)
        size = min(mtu - (1 + 4 + 32), m - off)
        count += 1
        last = 1 + 4 + size + 32
        if off + size >= m:
            break
        off += size
    return count, c0, last


def test_hmac_host_against_python():
    from vds_amd import chunk
    rng = np.random.default_rng(11)
    for kl in (0, 32, 64, 65, 100):
        key = rng.integers(0, 256, kl, dtype=np.uint8).tobytes()
        for n in range(131):
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            assert chunk.hmac_sha256_host(key, data) == hmac.digest(key, data, "sha256"), (kl, n)


RFC4231 = [  # (key, data, HMAC-SHA-256), test cases 1-4 and 6
    (b"\x0b" * 20, b"Hi There", "b0344c61d8db38535ca8afceaf0bf12b881dc200c9833da726e9376c2e32cff7"),
    (b"Jefe", b"what do ya want for nothing?", "5bdcc146bf60754e6a042426089575c75a003f089d2739839dec58b964ec3843"),
    (b"\xaa" * 20, b"\xdd" * 50, "773ea91e36800e46854db8ebd09181a72959098b3ef8c122d9635514ced565fe"),
    (bytes(range(1, 26)), b"\xcd" * 50, "82558a389a443c0ea4cc819899f2083a85f0faa3e578f8077a2e3ff46729665b"),
    (b"\xaa" * 131, b"Test Using Larger Than Block-Size Key - Hash Key First",
     "60e431591ee0b67f0d8a26aacbf5b77f8e0bc6213728c5140546040f0ee37f54"),
]


@pytest.mark.parametrize("case", range(len(RFC4231)))
def test_hmac_host_rfc4231(case):
    from vds_amd import chunk
    key, data, mac = RFC4231[case]
    assert chunk.hmac_sha256_host(key, data).hex() == mac


def test_layout_against_restatement():
    from vds_amd import chunk
    # (with the shapes of tests/test_dgram_edges_gpu.py: proxied routes of 4 to
    # 255 hops, r = 33 + 32 hops, wherever 41 + r fits the mtu, and mtu 9000)
    for mtu in (508, 509, 1400, 9000, 65535):
        for r in (0, 32, 33, 97, 161, 193, 449, 673, 1313, 8193):
            if 41 + r >= mtu:
                continue
            c0 = mtu - (41 + r)
            per = mtu - 37
            ms = {0, 1, c0 - 1, c0, c0 + 3, c0 + 4, c0 + 5, c0 + per - 1, c0 + per, c0 + per + 1, c0 + 2 * per,
                  c0 + 2 * per + 1, 2154 + r}
            if mtu == 508:
                ms |= set(range(0, 3 * mtu + 1))
            for m in sorted(ms):
                assert chunk.dgram_layout(mtu, r, m) == layout(mtu, r, m), (mtu, r, m)
    # the boundaries the issue names, from the rules: the largest single, the
    # smallest split (a 4-byte continuation), full and one-byte last continuations
    assert layout(508, 0, 470) == (1, 470, 507)
    assert layout(508, 0, 471) == (2, 467, 37 + 4)
    assert layout(508, 0, 467 + 471)[2] == 508 and layout(508, 0, 467 + 2 * 471) == (3, 467, 508)
    assert layout(508, 0, 467 + 2 * 471 + 1) == (4, 467, 38)
    assert layout(508, 0, 2154) == (5, 467, 37 + 2154 - 467 - 3 * 471)


def test_layout_rejects():
    from vds_amd import _lib
    lib = _lib.lib()
    n = C.c_uint32(0)
    for mtu, r, m in ((507, 0, 10), (65536, 0, 10), (508, 31, 10), (508, 33 + 32 * 256, 10), (508, 33 + 32 * 14, 10),
                      (508, 0, 1 << 32), (508, 34, 10)):
        assert lib.vds_ec_dgram_layout(mtu, r, m, C.byref(n), None, None) == _lib.EINVAL, (mtu, r, m)
    assert lib.vds_ec_dgram_layout(508, 33 + 32 * 13, 10, None, None, None) == 0  # 41 + 449 < 508


def _write_number(value):  # binary_serialize.cpp:44-66
    if value < 128:
        return bytes([value])
    value -= 128
    data = []
    while True:
        data.append(value & 0xFF)
        value >>= 8
        if value == 0:
            break
    return bytes([0x80 | len(data)]) + bytes(reversed(data))


def test_write_number():
    from vds_amd import chunk
    for v in (0, 127, 128, 383, 384, 2050, 1 << 32, (1 << 64) - 1):
        assert chunk.write_number(v) == _write_number(v), v
    assert chunk.write_number(127) == b"\x7f" and chunk.write_number(128) == b"\x81\x00"
    assert chunk.write_number(383) == b"\x81\xff" and chunk.write_number(384) == b"\x82\x01\x00"


def test_strerror_texts():
    from vds_amd import _lib
    assert _lib.strerror(_lib.EDGRAM_SIGNATURE) == "Invalid signature"
    assert _lib.strerror(_lib.EDGRAM_DATA) == "Invalid data"
    assert "incomplete" in _lib.strerror(_lib.EDGRAM_INCOMPLETE)
    assert (_lib.EDGRAM_SIGNATURE, _lib.EDGRAM_DATA, _lib.EDGRAM_INCOMPLETE) == (-11, -12, -13)


# ------------------------------------------------------------ validation
class _Args:
    """One well-formed message / datagram; the pointers are never dereferenced
    by a call that fails its validation."""

    def __init__(self):
        from vds_amd import _lib
        self.L = _lib
        self.buf = np.zeros(4096, dtype=np.uint8)
        self.keys = np.zeros(64, dtype=np.uint8)
        p = self.buf.ctypes.data
        self.ptr = (C.c_void_p * 1)(p)
        self.null = (C.c_void_p * 1)(None)
        self.len64 = (C.c_uint64 * 1)(100)
        self.len32 = (C.c_uint32 * 1)(100)
        self.zero = (C.c_uint32 * 1)(0)
        self.two = (C.c_uint32 * 1)(2)
        self.mtu = (C.c_uint32 * 1)(508)
        self.type = (C.c_uint8 * 1)(5)
        self.msgs = (_lib.DgramMessage * 1)()
        self.n = C.c_uint32(0)
        self.o64 = (C.c_uint64 * 1)(0)
        self.o32a = (C.c_uint32 * 1)(0)
        self.o32b = (C.c_uint32 * 1)(0)


def test_validation_hmac_batch():
    a = _Args()
    f, E = a.L.lib().vds_ec_hmac_sha256_batch_device, a.L.EINVAL
    k, p = a.keys.ctypes.data, a.buf.ctypes.data
    assert f(0, None, None, None, None, 0, None, None, None, None) == 0
    assert f(1, None, a.len64, a.zero, k, 2, p, None, None, None) == E
    assert f(1, a.ptr, None, a.zero, k, 2, p, None, None, None) == E
    assert f(1, a.ptr, a.len64, None, k, 2, p, None, None, None) == E
    assert f(1, a.ptr, a.len64, a.zero, None, 2, p, None, None, None) == E
    assert f(1, a.ptr, a.len64, a.two, k, 2, p, None, None, None) == E       # session_of >= nsessions
    assert f(1, a.null, a.len64, a.zero, k, 2, p, None, None, None) == E     # null message, non-zero length
    assert f(1, a.ptr, a.len64, a.zero, k, 2, None, None, None, None) == E   # nothing to write
    assert f(1, a.ptr, a.len64, a.zero, k, 2, p, p, None, None) == E         # expected without verdicts
    assert f(1, a.ptr, a.len64, a.zero, k, 2, p, None, p, None) == E
    assert f(1 << 30, a.ptr, a.len64, a.zero, k, 2, p, None, None, None) == E


def test_validation_seal():
    a = _Args()
    lib, E = a.L.lib(), a.L.EINVAL
    k, p = a.keys.ctypes.data, a.buf.ctypes.data

    def dev(count=1, msgs=a.ptr, lens=a.len64, types=a.type, i0=a.zero, routes=a.null, rl=a.zero, so=a.zero, keys=k,
            mtus=a.mtu, ns=2, outs=a.ptr, pitch=508):
        return lib.vds_ec_dgram_seal_batch_device(count, msgs, lens, types, i0, routes, rl, so, keys, mtus, ns, outs,
                                                  pitch, None)

    def host(count=1, msgs=a.ptr, lens=a.len64, types=a.type, i0=a.zero, routes=a.null, rl=a.zero, so=a.zero, keys=k,
             mtus=a.mtu, ns=2, slab=p, cap=4096, offs=a.o64, cnts=a.o32a, lasts=a.o32b):
        return lib.vds_ec_dgram_seal_host_batch(count, msgs, lens, types, i0, routes, rl, so, keys, mtus, ns, slab, cap,
                                                offs, cnts, lasts)

    for f in (dev, host):
        assert f(count=0) == 0
        assert f(msgs=None) == E and f(lens=None) == E and f(types=None) == E and f(i0=None) == E
        assert f(rl=None) == E and f(so=None) == E and f(keys=None) == E and f(mtus=None) == E
        assert f(msgs=a.null) == E
        assert f(types=(C.c_uint8 * 1)(32)) == E
        assert f(mtus=(C.c_uint32 * 1)(507)) == E and f(mtus=(C.c_uint32 * 1)(65536)) == E
        assert f(so=a.two) == E
        assert f(rl=(C.c_uint32 * 1)(32)) == E                    # a route length with no route
        assert f(routes=a.ptr, rl=(C.c_uint32 * 1)(31)) == E      # not one of the three forms
        assert f(count=1 << 30) == E
        # 100 bytes at mtu 508: one datagram, so i0 = 2^32 - 1 fits; 2154 bytes are 5 and pass 2^32
        assert f(lens=(C.c_uint64 * 1)(2154), i0=(C.c_uint32 * 1)(0xFFFFFFFC)) == E
    assert dev(outs=None) == E and dev(outs=a.null) == E and dev(pitch=507) == E and dev(pitch=1 << 32) == E
    assert host(slab=None) == E and host(cap=136) == E and host(offs=None) == E and host(cnts=None) == E
    assert host(lasts=None) == E


def test_validation_open():
    a = _Args()
    lib, E = a.L.lib(), a.L.EINVAL
    k, p = a.keys.ctypes.data, a.buf.ctypes.data

    def dev(count=1, dg=a.ptr, lens=a.len32, hdr=a.zero, so=a.zero, keys=k, ns=2, dsts=a.ptr, vd=p):
        return lib.vds_ec_dgram_open_batch_device(count, dg, lens, hdr, so, keys, ns, dsts, vd, None)

    def host(count=1, dg=a.ptr, lens=a.len32, so=a.zero, keys=k, ns=2, vd=p, slab=p, cap=4096, msgs=a.msgs,
             nm=C.byref(a.n)):
        return lib.vds_ec_dgram_open_host_batch(count, dg, lens, so, keys, ns, vd, slab, cap, msgs, nm)

    for f in (dev, host):
        assert f(count=0) == 0
        assert f(dg=None) == E and f(lens=None) == E and f(so=None) == E and f(keys=None) == E and f(vd=None) == E
        assert f(dg=a.null) == E and f(so=a.two) == E and f(count=1 << 30) == E
        assert f(lens=(C.c_uint32 * 1)(65536)) == E
    assert dev(hdr=None) == E and dev(hdr=(C.c_uint32 * 1)(69)) == E  # past len - 32
    assert host(msgs=None) == E and host(nm=None) == E
