"""vds_ec_inflate_host (inflate_host.cpp) against Python's zlib -- the library
the reference links -- over the streams of tests/inflate_cases.py, and the
argument checks of the five inflate / unpack entries, none of which needs a
GPU.  Status, length and bytes; bit-exact."""
import ctypes as C

import numpy as np
import pytest

import inflate_cases as K

GUARD = 64
FILL = 0xEE


def _run(lib, stream: bytes, cap: int):
    """(status, delivered bytes); the guard behind the capacity must be untouched whatever happens"""
    buf = np.full(cap + GUARD, FILL, dtype=np.uint8)
    src = np.frombuffer(stream, dtype=np.uint8) if stream else None
    n = C.c_uint64(0xDEAD)
    st = lib.vds_ec_inflate_host(src.ctypes.data if stream else None, len(stream), buf.ctypes.data, cap, C.byref(n))
    assert (buf[cap:] == FILL).all(), "a byte at or past the capacity was written"
    assert n.value <= cap
    if st in (K.EINFLATE_DATA, K.EINFLATE_SPACE):
        assert n.value == 0
    return st, buf[:n.value].tobytes()


@pytest.fixture(scope="module")
def valid():
    return K.valid_cases()


def test_statuses_and_binding(vds_lib):
    from vds_amd import _lib, chunk
    assert (_lib.EINFLATE_DATA, _lib.EINFLATE_SHORT, _lib.EINFLATE_SPACE) == (-20, -21, -22)
    assert (K.EINFLATE_DATA, K.EINFLATE_SHORT, K.EINFLATE_SPACE) == (-20, -21, -22)
    assert b"inflate failed" in vds_lib.vds_ec_strerror(K.EINFLATE_DATA)
    assert len({vds_lib.vds_ec_strerror(s) for s in (-20, -21, -22)}) == 3
    assert vds_lib.vds_ec_version() >= 102
    s = K.deflate(b"hello, hello, hello")
    assert chunk.inflate_host(s, 19) == (0, b"hello, hello, hello")
    assert chunk.inflate_host(s, 18) == (K.EINFLATE_SPACE, b"")
    assert chunk.inflate_host(s[:-1], 19) == (K.EINFLATE_SHORT, b"hello, hello, hello")
    assert chunk.inflate_host(b"", 0) == (K.EINFLATE_SHORT, b"")


def test_valid_streams(vds_lib, valid):
    for name, s, data in valid:
        assert _run(vds_lib, s, len(data)) == (0, data), name                       # OK at cap = length
        assert _run(vds_lib, s, len(data) + 100) == (0, data), name
        if data:
            assert _run(vds_lib, s, len(data) - 1) == (K.EINFLATE_SPACE, b""), name  # SPACE at cap = length - 1
            assert _run(vds_lib, s, 0) == (K.EINFLATE_SPACE, b""), name
        # bytes behind the stream's end are ignored, as the reference ignores them
        assert _run(vds_lib, s + b"\x00tail", len(data)) == (0, data), name


def test_failures(vds_lib):
    for name, s in K.failures():
        assert _run(vds_lib, s, K.mutation_cap(s)) == (K.EINFLATE_DATA, b""), name
        # an error shows only once its bits are inside the input: every prefix as zlib sees it
        for n in range(len(s)):
            assert _run(vds_lib, s[:n], K.mutation_cap(s)) == K.expected(s[:n]), (name, n)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_prefixes(vds_lib, kind):
    name, s = K.prefix_streams()[kind]
    pre = K.prefixes(s)
    assert pre[0][1:] == (K.EINFLATE_SHORT, b"") and pre[-1][1] == 0
    assert len({len(p[2]) for p in pre}) >= 100  # zlib delivers that many different lengths
    for p, st, out in pre:
        assert _run(vds_lib, p, K.mutation_cap(s)) == (st, out), (name, len(p))


def test_mutation_set_holds_every_class():
    """from zlib alone (the seed was chosen for it): the set holds all three classes"""
    by = [m[1] for kind in K.MUTATION_KINDS for m in K.mutations(kind)]
    assert len(by) == 256 * len(K.MUTATION_KINDS)
    assert by.count(0) >= 20 and by.count(K.EINFLATE_DATA) >= 20 and by.count(K.EINFLATE_SHORT) >= 5


@pytest.mark.parametrize("kind", K.MUTATION_KINDS)
def test_mutations(vds_lib, kind):
    muts = K.mutations(kind)
    for i, (s, st, out) in enumerate(muts):
        assert _run(vds_lib, s, K.mutation_cap(s)) == (st, out), (kind, i)


def test_short_keeps_what_fits(vds_lib, valid):
    """a prefix whose bytes do not fit is SPACE; one whose bytes fit exactly is SHORT with them"""
    s = dict((n, s) for n, s, _ in valid)["dynamic level 6"]
    st, out = K.expected(s[:len(s) // 2])
    assert st == K.EINFLATE_SHORT and len(out) > 100
    assert _run(vds_lib, s[:len(s) // 2], len(out)) == (st, out)
    assert _run(vds_lib, s[:len(s) // 2], len(out) - 1) == (K.EINFLATE_SPACE, b"")


def test_argument_checks(vds_lib):
    """all five entries: EINVAL before the device is looked for, so it shows here"""
    lib = vds_lib
    s = np.frombuffer(K.deflate(b"abc" * 50), dtype=np.uint8).copy()
    out = np.zeros(256, dtype=np.uint8)
    n = C.c_uint64(0)
    f = lib.vds_ec_inflate_host
    assert f(s.ctypes.data, s.size, out.ctypes.data, 256, None) == K.EINVAL
    assert f(None, s.size, out.ctypes.data, 256, C.byref(n)) == K.EINVAL
    assert f(s.ctypes.data, s.size, None, 256, C.byref(n)) == K.EINVAL
    assert f(s.ctypes.data, 1 << 32, out.ctypes.data, 256, C.byref(n)) == K.EINVAL
    assert f(s.ctypes.data, s.size, out.ctypes.data, 1 << 32, C.byref(n)) == K.EINVAL
    assert f(s.ctypes.data, s.size, s.ctypes.data + 5, 16, C.byref(n)) == K.EINVAL  # overlapping
    assert f(None, 0, None, 0, C.byref(n)) == K.EINFLATE_SHORT and n.value == 0

    one = lambda v: (C.c_void_p * 1)(v)
    u64 = lambda v: (C.c_uint64 * 1)(v)
    ip, op, ln, cp = one(s.ctypes.data), one(out.ctypes.data), u64(s.size), u64(256)
    ol32, ol64 = (C.c_uint32 * 1)(), (C.c_uint64 * 1)()
    st, failed = (C.c_int32 * 1)(), C.c_uint32(0)
    key, ident = np.zeros(32, dtype=np.uint32), np.zeros(32, dtype=np.uint8)
    a4 = lambda x: C.cast(x, C.c_void_p).value

    def inflate_dev(count=1, ip=ip, ln=ln, op=op, cp=cp, ol=a4(ol32), st=a4(st)):
        return lib.vds_ec_inflate_batch_device(count, ip, ln, op, cp, ol, st, None)

    def inflate_host(count=1, ip=ip, ln=ln, op=op, cp=cp, ol=ol64, st=st):
        return lib.vds_ec_inflate_host_batch(count, ip, ln, op, cp, ol, st, C.byref(failed))

    def unpack_dev(count=1, ip=ip, ln=ln, op=op, cp=cp, ol=a4(ol32), st=a4(st), keys=key.ctypes.data,
                   ids=ident.ctypes.data):
        return lib.vds_ec_block_unpack_batch_device(count, ip, ln, keys, ids, op, cp, ol, st, None)

    def unpack_host(count=1, ip=ip, ln=ln, op=op, cp=cp, ol=ol64, st=st, keys=key.ctypes.data,
                    ids=ident.ctypes.data):
        return lib.vds_ec_block_unpack_host_batch(count, ip, ln, keys, ids, op, cp, ol, st, C.byref(failed))

    for fn in (inflate_dev, inflate_host, unpack_dev, unpack_host):
        assert fn(count=0, ip=None, ln=None, op=None, cp=None, ol=None, st=None) == 0, fn.__name__  # count == 0 is OK
        assert fn(count=1 << 30) == K.EINVAL, fn.__name__
        for null in ("ip", "ln", "op", "cp", "ol", "st"):
            assert fn(**{null: None}) == K.EINVAL, (fn.__name__, null)
        assert fn(ip=one(None)) == K.EINVAL, fn.__name__                 # a null pointer with a non-zero size
        assert fn(op=one(None)) == K.EINVAL, fn.__name__
        assert fn(ln=u64(1 << 32)) == K.EINVAL, fn.__name__
        assert fn(cp=u64(1 << 32)) == K.EINVAL, fn.__name__
        assert fn(op=one(s.ctypes.data + s.size - 1), cp=u64(8)) == K.EINVAL, fn.__name__  # overlapping
    for fn in (unpack_dev, unpack_host):
        assert fn(keys=None) == K.EINVAL and fn(ids=None) == K.EINVAL, fn.__name__
    assert unpack_dev(keys=key.ctypes.data + 2) == K.EINVAL            # device keys: 4-byte aligned
    for fn in (inflate_dev, unpack_dev):
        assert fn(ol=a4(ol32) + 2) == K.EINVAL and fn(st=a4(st) + 2) == K.EINVAL, fn.__name__
