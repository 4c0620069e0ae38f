"""AES-256-CBC on the host (aes_host.cpp: vds_ec_aes256_cbc_*_host,
vds_ec_aes256_cbc_padded_size, vds_ec_block_iv) and the argument checks of the
batch entries, none of which needs a GPU.

The references are OpenSSL's recorded answers (tests/golden/aes_cbc_kats.json,
tests/aes_kats.py) and, where it loads, the live libcrypto.  Bit-exact."""
import ctypes as C
import ctypes.util
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import aes_kats as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECRYPT_LENGTH, ECRYPT_PADDING = K.EINVAL, K.ECRYPT_LENGTH, K.ECRYPT_PADDING


def test_padded_size_edges(vds_lib):
    f = vds_lib.vds_ec_aes256_cbc_padded_size
    assert [f(n) for n in (0, 1, 15, 16, 17, 31, 32, 65535, 65536)] == [16, 16, 16, 32, 32, 32, 48, 65536, 65552]
    assert f(0xFFFFFFFF) == 0x100000000 and f(0xFFFFFFF0) == 0x100000000 and f(0xFFFFFFEF) == 0xFFFFFFF0
    assert f((1 << 40) + 5) == (1 << 40) + 16


def test_block_iv_and_statuses(vds_lib):
    from vds_amd import _lib, chunk
    assert chunk.block_iv() == K.block_iv() == bytes.fromhex("a5bb9fcec2e44b91a8c9594462559024")
    assert vds_lib.vds_ec_block_iv(None) == EINVAL
    assert (_lib.ECRYPT_LENGTH, _lib.ECRYPT_PADDING) == (ECRYPT_LENGTH, ECRYPT_PADDING)
    for st in (ECRYPT_LENGTH, ECRYPT_PADDING):  # the reference's text for both
        assert b"EVP_CipherFinal_ex failed" in vds_lib.vds_ec_strerror(st)
    assert vds_lib.vds_ec_strerror(ECRYPT_LENGTH) != vds_lib.vds_ec_strerror(ECRYPT_PADDING)
    assert vds_lib.vds_ec_version() >= 101


def test_sp800_38a(vds_lib):
    r = K.kats()["sp800_38a"]
    key, iv, pt = (bytes.fromhex(r[x]) for x in ("key", "iv", "plaintext_hex"))
    ct = K.host_encrypt(vds_lib, key, iv, pt)
    assert ct[:16].hex() == "f58c4c04d6e5f1ba779eabfb5f7bfbd6"
    assert ct[:64].hex() == r["blocks_hex"] and ct.hex() == r["padded_hex"]
    assert K.host_decrypt(vds_lib, key, iv, ct) == (0, pt)


def test_encrypt_records(vds_lib):
    for r in K.kats()["encrypt"]:
        key = bytes.fromhex(r["key"])
        iv = bytes.fromhex(r["iv"]) if r["iv"] else K.block_iv()
        pt = K.sm(r["seed"], r["len"])
        ct = K.host_encrypt(vds_lib, key, iv, pt)
        assert K.matches(r, "out", ct), r["len"]
        assert K.host_decrypt(vds_lib, key, iv, ct) == (0, pt), r["len"]


def test_decrypt_records(vds_lib):
    seen = set()
    for r in K.kats()["decrypt"]:
        key, iv, ct = K.decrypt_case(vds_lib, r)
        st, out = K.host_decrypt(vds_lib, key, iv or K.block_iv(), ct)
        assert st == r["status"], r["name"]
        assert len(out) == r["out_len"], r["name"]
        if st == 0:
            assert K.matches(r, "out", out), r["name"]
        seen.add((st, "tampered" in r["name"]))
    # the fixture says which tampered ciphertexts fail and which still unpad: both kinds are there
    assert {(0, True), (ECRYPT_PADDING, True), (0, False), (ECRYPT_LENGTH, False)} <= seen


def test_pack_records_by_host_composition(vds_lib):
    """client::save in three lines of host calls against OpenSSL's records."""
    for r in K.kats()["pack"]:
        data, zipped = K.sm(r["data_seed"], r["data_len"]), K.sm(r["zipped_seed"], r["zipped_len"])
        bid = hashlib.sha256(data).digest()
        key = hashlib.sha256(K.host_encrypt(vds_lib, bid, K.block_iv(), data)).digest()
        crypted = K.host_encrypt(vds_lib, key, K.block_iv(), zipped)
        assert bid.hex() == r["id"] and key.hex() == r["key"] and K.matches(r, "crypted", crypted), r["data_len"]


def _pad_case(vds_lib, key, iv, blocks: bytes):
    """Decrypt status and length of the ciphertext whose plaintext blocks are `blocks` (CBC built by hand
    from single-block encryptions: encrypt(x)[:16] is the block cipher on x ^ iv)."""
    ct, prev = b"", iv
    for i in range(0, len(blocks), 16):
        prev = K.host_encrypt(vds_lib, key, prev, blocks[i:i + 16])[:16]
        ct += prev
    st, out = K.host_decrypt(vds_lib, key, iv, ct)
    if st == 0:
        assert out == blocks[:len(out)]
    return st, len(out)


def test_decrypt_statuses(vds_lib):
    rng = random.Random(5)
    key, iv, body = rng.randbytes(32), rng.randbytes(16), rng.randbytes(16)
    assert K.host_decrypt(vds_lib, key, iv, b"") == (ECRYPT_LENGTH, b"")
    assert K.host_decrypt(vds_lib, key, iv, rng.randbytes(17)) == (ECRYPT_LENGTH, b"")
    assert _pad_case(vds_lib, key, iv, body + bytes(16)) == (ECRYPT_PADDING, 0)            # pad byte 0x00
    assert _pad_case(vds_lib, key, iv, body + bytes([0x11]) * 16) == (ECRYPT_PADDING, 0)   # pad byte 0x11
    for w, v in ((0, 2), (1, 2), (2, 4)):  # pad 3 with one of the three bytes wrong
        tail = bytearray([3, 3, 3])
        tail[w] = v
        assert _pad_case(vds_lib, key, iv, body + rng.randbytes(13) + bytes(tail)) == (ECRYPT_PADDING, 0), w
    assert _pad_case(vds_lib, key, iv, body + rng.randbytes(13) + b"\x03\x03\x03") == (0, 29)
    assert _pad_case(vds_lib, key, iv, bytes([16]) * 16) == (0, 0)  # a whole block of 0x10: an empty message
    assert _pad_case(vds_lib, key, iv, body + bytes([16]) * 16) == (0, 16)
    # null arguments
    n = C.c_uint64(0)
    buf = np.zeros(32, dtype=np.uint8)
    assert vds_lib.vds_ec_aes256_cbc_encrypt_host(None, iv, body, 16, buf.ctypes.data) == EINVAL
    assert vds_lib.vds_ec_aes256_cbc_encrypt_host(key, None, body, 16, buf.ctypes.data) == EINVAL
    assert vds_lib.vds_ec_aes256_cbc_encrypt_host(key, iv, None, 16, buf.ctypes.data) == EINVAL
    assert vds_lib.vds_ec_aes256_cbc_encrypt_host(key, iv, body, 16, None) == EINVAL
    assert vds_lib.vds_ec_aes256_cbc_decrypt_host(key, iv, body, 16, buf.ctypes.data, None) == EINVAL
    assert vds_lib.vds_ec_aes256_cbc_decrypt_host(key, iv, None, 16, buf.ctypes.data, C.byref(n)) == EINVAL
    assert vds_lib.vds_ec_aes256_cbc_decrypt_host(key, iv, body, 16, None, C.byref(n)) == EINVAL


def test_in_place(vds_lib):
    rng = random.Random(6)
    key, iv = rng.randbytes(32), rng.randbytes(16)
    for n in (0, 5, 16, 100, 4096):
        pt = rng.randbytes(n)
        ref = K.host_encrypt(vds_lib, key, iv, pt)
        buf = np.zeros(n + 16, dtype=np.uint8)
        buf[:n] = np.frombuffer(pt, dtype=np.uint8)
        assert vds_lib.vds_ec_aes256_cbc_encrypt_host(key, iv, buf.ctypes.data, n, buf.ctypes.data) == 0
        assert buf[:len(ref)].tobytes() == ref
        m = C.c_uint64(0)
        assert vds_lib.vds_ec_aes256_cbc_decrypt_host(key, iv, buf.ctypes.data, len(ref), buf.ctypes.data,
                                                      C.byref(m)) == 0
        assert m.value == n and buf[:n].tobytes() == pt


def _libcrypto():
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = C.CDLL(name)
        lib.EVP_aes_256_cbc.restype = C.c_void_p
        lib.EVP_CIPHER_CTX_new.restype = C.c_void_p
        lib.EVP_CIPHER_CTX_free.argtypes = [C.c_void_p]
        lib.EVP_CipherInit_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_int]
        lib.EVP_CipherUpdate.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
        lib.EVP_CipherFinal_ex.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        return lib
    except (OSError, AttributeError):
        return None


def _evp(lib, key, iv, data, enc):
    ctx = lib.EVP_CIPHER_CTX_new()
    try:
        assert lib.EVP_CipherInit_ex(ctx, lib.EVP_aes_256_cbc(), None, key, iv, 1 if enc else 0) == 1
        buf = C.create_string_buffer(len(data) + 32)
        n, m = C.c_int(0), C.c_int(0)
        assert lib.EVP_CipherUpdate(ctx, buf, C.byref(n), data, len(data)) == 1
        if lib.EVP_CipherFinal_ex(ctx, C.byref(buf, n.value), C.byref(m)) != 1:
            return None
        return buf.raw[:n.value + m.value]
    finally:
        lib.EVP_CIPHER_CTX_free(ctx)


def test_against_live_libcrypto(vds_lib):
    lib = _libcrypto()
    if lib is None:
        pytest.skip("no libcrypto loads through ctypes here: the recorded OpenSSL answers "
                    "(tests/golden/aes_cbc_kats.json) are the reference on this machine")
    rng = random.Random(7)
    for i in range(200):
        key, iv, pt = rng.randbytes(32), rng.randbytes(16), rng.randbytes(rng.randrange(301))
        ct = _evp(lib, key, iv, pt, True)
        assert K.host_encrypt(vds_lib, key, iv, pt) == ct, i
        assert K.host_decrypt(vds_lib, key, iv, ct) == (0, pt), i
        # and a damaged ciphertext: the same verdict, and the same bytes where it still unpads
        bad = bytearray(ct)
        bad[rng.randrange(len(bad))] ^= 1 << rng.randrange(8)
        ref = _evp(lib, key, iv, bytes(bad), False)
        st, out = K.host_decrypt(vds_lib, key, iv, bytes(bad))
        assert (st, out) == ((ECRYPT_PADDING, b"") if ref is None else (0, ref)), i


_CHILD = r"""
import hashlib, random, sys
sys.path[:0] = [%r, %r]
import aes_kats as K
from vds_amd import build, _lib
build.build()
lib = _lib.lib()
rng = random.Random(8)
h = hashlib.sha256()
for i in range(120):
    key, iv, pt = rng.randbytes(32), rng.randbytes(16), rng.randbytes(rng.choice((0, 1, 15, 16, 17, 255, 4096, 5000)))
    ct = K.host_encrypt(lib, key, iv, pt)
    assert K.host_decrypt(lib, key, iv, ct) == (0, pt)
    bad = bytearray(ct)
    bad[-1 - rng.randrange(min(len(bad), 32))] ^= 1 + rng.randrange(255)
    st, out = K.host_decrypt(lib, key, iv, bytes(bad))
    h.update(ct + st.to_bytes(4, "little", signed=True) + out)
print(h.hexdigest())
"""


def test_portable_and_aesni_paths_agree(vds_lib):
    """The implementation is picked at first use from VDS_EC_AES_HOST, so each arm runs in a child
    process; on a CPU without AES-NI both arms are the portable code and agree trivially."""
    digests = []
    for mode in ("", "portable"):
        env = dict(os.environ, VDS_EC_AES_HOST=mode)
        r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        digests.append(r.stdout.strip().splitlines()[-1])
    assert digests[0] == digests[1] and len(digests[0]) == 64
    # the portable arm, in this process's terms: the fixture test above pins whichever arm runs here


def _tables(count, ptr=0x1000, length=16):
    p = (C.c_void_p * max(1, count))(*[ptr + 0x100000 * i for i in range(count)])
    ln = (C.c_uint64 * max(1, count))(*[length] * count)
    return p, ln


def test_batch_entries_validate_before_the_device(vds_lib):
    """Every EINVAL below comes back on a machine with no GPU: the arguments are checked before the
    device is looked for.  The pointers are never dereferenced."""
    from vds_amd import _lib
    L = vds_lib
    dev = 0x7000000  # stands for device memory, 4-byte aligned
    ins, lens = _tables(2)
    outs, _ = _tables(2, ptr=0x90000000)
    enc = L.vds_ec_aes256_cbc_encrypt_batch_device
    dec = L.vds_ec_aes256_cbc_decrypt_batch_device
    assert enc(0, None, None, None, None, None, None) == 0
    assert dec(0, None, None, None, None, None, None, None, None) == 0
    assert enc(1 << 30, ins, lens, dev, None, outs, None) == EINVAL
    assert dec(1 << 30, ins, lens, dev, None, outs, dev, dev, None) == EINVAL
    for bad in range(4):  # null arrays
        a = [ins, lens, dev, outs]
        a[bad] = None
        assert enc(2, a[0], a[1], a[2], None, a[3], None) == EINVAL, bad
        assert dec(2, a[0], a[1], a[2], None, a[3], dev, dev, None) == EINVAL, bad
    assert dec(2, ins, lens, dev, None, outs, None, dev, None) == EINVAL
    assert dec(2, ins, lens, dev, None, outs, dev, None, None) == EINVAL
    assert enc(2, ins, lens, dev + 2, None, outs, None) == EINVAL  # keys 4-byte aligned
    # a null pointer with a non-zero length; an output is never empty for the encrypt
    nul = (C.c_void_p * 2)(0x1000, None)
    assert enc(2, nul, lens, dev, None, outs, None) == EINVAL
    assert enc(2, ins, lens, dev, None, nul, None) == EINVAL
    zero = (C.c_uint64 * 2)(16, 0)
    assert enc(2, ins, zero, dev, None, nul, None) == EINVAL
    assert dec(2, nul, lens, dev, None, outs, dev, dev, None) == EINVAL
    assert dec(2, ins, lens, dev, None, nul, dev, dev, None) == EINVAL
    big = (C.c_uint64 * 2)(16, 1 << 32)
    assert enc(2, ins, big, dev, None, outs, None) == EINVAL
    assert dec(2, ins, big, dev, None, outs, dev, dev, None) == EINVAL
    # an input and output of one message that overlap: the padded output reaches the input, or lies inside it
    for delta in (0, 8, 31, -16, -31):
        ov = (C.c_void_p * 2)(0x90000000, 0x1000 + 0x100000 + delta)
        l32 = (C.c_uint64 * 2)(32, 32)
        assert enc(2, ins, l32, dev, None, ov, None) == EINVAL, delta
        assert dec(2, ins, l32, dev, None, ov, dev, dev, None) == EINVAL, delta
    # the pack: the same, for both inputs
    pack = L.vds_ec_block_pack_batch_device
    hpack = L.vds_ec_block_pack_host_batch
    z, zl = _tables(2, ptr=0x40000000)
    assert pack(0, None, None, None, None, None, None, None, None) == 0
    assert hpack(0, None, None, None, None, None, None, None, None) == 0
    for f, tail in ((pack, (None,)), (hpack, (None,))):
        assert f(1 << 30, ins, lens, z, zl, dev, dev + 64, outs, *tail) == EINVAL
        for bad in range(7):
            a = [ins, lens, z, zl, dev, dev + 64, outs]
            a[bad] = None
            assert f(2, *a, *tail) == EINVAL, bad
        assert f(2, nul, lens, z, zl, dev, dev + 64, outs, *tail) == EINVAL
        assert f(2, ins, lens, nul, zl, dev, dev + 64, outs, *tail) == EINVAL
        assert f(2, ins, lens, z, zl, dev, dev + 64, nul, *tail) == EINVAL
        assert f(2, ins, big, z, zl, dev, dev + 64, outs, *tail) == EINVAL
        assert f(2, ins, lens, z, big, dev, dev + 64, outs, *tail) == EINVAL
        ov = (C.c_void_p * 2)(0x90000000, 0x40000000 + 0x100000 + 8)
        assert f(2, ins, lens, z, zl, dev, dev + 64, ov, *tail) == EINVAL  # crypted over zipped
        ov = (C.c_void_p * 2)(0x90000000, 0x1000 + 0x100000 - 8)
        assert f(2, ins, lens, z, zl, dev, dev + 64, ov, *tail) == EINVAL  # crypted over data
    assert pack(2, ins, lens, z, zl, dev + 1, dev + 64, outs, None) == EINVAL
    # the host decrypt batch
    hdec = L.vds_ec_aes256_cbc_decrypt_host_batch
    ol = (C.c_uint64 * 2)()
    st = (C.c_int32 * 2)()
    assert hdec(0, None, None, None, None, None, None, None, None) == 0
    assert hdec(1 << 30, ins, lens, dev, None, outs, ol, st, None) == EINVAL
    for bad in range(6):
        a = [ins, lens, dev, outs, ol, st]
        a[bad] = None
        assert hdec(2, a[0], a[1], a[2], None, a[3], a[4], a[5], None) == EINVAL, bad
    assert hdec(2, nul, lens, dev, None, outs, ol, st, None) == EINVAL
    assert hdec(2, ins, lens, dev, None, nul, ol, st, None) == EINVAL
    assert hdec(2, ins, big, dev, None, outs, ol, st, None) == EINVAL
    ov = (C.c_void_p * 2)(0x90000000, 0x1000 + 0x100000 + 8)
    assert hdec(2, ins, lens, dev, None, ov, ol, st, None) == EINVAL
    assert _lib.EINVAL == EINVAL


def test_chunk_wrappers_on_the_host(vds_lib):
    from vds_amd import chunk, VdsEcError
    r = K.kats()["encrypt"][4]
    key, pt = bytes.fromhex(r["key"]), K.sm(r["seed"], r["len"])
    iv = bytes.fromhex(r["iv"]) if r["iv"] else None
    ct = chunk.aes256_cbc_encrypt_host(key, pt, iv)
    assert K.matches(r, "out", ct) and chunk.aes256_cbc_decrypt_host(key, ct, iv) == pt
    assert chunk.aes256_cbc_padded_size(len(pt)) == len(ct)
    with pytest.raises(VdsEcError) as e:
        chunk.aes256_cbc_decrypt_host(key, ct[:-1], iv)
    assert e.value.status == ECRYPT_LENGTH
    with pytest.raises(VdsEcError) as e:
        chunk.aes256_cbc_decrypt_host(key, b"", iv)
    assert e.value.status == ECRYPT_LENGTH
    with pytest.raises(VdsEcError) as e:
        chunk.aes256_cbc_encrypt_host(key[:31], pt, iv)
    assert e.value.status == EINVAL
