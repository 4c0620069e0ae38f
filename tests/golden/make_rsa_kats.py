"""Generate tests/golden/rsa_pkcs1_kats.json from the system's OpenSSL.

Run by hand (python tests/golden/make_rsa_kats.py), never by a test.  Every
key comes from libcrypto's EVP_PKEY keygen, every signature from
EVP_DigestSign(SHA-256) and every verdict from EVP_DigestVerify through ctypes
-- the calls the reference makes (asymmetric_sign / asymmetric_sign_verify,
kernel/vds_crypto/asymmetriccrypto.cpp:405-537) -- never from this project's
own arithmetic.  Blocks that only the comparison can reject are forged here
with the private exponent (Python's pow) and then judged by EVP_DigestVerify
like the rest.  No private key is written out: the file holds n and e, per case
the message as oracle_ctypes.splitmix(seed, len) with optional byte flips, the
signature bytes and libcrypto's verdict.
"""
import ctypes as C
import ctypes.util
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_ctypes as O  # noqa: E402

OUT = os.path.join(HERE, "rsa_pkcs1_kats.json")
LENGTHS = (0, 1, 55, 56, 64, 119, 4099)
LONG = 65537
EVP_PKEY_RSA = 6
DI_SHA256 = bytes.fromhex("3031300d060960864801650304020105000420")
DI_SHA256_NO_NULL = bytes.fromhex("302f300b0609608648016503040201" "0420")
DI_SHA1 = bytes.fromhex("3021300906052b0e03021a05000414")

_c = C.CDLL(ctypes.util.find_library("crypto"))
for name, res, args in (
        ("EVP_PKEY_CTX_new_id", C.c_void_p, [C.c_int, C.c_void_p]),
        ("EVP_PKEY_CTX_free", None, [C.c_void_p]),
        ("EVP_PKEY_keygen_init", C.c_int, [C.c_void_p]),
        ("EVP_PKEY_CTX_set_rsa_keygen_bits", C.c_int, [C.c_void_p, C.c_int]),
        ("EVP_PKEY_keygen", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
        ("EVP_PKEY_get_bn_param", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]),
        ("EVP_PKEY_free", None, [C.c_void_p]),
        ("BN_num_bits", C.c_int, [C.c_void_p]),
        ("BN_bn2bin", C.c_int, [C.c_void_p, C.c_char_p]),
        ("BN_free", None, [C.c_void_p]),
        ("EVP_MD_CTX_new", C.c_void_p, []),
        ("EVP_MD_CTX_free", None, [C.c_void_p]),
        ("EVP_sha256", C.c_void_p, []),
        ("EVP_DigestSignInit", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        ("EVP_DigestSign", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]),
        ("EVP_DigestVerifyInit", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        ("EVP_DigestVerify", C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]),
        ("ERR_clear_error", None, [])):
    f = getattr(_c, name)
    f.restype, f.argtypes = res, args


class Key:
    def __init__(self, bits: int):
        ctx = _c.EVP_PKEY_CTX_new_id(EVP_PKEY_RSA, None)
        assert ctx and _c.EVP_PKEY_keygen_init(ctx) == 1 and _c.EVP_PKEY_CTX_set_rsa_keygen_bits(ctx, bits) == 1
        p = C.c_void_p()
        assert _c.EVP_PKEY_keygen(ctx, C.byref(p)) == 1
        _c.EVP_PKEY_CTX_free(ctx)
        self.pkey = p
        self.n, self.e, self.d = (self._bn(x) for x in (b"n", b"e", b"d"))
        self.k = (self.n.bit_length() + 7) // 8
        assert self.n.bit_length() == bits

    def _bn(self, name: bytes) -> int:
        bn = C.c_void_p()
        assert _c.EVP_PKEY_get_bn_param(self.pkey, name, C.byref(bn)) == 1
        buf = C.create_string_buffer((_c.BN_num_bits(bn) + 7) // 8)
        n = _c.BN_bn2bin(bn, buf)
        _c.BN_free(bn)
        return int.from_bytes(buf.raw[:n], "big")

    def sign(self, msg: bytes) -> bytes:
        ctx = _c.EVP_MD_CTX_new()
        assert _c.EVP_DigestSignInit(ctx, None, _c.EVP_sha256(), None, self.pkey) == 1
        n = C.c_size_t(self.k)
        buf = C.create_string_buffer(self.k)
        assert _c.EVP_DigestSign(ctx, buf, C.byref(n), msg, len(msg)) == 1
        _c.EVP_MD_CTX_free(ctx)
        return buf.raw[:n.value]

    def verify(self, msg: bytes, sig: bytes) -> int:
        """EVP_DigestVerify's answer as the reference's bool: 1 only for its 1."""
        ctx = _c.EVP_MD_CTX_new()
        assert _c.EVP_DigestVerifyInit(ctx, None, _c.EVP_sha256(), None, self.pkey) == 1
        r = _c.EVP_DigestVerify(ctx, sig, len(sig), msg, len(msg))
        _c.ERR_clear_error()
        _c.EVP_MD_CTX_free(ctx)
        return 1 if r == 1 else 0

    def forge(self, em: bytes) -> bytes:
        v = int.from_bytes(em, "big")
        assert len(em) == self.k and v < self.n
        return pow(v, self.d, self.n).to_bytes(self.k, "big")


def sm(seed: int, n: int) -> bytes:
    return O.splitmix(seed, n).tobytes()


def main():
    keys = [Key(4096), Key(4096), Key(2048), Key(3072)]
    others = {0: keys[1], 1: keys[0], 2: Key(2048), 3: Key(3072)}  # another key of the same size
    cases = []

    def add(ki, name, seed, length, sig, flips=()):
        msg = bytearray(sm(seed, length))
        for at, mask in flips:
            msg[at] ^= mask
        v = keys[ki].verify(bytes(msg), sig)
        cases.append({"key": ki, "name": name, "seed": seed, "len": length, "flips": [list(f) for f in flips],
                      "sig": sig.hex(), "verdict": v})
        return v

    for ki, key in enumerate(keys):
        k, n = key.k, key.n
        base = 7000 + 100 * ki
        for i, length in enumerate(LENGTHS + ((LONG,) if ki == 0 else ())):
            assert add(ki, f"good, {length} bytes", base + i, length, key.sign(sm(base + i, length))) == 1
        seed, length = base + 20, 119
        msg = sm(seed, length)
        h = hashlib.sha256(msg).digest()
        good = key.sign(msg)
        s = int.from_bytes(good, "big")
        b = bytearray(good)
        b[k // 2] ^= 0x10
        assert add(ki, "one bit of the signature flipped", seed, length, bytes(b)) == 0
        assert add(ki, "one bit of the message flipped", seed, length, good, flips=[(60, 0x01)]) == 0
        assert add(ki, "signed by another key of the same size", seed, length, others[ki].sign(msg)) == 0
        for name, v in (("0", 0), ("1", 1), ("n-1", n - 1), ("n", n), ("s+n", s + n)):
            if v < 256 ** k:
                assert add(ki, "signature value " + name, seed, length, v.to_bytes(k, "big")) == 0
        # a good signature whose first byte is zero, then without it, and any good one behind a zero byte
        zs = next((t for t in range(base + 1000, base + 9000) if key.sign(sm(t, 32))[0] == 0), None)
        if zs is not None:
            z = key.sign(sm(zs, 32))
            assert add(ki, "good, first signature byte zero", zs, 32, z) == 1
            add(ki, "one byte short: the leading zero dropped", zs, 32, z[1:])
            add(ki, "one byte long: a zero in front of a leading zero", zs, 32, b"\x00" + z)
        add(ki, "one byte short: the first byte dropped", seed, length, good[1:])
        add(ki, "one byte long: a zero in front", seed, length, b"\x00" + good)
        # forged with the private exponent: only the comparison can reject them
        tail = DI_SHA256 + h
        ps = k - 3 - len(tail)
        forged = (
            ("the right block, forged (a check of the forging itself)", b"\x00\x01" + b"\xff" * ps + b"\x00" + tail),
            ("block type 02", b"\x00\x02" + b"\xff" * ps + b"\x00" + tail),
            ("first byte 01", b"\x01\x01" + b"\xff" * ps + b"\x00" + tail),
            ("eight FF, 00, DigestInfo, H and a garbage tail",
             b"\x00\x01" + b"\xff" * 8 + b"\x00" + tail + sm(seed + 1, ps - 8)),
            ("DigestInfo without the NULL parameter",
             b"\x00\x01" + b"\xff" * (ps + 2) + b"\x00" + DI_SHA256_NO_NULL + h),
            ("the SHA-1 DigestInfo",
             b"\x00\x01" + b"\xff" * (k - 3 - len(DI_SHA1) - 20) + b"\x00" + DI_SHA1 + hashlib.sha1(msg).digest()),
            ("the right frame around a wrong hash",
             b"\x00\x01" + b"\xff" * ps + b"\x00" + DI_SHA256 + hashlib.sha256(msg + b"x").digest()),
            ("no 00 separator", b"\x00\x01" + b"\xff" * (ps + 1) + tail),
        )
        for j, (name, em) in enumerate(forged):
            v = add(ki, "forged: " + name, seed, length, key.forge(em))
            assert v == (1 if j == 0 else 0), (ki, name, v)

    kats = {"source": "libcrypto EVP_PKEY keygen, EVP_DigestSign, EVP_DigestVerify via ctypes "
                      "(tests/golden/make_rsa_kats.py)",
            "keys": [{"bits": key.n.bit_length(), "n": "%x" % key.n, "e": "%x" % key.e} for key in keys],
            "cases": cases}
    with open(OUT, "w") as f:
        json.dump(kats, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes;", len(cases), "cases;",
          sum(c["verdict"] for c in cases), "of them verify")
    for c in cases:
        print(c["key"], c["verdict"], c["name"])


if __name__ == "__main__":
    main()
