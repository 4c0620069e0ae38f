"""What the RSA tests share: the libcrypto fixture, the moduli and operands of
the raw operation, the expected PKCS#1 encoding, signing keys of the tests' own
and a serializer for transaction-log blocks.  Nothing here touches the library
under test: Python integers decide every value."""
from __future__ import annotations

import hashlib
import json
import os
import random

import oracle_ctypes as O

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "rsa_pkcs1_kats.json")
DI_SHA256 = bytes.fromhex("3031300d060960864801650304020105000420")
EXPONENTS = (3, 17, 65537, 2 ** 32 - 1)

_kats = None


def kats() -> dict:
    global _kats
    if _kats is None:
        with open(FIXTURE) as f:
            k = json.load(f)
        for key in k["keys"]:
            key["n"], key["e"] = int(key["n"], 16), int(key["e"], 16)
        for c in k["cases"]:
            m = bytearray(O.splitmix(c["seed"], c["len"]).tobytes())
            for at, mask in c["flips"]:
                m[at] ^= mask
            c["msg"], c["sig"] = bytes(m), bytes.fromhex(c["sig"])
        _kats = k
    return _kats


def moduli() -> list:
    """The fixture's keys, then odd numbers that are no RSA moduli and give the
    longest carry runs."""
    r = random.Random(41)
    low_ones = (r.getrandbits(4096) | (1 << 4095) | ((1 << 1024) - 1))
    return [k["n"] for k in kats()["keys"]] + [2 ** 4096 - 1, 2 ** 4095 + 1, 2 ** 2048 - 1, low_ones,
                                                r.getrandbits(520) | (1 << 519) | 1]


def operands(n: int, seed: int) -> list:
    r = random.Random(seed)
    return [r.randrange(n), r.randrange(n), 0, 1, n - 1, 1 << (n.bit_length() - 1)]


def n_bytes(n: int) -> int:
    return (n.bit_length() + 7) // 8


def em_sha256(digest: bytes, k: int) -> bytes:
    """EMSA-PKCS1-v1_5 (RFC 8017 9.2) of a SHA-256 digest for a modulus of k bytes."""
    t = DI_SHA256 + digest
    return b"\x00\x01" + b"\xff" * (k - 3 - len(t)) + b"\x00" + t


def fingerprint(n: int, e: int) -> bytes:
    """asymmetriccrypto.cpp:657-681 restated: BN_bn2hex gives an even number of
    uppercase hex digits, a "00" goes in front where the first is above '8'."""
    def mag(v):
        h = "%X" % v
        if len(h) % 2:
            h = "0" + h
        if h[0] > "8":
            h = "00" + h
        return bytes.fromhex(h)
    rec = (7).to_bytes(4, "big") + b"ssh-rsa"
    for v in (e, n):
        rec += len(mag(v)).to_bytes(4, "big") + mag(v)
    return hashlib.sha256(rec).digest()


# ------------------------------------------------------------ signing keys
_SMALL = [p for p in range(3, 2000, 2) if all(p % q for q in range(3, int(p ** 0.5) + 1, 2))]


def _prime(bits: int, r: random.Random) -> int:
    while True:
        c = r.getrandbits(bits) | (3 << (bits - 2)) | 1
        if all(c % p for p in _SMALL) and pow(2, c - 1, c) == 1 and all(
                pow(a, c - 1, c) == 1 for a in (3, 5, 7)) and c % 65537 != 1:
            return c


_signers = {}


class Signer:
    """An RSA key of the tests' own, seeded: (n, e = 65537) and a CRT signer."""

    def __init__(self, bits: int, seed: int):
        r = random.Random(seed)
        self.p, self.q = _prime(bits // 2, r), _prime(bits // 2, r)
        self.n, self.e = self.p * self.q, 65537
        assert self.n.bit_length() == bits
        self.dp, self.dq = pow(self.e, -1, self.p - 1), pow(self.e, -1, self.q - 1)
        self.qinv = pow(self.q, -1, self.p)
        self.k = n_bytes(self.n)

    def raw(self, v: int) -> int:
        a, b = pow(v % self.p, self.dp, self.p), pow(v % self.q, self.dq, self.q)
        return b + self.q * ((a - b) * self.qinv % self.p)

    def sign(self, msg: bytes) -> bytes:
        em = int.from_bytes(em_sha256(hashlib.sha256(msg).digest(), self.k), "big")
        s = self.raw(em)
        assert pow(s, self.e, self.n) == em
        return s.to_bytes(self.k, "big")


def signer(bits: int, seed: int) -> Signer:
    if (bits, seed) not in _signers:
        _signers[bits, seed] = Signer(bits, seed)
    return _signers[bits, seed]


# ------------------------------------------------------ transaction blocks
VERSION = 0x31564453


def number(v: int) -> bytes:
    """binary_serializer::write_number (binary_serialize.cpp:44-66)"""
    if v < 128:
        return bytes([v])
    v -= 128
    b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
    return bytes([0x80 | len(b)]) + b


def buffer(b: bytes) -> bytes:
    return number(len(b)) + b


def block_prefix(time_point: int, order_no: int, key_id: bytes, ancestors, messages: bytes, version=VERSION,
                 sort=True) -> bytes:
    """What transaction_block::build signs (transaction_block.cpp:83-89): the
    ancestors in std::set order, const_data_buffer::operator< (size, then bytes)."""
    anc = sorted(set(ancestors), key=lambda a: (len(a), a)) if sort else list(ancestors)
    return (version.to_bytes(4, "big") + time_point.to_bytes(8, "big") + order_no.to_bytes(8, "big") + buffer(key_id) +
            number(len(anc)) + b"".join(buffer(a) for a in anc) + buffer(messages))


def block(prefix: bytes, signature: bytes) -> bytes:
    return prefix + buffer(signature)
