"""tests/golden/aes_cbc_kats.json (recorded from OpenSSL by
tests/golden/make_aes_kats.py) as the AES tests use it: inputs rebuilt from
their splitmix seeds, ciphertexts of the decrypt cases rebuilt and checked
against the recorded SHA-256 before any test trusts them."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np

import oracle_ctypes as O

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aes_cbc_kats.json")
ECRYPT_LENGTH, ECRYPT_PADDING, ECORRUPT, EINVAL = -18, -19, -10, -1


@functools.lru_cache(maxsize=None)
def kats() -> dict:
    with open(PATH) as f:
        return json.load(f)


def block_iv() -> bytes:
    return bytes.fromhex(kats()["block_iv"])


@functools.lru_cache(maxsize=None)
def sm(seed: int, n: int) -> bytes:
    return O.splitmix(seed, n).tobytes()


def matches(rec: dict, prefix: str, data: bytes) -> bool:
    """`data` is the output a record holds under `prefix` (hex up to 64 bytes, SHA-256 beyond)."""
    if len(data) != rec[prefix + "_len"]:
        return False
    if prefix + "_hex" in rec:
        return data.hex() == rec[prefix + "_hex"]
    return hashlib.sha256(data).hexdigest() == rec[prefix + "_sha256"]


def host_encrypt(lib, key: bytes, iv: bytes, data: bytes) -> bytes:
    out = np.zeros(len(data) // 16 * 16 + 16, dtype=np.uint8)
    assert lib.vds_ec_aes256_cbc_encrypt_host(key, iv, data, len(data), out.ctypes.data) == 0
    return out.tobytes()


def host_decrypt(lib, key: bytes, iv: bytes, ct: bytes):
    """(status, plaintext) of vds_ec_aes256_cbc_decrypt_host: the GPU tests' checker."""
    out = np.zeros(max(1, len(ct)), dtype=np.uint8)
    n = C.c_uint64(12345)
    rc = lib.vds_ec_aes256_cbc_decrypt_host(key, iv, ct, len(ct), out.ctypes.data, C.byref(n))
    if rc:
        assert n.value == 0
    return rc, out[:n.value].tobytes()


def decrypt_case(lib, rec: dict):
    """(key, iv or None, ciphertext) of a decrypt record; the ciphertext is the one OpenSSL was given."""
    key = bytes.fromhex(rec["key"])
    iv = bytes.fromhex(rec["iv"]) if rec["iv"] else None
    if "ct_hex" in rec:
        ct = bytes.fromhex(rec["ct_hex"])
    else:
        src = rec["from"]
        b = bytearray(host_encrypt(lib, key, iv or block_iv(), sm(src["seed"], src["len"]))[:rec["ct_len"]])
        for at, mask in src.get("flips", []):
            b[at] ^= mask
        ct = bytes(b)
    assert len(ct) == rec["ct_len"] and hashlib.sha256(ct).hexdigest() == rec["ct_sha256"], rec["name"]
    return key, iv, ct
