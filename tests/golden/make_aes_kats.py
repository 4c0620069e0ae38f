"""Generate tests/golden/aes_cbc_kats.json from the system's OpenSSL.

Run by hand (python tests/golden/make_aes_kats.py), never by a test.  Every
record comes from libcrypto's EVP_aes_256_cbc through ctypes -- the library and
the calls the reference makes (symmetric_encrypt / symmetric_decrypt,
private/symmetriccrypto_p.h: EVP_CipherInit_ex, EVP_CipherUpdate,
EVP_CipherFinal_ex with the default PKCS#7 padding) -- never from this
project's own cipher.  Inputs are oracle_ctypes.splitmix(seed, len), so the
file holds seeds, lengths, keys and ivs, the outputs as hex up to 64 bytes and
as a SHA-256 beyond, and for decrypt cases the status OpenSSL gave
(0, -18 "wrong final block length", -19 "bad decrypt") and the output length.

Padding is not authentication: a tampered ciphertext may still unpad.  Which
tampered cases fail and which pass is what OpenSSL said, recorded here.
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

OUT = os.path.join(HERE, "aes_cbc_kats.json")
BLOCK_IV = bytes.fromhex("a5bb9fcec2e44b91a8c9594462559024")  # pack_block_iv, dht_network_client.cpp:1101-1105
ECRYPT_LENGTH, ECRYPT_PADDING = -18, -19

_crypto = C.CDLL(ctypes.util.find_library("crypto"))
_crypto.EVP_CIPHER_CTX_new.restype = C.c_void_p
_crypto.EVP_aes_256_cbc.restype = C.c_void_p
_crypto.EVP_CIPHER_CTX_free.argtypes = [C.c_void_p]
_crypto.EVP_CipherInit_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_int]
_crypto.EVP_CIPHER_CTX_set_padding.argtypes = [C.c_void_p, C.c_int]
_crypto.EVP_CipherUpdate.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
_crypto.EVP_CipherFinal_ex.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
_crypto.ERR_peek_last_error.restype = C.c_ulong
_crypto.ERR_reason_error_string.restype = C.c_char_p
_crypto.ERR_reason_error_string.argtypes = [C.c_ulong]


def evp(key: bytes, iv: bytes, data: bytes, enc: bool, padding: bool = True):
    """(status, output) of one EVP_aes_256_cbc pass as the reference runs it."""
    ctx = _crypto.EVP_CIPHER_CTX_new()
    try:
        assert _crypto.EVP_CipherInit_ex(ctx, _crypto.EVP_aes_256_cbc(), None, key, iv, 1 if enc else 0) == 1
        if not padding:
            _crypto.EVP_CIPHER_CTX_set_padding(ctx, 0)
        buf = C.create_string_buffer(len(data) + 32)
        n = C.c_int(0)
        assert _crypto.EVP_CipherUpdate(ctx, buf, C.byref(n), data, len(data)) == 1
        m = C.c_int(0)
        _crypto.ERR_clear_error()
        if _crypto.EVP_CipherFinal_ex(ctx, C.byref(buf, n.value), C.byref(m)) != 1:
            why = (_crypto.ERR_reason_error_string(_crypto.ERR_peek_last_error()) or b"").decode()
            if "wrong final block length" in why:
                return ECRYPT_LENGTH, b""
            assert "bad decrypt" in why, why
            return ECRYPT_PADDING, b""
        return 0, buf.raw[:n.value + m.value]
    finally:
        _crypto.EVP_CIPHER_CTX_free(ctx)


def out_fields(prefix: str, data: bytes) -> dict:
    d = {prefix + "_len": len(data)}
    if len(data) <= 64:
        d[prefix + "_hex"] = data.hex()
    else:
        d[prefix + "_sha256"] = hashlib.sha256(data).hexdigest()
    return d


def sm(seed: int, n: int) -> bytes:
    return O.splitmix(seed, n).tobytes()


def main():
    kats = {"block_iv": BLOCK_IV.hex(), "source": "libcrypto EVP_aes_256_cbc via ctypes (tests/golden/make_aes_kats.py)"}

    # SP 800-38A F.2.5 / F.2.6, CBC-AES256: the four blocks, checked against the standard's text
    key = bytes.fromhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4")
    iv = bytes.fromhex("000102030405060708090a0b0c0d0e0f")
    pt = bytes.fromhex("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e51"
                       "30c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710")
    st, ct = evp(key, iv, pt, True)
    assert st == 0 and len(ct) == 80
    assert ct[:64].hex() == ("f58c4c04d6e5f1ba779eabfb5f7bfbd69cfc4e967edb808d679f777bc6702c7d"
                             "39f23369a9d9bacfa530e26304231461b2eb05e2c39be9fcda6c19078c6a9d1b")
    kats["sp800_38a"] = {"key": key.hex(), "iv": iv.hex(), "plaintext_hex": pt.hex(), "blocks_hex": ct[:64].hex(),
                         "padded_hex": ct.hex()}

    # encrypt: splitmix inputs, per-record keys, with an iv of their own or pack_block_iv (iv null)
    enc = []
    for i, n in enumerate((0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 255, 256, 257, 4095, 4096, 65536, 65537)):
        key = sm(1000 + i, 32)
        iv = None if i % 3 == 0 else sm(2000 + i, 16)
        st, ct = evp(key, iv or BLOCK_IV, sm(3000 + i, n), True)
        assert st == 0 and len(ct) == (n // 16 + 1) * 16
        enc.append({"seed": 3000 + i, "len": n, "key": key.hex(), "iv": iv.hex() if iv else None, **out_fields("out", ct)})
    kats["encrypt"] = enc

    # decrypt: ciphertexts given in full (built block by block without padding), or as a recorded
    # encryption with a length cut and bytes flipped; status and output as OpenSSL gave them
    dec = []

    def add(name, key, iv, ct=None, src=None):
        if src is not None:
            st, whole = evp(key, iv or BLOCK_IV, sm(src["seed"], src["len"]), True)
            assert st == 0
            b = bytearray(whole[:src.get("ct_len", len(whole))])
            for at, mask in src.get("flips", []):
                b[at] ^= mask
            ct = bytes(b)
        st, out = evp(key, iv or BLOCK_IV, ct, False)
        r = {"name": name, "key": key.hex(), "iv": iv.hex() if iv else None}
        if src is not None:
            r["from"] = src
        else:
            r["ct_hex"] = ct.hex()
        r["ct_len"] = len(ct)
        r["ct_sha256"] = hashlib.sha256(ct).hexdigest()
        r["status"] = st
        r.update(out_fields("out", out) if st == 0 else {"out_len": 0})
        dec.append(r)
        return st

    key, iv = sm(4000, 32), sm(4001, 16)

    def raw(blocks: bytes) -> bytes:  # the ciphertext of exactly these plaintext blocks
        st, ct = evp(key, iv, blocks, True, padding=False)
        assert st == 0 and len(ct) == len(blocks)
        return ct

    body = sm(4002, 16)
    assert add("length 0", key, iv, ct=b"") == ECRYPT_LENGTH
    assert add("length 17", key, iv, ct=raw(body + bytes([16]) * 16)[:17]) == ECRYPT_LENGTH
    assert add("length 40", key, iv, ct=raw(body * 3)[:40]) == ECRYPT_LENGTH
    assert add("pad byte 0x00", key, iv, ct=raw(body + bytes(16))) == ECRYPT_PADDING
    assert add("pad byte 0x11", key, iv, ct=raw(body + bytes([0x11]) * 16)) == ECRYPT_PADDING
    for w in range(3):
        tail = bytearray([3, 3, 3])
        tail[w] = 2 if w < 2 else 4
        assert add(f"pad 3, byte {w} of the three wrong", key, iv, ct=raw(body + sm(4003, 13) + bytes(tail))) != 0
    assert add("a whole block of 0x10: out_len 0", key, iv, ct=raw(bytes([16]) * 16)) == 0
    assert add("two blocks, whole pad block", key, iv, ct=raw(body + bytes([16]) * 16)) == 0
    assert add("pad 1", key, iv, ct=raw(sm(4004, 15) + b"\x01")) == 0
    assert add("pad 15", key, iv, ct=raw(b"\x77" + bytes([15]) * 15)) == 0
    assert add("pad 16 with a wrong first byte", key, iv, ct=raw(b"\x0f" + bytes([16]) * 15)) == ECRYPT_PADDING
    # tampered ciphertexts of good messages: padding is no authentication, so OpenSSL's answer is recorded
    statuses = []
    for j, (n, flips) in enumerate((
            (30, [[31, 0x01]]),            # last ciphertext byte: the pad byte itself changes
            (30, [[15, 0x02 ^ 0x01]]),     # the byte before the last block's pad byte: pad 2 -> a valid pad 1
            (30, [[0, 0x80]]),             # first block: garbles data only, the padding still holds
            (30, [[16, 0x40]]),            # last block's first byte: garbles the whole last block
            (100, [[95, 0xFF]]),           # the block before the last: flips the pad byte 12 -> 0xF3
            (100, [[50, 0x10]]),           # the middle: data only
            (4096, [[4095, 0x01]]),        # second last block's last byte: whole pad block's last byte 0x10 -> 0x11
            (4096, [[4111, 0x20]]),        # the pad block itself
            (4096, [[7, 0x04], [2000, 0x08]]),
            (65536, [[65551, 0x01]]),
            (65536, [[32768, 0x01]]),
            (65536, [[65535, 0x10 ^ 0x01]]),  # whole pad block's last byte 0x10 -> 0x01: unpads to 65551 bytes
    )):
        k2 = sm(4100 + j, 32)
        iv2 = None if j % 2 else sm(4200 + j, 16)
        statuses.append(add(f"tampered {n} {flips}", k2, iv2, src={"seed": 4300 + j, "len": n, "flips": flips}))
        statuses.append(add(f"untampered {n}", k2, iv2, src={"seed": 4300 + j, "len": n}))
    assert 0 in statuses and ECRYPT_PADDING in statuses
    assert add("cut to 4096 of 4112", sm(4400, 32), None, src={"seed": 4401, "len": 4096, "ct_len": 4096}) in (0, -19)
    assert add("cut to 4100 of 4112", sm(4400, 32), None,
               src={"seed": 4401, "len": 4096, "ct_len": 4100}) == ECRYPT_LENGTH
    kats["decrypt"] = dec

    # pack (client::save): id = SHA-256(data), key = SHA-256(AES(id, iv, data)), crypted = AES(key, iv, zipped);
    # zipped is given as splitmix bytes (the call does not look inside it)
    pack = []
    for i, n in enumerate((0, 1, 15, 16, 17, 4096, 65536)):
        data = sm(5000 + i, n)
        zlen = (0, 9, 16, 23, 32, 1500, 40000)[i]
        zipped = sm(5100 + i, zlen)
        bid = hashlib.sha256(data).digest()
        st, c1 = evp(bid, BLOCK_IV, data, True)
        assert st == 0
        bkey = hashlib.sha256(c1).digest()
        st, crypted = evp(bkey, BLOCK_IV, zipped, True)
        assert st == 0
        st, back = evp(bkey, BLOCK_IV, crypted, False)
        assert st == 0 and back == zipped
        pack.append({"data_seed": 5000 + i, "data_len": n, "zipped_seed": 5100 + i, "zipped_len": zlen,
                     "id": bid.hex(), "key": bkey.hex(), **out_fields("crypted", crypted)})
    kats["pack"] = pack

    with open(OUT, "w") as f:
        json.dump(kats, f, indent=1)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes;", len(enc), "encrypt,", len(dec), "decrypt,", len(pack), "pack records")
    print("decrypt statuses:", [r["status"] for r in dec])


if __name__ == "__main__":
    main()
