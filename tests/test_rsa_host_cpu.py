"""The host half of the RSA verification (rsa_host.cpp), no GPU: key
preparation and the raw operation against Python integers, every case of the
libcrypto fixture (tests/golden/rsa_pkcs1_kats.json: keys, signatures and
verdicts all from EVP_* calls), the key fingerprint against a restatement of
the reference's lines, and the split of a transaction-log block against a
serializer written here."""
import ctypes as C
import hashlib

import pytest

import rsa_cases as R
from vds_amd import VdsEcError, _lib, chunk


def _limbs(a) -> int:
    return sum(int(v) << (32 * i) for i, v in enumerate(a))


def test_prepare_matches_python(vds_lib):
    for n in R.moduli():
        for e in R.EXPONENTS:
            key = chunk.rsa_key_prepare(n, e)
            limbs = 64 if n.bit_length() <= 2048 else 128
            assert (key.limbs, key.n_bytes, key.e) == (limbs, R.n_bytes(n), e)
            assert _limbs(key.n) == n
            assert key.n0inv == (-pow(n, -1, 2 ** 32)) % 2 ** 32
            assert _limbs(key.rr) == pow(2, 64 * limbs, n)
    # the magnitudes as the caller holds them: leading zero bytes change nothing
    n = R.moduli()[2]
    a = chunk.rsa_key_prepare(n, 65537)
    b = chunk.rsa_key_prepare(b"\x00\x00" + n.to_bytes(256, "big"), b"\x00\x00\x00\x01\x00\x01")
    assert bytes(a) == bytes(b)


def test_public_host_matches_pow(vds_lib):
    for i, n in enumerate(R.moduli()):
        k = R.n_bytes(n)
        for e in R.EXPONENTS:
            key = chunk.rsa_key_prepare(n, e)
            for s in R.operands(n, 100 + i):
                got = chunk.rsa_public_host(key, s.to_bytes(k, "big"))
                assert got == pow(s, e, n).to_bytes(k, "big"), (i, e, hex(s)[:18])


def test_out_of_range_inputs_and_bad_keys(vds_lib):
    n = R.kats()["keys"][2]["n"]
    k = R.n_bytes(n)
    key = chunk.rsa_key_prepare(n, 65537)
    for bad in (n.to_bytes(k, "big"), (2 ** (8 * k) - 1).to_bytes(k, "big"), (5).to_bytes(k - 1, "big"),
                (5).to_bytes(k + 1, "big"), b""):
        with pytest.raises(VdsEcError) as e:
            chunk.rsa_public_host(key, bad)
        assert e.value.status == _lib.EINVAL
    for bn, be in ((n + 1, 65537), (2 ** 511 - 1, 65537), (2 ** 4096 + 1, 65537), (0, 65537), (n, 65536), (n, 1),
                   (n, 0), (n, 2 ** 32 + 1)):
        with pytest.raises(VdsEcError) as e:
            chunk.rsa_key_prepare(bn, be)
        assert e.value.status == _lib.EINVAL, (hex(bn)[:12], be)
    assert chunk.rsa_key_prepare(2 ** 511 + 1, 3).limbs == 64  # the smallest modulus taken
    # a key that prepare did not make is refused, not used
    broken = chunk.rsa_key_prepare(n, 65537)
    broken.limbs = 96
    with pytest.raises(VdsEcError):
        chunk.rsa_public_host(broken, (5).to_bytes(k, "big"))


def test_every_fixture_case(vds_lib):
    f = R.kats()
    keys = [chunk.rsa_key_prepare(k["n"], k["e"]) for k in f["keys"]]
    assert sorted(k["bits"] for k in f["keys"]) == [2048, 3072, 4096, 4096]
    assert {c["len"] for c in f["cases"]} >= {0, 1, 55, 56, 64, 119, 4099, 65537}
    assert {c["verdict"] for c in f["cases"]} == {0, 1}
    for c in f["cases"]:
        assert chunk.rsa_verify_sha256_host(keys[c["key"]], c["msg"], c["sig"]) == bool(c["verdict"]), \
            (c["key"], c["name"])
    # a verdict of 1 is a signature that opens, with Python's pow, to exactly the encoding
    for c in f["cases"]:
        n, e = f["keys"][c["key"]]["n"], f["keys"][c["key"]]["e"]
        k = R.n_bytes(n)
        s = int.from_bytes(c["sig"], "big")
        opens = len(c["sig"]) == k and s < n and \
            pow(s, e, n).to_bytes(k, "big") == R.em_sha256(hashlib.sha256(c["msg"]).digest(), k)
        assert opens == bool(c["verdict"]), (c["key"], c["name"])


def test_fingerprint(vds_lib):
    for k in R.kats()["keys"]:
        assert chunk.rsa_fingerprint(k["n"], k["e"]) == R.fingerprint(k["n"], k["e"])
    # the 00 prefix rule at its edges, for both magnitudes: a top nibble of 7, 8 (none), 9, f (one)
    tops = (0x7F, 0x80, 0x8F, 0x90, 0xFF, 0x08, 0x09, 0x01)
    for tn in tops:
        for te in tops:
            n = int.from_bytes(bytes([tn]) + bytes(range(1, 70)), "big")
            e = int.from_bytes(bytes([te, 0x00, 0x01]), "big")
            assert chunk.rsa_fingerprint(n, e) == R.fingerprint(n, e), (tn, te)
            assert chunk.rsa_fingerprint(b"\x00" + n.to_bytes(70, "big"), e) == R.fingerprint(n, e)


def _block():
    key_id = bytes(range(32))
    ancestors = [bytes([i]) * 32 for i in (9, 3, 200)] + [b"\x05" * 31]
    prefix = R.block_prefix(1700000000, 300, key_id, ancestors, bytes(range(200)))
    return prefix, R.block(prefix, bytes(range(256)) * 2)


def test_txblock_parse_fields(vds_lib):
    prefix, blk = _block()
    st, f = chunk.txblock_parse(blk)
    assert st == 0
    assert (f["time_point"], f["order_no"]) == (1700000000, 300)
    assert blk[f["key_id_off"]:f["key_id_off"] + f["key_id_len"]] == bytes(range(32)) and f["key_id_off"] == 21
    assert f["ancestors_count"] == 4 and f["ancestors_off"] == 53
    anc = blk[f["ancestors_off"]:f["ancestors_off"] + f["ancestors_len"]]
    assert anc == b"\x04" + b"\x1f" + b"\x05" * 31 + b"".join(b"\x20" + bytes([i]) * 32 for i in (3, 9, 200))
    assert blk[f["messages_off"]:f["messages_off"] + f["messages_len"]] == bytes(range(200))
    assert f["messages_off"] == f["ancestors_off"] + f["ancestors_len"] + 2  # 200 is written 81 48
    assert f["signed_len"] == len(prefix) == f["messages_off"] + 200
    assert f["signature_off"] == len(prefix) + 3 and f["signature_len"] == 512  # 512 is written 82 01 80
    assert f["signature_off"] + f["signature_len"] == len(blk)
    # no ancestors, empty messages, empty signature: still a block
    p = R.block_prefix(0, 0, b"", [], b"")
    st, f = chunk.txblock_parse(R.block(p, b""))
    assert st == 0 and f["signed_len"] == len(p) == 23 and f["signature_len"] == 0 and f["ancestors_count"] == 0
    # numbers at the edges of write_number's forms
    for n in (127, 128, 383, 384, 65663, 65664):
        p = R.block_prefix(5, 6, b"k" * 32, [], bytes(n))
        st, f = chunk.txblock_parse(R.block(p, b"s" * n))
        assert st == 0 and (f["messages_len"], f["signature_len"], f["signed_len"]) == (n, n, len(p)), n


def test_txblock_parse_refuses_what_validate_would_not_sign(vds_lib):
    prefix, blk = _block()
    sig = bytes(512)
    key_id, msgs = b"k" * 32, bytes(200)
    a, b = b"\x01" * 32, b"\x02" * 32
    forms = {
        "version": R.block(R.block_prefix(1, 2, key_id, [a], msgs, version=0x31564454), sig),
        "ancestors descending": R.block(R.block_prefix(1, 2, key_id, [b, a], msgs, sort=False), sig),
        "an ancestor twice": R.block(R.block_prefix(1, 2, key_id, [a, a], msgs, sort=False), sig),
        "a longer ancestor first": R.block(R.block_prefix(1, 2, key_id, [b"\x01\x00", b"\x02"], msgs, sort=False), sig),
        "a byte behind the signature": blk + b"\x00",
        "a time from_time_t cannot hold": R.block(R.block_prefix(2 ** 63 // 10 ** 9, 2, key_id, [a], msgs), sig),
    }
    # numbers not in their shortest form: 200 as 82 00 48, 128 as 80, 512 as 83 00 01 80, nine length bytes
    head = R.block_prefix(1, 2, key_id, [a], b"")[:-1]
    forms["82 00 48"] = head + b"\x82\x00\x48" + msgs + R.buffer(sig)
    forms["80"] = head + b"\x80" + bytes(128) + R.buffer(sig)
    forms["83 00 01 80"] = head + R.buffer(msgs) + b"\x83\x00\x01\x80" + sig
    forms["89"] = head + b"\x89" + bytes(8) + b"\x48" + msgs + R.buffer(sig)
    forms["count 81 00 written 82 00 00"] = (R.block_prefix(1, 2, key_id, [], b"")[:-2] + b"\x82\x00\x00" +
                                             b"".join(R.buffer(bytes([1, i // 256, i % 256])) for i in range(128)) +
                                             R.buffer(msgs) + R.buffer(sig))
    # (their canonical spellings are blocks)
    assert chunk.txblock_parse(head + R.buffer(msgs) + R.buffer(sig))[0] == 0
    assert chunk.txblock_parse(R.block(R.block_prefix(1, 2, key_id, [b"\x02", b"\x01\x00"], msgs, sort=False), sig))[0] == 0
    assert chunk.txblock_parse(R.block(R.block_prefix(2 ** 63 // 10 ** 9 - 1, 2, key_id, [a], msgs), sig))[0] == 0
    many = [bytes([1, i // 256, i % 256]) for i in range(128)]
    assert chunk.txblock_parse(R.block(R.block_prefix(1, 2, key_id, many, msgs), sig))[1]["ancestors_count"] == 128
    for name, data in forms.items():
        assert chunk.txblock_parse(data) == (_lib.ETX_FORM, None), name
    # every truncation point of one block
    assert chunk.txblock_parse(blk)[0] == 0
    for cut in range(len(blk)):
        assert chunk.txblock_parse(blk[:cut])[0] == _lib.ETX_FORM, cut
    # a length that points past the end, and one past 1 GiB
    assert chunk.txblock_parse(head + b"\x84\x7f\xff\xff\xff" + msgs)[0] == _lib.ETX_FORM
    assert chunk.txblock_parse(head + b"\x88" + b"\xff" * 8 + msgs)[0] == _lib.ETX_FORM
    # null arguments
    assert vds_lib.vds_ec_txblock_parse(None, 5, C.byref(_lib.TxBlock())) == _lib.EINVAL
    assert vds_lib.vds_ec_txblock_parse(blk, len(blk), None) == _lib.EINVAL
