"""RSA on the device (rsa.hip through vds_ec_rsa_*_batch_device and
vds_ec_txblock_validate_host_batch): the raw operation against Python's pow on
the CPU test's moduli, exponents and operands, 64- and 128-limb keys
interleaved in one call; every case of the libcrypto fixture in one call, in
the digest form and the SHA form; a mixed call against the host form item by
item; and a drained batch of transaction-log blocks built and signed here."""
import hashlib
import random

import numpy as np
import pytest
import torch

import rsa_cases as R
from vds_amd import _lib, chunk

pytestmark = pytest.mark.gpu
GUARD = 16
FILL = 0xA5


def _dev(b: bytes, device):
    return torch.from_numpy(np.frombuffer(b or b"\x00", dtype=np.uint8).copy()).to(device)


def _pack(parts, device):
    """The byte strings behind one another on the device -> (tensor, pointers)"""
    offs, at = [], 0
    for p in parts:
        offs.append(at)
        at += len(p)
    t = _dev(b"".join(parts), device)
    return t, [t.data_ptr() + o for o in offs]


@pytest.fixture(scope="module")
def raw_pool(vds_lib):
    """(key index, operand bytes, expected status, expected bytes) over every modulus, exponent and operand
    of the CPU test, then the out-of-range forms; keys of 64 and 128 limbs alternate through the pool."""
    keys, items = [], {64: [], 128: []}
    for i, n in enumerate(R.moduli()):
        k = R.n_bytes(n)
        for e in R.EXPONENTS:
            keys.append(chunk.rsa_key_prepare(n, e))
            ki, limbs = len(keys) - 1, keys[-1].limbs
            for s in R.operands(n, 100 + i):
                items[limbs].append((ki, s.to_bytes(k, "big"), 0, pow(s, e, n).to_bytes(k, "big")))
            if e == 65537:
                for bad in (n.to_bytes(k, "big"), b"\xff" * k, (5).to_bytes(k - 1, "big"), (5).to_bytes(k + 1, "big"), b""):
                    items[limbs].append((ki, bad, 0xFF, None))
    r = random.Random(7)
    r.shuffle(items[64])
    r.shuffle(items[128])
    pool = []
    while items[64] or items[128]:
        for limbs in (128, 64):
            if items[limbs]:
                pool.append(items[limbs].pop())
    return keys, pool


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_raw_operation_matches_pow(gpu, raw_pool, count):
    keys, pool = raw_pool
    start = {1: 0, 63: 1, 64: 64, 65: 128, 257: 0}[count]
    batch = [pool[(start + j) % len(pool)] for j in range(count)]
    if count >= 63:
        assert {keys[b[0]].limbs for b in batch} == {64, 128} and {b[2] for b in batch} == {0, 0xFF}
    ins, in_ptrs = _pack([b[1] for b in batch], gpu)
    out_offs, at = [], GUARD
    for b in batch:
        out_offs.append(at)
        at += keys[b[0]].n_bytes + GUARD
    outs = torch.full((at,), FILL, dtype=torch.uint8, device=gpu)
    statuses = torch.full((count + 2 * GUARD,), FILL, dtype=torch.uint8, device=gpu)
    chunk.rsa_public_batch_device(in_ptrs, [len(b[1]) for b in batch], [b[0] for b in batch], keys,
                                  [outs.data_ptr() + o for o in out_offs], statuses.data_ptr() + GUARD)
    torch.cuda.synchronize()
    got, st = outs.cpu().numpy().tobytes(), statuses.cpu().numpy()
    assert (st[:GUARD] == FILL).all() and (st[GUARD + count:] == FILL).all()
    want = bytearray([FILL]) * at
    for (ki, _, status, value), o in zip(batch, out_offs):
        if status == 0:
            want[o:o + len(value)] = value
    assert st[GUARD:GUARD + count].tolist() == [b[2] for b in batch]
    bad = [j for j, o in enumerate(out_offs) if got[o - GUARD:o + keys[batch[j][0]].n_bytes + GUARD] !=
           bytes(want[o - GUARD:o + keys[batch[j][0]].n_bytes + GUARD])]
    assert not bad, [(j, batch[j][0], keys[batch[j][0]].limbs, keys[batch[j][0]].e) for j in bad[:8]]
    assert got == bytes(want)


@pytest.fixture(scope="module")
def fixture_keys(vds_lib):
    return [chunk.rsa_key_prepare(k["n"], k["e"]) for k in R.kats()["keys"]]


def _verify_both_forms(gpu, keys, cases):
    """cases: (key index, msg, sig) -> the verdicts, after checking that the digest form, the SHA form and the
    SHA form with the library's own digest scratch agree, the digests are hashlib's and the guards are whole"""
    count = len(cases)
    msgs, msg_ptrs = _pack([c[1] for c in cases], gpu)
    sigs, sig_ptrs = _pack([c[2] for c in cases], gpu)
    ml, sl, ki = [len(c[1]) for c in cases], [len(c[2]) for c in cases], [c[0] for c in cases]
    want_digests = b"".join(hashlib.sha256(c[1]).digest() for c in cases)
    dig_in = _dev(want_digests, gpu)
    v = [torch.full((count + 2 * GUARD,), FILL, dtype=torch.uint8, device=gpu) for _ in range(3)]
    dig_out = torch.full((32 * count + 2 * GUARD,), FILL, dtype=torch.uint8, device=gpu)
    chunk.rsa_verify_digest_batch_device(dig_in, sig_ptrs, sl, ki, keys, v[0].data_ptr() + GUARD)
    chunk.rsa_verify_sha256_batch_device(msg_ptrs, ml, sig_ptrs, sl, ki, keys, v[1].data_ptr() + GUARD,
                                         digests=dig_out.data_ptr() + GUARD)
    chunk.rsa_verify_sha256_batch_device(msg_ptrs, ml, sig_ptrs, sl, ki, keys, v[2].data_ptr() + GUARD)
    torch.cuda.synchronize()
    v = [x.cpu().numpy() for x in v]
    for x in v:
        assert (x[:GUARD] == FILL).all() and (x[GUARD + count:] == FILL).all()
    d = dig_out.cpu().numpy()
    assert (d[:GUARD] == FILL).all() and (d[GUARD + 32 * count:] == FILL).all()
    assert d[GUARD:GUARD + 32 * count].tobytes() == want_digests
    got = v[0][GUARD:GUARD + count].tolist()
    assert got == v[1][GUARD:GUARD + count].tolist() == v[2][GUARD:GUARD + count].tolist()
    return got


def test_every_fixture_case_in_one_call(gpu, fixture_keys):
    cases = R.kats()["cases"]
    got = _verify_both_forms(gpu, fixture_keys, [(c["key"], c["msg"], c["sig"]) for c in cases])
    wrong = [(c["key"], c["name"], g) for c, g in zip(cases, got) if g != c["verdict"]]
    assert not wrong, wrong


def test_mixed_call_matches_the_host_form(gpu, fixture_keys):
    good = [c for c in R.kats()["cases"] if c["verdict"] == 1 and c["len"] <= 4099]
    assert {c["key"] for c in good} == {0, 1, 2, 3}
    r = random.Random(11)
    cases = []
    for j in range(257):
        c = good[(j * 7) % len(good)]
        ki, msg, sig = c["key"], bytearray(c["msg"]), bytearray(c["sig"])
        if r.randrange(3) == 0:
            what = r.randrange(3)
            if what == 0 or (what == 1 and not msg):
                sig[r.randrange(len(sig))] ^= 1 << r.randrange(8)
            elif what == 1:
                msg[r.randrange(len(msg))] ^= 1 << r.randrange(8)
            else:
                ki = (ki + 1 + r.randrange(3)) % 4
        cases.append((ki, bytes(msg), bytes(sig)))
    got = _verify_both_forms(gpu, fixture_keys, cases)
    want = [int(chunk.rsa_verify_sha256_host(fixture_keys[ki], msg, sig)) for ki, msg, sig in cases]
    assert 60 < want.count(0) < 120
    assert got == want


def test_txblock_validate_host_batch(gpu):
    # (seeds whose prime searches are short: about a second for the three keys)
    big, small, stranger = R.signer(4096, 7), R.signer(2048, 7), R.signer(2048, 1)
    keys = [chunk.rsa_key_prepare(s.n, s.e) for s in (big, small)]
    prints = [R.fingerprint(s.n, s.e) for s in (big, small)]
    assert prints == [chunk.rsa_fingerprint(s.n, s.e) for s in (big, small)]
    r = random.Random(5)
    blocks, want = [], []
    for j in range(65):
        kind = ("good", "good", "flipped", "small", "good", "unknown", "form", "small")[j % 8]
        s = {"small": small, "unknown": stranger}.get(kind, big)
        ancestors = [bytes(r.getrandbits(8) for _ in range(32)) for _ in range(j % 4)]
        messages = bytes(r.getrandbits(8) for _ in range(1 + (j * 53) % 700))
        prefix = R.block_prefix(1700000000 + j, 1 + j, R.fingerprint(s.n, s.e), ancestors, messages)
        blk = bytearray(R.block(prefix, s.sign(prefix)))
        status, verdict = 0, 1
        if kind == "flipped":
            blk[len(prefix) - 1 - (j % len(messages))] ^= 0x20
            verdict = 0
        elif kind == "unknown":
            status, verdict = _lib.ETX_KEY, 0
        elif kind == "form":
            blk += b"\x00"
            status, verdict = _lib.ETX_FORM, 0
        blocks.append(bytes(blk))
        want.append((hashlib.sha256(blk).digest(), status, verdict))
    got = chunk.txblock_validate_host_batch(blocks, keys, prints)
    assert [g[1:] for g in got] == [w[1:] for w in want]
    assert [g[0] for g in got] == [w[0] for w in want]
    # no keys at all: every canonical block's writer is unknown
    got = chunk.txblock_validate_host_batch(blocks[:9], [], [])
    assert [g[1] for g in got] == [_lib.ETX_FORM if w[1] == _lib.ETX_FORM else _lib.ETX_KEY for w in want[:9]]
    assert [g[0] for g in got] == [w[0] for w in want[:9]] and not any(g[2] for g in got)
