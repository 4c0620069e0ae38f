"""Batched AES-256-CBC on the device (vds_ec_aes256_cbc_encrypt_batch_device /
_decrypt_batch_device, aes.hip): messages of different lengths in one launch
each way.

The checker is the library's host cipher vds_ec_aes256_cbc_*_host (pinned
against OpenSSL's recorded answers by tests/test_aes_host_cpu.py) and those
records themselves (tests/golden/aes_cbc_kats.json).  Bit-exact.

Layout: every input of a launch lies in ONE device buffer with foreign bytes
(0xA5) between the messages, every output in ONE buffer between 0x5A guard
bytes, and the statuses and lengths start as a sentinel, so that one the launch
did not write shows."""
import os
import random
import re

import numpy as np
import pytest

import aes_kats as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOD16 = (0, 1, 2, 3, 4, 8, 12)
LENGTHS = list(range(50)) + [255, 256, 257, 4095, 4096, 65536, 65537]
GUARD = 16
FILL = 0x5A
SENTINEL = 0x5A5A5A5A


def _dec_tile() -> int:
    """kAesDecTile (ec_internal.hpp): the decrypt's tile, whose borders the lengths below straddle."""
    with open(os.path.join(ROOT, "vds_amd", "csrc", "ec_internal.hpp")) as f:
        m = re.search(r"constexpr uint32_t kAesDecTile = (\d+);", f.read())
    tile = int(m.group(1))
    assert tile % 16 == 0 and 256 <= tile <= (1 << 20)
    return tile


def _place(lens, mods, lead):
    """Offsets of pieces of `lens` bytes, piece i at mods[i] modulo 16, at least `lead` bytes apart."""
    offs, pos = [], 0
    for ln, m in zip(lens, mods):
        pos = (pos + 15) // 16 * 16 + 16 * ((lead + 15) // 16) + m
        offs.append(pos)
        pos += ln
    return offs, pos + lead + 16


def _mods(count, shift=0):
    """Message i reads at MOD16[i % 7] and writes at MOD16[(i // 7 + shift) % 7] mod 16: 49 consecutive
    messages meet every pair."""
    return [MOD16[i % 7] for i in range(count)], [MOD16[(i // 7 + shift) % 7] for i in range(count)]


def _upload(torch, pieces, offs, total):
    buf = np.full(total, 0xA5, dtype=np.uint8)
    for p, off in zip(pieces, offs):
        buf[off:off + len(p)] = np.frombuffer(p, dtype=np.uint8)
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _dev_bytes(torch, rows):
    return torch.from_numpy(np.frombuffer(b"".join(rows), dtype=np.uint8).copy()).cuda()


def _run_encrypt(torch, lib, msgs, keys, ivs, shift=0):
    """One encrypt launch over msgs with per-message keys (and ivs, or None for pack_block_iv): every
    output against the host function's, in the caller's order, and every byte outside the outputs
    untouched.  Returns the ciphertexts."""
    from vds_amd import chunk
    count = len(msgs)
    want_ct = [K.host_encrypt(lib, keys[i], ivs[i] if ivs else K.block_iv(), m) for i, m in enumerate(msgs)]
    in_mods, out_mods = _mods(count, shift)
    i_offs, i_total = _place([len(m) for m in msgs], in_mods, 16)
    o_offs, o_total = _place([len(c) for c in want_ct], out_mods, GUARD)
    d_in = _upload(torch, msgs, i_offs, i_total)
    d_keys = _dev_bytes(torch, keys)
    d_ivs = _dev_bytes(torch, ivs) if ivs else None
    d_out = torch.full((o_total,), FILL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    want = np.full(o_total, FILL, dtype=np.uint8)
    for c, off in zip(want_ct, o_offs):
        want[off:off + len(c)] = np.frombuffer(c, dtype=np.uint8)
    chunk.aes256_cbc_encrypt_batch_device([d_in.data_ptr() + o for o in i_offs], [len(m) for m in msgs], d_keys,
                                          [d_out.data_ptr() + o for o in o_offs], ivs=d_ivs)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    wrong = np.flatnonzero(got != want)
    if wrong.size:
        at = int(wrong[0])
        i = max(int(np.searchsorted(np.asarray(o_offs), at, side="right")) - 1, 0)
        raise AssertionError(("bytes", at, "message", i, "offset in it", at - o_offs[i], "length", len(msgs[i]),
                              "padded", len(want_ct[i]), int(got[at]), int(want[at]), "wrong bytes", int(wrong.size)))
    return want_ct


def _run_decrypt(torch, lib, cts, keys, ivs, shift=0):
    """One decrypt launch over cts: every status and out_len against the host function's, the first
    out_len bytes of every good message against its plaintext, nothing checked beyond them inside the
    message's own lens[o] bytes, and every byte outside those ranges untouched.  Returns
    [(status, plaintext)]."""
    from vds_amd import chunk
    count = len(cts)
    ref = [K.host_decrypt(lib, keys[i], ivs[i] if ivs else K.block_iv(), c) for i, c in enumerate(cts)]
    in_mods, out_mods = _mods(count, shift)
    i_offs, i_total = _place([len(c) for c in cts], in_mods, 16)
    o_offs, o_total = _place([len(c) for c in cts], out_mods, GUARD)
    d_in = _upload(torch, cts, i_offs, i_total)
    d_keys = _dev_bytes(torch, keys)
    d_ivs = _dev_bytes(torch, ivs) if ivs else None
    d_out = torch.full((o_total,), FILL, dtype=torch.uint8, device="cuda")
    d_len = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    d_st = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    want = np.full(o_total, FILL, dtype=np.uint8)
    must = np.ones(o_total, dtype=bool)  # bytes whose value is specified
    for (st, pt), c, off in zip(ref, cts, o_offs):
        if st != K.ECRYPT_LENGTH:  # (a bad length gets its status and no other work: not a byte written)
            must[off:off + len(c)] = False
        if st == 0:
            want[off:off + len(pt)] = np.frombuffer(pt, dtype=np.uint8)
            must[off:off + len(pt)] = True
    chunk.aes256_cbc_decrypt_batch_device([d_in.data_ptr() + o for o in i_offs], [len(c) for c in cts], d_keys,
                                          [d_out.data_ptr() + o for o in o_offs], d_len, d_st, ivs=d_ivs)
    torch.cuda.synchronize()
    st, ol, got = d_st.cpu().numpy(), d_len.cpu().numpy(), d_out.cpu().numpy()
    want_st = np.asarray([r[0] for r in ref], dtype=np.int32)
    want_ol = np.asarray([len(r[1]) for r in ref], dtype=np.int32)
    bad = np.flatnonzero(st != want_st)
    assert bad.size == 0, ("status", int(bad[0]), len(cts[bad[0]]), int(st[bad[0]]), int(want_st[bad[0]]))
    bad = np.flatnonzero(ol != want_ol)
    assert bad.size == 0, ("out_len", int(bad[0]), len(cts[bad[0]]), int(ol[bad[0]]), int(want_ol[bad[0]]))
    wrong = np.flatnonzero((got != want) & must)
    if wrong.size:
        at = int(wrong[0])
        i = max(int(np.searchsorted(np.asarray(o_offs), at, side="right")) - 1, 0)
        raise AssertionError(("bytes", at, "message", i, "offset in it", at - o_offs[i], "length", len(cts[i]),
                              int(got[at]), int(want[at]), "wrong bytes", int(wrong.size)))
    return ref


def _keys_ivs(rng, count):
    return [rng.randbytes(32) for _ in range(count)], [rng.randbytes(16) for _ in range(count)]


@pytest.fixture(scope="module")
def mixed():
    """Every length of LENGTHS in one batch, shuffled, the longest beside the shortest."""
    rng = random.Random(11)
    lengths = [n for n in LENGTHS if n not in (0, 65536, 65537)]
    rng.shuffle(lengths)
    lengths[len(lengths) // 2:len(lengths) // 2] = [65537, 0, 65536]
    assert sorted(lengths) == sorted(LENGTHS)
    data = rng.randbytes(max(LENGTHS) + len(lengths))
    msgs = [data[i:i + n] for i, n in enumerate(lengths)]
    keys, ivs = _keys_ivs(rng, len(msgs))
    return msgs, keys, ivs


@pytest.mark.parametrize("with_ivs", (True, False))
def test_encrypt_mixed_lengths_one_launch(gpu, vds_lib, mixed, with_ivs):
    """Lengths 0..49, 255..257, 4095, 4096, 65536, 65537 in ONE launch: the quads of a wave end at
    different steps, each after exactly its own padded size (the guards), at every input and output
    alignment, under per-message keys."""
    import torch
    msgs, keys, ivs = mixed
    assert len(msgs) >= 49
    _run_encrypt(torch, vds_lib, msgs, keys, ivs if with_ivs else None, shift=0 if with_ivs else 3)


@pytest.mark.parametrize("arm", ("quad", "lane"))
def test_encrypt_arms(gpu, vds_lib, mixed, monkeypatch, arm):
    """The one-lane-a-chain kernel behind VDS_EC_AES_ENC=lane (the A/B arm, which no other test
    launches) and the quad kernel with the switch cleared: the mixed batch, and 130 short chains (more
    than one wave of either form), byte for byte the host function's."""
    import torch
    if arm == "lane":
        monkeypatch.setenv("VDS_EC_AES_ENC", "lane")
    else:
        monkeypatch.delenv("VDS_EC_AES_ENC", raising=False)
    msgs, keys, ivs = mixed
    _run_encrypt(torch, vds_lib, msgs, keys, ivs, shift=1)
    rng = random.Random(16)
    short = [rng.randbytes(rng.randrange(70)) for _ in range(130)]
    k2, _ = _keys_ivs(rng, len(short))
    _run_encrypt(torch, vds_lib, short, k2, None, shift=6)


@pytest.mark.parametrize("count", (1, 3, 16, 17, 65, 130))
def test_encrypt_batch_counts(gpu, vds_lib, count):
    """Quad and wave borders of the batch: 16 chains a wave."""
    import torch
    rng = random.Random(100 + count)
    msgs = [rng.randbytes(rng.choice((0, 1, 15, 16, 17, 40, 100, 333, 600))) for _ in range(count)]
    keys, ivs = _keys_ivs(rng, count)
    _run_encrypt(torch, vds_lib, msgs, keys, ivs if count % 2 else None, shift=count)


def test_encrypt_outputs_in_caller_order(gpu, vds_lib):
    """Ascending lengths: the kernel's order (longest first) is the reverse of the caller's."""
    import torch
    rng = random.Random(12)
    msgs = [rng.randbytes(16 * i + i % 5) for i in range(40)]
    keys, ivs = _keys_ivs(rng, len(msgs))
    cts = _run_encrypt(torch, vds_lib, msgs, keys, ivs)
    assert [len(c) for c in cts] == sorted(len(c) for c in cts)


def test_encrypt_fixture_records(gpu, vds_lib):
    import torch
    recs = K.kats()["encrypt"]
    for with_ivs in (True, False):
        rs = [r for r in recs if bool(r["iv"]) == with_ivs]
        msgs = [K.sm(r["seed"], r["len"]) for r in rs]
        cts = _run_encrypt(torch, vds_lib, msgs, [bytes.fromhex(r["key"]) for r in rs],
                           [bytes.fromhex(r["iv"]) for r in rs] if with_ivs else None, shift=2)
        for r, c in zip(rs, cts):  # (what the device wrote equals these: _run_encrypt)
            assert K.matches(r, "out", c), r["len"]


@pytest.mark.parametrize("with_ivs", (True, False))
def test_decrypt_round_trip_and_tile_borders(gpu, vds_lib, mixed, with_ivs):
    """The mixed batch back, plus ciphertexts of kAesDecTile - 16, kAesDecTile, kAesDecTile + 16 and
    2 kAesDecTile + 16 bytes: a block's predecessor lies in the previous tile (and wave), and only
    tile 0 may take the iv."""
    import torch
    tile = _dec_tile()
    rng = random.Random(13)
    msgs, keys, ivs = mixed
    extra = [rng.randbytes(n - 1) for n in (tile - 16, tile, tile + 16, 2 * tile + 16)]
    ek, ei = _keys_ivs(rng, len(extra))
    msgs, keys, ivs = extra[:2] + list(msgs) + extra[2:], ek[:2] + list(keys) + ek[2:], ei[:2] + list(ivs) + ei[2:]
    use = ivs if with_ivs else None
    cts = [K.host_encrypt(vds_lib, keys[i], use[i] if use else K.block_iv(), m) for i, m in enumerate(msgs)]
    assert {tile - 16, tile, tile + 16, 2 * tile + 16} <= {len(c) for c in cts}
    ref = _run_decrypt(torch, vds_lib, cts, keys, use, shift=0 if with_ivs else 4)
    assert [r for r in ref] == [(0, m) for m in msgs]


@pytest.mark.parametrize("count", (1, 3, 16, 17, 65, 130))
def test_decrypt_batch_counts(gpu, vds_lib, count):
    import torch
    rng = random.Random(200 + count)
    msgs = [rng.randbytes(rng.choice((0, 1, 15, 16, 17, 40, 100, 333, 600))) for _ in range(count)]
    keys, ivs = _keys_ivs(rng, count)
    use = ivs if count % 2 else None
    cts = [K.host_encrypt(vds_lib, keys[i], use[i] if use else K.block_iv(), m) for i, m in enumerate(msgs)]
    ref = _run_decrypt(torch, vds_lib, cts, keys, use, shift=count)
    assert ref == [(0, m) for m in msgs]


def test_decrypt_fixture_status_cases(gpu, vds_lib):
    """Every recorded decrypt case -- bad lengths, bad paddings, tampered ciphertexts that fail and
    that still unpad -- in launches beside good messages; the statuses are OpenSSL's."""
    import torch
    recs = K.kats()["decrypt"]
    rng = random.Random(14)
    for with_ivs in (True, False):
        rs = [r for r in recs if bool(r["iv"]) == with_ivs]
        cases = [K.decrypt_case(vds_lib, r) for r in rs]
        cts, keys, ivs, want = [], [], [], []
        for r, (key, iv, ct) in zip(rs, cases):
            good_key, good_iv, good = rng.randbytes(32), rng.randbytes(16), rng.randbytes(rng.randrange(200))
            cts += [ct, K.host_encrypt(vds_lib, good_key, good_iv if with_ivs else K.block_iv(), good)]
            keys += [key, good_key]
            ivs += [iv or K.block_iv(), good_iv]
            want += [(r["status"], r["out_len"], r), (0, len(good), None)]
        ref = _run_decrypt(torch, vds_lib, cts, keys, ivs if with_ivs else None, shift=5)
        assert len(ref) == len(want)
        for (st, pt), (wst, wlen, r) in zip(ref, want):  # (what the device wrote equals ref: _run_decrypt)
            assert (st, len(pt)) == (wst, wlen), r and r["name"]
            if r is not None and st == 0:
                assert K.matches(r, "out", pt), r["name"]
        assert {w[0] for w in want} >= {0, K.ECRYPT_PADDING} and (with_ivs or K.ECRYPT_LENGTH in {w[0] for w in want})


def test_decrypt_bad_lengths_get_status_only(gpu, vds_lib):
    """Lengths 0 and not a multiple of 16 between good messages: status, out_len 0, not one byte written."""
    import torch
    rng = random.Random(15)
    keys, ivs = _keys_ivs(rng, 6)
    good = K.host_encrypt(vds_lib, keys[1], ivs[1], rng.randbytes(70))
    cts = [b"", good, rng.randbytes(17), rng.randbytes(5000), K.host_encrypt(vds_lib, keys[4], ivs[4], b""),
           rng.randbytes(15)]
    ref = _run_decrypt(torch, vds_lib, cts, keys, ivs)
    assert [r[0] for r in ref] == [K.ECRYPT_LENGTH, 0, K.ECRYPT_LENGTH, K.ECRYPT_LENGTH, 0, K.ECRYPT_LENGTH]
    assert ref[4] == (0, b"")


def test_empty_batches(gpu, vds_lib):
    from vds_amd import chunk
    chunk.aes256_cbc_encrypt_batch_device([], [], None, [])
    chunk.aes256_cbc_decrypt_batch_device([], [], None, [], None, None)
