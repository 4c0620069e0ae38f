"""SHA-256 of device messages of different lengths in one launch
(vds_ec_sha256_batch_device): the names of a ragged upload batch
(dht_network_client.cpp:77-79, :591-593).  The checker is Python's hashlib
(OpenSSL, as the reference's hash::sha256) and the FIPS 180-4 examples.
Bit-exact; every digest is looked for at the caller's index, whatever order
the launch walks the messages in."""
import hashlib

import numpy as np
import pytest

import oracle_ctypes as O

pytestmark = pytest.mark.gpu

FIPS = {  # FIPS 180-4 / NIST example messages (as tests/test_sha256_gpu.py)
    b"": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    b"abc": "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad",
    b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq":
        "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1",
}
ALIGNMENTS = [0, 1, 2, 3, 4, 8, 12]  # start address mod 16: every byte offset, every dword of a 16-byte line
GUARD = 61                           # guard bytes either side of the digests (odd: the digest array is unaligned)


@pytest.fixture(scope="module")
def chunk(gpu):
    from vds_amd import chunk as c
    return c


def batch_digests(chunk, torch, messages, aligns, null_empty=False):
    """messages[j] (bytes) placed at an address = aligns[j] mod 16 of ONE device
    buffer whose gaps hold other bytes; one call; the digests, from between
    two guards that must come back untouched."""
    offs, pos = [], 0
    for m, a in zip(messages, aligns):
        pos = (pos + 15) // 16 * 16 + 16 + a
        offs.append(pos)
        pos += len(m)
    host = np.full(pos + 64, 0xA5, dtype=np.uint8)
    for m, off in zip(messages, offs):
        host[off:off + len(m)] = np.frombuffer(m, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 16 == 0
    count = len(messages)
    dig = torch.full((2 * GUARD + 32 * count,), 0x5A, dtype=torch.uint8, device="cuda")
    ptrs = [0 if (null_empty and not m) else dev.data_ptr() + off for m, off in zip(messages, offs)]
    chunk.sha256_batch_device(ptrs, [len(m) for m in messages], dig.data_ptr() + GUARD)
    torch.cuda.synchronize()
    got = dig.cpu().numpy()
    assert (got[:GUARD] == 0x5A).all() and (got[GUARD + 32 * count:] == 0x5A).all(), "guard bytes written"
    return [bytes(got[GUARD + 32 * j:GUARD + 32 * j + 32]) for j in range(count)]


def test_every_length_and_alignment_in_one_launch(chunk):
    """Every length 0..200 (every padding case: 55/56/63/64/119/120 ...) plus
    1000, 4099 and 65,543, each at every start alignment, shuffled so that the
    caller's order puts lengths 0 and 65,543 side by side: per-lane alignment,
    extreme divergence and the launch's internal reordering."""
    import torch
    rng = np.random.default_rng(20)
    cases = [(length, a) for length in list(range(201)) + [1000, 4099, 65543] for a in ALIGNMENTS]
    order = rng.permutation(len(cases))
    # the two extremes next to each other in the caller's order
    i0 = next(i for i in order if cases[i] == (0, 3))
    i1 = next(i for i in order if cases[i] == (65543, 1))
    order = [i0, i1] + [i for i in order if i not in (i0, i1)]
    cases = [cases[i] for i in order]
    messages = [rng.integers(0, 256, length, dtype=np.uint8).tobytes() for length, _ in cases]
    got = batch_digests(chunk, torch, messages, [a for _, a in cases])
    for j, (m, (length, a)) in enumerate(zip(messages, cases)):
        assert got[j] == hashlib.sha256(m).digest(), (j, length, a)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_wave_boundaries(chunk, count):
    import torch
    rng = np.random.default_rng(count)
    lengths = [int(x) for x in rng.permutation(count) * 5 + 1]  # distinct
    messages = [rng.integers(0, 256, length, dtype=np.uint8).tobytes() for length in lengths]
    got = batch_digests(chunk, torch, messages, [j % 4 for j in range(count)])
    for j, m in enumerate(messages):
        assert got[j] == hashlib.sha256(m).digest(), (count, j, lengths[j])


def test_fips_examples(chunk):
    """The standard's examples through the batch entry; the empty message with a NULL pointer."""
    import torch
    messages = list(FIPS)
    got = batch_digests(chunk, torch, messages, [0, 1, 2], null_empty=True)
    assert [g.hex() for g in got] == [FIPS[m] for m in messages]


def test_names_of_regenerated_replicas(chunk):
    """Repair re-saves what it regenerates (sync_process.cpp:313-335): the
    outputs of a regenerate_batch_device call named through
    sha256_batch_device, passing outs and the repeated chunk sizes."""
    import torch
    k = 16
    nodes = [list(range(1, 17)), [19, 18] + list(range(2, 16)), list(range(16))]
    targets = [[0, 17], [0, 1], [16, 19]]
    sizes = [5000, 32 * 1024 + 7, 33]
    rng = np.random.default_rng(7)
    data = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
    keep = [[torch.from_numpy(O.encode(k, r, d)).cuda() for r in nd] for nd, d in zip(nodes, data)]
    csz = [chunk.replica_size(k, s) for s in sizes]
    outs = [[torch.zeros(c + 3, dtype=torch.uint8, device="cuda") for _ in tg] for c, tg in zip(csz, targets)]
    ptrs = [[o.data_ptr() + 1 for o in row] for row in outs]  # (odd addresses: unaligned hashing)
    chunk.regenerate_batch_device(k, nodes, [[b.data_ptr() for b in row] for row in keep], csz, targets, ptrs)
    dig = torch.zeros((6, 32), dtype=torch.uint8, device="cuda")
    chunk.sha256_batch_device([p for row in ptrs for p in row], [c for c in csz for _ in range(2)], dig)
    torch.cuda.synchronize()
    got = dig.cpu().numpy()
    for o, (d, tg) in enumerate(zip(data, targets)):
        for i, t in enumerate(tg):
            assert bytes(got[2 * o + i]) == hashlib.sha256(O.encode(k, t, d).tobytes()).digest(), (o, t)
