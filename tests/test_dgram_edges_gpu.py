"""The edges of the datagram kernels (vds_amd/csrc/dgram.hip and the planning
in api_dgram_batch.cpp) that tests/test_dgram_gpu.py does not reach: opening
more than one wave of datagrams, every regime of the wave copy and the per-lane
copy it is measured against, routes long enough for the whole-block path of
seg_block, a message that owns whole waves of a seal, a launch whose messages
differ in mtu, route and session, 65,535-byte datagrams, and HMAC chains long
enough for the comparison sort of order_by_blocks.

The reference is the one test_dgram_gpu.py uses: Python's hmac / hashlib and
the seal_ref restatement of dht_datagram_protocol::prepare_to_send.  Every
comparison is bit-exact; every output lies between guard bytes and the whole
buffer is compared, the bytes a call must not write included; every verdict
array starts as a sentinel; the expected side is computed on the CPU only."""
import numpy as np
import pytest

from test_dgram_gpu import GUARD, KEYS, _seal_cases, be32, mac, place, route_blob, seal_ref

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ opening
def _cont(key, index, payload):
    """A continuation datagram: 0x03, BE32 index, payload, MAC (hdr_len 5)."""
    body = b"\x03" + be32(index) + bytes(payload)
    return body + mac(key, body)


def _forge(dg, hdr, pick, bit):
    """One bit of the datagram flipped: in its header, its payload or its MAC
    by turns (pick), as test_open does; a datagram with no payload byte to
    choose takes the header flip instead."""
    dg, n = bytearray(dg), len(dg) - 32
    where = (hdr // 2, hdr + (n - hdr) // 2, n + 13)[pick % 3]
    if pick % 3 == 1 and n <= hdr:
        where = 0
    dg[where] ^= 1 << (bit % 8)
    return bytes(dg)


def _open_check(items, nkeys):
    """One dgram_open_batch_device launch and every byte it may and may not
    write.  items: [(datagram as sent, session, hdr_len, src & 3 of the payload,
    dst & 3, forged)] -- a forged datagram is the sent one with a bit flipped,
    so what the payload would have been is still known: its range must keep the
    guard.  The destinations share one assembly buffer, five guard bytes or
    more between neighbours; the verdicts sit at an odd address between guard
    bytes."""
    import torch
    from vds_amd import chunk
    n = len(items)
    pos, at = [], 8
    for dg, _, hdr, _, da, _ in items:
        at += 5
        at += (da - at) % 4
        pos.append(at)
        at += len(dg) - 32 - hdr
    total = at + 8
    exp = np.full(total, GUARD, dtype=np.uint8)
    for (dg, _, hdr, _, _, forged), p in zip(items, pos):
        if not forged:
            pay = dg[hdr:len(dg) - 32]
            exp[p:p + len(pay)] = np.frombuffer(pay, dtype=np.uint8)
    dbuf, dptr = place(torch, [it[0] for it in items], [(it[3] - it[2]) % 4 for it in items])
    asm = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    assert asm.data_ptr() % 4 == 0 and dbuf.data_ptr() % 4 == 0
    for (dg, _, hdr, sa, da, _), sp, p in zip(items, dptr, pos):
        assert (sp + hdr) % 4 == sa and (asm.data_ptr() + p) % 4 == da
    before = dbuf.cpu().numpy().copy()
    vd = torch.full((n + 16,), GUARD, dtype=torch.uint8, device="cuda")
    chunk.dgram_open_batch_device(dptr, [len(it[0]) for it in items], [it[2] for it in items],
                                  [it[1] for it in items], KEYS[:nkeys], [asm.data_ptr() + p for p in pos],
                                  vd.data_ptr() + 7)
    torch.cuda.synchronize()
    v = vd.cpu().numpy()
    assert (v[:7] == GUARD).all() and (v[7 + n:] == GUARD).all()
    bad = [j for j in range(n) if items[j][5]]
    assert [j for j in range(n) if v[7 + j] != 0] == bad and all(v[7 + j] == 1 for j in bad)
    got = asm.cpu().numpy()
    diff = np.nonzero(got != exp)[0]
    assert diff.size == 0, (diff[:8], [(j, p) for j, p in enumerate(pos) if p <= diff[0]][-1:])
    assert np.array_equal(dbuf.cpu().numpy(), before)  # the datagrams are read, never written


# payload lengths: cnt < head and nd == 0 (1..9); nd around 64 (250..262) and
# around 128 (506..518) for every head length 0..3; the two continuations of the
# existing tests' mtus (463, 1363)
_COPY_LENGTHS = list(range(1, 10)) + list(range(250, 263)) + list(range(506, 519)) + [463, 1363]


@pytest.mark.parametrize("copy", ["wave", "lane"])
def test_open_copy_matrix(gpu, monkeypatch, copy):
    """copy_bytes_wave (k_dgram_open<true>) and, with VDS_EC_DGRAM_COPY=lane,
    the per-lane copy_bytes of k_dgram_open<false>, which no other test
    launches: one launch of 592 continuation datagrams, every payload length of
    _COPY_LENGTHS times every (src & 3, dst & 3) pair -- the three regimes of
    the copy (bytes before the destination's first dword, the dword loop
    i = lane; i < nd; i += 64, the tail bytes) at cnt < head, nd == 0, nd
    crossing 64 and 128, and all 16 alignment pairs, where the host form only
    ever gives src & 3 of 1 or 2.  Ten waves, so verified and forged datagrams
    (every seventh; header, payload and MAC by turns) are spread over several
    of them, with three sessions."""
    if copy == "lane":
        monkeypatch.setenv("VDS_EC_DGRAM_COPY", "lane")
    else:
        monkeypatch.delenv("VDS_EC_DGRAM_COPY", raising=False)
    rng = np.random.default_rng(1234)
    combos = [(p, sa, da) for p in _COPY_LENGTHS for sa in range(4) for da in range(4)]
    combos = [combos[int(x)] for x in rng.permutation(len(combos))]
    assert len(combos) == 592
    items = []
    for j, (p, sa, da) in enumerate(combos):
        ses = j % 3
        dg = _cont(KEYS[ses], 70000 + j, rng.integers(0, 256, p, dtype=np.uint8).tobytes())
        forged = j % 7 == 3
        if forged:
            dg = _forge(dg, 5, j // 7, j)
        items.append((dg, ses, 5, sa, da, forged))
    _open_check(items, 3)


@pytest.mark.parametrize("count", [63, 64, 65, 128, 129, 192])
def test_open_wave_boundaries(gpu, count):
    """k_dgram_open with one wave short of full, exactly full (count % 64 == 0:
    no idle lane joins the ballot), one lane into the next wave, and two and
    three waves.  The datagrams have distinct lengths from 38 to 600, so the
    host's order_by_blocks reordering is not the identity and a verdict or a
    payload written through the wrong ln.index would show; two sessions.
    Forged: one datagram in the first wave, the one at the last lane of every
    full wave, and the last lane of the launch (the positions are the host's,
    restated here: most compressions first, equal counts in the caller's
    order)."""
    rng = np.random.default_rng(4000 + count)
    lens = [int(x) for x in rng.choice(np.arange(38, 601), count, replace=False)]
    order = sorted(range(count), key=lambda j: -((lens[j] + 8) // 64))  # (stable, as the host's)
    assert order != list(range(count))
    forged = {order[3], order[count - 1]} | {order[64 * k - 1] for k in range(1, count // 64 + 1)}
    items = []
    for j, L in enumerate(lens):
        ses = (j // 3) % 2
        dg = _cont(KEYS[ses], 9 * j + 1, rng.integers(0, 256, L - 37, dtype=np.uint8).tobytes())
        if j in forged:
            dg = _forge(dg, 5, j, j // 3)
        items.append((dg, ses, 5, j % 4, (j // 4) % 4, j in forged))
    _open_check(items, 2)


def test_open_jumbo(gpu):
    """The largest datagram the entry point accepts: 65,535 bytes (1,024
    compressions in one lane, a wave copy of 65,498 bytes), with one of 9,000
    and one of 33 bytes (hdr_len 1: nothing to copy) in the same launch, to
    destinations at dst & 3 of 1, 2, 3.  Then the same launch with the last
    payload byte of the large one flipped: verdict 1 and its range untouched."""
    rng = np.random.default_rng(65535)
    big = _cont(KEYS[1], 0xFFFFFFFF, rng.integers(0, 256, 65498, dtype=np.uint8).tobytes())
    mid = _cont(KEYS[0], 77, rng.integers(0, 256, 9000 - 37, dtype=np.uint8).tobytes())
    tiny = b"\x27" + mac(KEYS[1], b"\x27")
    assert (len(big), len(mid), len(tiny)) == (65535, 9000, 33)
    flipped = bytearray(big)
    flipped[65535 - 33] ^= 0x80
    for first, forged in ((big, False), (bytes(flipped), True)):
        _open_check([(first, 1, 5, 2, 1, forged), (mid, 0, 5, 0, 2, False), (tiny, 1, 1, 3, 3, False)], 2)


# ------------------------------------------------------------------ sealing
def _seal_check(msgs, routes, types, ses, i0, mtus, nkeys, pitch):
    """One dgram_seal_batch_device launch against seal_ref: the whole slab,
    guard bytes between and after the datagrams included; messages at start
    offsets 0..3 from a dword, routes likewise; every third message's slot from
    a 16-byte aligned address, the others wherever they fall.  Returns the
    restatement's datagrams."""
    import torch
    from vds_amd import chunk
    n = len(msgs)
    want = [seal_ref(KEYS[s], mtu, t, i, rt, m) for s, mtu, t, i, rt, m in zip(ses, mtus, types, i0, routes, msgs)]
    for i, w in enumerate(want):  # the layout call says the same
        cnt, c0, last = chunk.dgram_layout(mtus[i], len(routes[i]), len(msgs[i]))
        assert (cnt, last) == (len(w), len(w[-1])) and all(len(x) == mtus[i] for x in w[:-1]), i
        assert i0[i] + cnt <= 1 << 32
    mbuf, mptr = place(torch, msgs, [i % 4 for i in range(n)])
    rbuf, rptr = place(torch, routes, [(i // 4) % 4 for i in range(n)])
    start, at = [], 16
    for i, w in enumerate(want):
        if i % 3 == 0:
            at = (at + 15) // 16 * 16
        start.append(at)
        at += len(w) * pitch + 5
    slab = torch.full((at + 16,), GUARD, dtype=torch.uint8, device="cuda")
    assert slab.data_ptr() % 16 == 0
    exp = np.full(at + 16, GUARD, dtype=np.uint8)
    for s0, w in zip(start, want):
        for d, dg in enumerate(w):
            exp[s0 + d * pitch:s0 + d * pitch + len(dg)] = np.frombuffer(dg, dtype=np.uint8)
    chunk.dgram_seal_batch_device(mptr, [len(m) for m in msgs], types, i0, rptr, [len(r) for r in routes], ses,
                                  KEYS[:nkeys], mtus, [slab.data_ptr() + s0 for s0 in start], pitch)
    torch.cuda.synchronize()
    got = slab.cpu().numpy()
    diff = np.nonzero(got != exp)[0]
    assert diff.size == 0, (diff[:8], [(i, s0) for i, s0 in enumerate(start) if s0 <= diff[0]][-1:],
                            [len(m) for m in msgs])
    return want


@pytest.mark.parametrize("mtu,hops", [(508, 4), (508, 5), (508, 13), (1400, 20), (1400, 40), (65535, 255)])
def test_seal_long_routes(gpu, mtu, hops):
    """Proxied routes of 4 hops and more (r = 33 + 32 hops: 161, 193, 449 at
    mtu 508 -- 13 hops leave 18 payload bytes in the first datagram; 673, 1313
    at 1400; 8193, the 255 hops the format allows, at 65535).  From stream byte
    5 or 9 such a route covers whole 64-byte blocks with their 17th dword, so
    seg_block takes its seg_whole path for the route, which the routes of 0,
    32, 33 and 97 bytes of the other tests never do; the routes start at
    offsets 0..3 from a dword, so every selector of that path is used.  The
    message lengths are _seal_cases' (at mtu 65535 with 8 of its random ones:
    the named lengths already give 28 datagrams of 65,535 bytes)."""
    r = 33 + 32 * hops
    rng = np.random.default_rng(mtu * 1000 + r)
    lens = _seal_cases(rng, mtu, r)
    if mtu == 65535:
        lens = lens[:-62]
    assert min(lens) >= 0
    n = len(lens)
    msgs = [rng.integers(0, 256, m, dtype=np.uint8).tobytes() for m in lens]
    routes = [route_blob(rng, r) for _ in range(n)]
    assert all(len(rt) == r and rt[32] == hops for rt in routes)
    types = [int(x) for x in rng.integers(0, 32, n)]
    ses = [int(x) for x in rng.integers(0, 2, n)]
    i0 = [int(x) for x in rng.integers(0, 1 << 31, n)]
    # stream block 1 and its 17th dword lie inside the route wherever it starts (seg_whole)
    assert 9 <= 64 and 64 + 68 <= 5 + r
    pitch = mtu + {4: 0, 5: 3, 13: 4, 20: 5, 40: 8, 255: 1}[hops]
    want = _seal_check(msgs, routes, types, ses, i0, [mtu] * n, 2, pitch)
    assert any(len(w) == 1 for w in want) and any(len(w) > 2 for w in want)


def test_seal_message_owning_waves(gpu):
    """wave_msg and the binary search of k_dgram_seal where one message owns
    whole waves: 37 single-datagram messages, then one of 200 datagrams (first
    lane 37: it owns waves 1 and 2 entirely, wave_msg[1] == wave_msg[2] ==
    wave_msg[3], and ends in wave 3), 19 singles up to lane 255, a message of
    three datagrams whose first lane is exactly 64 * 4, and 70 more singles.
    The longest message of the other tests has five datagrams.  index0 of the
    long message is 0x0000FF80, so its index carries across a byte inside it."""
    from vds_amd import chunk
    rng = np.random.default_rng(200)
    mtu, c0, per = 508, 467, 471
    lens = [int(x) for x in rng.integers(0, 471, 37)] + [c0 + 198 * per + 100] + \
        [int(x) for x in rng.integers(0, 471, 19)] + [c0 + per + 7] + [int(x) for x in rng.integers(0, 471, 70)]
    n = len(lens)
    counts = [chunk.dgram_layout(mtu, 0, m)[0] for m in lens]
    first = np.concatenate([[0], np.cumsum(counts)])
    assert counts[37] == 200 and first[37] == 37 and first[38] == 237 and counts[57] == 3 and first[57] == 256
    assert all(c == 1 for i, c in enumerate(counts) if i not in (37, 57)) and first[-1] == 329
    msgs = [rng.integers(0, 256, m, dtype=np.uint8).tobytes() for m in lens]
    i0 = [int(x) for x in rng.integers(0, 1 << 31, n)]
    i0[37] = 0x0000FF80
    want = _seal_check(msgs, [b""] * n, [int(x) for x in rng.integers(0, 32, n)], [i % 2 for i in range(n)], i0,
                       [mtu] * n, 2, 512)
    assert want[37][128][1:5] == be32(0x00010000)


def test_seal_mixed_launch(gpu):
    """Per-message mtu, route length, session and so datagram count in ONE
    launch (the other device-level seal tests pass [mtu] * n and [r] * n): 60
    messages, mtu from 508, 509, 1400, 9000, route length from 0, 32, 33, 97,
    193, three sessions, lengths from nothing to three datagrams' worth, one
    pitch of 9008 for all."""
    rng = np.random.default_rng(60)
    n = 60
    mtus = [(508, 509, 1400, 9000)[i % 4] for i in range(n)]
    rls = [(0, 32, 33, 97, 193)[i % 5] for i in range(n)]
    ses = [i % 3 for i in range(n)]
    lens = [int(rng.integers(0, 3 * mtus[i])) for i in range(n)]
    lens[0] = 0
    lens[7] = mtus[7] - 37 - rls[7]  # the smallest split
    lens[13] = mtus[13] - 38 - rls[13]  # the largest single
    msgs = [rng.integers(0, 256, m, dtype=np.uint8).tobytes() for m in lens]
    routes = [route_blob(rng, r) for r in rls]
    want = _seal_check(msgs, routes, [int(x) for x in rng.integers(0, 32, n)], ses,
                       [int(x) for x in rng.integers(0, 1 << 31, n)], mtus, 3, 9008)
    assert len(want[7]) == 2 and len(want[13]) == 1
    assert len({(mtus[i], rls[i]) for i in range(n)}) == 20  # every mtu with every route length


def test_seal_then_open_jumbo(gpu):
    """mtu 65535 on the device, which only vds_ec_dgram_layout's CPU test
    knew: one message of 2 * 65535 bytes sealed into a slab (three datagrams,
    two of 65,535 bytes), compared with seal_ref, then opened from that slab
    into a fresh guarded buffer and compared with the message."""
    import torch
    from vds_amd import chunk
    rng = np.random.default_rng(131070)
    mtu, pitch, m = 65535, 65536 + 16, 2 * 65535
    msg = rng.integers(0, 256, m, dtype=np.uint8).tobytes()
    want = seal_ref(KEYS[2], mtu, 21, 0x00FFFFFF, b"", msg)
    assert [len(w) for w in want] == [65535, 65535, 37 + m - (mtu - 41) - (mtu - 37)]
    assert chunk.dgram_layout(mtu, 0, m) == (3, mtu - 41, len(want[2]))
    mbuf, mptr = place(torch, [msg], [3])
    slab = torch.full((16 + 3 * pitch + 16,), GUARD, dtype=torch.uint8, device="cuda")
    exp = np.full(slab.numel(), GUARD, dtype=np.uint8)
    for d, dg in enumerate(want):
        exp[16 + d * pitch:16 + d * pitch + len(dg)] = np.frombuffer(dg, dtype=np.uint8)
    chunk.dgram_seal_batch_device(mptr, [m], [21], [0x00FFFFFF], [0], [0], [2], KEYS, [mtu], [slab.data_ptr() + 16],
                                  pitch)
    torch.cuda.synchronize()
    sealed = slab.cpu().numpy()
    assert np.array_equal(sealed, exp), np.nonzero(sealed != exp)[0][:8]
    out = torch.full((8 + 3 + m + 8,), GUARD, dtype=torch.uint8, device="cuda")
    vd = torch.full((3 + 2,), GUARD, dtype=torch.uint8, device="cuda")
    hdr = [9, 5, 5]
    dst, at = [], out.data_ptr() + 11
    for d, dg in enumerate(want):
        dst.append(at)
        at += len(dg) - 32 - hdr[d]
    chunk.dgram_open_batch_device([slab.data_ptr() + 16 + d * pitch for d in range(3)], [len(w) for w in want], hdr,
                                  [2, 2, 2], KEYS, dst, vd.data_ptr() + 1)
    torch.cuda.synchronize()
    assert vd.cpu().tolist() == [GUARD, 0, 0, 0, GUARD]
    got = out.cpu().numpy()
    assert (got[:11] == GUARD).all() and (got[11 + m:] == GUARD).all() and got[11:11 + m].tobytes() == msg
    assert np.array_equal(slab.cpu().numpy(), exp)  # opening writes nothing into the datagrams


# --------------------------------------------------------------- HMAC batch
def test_hmac_batch_comparison_sort(gpu):
    """order_by_blocks sorts by comparison, not by counting, when the longest
    message's block count exceeds 4 * count + 4096; the longest message of the
    other tests has 199 bytes.  Six messages of 300,000, 0, 64, 263,737, 55 and
    1 bytes (4,687 blocks against 4 * 6 + 4096 = 4,120) at start offsets 0..3:
    the MACs at the caller's indices, so the reordering must not show."""
    import torch
    from vds_amd import chunk
    lens = [300000, 0, 64, 263737, 55, 1]
    assert (max(lens) + 8) // 64 > 4 * len(lens) + 4096  # the comparison-sort branch
    rng = np.random.default_rng(300000)
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    ses = [0, 1, 2, 2, 1, 0]
    buf, ptrs = place(torch, msgs, [0, 1, 2, 3, 0, 1])
    macs = torch.full((32 + 6 * 32 + 32,), GUARD, dtype=torch.uint8, device="cuda")
    chunk.hmac_sha256_batch_device(ptrs, lens, ses, KEYS, macs.data_ptr() + 32)
    torch.cuda.synchronize()
    got = macs.cpu().numpy()
    assert (got[:32] == GUARD).all() and (got[32 + 192:] == GUARD).all()
    for j in range(6):
        assert got[32 + 32 * j:64 + 32 * j].tobytes() == mac(KEYS[ses[j]], msgs[j]), j


def test_hmac_batch_store_and_check(gpu):
    """macs and expected / verdicts given together: k_hmac_sha256_batch stores
    and checks in one launch (the other test does one or the other).  130
    messages of lengths 0..129, three waves; every fifth expected MAC has one
    bit flipped."""
    import torch
    from vds_amd import chunk
    n = 130
    rng = np.random.default_rng(130)
    msgs = [rng.integers(0, 256, m, dtype=np.uint8).tobytes() for m in range(n)]
    ses = [(j // 2) % 3 for j in range(n)]
    want = [mac(KEYS[s], m) for s, m in zip(ses, msgs)]
    exp = np.frombuffer(b"".join(want), dtype=np.uint8).copy()
    bad = list(range(2, n, 5))
    for j in bad:
        exp[32 * j + (7 * j) % 32] ^= 1 << (j % 8)
    buf, ptrs = place(torch, msgs, [(j // 3) % 4 for j in range(n)])
    e = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), exp])).cuda()  # an odd address
    macs = torch.full((32 + n * 32 + 32,), GUARD, dtype=torch.uint8, device="cuda")
    vd = torch.full((n + 2,), GUARD, dtype=torch.uint8, device="cuda")
    chunk.hmac_sha256_batch_device(ptrs, list(range(n)), ses, KEYS, macs.data_ptr() + 32, e.data_ptr() + 3,
                                   vd.data_ptr() + 1)
    torch.cuda.synchronize()
    got, v = macs.cpu().numpy(), vd.cpu().numpy()
    assert (got[:32] == GUARD).all() and (got[32 + 32 * n:] == GUARD).all()
    assert got[32:32 + 32 * n].tobytes() == b"".join(want)
    assert v[0] == GUARD and v[n + 1] == GUARD
    assert [j for j in range(n) if v[1 + j]] == bad and set(v[1:n + 1].tolist()) <= {0, 1}
    assert np.array_equal(e.cpu().numpy()[3:], exp)  # expected is read, never written
