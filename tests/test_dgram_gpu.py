"""The node-to-node datagram layer on the device: batched HMAC-SHA256, sealing
and opening of datagrams (vds_ec_hmac_sha256_batch_device,
vds_ec_dgram_seal_batch_device, vds_ec_dgram_open_batch_device and the host
forms).  The reference for every byte is Python's own hmac / hashlib (OpenSSL,
as the reference's hmac::signature) and a plain restatement of
dht_datagram_protocol::prepare_to_send (impl/dht_datagram_protocol.cpp:335-541)
written below.  Bit-exact."""
import hmac

import numpy as np
import pytest

import oracle_ctypes as O

pytestmark = pytest.mark.gpu
GUARD = 0x5A
KEYS = [bytes((37 * s + 11 * i + 1) & 0xFF for i in range(32)) for s in range(3)]


def mac(key, data):
    return hmac.digest(key, bytes(data), "sha256")


def be32(v):
    return int(v).to_bytes(4, "big")


def seal_ref(key, mtu, mtype, i0, route, msg):
    """prepare_to_send: the datagrams of one message (route = b"" direct, 32
    bytes routed, target + count + hops proxied)."""
    msg, r = bytes(msg), len(route)
    kind = 1 if r == 0 else 3 if r == 32 else 5  # SingleData 0x20, RouteSingleData 0x60, ProxySingleData 0xA0
    total = 1 + 4 + 32 + r + len(msg)
    if total < mtu:
        body = bytes([(kind << 5) | mtype]) + be32(i0) + route + msg
        return [body + mac(key, body)]
    off = mtu - (1 + 4 + 4 + 32 + r)
    body = bytes([((kind + 1) << 5) | mtype]) + be32(i0) + be32(len(msg)) + route + msg[:off]
    out = [body + mac(key, body)]
    index = i0 + 1
    while True:
        size = min(mtu - (1 + 4 + 32), len(msg) - off)
        body = b"\x03" + be32(index) + msg[off:off + size]
        out.append(body + mac(key, body))
        index += 1
        if off + size >= len(msg):
            return out
        off += size


def route_blob(rng, r):
    if r <= 32:
        return rng.integers(0, 256, r, dtype=np.uint8).tobytes()
    h = (r - 33) // 32
    return rng.integers(0, 256, 32, dtype=np.uint8).tobytes() + bytes([h]) + \
        rng.integers(0, 256, 32 * h, dtype=np.uint8).tobytes()


def place(torch, blobs, offsets):
    """The blobs in one device buffer, blob i at a dword plus offsets[i]:
    (tensor, [addresses])."""
    at, pos = 0, []
    for b, o in zip(blobs, offsets):
        at = (at + 3) // 4 * 4 + 4
        pos.append(at + o)
        at += o + len(b)
    host = np.full(at + 8, 0xEE, dtype=np.uint8)
    for b, p in zip(blobs, pos):
        host[p:p + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    t = torch.from_numpy(host).cuda()
    return t, [t.data_ptr() + p for p in pos]


def test_hmac_batch(gpu):
    """200 messages of lengths 0..199 (55, 56, 63, 64, 119, 120: the padding
    boundaries after the 64-byte pad block), start offsets 0..3 from a dword,
    3 sessions; then the check form with a quarter of the expected MACs flipped
    in one bit: exactly those verdicts are non-zero."""
    import torch
    from vds_amd import chunk
    rng = np.random.default_rng(5)
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in range(200)]
    ses = [j % 3 for j in range(200)]
    buf, ptrs = place(torch, msgs, [(j // 3) % 4 for j in range(200)])
    macs = torch.full((200 * 32 + 64,), GUARD, dtype=torch.uint8, device="cuda")
    chunk.hmac_sha256_batch_device(ptrs, [len(m) for m in msgs], ses, KEYS, macs.data_ptr() + 32)
    torch.cuda.synchronize()
    got = macs.cpu().numpy()
    want = [mac(KEYS[s], m) for s, m in zip(ses, msgs)]
    assert (got[:32] == GUARD).all() and (got[32 + 6400:] == GUARD).all()
    for j in range(200):
        assert got[32 + 32 * j:64 + 32 * j].tobytes() == want[j], j
    exp = np.frombuffer(b"".join(want), dtype=np.uint8).copy()
    bad = sorted(rng.choice(200, 50, replace=False).tolist())
    for j in bad:
        exp[32 * j + int(rng.integers(32))] ^= 1 << int(rng.integers(8))
    e = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), exp])).cuda()  # an odd address
    vd = torch.full((200 + 2,), GUARD, dtype=torch.uint8, device="cuda")
    chunk.hmac_sha256_batch_device(ptrs, [len(m) for m in msgs], ses, KEYS, None, e.data_ptr() + 1, vd.data_ptr() + 1)
    torch.cuda.synchronize()
    v = vd.cpu().numpy()
    assert v[0] == GUARD and v[201] == GUARD
    assert [j for j in range(200) if v[1 + j]] == bad and set(v[1:201].tolist()) <= {0, 1}


def _seal_cases(rng, mtu, r):
    """Message lengths from the rules: around the largest single message, the
    smallest split, and full / one-byte last continuations; plus random ones."""
    c0, per = mtu - (41 + r), mtu - 37
    ms = [0, 1, c0 + 3, c0 + 4, c0 + 5, c0 + per - 1, c0 + per, c0 + per + 1, c0 + 2 * per, c0 + 2 * per + 1,
          c0 + 3 * per + 270]
    if mtu == 508:  # the lengths the issue lists, shifted by r
        ms += [x - r for x in (470, 471, 472, 937, 938, 942, 943)] + [2154]
    ms += [int(x) for x in rng.integers(0, 3 * mtu, 70)]
    return ms


@pytest.mark.parametrize("mtu,r,pitch_pad", [(508, 0, 0), (508, 32, 4), (508, 97, 3), (509, 0, 0), (1400, 32, 8),
                                             (1400, 0, 5)])
def test_seal_against_restatement(gpu, mtu, r, pitch_pad):
    """Every datagram byte and every byte of the output slab outside the
    datagrams, for message start offsets 0..3, two sessions, an index that
    carries across bytes, aligned and unaligned slots, 130 datagrams or more."""
    import torch
    from vds_amd import chunk
    rng = np.random.default_rng(mtu * 1000 + r)
    lens = _seal_cases(rng, mtu, r)
    n = len(lens)
    msgs = [rng.integers(0, 256, m, dtype=np.uint8).tobytes() for m in lens]
    routes = [route_blob(rng, r) for _ in range(n)]
    types = [int(x) for x in rng.integers(0, 32, n)]
    ses = [int(x) for x in rng.integers(0, 2, n)]
    i0 = [int(x) for x in rng.integers(0, 1 << 32, n)]
    five = lens.index(mtu - (41 + r) + 3 * (mtu - 37) + 270)  # 5 datagrams: the index carries across its bytes
    i0[five] = 0xFFFFFFF0 if mtu != 509 else 0x00FFFFFE
    want = [seal_ref(KEYS[s], mtu, t, i, rt, m) for s, t, i, rt, m in zip(ses, types, i0, routes, msgs)]
    assert len(want[five]) == 5 and sum(len(w) for w in want) >= 130
    for i in range(n):  # an index past 2^32 is refused by the call: keep the random ones below
        if i0[i] + len(want[i]) > 1 << 32:
            i0[i] -= 1 << 16
            want[i] = seal_ref(KEYS[ses[i]], mtu, types[i], i0[i], routes[i], msgs[i])
    mbuf, mptr = place(torch, msgs, [i % 4 for i in range(n)])
    rbuf, rptr = place(torch, routes, [(i // 4) % 4 for i in range(n)])
    pitch = mtu + pitch_pad
    start, at = [], 16
    for i, w in enumerate(want):  # every third message from a 16-byte aligned address, the others wherever they fall
        if i % 3 == 0:
            at = (at + 15) // 16 * 16
        start.append(at)
        at += len(w) * pitch + 5
    slab = torch.full((at + 16,), GUARD, dtype=torch.uint8, device="cuda")
    assert slab.data_ptr() % 16 == 0
    exp = np.full(at + 16, GUARD, dtype=np.uint8)
    for s0, w in zip(start, want):
        for d, dg in enumerate(w):
            assert len(dg) <= mtu
            exp[s0 + d * pitch:s0 + d * pitch + len(dg)] = np.frombuffer(dg, dtype=np.uint8)
    chunk.dgram_seal_batch_device(mptr, lens, types, i0, rptr, [r] * n, ses, KEYS[:2], [mtu] * n,
                                  [slab.data_ptr() + s0 for s0 in start], pitch)
    torch.cuda.synchronize()
    got = slab.cpu().numpy()
    diff = np.nonzero(got != exp)[0]
    assert diff.size == 0, (diff[:8], [(i, s0) for i, s0 in enumerate(start) if s0 <= diff[0]][-1], lens)
    for i, w in enumerate(want):  # and the layout call says the same
        cnt, c0, last = chunk.dgram_layout(mtu, r, lens[i])
        assert (cnt, last) == (len(w), len(w[-1])) and all(len(x) == mtu for x in w[:-1])


def _sealed_batch(rng):
    """Messages of every route kind at mtu 508 and 1400, sealed by the
    restatement: [(session, route, msg, [datagrams], hdr of the first)]."""
    out = []
    for i, (mtu, r, m) in enumerate([(508, 0, 100), (508, 0, 470), (508, 0, 471), (508, 32, 2154), (508, 97, 943),
                                     (1400, 0, 5000), (1400, 32, 1300), (508, 33, 300), (508, 0, 0), (508, 32, 1)]):
        ses = i % 2
        route, msg = route_blob(rng, r), rng.integers(0, 256, m, dtype=np.uint8).tobytes()
        dgs = seal_ref(KEYS[ses], mtu, i % 32, 1000 * i + 7, route, msg)
        out.append((ses, route, msg, dgs, (5 if len(dgs) == 1 else 9) + r))
    return out


def test_open(gpu):
    """The sealed datagrams shuffled: every verdict 0 and every message
    reassembled bit-exact into a guarded buffer.  Then one bit flipped in the
    header, the payload or the MAC of chosen datagrams: exactly those verdicts
    are 1 and their payload ranges still hold the guard value.  A 32-byte
    datagram gives verdict 2."""
    import torch
    from vds_amd import chunk
    rng = np.random.default_rng(77)
    batch = _sealed_batch(rng)
    flat = []  # (datagram, session, hdr_len, message number, offset in its message)
    moff, at = [], 7
    for mi, (ses, route, msg, dgs, hdr) in enumerate(batch):
        moff.append(at)
        at += len(msg) + 9
        o = 0
        for d, dg in enumerate(dgs):
            h = hdr if d == 0 else 5
            flat.append((dg, ses, h, mi, o))
            o += len(dg) - 32 - h
        assert o == len(msg)
    total = at
    order = [int(x) for x in rng.permutation(len(flat))]
    flat = [flat[i] for i in order] + [(b"\x21" + bytes(31), 0, 0, None, 0)]  # and a 32-byte datagram
    n = len(flat)
    for mode in ("clean", "flipped"):
        dgs = [bytearray(f[0]) for f in flat]
        bad = []
        if mode == "flipped":
            for pick, j in enumerate(sorted(rng.choice(n - 1, 9, replace=False).tolist())):
                L, h = len(dgs[j]), flat[j][2]
                where = (int(rng.integers(0, h)), int(rng.integers(h, L - 32)) if L - 32 > h else 0,
                         int(rng.integers(L - 32, L)))[pick % 3]
                dgs[j][where] ^= 1 << int(rng.integers(8))
                bad.append(j)
        dbuf, dptr = place(torch, dgs, [j % 4 for j in range(n)])
        asm = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
        dst = [asm.data_ptr() + moff[f[3]] + f[4] if f[3] is not None else 0 for f in flat]
        vd = torch.full((n + 2,), GUARD, dtype=torch.uint8, device="cuda")
        chunk.dgram_open_batch_device(dptr, [len(d) for d in dgs], [f[2] for f in flat], [f[1] for f in flat],
                                      KEYS[:2], dst, vd.data_ptr() + 1)
        torch.cuda.synchronize()
        v = vd.cpu().numpy()
        assert v[0] == GUARD and v[n + 1] == GUARD
        assert v[n] == 2
        assert [j for j in range(n - 1) if v[1 + j] != 0] == bad and all(v[1 + j] == 1 for j in bad), mode
        exp = np.full(total, GUARD, dtype=np.uint8)
        for j, f in enumerate(flat[:-1]):
            if j not in bad:
                pay = f[0][f[2]:len(f[0]) - 32]
                exp[moff[f[3]] + f[4]:moff[f[3]] + f[4] + len(pay)] = np.frombuffer(pay, dtype=np.uint8)
        got = asm.cpu().numpy()
        assert np.array_equal(got, exp), (mode, np.nonzero(got != exp)[0][:8])
        if mode == "clean":
            for mi, (ses, route, msg, _, _) in enumerate(batch):
                assert got[moff[mi]:moff[mi] + len(msg)].tobytes() == msg


def test_open_verify_only(gpu):
    """dsts None: verdicts only."""
    import torch
    from vds_amd import chunk
    dgs = seal_ref(KEYS[1], 508, 3, 5, b"", bytes(range(256)) * 4)
    dgs[1] = dgs[1][:40] + bytes([dgs[1][40] ^ 0x10]) + dgs[1][41:]
    dbuf, dptr = place(torch, dgs, [1, 2, 3])
    vd = torch.full((3,), GUARD, dtype=torch.uint8, device="cuda")
    chunk.dgram_open_batch_device(dptr, [len(d) for d in dgs], [9, 5, 5], [0, 0, 0], KEYS[1:2], None, vd)
    assert vd.cpu().tolist() == [0, 1, 0]


def test_host_forms(gpu):
    """Seal then open a mixed batch through host memory: 2 sessions, all three
    route kinds, an MTUTest and an Acknowledgment datagram interleaved, one
    duplicate index (the first arrival wins), a message with a missing
    continuation (INCOMPLETE), a first datagram whose BE32(m) is no larger than
    its payload, re-signed with the right key (DATA), and a forged datagram
    (its message INCOMPLETE, its bytes not handed out)."""
    from vds_amd import _lib, chunk
    rng = np.random.default_rng(99)
    spec = [(0, 508, 0, 100), (1, 508, 32, 2154), (0, 508, 97, 943), (1, 1400, 0, 5000), (0, 508, 32, 471 - 32),
            (1, 508, 33, 0), (0, 509, 0, 1500), (1, 508, 0, 1200), (0, 508, 0, 1100)]
    msgs = [rng.integers(0, 256, m, dtype=np.uint8).tobytes() for _, _, _, m in spec]
    routes = [route_blob(rng, r) for _, _, r, _ in spec]
    i0 = [100 * (i + 1) for i in range(len(spec))]
    types = [(3 * i + 1) % 32 for i in range(len(spec))]
    ses = [s for s, _, _, _ in spec]
    sealed = chunk.dgram_seal_batch(msgs, types, i0, routes, ses, KEYS[:2], [mtu for _, mtu, _, _ in spec])
    for i in range(len(spec)):
        assert sealed[i] == seal_ref(KEYS[ses[i]], spec[i][1], types[i], i0[i], routes[i], msgs[i]), i
    # the socket batch
    arrivals = [(dg, ses[i]) for i in range(len(spec)) for dg in sealed[i]]
    arrivals = [arrivals[int(x)] for x in rng.permutation(len(arrivals))]
    # message 7 loses a continuation; message 8's second datagram is forged
    arrivals = [a for a in arrivals if a[0] != sealed[7][1]]
    forged = bytearray(sealed[8][1])
    forged[20] ^= 0x40
    arrivals = [(bytes(forged), s) if dg == sealed[8][1] else (dg, s) for dg, s in arrivals]
    # a first datagram announcing no more than it carries, properly signed (session 0, index 5000)
    body = bytes([0x40 | 9]) + be32(5000) + be32(467) + bytes(467)
    small = body + mac(KEYS[0], body)
    # a second, properly signed datagram at message 0's index: it arrives later and loses
    dup_body = bytes([0x20 | 1]) + be32(i0[0]) + b"another message"
    dup = dup_body + mac(KEYS[0], dup_body)
    arrivals.insert(3, (b"\x06" + bytes(700), 0))
    arrivals.insert(9, (b"\x07" + bytes(9), 1))
    arrivals += [(small, 0), (dup, 0)]
    vd, found = chunk.dgram_open_batch([a[0] for a in arrivals], [a[1] for a in arrivals], KEYS[:2])
    for j, (dg, s) in enumerate(arrivals):
        want = 3 if dg[0] in (6, 7) else 1 if dg == bytes(forged) else 0
        assert vd[j] == want, (j, vd[j], want)
    by = {(m["session"], m["index0"]): m for m in found}
    assert len(by) == len(found) == len(spec) + 1
    assert [(m["session"], m["index0"]) for m in found] == sorted(by)
    for i in range(len(spec)):
        m = by[(ses[i], i0[i])]
        assert m["type"] == types[i]
        if i == 7:
            assert m["status"] == _lib.EDGRAM_INCOMPLETE and m["message"] is None and m["dgrams"] == 1
        elif i == 8:
            assert m["status"] == _lib.EDGRAM_INCOMPLETE and m["message"] is None and m["route"] is None
        else:
            assert m["status"] == 0 and m["message"] == msgs[i] and m["route"] == routes[i], i
            assert m["dgrams"] == len(sealed[i])
    assert by[(0, 5000)]["status"] == _lib.EDGRAM_DATA and by[(0, 5000)]["message"] is None


def test_end_to_end_with_repair(gpu):
    """repair_batch_device on 4 objects at k = 16 with its outs pointing into
    sync_replica_data message slabs (object_id, the length prefix, the replica,
    owner, value_id, BE16(replica)); the messages are sealed, opened, and the
    replicas compared with the oracle's."""
    import torch
    from vds_amd import chunk
    k, n, SEED = 16, 20, 0x7664730000000000
    rng = np.random.default_rng(2024)
    sizes = [1, 2 * k * 9 + 1, 4097, 20000]
    nodes = [r for r in range(n) if r not in (0, 5)][:k]
    targets = [0, 5]
    surv, csz, hosts = [], [], []
    for i, size in enumerate(sizes):
        host = O.splitmix(SEED + 500 + i, size)
        hosts.append(host)
        L = chunk.replica_size(k, size)
        reps = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
        chunk.encode_device(k, list(range(n)), torch.from_numpy(host.copy()).cuda(), size, size, 1,
                            [reps[i].data_ptr() for i in range(n)], L)
        surv.append(reps)
        csz.append(L)
    # the message slabs: everything but the replica written by the host
    ids = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(3)]
    blobs, gap = [], []
    for o in range(4):
        for t in targets:
            head = chunk.write_number(32) + ids[0] + chunk.write_number(csz[o])
            tail = chunk.write_number(32) + ids[1] + chunk.write_number(32) + ids[2] + t.to_bytes(2, "big")
            blobs.append(head + bytes(csz[o]) + tail)
            gap.append(len(head))
    # (the gaps at even addresses, alternately 0 and 2 from a dword)
    mbuf, mptr = place(torch, blobs, [(2 * (i % 2) - gap[i]) % 4 for i in range(len(blobs))])
    digests = torch.zeros((8, 32), dtype=torch.uint8, device="cuda")
    chunk.repair_batch_device(k, [nodes] * 4, [[surv[o][r].data_ptr() for r in nodes] for o in range(4)], csz,
                              [targets] * 4, [[mptr[2 * o + i] + gap[2 * o + i] for i in range(2)] for o in range(4)],
                              digests)
    mtu, nm = 508, len(blobs)
    lay = [chunk.dgram_layout(mtu, 0, len(b)) for b in blobs]
    pitch = 512
    first = np.concatenate([[0], np.cumsum([c for c, _, _ in lay])]).astype(np.int64)
    slab = torch.full((int(first[-1]) * pitch,), GUARD, dtype=torch.uint8, device="cuda")
    i0 = [int(first[i]) for i in range(nm)]
    chunk.dgram_seal_batch_device(mptr, [len(b) for b in blobs], [17] * nm, i0, [0] * nm, [0] * nm, [0] * nm, KEYS[:1],
                                  [mtu] * nm, [slab.data_ptr() + int(first[i]) * pitch for i in range(nm)], pitch)
    # the receiver: every datagram of every message, payloads into fresh message buffers
    rbuf, rptr = place(torch, [bytes(len(b)) for b in blobs], [(i + 1) % 4 for i in range(nm)])
    dg, ln, hd, dst = [], [], [], []
    for i in range(nm):
        cnt, c0, last = lay[i]
        for d in range(cnt):
            dg.append(slab.data_ptr() + (int(first[i]) + d) * pitch)
            ln.append(last if d == cnt - 1 else mtu)
            hd.append((5 if cnt == 1 else 9) if d == 0 else 5)
            dst.append(rptr[i] + (0 if d == 0 else c0 + (d - 1) * (mtu - 37)))
    vd = torch.full((len(dg),), GUARD, dtype=torch.uint8, device="cuda")
    chunk.dgram_open_batch_device(dg, ln, hd, [0] * len(dg), KEYS[:1], dst, vd)
    torch.cuda.synchronize()
    assert not vd.cpu().numpy().any()
    got = rbuf.cpu().numpy()
    base = rbuf.data_ptr()
    for o in range(4):
        for i, t in enumerate(targets):
            j = 2 * o + i
            at = rptr[j] - base
            m = got[at:at + len(blobs[j])].tobytes()
            want = O.encode(k, t, hosts[o]).tobytes()
            assert m[:gap[j]] == blobs[j][:gap[j]] and m[gap[j] + csz[o]:] == blobs[j][gap[j] + csz[o]:]
            assert m[gap[j]:gap[j] + csz[o]] == want, (o, t)
