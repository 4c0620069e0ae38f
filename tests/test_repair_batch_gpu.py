"""The repair loop for a ragged batch in one call (vds_ec_repair16_batch_device
/ _host_batch: regenerate the lost replicas, name them, compare the names with
the catalogue's; sync_process.cpp:313-335 -> restore_async -> save_data,
dht_network_client.cpp:582-658) and vds_ec_sha256_check_batch_device.  Replica
bytes against the oracle (chunk.h:402-444 then chunk.h:245-281), names against
Python's hashlib (OpenSSL, as the reference's hash::sha256).  Bit-exact."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle_ctypes as O

SEED = 0x7664730000000000
pytestmark = pytest.mark.gpu
NT = 2
GUARD = 61  # guard bytes either side (odd: the arrays between them are unaligned)
SHAPES = [(16, 20), (32, 40), (32, 64), (3, 5)]


def _sizes(k):
    tile = 2048 * 2 * k  # sub-stripe, ragged, just past one half tile, the live size
    return [1, 2 * k * 9 + 1, tile // 2 + 1, 65536]


def _objects(torch, k, n, sizes, seed):
    """Encode objects of the given sizes (all n replicas, oracle-checked
    encode path) into separate device buffers: [(host bytes, [n tensors])]."""
    from vds_amd import chunk
    out = []
    for i, size in enumerate(sizes):
        host = O.splitmix(SEED + seed + i, size)
        t = torch.from_numpy(host.copy()).cuda()
        L = chunk.replica_size(k, size)
        reps = [torch.zeros(L, dtype=torch.uint8, device="cuda") for _ in range(n)]
        chunk.encode_device(k, list(range(n)), t, size, size, 1, [r.data_ptr() for r in reps], L)
        out.append((host, reps))
    return out


def _survivors(rng, k, n, i):
    """restore_async's choice, the first k replica ids found, with two or more
    of the first replicas lost; n = 64: enough of them that the survivors
    reach ids >= 40 (the runtime-coefficient route).  Two lost ids to repair."""
    pool = min(n, k + k // 4) if n > k + 2 else n
    lost = int(rng.integers(pool - k + 1, pool - k + 4)) if n == 64 else int(rng.integers(NT, n - k + 1))
    gone = set(rng.choice(pool, lost, replace=False).tolist())
    nd = [r for r in range(n) if r not in gone][:k]
    if i % 2:
        nd = [int(x) for x in rng.permutation(nd)]
    tg = sorted(rng.choice(sorted(gone), NT, replace=False).tolist())
    return nd, tg


class _Outs:
    """nt output buffers an object between 0x5A guards.  layout 0: equally
    spaced in one allocation; 1: the two in swapped order (a negative pitch)."""

    def __init__(self, torch, L, nt, layout):
        self.L, self.nt = L, nt
        self.slot = L + 2 * 14
        self.buf = torch.full((nt * self.slot,), 0x5A, dtype=torch.uint8, device="cuda")
        order = list(range(nt)) if layout == 0 else list(range(nt))[::-1]
        self.off = [14 + s * self.slot for s in order]
        self.ptrs = [self.buf.data_ptr() + o for o in self.off]

    def check(self, want, what):
        got = self.buf.cpu().numpy()
        mask = np.ones(got.size, dtype=bool)
        for i, o in enumerate(self.off):
            assert np.array_equal(got[o:o + self.L], want[i]), (what, i)
            mask[o:o + self.L] = False
        assert (got[mask] == 0x5A).all(), (what, "guard bytes written")


def _guarded(torch, nbytes):
    return torch.full((2 * GUARD + nbytes,), 0x5A, dtype=torch.uint8, device="cuda")


def _inner(t, nbytes):
    got = t.cpu().numpy()
    assert (got[:GUARD] == 0x5A).all() and (got[GUARD + nbytes:] == 0x5A).all(), "guard bytes written"
    return got[GUARD:GUARD + nbytes]


def _names(replicas):
    return [hashlib.sha256(r.tobytes()).digest() for r in replicas]


def _dev_bytes(torch, names):
    """The names back to back on the device at an odd address: (keep-alive tensor, address)."""
    raw = np.frombuffer(b"\x00" + b"".join(names), dtype=np.uint8).copy()
    t = torch.from_numpy(raw).cuda()
    return t, t.data_ptr() + 1


@pytest.mark.parametrize("k,n", SHAPES)
def test_bytes_and_names_every_route(gpu, k, n):
    """(16,20) and (32,40): the syndrome routes; (32,64): survivors past id 39,
    the runtime-coefficient route; (3,5): one launch per object.  Replicas
    equal the oracle's encode, names hashlib's at the caller's index; with the
    true names expected every verdict is 0, without them the verdict buffer is
    never written."""
    import torch
    from vds_amd import chunk
    rng = np.random.default_rng(1000 * k + n)
    sizes = _sizes(k)
    objs = _objects(torch, k, n, sizes, seed=3000 + k + n)
    nodes, targets, chunks, csz, want = [], [], [], [], []
    for i, (host, reps) in enumerate(objs):
        nd, tg = _survivors(rng, k, n, i)
        nodes.append(nd)
        targets.append(tg)
        chunks.append([reps[r].data_ptr() for r in nd])
        csz.append(reps[0].numel())
        want.append([O.encode(k, t, host) for t in tg])
    if n == 64:
        assert all(max(nd) >= 40 for nd in nodes)
    names = [x for w in want for x in _names(w)]
    count = len(sizes)
    ex_keep, ex_ptr = _dev_bytes(torch, names)
    stream = torch.cuda.Stream() if (k, n) == (32, 40) else None
    for with_expected in (False, True):
        outs = [_Outs(torch, L, NT, i % 2) for i, L in enumerate(csz)]
        dig = _guarded(torch, 32 * count * NT)
        ver = _guarded(torch, count * NT)
        torch.cuda.synchronize()  # (the fills, before a call on another stream)
        chunk.repair_batch_device(k, nodes, chunks, csz, targets, [o.ptrs for o in outs], dig.data_ptr() + GUARD,
                                  expected=ex_ptr if with_expected else None,
                                  verdicts=ver.data_ptr() + GUARD if with_expected else None, stream=stream)
        torch.cuda.synchronize()
        for o in range(count):
            outs[o].check(want[o], (k, n, sizes[o], nodes[o], targets[o]))
        got = _inner(dig, 32 * count * NT)
        for j, name in enumerate(names):
            assert bytes(got[32 * j:32 * j + 32]) == name, (k, n, j)
        v = ver.cpu().numpy()
        if with_expected:
            assert (_inner(ver, count * NT) == 0).all()
        else:
            assert (v == 0x5A).all(), "verdicts written without expected names"


def test_group_of_seventy_names_spans_two_waves(gpu):
    """k = 3, 70 targets an object: a group of the hash launch spans two waves;
    object 0's outputs are equally spaced (one descriptor), object 1's are
    shuffled (a pointer table).  One expected name of each object is wrong."""
    import torch
    from vds_amd import chunk
    k, nt = 3, 70
    rng = np.random.default_rng(70)
    sizes = [2 * k * 9 + 1, 1000]
    nodes = [[4, 0, 2], [1, 3, 5]]
    targets = [[t for t in range(100) if t not in nd][:nt] for nd in nodes]
    hosts = [O.splitmix(SEED + 7000 + i, s) for i, s in enumerate(sizes)]
    keep = [[torch.from_numpy(O.encode(k, r, h)).cuda() for r in nd] for nd, h in zip(nodes, hosts)]
    csz = [chunk.replica_size(k, s) for s in sizes]
    want = [[O.encode(k, t, h) for t in tg] for tg, h in zip(targets, hosts)]
    bufs = [torch.full((nt * (L + 6),), 0x5A, dtype=torch.uint8, device="cuda") for L in csz]
    slots = [list(range(nt)), [int(x) for x in rng.permutation(nt)]]
    ptrs = [[b.data_ptr() + s * (L + 6) for s in sl] for b, sl, L in zip(bufs, slots, csz)]
    names = [x for w in want for x in _names(w)]
    wrong = list(names)
    wrong[5] = bytes([names[5][0] ^ 1]) + names[5][1:]
    wrong[nt + 69] = names[nt + 69][:31] + bytes([names[nt + 69][31] ^ 0x80])
    ex_keep, ex_ptr = _dev_bytes(torch, wrong)
    dig = _guarded(torch, 32 * 2 * nt)
    ver = _guarded(torch, 2 * nt)
    chunk.repair_batch_device(k, nodes, [[b.data_ptr() for b in row] for row in keep], csz, targets, ptrs,
                              dig.data_ptr() + GUARD, expected=ex_ptr, verdicts=ver.data_ptr() + GUARD)
    torch.cuda.synchronize()
    for o in range(2):
        got = bufs[o].cpu().numpy().reshape(nt, csz[o] + 6)
        for i, s in enumerate(slots[o]):
            assert np.array_equal(got[s, :csz[o]], want[o][i]), (o, i)
        assert (got[:, csz[o]:] == 0x5A).all()
    got = _inner(dig, 32 * 2 * nt)
    assert [bytes(got[32 * j:32 * j + 32]) for j in range(2 * nt)] == names
    assert np.flatnonzero(_inner(ver, 2 * nt)).tolist() == [5, nt + 69]


def _three_objects(torch, k, n, seed):
    """Three objects, their survivors (host copies too) and two targets each."""
    rng = np.random.default_rng(seed)
    sizes = [2 * k * 9 + 1, 65536, 2048 * k + 1]
    objs = _objects(torch, k, n, sizes, seed=seed)
    nodes, targets = zip(*[_survivors(rng, k, n, i) for i in range(3)])
    surv = [[reps[r].cpu().numpy().copy() for r in nd] for (_, reps), nd in zip(objs, nodes)]
    true = [[O.encode(k, t, host) for t in tg] for (host, _), tg in zip(objs, targets)]
    return sizes, objs, list(nodes), list(targets), surv, true


def _run(torch, chunk, k, nodes, targets, surv, expected_names):
    """One repair_batch_device call on the survivors `surv` (host arrays):
    (replicas per object, names, verdicts)."""
    count = len(nodes)
    keep = [[torch.from_numpy(c).cuda() for c in row] for row in surv]
    csz = [row[0].size for row in surv]
    outs = [_Outs(torch, L, NT, i % 2) for i, L in enumerate(csz)]
    ex_keep, ex_ptr = _dev_bytes(torch, expected_names)
    dig = _guarded(torch, 32 * count * NT)
    ver = _guarded(torch, count * NT)
    chunk.repair_batch_device(k, nodes, [[c.data_ptr() for c in row] for row in keep], csz, targets,
                              [o.ptrs for o in outs], dig.data_ptr() + GUARD, expected=ex_ptr,
                              verdicts=ver.data_ptr() + GUARD)
    torch.cuda.synchronize()
    got = _inner(dig, 32 * count * NT)
    return outs, [bytes(got[32 * j:32 * j + 32]) for j in range(count * NT)], _inner(ver, count * NT).tolist()


@pytest.mark.parametrize("k,n", [(16, 20), (32, 64)])
def test_corrupt_survivor_is_caught(gpu, k, n):
    """One bit of one cell of one survivor (not the first, not a trailer) of
    object 1 of 3 flipped: the code is MDS, so that stripe's cell changes in
    every other replica -- both verdicts of object 1 are 1, every verdict of
    objects 0 and 2 is 0.  The bytes are still the reference route's (restore,
    then re-encode, of the survivors as they are)."""
    import torch
    from vds_amd import chunk
    sizes, objs, nodes, targets, surv, true = _three_objects(torch, k, n, seed=5100 + k + n)
    cell = 2 * 517  # a stripe in the middle of the 64 KiB object
    surv[1][5][cell + 1] ^= 0x10
    # the oracle alone, beforehand: the corrupted route's replicas differ from the true ones
    ref = O.restore(k, nodes[1], surv[1])
    assert ref is not None and ref.size == sizes[1]
    corrupted = [O.encode(k, t, ref) for t in targets[1]]
    for c, t in zip(corrupted, true[1]):
        assert not np.array_equal(c, t) and np.array_equal(c[-2:], t[-2:])
    names = [x for w in true for x in _names(w)]
    outs, got_names, verdicts = _run(torch, chunk, k, nodes, targets, surv, names)
    assert verdicts == [0, 0, 1, 1, 0, 0]
    want = [true[0], corrupted, true[2]]
    for o in range(3):
        outs[o].check(want[o], (k, n, o))
    assert got_names == [x for w in want for x in _names(w)]


def test_wrong_trailer_on_a_later_survivor_is_not_seen(gpu):
    """The documented limit: the reference route reads the first survivor's
    trailer only (chunk.h:408), so a wrong trailer on survivor 3 changes no
    regenerated replica and no verdict."""
    import torch
    from vds_amd import chunk
    k, n = 32, 40
    sizes, objs, nodes, targets, surv, true = _three_objects(torch, k, n, seed=5300)
    for row in surv:
        row[3][-2:] = [0x12, 0x34]
    names = [x for w in true for x in _names(w)]
    outs, got_names, verdicts = _run(torch, chunk, k, nodes, targets, surv, names)
    assert verdicts == [0] * 6
    for o in range(3):
        outs[o].check(true[o], (o,))
    assert got_names == names


def test_sha256_check_batch_alone(gpu):
    """Every padding case and a long message at odd addresses, then 70 messages
    of one length (the launch spans two waves); expected at an odd address with
    two entries wrong, one in byte 0 only and one in byte 31 only: the verdicts
    are exactly those two.  digests None: check only, nothing else written."""
    import torch
    from vds_amd import chunk
    rng = np.random.default_rng(44)
    lengths = [0, 1, 55, 56, 64, 119, 120, 4095, 65538] + [100] * 70
    messages = [rng.integers(0, 256, length, dtype=np.uint8).tobytes() for length in lengths]
    offs, pos = [], 0
    for m in messages:
        pos = (pos + 15) // 16 * 16 + 16 + (1 if len(offs) % 2 else 3)
        offs.append(pos)
        pos += len(m)
    host = np.full(pos + 64, 0xA5, dtype=np.uint8)
    for m, off in zip(messages, offs):
        host[off:off + len(m)] = np.frombuffer(m, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 16 == 0
    count = len(messages)
    names = [hashlib.sha256(m).digest() for m in messages]
    wrong = list(names)
    bad = [7, 40]  # the 4095-byte message; one of the seventy
    wrong[7] = bytes([names[7][0] ^ 0x80]) + names[7][1:]
    wrong[40] = names[40][:31] + bytes([names[40][31] ^ 1])
    ex_keep, ex_ptr = _dev_bytes(torch, wrong)
    assert ex_ptr % 2 == 1
    ptrs = [dev.data_ptr() + off for off in offs]
    for with_digests in (False, True):
        dig = _guarded(torch, 32 * count)
        ver = _guarded(torch, count)
        chunk.sha256_check_batch_device(ptrs, lengths, ex_ptr, ver.data_ptr() + GUARD,
                                        digests=dig.data_ptr() + GUARD if with_digests else None)
        torch.cuda.synchronize()
        assert np.flatnonzero(_inner(ver, count)).tolist() == bad
        assert set(_inner(ver, count).tolist()) == {0, 1}
        if with_digests:
            got = _inner(dig, 32 * count)
            assert [bytes(got[32 * j:32 * j + 32]) for j in range(count)] == names
        else:
            assert (dig.cpu().numpy() == 0x5A).all(), "digests written in a check-only call"
    assert np.array_equal(dev.cpu().numpy(), host)


# --------------------------------------------------------------- the host form
def _host_call(k, nodes, surv, targets, expected):
    """vds_ec_repair16_host_batch through the C ABI: (replicas, names, verdicts, mismatches)."""
    from vds_amd import _lib
    count, nt = len(nodes), len(targets[0])
    nd = np.asarray(nodes, dtype=np.uint16).reshape(-1)
    tg = np.asarray(targets, dtype=np.uint16).reshape(-1)
    cs = np.asarray([row[0].size for row in surv], dtype=np.uint64)
    outs = [[np.full(int(c) + 8, 0x5A, dtype=np.uint8) for _ in range(nt)] for c in cs]
    cp = (C.c_void_p * (count * k))(*[c.ctypes.data for row in surv for c in row])
    op = (C.c_void_p * (count * nt))(*[o.ctypes.data for row in outs for o in row])
    dg = np.full(32 * count * nt + 8, 0x5A, dtype=np.uint8)
    vd = np.full(count * nt + 8, 0x5A, dtype=np.uint8)
    ex = np.frombuffer(b"".join(expected), dtype=np.uint8).copy() if expected is not None else None
    bad = C.c_uint32(12345)
    _lib.check(_lib.lib().vds_ec_repair16_host_batch(k, count, nd.ctypes.data_as(_lib.u16p), cp,
                                                     cs.ctypes.data_as(_lib.u64p), nt, tg.ctypes.data_as(_lib.u16p),
                                                     op, dg.ctypes.data, ex.ctypes.data if ex is not None else None,
                                                     vd.ctypes.data if ex is not None else None, C.byref(bad)),
               "repair16_host_batch")
    for row, c in zip(outs, cs):
        for o in row:
            assert (o[int(c):] == 0x5A).all()
    assert (dg[32 * count * nt:] == 0x5A).all() and (vd[count * nt:] == 0x5A).all()
    return ([[o[:int(c)] for o in row] for row, c in zip(outs, cs)],
            [bytes(dg[32 * j:32 * j + 32]) for j in range(count * nt)], vd[:count * nt].tolist(), bad.value)


@pytest.mark.parametrize("k,n", [(32, 64), (16, 20)])
def test_host_form(gpu, k, n):
    """From and to host memory, against regenerate_host plus hashlib object by
    object; one object has a corrupt survivor: its verdicts are set and
    `mismatches` counts them.  Without expected names nothing is compared."""
    import torch
    from vds_amd import chunk
    rng = np.random.default_rng(6000 + k + n)
    sizes = _sizes(k)
    objs = _objects(torch, k, n, sizes, seed=6100 + k + n)
    nodes, targets = zip(*[_survivors(rng, k, n, i) for i in range(len(sizes))])
    nodes, targets = list(nodes), list(targets)
    surv = [[reps[r].cpu().numpy().copy() for r in nd] for (_, reps), nd in zip(objs, nodes)]
    true_names = [x for (host, _), tg in zip(objs, targets) for x in _names([O.encode(k, t, host) for t in tg])]
    surv[3][k - 1][2 * 200] ^= 0x01  # the 64 KiB object, its last survivor
    want = [chunk.regenerate_host(k, nd, row, tg) for nd, row, tg in zip(nodes, surv, targets)]
    want_names = [x for w in want for x in _names(w)]
    reps, names, verdicts, bad = _host_call(k, nodes, surv, targets, true_names)
    for o in range(len(sizes)):
        for i in range(NT):
            assert np.array_equal(reps[o][i], want[o][i]), (k, n, o, i)
    assert names == want_names
    assert verdicts == [0] * (NT * 3) + [1] * NT and bad == NT
    reps2, names2, verdicts2, bad2 = _host_call(k, nodes, surv, targets, None)
    assert names2 == want_names and bad2 == 0 and verdicts2 == [0x5A] * (NT * 4)
    # the Python mirror: the same call from {id: bytes} mappings
    res = chunk.repair_batch(k, [dict(zip(nd, row)) for nd, row in zip(nodes, surv)], targets,
                             expected=[true_names[NT * o:NT * o + NT] for o in range(len(sizes))])
    for o, (r, nm, vd) in enumerate(res):
        assert all(np.array_equal(a, b) for a, b in zip(r, want[o]))
        assert nm == want_names[NT * o:NT * o + NT] and vd == verdicts[NT * o:NT * o + NT]
    assert chunk.repair_batch(k, [dict(zip(nodes[0], surv[0]))], [targets[0]])[0][2] is None


def test_host_form_beyond_one_staging_group(gpu):
    """Three objects of 24 MiB + 5 bytes at k = 16: 24 MiB of survivors each,
    so the 64 MiB staging group holds two of them and the call takes two."""
    from vds_amd import chunk
    k, size = 16, (24 << 20) + 5
    nodes = [[r for r in range(20) if r not in lost][:k] for lost in ((0, 7), (3, 19), (1, 2, 16))]
    targets = [[0, 7], [19, 3], [2, 16]]
    surv, want = [], []
    for i, (nd, tg) in enumerate(zip(nodes, targets)):
        body = O.splitmix(SEED + 8800 + i, size)
        reps = chunk.encode_host(k, nd + tg, body)
        surv.append([np.ascontiguousarray(r) for r in reps[:k]])
        want.append(reps[k:])
    assert sum(row[0].size * k for row in surv[:2]) <= 64 << 20 < sum(row[0].size * k for row in surv)
    true_names = [x for w in want for x in _names(w)]
    reps, names, verdicts, bad = _host_call(k, nodes, surv, targets, true_names)
    for o in range(3):
        for i in range(NT):
            assert np.array_equal(reps[o][i], want[o][i]), (o, i)
    assert names == true_names and verdicts == [0] * 6 and bad == 0
