"""save_temp for a batch of bodies of different sizes
(vds_ec_save_temp16_batch_device / _host_batch): the batched encode, then
every replica's SHA-256 name and every body's SHA-256 in one hash launch
(dht_network_client.cpp:62-107, server_api.cpp:16).  Replica bytes are checked
against the oracle (chunk.h:245-281), names and body hashes against hashlib
over the oracle's bytes, the host form against the already-tested
chunk.save_temp.

Layout of the device tests: the bodies in ONE device buffer (gaps filled with
0xA5), every replica in its own slice of ONE output buffer between 0x5A
canaries, the two digest arrays each between 0x5A guards."""
import hashlib

import numpy as np
import pytest

import oracle_ctypes as O

pytestmark = pytest.mark.gpu

SHAPES = [(16, 20), (32, 40), (32, 64), (3, 5)]  # the three batch shapes and one that takes encode_device
CANARY = 64
GUARD = 64


def _sizes(k):
    B = 2 * k
    G = 128 * B  # one 128-stripe group
    return [0, 1, B - 1, B, B + 1, 4095, 4096, 65536, 65537, 70001, G - 1, G, G + 1]


class Batch:
    """layout: "slab" -- object o's replicas equally spaced (one descriptor an
    object); "scattered" -- two of them swapped (no common pitch: a pointer
    table); "odd" -- as slab, but object 1's replicas at odd addresses and
    object 2's body at an address = 2 mod 4 (both take encode_device; the
    names are hashed from unaligned bytes)."""

    def __init__(self, torch, k, n, sizes, layout, seed):
        from vds_amd import chunk
        self.torch, self.k, self.n, self.sizes = torch, k, n, [int(s) for s in sizes]
        rng = np.random.default_rng(seed)
        self.L = [chunk.replica_size(k, s) for s in self.sizes]
        in_off, pos = [], 0
        for o, s in enumerate(self.sizes):
            pos = (pos + 15) // 16 * 16 + 16 + (2 if layout == "odd" and o == 2 else 0)
            in_off.append(pos)
            pos += s
        host_in = np.full(pos + 64, 0xA5, dtype=np.uint8)
        self.data = []
        for s, off in zip(self.sizes, in_off):
            d = rng.integers(1, 256, s, dtype=np.uint8)
            host_in[off:off + s] = d
            self.data.append(d)
        self.out_off, pos = [], 0
        for o, L in enumerate(self.L):
            slot = 2 * CANARY + L
            order = list(range(n))
            if layout == "scattered":
                order[1], order[n - 2] = order[n - 2], order[1]
            base = pos + (1 if layout == "odd" and o == 1 else 0)
            self.out_off.append([base + order[i] * slot + CANARY for i in range(n)])
            pos += n * slot + 2
        self.out_bytes = pos + 2
        self.d_in = torch.from_numpy(host_in).cuda()
        self.ins = [self.d_in.data_ptr() + off for off in in_off]
        self.want = [[O.encode(k, r, d) for r in range(n)] for d in self.data]

    def run(self, body_digests=True, stream=None):
        """One call; returns (replica bytes, names, body digests or None) after checking every guard."""
        from vds_amd import chunk
        torch, n, count = self.torch, self.n, len(self.sizes)
        out = torch.full((self.out_bytes,), 0x5A, dtype=torch.uint8, device="cuda")
        rd = torch.full((2 * GUARD + 32 * count * n,), 0x5A, dtype=torch.uint8, device="cuda")
        dd = torch.full((2 * GUARD + 32 * count,), 0x5A, dtype=torch.uint8, device="cuda")
        ptrs = [[out.data_ptr() + off for off in row] for row in self.out_off]
        chunk.save_temp_batch_device(self.k, n, self.ins, self.sizes, ptrs, rd.data_ptr() + GUARD,
                                     dd.data_ptr() + GUARD if body_digests else None, stream=stream)
        torch.cuda.synchronize()
        rd, dd = rd.cpu().numpy(), dd.cpu().numpy()
        assert (rd[:GUARD] == 0x5A).all() and (rd[GUARD + 32 * count * n:] == 0x5A).all(), "name guards written"
        if body_digests:
            assert (dd[:GUARD] == 0x5A).all() and (dd[GUARD + 32 * count:] == 0x5A).all(), "body guards written"
        else:
            assert (dd == 0x5A).all(), "body digests written although none were asked for"
        return out.cpu().numpy(), rd[GUARD:GUARD + 32 * count * n].reshape(count, n, 32), \
            dd[GUARD:GUARD + 32 * count].reshape(count, 32) if body_digests else None

    def check(self, got, names, bodies):
        for o, d in enumerate(self.data):
            for r in range(self.n):
                off, L, ref = self.out_off[o][r], self.L[o], self.want[o][r]
                assert ref.size == L
                assert np.array_equal(got[off:off + L], ref), (self.sizes[o], o, r)
                assert (got[off - CANARY:off] == 0x5A).all(), ("canary before", self.sizes[o], o, r)
                assert (got[off + L:off + L + CANARY] == 0x5A).all(), ("canary after", self.sizes[o], o, r)
                assert bytes(names[o, r]) == hashlib.sha256(ref.tobytes()).digest(), ("name", self.sizes[o], o, r)
            if bodies is not None:
                assert bytes(bodies[o]) == hashlib.sha256(d.tobytes()).digest(), ("body", self.sizes[o], o)


@pytest.mark.parametrize("layout", ["slab", "scattered", "odd"])
@pytest.mark.parametrize("k,n", SHAPES)
def test_replicas_names_and_body_digests(gpu, k, n, layout):
    import torch
    from vds_amd import chunk
    b = Batch(torch, k, n, _sizes(k), layout, seed=100 * k + n)
    if (k, n) != (3, 5):  # the layouts reach the routes they are meant for
        ptrs = [[0x10000 + off for off in row] for row in b.out_off]
        fast = sum(1 for s in b.sizes if s) - (2 if layout == "odd" else 0)
        assert chunk.encode_batch_path(k, list(range(n)), b.ins, b.sizes, ptrs) == (2, fast)
    b.check(*b.run())
    b.check(*b.run(body_digests=False))


def test_waves_span_objects(gpu):
    """n = 20 and 7 objects of different sizes: 140 replica lanes and 7 body
    lanes, so waves span objects; every digest at the caller's index."""
    import torch
    b = Batch(torch, 16, 20, [70001, 3, 4096, 65537, 0, 33000, 1500], "slab", seed=7)
    b.check(*b.run())
    b = Batch(torch, 16, 20, [70001, 3, 4096, 65537, 0, 33000, 1500], "scattered", seed=8)
    b.check(*b.run(stream=torch.cuda.Stream()))


@pytest.mark.parametrize("k,n", [(32, 64), (16, 20)])
def test_host_batch(gpu, k, n):
    from vds_amd import chunk
    rng = np.random.default_rng(k + n)
    bodies = [rng.integers(0, 256, s, dtype=np.uint8) for s in (0, 1, 63, 64, 65, 4095, 65536, 70001)]
    got = chunk.save_temp_batch(k, n, bodies)
    assert len(got) == len(bodies)
    for body, (reps, names, body_hash, rsize) in zip(bodies, got):
        w_reps, w_names, w_hash, w_rsize = chunk.save_temp(k, n, body)
        assert rsize == w_rsize == chunk.replica_size(k, body.size)
        assert body_hash == w_hash == hashlib.sha256(body.tobytes()).digest(), body.size
        assert names == w_names, body.size
        for r in range(n):
            assert np.array_equal(reps[r], w_reps[r]), (body.size, r)
            assert names[r] == hashlib.sha256(reps[r].tobytes()).digest(), (body.size, r)


def test_host_batch_beyond_one_staging_group(gpu):
    """Three bodies of 24 MiB + 5 bytes: more than one 64 MiB staging group."""
    from vds_amd import chunk
    k, n = 16, 20
    rng = np.random.default_rng(24)
    bodies = [rng.integers(0, 256, (24 << 20) + 5, dtype=np.uint8) for _ in range(3)]
    got = chunk.save_temp_batch(k, n, bodies)
    for body, (reps, names, body_hash, rsize) in zip(bodies, got):
        w_reps, w_names, w_hash, w_rsize = chunk.save_temp(k, n, body)
        assert rsize == w_rsize
        assert body_hash == w_hash
        assert names == w_names
        for r in range(n):
            assert np.array_equal(reps[r], w_reps[r]), r
