"""Batched encode of objects of different sizes in one launch
(vds_ec_encode16_batch_device): the upload loop's shape -- every body
save_temp encodes (dht_network_client.cpp:62-107) has its own length.  Bytes
are checked against the oracle (chunk.h:245-281) and against the per-object
vds_ec_encode16_device, which is itself oracle-tested.

Layout of every test: the objects' inputs in ONE device buffer (gaps filled
with 0xA5, the objects with non-zero random bytes, so a load past an object's
end gives wrong cells), every replica in its own slice of ONE output buffer
between two 64-byte 0x5A canaries (so a store past a replica's end, or before
its start, shows)."""
import numpy as np
import pytest

import oracle_ctypes as O

pytestmark = pytest.mark.gpu

SHAPES = [(16, 20), (32, 40), (32, 64)]
CANARY = 64


class Batch:
    """sizes[o] bytes per object.  in_mis[o]: the input's address mod 4;
    out_odd[o]: its replica slices start at odd addresses.  Replica slices of
    object o are equally spaced (o % 3 == 0), equally spaced in reverse order
    (1) or with two slices swapped (2: no common pitch), so both forms of the
    replica addresses are used."""

    def __init__(self, torch, k, n, sizes, seed, write_padding=True, in_mis=None, out_odd=None):
        from vds_amd import chunk
        self.torch, self.k, self.n, self.sizes, self.wp = torch, k, n, [int(s) for s in sizes], write_padding
        rng = np.random.default_rng(seed)
        in_mis = in_mis or [0] * len(sizes)
        out_odd = out_odd or [0] * len(sizes)
        self.L = [chunk.replica_size(k, s, 2, write_padding) for s in self.sizes]
        in_off, pos = [], 0
        for s, mis in zip(self.sizes, in_mis):
            pos = (pos + 3) // 4 * 4 + 8 + mis  # a gap, then the requested alignment
            in_off.append(pos)
            pos += s
        host_in = np.full(pos + 64, 0xA5, dtype=np.uint8)
        self.data = []
        for s, off in zip(self.sizes, in_off):
            d = rng.integers(1, 256, s, dtype=np.uint8)
            host_in[off:off + s] = d
            self.data.append(d)
        self.out_off, pos = [], 0
        for o, (L, odd) in enumerate(zip(self.L, out_odd)):
            slot = (2 * CANARY + L + 1) // 2 * 2
            order = list(range(n))
            if o % 3 == 1:
                order.reverse()
            elif o % 3 == 2:
                order[1], order[2] = order[2], order[1]
            base = pos + odd
            self.out_off.append([base + order[i] * slot + CANARY for i in range(n)])
            pos += n * slot + 2
        self.out_bytes = pos + 2
        self.d_in = torch.from_numpy(host_in).cuda()
        self.ins = [self.d_in.data_ptr() + off for off in in_off]

    def new_out(self):
        return self.torch.full((self.out_bytes,), 0x5A, dtype=self.torch.uint8, device="cuda")

    def ptrs(self, out):
        return [[out.data_ptr() + off for off in row] for row in self.out_off]

    def run(self, out, stream=None):
        from vds_amd import chunk
        chunk.encode_batch_device(self.k, list(range(self.n)), self.ins, self.sizes, self.ptrs(out),
                                  write_padding=self.wp, stream=stream)

    def path(self, out):
        from vds_amd import chunk
        return chunk.encode_batch_path(self.k, list(range(self.n)), self.ins, self.sizes, self.ptrs(out),
                                       write_padding=self.wp)

    def per_object(self):
        """The same layout written by one vds_ec_encode16_device call per object."""
        from vds_amd import chunk
        out = self.new_out()
        rows = self.ptrs(out)
        for o, size in enumerate(self.sizes):
            chunk.encode_device(self.k, list(range(self.n)), self.ins[o], size, 0, 1, rows[o], 0,
                                write_padding=self.wp)
        return out

    def check_oracle(self, got, objects=None, replicas=None):
        """got: the output buffer on the host.  Replica bytes and both canaries."""
        for o in (range(len(self.sizes)) if objects is None else objects):
            for r in (range(self.n) if replicas is None else replicas):
                off, L = self.out_off[o][r], self.L[o]
                ref = O.encode(self.k, r, self.data[o], 2, self.wp)
                assert ref.size == L
                assert np.array_equal(got[off:off + L], ref), (self.sizes[o], o, r)
                assert (got[off - CANARY:off] == 0x5A).all(), ("canary before", self.sizes[o], o, r)
                assert (got[off + L:off + L + CANARY] == 0x5A).all(), ("canary after", self.sizes[o], o, r)


def _edge_sizes(k):
    B = 2 * k
    G = 128 * B
    return [1, B - 1, B, B + 1, 127 * B, G - 1, G, G + 1, G + 16, 129 * B + B // 2, 16 * G, 16 * G + 5 * B + 7,
            33 * G - 3, 0]


@pytest.mark.parametrize("k,n", SHAPES)
def test_edge_sizes_one_call(gpu, k, n):
    import torch
    b = Batch(torch, k, n, _edge_sizes(k), seed=k * 1000 + n)
    out = b.new_out()
    assert b.path(out) == (2, len(b.sizes) - 1)  # every non-zero object rides the shared launch
    b.run(out)
    torch.cuda.synchronize()
    b.check_oracle(out.cpu().numpy())


@pytest.mark.parametrize("k,n", SHAPES)
def test_random_ragged_batch(gpu, k, n):
    import torch
    G = 128 * 2 * k
    rng = np.random.default_rng(1000 + 31 * k + n)  # (a seed whose total groups are no multiple of 16, below)
    sizes = rng.integers(0, 3 * G + 1, 300)
    b = Batch(torch, k, n, sizes, seed=77 + k + n)
    B = 2 * k
    groups = sum((-(-int(s) // B) + 127) // 128 for s in sizes)
    assert groups % 16 != 0 and groups // 16 >= 8  # a partly used last tile, several workgroups
    out = b.new_out()
    b.run(out)
    ref = b.per_object()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    b.check_oracle(got, replicas=[0, 1, n // 2, n - 1])
    b.check_oracle(got, objects=[int(o) for o in rng.choice(300, 16, replace=False)])
    assert torch.equal(out, ref)


def test_upload_like_batch(gpu):
    import torch
    k, n = 32, 64
    rng = np.random.default_rng(2048)
    sizes = 16 * rng.integers(60000 // 16, 65552 // 16 + 1, 2048)
    assert sizes.min() >= 60000 and sizes.max() <= 65552
    b = Batch(torch, k, n, sizes, seed=5)
    out = b.new_out()
    assert b.path(out) == (2, 2048)
    b.run(out)
    ref = b.per_object()
    torch.cuda.synchronize()
    b.check_oracle(out.cpu().numpy(), objects=[int(o) for o in rng.choice(2048, 8, replace=False)])
    assert torch.equal(out, ref)


@pytest.mark.parametrize("k,n", SHAPES)
def test_mixed_eligibility(gpu, k, n):
    import torch
    B = 2 * k
    G = 128 * B
    sizes = [G + 5, 3 * B + 1, 2 * G, 0, G - 1, 17 * B, G + B, 130 * B + 9, 5, 2 * G + 3]
    in_mis = [0, 1, 0, 0, 2, 0, 0, 2, 0, 1]
    out_odd = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0]
    eligible = sum(1 for s, m, o in zip(sizes, in_mis, out_odd) if s and not m and not o)
    assert 0 < eligible < len(sizes) - 1
    b = Batch(torch, k, n, sizes, seed=9 + k, in_mis=in_mis, out_odd=out_odd)
    out = b.new_out()
    assert b.path(out) == (2, eligible)
    b.run(out)
    torch.cuda.synchronize()
    b.check_oracle(out.cpu().numpy())


@pytest.mark.parametrize("k,replicas", [(4, list(range(6))), (16, [3, 7, 19])])
def test_other_shapes_take_the_per_object_route(gpu, k, replicas):
    import torch
    from vds_amd import chunk
    B = 2 * k
    G = 128 * B
    sizes = [G + 3, 1, 2 * G, 16 * G + B + 1, 77 * B - 1]
    rng = np.random.default_rng(k)
    data = [rng.integers(1, 256, s, dtype=np.uint8) for s in sizes]
    ins = [torch.from_numpy(d).cuda() for d in data]
    outs = [[torch.full((chunk.replica_size(k, s) + 2 * CANARY,), 0x5A, dtype=torch.uint8, device="cuda")
             for _ in replicas] for s in sizes]
    ptrs = [[t.data_ptr() + CANARY for t in row] for row in outs]
    assert chunk.encode_batch_path(k, replicas, [t.data_ptr() for t in ins], sizes, ptrs) == (1, 0)
    chunk.encode_batch_device(k, replicas, [t.data_ptr() for t in ins], sizes, ptrs)
    torch.cuda.synchronize()
    for d, row in zip(data, outs):
        for r, t in zip(replicas, row):
            got = t.cpu().numpy()
            ref = O.encode(k, r, d)
            assert np.array_equal(got[CANARY:CANARY + ref.size], ref), (d.size, r)
            assert (got[:CANARY] == 0x5A).all() and (got[CANARY + ref.size:] == 0x5A).all()


@pytest.mark.parametrize("calls", [2, 20])
def test_stream_order(gpu, calls):
    """Back-to-back calls on one stream with no synchronise between them: each
    call's tables must stay valid until its kernel has read them (20 calls:
    more than the parameter ring's 16 slots)."""
    import torch
    k, n = 32, 64
    G = 128 * 2 * k
    rng = np.random.default_rng(calls)
    batches = [Batch(torch, k, n, rng.integers(1, 2 * G, 24), seed=100 * calls + c) for c in range(calls)]
    outs = [b.new_out() for b in batches]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    for b, out in zip(batches, outs):
        b.run(out, stream=stream)
    stream.synchronize()
    for b, out in zip(batches, outs):
        assert torch.equal(out, b.per_object())
    torch.cuda.synchronize()


@pytest.mark.parametrize("k,n", SHAPES)
def test_no_trailer(gpu, k, n):
    import torch
    B = 2 * k
    G = 128 * B
    sizes = [B, 5 * B, G, G + B, 16 * G + 3 * B, 127 * B, 0]
    b = Batch(torch, k, n, sizes, seed=3 * k + n, write_padding=False)
    assert b.L == [2 * (s // B) for s in sizes]
    out = b.new_out()
    b.run(out)
    torch.cuda.synchronize()
    b.check_oracle(out.cpu().numpy())  # (the canary right after the last cell included)


@pytest.mark.parametrize("k,n", [(32, 64), (16, 20)])
def test_host_batch_mixed_sizes(gpu, k, n):
    from vds_amd import chunk
    G = 128 * 2 * k
    rng = np.random.default_rng(40 + k)
    sizes = [int(s) for s in rng.integers(0, 2 * G + 1, 40)]
    sizes[7] = sizes[8] = sizes[9]  # a run of equal sizes inside the mixed ones
    objects = [rng.integers(1, 256, s, dtype=np.uint8) for s in sizes]
    got = chunk.encode_host_batch(k, list(range(n)), objects)
    for d, row in zip(objects, got):
        for r in (0, 1, n // 2, n - 1):
            assert np.array_equal(row[r], O.encode(k, r, d)), (d.size, r)
    # the same objects as runs of equal sizes (today's route): the same bytes
    order = sorted(range(40), key=lambda o: sizes[o])
    runs = []
    for o in order:
        runs += [o, o]  # every object twice in a row: only equal-size runs
    again = chunk.encode_host_batch(k, list(range(n)), [objects[o] for o in runs])
    for i, o in enumerate(runs):
        for r in range(n):
            assert np.array_equal(again[i][r], got[o][r]), (sizes[o], r)
