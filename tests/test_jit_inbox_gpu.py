"""The inbox fill form of the run-time compiled k = 16 restore kernels on the
device (restore_syn.hpp kInbox): survivor sets with at most one erased point
below k in each interpolation group {4g..4g+3} keep their survivors in
registers from stage 1 through S1, and the fill's foreign shares pass through
per-wave inboxes inside the owner's own LDS slots.  Every byte must equal the
input (codewords) or the reference's V_S^{-1} route (any survivors)."""
import numpy as np
import pytest

import oracle_ctypes as O

SEED = 0x7664730000000000
K, N = 16, 20
TILE = 2048 * 2 * K
# (erased set, what it covers)
SETS = [((0, 5, 10, 15), "the erased point in each position of its group"),
        ((3, 4, 9, 14), "other positions"),
        ((1, 6, 16, 19), "two groups whole, two extras"),
        ((2, 17, 18, 19), "one inbox only"),
        ((16, 17, 18, 19), "no fill, everything from registers"),
        ((0, 1, 5, 10), "ineligible: the scatter form")]
# two whole tiles plus a 37-stripe tail, size % 32 == 5
SIZE = 2 * TILE + 37 * 2 * K + 5
COUNT = 3


def _nodes(erased):
    return [r for r in range(N) if r not in erased]


def _path(nodes, L, padding, count=1):
    from vds_amd import _lib
    arr = np.asarray(nodes, dtype=np.uint16)
    return _lib.lib().vds_ec_restore16_path(K, arr.ctypes.data_as(_lib.u16p), L, padding, count)


@pytest.fixture
def jit_sync(gpu):
    from vds_amd import chunk
    chunk.jit_set_mode(2)
    yield
    chunk.jit_set_mode(0)


@pytest.fixture(scope="module")
def codewords(gpu):
    """Three objects and their twenty replicas at an odd replica stride."""
    import torch
    from vds_amd import chunk
    assert SIZE % 32 == 5
    L = chunk.replica_size(K, SIZE)
    rstride = L + 7
    data = torch.zeros((COUNT, SIZE), dtype=torch.uint8, device="cuda")
    for o in range(COUNT):
        chunk.fill_splitmix_device(data[o], SIZE, SEED + 5100 + o)
    reps = torch.zeros((N, COUNT * rstride), dtype=torch.uint8, device="cuda")
    chunk.encode_device(K, list(range(N)), data, SIZE, SIZE, COUNT, [reps[i].data_ptr() for i in range(N)], rstride)
    torch.cuda.synchronize()
    return data, reps, L, rstride


@pytest.mark.gpu
@pytest.mark.parametrize("erased", [s for s, _ in SETS], ids=["-".join(map(str, s)) for s, _ in SETS])
def test_inbox_restores_codewords(jit_sync, codewords, erased):
    import torch
    from vds_amd import chunk
    data, reps, L, rstride = codewords
    nodes = _nodes(erased)
    np.random.default_rng(sum(erased)).shuffle(nodes)
    ostride = SIZE + 41
    out = torch.full((COUNT, ostride), 0x5A, dtype=torch.uint8, device="cuda")
    chunk.restore_device(K, nodes, [reps[r].data_ptr() for r in nodes], L, rstride, SIZE % (2 * K), COUNT, out, ostride)
    torch.cuda.synchronize()
    assert _path(nodes, L, SIZE % (2 * K), COUNT) == 4, erased
    for o in range(COUNT):
        assert torch.equal(out[o, :SIZE], data[o]), (erased, o)
    assert bool((out[:, SIZE:] == 0x5A).all()), "bytes written past an object's output"


@pytest.mark.gpu
@pytest.mark.parametrize("erased", [s for s, _ in SETS], ids=["-".join(map(str, s)) for s, _ in SETS])
def test_inbox_restores_random_survivors_as_the_oracle(jit_sync, erased):
    """Survivors that are no codeword: V_S^{-1} applied to them, as the
    reference's chunk_restore gives (the oracle)."""
    import torch
    from vds_amd import chunk
    rng = np.random.default_rng(900 + sum(erased))
    L = chunk.replica_size(K, SIZE)
    rstride = L + 7
    pad = SIZE % (2 * K)
    nodes = _nodes(erased)
    rng.shuffle(nodes)
    host = np.zeros((K, COUNT * rstride), dtype=np.uint8)
    objs = []
    for o in range(COUNT):
        sv = [rng.integers(0, 256, L, dtype=np.uint8) for _ in nodes]
        for c in sv:
            c[-2], c[-1] = pad >> 8, pad & 0xFF
        for j, c in enumerate(sv):
            host[j, o * rstride:o * rstride + L] = c
        objs.append(sv)
    refs = [O.restore(K, nodes, sv) for sv in objs]
    assert all(len(r) == SIZE for r in refs)
    dev = torch.from_numpy(host).cuda()
    ostride = SIZE + 41
    out = torch.full((COUNT, ostride), 0x5A, dtype=torch.uint8, device="cuda")
    chunk.restore_device(K, nodes, [dev[j].data_ptr() for j in range(K)], L, rstride, pad, COUNT, out, ostride)
    torch.cuda.synchronize()
    assert _path(nodes, L, pad, COUNT) == 4, erased
    got = out.cpu().numpy()
    for o in range(COUNT):
        assert np.array_equal(got[o, :SIZE], refs[o]), (erased, o)
    assert (got[:, SIZE:] == 0x5A).all(), "bytes written past an object's output"


@pytest.mark.gpu
def test_inbox_tile_loop_against_the_syndrome_kernel(gpu):
    """One object of 1,100 tiles: every one of the launch's 512 workgroups
    (launch_restore_syn_jit: 2 per CU x 256) walks at least two tiles of its
    XCD's range, so each tile's inbox writes follow a copy-out that read the
    same LDS bytes.  Checked against the input and, byte for byte, against
    JIT mode 0 -- k_restore_syn, the syndrome route."""
    import torch
    from vds_amd import chunk
    erased = (0, 5, 10, 15)
    tiles = 1100
    assert tiles // 8 >= 2 * (512 // 8)
    size = tiles * TILE + 3 * 2 * K + 5
    L = chunk.replica_size(K, size)
    data = torch.empty(size, dtype=torch.uint8, device="cuda")
    chunk.fill_splitmix_device(data, size, SEED + 5200)
    reps = torch.zeros((N, L), dtype=torch.uint8, device="cuda")
    chunk.encode_device(K, list(range(N)), data, size, size, 1, [reps[i].data_ptr() for i in range(N)], L)
    nodes = _nodes(erased)
    outs = []
    try:
        for mode, path in ((2, 4), (0, 3)):
            chunk.jit_set_mode(mode)
            out = torch.full((size + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            chunk.restore_device(K, nodes, [reps[r].data_ptr() for r in nodes], L, L, size % (2 * K), 1, out, size)
            torch.cuda.synchronize()
            assert _path(nodes, L, size % (2 * K)) == path
            outs.append(out)
    finally:
        chunk.jit_set_mode(0)
    assert torch.equal(outs[0][:size], data)
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0][size:] == 0x5A).all())
