"""Host side of the batched encode (vds_ec_encode16_batch_device / _path): the
planning query and the argument validation, which run before the device is
looked for.  No GPU: the pointers are fabricated integers, nothing
dereferences them."""
import ctypes as C

import numpy as np
import pytest

from vds_amd import _lib, chunk

SHAPES = [(16, 20), (32, 40), (32, 64)]
IN0 = 0x7F0000000000   # fabricated device addresses
OUT0 = 0x7E0000000000


def _layout(k, n, sizes, in_mis=None, out_odd=None):
    """ins / outs as tests/test_encode_batch_gpu.py lays them out, fabricated."""
    in_mis = in_mis or [0] * len(sizes)
    out_odd = out_odd or [0] * len(sizes)
    ins, outs, ipos, opos = [], [], IN0, OUT0
    for s, mis, odd in zip(sizes, in_mis, out_odd):
        ipos = (ipos + 3) // 4 * 4 + 8 + mis
        ins.append(ipos)
        ipos += s
        slot = (128 + chunk.replica_size(k, s) + 1) // 2 * 2
        outs.append([opos + odd + i * slot + 64 for i in range(n)])
        opos += n * slot + 2
    return ins, outs


def _edge_sizes(k):
    B = 2 * k
    G = 128 * B
    return [1, B - 1, B, B + 1, 127 * B, G - 1, G, G + 1, G + 16, 129 * B + B // 2, 16 * G, 16 * G + 5 * B + 7,
            33 * G - 3, 0]


@pytest.mark.parametrize("k,n", SHAPES)
def test_path_edge_sizes(vds_lib, k, n):
    sizes = _edge_sizes(k)
    ins, outs = _layout(k, n, sizes)
    assert chunk.encode_batch_path(k, list(range(n)), ins, sizes, outs) == (2, len(sizes) - 1)


@pytest.mark.parametrize("k,n", SHAPES)
def test_path_mixed_eligibility(vds_lib, k, n):
    B = 2 * k
    G = 128 * B
    sizes = [G + 5, 3 * B + 1, 2 * G, 0, G - 1, 17 * B, G + B, 130 * B + 9, 5, 2 * G + 3]
    in_mis = [0, 1, 0, 0, 2, 0, 0, 2, 0, 1]
    out_odd = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0]
    ins, outs = _layout(k, n, sizes, in_mis, out_odd)
    eligible = sum(1 for s, m, o in zip(sizes, in_mis, out_odd) if s and not m and not o)
    assert chunk.encode_batch_path(k, list(range(n)), ins, sizes, outs) == (2, eligible)
    # one odd replica pointer is enough to take an object off the shared launch
    outs[0][n - 1] += 1
    assert chunk.encode_batch_path(k, list(range(n)), ins, sizes, outs) == (2, eligible - 1)


@pytest.mark.parametrize("k,replicas", [(4, list(range(6))), (16, [3, 7, 19]), (16, list(range(1, 21))),
                                        (32, list(range(48)))])
def test_path_other_shapes(vds_lib, k, replicas):
    B = 2 * k
    G = 128 * B
    sizes = [G + 3, 1, 2 * G, 16 * G + B + 1, 77 * B - 1]
    ins, outs = _layout(k, len(replicas), sizes)
    assert chunk.encode_batch_path(k, replicas, ins, sizes, outs) == (1, 0)


def _call(lib, k, n, ins, sizes, outs, flags=0, count=None, replicas=None):
    ids = np.asarray(list(range(n)) if replicas is None else replicas, dtype=np.uint16)
    ip = np.asarray(ins, dtype=np.uint64)
    sz = np.asarray(sizes, dtype=np.uint64)
    op = np.asarray(outs, dtype=np.uint64).reshape(-1)
    return lib.vds_ec_encode16_batch_device(k, ids.ctypes.data_as(_lib.u16p), n, len(sizes) if count is None else count,
                                            ip.ctypes.data_as(_lib.vpp), sz.ctypes.data_as(_lib.u64p),
                                            op.ctypes.data_as(_lib.vpp), flags, None)


def test_invalid_arguments(vds_lib):
    k, n = 32, 64
    sizes = [64 * 130, 64, 0, 8192]
    ins, outs = _layout(k, n, sizes)
    bad = list(ins)
    bad[1] = 0  # a null input with a non-zero size
    assert _call(vds_lib, k, n, bad, sizes, outs) == _lib.EINVAL
    bad_out = [list(r) for r in outs]
    bad_out[3][n - 1] = 0  # a null replica pointer
    assert _call(vds_lib, k, n, ins, sizes, bad_out) == _lib.EINVAL
    assert _call(vds_lib, 0, n, ins, sizes, outs) == _lib.EINVAL
    assert _call(vds_lib, k, n, ins, sizes, outs, count=1 << 30) == _lib.EINVAL
    assert _call(vds_lib, k, n, ins, sizes, outs, flags=_lib.F_CELLS) == _lib.EINVAL
    # no trailer: every size a multiple of 2k
    assert _call(vds_lib, k, n, ins, [64 * 130, 64, 0, 8191], outs, flags=_lib.F_NO_TRAILER) == _lib.EINVAL
    # the query reports an invalid batch as path 1 with nothing on the shared launch
    assert chunk.encode_batch_path(k, list(range(n)), bad, sizes, outs) == (1, 0)


def test_null_input_of_an_empty_object_is_valid(vds_lib):
    k, n = 32, 64
    sizes = [64 * 130, 0]
    ins, outs = _layout(k, n, sizes)
    ins[1] = 0
    assert chunk.encode_batch_path(k, list(range(n)), ins, sizes, outs) == (2, 1)


def test_valid_call_needs_a_device(vds_lib):
    """Validation comes first, the device check second: on a machine without
    a GPU a good call is VDS_EC_ENODEV (where one is present this test has
    nothing to assert and the GPU suite covers the call)."""
    cnt = C.c_int(0)
    assert vds_lib.vds_ec_device_count(C.byref(cnt)) == 0
    if cnt.value:
        return
    k, n = 32, 64
    sizes = [64 * 130, 64, 0, 8192]
    ins, outs = _layout(k, n, sizes)
    assert _call(vds_lib, k, n, ins, sizes, outs) == _lib.ENODEV
    assert _call(vds_lib, k, n, ins, sizes, outs, flags=_lib.F_NO_TRAILER) == _lib.ENODEV
    assert _call(vds_lib, 16, 3, ins, sizes, [r[:3] for r in outs], replicas=[3, 7, 19]) == _lib.ENODEV
