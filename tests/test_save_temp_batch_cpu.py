"""Host side of vds_ec_sha256_batch_device and the batched save_temp
(vds_ec_save_temp16_batch_device / _host_batch): the argument validation,
which runs before anything is enqueued and before the device is looked for.
No GPU: the device pointers are fabricated integers, nothing dereferences
them."""
import ctypes as C

import numpy as np

from vds_amd import _lib, chunk

IN0 = 0x7F0000000000   # fabricated device addresses
OUT0 = 0x7E0000000000
DIG0 = 0x7D0000000000
K, N = 32, 64
SIZES = [64 * 130, 64, 0, 8192]
NULL = None


def _layout(k, n, sizes):
    ins, outs, ipos, opos = [], [], IN0, OUT0
    for s in sizes:
        ipos = (ipos + 15) // 16 * 16 + 16
        ins.append(ipos)
        ipos += s
        slot = chunk.replica_size(k, s) + 14
        outs.append([opos + i * slot for i in range(n)])
        opos += n * slot
    return ins, outs


def _no_device(lib):
    cnt = C.c_int(0)
    assert lib.vds_ec_device_count(C.byref(cnt)) == 0
    return cnt.value == 0


def _sha(lib, msgs, lens, digests=DIG0, count=None, null_msgs=False, null_lens=False):
    mp = np.asarray(msgs, dtype=np.uint64)
    ln = np.asarray(lens, dtype=np.uint64)
    return lib.vds_ec_sha256_batch_device(len(lens) if count is None else count,
                                          None if null_msgs else mp.ctypes.data_as(_lib.vpp),
                                          None if null_lens else ln.ctypes.data_as(_lib.u64p), digests, None)


def _save(lib, k, n, ins, sizes, outs, rd=DIG0, dd=DIG0 + (1 << 30), count=None, null=()):
    ip = np.asarray(ins, dtype=np.uint64)
    sz = np.asarray(sizes, dtype=np.uint64)
    op = np.asarray(outs, dtype=np.uint64).reshape(-1)
    return lib.vds_ec_save_temp16_batch_device(k, n, len(sizes) if count is None else count,
                                               None if "ins" in null else ip.ctypes.data_as(_lib.vpp),
                                               None if "sizes" in null else sz.ctypes.data_as(_lib.u64p),
                                               None if "outs" in null else op.ctypes.data_as(_lib.vpp), rd, dd, None)


def test_sha256_batch_invalid_arguments(vds_lib):
    msgs, lens = [IN0, IN0 + 100, 0, IN0 + 301], [100, 200, 0, 7]
    assert _sha(vds_lib, msgs, lens, null_msgs=True) == _lib.EINVAL
    assert _sha(vds_lib, msgs, lens, null_lens=True) == _lib.EINVAL
    assert _sha(vds_lib, msgs, lens, digests=NULL) == _lib.EINVAL
    assert _sha(vds_lib, msgs, lens, count=1 << 30) == _lib.EINVAL
    assert _sha(vds_lib, [IN0, 0], [5, 5]) == _lib.EINVAL  # a null message with a non-zero length


def test_sha256_batch_empty_is_ok(vds_lib):
    assert _sha(vds_lib, [], [], count=0) == _lib.OK
    assert vds_lib.vds_ec_sha256_batch_device(0, None, None, None, None) == _lib.OK


def test_sha256_batch_valid_call_needs_a_device(vds_lib):
    """Validation comes first, the device check second (where a GPU is present
    this test has nothing to assert and the GPU suite covers the call)."""
    if not _no_device(vds_lib):
        return
    assert _sha(vds_lib, [IN0, IN0 + 100, 0, IN0 + 301], [100, 200, 0, 7]) == _lib.ENODEV


def test_save_temp_batch_device_invalid_arguments(vds_lib):
    ins, outs = _layout(K, N, SIZES)
    for null in ("ins", "sizes", "outs"):
        assert _save(vds_lib, K, N, ins, SIZES, outs, null=(null,)) == _lib.EINVAL
    assert _save(vds_lib, K, N, ins, SIZES, outs, rd=NULL) == _lib.EINVAL  # names wanted: count * n > 0
    assert _save(vds_lib, 0, N, ins, SIZES, outs) == _lib.EINVAL
    assert _save(vds_lib, K, N, ins, SIZES, outs, count=1 << 30) == _lib.EINVAL
    bad = list(ins)
    bad[1] = 0  # a null body with a non-zero size
    assert _save(vds_lib, K, N, bad, SIZES, outs) == _lib.EINVAL
    bad_out = [list(r) for r in outs]
    bad_out[3][N - 1] = 0  # a null replica pointer
    assert _save(vds_lib, K, N, ins, SIZES, bad_out) == _lib.EINVAL
    # k == 0 is invalid whatever the count
    assert _save(vds_lib, 0, N, [], [], [], count=0) == _lib.EINVAL


def test_save_temp_batch_device_empty_is_ok(vds_lib):
    assert _save(vds_lib, K, N, [], [], [], count=0) == _lib.OK
    assert vds_lib.vds_ec_save_temp16_batch_device(K, N, 0, None, None, None, None, None, None) == _lib.OK


def test_save_temp_batch_device_valid_call_needs_a_device(vds_lib):
    if not _no_device(vds_lib):
        return
    ins, outs = _layout(K, N, SIZES)
    assert _save(vds_lib, K, N, ins, SIZES, outs) == _lib.ENODEV
    assert _save(vds_lib, K, N, ins, SIZES, outs, dd=NULL) == _lib.ENODEV  # body digests are optional
    ins[2] = 0  # an empty body may be null
    assert _save(vds_lib, K, N, ins, SIZES, outs) == _lib.ENODEV
    assert _save(vds_lib, 3, 5, ins, SIZES, [r[:5] for r in outs]) == _lib.ENODEV
    assert _save(vds_lib, K, 0, ins, SIZES, [], rd=NULL) == _lib.ENODEV  # no replicas: no names to write


def _host(lib, k, n, bodies, count=None, null=(), null_body=None, null_out=None):
    """vds_ec_save_temp16_host_batch on real host buffers (a failed validation touches none)."""
    count = len(bodies) if count is None else count
    bufs = [np.frombuffer(b, dtype=np.uint8) for b in bodies]
    sz = np.asarray([b.size for b in bufs], dtype=np.uint64)
    outs = [[np.zeros(max(1, chunk.replica_size(k, b.size)), dtype=np.uint8) for _ in range(n)] for b in bufs]
    ip = (C.c_void_p * max(1, len(bufs)))(*[b.ctypes.data if b.size else None for b in bufs])
    op = (C.c_void_p * max(1, len(bufs) * n))(*[o.ctypes.data for row in outs for o in row])
    if null_body is not None:
        ip[null_body] = None
    if null_out is not None:
        op[null_out] = None
    rd = np.zeros(max(1, len(bufs) * n * 32), dtype=np.uint8)
    dd = np.zeros(max(1, len(bufs) * 32), dtype=np.uint8)
    rs = np.zeros(max(1, len(bufs)), dtype=np.uint32)
    return lib.vds_ec_save_temp16_host_batch(k, n, count, None if "objs" in null else ip,
                                             None if "sizes" in null else sz.ctypes.data_as(_lib.u64p),
                                             None if "outs" in null else op,
                                             None if "rd" in null else rd.ctypes.data,
                                             None if "dd" in null else dd.ctypes.data,
                                             None if "rs" in null else rs.ctypes.data_as(C.POINTER(C.c_uint32)))


def test_save_temp_host_batch_arguments(vds_lib):
    bodies = [b"a" * 100, b"", b"b" * 4097]
    for null in ("objs", "sizes", "outs", "rd"):
        assert _host(vds_lib, 16, 20, bodies, null=(null,)) == _lib.EINVAL
    assert _host(vds_lib, 0, 20, bodies) == _lib.EINVAL
    assert _host(vds_lib, 16, 20, bodies, count=1 << 30) == _lib.EINVAL
    assert _host(vds_lib, 16, 20, bodies, null_body=2) == _lib.EINVAL
    assert _host(vds_lib, 16, 20, bodies, null_out=20 * 2 + 7) == _lib.EINVAL
    assert _host(vds_lib, 16, 20, [], count=0) == _lib.OK
    assert vds_lib.vds_ec_save_temp16_host_batch(16, 20, 0, None, None, None, None, None, None) == _lib.OK
    if _no_device(vds_lib):
        assert _host(vds_lib, 16, 20, bodies) == _lib.ENODEV
        assert _host(vds_lib, 16, 20, bodies, null=("dd", "rs")) == _lib.ENODEV
