"""Host side of the batched repair (vds_ec_repair16_batch_device /
_host_batch) and of vds_ec_sha256_check_batch_device: the argument validation,
which runs before anything is enqueued and before the device is looked for.
No GPU: the device pointers are fabricated integers, nothing dereferences
them; the host form's buffers are real (it reads the first chunk's trailer)."""
import ctypes as C

import numpy as np

from vds_amd import _lib, chunk

IN0 = 0x7F0000000000   # fabricated device addresses
OUT0 = 0x7E0000000000
DIG0 = 0x7D0000000000
EXP0 = 0x7C0000000000
VER0 = 0x7B0000000000
K, NT = 32, 2
SIZES = [64 * 130, 64, 1, 65536]
NULL = None


def _no_device(lib):
    cnt = C.c_int(0)
    assert lib.vds_ec_device_count(C.byref(cnt)) == 0
    return cnt.value == 0


def test_symbols_exist(vds_lib):
    for name in ("vds_ec_sha256_check_batch_device", "vds_ec_repair16_batch_device", "vds_ec_repair16_host_batch"):
        assert hasattr(vds_lib, name) and name in _lib.SIGNATURES


# ------------------------------------------------------------- the check alone
def _check(lib, msgs, lens, expected=EXP0, digests=DIG0, verdicts=VER0, count=None, null_msgs=False,
           null_lens=False):
    mp = np.asarray(msgs, dtype=np.uint64)
    ln = np.asarray(lens, dtype=np.uint64)
    return lib.vds_ec_sha256_check_batch_device(len(lens) if count is None else count,
                                                None if null_msgs else mp.ctypes.data_as(_lib.vpp),
                                                None if null_lens else ln.ctypes.data_as(_lib.u64p), expected,
                                                digests, verdicts, None)


def test_sha256_check_batch_arguments(vds_lib):
    msgs, lens = [IN0, IN0 + 100, 0, IN0 + 301], [100, 200, 0, 7]
    assert _check(vds_lib, msgs, lens, null_msgs=True) == _lib.EINVAL
    assert _check(vds_lib, msgs, lens, null_lens=True) == _lib.EINVAL
    assert _check(vds_lib, msgs, lens, expected=NULL) == _lib.EINVAL
    assert _check(vds_lib, msgs, lens, verdicts=NULL) == _lib.EINVAL
    assert _check(vds_lib, msgs, lens, count=1 << 30) == _lib.EINVAL
    assert _check(vds_lib, [IN0, 0], [5, 5]) == _lib.EINVAL  # a null message with a non-zero length
    assert _check(vds_lib, [], [], count=0) == _lib.OK
    assert vds_lib.vds_ec_sha256_check_batch_device(0, None, None, None, None, None, None) == _lib.OK
    if _no_device(vds_lib):  # validation first, the device second; digests are optional
        assert _check(vds_lib, msgs, lens) == _lib.ENODEV
        assert _check(vds_lib, msgs, lens, digests=NULL) == _lib.ENODEV


# ------------------------------------------------------------- the device form
def _layout(k, nt, sizes):
    """Per object: k survivor addresses, the chunk size, nt output addresses."""
    chunks, csz, outs, ipos, opos = [], [], [], IN0, OUT0
    for s in sizes:
        L = chunk.replica_size(k, s)
        chunks.append([ipos + j * (L + 14) for j in range(k)])
        ipos += k * (L + 14)
        outs.append([opos + i * (L + 6) for i in range(nt)])
        opos += nt * (L + 6)
        csz.append(L)
    return chunks, csz, outs


def _nodes(k, count, lost=(1, 5)):
    return [[r for r in range(k + len(lost)) if r not in lost] for _ in range(count)]


def _repair(lib, k, nodes, chunks, csz, targets, outs, digests=DIG0, expected=EXP0, verdicts=VER0, count=None,
            nt=None, null=()):
    nd = np.asarray(nodes, dtype=np.uint16).reshape(-1)
    cp = np.asarray(chunks, dtype=np.uint64).reshape(-1)
    cs = np.asarray(csz, dtype=np.uint64)
    tg = np.asarray(targets, dtype=np.uint16).reshape(-1)
    op = np.asarray(outs, dtype=np.uint64).reshape(-1)
    return lib.vds_ec_repair16_batch_device(k, len(csz) if count is None else count,
                                            None if "nodes" in null else nd.ctypes.data_as(_lib.u16p),
                                            None if "chunks" in null else cp.ctypes.data_as(_lib.vpp),
                                            None if "sizes" in null else cs.ctypes.data_as(_lib.u64p),
                                            (len(targets[0]) if targets else 0) if nt is None else nt,
                                            None if "targets" in null else tg.ctypes.data_as(_lib.u16p),
                                            None if "outs" in null else op.ctypes.data_as(_lib.vpp),
                                            digests, expected, verdicts, None)


def test_repair_batch_device_invalid_arguments(vds_lib):
    chunks, csz, outs = _layout(K, NT, SIZES)
    nodes, targets = _nodes(K, len(SIZES)), [[1, 5]] * len(SIZES)
    # the checks of vds_ec_regenerate16_batch_device
    for null in ("nodes", "chunks", "sizes", "targets", "outs"):
        assert _repair(vds_lib, K, nodes, chunks, csz, targets, outs, null=(null,)) == _lib.EINVAL
    assert _repair(vds_lib, 0, nodes, chunks, csz, targets, outs) == _lib.EINVAL
    assert _repair(vds_lib, K, nodes, chunks, csz, targets, outs, count=1 << 30) == _lib.EINVAL
    for bad_size in (0, 1, 7):  # cells of two bytes and a two-byte trailer
        bad = list(csz)
        bad[2] = bad_size
        assert _repair(vds_lib, K, nodes, chunks, bad, targets, outs) == _lib.EINVAL
    bad_ch = [list(c) for c in chunks]
    bad_ch[3][K - 1] = 0
    assert _repair(vds_lib, K, nodes, bad_ch, csz, targets, outs) == _lib.EINVAL
    bad_out = [list(o) for o in outs]
    bad_out[1][1] = 0
    assert _repair(vds_lib, K, nodes, chunks, csz, targets, bad_out) == _lib.EINVAL
    dup = [list(nd) for nd in nodes]
    dup[2][7] = dup[2][3]  # a repeated id: V_S is singular
    assert _repair(vds_lib, K, dup, chunks, csz, targets, outs) == _lib.ESINGULAR
    # the names and the check
    assert _repair(vds_lib, K, nodes, chunks, csz, targets, outs, digests=NULL) == _lib.EINVAL
    assert _repair(vds_lib, K, nodes, chunks, csz, targets, outs, expected=NULL) == _lib.EINVAL  # verdicts alone
    assert _repair(vds_lib, K, nodes, chunks, csz, targets, outs, verdicts=NULL) == _lib.EINVAL  # expected alone
    # the hash launch's lanes: count * (nt + 64) < 2^32 (checked before any array is read)
    assert _repair(vds_lib, K, nodes, chunks, csz, targets, outs, count=(1 << 30) - 1, nt=4) == _lib.EINVAL
    # k == 0 is invalid whatever the count
    assert _repair(vds_lib, 0, [], [], [], [], [], count=0, nt=2) == _lib.EINVAL


def test_repair_batch_device_empty_is_ok(vds_lib):
    chunks, csz, outs = _layout(K, NT, SIZES)
    nodes = _nodes(K, len(SIZES))
    assert _repair(vds_lib, K, [], [], [], [], [], count=0, nt=2) == _lib.OK
    assert vds_lib.vds_ec_repair16_batch_device(K, 0, None, None, None, 2, None, None, None, None, None,
                                                None) == _lib.OK
    # no targets: nothing to write, no names wanted
    assert _repair(vds_lib, K, nodes, chunks, csz, [], [], digests=NULL, expected=NULL, verdicts=NULL,
                   nt=0, null=("targets", "outs")) == _lib.OK


def test_repair_batch_device_valid_call_needs_a_device(vds_lib):
    """Validation comes first, the device check second, and there is no CPU
    fallback (where a GPU is present the GPU suite covers the call)."""
    if not _no_device(vds_lib):
        return
    chunks, csz, outs = _layout(K, NT, SIZES)
    nodes, targets = _nodes(K, len(SIZES)), [[1, 5]] * len(SIZES)
    assert _repair(vds_lib, K, nodes, chunks, csz, targets, outs) == _lib.ENODEV
    assert _repair(vds_lib, K, nodes, chunks, csz, targets, outs, expected=NULL, verdicts=NULL) == _lib.ENODEV
    ch3, cs3, out3 = _layout(3, NT, SIZES)  # any k: one launch per object
    assert _repair(vds_lib, 3, _nodes(3, len(SIZES), (0, 2)), ch3, cs3, [[0, 2]] * len(SIZES), out3) == _lib.ENODEV


# --------------------------------------------------------------- the host form
def _host(lib, k, sizes, nt=NT, trailers=None, count=None, null=(), null_chunk=None, null_out=None, dup=False,
          expected=True, bad_size=None):
    """vds_ec_repair16_host_batch on real host buffers (a failed validation
    transfers nothing).  trailers[o]: the first chunk's trailer of object o."""
    n_obj = len(sizes)
    k_arg, k = k, k or 16  # (k == 0: buffers as for k = 16, the call gets 0)
    csz = [chunk.replica_size(k, s) for s in sizes]
    bufs = [[np.zeros(L, dtype=np.uint8) for _ in range(k)] for L in csz]
    for o, s in enumerate(sizes):
        p = s % (2 * k) if trailers is None else trailers[o]
        for b in bufs[o]:
            b[-2], b[-1] = s % (2 * k) >> 8, s % (2 * k) & 0xFF
        bufs[o][0][-2], bufs[o][0][-1] = p >> 8, p & 0xFF
    nodes = np.asarray(_nodes(k, n_obj), dtype=np.uint16)
    if dup:
        nodes[n_obj - 1][2] = nodes[n_obj - 1][0]
    targets = np.asarray([[1, 5][:nt]] * n_obj, dtype=np.uint16)
    cs = np.asarray(csz if bad_size is None else [bad_size] + csz[1:], dtype=np.uint64)
    outs = [[np.zeros(L, dtype=np.uint8) for _ in range(nt)] for L in csz]
    cp = (C.c_void_p * max(1, n_obj * k))(*[b.ctypes.data for row in bufs for b in row])
    op = (C.c_void_p * max(1, n_obj * nt))(*[o.ctypes.data for row in outs for o in row])
    if null_chunk is not None:
        cp[null_chunk] = None
    if null_out is not None:
        op[null_out] = None
    dg = np.zeros(max(1, n_obj * nt * 32), dtype=np.uint8)
    ex = np.zeros(max(1, n_obj * nt * 32), dtype=np.uint8)
    vd = np.zeros(max(1, n_obj * nt), dtype=np.uint8)
    bad = C.c_uint32(77)
    rc = lib.vds_ec_repair16_host_batch(k_arg, n_obj if count is None else count,
                                        None if "nodes" in null else nodes.ctypes.data_as(_lib.u16p),
                                        None if "chunks" in null else cp,
                                        None if "sizes" in null else cs.ctypes.data_as(_lib.u64p), nt,
                                        None if "targets" in null else targets.ctypes.data_as(_lib.u16p),
                                        None if "outs" in null else op,
                                        None if "digests" in null else dg.ctypes.data,
                                        ex.ctypes.data if expected and "expected" not in null else None,
                                        vd.ctypes.data if expected and "verdicts" not in null else None,
                                        None if "mismatches" in null else C.byref(bad))
    return rc


def test_repair_host_batch_arguments(vds_lib):
    for null in ("nodes", "chunks", "sizes", "targets", "outs", "digests", "expected", "verdicts"):
        assert _host(vds_lib, 16, SIZES, null=(null,)) == _lib.EINVAL, null
    assert _host(vds_lib, 0, SIZES) == _lib.EINVAL
    assert _host(vds_lib, 16, SIZES, count=1 << 30) == _lib.EINVAL
    assert _host(vds_lib, 16, SIZES, null_chunk=16 * 2 + 9) == _lib.EINVAL
    assert _host(vds_lib, 16, SIZES, null_out=NT * 3 + 1) == _lib.EINVAL
    assert _host(vds_lib, 16, SIZES, bad_size=1) == _lib.EINVAL
    assert _host(vds_lib, 16, SIZES, dup=True) == _lib.ESINGULAR
    assert _host(vds_lib, 16, [], count=0) == _lib.OK
    assert _host(vds_lib, 16, SIZES, nt=0, null=("targets", "outs", "digests"), expected=False) == _lib.OK
    assert vds_lib.vds_ec_repair16_host_batch(16, 0, None, None, None, 2, None, None, None, None, None,
                                              None) == _lib.OK
    if _no_device(vds_lib):
        assert _host(vds_lib, 16, SIZES) == _lib.ENODEV
        assert _host(vds_lib, 16, SIZES, expected=False, null=("mismatches",)) == _lib.ENODEV
        assert _host(vds_lib, 32, SIZES, trailers=[64, 0, 1, 0]) == _lib.ENODEV  # p == 2k trims nothing


def test_repair_host_batch_rejects_a_first_trailer_above_2k(vds_lib):
    """The reference route restores with the first chunk's trailer
    (chunk.h:408): above 2k there is no chunk_size-byte answer, and the whole
    call fails before the device is looked for -- on a machine with no GPU the
    status is VDS_EC_ERESTORE, not VDS_EC_ENODEV."""
    k = 16
    ok = [s % (2 * k) for s in SIZES]
    for o in range(len(SIZES)):
        tr = list(ok)
        tr[o] = 2 * k + 1
        assert _host(vds_lib, k, SIZES, trailers=tr) == _lib.ERESTORE, o
    assert _host(vds_lib, k, SIZES, trailers=[0, 0, 0, 65535]) == _lib.ERESTORE
