"""Host side of the batched download (vds_ec_download16_batch_device /
_host_batch) and of the gated base64 encode: the argument validation, which
runs before anything is enqueued and before the device is looked for -- every
VDS_EC_EINVAL and VDS_EC_ESINGULAR below is returned on a machine with no
device.  No GPU: the device pointers are fabricated integers, nothing
dereferences them; the host form's buffers are real (it reads the first
chunk's trailer)."""
import ctypes as C

import numpy as np

from vds_amd import _lib, chunk

IN0 = 0x7F0000000000   # fabricated device addresses
OBJ0 = 0x7E0000000000
TXT0 = 0x7D0000000000
SN0 = 0x7C0000000000
VER0 = 0x7B0000000000
ST0 = 0x7A0000000000
WN0 = 0x790000000000
WO0 = 0x780000000000
K = 32
SIZES = [64 * 130, 64, 1, 65536]
NULL = None


def _no_device(lib):
    cnt = C.c_int(0)
    assert lib.vds_ec_device_count(C.byref(cnt)) == 0
    return cnt.value == 0


def test_symbols_and_the_new_status(vds_lib):
    for name in ("vds_ec_download16_batch_device", "vds_ec_download16_host_batch",
                 "vds_ec_base64_encode_gated_batch_device"):
        assert hasattr(vds_lib, name) and name in _lib.SIGNATURES
    assert _lib.ECORRUPT == -10
    assert vds_lib.vds_ec_strerror(-10) == b"Data is corrupted"
    assert _lib.strerror(_lib.ECORRUPT) == "Data is corrupted"


# ------------------------------------------------------------- the device form
def _nodes(k, count, lost=(1, 5)):
    return [[r for r in range(k + len(lost)) if r not in lost] for _ in range(count)]


def _device(lib, k=K, sizes=SIZES, mode="survivor", nodes=None, witness=None, count=None, null=(), both=False,
            neither=False, chunk_sizes=None, null_chunk=None, null_object=None, null_text=None, null_wout=None,
            paddings=None):
    n_obj = len(sizes)
    kk = k or K
    csz = [chunk.replica_size(kk, s) for s in sizes] if chunk_sizes is None else chunk_sizes
    nd = np.asarray(_nodes(kk, n_obj) if nodes is None else nodes, dtype=np.uint16).reshape(-1)
    ch, pos = [], IN0
    for L in csz:
        ch.append([pos + j * (L + 14) for j in range(kk)])
        pos += kk * (L + 14)
    if null_chunk is not None:
        ch[null_chunk[0]][null_chunk[1]] = 0
    cp = np.asarray(ch, dtype=np.uint64).reshape(-1)
    cs = np.asarray(csz, dtype=np.uint64)
    pd = np.asarray([s % (2 * kk) for s in sizes] if paddings is None else paddings, dtype=np.uint16)
    ob = np.asarray([OBJ0 + 70001 * o for o in range(n_obj)], dtype=np.uint64)
    tp = np.asarray([TXT0 + 100003 * o for o in range(n_obj)], dtype=np.uint64)
    wo = np.asarray([WO0 + 70001 * o for o in range(n_obj)], dtype=np.uint64)
    if null_object is not None:
        ob[null_object] = 0
    if null_text is not None:
        tp[null_text] = 0
    if null_wout is not None:
        wo[null_wout] = 0
    wi = np.asarray([1] * n_obj if witness is None else witness, dtype=np.uint16)
    surv = mode == "survivor" or both
    wit = mode == "witness" or both
    if neither:
        surv = wit = False

    def arg(name, value):
        return None if name in null else value

    return lib.vds_ec_download16_batch_device(
        k, n_obj if count is None else count, arg("nodes", nd.ctypes.data_as(_lib.u16p)),
        arg("chunks", cp.ctypes.data_as(_lib.vpp)), arg("sizes", cs.ctypes.data_as(_lib.u64p)),
        arg("paddings", pd.ctypes.data_as(_lib.u16p)), SN0 if surv else None,
        arg("witness_ids", wi.ctypes.data_as(_lib.u16p)) if wit else None,
        arg("witness_names", WN0) if wit else None, arg("witness_outs", wo.ctypes.data_as(_lib.vpp)) if wit else None,
        arg("objects", ob.ctypes.data_as(_lib.vpp)), arg("texts", tp.ctypes.data_as(_lib.vpp)),
        arg("verdicts", VER0), arg("statuses", ST0), None)


def test_download_batch_device_exactly_one_check(vds_lib):
    assert _device(vds_lib, both=True) == _lib.EINVAL
    assert _device(vds_lib, neither=True) == _lib.EINVAL
    # the witness triple is given whole or not at all
    for part in ("witness_ids", "witness_names", "witness_outs"):
        assert _device(vds_lib, mode="witness", null=(part,)) == _lib.EINVAL, part


def test_download_batch_device_invalid_arguments(vds_lib):
    for mode in ("survivor", "witness"):
        for null in ("nodes", "chunks", "sizes", "paddings", "objects", "texts", "verdicts", "statuses"):
            assert _device(vds_lib, mode=mode, null=(null,)) == _lib.EINVAL, (mode, null)
        assert _device(vds_lib, k=0, mode=mode) == _lib.EINVAL
        assert _device(vds_lib, mode=mode, count=1 << 30) == _lib.EINVAL
        assert _device(vds_lib, mode=mode, null_chunk=(3, K - 1)) == _lib.EINVAL
        assert _device(vds_lib, mode=mode, null_object=0) == _lib.EINVAL
        assert _device(vds_lib, mode=mode, null_text=3) == _lib.EINVAL
        dup = _nodes(K, len(SIZES))
        dup[2][7] = dup[2][3]  # a repeated survivor id: V_S is singular
        assert _device(vds_lib, mode=mode, nodes=dup) == _lib.ESINGULAR
        # restore's own: a trailer the chunk size has no answer for
        assert _device(vds_lib, mode=mode, paddings=[0, 0, 0, 65535]) == _lib.ERESTORE
    # a witness that is one of its object's survivors (survivors: 0, 2, 3, 4, 6, ...)
    for o in range(len(SIZES)):
        wi = [1] * len(SIZES)
        wi[o] = 6
        assert _device(vds_lib, mode="witness", witness=wi) == _lib.EINVAL, o
    # repair's checks: whole cells and a trailer; a buffer for every witness
    bad = [chunk.replica_size(K, s) for s in SIZES]
    bad[1] += 1
    assert _device(vds_lib, mode="witness", chunk_sizes=bad) == _lib.EINVAL
    assert _device(vds_lib, mode="witness", null_wout=2) == _lib.EINVAL
    # the hash launch's lanes (checked before any array is read)
    assert _device(vds_lib, mode="survivor", count=1 << 26) == _lib.EINVAL  # count * (k + 64) >= 2^32
    assert _device(vds_lib, mode="witness", count=(1 << 30) - 1) == _lib.EINVAL  # count * 65 >= 2^32


def test_download_batch_device_empty_is_ok(vds_lib):
    assert _device(vds_lib, sizes=[], count=0) == _lib.OK
    assert _device(vds_lib, sizes=[], mode="witness", count=0) == _lib.OK
    assert vds_lib.vds_ec_download16_batch_device(K, 0, None, None, None, None, None, None, None, None, None, None,
                                                  None, None, None) == _lib.OK
    assert vds_lib.vds_ec_download16_batch_device(0, 0, None, None, None, None, None, None, None, None, None, None,
                                                  None, None, None) == _lib.EINVAL


def test_download_batch_device_valid_call_needs_a_device(vds_lib):
    """Validation comes first, the device check second, and there is no CPU
    fallback (where a GPU is present the GPU suite covers the call)."""
    if not _no_device(vds_lib):
        return
    assert _device(vds_lib) == _lib.ENODEV
    assert _device(vds_lib, mode="witness") == _lib.ENODEV
    assert _device(vds_lib, k=3, nodes=_nodes(3, len(SIZES), (0, 2)), mode="witness", witness=[0] * 4) == _lib.ENODEV
    # an empty object needs neither an object buffer nor a text
    assert _device(vds_lib, sizes=[0, 5], null_object=0, null_text=0) == _lib.ENODEV


# ------------------------------------------------------------- the gated encode
def _gated(lib, lens, ngates, count=None, null=(), null_gate=None, null_in=None):
    n = len(lens)
    ip = np.asarray([IN0 + 70001 * o for o in range(n)], dtype=np.uint64)
    op = np.asarray([TXT0 + 100003 * o for o in range(n)], dtype=np.uint64)
    gp = np.asarray([VER0 + 71 * o for o in range(n)], dtype=np.uint64)
    ln = np.asarray(lens, dtype=np.uint64)
    ng = np.asarray(ngates, dtype=np.uint32)
    if null_gate is not None:
        gp[null_gate] = 0
    if null_in is not None:
        ip[null_in] = 0

    def arg(name, value):
        return None if name in null else value

    return lib.vds_ec_base64_encode_gated_batch_device(
        n if count is None else count, arg("ins", ip.ctypes.data_as(_lib.vpp)), arg("lens", ln.ctypes.data_as(_lib.u64p)),
        arg("outs", op.ctypes.data_as(_lib.vpp)), arg("gates", gp.ctypes.data_as(_lib.vpp)),
        arg("ngates", ng.ctypes.data_as(C.POINTER(C.c_uint32))), arg("statuses", ST0), None)


def test_gated_encode_arguments(vds_lib):
    lens, ng = [100, 0, 7000, 3], [1, 32, 0, 70]
    for null in ("ins", "lens", "outs", "gates", "ngates", "statuses"):
        assert _gated(vds_lib, lens, ng, null=(null,)) == _lib.EINVAL, null
    assert _gated(vds_lib, lens, ng, count=1 << 30) == _lib.EINVAL
    assert _gated(vds_lib, lens, ng, null_gate=3) == _lib.EINVAL   # a gate of 70 bytes at a null address
    assert _gated(vds_lib, lens, ng, null_in=0) == _lib.EINVAL
    assert _gated(vds_lib, [1 << 32, 1], [0, 0]) == _lib.EINVAL
    assert _gated(vds_lib, [], [], count=0) == _lib.OK
    assert vds_lib.vds_ec_base64_encode_gated_batch_device(0, None, None, None, None, None, None, None) == _lib.OK
    if _no_device(vds_lib):
        assert _gated(vds_lib, lens, ng) == _lib.ENODEV
        assert _gated(vds_lib, lens, ng, null_gate=2) == _lib.ENODEV  # ungated: its gate is never read
        assert _gated(vds_lib, lens, ng, null_in=1) == _lib.ENODEV    # empty: its input is never read


# --------------------------------------------------------------- the host form
def _host(lib, k, sizes, witness=False, trailers=None, count=None, null=(), null_chunk=None, null_text=None,
          dup=False, bad_size=None, short_text=None, witness_id=1):
    """vds_ec_download16_host_batch on real host buffers (a failed validation
    transfers nothing).  trailers[o]: the first chunk's trailer of object o."""
    n_obj = len(sizes)
    k_arg, k = k, k or 16
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
    cs = np.asarray(csz if bad_size is None else [bad_size] + csz[1:], dtype=np.uint64)
    caps = [(L * k + 2) // 3 * 4 for L in csz]
    texts = [np.zeros(max(1, c), dtype=np.uint8) for c in caps]
    tl = np.asarray(caps, dtype=np.uint64)
    if short_text is not None:
        tl[short_text] = (sizes[short_text] + 2) // 3 * 4 - 1
    cp = (C.c_void_p * max(1, n_obj * k))(*[b.ctypes.data for row in bufs for b in row])
    tp = (C.c_void_p * max(1, n_obj))(*[t.ctypes.data for t in texts])
    if null_chunk is not None:
        cp[null_chunk] = None
    if null_text is not None:
        tp[null_text] = None
    sn = np.zeros(max(1, n_obj * k * 32), dtype=np.uint8)
    wi = np.full(max(1, n_obj), witness_id, dtype=np.uint16)
    wn = np.zeros(max(1, n_obj * 32), dtype=np.uint8)
    st = np.zeros(max(1, n_obj), dtype=np.int32)
    sv = np.zeros(max(1, n_obj * k), dtype=np.uint8)
    bad = C.c_uint32(77)

    def arg(name, value):
        return None if name in null else value

    return lib.vds_ec_download16_host_batch(
        k_arg, n_obj if count is None else count, arg("nodes", nodes.ctypes.data_as(_lib.u16p)), arg("chunks", cp),
        arg("sizes", cs.ctypes.data_as(_lib.u64p)), arg("survivor_names", sn.ctypes.data),
        arg("witness_ids", wi.ctypes.data_as(_lib.u16p)) if witness else None,
        arg("witness_names", wn.ctypes.data) if witness else None, arg("texts", tp),
        arg("text_lens", tl.ctypes.data_as(_lib.u64p)), arg("statuses", st.ctypes.data_as(C.POINTER(C.c_int32))),
        arg("survivor_verdicts", sv.ctypes.data), arg("failed", C.byref(bad)))


def test_download_host_batch_arguments(vds_lib):
    for witness in (False, True):
        for null in ("nodes", "chunks", "sizes", "survivor_names", "texts", "text_lens", "statuses",
                     "survivor_verdicts"):
            assert _host(vds_lib, 16, SIZES, witness, null=(null,)) == _lib.EINVAL, null
        assert _host(vds_lib, 0, SIZES, witness) == _lib.EINVAL
        assert _host(vds_lib, 16, SIZES, witness, count=1 << 30) == _lib.EINVAL
        assert _host(vds_lib, 16, SIZES, witness, null_chunk=16 * 2 + 9) == _lib.EINVAL
        assert _host(vds_lib, 16, SIZES, witness, null_text=1) == _lib.EINVAL
        assert _host(vds_lib, 16, SIZES, witness, bad_size=1) == _lib.EINVAL
        assert _host(vds_lib, 16, SIZES, witness, short_text=3) == _lib.EINVAL  # one character short
        assert _host(vds_lib, 16, SIZES, witness, dup=True) == _lib.ESINGULAR
        assert _host(vds_lib, 16, [], witness, count=0) == _lib.OK
    # the witness's id and name come together; a survivor is no witness
    assert _host(vds_lib, 16, SIZES, True, null=("witness_ids",)) == _lib.EINVAL
    assert _host(vds_lib, 16, SIZES, True, null=("witness_names",)) == _lib.EINVAL
    assert _host(vds_lib, 16, SIZES, True, witness_id=4) == _lib.EINVAL
    assert vds_lib.vds_ec_download16_host_batch(16, 0, None, None, None, None, None, None, None, None, None, None,
                                                None) == _lib.OK
    if _no_device(vds_lib):
        assert _host(vds_lib, 16, SIZES) == _lib.ENODEV
        assert _host(vds_lib, 16, SIZES, True, null=("failed",)) == _lib.ENODEV
        # a first trailer with no answer fails its object, not the call
        assert _host(vds_lib, 16, SIZES, True, trailers=[0, 33, 1, 0]) == _lib.ENODEV
        assert _host(vds_lib, 16, SIZES, False, trailers=[0, 0, 1, 65535]) == _lib.ENODEV
