"""Host side of the base64 wire text on the device
(vds_ec_base64_decode_batch_device / _encode_batch_device) and of the batched
upload from text (vds_ec_upload16_host_batch): the argument validation, which
runs before anything is enqueued and before the device is looked for.  No GPU:
the device pointers are fabricated integers, nothing dereferences them."""
import base64
import ctypes as C
import os
import re

import numpy as np

from vds_amd import _lib

TXT0 = 0x7F0000000000   # fabricated device addresses
OUT0 = 0x7E0000000000
ST0 = 0x7D0000000000
K, N = 32, 64
LENS = [88, 4, 0, 1024, 8]           # characters
SIZES = [66, 1, 0, 767, 4]           # len/4*3 - p for p = 0, 2, 0, 1, 2
I32P = C.POINTER(C.c_int32)
U32P = C.POINTER(C.c_uint32)


def _no_device(lib):
    cnt = C.c_int(0)
    assert lib.vds_ec_device_count(C.byref(cnt)) == 0
    return cnt.value == 0


def _ptrs(base, lens, pitch=1 << 20):
    return [base + i * pitch for i in range(len(lens))]


def _dec(lib, lens=LENS, sizes=SIZES, texts=None, outs=None, statuses=ST0, count=None, null=()):
    tp = np.asarray(_ptrs(TXT0, lens) if texts is None else texts, dtype=np.uint64)
    op = np.asarray(_ptrs(OUT0, lens) if outs is None else outs, dtype=np.uint64)
    tl = np.asarray(lens, dtype=np.uint64)
    os_ = np.asarray(sizes, dtype=np.uint64)
    return lib.vds_ec_base64_decode_batch_device(len(lens) if count is None else count,
                                                 None if "texts" in null else tp.ctypes.data_as(_lib.vpp),
                                                 None if "lens" in null else tl.ctypes.data_as(_lib.u64p),
                                                 None if "outs" in null else op.ctypes.data_as(_lib.vpp),
                                                 None if "sizes" in null else os_.ctypes.data_as(_lib.u64p),
                                                 statuses, None)


def _enc(lib, lens, ins=None, outs=None, count=None, null=()):
    ip = np.asarray(_ptrs(TXT0, lens) if ins is None else ins, dtype=np.uint64)
    op = np.asarray(_ptrs(OUT0, lens) if outs is None else outs, dtype=np.uint64)
    ln = np.asarray(lens, dtype=np.uint64)
    return lib.vds_ec_base64_encode_batch_device(len(lens) if count is None else count,
                                                 None if "ins" in null else ip.ctypes.data_as(_lib.vpp),
                                                 None if "lens" in null else ln.ctypes.data_as(_lib.u64p),
                                                 None if "outs" in null else op.ctypes.data_as(_lib.vpp), None)


class Upload:
    """Real host buffers for one call of vds_ec_upload16_host_batch."""

    def __init__(self, texts, k=K, n=N):
        self.k, self.n, self.texts = k, n, texts
        self.count = len(texts)
        self.lens = np.asarray([len(t) for t in texts], dtype=np.uint64)
        self.tp = (C.c_char_p * max(1, self.count))(*texts)
        self.outs = [np.zeros(70000, dtype=np.uint8) for _ in range(self.count * n)]
        self.op = (C.c_void_p * max(1, self.count * n))(*[o.ctypes.data for o in self.outs])
        self.rd = np.zeros(max(1, 32 * self.count * n), dtype=np.uint8)
        self.st = np.zeros(max(1, self.count), dtype=np.int32)

    def call(self, lib, count=None, k=None, n=None, null=(), lens=None, tp=None, op=None):
        ln = self.lens if lens is None else np.asarray(lens, dtype=np.uint64)
        return lib.vds_ec_upload16_host_batch(
            self.k if k is None else k, self.n if n is None else n, self.count if count is None else count,
            None if "texts" in null else C.cast(self.tp if tp is None else tp, _lib.vpp),
            None if "lens" in null else ln.ctypes.data_as(_lib.u64p),
            None if "outs" in null else (self.op if op is None else op),
            None if "rd" in null else self.rd.ctypes.data, None, None, None, None,
            None if "statuses" in null else self.st.ctypes.data_as(I32P), None)


def test_decode_invalid_arguments(vds_lib):
    for null in ("texts", "lens", "outs", "sizes"):
        assert _dec(vds_lib, null=(null,)) == _lib.EINVAL, null
    assert _dec(vds_lib, statuses=None) == _lib.EINVAL
    assert _dec(vds_lib, count=1 << 30) == _lib.EINVAL
    # a null text or output where a length is non-zero (allowed where it is zero)
    texts, outs = _ptrs(TXT0, LENS), _ptrs(OUT0, LENS)
    assert _dec(vds_lib, texts=[0] + texts[1:]) == _lib.EINVAL
    assert _dec(vds_lib, outs=outs[:3] + [0] + outs[4:]) == _lib.EINVAL
    # a text of 2^32 characters or more
    assert _dec(vds_lib, lens=[1 << 32], sizes=[(1 << 30) * 3]) == _lib.EINVAL
    assert _dec(vds_lib, lens=[(1 << 32) + 4], sizes=[(1 << 30) * 3 + 3]) == _lib.EINVAL
    # a declared size that no text of that length decodes to
    for ln, sz in ((88, 67), (88, 63), (88, 0), (4, 4), (4, 0), (0, 1), (8, 7), (5, 3), (6, 1), (7, 5), (3, 2)):
        assert _dec(vds_lib, lens=[8, ln], sizes=[6, sz]) == _lib.EINVAL, (ln, sz)


def test_encode_invalid_arguments(vds_lib):
    lens = [66, 1, 0, 767]
    for null in ("ins", "lens", "outs"):
        assert _enc(vds_lib, lens, null=(null,)) == _lib.EINVAL, null
    assert _enc(vds_lib, lens, count=1 << 30) == _lib.EINVAL
    ins, outs = _ptrs(TXT0, lens), _ptrs(OUT0, lens)
    assert _enc(vds_lib, lens, ins=[0] + ins[1:]) == _lib.EINVAL
    assert _enc(vds_lib, lens, outs=outs[:1] + [0] + outs[2:]) == _lib.EINVAL
    assert _enc(vds_lib, [5, 1 << 32]) == _lib.EINVAL


def test_upload_invalid_arguments(vds_lib):
    body = bytes(range(200))
    u = Upload([base64.b64encode(body[:s]) for s in (0, 1, 2, 3, 100, 200)])
    for null in ("texts", "lens", "outs", "rd", "statuses"):
        assert u.call(vds_lib, null=(null,)) == _lib.EINVAL, null
    assert u.call(vds_lib, k=0) == _lib.EINVAL
    assert u.call(vds_lib, n=65537) == _lib.EINVAL
    assert u.call(vds_lib, count=1 << 30) == _lib.EINVAL
    assert u.call(vds_lib, count=(1 << 32) // (N + 64) + 1) == _lib.EINVAL  # the hash launch's lanes
    # a text of 2^32 characters or more; a null text with a non-zero length; a null replica buffer
    assert u.call(vds_lib, lens=[int(x) for x in u.lens[:5]] + [1 << 32]) == _lib.EINVAL
    tp = (C.c_char_p * u.count)(*(u.texts[:4] + [None] + u.texts[5:]))
    assert u.call(vds_lib, tp=tp) == _lib.EINVAL
    op = (C.c_void_p * (u.count * N))(*[o.ctypes.data for o in u.outs])
    op[3 * N + 7] = None
    assert u.call(vds_lib, op=op) == _lib.EINVAL
    assert (u.st == 0).all() and not u.rd.any(), "a rejected call wrote something"


def test_empty_batches_are_ok(vds_lib):
    assert vds_lib.vds_ec_base64_decode_batch_device(0, None, None, None, None, None, None) == _lib.OK
    assert vds_lib.vds_ec_base64_encode_batch_device(0, None, None, None, None) == _lib.OK
    assert _dec(vds_lib, count=0) == _lib.OK
    assert _enc(vds_lib, [3, 4], count=0) == _lib.OK
    failed = C.c_uint32(7)
    assert vds_lib.vds_ec_upload16_host_batch(K, N, 0, None, None, None, None, None, None, None, None, None,
                                              C.byref(failed)) == _lib.OK
    assert failed.value == 0


def test_valid_calls_need_a_device(vds_lib):
    """Validation comes first, the device check second (where a GPU is present
    this test has nothing to assert and the GPU suite covers the calls)."""
    if not _no_device(vds_lib):
        return
    assert _dec(vds_lib) == _lib.ENODEV
    assert _dec(vds_lib, lens=[8, 5, 0], sizes=[5, 0, 0], texts=[TXT0, TXT0 + 99, 0], outs=[OUT0, 0, 0]) == \
        _lib.ENODEV
    assert _enc(vds_lib, [66, 1, 0, 767]) == _lib.ENODEV
    assert _enc(vds_lib, [0, 0], ins=[0, 0], outs=[0, 0]) == _lib.ENODEV
    body = bytes(range(200))
    u = Upload([base64.b64encode(body[:s]) for s in (0, 1, 100)] + [b"QUJ", b"A=AA", b"AA*A"])
    assert u.call(vds_lib) == _lib.ENODEV
    assert (u.st == 0).all(), "statuses written without a device"


def test_header_entry_points_are_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "vds_ec.h")).read(), flags=re.S)
    for name in ("vds_ec_base64_decode_batch_device", "vds_ec_base64_encode_batch_device",
                 "vds_ec_upload16_host_batch"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
