"""Python mirror of lboss75/vds kernel/vds_data's chunk-transform API.

Same names, argument meaning and error behaviour as the reference's C++
templates (chunk.h:59-114, chunk_storage.h:13-34), backed by the HIP kernels
through the C ABI.  `cell_bytes` selects the uint16_t (2, production) or
uint8_t (1) instantiation.

  ChunkGenerator(k, n).write(data, write_padding=True)   chunk.h:245-281
  ChunkGenerator.write_padding(size)                     chunk.h:283-287
  chunk_cells(generator, cells)                          chunk.h:206-224
  ChunkRestore(k, nodes).restore(chunks)                 chunk.h:290-444
  ChunkRestore.restore_cells(chunks)                     chunk.h:383-400
  ChunkStorage(min_horcrux).generate_replica / restore_data
                                                         chunk_storage.cpp:41-86
  encode_device / restore_device                          batched device-memory
                                                         forms for torch tensors
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Iterable, Mapping, Sequence

import numpy as np

from . import _lib
from ._lib import F_CELLS, F_NO_TRAILER, VdsEcError, check

__all__ = [
    "ChunkGenerator", "ChunkRestore", "ChunkStorage", "chunk_cells", "replica_size",
    "encode_device", "restore_device", "fill_splitmix_device", "encode_host_batch", "restore_host_batch",
    "regenerate_host",
    "regenerate_device", "sha256_device", "encode_hash_host", "replica_storage_paths",
    "VdsEcError", "multipliers", "inverse", "encode_range_device", "restore_range_device", "encode_host_split",
    "restore_host_split", "sha256_batch_device", "save_temp_batch_device", "save_temp_batch",
    "base64_decode_batch_device", "base64_encode_batch_device", "upload_batch",
    "base64_encode_gated_batch_device", "download_batch_device", "download_batch",
    "hmac_sha256_host", "dgram_layout", "write_number", "hmac_sha256_batch_device", "dgram_seal_batch_device",
    "dgram_open_batch_device", "dgram_seal_batch", "dgram_open_batch",
    "ws_frame_parse", "ws_frame_header", "ws_upload_request", "ws_upload_answer_size", "ws_download_answer_layout",
    "ws_error_answer", "base64_decode_masked_batch_device", "ws_upload_answer_batch_device", "ws_upload_batch",
    "ws_download_batch",
]


def _u8(data) -> np.ndarray:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(data), dtype=np.uint8)
    return np.ascontiguousarray(data).view(np.uint8).reshape(-1)


def _ids(values: Iterable[int], cell_bytes: int) -> np.ndarray:
    dt = np.uint16 if cell_bytes == 2 else np.uint8
    return np.ascontiguousarray(np.asarray(list(values), dtype=np.int64).astype(dt))


def _idp(a: np.ndarray, cell_bytes: int):
    return a.ctypes.data_as(_lib.u16p if cell_bytes == 2 else _lib.u8p)


def replica_size(k: int, size: int, cell_bytes: int = 2, write_padding: bool = True) -> int:
    return int(_lib.lib().vds_ec_replica_size(cell_bytes, k, size, 0 if write_padding else F_NO_TRAILER))


def multipliers(k: int, node: int, cell_bytes: int = 2) -> np.ndarray:
    """chunk<cell>::generate_multipliers (chunk.h:183-194)."""
    dt = np.uint16 if cell_bytes == 2 else np.uint8
    out = np.zeros(k, dtype=dt)
    f = _lib.lib().vds_ec_multipliers16 if cell_bytes == 2 else _lib.lib().vds_ec_multipliers8
    check(f(k, node, _idp(out, cell_bytes)))
    return out


def inverse(k: int, nodes: Sequence[int], cell_bytes: int = 2) -> np.ndarray:
    """The chunk_restore<cell>(k, n) multipliers matrix (chunk.h:290-375)."""
    ids = _ids(nodes, cell_bytes)
    dt = np.uint16 if cell_bytes == 2 else np.uint8
    out = np.zeros(k * k, dtype=dt)
    f = _lib.lib().vds_ec_inverse16 if cell_bytes == 2 else _lib.lib().vds_ec_inverse8
    check(f(k, _idp(ids, cell_bytes), _idp(out, cell_bytes)), "chunk_restore")
    return out.reshape(k, k)


class ChunkGenerator:
    """chunk_generator<cell>(k, n) (chunk.h:59-88, 232-243)."""

    def __init__(self, k: int, n: int, cell_bytes: int = 2):
        if cell_bytes not in (1, 2):
            raise ValueError("cell_bytes must be 1 (uint8_t) or 2 (uint16_t)")
        limit = 0xFFFF if cell_bytes == 2 else 0xFF
        self._k = int(k) & limit  # cell_type arithmetic
        self._n = int(n) & limit
        self.cell_bytes = cell_bytes
        self._mult = multipliers(self._k, self._n, cell_bytes)

    def k(self) -> int:
        return self._k

    def n(self) -> int:
        return self._n

    def multipliers(self) -> np.ndarray:
        return self._mult

    def write(self, data, write_padding: bool = True) -> np.ndarray:
        """Bytes chunk_generator::write appends to the serializer."""
        return encode_host(self._k, [self._n], data, self.cell_bytes, write_padding)[0]

    def write_padding(self, size: int) -> np.ndarray:
        pad = size % (self.cell_bytes * self._k)  # chunk.h:286
        return np.array([(pad >> 8) & 0xFF, pad & 0xFF], dtype=np.uint8)


def encode_host(k: int, replicas: Sequence[int], data, cell_bytes: int = 2,
                write_padding: bool = True, cells: bool = False) -> list:
    """All requested replicas of one host object in one device pass."""
    buf = _u8(data)
    ids = _ids(replicas, cell_bytes)
    flags = (0 if write_padding else F_NO_TRAILER) | (F_CELLS if cells else 0)
    L = int(_lib.lib().vds_ec_replica_size(cell_bytes, k, buf.size, flags))
    outs = [np.empty(max(L, 1), dtype=np.uint8) for _ in range(ids.size)]
    ptrs = (C.c_void_p * max(1, ids.size))(*[o.ctypes.data for o in outs])
    f = _lib.lib().vds_ec_encode16_host if cell_bytes == 2 else _lib.lib().vds_ec_encode8_host
    check(f(k, _idp(ids, cell_bytes), ids.size, buf.ctypes.data if buf.size else None, buf.size, ptrs, flags),
          "chunk_generator::write")
    return [o[:L] for o in outs]


def chunk_cells(generator: ChunkGenerator, cells) -> np.ndarray:
    """chunk<cell>(generator, data, len).data() (chunk.h:206-224)."""
    dt = np.uint16 if generator.cell_bytes == 2 else np.uint8
    arr = np.ascontiguousarray(cells, dtype=dt)
    out = encode_host(generator.k(), [generator.n()], arr.view(np.uint8), generator.cell_bytes, cells=True)[0]
    return out.view(dt).copy()


class ChunkRestore:
    """chunk_restore<cell>(k, n) (chunk.h:90-114, 290-444)."""

    def __init__(self, k: int, nodes: Sequence[int], cell_bytes: int = 2):
        self._k = int(k)
        self.cell_bytes = cell_bytes
        self._nodes = _ids(nodes, cell_bytes)
        if self._nodes.size < self._k:
            raise ValueError("chunk_restore needs k replica ids")
        self._nodes = self._nodes[: self._k]
        self._error = None
        try:
            self._mult = inverse(self._k, self._nodes, cell_bytes)
        except VdsEcError as e:  # duplicate ids: the reference yields garbage here
            self._mult = None
            self._error = e

    def multipliers(self) -> np.ndarray:
        if self._error is not None:
            raise self._error
        return self._mult

    def restore(self, chunks: Sequence) -> np.ndarray:
        """chunk_restore::restore(const std::vector<const_data_buffer>&)."""
        if self._error is not None:
            raise self._error
        bufs = [_u8(c) for c in chunks[: self._k]]
        if len(bufs) < self._k:
            raise VdsEcError(_lib.EINVAL, "chunk_restore::restore")
        size = bufs[0].size
        if any(b.size != size for b in bufs):
            raise VdsEcError(_lib.EINVAL, "chunk_restore::restore")
        # a corrupt trailer can make the reference return up to size*k bytes (chunk.h:415-441)
        out = np.empty(max(1, size * self._k), dtype=np.uint8)
        out_size = C.c_uint64(0)
        ptrs = (C.c_void_p * self._k)(*[b.ctypes.data for b in bufs])
        f = _lib.lib().vds_ec_restore16_host if self.cell_bytes == 2 else _lib.lib().vds_ec_restore8_host
        check(f(self._k, _idp(self._nodes, self.cell_bytes), ptrs, size, out.ctypes.data, C.byref(out_size), 0),
              "chunk_restore::restore")
        return out[: out_size.value]

    def restore_cells(self, chunks: Sequence) -> np.ndarray:
        """chunk_restore::restore(std::vector<cell>&, const chunk<cell>**)."""
        if self._error is not None:
            raise self._error
        dt = np.uint16 if self.cell_bytes == 2 else np.uint8
        arrs = [np.ascontiguousarray(c, dtype=dt) for c in chunks[: self._k]]
        n_cells = arrs[0].size
        out = np.empty(max(1, n_cells * self._k), dtype=dt)
        out_size = C.c_uint64(0)
        ptrs = (C.c_void_p * self._k)(*[a.ctypes.data for a in arrs])
        f = _lib.lib().vds_ec_restore16_host if self.cell_bytes == 2 else _lib.lib().vds_ec_restore8_host
        check(f(self._k, _idp(self._nodes, self.cell_bytes), ptrs, n_cells * self.cell_bytes, out.ctypes.data,
                C.byref(out_size), F_CELLS), "chunk_restore::restore")
        return out[: n_cells * self._k]


class ChunkStorage:
    """chunk_storage (chunk_storage.h:13-34, chunk_storage.cpp:10-86)."""

    def __init__(self, min_horcrux: int):
        self.min_horcrux = int(min_horcrux) & 0xFFFF
        self._generators: Dict[int, ChunkGenerator] = {}

    def generate_replica(self, replica: int, data) -> np.ndarray:
        g = self._generators.get(replica)
        if g is None:
            g = self._generators[replica] = ChunkGenerator(self.min_horcrux, replica)
        return g.write(data)

    def generate_replicas(self, replicas: Sequence[int], data) -> list:
        """Batched form of generate_replica for the save_temp / save_data loops."""
        return encode_host(self.min_horcrux, replicas, data)

    def regenerate_replicas(self, horcruxes: Mapping[int, object], targets: Sequence[int]) -> list:
        """Replicas `targets` from exactly min_horcrux equal-size horcruxes, in
        one pass (the repair's restore_data + generate_replica, fused)."""
        if self.min_horcrux != len(horcruxes):
            raise VdsEcError(_lib.EINVAL, "Error at restoring data")
        items = list(horcruxes.items())
        return regenerate_host(self.min_horcrux, [r for r, _ in items], [v for _, v in items], targets)

    def restore_data(self, horcruxes: Mapping[int, object]) -> np.ndarray:
        if self.min_horcrux != len(horcruxes):
            raise VdsEcError(_lib.EINVAL, "Error at restoring data")  # chunk_storage.cpp:65-67
        items = list(horcruxes.items())
        size = _u8(items[0][1]).size
        for _, v in items:
            if _u8(v).size != size:
                raise VdsEcError(_lib.EINVAL, "Error at restoring data")  # chunk_storage.cpp:76-78
        return ChunkRestore(self.min_horcrux, [r for r, _ in items]).restore([v for _, v in items])


# --------------------------------------------------------------- device forms

def _stream_ptr(stream) -> int | None:
    """A hipStream_t for the C ABI: None = torch's current stream; a
    torch.cuda.Stream or a raw handle otherwise."""
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    if hasattr(stream, "cuda_stream"):
        return stream.cuda_stream
    return int(stream)


def encode_device(k: int, replicas: Sequence[int], inp, size: int, in_stride: int, count: int,
                  outs: Sequence[int], out_stride: int, write_padding: bool = True, stream=None) -> None:
    """vds_ec_encode16_device on raw device pointers (ints) / torch tensors."""
    ids = _ids(replicas, 2)
    ptrs = (C.c_void_p * ids.size)(*[int(o) for o in outs])
    in_ptr = inp.data_ptr() if hasattr(inp, "data_ptr") else int(inp)
    check(_lib.lib().vds_ec_encode16_device(k, _idp(ids, 2), ids.size, in_ptr, size, in_stride, count, ptrs,
                                            out_stride, 0 if write_padding else F_NO_TRAILER,
                                            _stream_ptr(stream)), "encode16_device")


def restore_device(k: int, nodes: Sequence[int], chunks: Sequence[int], chunk_size: int, chunk_stride: int,
                   padding: int, count: int, out, out_stride: int, stream=None) -> None:
    ids = _ids(nodes, 2)
    ptrs = (C.c_void_p * ids.size)(*[int(c) for c in chunks])
    out_ptr = out.data_ptr() if hasattr(out, "data_ptr") else int(out)
    check(_lib.lib().vds_ec_restore16_device(k, _idp(ids, 2), ptrs, chunk_size, chunk_stride, padding, count,
                                             out_ptr, out_stride, 0, _stream_ptr(stream)), "restore16_device")


def encode_range_device(k: int, replicas: Sequence[int], inp, size: int, t0: int, t1: int, outs: Sequence[int],
                        write_padding: bool = True, stream=None) -> None:
    """vds_ec_encode16_range_device: stripes [t0, t1) of one device object
    into replica bytes [2 t0, 2 t1) of the whole replica buffers `outs`
    (SURVEY.md 8(e) stripe-range split)."""
    ids = _ids(replicas, 2)
    ptrs = (C.c_void_p * max(1, ids.size))(*[int(o) for o in outs])
    in_ptr = inp.data_ptr() if hasattr(inp, "data_ptr") else int(inp)
    check(_lib.lib().vds_ec_encode16_range_device(k, _idp(ids, 2), ids.size, in_ptr, size, t0, t1, ptrs,
                                                  0 if write_padding else F_NO_TRAILER, _stream_ptr(stream)),
          "encode16_range_device")


def restore_range_device(k: int, nodes: Sequence[int], chunks: Sequence[int], chunk_size: int, padding: int,
                         t0: int, t1: int, out, stream=None) -> None:
    """vds_ec_restore16_range_device: object bytes [2k t0, min(2k t1, E)) of
    `out` from stripes [t0, t1) of the whole survivor buffers."""
    ids = _ids(nodes, 2)
    ptrs = (C.c_void_p * ids.size)(*[int(c) for c in chunks])
    out_ptr = out.data_ptr() if hasattr(out, "data_ptr") else int(out)
    check(_lib.lib().vds_ec_restore16_range_device(k, _idp(ids, 2), ptrs, chunk_size, padding, t0, t1, out_ptr, 0,
                                                   _stream_ptr(stream)), "restore16_range_device")


def encode_host_split(k: int, replicas: Sequence[int], data, parts: int = 0, max_devices: int = 0) -> list:
    """One host object over the GPUs by stripe ranges (vds_ec_encode16_host_split);
    returns the n replicas."""
    ids = _ids(replicas, 2)
    buf = _u8(data)
    L = replica_size(k, buf.size)
    outs = [np.empty(max(L, 1), dtype=np.uint8) for _ in range(ids.size)]
    ptrs = (C.c_void_p * max(1, ids.size))(*[o.ctypes.data for o in outs])
    check(_lib.lib().vds_ec_encode16_host_split(k, _idp(ids, 2), ids.size, buf.ctypes.data, buf.size, ptrs, 0,
                                                max_devices, parts), "encode16_host_split")
    return [o[:L] for o in outs]


def restore_host_split(k: int, nodes: Sequence[int], chunks: Sequence, parts: int = 0, max_devices: int = 0):
    """One object restored over the GPUs by stripe ranges from k host
    replicas (vds_ec_restore16_host_split); returns the restored bytes."""
    ids = _ids(nodes, 2)
    bufs = [_u8(c) for c in chunks]
    cs = bufs[0].size
    out = np.empty(max(cs * k, 1), dtype=np.uint8)
    n_out = C.c_uint64(out.size)
    ptrs = (C.c_void_p * ids.size)(*[b.ctypes.data for b in bufs])
    check(_lib.lib().vds_ec_restore16_host_split(k, _idp(ids, 2), ptrs, cs, out.ctypes.data, C.byref(n_out), 0,
                                                 max_devices, parts), "restore16_host_split")
    return out[: n_out.value]


def restore_batch_device(k: int, nodes: Sequence[Sequence[int]], chunks: Sequence[Sequence[int]],
                         chunk_sizes: Sequence[int], paddings: Sequence[int], outs: Sequence[int],
                         stream=None) -> None:
    """vds_ec_restore16_batch_device: object o restored from its own survivors
    nodes[o] at device pointers chunks[o] (chunk_sizes[o] bytes, trailer
    value paddings[o]) into the device pointer outs[o]."""
    count = len(nodes)
    ids = _ids([r for nd in nodes for r in nd], 2)
    cp = (C.c_void_p * max(1, count * k))(*[int(c) for ch in chunks for c in ch])
    cs = np.asarray(chunk_sizes, dtype=np.uint64)
    pd = np.asarray(paddings, dtype=np.uint16)
    op = (C.c_void_p * max(1, count))(*[int(o) for o in outs])
    check(_lib.lib().vds_ec_restore16_batch_device(k, count, _idp(ids, 2), cp, cs.ctypes.data_as(_lib.u64p),
                                                   pd.ctypes.data_as(_lib.u16p), op, 0, _stream_ptr(stream)),
          "restore16_batch_device")


def regenerate_batch_device(k: int, nodes: Sequence[Sequence[int]], chunks: Sequence[Sequence[int]],
                            chunk_sizes: Sequence[int], targets: Sequence[Sequence[int]],
                            outs: Sequence[Sequence[int]], stream=None) -> None:
    """vds_ec_regenerate16_batch_device: replicas targets[o] of object o from
    its own survivors, into the device pointers outs[o]."""
    count = len(nodes)
    nt = len(targets[0]) if count else 0
    ids = _ids([r for nd in nodes for r in nd], 2)
    tg = _ids([t for ts in targets for t in ts], 2)
    cp = (C.c_void_p * max(1, count * k))(*[int(c) for ch in chunks for c in ch])
    cs = np.asarray(chunk_sizes, dtype=np.uint64)
    op = (C.c_void_p * max(1, count * nt))(*[int(x) for os_ in outs for x in os_])
    check(_lib.lib().vds_ec_regenerate16_batch_device(k, count, _idp(ids, 2), cp, cs.ctypes.data_as(_lib.u64p), nt,
                                                      _idp(tg, 2), op, _stream_ptr(stream)),
          "regenerate16_batch_device")


def _encode_batch_args(k: int, replicas: Sequence[int], ins, sizes, outs):
    """The host arrays of the batched encode: ins (count device pointers),
    sizes (count) and outs (count x n device pointers, row o = object o's
    replicas), from sequences or numpy arrays of ints.  The arrays are
    returned too: they must outlive the call."""
    ids = _ids(replicas, 2)
    ip = np.ascontiguousarray(np.asarray(ins, dtype=np.uint64).reshape(-1))
    sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.uint64).reshape(-1))
    op = np.ascontiguousarray(np.asarray(outs, dtype=np.uint64).reshape(-1))
    if sz.size != ip.size or op.size != ip.size * ids.size:
        raise VdsEcError(_lib.EINVAL, "encode_batch: ins, sizes and outs do not describe one batch")
    return ids, ip, sz, op


def encode_batch_device(k: int, replicas: Sequence[int], ins, sizes, outs, write_padding: bool = True,
                        stream=None) -> None:
    """vds_ec_encode16_batch_device: object o (sizes[o] bytes at the device
    pointer ins[o]) encoded into the device pointers outs[o][i], one per
    replica id; objects of any sizes share one bit-sliced launch."""
    ids, ip, sz, op = _encode_batch_args(k, replicas, ins, sizes, outs)
    check(_lib.lib().vds_ec_encode16_batch_device(k, _idp(ids, 2), ids.size, ip.size, ip.ctypes.data_as(_lib.vpp),
                                                  sz.ctypes.data_as(_lib.u64p), op.ctypes.data_as(_lib.vpp),
                                                  0 if write_padding else F_NO_TRAILER, _stream_ptr(stream)),
          "encode16_batch_device")


def encode_batch_path(k: int, replicas: Sequence[int], ins, sizes, outs, write_padding: bool = True):
    """vds_ec_encode16_batch_path: (path, fast_objects) of the batch call with
    these arguments -- 2 when objects ride the shared bit-sliced launch, and
    how many do.  Host only: the pointers are never dereferenced."""
    ids, ip, sz, op = _encode_batch_args(k, replicas, ins, sizes, outs)
    fast = C.c_uint32(0)
    path = _lib.lib().vds_ec_encode16_batch_path(k, _idp(ids, 2), ids.size, ip.size, ip.ctypes.data_as(_lib.vpp),
                                                 sz.ctypes.data_as(_lib.u64p), op.ctypes.data_as(_lib.vpp),
                                                 0 if write_padding else F_NO_TRAILER, C.byref(fast))
    return int(path), int(fast.value)


def regenerate_host(k: int, nodes: Sequence[int], chunks: Sequence, targets: Sequence[int]) -> list:
    """vds_ec_regenerate16_host: replicas `targets` of one object from k
    survivor replicas (host buffers), bytes as restore + re-encode."""
    ids = _ids(nodes, 2)[:k]
    tg = _ids(targets, 2)
    bufs = [_u8(c) for c in chunks[:k]]
    if len(bufs) < k or any(b.size != bufs[0].size for b in bufs):
        raise VdsEcError(_lib.EINVAL, "regenerate")
    size = bufs[0].size
    outs = [np.empty(max(size, 1), dtype=np.uint8) for _ in range(tg.size)]
    cp = (C.c_void_p * k)(*[b.ctypes.data for b in bufs])
    op = (C.c_void_p * max(1, tg.size))(*[o.ctypes.data for o in outs])
    check(_lib.lib().vds_ec_regenerate16_host(k, _idp(ids, 2), cp, size, _idp(tg, 2), tg.size, op), "regenerate")
    return [o[:size] for o in outs]


def regenerate_device(k: int, nodes: Sequence[int], chunks: Sequence[int], chunk_size: int, chunk_stride: int,
                      count: int, targets: Sequence[int], outs: Sequence[int], out_stride: int, stream=None) -> None:
    ids = _ids(nodes, 2)
    tg = _ids(targets, 2)
    cp = (C.c_void_p * ids.size)(*[int(c) for c in chunks])
    op = (C.c_void_p * max(1, tg.size))(*[int(o) for o in outs])
    check(_lib.lib().vds_ec_regenerate16_device(k, _idp(ids, 2), cp, chunk_size, chunk_stride, count, _idp(tg, 2),
                                                tg.size, op, out_stride, _stream_ptr(stream)), "regenerate16_device")


def sha256_device(base, length: int, stride: int, count: int, digests, stream=None) -> None:
    """SHA-256 of `count` device messages of `length` bytes at base + j*stride
    into digests (device, 32*count bytes): the replica names of
    dht_network_client.cpp:79 / :593."""
    bp = base.data_ptr() if hasattr(base, "data_ptr") else int(base)
    dp = digests.data_ptr() if hasattr(digests, "data_ptr") else int(digests)
    check(_lib.lib().vds_ec_sha256_device(bp, length, stride, count, dp, _stream_ptr(stream)), "sha256_device")


def _dev_ptr(x) -> int | None:
    """A device address for a void* argument: a tensor, an int, or None (NULL)."""
    if x is None:
        return None
    return x.data_ptr() if hasattr(x, "data_ptr") else int(x)


def sha256_batch_device(msgs, lens, digests, stream=None) -> None:
    """vds_ec_sha256_batch_device: SHA-256 of len(lens) device messages of
    different lengths in one launch -- message j is lens[j] bytes at the
    device pointer msgs[j] (0 allowed where lens[j] == 0); digest j goes to
    digests + 32 j (device)."""
    mp = np.ascontiguousarray(np.asarray(msgs, dtype=np.uint64).reshape(-1))
    ln = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64).reshape(-1))
    if mp.size != ln.size:
        raise VdsEcError(_lib.EINVAL, "sha256_batch: msgs and lens do not describe one batch")
    check(_lib.lib().vds_ec_sha256_batch_device(ln.size, mp.ctypes.data_as(_lib.vpp), ln.ctypes.data_as(_lib.u64p),
                                                _dev_ptr(digests), _stream_ptr(stream)), "sha256_batch_device")


def sha256_check_batch_device(msgs, lens, expected, verdicts, digests=None, stream=None) -> None:
    """vds_ec_sha256_check_batch_device: as sha256_batch_device, and digest j
    compared with the 32 bytes at expected + 32 j into verdicts[j] (device
    buffers; 0 equal, 1 different).  digests None: check only."""
    mp = np.ascontiguousarray(np.asarray(msgs, dtype=np.uint64).reshape(-1))
    ln = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64).reshape(-1))
    if mp.size != ln.size:
        raise VdsEcError(_lib.EINVAL, "sha256_check_batch: msgs and lens do not describe one batch")
    check(_lib.lib().vds_ec_sha256_check_batch_device(ln.size, mp.ctypes.data_as(_lib.vpp),
                                                      ln.ctypes.data_as(_lib.u64p), _dev_ptr(expected),
                                                      _dev_ptr(digests), _dev_ptr(verdicts), _stream_ptr(stream)),
          "sha256_check_batch_device")


def repair_batch_device(k: int, nodes: Sequence[Sequence[int]], chunks: Sequence[Sequence[int]],
                        chunk_sizes: Sequence[int], targets: Sequence[Sequence[int]],
                        outs: Sequence[Sequence[int]], digests, expected=None, verdicts=None, stream=None) -> None:
    """vds_ec_repair16_batch_device: regenerate_batch_device, then replica
    targets[o][i] named at digests + 32 (o nt + i) and, with expected, checked
    against expected + 32 (o nt + i) into verdicts[o nt + i] (device buffers),
    names and verdicts in one launch."""
    count = len(nodes)
    nt = len(targets[0]) if count else 0
    ids = _ids([r for nd in nodes for r in nd], 2)
    tg = _ids([t for ts in targets for t in ts], 2)
    cp = (C.c_void_p * max(1, count * k))(*[int(c) for ch in chunks for c in ch])
    cs = np.asarray(chunk_sizes, dtype=np.uint64)
    op = (C.c_void_p * max(1, count * nt))(*[int(x) for os_ in outs for x in os_])
    check(_lib.lib().vds_ec_repair16_batch_device(k, count, _idp(ids, 2), cp, cs.ctypes.data_as(_lib.u64p), nt,
                                                  _idp(tg, 2), op, _dev_ptr(digests), _dev_ptr(expected),
                                                  _dev_ptr(verdicts), _stream_ptr(stream)),
          "repair16_batch_device")


def repair_batch(k: int, horcruxes: Sequence[Mapping[int, object]], targets: Sequence[Sequence[int]],
                 expected=None) -> list:
    """vds_ec_repair16_host_batch: the repair loop for a batch of host objects.
    horcruxes[o] maps replica id -> bytes (its first k entries are used, in
    order); targets[o] lists the ids to regenerate (every object the same
    number); expected, when given, holds per object the names those replicas
    must have (32 bytes each).  Returns per object (replicas, names, verdicts
    or None)."""
    count = len(horcruxes)
    nt = len(targets[0]) if count else 0
    items = [list(h.items())[:k] for h in horcruxes]
    if any(len(it) < k for it in items) or any(len(t) != nt for t in targets):
        raise VdsEcError(_lib.EINVAL, "repair_batch")
    ids = _ids([r for it in items for r, _ in it], 2)
    tg = _ids([t for ts in targets for t in ts], 2)
    bufs = [[_u8(v) for _, v in it] for it in items]
    if any(b.size != bs[0].size for bs in bufs for b in bs):
        raise VdsEcError(_lib.EINVAL, "repair_batch")
    cs = np.asarray([bs[0].size for bs in bufs], dtype=np.uint64)
    outs = [[np.empty(max(int(c), 1), dtype=np.uint8) for _ in range(nt)] for c in cs]
    dg = np.empty((max(1, count * nt), 32), dtype=np.uint8)
    ex = vd = None
    if expected is not None:
        ex = np.ascontiguousarray(np.frombuffer(b"".join(bytes(e) for es in expected for e in es), dtype=np.uint8))
        if ex.size != 32 * count * nt:
            raise VdsEcError(_lib.EINVAL, "repair_batch: expected does not hold one name per target")
        vd = np.zeros(max(1, count * nt), dtype=np.uint8)
    bad = C.c_uint32(0)
    cp = (C.c_void_p * max(1, count * k))(*[b.ctypes.data for bs in bufs for b in bs])
    op = (C.c_void_p * max(1, count * nt))(*[o.ctypes.data for os_ in outs for o in os_])
    check(_lib.lib().vds_ec_repair16_host_batch(k, count, _idp(ids, 2), cp, cs.ctypes.data_as(_lib.u64p), nt,
                                                _idp(tg, 2), op, dg.ctypes.data,
                                                ex.ctypes.data if ex is not None and ex.size else None,
                                                vd.ctypes.data if vd is not None and ex.size else None,
                                                C.byref(bad)), "repair16_host_batch")
    return [([r[:int(cs[o])] for r in outs[o]], [bytes(x) for x in dg[o * nt:(o + 1) * nt]],
             None if vd is None else [int(v) for v in vd[o * nt:(o + 1) * nt]]) for o in range(count)]


def base64_encode_gated_batch_device(ins, lens, outs, gates, ngates, statuses, stream=None) -> None:
    """vds_ec_base64_encode_gated_batch_device: base64_encode_batch_device
    behind verdict bytes -- message o is written only when its ngates[o] bytes
    at the device pointer gates[o] are all zero; statuses (device, one int32 a
    message) receives 0 or ECORRUPT for every message."""
    ip = np.ascontiguousarray(np.asarray(ins, dtype=np.uint64).reshape(-1))
    ln = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64).reshape(-1))
    op = np.ascontiguousarray(np.asarray(outs, dtype=np.uint64).reshape(-1))
    gp = np.ascontiguousarray(np.asarray(gates, dtype=np.uint64).reshape(-1))
    ng = np.ascontiguousarray(np.asarray(ngates, dtype=np.uint32).reshape(-1))
    if not (ip.size == ln.size == op.size == gp.size == ng.size):
        raise VdsEcError(_lib.EINVAL, "base64_encode_gated_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_base64_encode_gated_batch_device(ln.size, ip.ctypes.data_as(_lib.vpp),
                                                             ln.ctypes.data_as(_lib.u64p),
                                                             op.ctypes.data_as(_lib.vpp),
                                                             gp.ctypes.data_as(_lib.vpp),
                                                             ng.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                             _dev_ptr(statuses), _stream_ptr(stream)),
          "base64_encode_gated_batch_device")


def download_batch_device(k: int, nodes: Sequence[Sequence[int]], chunks: Sequence[Sequence[int]],
                          chunk_sizes: Sequence[int], paddings: Sequence[int], objects: Sequence[int],
                          texts: Sequence[int], verdicts, statuses, survivor_names=None, witness_ids=None,
                          witness_names=None, witness_outs=None, stream=None) -> None:
    """vds_ec_download16_batch_device: the name check, restore_batch_device into
    the device pointers objects[o] and the gated base64 encode into the device
    pointers texts[o], on one stream.  Survivor mode: survivor_names (device,
    32 bytes a survivor), verdicts k bytes an object.  Witness mode:
    witness_ids[o], witness_names (device, 32 bytes an object) and the device
    pointers witness_outs[o], verdicts one byte an object.  statuses (device,
    one int32 an object) receives 0 or ECORRUPT."""
    count = len(nodes)
    ids = _ids([r for nd in nodes for r in nd], 2)
    cp = (C.c_void_p * max(1, count * k))(*[int(c) for ch in chunks for c in ch])
    cs = np.asarray(chunk_sizes, dtype=np.uint64)
    pd = np.asarray(paddings, dtype=np.uint16)
    ob = (C.c_void_p * max(1, count))(*[int(o) or None for o in objects])
    tp = (C.c_void_p * max(1, count))(*[int(t) or None for t in texts])
    wi = _ids(witness_ids, 2) if witness_ids is not None else None
    wo = (C.c_void_p * max(1, count))(*[int(w) for w in witness_outs]) if witness_outs is not None else None
    check(_lib.lib().vds_ec_download16_batch_device(k, count, _idp(ids, 2), cp, cs.ctypes.data_as(_lib.u64p),
                                                    pd.ctypes.data_as(_lib.u16p), _dev_ptr(survivor_names),
                                                    _idp(wi, 2) if wi is not None else None,
                                                    _dev_ptr(witness_names), wo, ob, tp, _dev_ptr(verdicts),
                                                    _dev_ptr(statuses), _stream_ptr(stream)),
          "download16_batch_device")


def download_batch(k: int, horcruxes: Sequence[Mapping[int, object]], names: Sequence[Sequence[bytes]],
                   witnesses: Sequence | None = None) -> list:
    """vds_ec_download16_host_batch: the download loop for a batch of host
    objects, checked.  horcruxes[o] maps replica id -> bytes (its first k
    entries are used, in order), names[o] their k SHA-256 names; witnesses,
    when given, holds per object (replica id, name) of one replica that is not
    among them (witness mode: 1/k of the hashing).  Returns per object
    (text or None, status, survivor verdicts): the base64 text of the restored
    object when its status is 0."""
    count = len(horcruxes)
    items = [list(h.items())[:k] for h in horcruxes]
    if any(len(it) < k for it in items) or len(names) != count or (witnesses is not None and len(witnesses) != count):
        raise VdsEcError(_lib.EINVAL, "download_batch")
    ids = _ids([r for it in items for r, _ in it], 2)
    bufs = [[_u8(v) for _, v in it] for it in items]
    if any(b.size != bs[0].size for bs in bufs for b in bs):
        raise VdsEcError(_lib.EINVAL, "download_batch")
    cs = np.asarray([bs[0].size for bs in bufs], dtype=np.uint64)
    sn = np.ascontiguousarray(np.frombuffer(b"".join(bytes(x) for row in names for x in row), dtype=np.uint8))
    if sn.size != 32 * count * k:
        raise VdsEcError(_lib.EINVAL, "download_batch: names does not hold one name per survivor")
    wi = wn = None
    if witnesses is not None:
        wi = _ids([w for w, _ in witnesses], 2)
        wn = np.ascontiguousarray(np.frombuffer(b"".join(bytes(x) for _, x in witnesses), dtype=np.uint8))
        if wn.size != 32 * count:
            raise VdsEcError(_lib.EINVAL, "download_batch: one (id, name) per object")
    caps = [(int(c) * k + 2) // 3 * 4 for c in cs]  # (E <= chunk_size * k)
    outs = [C.create_string_buffer(max(1, c)) for c in caps]
    tl = np.asarray(caps, dtype=np.uint64)
    st = np.zeros(max(1, count), dtype=np.int32)
    sv = np.zeros(max(1, count * k), dtype=np.uint8)
    failed = C.c_uint32(0)
    cp = (C.c_void_p * max(1, count * k))(*[b.ctypes.data for bs in bufs for b in bs])
    tp = (C.c_void_p * max(1, count))(*[C.addressof(o) for o in outs])
    check(_lib.lib().vds_ec_download16_host_batch(k, count, _idp(ids, 2), cp, cs.ctypes.data_as(_lib.u64p),
                                                  sn.ctypes.data if sn.size else None,
                                                  _idp(wi, 2) if wi is not None and count else None,
                                                  wn.ctypes.data if wn is not None and count else None, tp,
                                                  tl.ctypes.data_as(_lib.u64p),
                                                  st.ctypes.data_as(C.POINTER(C.c_int32)), sv.ctypes.data,
                                                  C.byref(failed)), "download16_host_batch")
    return [(None if st[o] else outs[o].raw[:int(tl[o])].decode(), int(st[o]),
             [int(v) for v in sv[o * k:(o + 1) * k]]) for o in range(count)]


def save_temp_batch_device(k: int, n: int, ins, sizes, outs, replica_digests, data_digests=None,
                           stream=None) -> None:
    """vds_ec_save_temp16_batch_device: the batched encode of replicas 0..n-1
    (arguments as encode_batch_device), then every replica's SHA-256 name at
    replica_digests + 32 (o n + i) and, unless data_digests is None, every
    body's SHA-256 at data_digests + 32 o (device buffers), all hashes in one
    launch."""
    _, ip, sz, op = _encode_batch_args(k, range(n), ins, sizes, outs)
    check(_lib.lib().vds_ec_save_temp16_batch_device(k, n, ip.size, ip.ctypes.data_as(_lib.vpp),
                                                     sz.ctypes.data_as(_lib.u64p), op.ctypes.data_as(_lib.vpp),
                                                     _dev_ptr(replica_digests), _dev_ptr(data_digests),
                                                     _stream_ptr(stream)), "save_temp16_batch_device")


def save_temp_batch(k: int, n: int, bodies: Sequence) -> list:
    """vds_ec_save_temp16_host_batch: save_temp for a batch of host bodies of
    any sizes; per body the tuple save_temp returns (replicas, their SHA-256
    names, the body's SHA-256, the replica size)."""
    bufs = [_u8(b) for b in bodies]
    count = len(bufs)
    sz = np.asarray([b.size for b in bufs], dtype=np.uint64)
    Ls = [replica_size(k, b.size) for b in bufs]
    outs = [[np.empty(max(L, 1), dtype=np.uint8) for _ in range(n)] for L in Ls]
    rd = np.empty((max(1, count * n), 32), dtype=np.uint8)
    dd = np.empty((max(1, count), 32), dtype=np.uint8)
    rs = np.zeros(max(1, count), dtype=np.uint32)
    ip = (C.c_void_p * max(1, count))(*[b.ctypes.data if b.size else None for b in bufs])
    op = (C.c_void_p * max(1, count * n))(*[o.ctypes.data for os_ in outs for o in os_])
    check(_lib.lib().vds_ec_save_temp16_host_batch(k, n, count, ip, sz.ctypes.data_as(_lib.u64p), op, rd.ctypes.data,
                                                   dd.ctypes.data, rs.ctypes.data_as(C.POINTER(C.c_uint32))),
          "save_temp16_host_batch")
    return [([r[:Ls[o]] for r in outs[o]], [bytes(x) for x in rd[o * n:(o + 1) * n]], bytes(dd[o]), int(rs[o]))
            for o in range(count)]


def encode_hash_host(k: int, replicas: Sequence[int], data, write_padding: bool = True):
    """All requested replicas of one host object plus their SHA-256 names
    (save_temp / save_data: write, then hash::signature(sha256, replica))."""
    buf = _u8(data)
    ids = _ids(replicas, 2)
    flags = 0 if write_padding else F_NO_TRAILER
    L = replica_size(k, buf.size, 2, write_padding)
    outs = [np.empty(max(L, 1), dtype=np.uint8) for _ in range(ids.size)]
    digests = np.empty((max(1, ids.size), 32), dtype=np.uint8)
    ptrs = (C.c_void_p * max(1, ids.size))(*[o.ctypes.data for o in outs])
    check(_lib.lib().vds_ec_encode16_hash_host(k, _idp(ids, 2), ids.size, buf.ctypes.data if buf.size else None,
                                               buf.size, ptrs, digests.ctypes.data, flags), "encode16_hash_host")
    return [o[:L] for o in outs], [bytes(d) for d in digests[: ids.size]]


def replica_storage_paths(digests) -> list:
    """Storage paths <b64[0:10]>/<b64[10:20]>/<b64[20:]> of replicas from their
    SHA-256 names (dht_network_client.cpp:483-505; base64 with '+' -> '#',
    '/' -> '_').  Host-only."""
    d = np.ascontiguousarray(np.frombuffer(b"".join(bytes(x) for x in digests), dtype=np.uint8))
    count = d.size // 32
    out = np.zeros(48 * max(count, 1), dtype=np.uint8)
    check(_lib.lib().vds_ec_replica_paths(d.ctypes.data if count else None, count, out.ctypes.data), "replica_paths")
    return [bytes(out[48 * i:48 * i + 46]).decode() for i in range(count)]


# ------------------------------------------------- upload path (wire formats)

def base64_decode(text) -> bytes:
    """base64::to_bytes (encoding.cpp:181-247), reference quirks included;
    raises VdsEcError with the reference's message on malformed input."""
    raw = text.encode() if isinstance(text, str) else bytes(text)
    size = _lib.lib().vds_ec_base64_decoded_size(raw, len(raw))
    out = np.empty(max(1, size), dtype=np.uint8)
    n = C.c_size_t(0)
    check(_lib.lib().vds_ec_base64_decode(raw, len(raw), out.ctypes.data, C.byref(n)), "base64_decode")
    return bytes(out[: n.value])


def base64_encode(data) -> str:
    """base64::from_bytes (encoding.cpp:138-174)."""
    buf = _u8(data)
    n = C.c_size_t(0)
    lib = _lib.lib()
    check(lib.vds_ec_base64_encode(buf.ctypes.data if buf.size else None, buf.size, None, 0, C.byref(n)))
    out = C.create_string_buffer(n.value + 1)
    check(lib.vds_ec_base64_encode(buf.ctypes.data if buf.size else None, buf.size, out, n.value + 1, C.byref(n)))
    return out.value.decode()


def tmp_names(digests) -> list:
    """save_temp's tmp-file names of replicas (dht_network_client.cpp:91-95)."""
    d = np.ascontiguousarray(np.frombuffer(b"".join(bytes(x) for x in digests), dtype=np.uint8))
    count = d.size // 32
    out = np.zeros(45 * max(count, 1), dtype=np.uint8)
    check(_lib.lib().vds_ec_tmp_names(d.ctypes.data if count else None, count, out.ctypes.data), "tmp_names")
    return [bytes(out[45 * i:45 * i + 44]).decode() for i in range(count)]


def upload_response_json(req_id: int, replica_digests, data_digest, replica_size: int) -> str:
    """The websocket answer to "upload" (websocket_api.cpp:120-121, 472-482)."""
    d = np.ascontiguousarray(np.frombuffer(b"".join(bytes(x) for x in replica_digests), dtype=np.uint8))
    n = d.size // 32
    h = np.frombuffer(bytes(data_digest), dtype=np.uint8).copy()
    ln = C.c_size_t(0)
    lib = _lib.lib()
    args = (req_id, d.ctypes.data if n else None, n, h.ctypes.data, replica_size)
    check(lib.vds_ec_upload_response_json(*args, None, 0, C.byref(ln)))
    out = C.create_string_buffer(ln.value + 1)
    check(lib.vds_ec_upload_response_json(*args, out, ln.value + 1, C.byref(ln)))
    return out.value.decode()


def save_temp(k: int, n: int, body):
    """upload_data + save_temp on the device (server_api.cpp:12-30,
    dht_network_client.cpp:62-107): replicas 0..n-1 of `body`, their SHA-256
    names, the body's SHA-256 and the replica size."""
    buf = _u8(body)
    L = replica_size(k, buf.size)
    outs = [np.empty(max(L, 1), dtype=np.uint8) for _ in range(n)]
    rd = np.empty((max(1, n), 32), dtype=np.uint8)
    dd = np.empty(32, dtype=np.uint8)
    rs = C.c_uint32(0)
    ptrs = (C.c_void_p * max(1, n))(*[o.ctypes.data for o in outs])
    check(_lib.lib().vds_ec_save_temp16_host(k, n, buf.ctypes.data if buf.size else None, buf.size, ptrs,
                                             rd.ctypes.data, dd.ctypes.data, C.byref(rs)), "save_temp16_host")
    return [o[:L] for o in outs], [bytes(x) for x in rd[:n]], bytes(dd), rs.value


def upload(req_id: int, body_b64, k: int = 32, n: int = 64):
    """The live upload end to end: websocket "upload" body (base64) ->
    replicas, tmp-file names and the JSON answer (MIN_HORCRUX = 32,
    GENERATE_HORCRUX = 64 by default, dht_network.h:22-25).  One body, its
    text decoded on the calling thread; a batch of bodies goes through
    upload_batch, which decodes the texts on the device."""
    body = base64_decode(body_b64)
    reps, names, data_hash, rsize = save_temp(k, n, body)
    return {"replicas": reps, "tmp_names": tmp_names(names), "replica_digests": names, "data_hash": data_hash,
            "json": upload_response_json(req_id, names, data_hash, rsize)}


def base64_decode_batch_device(texts, text_lens, outs, out_sizes, statuses, stream=None) -> None:
    """vds_ec_base64_decode_batch_device: len(text_lens) base64 texts of
    different lengths decoded in one launch -- text o is text_lens[o]
    characters at the device pointer texts[o], its out_sizes[o] bytes (what
    vds_ec_base64_decoded_size gives for the text) go to the device pointer
    outs[o]; statuses (device, one int32 a text) receives what base64_decode
    would return for each."""
    tp = np.ascontiguousarray(np.asarray(texts, dtype=np.uint64).reshape(-1))
    tl = np.ascontiguousarray(np.asarray(text_lens, dtype=np.uint64).reshape(-1))
    op = np.ascontiguousarray(np.asarray(outs, dtype=np.uint64).reshape(-1))
    os_ = np.ascontiguousarray(np.asarray(out_sizes, dtype=np.uint64).reshape(-1))
    if not (tp.size == tl.size == op.size == os_.size):
        raise VdsEcError(_lib.EINVAL, "base64_decode_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_base64_decode_batch_device(tl.size, tp.ctypes.data_as(_lib.vpp),
                                                       tl.ctypes.data_as(_lib.u64p), op.ctypes.data_as(_lib.vpp),
                                                       os_.ctypes.data_as(_lib.u64p), _dev_ptr(statuses),
                                                       _stream_ptr(stream)), "base64_decode_batch_device")


def base64_encode_batch_device(ins, lens, outs, stream=None) -> None:
    """vds_ec_base64_encode_batch_device: input o, lens[o] bytes at the device
    pointer ins[o], as (lens[o] + 2) // 3 * 4 characters of base64 at the
    device pointer outs[o]; the whole batch in one launch."""
    ip = np.ascontiguousarray(np.asarray(ins, dtype=np.uint64).reshape(-1))
    ln = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64).reshape(-1))
    op = np.ascontiguousarray(np.asarray(outs, dtype=np.uint64).reshape(-1))
    if not (ip.size == ln.size == op.size):
        raise VdsEcError(_lib.EINVAL, "base64_encode_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_base64_encode_batch_device(ln.size, ip.ctypes.data_as(_lib.vpp),
                                                       ln.ctypes.data_as(_lib.u64p), op.ctypes.data_as(_lib.vpp),
                                                       _stream_ptr(stream)), "base64_encode_batch_device")


def upload_batch(req_ids: Sequence[int], texts: Sequence, k: int = 32, n: int = 64, bodies: bool = False) -> list:
    """vds_ec_upload16_host_batch: the live upload for a batch of websocket
    "upload" bodies (base64 texts), decoded, encoded and named on the device.
    Per message either what upload() returns (with "body", the decoded body,
    when bodies is set) or, for a malformed text, the reference's error text."""
    raws = [t.encode() if isinstance(t, str) else bytes(t) for t in texts]
    count = len(raws)
    if len(req_ids) != count:
        raise VdsEcError(_lib.EINVAL, "upload_batch: one request id per text")
    lib = _lib.lib()
    tl = np.asarray([len(r) for r in raws], dtype=np.uint64)
    sizes = [lib.vds_ec_base64_decoded_size(r, len(r)) for r in raws]
    Ls = [replica_size(k, s) for s in sizes]
    outs = [[np.empty(max(L, 1), dtype=np.uint8) for _ in range(n)] for L in Ls]
    rd = np.empty((max(1, count * n), 32), dtype=np.uint8)
    dd = np.empty((max(1, count), 32), dtype=np.uint8)
    rs = np.zeros(max(1, count), dtype=np.uint32)
    st = np.zeros(max(1, count), dtype=np.int32)
    bs = np.zeros(max(1, count), dtype=np.uint64)
    bufs = [np.empty(max(s, 1), dtype=np.uint8) for s in sizes] if bodies else None
    failed = C.c_uint32(0)
    tp = (C.c_char_p * max(1, count))(*raws)
    op = (C.c_void_p * max(1, count * n))(*[o.ctypes.data for os_ in outs for o in os_])
    bp = (C.c_void_p * max(1, count))(*[b.ctypes.data for b in bufs]) if bodies else None
    check(lib.vds_ec_upload16_host_batch(k, n, count, C.cast(tp, _lib.vpp), tl.ctypes.data_as(_lib.u64p), op,
                                         rd.ctypes.data, dd.ctypes.data, rs.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         bp, bs.ctypes.data_as(_lib.u64p), st.ctypes.data_as(C.POINTER(C.c_int32)),
                                         C.byref(failed)), "upload16_host_batch")
    res = []
    for o in range(count):
        if st[o]:
            res.append(_lib.strerror(int(st[o])))
            continue
        names = [bytes(x) for x in rd[o * n:(o + 1) * n]]
        r = {"replicas": [x[:Ls[o]] for x in outs[o]], "tmp_names": tmp_names(names), "replica_digests": names,
             "data_hash": bytes(dd[o]), "json": upload_response_json(req_ids[o], names, bytes(dd[o]), int(rs[o]))}
        if bodies:
            r["body"] = bytes(bufs[o][:int(bs[o])])
        res.append(r)
    return res


def restore_path(k: int, nodes: Sequence[int], chunk_size: int, padding: int = 0, count: int = 1) -> int:
    """vds_ec_restore16_path: 4 = the survivor set's run-time compiled kernel,
    3 = k_restore_syn, 2 = k_restore_bs, 1 = generic only."""
    a = _ids(nodes, 2)
    return int(_lib.lib().vds_ec_restore16_path(k, _idp(a, 2), chunk_size, padding, count))


def jit_set_mode(mode: int) -> None:
    """0 = off, 1 = background compiles from a survivor set's second use
    (default), 2 = compile at the first use (vds_ec_jit_set_mode)."""
    check(_lib.lib().vds_ec_jit_set_mode(mode))


def jit_wait() -> None:
    """Block until the library's run-time compiles of survivor-set-specific
    restore kernels (vds_ec_jit_*) are done."""
    check(_lib.lib().vds_ec_jit_wait())


def jit_build(k: int, nodes: Sequence[int]) -> int:
    """Compile (no device needed) the restore kernel of survivor set `nodes`;
    returns its code object size."""
    a = _ids(nodes, 2)
    out = C.c_uint64(0)
    check(_lib.lib().vds_ec_jit_build16(k, _idp(a, 2), C.byref(out)))
    return out.value


def jit_ready(k: int, nodes: Sequence[int]) -> bool:
    a = _ids(nodes, 2)
    return bool(_lib.lib().vds_ec_jit_ready16(k, _idp(a, 2)))


def jit_dump(k: int, nodes: Sequence[int], directory: str, regen: bool = False) -> None:
    """Compile (no device needed) the kernel of survivor set `nodes` and write
    its source and code object into `directory` (vds_ec_jit_dump16)."""
    a = _ids(nodes, 2)
    check(_lib.lib().vds_ec_jit_dump16(k, _idp(a, 2), 1 if regen else 0, os.fsencode(directory)))


def fill_splitmix_device(dst, size: int, seed: int, stream=None) -> None:
    ptr = dst.data_ptr() if hasattr(dst, "data_ptr") else int(dst)
    check(_lib.lib().vds_ec_fill_splitmix_device(ptr, size, seed, _stream_ptr(stream)), "fill_splitmix")


def restore_host_batch(k: int, nodes: Sequence, chunks: Sequence[Sequence], max_devices: int = 0,
                       outs: list | None = None) -> list:
    """Multi-GPU host-memory restore of many objects (chunk_storage::restore_data
    per object, chunk_storage.cpp:62-85).  `chunks[o]` are the k replicas of
    object o, holding replica ids `nodes[o]` (or one id list for every object).
    `outs[o]` (optional) are caller-owned uint8 buffers; each must hold the
    restored object.  Returns the restored objects (trailer-trimmed, as
    restore16_host), as views of `outs` when given."""
    count = len(chunks)
    per = [list(nodes)] * count if count and np.ndim(nodes) == 1 else [list(n) for n in nodes]
    if len(per) != count or any(len(n) != k or len(c) != k for n, c in zip(per, chunks)):
        raise VdsEcError(_lib.EINVAL, "restore_host_batch: need k ids and k chunks per object")
    bufs = [[_u8(c) for c in row] for row in chunks]
    if any(c.size != row[0].size for row in bufs for c in row):  # chunk_storage.cpp:73-76
        raise VdsEcError(_lib.EINVAL, "restore_host_batch: chunks of one object differ in size")
    sizes = np.array([row[0].size for row in bufs], dtype=np.uint64)
    ids = np.ascontiguousarray(np.array(per, dtype=np.uint16).reshape(-1))
    if outs is None:
        outs = [np.empty(max(int(s) * k, 1), dtype=np.uint8) for s in sizes]
    outs = [_u8(o) for o in outs]
    if len(outs) != count:
        raise VdsEcError(_lib.EINVAL, "restore_host_batch: one output buffer per object")
    caps = np.array([o.size for o in outs], dtype=np.uint64)
    cptrs = (C.c_void_p * max(1, count * k))(*[c.ctypes.data for row in bufs for c in row])
    optrs = (C.c_void_p * max(1, count))(*[o.ctypes.data for o in outs])
    check(_lib.lib().vds_ec_restore16_host_batch(k, ids.ctypes.data_as(_lib.u16p), cptrs,
                                                 sizes.ctypes.data_as(_lib.u64p), count, optrs,
                                                 caps.ctypes.data_as(_lib.u64p), 0, max_devices),
          "restore16_host_batch")
    return [o[: int(n)] for o, n in zip(outs, caps)]


def encode_host_batch(k: int, replicas: Sequence[int], objects: Sequence, max_devices: int = 0,
                      outs: list | None = None) -> list:
    """Multi-GPU host-memory encode (one thread + pinned ring per device).
    `outs[o][i]` (optional) are caller-owned uint8 buffers of at least
    replica_size(k, len(objects[o])) bytes that receive replica i of object o."""
    ids = _ids(replicas, 2)
    bufs = [_u8(o) for o in objects]
    sizes = np.array([b.size for b in bufs], dtype=np.uint64)
    if outs is None:
        outs = [[np.empty(max(replica_size(k, b.size), 1), dtype=np.uint8) for _ in range(ids.size)] for b in bufs]
    for row, b in zip(outs, bufs):
        if len(row) != ids.size or any(_u8(o).size < replica_size(k, b.size) for o in row):
            raise VdsEcError(_lib.EINVAL, "encode_host_batch: output buffer too small")
    optrs = (C.c_void_p * (len(bufs) * ids.size))(*[o.ctypes.data for row in outs for o in row])
    iptrs = (C.c_void_p * max(1, len(bufs)))(*[b.ctypes.data for b in bufs])
    check(_lib.lib().vds_ec_encode16_host_batch(k, _idp(ids, 2), ids.size, iptrs,
                                                sizes.ctypes.data_as(_lib.u64p), len(bufs), optrs, 0,
                                                max_devices), "encode16_host_batch")
    return [[o[: replica_size(k, b.size)] for o in row] for row, b in zip(outs, bufs)]


class PinnedBuffer:
    """Caller-owned pinned host memory (vds_ec_host_alloc): page-locked,
    device-mapped.  Host batches whose objects, replicas, survivors or outputs
    lie back to back in such a buffer read and write it directly (no staging
    copies).  `.array` is a uint8 numpy view; close() (or del) frees it."""

    def __init__(self, nbytes: int):
        p = C.c_void_p()
        check(_lib.lib().vds_ec_host_alloc(int(nbytes), C.byref(p)), "host_alloc")
        self.ptr, self.nbytes = p.value, int(nbytes)
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self.ptr))

    def close(self) -> None:
        if self.ptr:
            self.array = None
            check(_lib.lib().vds_ec_host_free(self.ptr), "host_free")
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter teardown)
            pass


def host_register(arr) -> None:
    """Pin (and map) a caller's contiguous numpy buffer for the host batches
    (vds_ec_host_register); host_unregister before it is freed."""
    a = _u8(arr)
    check(_lib.lib().vds_ec_host_register(a.ctypes.data, a.size), "host_register")


def host_unregister(arr) -> None:
    check(_lib.lib().vds_ec_host_unregister(_u8(arr).ctypes.data), "host_unregister")


# ------------------------------------------------------- node-to-node transport
def hmac_sha256_host(key, data) -> bytes:
    """vds_ec_hmac_sha256_host: HMAC-SHA256 of one host message on the calling
    thread (hmac::signature, kernel/vds_crypto/hash.cpp:218-260)."""
    k, d = _u8(key), _u8(data)
    out = np.empty(32, dtype=np.uint8)
    check(_lib.lib().vds_ec_hmac_sha256_host(k.ctypes.data if k.size else None, k.size,
                                             d.ctypes.data if d.size else None, d.size, out.ctypes.data),
          "hmac_sha256_host")
    return out.tobytes()


def dgram_layout(mtu: int, route_len: int, msg_len: int) -> tuple:
    """vds_ec_dgram_layout: (datagram count, message bytes in the first, length
    of the last) as prepare_to_send cuts a message
    (dht_datagram_protocol.cpp:335-541)."""
    n, c0, last = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    check(_lib.lib().vds_ec_dgram_layout(mtu, route_len, msg_len, C.byref(n), C.byref(c0), C.byref(last)),
          "dgram_layout")
    return n.value, c0.value, last.value


def write_number(value: int) -> bytes:
    """vds_ec_write_number: binary_serializer::write_number
    (binary_serialize.cpp:44-66)."""
    out = np.empty(9, dtype=np.uint8)
    n = C.c_uint32(0)
    check(_lib.lib().vds_ec_write_number(value, out.ctypes.data, C.byref(n)), "write_number")
    return out[:n.value].tobytes()


def _u32(values) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(values, dtype=np.uint32).reshape(-1))


def _keys(keys) -> np.ndarray:
    """Session keys (a sequence of 32-byte keys, or their bytes back to back)."""
    if isinstance(keys, (bytes, bytearray, memoryview, np.ndarray)):
        return _u8(keys)
    return _u8(b"".join(bytes(k) for k in keys))


def hmac_sha256_batch_device(msgs, lens, session_of, keys, macs, expected=None, verdicts=None, stream=None) -> None:
    """vds_ec_hmac_sha256_batch_device: HMAC-SHA256 of len(lens) device
    messages in one launch -- message j is lens[j] bytes at the device pointer
    msgs[j], under key session_of[j] of keys (host, 32 bytes each); MAC j goes
    to macs + 32 j (device; None with expected: check only) and, with expected,
    is compared into verdicts[j] (device; 0 equal, 1 different)."""
    mp = np.ascontiguousarray(np.asarray(msgs, dtype=np.uint64).reshape(-1))
    ln = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64).reshape(-1))
    so, ks = _u32(session_of), _keys(keys)
    if not (mp.size == ln.size == so.size) or ks.size % 32:
        raise VdsEcError(_lib.EINVAL, "hmac_sha256_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_hmac_sha256_batch_device(ln.size, mp.ctypes.data_as(_lib.vpp),
                                                     ln.ctypes.data_as(_lib.u64p), so.ctypes.data_as(_lib.u32p),
                                                     ks.ctypes.data if ks.size else None, ks.size // 32,
                                                     _dev_ptr(macs), _dev_ptr(expected), _dev_ptr(verdicts),
                                                     _stream_ptr(stream)), "hmac_sha256_batch_device")


def dgram_seal_batch_device(msgs, msg_lens, types, index0, routes, route_lens, session_of, keys, mtus, outs,
                            pitch: int, stream=None) -> None:
    """vds_ec_dgram_seal_batch_device: message o (msg_lens[o] bytes at the
    device pointer msgs[o]) cut into datagrams, each with its header and
    HMAC-SHA256 under key session_of[o]; datagram d of message o lands at the
    device pointer outs[o] + d * pitch, as long as dgram_layout says.  routes[o]
    is the device pointer of its route blob (route_lens[o] bytes)."""
    mp = np.ascontiguousarray(np.asarray(msgs, dtype=np.uint64).reshape(-1))
    ln = np.ascontiguousarray(np.asarray(msg_lens, dtype=np.uint64).reshape(-1))
    ty = np.ascontiguousarray(np.asarray(types, dtype=np.uint8).reshape(-1))
    i0, rl, so, mt = _u32(index0), _u32(route_lens), _u32(session_of), _u32(mtus)
    rp = np.ascontiguousarray(np.asarray(routes, dtype=np.uint64).reshape(-1))
    op = np.ascontiguousarray(np.asarray(outs, dtype=np.uint64).reshape(-1))
    ks = _keys(keys)
    if not (mp.size == ln.size == ty.size == i0.size == rl.size == so.size == mt.size == rp.size == op.size) \
            or ks.size % 32:
        raise VdsEcError(_lib.EINVAL, "dgram_seal_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_dgram_seal_batch_device(ln.size, mp.ctypes.data_as(_lib.vpp), ln.ctypes.data_as(_lib.u64p),
                                                    ty.ctypes.data, i0.ctypes.data_as(_lib.u32p),
                                                    rp.ctypes.data_as(_lib.vpp), rl.ctypes.data_as(_lib.u32p),
                                                    so.ctypes.data_as(_lib.u32p), ks.ctypes.data if ks.size else None,
                                                    mt.ctypes.data_as(_lib.u32p), ks.size // 32,
                                                    op.ctypes.data_as(_lib.vpp), pitch, _stream_ptr(stream)),
          "dgram_seal_batch_device")


def dgram_open_batch_device(dgrams, lens, hdr_lens, session_of, keys, dsts, verdicts, stream=None) -> None:
    """vds_ec_dgram_open_batch_device: datagram j (lens[j] bytes at the device
    pointer dgrams[j]) verified under key session_of[j]; verdicts[j] (device) =
    0 verified, 1 invalid signature, 2 shorter than 33 bytes; bytes
    [hdr_lens[j], lens[j] - 32) copied to the device pointer dsts[j] (0: nowhere;
    dsts None: verify only) only when the datagram verified."""
    dp = np.ascontiguousarray(np.asarray(dgrams, dtype=np.uint64).reshape(-1))
    ln, hl, so, ks = _u32(lens), _u32(hdr_lens), _u32(session_of), _keys(keys)
    tp = None if dsts is None else np.ascontiguousarray(np.asarray(dsts, dtype=np.uint64).reshape(-1))
    if not (dp.size == ln.size == hl.size == so.size) or (tp is not None and tp.size != dp.size) or ks.size % 32:
        raise VdsEcError(_lib.EINVAL, "dgram_open_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_dgram_open_batch_device(ln.size, dp.ctypes.data_as(_lib.vpp), ln.ctypes.data_as(_lib.u32p),
                                                    hl.ctypes.data_as(_lib.u32p), so.ctypes.data_as(_lib.u32p),
                                                    ks.ctypes.data if ks.size else None, ks.size // 32,
                                                    None if tp is None else tp.ctypes.data_as(_lib.vpp),
                                                    _dev_ptr(verdicts), _stream_ptr(stream)),
          "dgram_open_batch_device")


def dgram_seal_batch(msgs: Sequence, types: Sequence[int], index0: Sequence[int], routes: Sequence,
                     session_of: Sequence[int], keys, mtus: Sequence[int]) -> list:
    """vds_ec_dgram_seal_host_batch: host messages (bytes) with their route
    blobs (bytes, b"" = direct) sealed on the device.  Returns per message the
    list of its datagrams (bytes)."""
    count = len(msgs)
    mb = [_u8(m) for m in msgs]
    rb = [_u8(r) for r in routes]
    ln = np.asarray([m.size for m in mb], dtype=np.uint64)
    rl = _u32([r.size for r in rb])
    ty = np.ascontiguousarray(np.asarray(types, dtype=np.uint8).reshape(-1))
    i0, so, mt, ks = _u32(index0), _u32(session_of), _u32(mtus), _keys(keys)
    if not (count == ty.size == i0.size == rl.size == so.size == mt.size) or ks.size % 32:
        raise VdsEcError(_lib.EINVAL, "dgram_seal_batch: the arrays do not describe one batch")
    need = 0
    for o in range(count):
        n, _, last = dgram_layout(int(mt[o]), int(rl[o]), int(ln[o]))
        need += (n - 1) * int(mt[o]) + last
    slab = np.empty(max(1, need), dtype=np.uint8)
    offs = np.zeros(max(1, count), dtype=np.uint64)
    cnts = np.zeros(max(1, count), dtype=np.uint32)
    lasts = np.zeros(max(1, count), dtype=np.uint32)
    mp = (C.c_void_p * max(1, count))(*[m.ctypes.data if m.size else None for m in mb])
    rp = (C.c_void_p * max(1, count))(*[r.ctypes.data if r.size else None for r in rb])
    check(_lib.lib().vds_ec_dgram_seal_host_batch(count, mp, ln.ctypes.data_as(_lib.u64p), ty.ctypes.data,
                                                  i0.ctypes.data_as(_lib.u32p), rp, rl.ctypes.data_as(_lib.u32p),
                                                  so.ctypes.data_as(_lib.u32p), ks.ctypes.data if ks.size else None,
                                                  mt.ctypes.data_as(_lib.u32p), ks.size // 32, slab.ctypes.data, need,
                                                  offs.ctypes.data_as(_lib.u64p), cnts.ctypes.data_as(_lib.u32p),
                                                  lasts.ctypes.data_as(_lib.u32p)), "dgram_seal_host_batch")
    out = []
    for o in range(count):
        at, m = int(offs[o]), int(mt[o])
        ds = [slab[at + d * m:at + (d + 1) * m].tobytes() for d in range(int(cnts[o]) - 1)]
        at += (int(cnts[o]) - 1) * m
        ds.append(slab[at:at + int(lasts[o])].tobytes())
        out.append(ds)
    return out


def dgram_open_batch(dgrams: Sequence, session_of: Sequence[int], keys) -> tuple:
    """vds_ec_dgram_open_host_batch: the datagrams of a drained socket batch
    (bytes, arrival order) with their sessions.  Returns (verdicts, messages):
    verdicts[j] = 0 verified, 1 invalid signature, 2 shorter than 33 bytes, 3
    service datagram skipped; messages = a list of dicts (session, index0,
    dgrams, type, status, route, message) ordered by (session, index0), route
    and message None unless status is 0."""
    count = len(dgrams)
    db = [_u8(d) for d in dgrams]
    ln, so, ks = _u32([d.size for d in db]), _u32(session_of), _keys(keys)
    if count != so.size or ks.size % 32:
        raise VdsEcError(_lib.EINVAL, "dgram_open_batch: the arrays do not describe one batch")
    cap = int(ln.sum()) if count else 0
    slab = np.empty(max(1, cap), dtype=np.uint8)
    vd = np.zeros(max(1, count), dtype=np.uint8)
    msgs = (_lib.DgramMessage * max(1, count))()
    nm = C.c_uint32(0)
    dp = (C.c_void_p * max(1, count))(*[d.ctypes.data if d.size else None for d in db])
    check(_lib.lib().vds_ec_dgram_open_host_batch(count, dp, ln.ctypes.data_as(_lib.u32p),
                                                  so.ctypes.data_as(_lib.u32p), ks.ctypes.data if ks.size else None,
                                                  ks.size // 32, vd.ctypes.data, slab.ctypes.data, cap, msgs,
                                                  C.byref(nm)), "dgram_open_host_batch")
    out = []
    for i in range(nm.value):
        m = msgs[i]
        ok = m.status == 0
        out.append({"session": m.session, "index0": m.index0, "dgrams": m.dgrams, "type": m.type,
                    "status": m.status,
                    "route": slab[m.route_off:m.route_off + m.route_len].tobytes() if ok else None,
                    "message": slab[m.msg_off:m.msg_off + m.msg_len].tobytes() if ok else None})
    return [int(v) for v in vd[:count]], out


# ------------------------------------------------------------ websocket frames
def ws_frame_parse(buf) -> tuple:
    """vds_ec_ws_frame_parse: (status, frame) of the frame header at the start
    of buf; status OK (text, binary, ping), EWS_FRAME (another opcode) or
    EWS_SHORT (frame["need"] bytes are needed).  frame holds fin, rsv1-3,
    opcode, masked, mask (bytes), header_len, need, payload_len."""
    b = bytes(buf)
    f = _lib.WsFrame()
    rc = _lib.lib().vds_ec_ws_frame_parse(b, len(b), C.byref(f))
    if rc == _lib.EINVAL:
        raise VdsEcError(rc, "ws_frame_parse")
    d = {name: getattr(f, name) for name, _ in _lib.WsFrame._fields_ if name != "mask"}
    d["mask"] = bytes(f.mask)
    return rc, d


def ws_frame_header(payload_len: int, binary: bool = False) -> bytes:
    """vds_ec_ws_frame_header: the 2, 4 or 10 header bytes of an unmasked frame."""
    out = (C.c_uint8 * 10)()
    n = C.c_uint32(0)
    check(_lib.lib().vds_ec_ws_frame_header(payload_len, int(binary), out, C.byref(n)), "ws_frame_header")
    return bytes(out[:n.value])


def ws_upload_request(payload, mask: bytes | None = None) -> tuple:
    """vds_ec_ws_upload_request: (status, id, body_off, body_len, decoded_size)
    of a payload still under `mask` (None: not masked); status OK or EWS_FORM."""
    b = bytes(payload)
    rid, off, ln, size = C.c_int32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    mk = bytes(mask) if mask is not None else None
    rc = _lib.lib().vds_ec_ws_upload_request(b, len(b), mk, C.byref(rid), C.byref(off), C.byref(ln), C.byref(size))
    if rc == _lib.EINVAL:
        raise VdsEcError(rc, "ws_upload_request")
    return rc, rid.value, off.value, ln.value, size.value


def ws_upload_answer_size(req_id: int, n: int, replica_size_: int) -> tuple:
    """vds_ec_ws_upload_answer_size: (frame_len, header_len)."""
    fl, hl = C.c_uint64(0), C.c_uint32(0)
    check(_lib.lib().vds_ec_ws_upload_answer_size(req_id, n, replica_size_, C.byref(fl), C.byref(hl)))
    return fl.value, hl.value


def ws_download_answer_layout(req_id: int, object_size: int) -> tuple:
    """vds_ec_ws_download_answer_layout: (frame_len, header_len, text_off)."""
    fl, hl, to = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    check(_lib.lib().vds_ec_ws_download_answer_layout(req_id, object_size, C.byref(fl), C.byref(hl), C.byref(to)))
    return fl.value, hl.value, to.value


def ws_error_answer(req_id: int, status: int) -> bytes:
    """vds_ec_ws_error_answer: the frame {"id":"..","error":".."} behind its header."""
    ln = C.c_size_t(0)
    check(_lib.lib().vds_ec_ws_error_answer(req_id, status, None, 0, C.byref(ln)))
    out = C.create_string_buffer(max(1, ln.value))
    check(_lib.lib().vds_ec_ws_error_answer(req_id, status, out, ln.value, C.byref(ln)))
    return out.raw[:ln.value]


def base64_decode_masked_batch_device(texts, text_lens, masks, outs, out_sizes, statuses, stream=None) -> None:
    """vds_ec_base64_decode_masked_batch_device: base64_decode_batch_device for
    texts still under their websocket masks -- masks holds 4 bytes a text, and
    character j of text o is texts[o][j] ^ masks[o][j & 3]."""
    tp = np.ascontiguousarray(np.asarray(texts, dtype=np.uint64).reshape(-1))
    tl = np.ascontiguousarray(np.asarray(text_lens, dtype=np.uint64).reshape(-1))
    op = np.ascontiguousarray(np.asarray(outs, dtype=np.uint64).reshape(-1))
    os_ = np.ascontiguousarray(np.asarray(out_sizes, dtype=np.uint64).reshape(-1))
    if isinstance(masks, (bytes, bytearray)):
        masks = np.frombuffer(bytes(masks), dtype=np.uint8)
    mk = np.ascontiguousarray(np.asarray(masks, dtype=np.uint8).reshape(-1))
    if not (tp.size == tl.size == op.size == os_.size and mk.size == 4 * tl.size):
        raise VdsEcError(_lib.EINVAL, "base64_decode_masked_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_base64_decode_masked_batch_device(
        tl.size, tp.ctypes.data_as(_lib.vpp), tl.ctypes.data_as(_lib.u64p), mk.ctypes.data,
        op.ctypes.data_as(_lib.vpp), os_.ctypes.data_as(_lib.u64p), _dev_ptr(statuses), _stream_ptr(stream)),
        "base64_decode_masked_batch_device")


def ws_upload_answer_batch_device(req_ids, n: int, replica_digests, data_digests, replica_sizes, outs,
                                  stream=None) -> None:
    """vds_ec_ws_upload_answer_batch_device: the "upload" answers of
    len(req_ids) messages as websocket frames at the device pointers outs[o],
    from the names (device, 32 n bytes a message) and body hashes (device, 32
    bytes a message) save_temp_batch_device left."""
    ids = np.ascontiguousarray(np.asarray(req_ids, dtype=np.int32).reshape(-1))
    rs = np.ascontiguousarray(np.asarray(replica_sizes, dtype=np.uint32).reshape(-1))
    op = np.ascontiguousarray(np.asarray(outs, dtype=np.uint64).reshape(-1))
    if not (ids.size == rs.size == op.size):
        raise VdsEcError(_lib.EINVAL, "ws_upload_answer_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_ws_upload_answer_batch_device(
        ids.size, ids.ctypes.data_as(_lib.i32p), n, _dev_ptr(replica_digests), _dev_ptr(data_digests),
        rs.ctypes.data_as(_lib.u32p), op.ctypes.data_as(_lib.vpp), _stream_ptr(stream)),
        "ws_upload_answer_batch_device")


def ws_upload_batch(frames: Sequence, k: int = 32, n: int = 64) -> list:
    """vds_ec_ws_upload16_host_batch: the live upload for a batch of websocket
    FRAMES, unmasked, decoded, encoded, named and answered on the device.  Per
    frame a dict with "status" and "answer" (the answer frame's bytes, or None
    for a frame that got no device work: EWS_SHORT, EWS_FRAME, EWS_PING,
    EWS_FORM) and, with status 0, what upload_batch returns but "json"."""
    raws = [bytes(f) for f in frames]
    count = len(raws)
    lib = _lib.lib()
    # room for every replica: a body is shorter than 3/4 of its frame
    Ls = [replica_size(k, len(r) // 4 * 3) for r in raws]
    outs = [[np.empty(max(L, 1), dtype=np.uint8) for _ in range(n)] for L in Ls]
    cap = sum(ws_upload_answer_size(-1, n, 0xFFFFFFFF)[0] for _ in raws)
    ans = np.zeros(max(1, cap), dtype=np.uint8)
    rd = np.empty((max(1, count * n), 32), dtype=np.uint8)
    dd = np.empty((max(1, count), 32), dtype=np.uint8)
    rs = np.zeros(max(1, count), dtype=np.uint32)
    st = np.zeros(max(1, count), dtype=np.int32)
    ao = np.zeros(max(1, count), dtype=np.uint64)
    al = np.zeros(max(1, count), dtype=np.uint64)
    fl = np.asarray([len(r) for r in raws] or [0], dtype=np.uint64)
    failed = C.c_uint32(0)
    fp = (C.c_char_p * max(1, count))(*raws)
    op = (C.c_void_p * max(1, count * n))(*[o.ctypes.data for os_ in outs for o in os_])
    check(lib.vds_ec_ws_upload16_host_batch(k, n, count, C.cast(fp, _lib.vpp), fl.ctypes.data_as(_lib.u64p), op,
                                            rd.ctypes.data, dd.ctypes.data, rs.ctypes.data_as(_lib.u32p),
                                            ans.ctypes.data, ans.size, ao.ctypes.data_as(_lib.u64p),
                                            al.ctypes.data_as(_lib.u64p), st.ctypes.data_as(_lib.i32p),
                                            C.byref(failed)), "ws_upload16_host_batch")
    res = []
    for o in range(count):
        r = {"status": int(st[o]), "answer": bytes(ans[int(ao[o]):int(ao[o] + al[o])]) if al[o] else None}
        if not st[o]:
            names = [bytes(x) for x in rd[o * n:(o + 1) * n]]
            r.update({"replicas": [x[:int(rs[o])] for x in outs[o]], "tmp_names": tmp_names(names),
                      "replica_digests": names, "data_hash": bytes(dd[o]), "replica_size": int(rs[o])})
        res.append(r)
    return res


def ws_download_batch(k: int, req_ids: Sequence[int], horcruxes: Sequence[Mapping[int, object]],
                      names: Sequence[Sequence[bytes]], witnesses: Sequence | None = None) -> list:
    """vds_ec_ws_download16_host_batch: download_batch answering in websocket
    frames.  Returns per object (frame bytes, status, survivor verdicts): the
    answer frame {"id":"N","result":"<base64>"} when the status is 0, else the
    error frame."""
    count = len(horcruxes)
    items = [list(h.items())[:k] for h in horcruxes]
    if any(len(it) < k for it in items) or len(names) != count or len(req_ids) != count or \
            (witnesses is not None and len(witnesses) != count):
        raise VdsEcError(_lib.EINVAL, "ws_download_batch")
    ids = _ids([r for it in items for r, _ in it], 2)
    bufs = [[_u8(v) for _, v in it] for it in items]
    if any(b.size != bs[0].size for bs in bufs for b in bs):
        raise VdsEcError(_lib.EINVAL, "ws_download_batch")
    cs = np.asarray([bs[0].size for bs in bufs] or [0], dtype=np.uint64)
    sn = np.ascontiguousarray(np.frombuffer(b"".join(bytes(x) for row in names for x in row), dtype=np.uint8))
    if sn.size != 32 * count * k:
        raise VdsEcError(_lib.EINVAL, "ws_download_batch: names does not hold one name per survivor")
    wi = wn = None
    if witnesses is not None:
        wi = _ids([w for w, _ in witnesses], 2)
        wn = np.ascontiguousarray(np.frombuffer(b"".join(bytes(x) for _, x in witnesses), dtype=np.uint8))
        if wn.size != 32 * count:
            raise VdsEcError(_lib.EINVAL, "ws_download_batch: one (id, name) per object")
    rid = np.asarray(list(req_ids) or [0], dtype=np.int32)
    # (E <= chunk_size * k; an error answer is shorter than 128 bytes)
    cap = sum(max(ws_download_answer_layout(int(rid[o]), int(cs[o]) * k)[0], 128) for o in range(count))
    slab = np.zeros(max(1, cap), dtype=np.uint8)
    fo = np.zeros(max(1, count), dtype=np.uint64)
    fl = np.zeros(max(1, count), dtype=np.uint64)
    st = np.zeros(max(1, count), dtype=np.int32)
    sv = np.zeros(max(1, count * k), dtype=np.uint8)
    failed = C.c_uint32(0)
    cp = (C.c_void_p * max(1, count * k))(*[b.ctypes.data for bs in bufs for b in bs])
    check(_lib.lib().vds_ec_ws_download16_host_batch(
        k, count, rid.ctypes.data_as(_lib.i32p), _idp(ids, 2), cp, cs.ctypes.data_as(_lib.u64p),
        sn.ctypes.data if sn.size else None, _idp(wi, 2) if wi is not None and count else None,
        wn.ctypes.data if wn is not None and count else None, slab.ctypes.data, slab.size,
        fo.ctypes.data_as(_lib.u64p), fl.ctypes.data_as(_lib.u64p), st.ctypes.data_as(_lib.i32p), sv.ctypes.data,
        C.byref(failed)), "ws_download16_host_batch")
    return [(bytes(slab[int(fo[o]):int(fo[o] + fl[o])]), int(st[o]), [int(v) for v in sv[o * k:(o + 1) * k]])
            for o in range(count)]


# ------------------------------------------------------------- file blocks
def aes256_cbc_padded_size(length: int) -> int:
    """vds_ec_aes256_cbc_padded_size: what `length` bytes encrypt to under PKCS#7."""
    return int(_lib.lib().vds_ec_aes256_cbc_padded_size(length))


def block_iv() -> bytes:
    """vds_ec_block_iv: pack_block_iv (dht_network_client.cpp:1101-1105)."""
    iv = np.zeros(16, dtype=np.uint8)
    check(_lib.lib().vds_ec_block_iv(iv.ctypes.data), "block_iv")
    return iv.tobytes()


def aes256_cbc_encrypt_host(key, data, iv=None) -> bytes:
    """vds_ec_aes256_cbc_encrypt_host: one message on the calling thread
    (symmetric_encrypt::encrypt; iv None: pack_block_iv)."""
    k, d, v = _u8(key), _u8(data), _u8(block_iv() if iv is None else iv)
    if k.size != 32 or v.size != 16:
        raise VdsEcError(_lib.EINVAL, "aes256_cbc_encrypt_host: a key of 32 bytes and an iv of 16")
    out = np.empty(aes256_cbc_padded_size(d.size), dtype=np.uint8)
    check(_lib.lib().vds_ec_aes256_cbc_encrypt_host(k.ctypes.data, v.ctypes.data, d.ctypes.data if d.size else None,
                                                    d.size, out.ctypes.data), "aes256_cbc_encrypt_host")
    return out.tobytes()


def aes256_cbc_decrypt_host(key, data, iv=None) -> bytes:
    """vds_ec_aes256_cbc_decrypt_host: one message on the calling thread
    (symmetric_decrypt::decrypt); raises VdsEcError with VDS_EC_ECRYPT_LENGTH
    or VDS_EC_ECRYPT_PADDING where the reference's EVP_CipherFinal_ex fails."""
    k, d, v = _u8(key), _u8(data), _u8(block_iv() if iv is None else iv)
    if k.size != 32 or v.size != 16:
        raise VdsEcError(_lib.EINVAL, "aes256_cbc_decrypt_host: a key of 32 bytes and an iv of 16")
    out = np.empty(max(1, d.size), dtype=np.uint8)
    n = C.c_uint64(0)
    check(_lib.lib().vds_ec_aes256_cbc_decrypt_host(k.ctypes.data, v.ctypes.data, d.ctypes.data if d.size else None,
                                                    d.size, out.ctypes.data, C.byref(n)), "aes256_cbc_decrypt_host")
    return out[:n.value].tobytes()


def _ptr_table(values) -> np.ndarray:
    return np.ascontiguousarray(np.asarray([_dev_ptr(v) or 0 for v in values], dtype=np.uint64).reshape(-1))


def aes256_cbc_encrypt_batch_device(ins, lens, keys, outs, ivs=None, stream=None) -> None:
    """vds_ec_aes256_cbc_encrypt_batch_device: message o, lens[o] bytes at the
    device pointer ins[o], encrypted under the 32 bytes at keys + 32 o (device)
    and the 16 at ivs + 16 o (device; None: pack_block_iv) into
    aes256_cbc_padded_size(lens[o]) bytes at the device pointer outs[o]; the
    whole batch in one launch."""
    ip, op = _ptr_table(ins), _ptr_table(outs)
    ln = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64).reshape(-1))
    if not (ip.size == ln.size == op.size):
        raise VdsEcError(_lib.EINVAL, "aes256_cbc_encrypt_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_aes256_cbc_encrypt_batch_device(
        ln.size, ip.ctypes.data_as(_lib.vpp), ln.ctypes.data_as(_lib.u64p), _dev_ptr(keys), _dev_ptr(ivs),
        op.ctypes.data_as(_lib.vpp), _stream_ptr(stream)), "aes256_cbc_encrypt_batch_device")


def aes256_cbc_decrypt_batch_device(ins, lens, keys, outs, out_lens, statuses, ivs=None, stream=None) -> None:
    """vds_ec_aes256_cbc_decrypt_batch_device: the mirror; out_lens (uint32)
    and statuses (int32) are device buffers of one entry a message, all written
    by the launch."""
    ip, op = _ptr_table(ins), _ptr_table(outs)
    ln = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64).reshape(-1))
    if not (ip.size == ln.size == op.size):
        raise VdsEcError(_lib.EINVAL, "aes256_cbc_decrypt_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_aes256_cbc_decrypt_batch_device(
        ln.size, ip.ctypes.data_as(_lib.vpp), ln.ctypes.data_as(_lib.u64p), _dev_ptr(keys), _dev_ptr(ivs),
        op.ctypes.data_as(_lib.vpp), _dev_ptr(out_lens), _dev_ptr(statuses), _stream_ptr(stream)),
        "aes256_cbc_decrypt_batch_device")


def block_pack_batch_device(datas, data_lens, zipped, zipped_lens, ids, keys, crypted, stream=None) -> None:
    """vds_ec_block_pack_batch_device: client::save for a batch of blocks on
    device pointers -- ids + 32 o = SHA-256(data o), keys + 32 o =
    SHA-256(AES(id, data)), crypted[o] = AES(key, zipped o), four launches."""
    dp, zp, cp = _ptr_table(datas), _ptr_table(zipped), _ptr_table(crypted)
    dl = np.ascontiguousarray(np.asarray(data_lens, dtype=np.uint64).reshape(-1))
    zl = np.ascontiguousarray(np.asarray(zipped_lens, dtype=np.uint64).reshape(-1))
    if not (dp.size == dl.size == zp.size == zl.size == cp.size):
        raise VdsEcError(_lib.EINVAL, "block_pack_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_block_pack_batch_device(
        dl.size, dp.ctypes.data_as(_lib.vpp), dl.ctypes.data_as(_lib.u64p), zp.ctypes.data_as(_lib.vpp),
        zl.ctypes.data_as(_lib.u64p), _dev_ptr(ids), _dev_ptr(keys), cp.ctypes.data_as(_lib.vpp),
        _stream_ptr(stream)), "block_pack_batch_device")


def block_pack_host_batch(datas: Sequence, zipped: Sequence) -> list:
    """vds_ec_block_pack_host_batch: one (id, key, crypted) per block from the
    blocks and their deflated forms (host bytes)."""
    ds, zs = [_u8(d) for d in datas], [_u8(z) for z in zipped]
    count = len(ds)
    if len(zs) != count:
        raise VdsEcError(_lib.EINVAL, "block_pack_host_batch: one deflated form per block")
    dl = np.asarray([d.size for d in ds] or [0], dtype=np.uint64)
    zl = np.asarray([z.size for z in zs] or [0], dtype=np.uint64)
    outs = [np.empty(aes256_cbc_padded_size(z.size), dtype=np.uint8) for z in zs]
    ids = np.empty((max(1, count), 32), dtype=np.uint8)
    keys = np.empty((max(1, count), 32), dtype=np.uint8)
    cs = np.zeros(max(1, count), dtype=np.uint64)
    dp = (C.c_void_p * max(1, count))(*[d.ctypes.data if d.size else None for d in ds])
    zp = (C.c_void_p * max(1, count))(*[z.ctypes.data if z.size else None for z in zs])
    cp = (C.c_void_p * max(1, count))(*[o.ctypes.data for o in outs])
    check(_lib.lib().vds_ec_block_pack_host_batch(count, dp, dl.ctypes.data_as(_lib.u64p), zp,
                                                  zl.ctypes.data_as(_lib.u64p), ids.ctypes.data, keys.ctypes.data, cp,
                                                  cs.ctypes.data_as(_lib.u64p)), "block_pack_host_batch")
    return [(bytes(ids[o]), bytes(keys[o]), outs[o][:int(cs[o])].tobytes()) for o in range(count)]


def aes256_cbc_decrypt_host_batch(ins: Sequence, keys: Sequence, ivs: Sequence | None = None) -> list:
    """vds_ec_aes256_cbc_decrypt_host_batch: per message (plaintext or None,
    status) -- host ciphertexts decrypted on the device in one call."""
    cts = [_u8(c) for c in ins]
    count = len(cts)
    if len(keys) != count or (ivs is not None and len(ivs) != count):
        raise VdsEcError(_lib.EINVAL, "aes256_cbc_decrypt_host_batch: one key (and iv) per message")
    kk = np.ascontiguousarray(np.frombuffer(b"".join(bytes(k) for k in keys), dtype=np.uint8))
    vv = None if ivs is None else np.ascontiguousarray(np.frombuffer(b"".join(bytes(v) for v in ivs), dtype=np.uint8))
    if kk.size != 32 * count or (vv is not None and vv.size != 16 * count):
        raise VdsEcError(_lib.EINVAL, "aes256_cbc_decrypt_host_batch: keys of 32 bytes, ivs of 16")
    ln = np.asarray([c.size for c in cts] or [0], dtype=np.uint64)
    outs = [np.empty(max(1, c.size), dtype=np.uint8) for c in cts]
    ol = np.zeros(max(1, count), dtype=np.uint64)
    st = np.zeros(max(1, count), dtype=np.int32)
    failed = C.c_uint32(0)
    ip = (C.c_void_p * max(1, count))(*[c.ctypes.data if c.size else None for c in cts])
    op = (C.c_void_p * max(1, count))(*[o.ctypes.data for o in outs])
    check(_lib.lib().vds_ec_aes256_cbc_decrypt_host_batch(
        count, ip, ln.ctypes.data_as(_lib.u64p), kk.ctypes.data if count else None,
        vv.ctypes.data if vv is not None and count else None, op, ol.ctypes.data_as(_lib.u64p),
        st.ctypes.data_as(_lib.i32p), C.byref(failed)), "aes256_cbc_decrypt_host_batch")
    return [(None if st[o] else outs[o][:int(ol[o])].tobytes(), int(st[o])) for o in range(count)]


def inflate_host(data, cap: int) -> tuple:
    """vds_ec_inflate_host: one zlib stream on the calling thread, no GPU and
    no zlib -> (status, bytes): the plaintext under VDS_EC_OK, what the input
    held under VDS_EC_EINFLATE_SHORT, nothing under VDS_EC_EINFLATE_DATA and
    VDS_EC_EINFLATE_SPACE (`cap`: the output's capacity)."""
    d = _u8(data)
    out = np.empty(max(1, cap), dtype=np.uint8)
    n = C.c_uint64(0)
    st = _lib.lib().vds_ec_inflate_host(d.ctypes.data if d.size else None, d.size, out.ctypes.data if cap else None,
                                        cap, C.byref(n))
    if st not in (_lib.OK, _lib.EINFLATE_DATA, _lib.EINFLATE_SHORT, _lib.EINFLATE_SPACE):
        check(st, "inflate_host")
    return int(st), out[:n.value].tobytes()


def inflate_batch_device(ins, lens, outs, out_caps, out_lens, statuses, stream=None) -> None:
    """vds_ec_inflate_batch_device: stream o, lens[o] bytes at the device
    pointer ins[o], inflated into at most out_caps[o] bytes at the device
    pointer outs[o]; out_lens (uint32) and statuses (int32) are device buffers
    of one entry a stream, all written by the one launch."""
    ip, op = _ptr_table(ins), _ptr_table(outs)
    ln = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64).reshape(-1))
    cp = np.ascontiguousarray(np.asarray(out_caps, dtype=np.uint64).reshape(-1))
    if not (ip.size == ln.size == op.size == cp.size):
        raise VdsEcError(_lib.EINVAL, "inflate_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_inflate_batch_device(
        ln.size, ip.ctypes.data_as(_lib.vpp), ln.ctypes.data_as(_lib.u64p), op.ctypes.data_as(_lib.vpp),
        cp.ctypes.data_as(_lib.u64p), _dev_ptr(out_lens), _dev_ptr(statuses), _stream_ptr(stream)),
        "inflate_batch_device")


def _unpack_outs(caps):
    outs = [np.full(max(1, int(c)), 0xA5, dtype=np.uint8) for c in caps]
    return outs, (C.c_void_p * max(1, len(outs)))(*[o.ctypes.data for o in outs])


def inflate_host_batch(ins: Sequence, caps: Sequence) -> list:
    """vds_ec_inflate_host_batch: per stream (plaintext or None, status) --
    host streams inflated on the device in one call; caps[o] is stream o's
    capacity."""
    zs = [_u8(z) for z in ins]
    count = len(zs)
    if len(caps) != count:
        raise VdsEcError(_lib.EINVAL, "inflate_host_batch: one capacity per stream")
    ln = np.asarray([z.size for z in zs] or [0], dtype=np.uint64)
    cp = np.asarray([int(c) for c in caps] or [0], dtype=np.uint64)
    outs, op = _unpack_outs(caps)
    ol = np.zeros(max(1, count), dtype=np.uint64)
    st = np.zeros(max(1, count), dtype=np.int32)
    failed = C.c_uint32(0)
    ip = (C.c_void_p * max(1, count))(*[z.ctypes.data if z.size else None for z in zs])
    check(_lib.lib().vds_ec_inflate_host_batch(count, ip, ln.ctypes.data_as(_lib.u64p), op,
                                               cp.ctypes.data_as(_lib.u64p), ol.ctypes.data_as(_lib.u64p),
                                               st.ctypes.data_as(_lib.i32p), C.byref(failed)), "inflate_host_batch")
    return [(None if st[o] else outs[o][:int(ol[o])].tobytes(), int(st[o])) for o in range(count)]


def block_unpack_batch_device(crypted, crypted_lens, keys, ids, outs, out_caps, out_lens, statuses,
                              stream=None) -> None:
    """vds_ec_block_unpack_batch_device: client::restore for a batch of blocks
    on device pointers -- decrypt crypted[o] under keys + 32 o, inflate into
    outs[o] (at most out_caps[o] bytes), SHA-256 against ids + 32 o; three
    launches, statuses (int32) and out_lens (uint32) on the device."""
    ip, op = _ptr_table(crypted), _ptr_table(outs)
    ln = np.ascontiguousarray(np.asarray(crypted_lens, dtype=np.uint64).reshape(-1))
    cp = np.ascontiguousarray(np.asarray(out_caps, dtype=np.uint64).reshape(-1))
    if not (ip.size == ln.size == op.size == cp.size):
        raise VdsEcError(_lib.EINVAL, "block_unpack_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_block_unpack_batch_device(
        ln.size, ip.ctypes.data_as(_lib.vpp), ln.ctypes.data_as(_lib.u64p), _dev_ptr(keys), _dev_ptr(ids),
        op.ctypes.data_as(_lib.vpp), cp.ctypes.data_as(_lib.u64p), _dev_ptr(out_lens), _dev_ptr(statuses),
        _stream_ptr(stream)), "block_unpack_batch_device")


def block_unpack_host_batch(crypted: Sequence, keys: Sequence, ids: Sequence, caps: Sequence) -> list:
    """vds_ec_block_unpack_host_batch: per block (data or None, status) -- host
    bodies decrypted, inflated and checked against their ids on the device in
    one call; caps[o] is block o's capacity.  Unlike block_unpack_batch it
    raises for no block: a failed one has its status."""
    cts = [_u8(c) for c in crypted]
    count = len(cts)
    if not (len(keys) == len(ids) == len(caps) == count):
        raise VdsEcError(_lib.EINVAL, "block_unpack_host_batch: one key, id and capacity per block")
    kk = np.ascontiguousarray(np.frombuffer(b"".join(bytes(k) for k in keys), dtype=np.uint8))
    ii = np.ascontiguousarray(np.frombuffer(b"".join(bytes(i) for i in ids), dtype=np.uint8))
    if kk.size != 32 * count or ii.size != 32 * count:
        raise VdsEcError(_lib.EINVAL, "block_unpack_host_batch: keys and ids of 32 bytes")
    ln = np.asarray([c.size for c in cts] or [0], dtype=np.uint64)
    cp = np.asarray([int(c) for c in caps] or [0], dtype=np.uint64)
    outs, op = _unpack_outs(caps)
    ol = np.zeros(max(1, count), dtype=np.uint64)
    st = np.zeros(max(1, count), dtype=np.int32)
    failed = C.c_uint32(0)
    ip = (C.c_void_p * max(1, count))(*[c.ctypes.data if c.size else None for c in cts])
    check(_lib.lib().vds_ec_block_unpack_host_batch(
        count, ip, ln.ctypes.data_as(_lib.u64p), kk.ctypes.data if count else None, ii.ctypes.data if count else None,
        op, cp.ctypes.data_as(_lib.u64p), ol.ctypes.data_as(_lib.u64p), st.ctypes.data_as(_lib.i32p),
        C.byref(failed)), "block_unpack_host_batch")
    return [(None if st[o] else outs[o][:int(ol[o])].tobytes(), int(st[o])) for o in range(count)]


def deflate_bound(length: int) -> int:
    """vds_ec_deflate_bound: the size of the all-stored form, which no output
    of the library's deflate passes."""
    return int(_lib.lib().vds_ec_deflate_bound(length))


def deflate_host(data) -> bytes:
    """vds_ec_deflate_host: one buffer into a zlib stream on the calling
    thread, no GPU and no zlib; the bytes the device writes for the same data."""
    d = _u8(data)
    out = np.empty(deflate_bound(d.size), dtype=np.uint8)
    n = C.c_uint64(0)
    check(_lib.lib().vds_ec_deflate_host(d.ctypes.data if d.size else None, d.size, out.ctypes.data, out.size,
                                         C.byref(n)), "deflate_host")
    return out[:n.value].tobytes()


def deflate_batch_device(ins, lens, outs, out_caps, out_lens, stream=None) -> None:
    """vds_ec_deflate_batch_device: message o, lens[o] bytes at the device
    pointer ins[o], deflated into a zlib stream at the device pointer outs[o]
    (out_caps[o] >= deflate_bound(lens[o]) bytes); out_lens (uint32) is a
    device buffer of one entry a message, all written by the one launch."""
    ip, op = _ptr_table(ins), _ptr_table(outs)
    ln = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64).reshape(-1))
    cp = np.ascontiguousarray(np.asarray(out_caps, dtype=np.uint64).reshape(-1))
    if not (ip.size == ln.size == op.size == cp.size):
        raise VdsEcError(_lib.EINVAL, "deflate_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_deflate_batch_device(
        ln.size, ip.ctypes.data_as(_lib.vpp), ln.ctypes.data_as(_lib.u64p), op.ctypes.data_as(_lib.vpp),
        cp.ctypes.data_as(_lib.u64p), _dev_ptr(out_lens), _stream_ptr(stream)), "deflate_batch_device")


def deflate_host_batch(ins: Sequence) -> list:
    """vds_ec_deflate_host_batch: host buffers deflated on the device in one
    call -> one zlib stream (bytes) per buffer."""
    ds = [_u8(d) for d in ins]
    count = len(ds)
    ln = np.asarray([d.size for d in ds] or [0], dtype=np.uint64)
    outs = [np.empty(deflate_bound(d.size), dtype=np.uint8) for d in ds]
    cp = np.asarray([o.size for o in outs] or [0], dtype=np.uint64)
    ol = np.zeros(max(1, count), dtype=np.uint64)
    ip = (C.c_void_p * max(1, count))(*[d.ctypes.data if d.size else None for d in ds])
    op = (C.c_void_p * max(1, count))(*[o.ctypes.data for o in outs])
    check(_lib.lib().vds_ec_deflate_host_batch(count, ip, ln.ctypes.data_as(_lib.u64p), op,
                                               cp.ctypes.data_as(_lib.u64p), ol.ctypes.data_as(_lib.u64p)),
          "deflate_host_batch")
    return [outs[o][:int(ol[o])].tobytes() for o in range(count)]


def aes256_cbc_encrypt_gated_batch_device(ins, max_lens, lens, keys, outs, out_lens, ivs=None, stream=None) -> None:
    """vds_ec_aes256_cbc_encrypt_gated_batch_device: the batched encrypt with
    the lengths on the device -- message o is the first lens[o] (device uint32)
    bytes at ins[o], at most max_lens[o] (host); out_lens (device uint32)
    receives aes256_cbc_padded_size(lens[o])."""
    ip, op = _ptr_table(ins), _ptr_table(outs)
    ml = np.ascontiguousarray(np.asarray(max_lens, dtype=np.uint64).reshape(-1))
    if not (ip.size == ml.size == op.size):
        raise VdsEcError(_lib.EINVAL, "aes256_cbc_encrypt_gated_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_aes256_cbc_encrypt_gated_batch_device(
        ml.size, ip.ctypes.data_as(_lib.vpp), ml.ctypes.data_as(_lib.u64p), _dev_ptr(lens), _dev_ptr(keys),
        _dev_ptr(ivs), op.ctypes.data_as(_lib.vpp), _dev_ptr(out_lens), _stream_ptr(stream)),
        "aes256_cbc_encrypt_gated_batch_device")


def block_pack_deflate_batch_device(datas, data_lens, ids, keys, crypted, crypted_caps, crypted_lens,
                                    stream=None) -> None:
    """vds_ec_block_pack_deflate_batch_device: client::save for a batch of
    blocks on device pointers with the deflate on the device too -- ids + 32 o
    = SHA-256(data o), keys + 32 o = SHA-256(AES(id, data)), crypted[o] =
    AES(key, deflate(data o)), five launches; crypted_caps[o] >=
    aes256_cbc_padded_size(deflate_bound(data_lens[o])), crypted_lens (device
    uint32) receives the bodies' sizes."""
    dp, cp = _ptr_table(datas), _ptr_table(crypted)
    dl = np.ascontiguousarray(np.asarray(data_lens, dtype=np.uint64).reshape(-1))
    cc = np.ascontiguousarray(np.asarray(crypted_caps, dtype=np.uint64).reshape(-1))
    if not (dp.size == dl.size == cp.size == cc.size):
        raise VdsEcError(_lib.EINVAL, "block_pack_deflate_batch: the arrays do not describe one batch")
    check(_lib.lib().vds_ec_block_pack_deflate_batch_device(
        dl.size, dp.ctypes.data_as(_lib.vpp), dl.ctypes.data_as(_lib.u64p), _dev_ptr(ids), _dev_ptr(keys),
        cp.ctypes.data_as(_lib.vpp), cc.ctypes.data_as(_lib.u64p), _dev_ptr(crypted_lens), _stream_ptr(stream)),
        "block_pack_deflate_batch_device")


def block_pack_deflate_host_batch(datas: Sequence) -> list:
    """vds_ec_block_pack_deflate_host_batch: one (id, key, crypted) per block
    (host bytes), every step on the device: crypted = AES(key,
    deflate_host(data))."""
    ds = [_u8(d) for d in datas]
    count = len(ds)
    dl = np.asarray([d.size for d in ds] or [0], dtype=np.uint64)
    outs = [np.empty(aes256_cbc_padded_size(deflate_bound(d.size)), dtype=np.uint8) for d in ds]
    cc = np.asarray([o.size for o in outs] or [0], dtype=np.uint64)
    ids = np.empty((max(1, count), 32), dtype=np.uint8)
    keys = np.empty((max(1, count), 32), dtype=np.uint8)
    cs = np.zeros(max(1, count), dtype=np.uint64)
    dp = (C.c_void_p * max(1, count))(*[d.ctypes.data if d.size else None for d in ds])
    cp = (C.c_void_p * max(1, count))(*[o.ctypes.data for o in outs])
    check(_lib.lib().vds_ec_block_pack_deflate_host_batch(
        count, dp, dl.ctypes.data_as(_lib.u64p), ids.ctypes.data, keys.ctypes.data, cp,
        cc.ctypes.data_as(_lib.u64p), cs.ctypes.data_as(_lib.u64p)), "block_pack_deflate_host_batch")
    return [(bytes(ids[o]), bytes(keys[o]), outs[o][:int(cs[o])].tobytes()) for o in range(count)]


def block_pack_batch(datas: Sequence, level: int = 6) -> list:
    """save_block / client::save for a batch of blocks: per block (id, key,
    crypted) with id = SHA-256(data), key = SHA-256(AES(id, data)) and crypted
    = AES(key, zlib.compress(data, level)); the hashes and ciphers run on the
    device (vds_ec_block_pack_host_batch), the deflate here."""
    import zlib
    ds = [bytes(_u8(d)) for d in datas]
    return block_pack_host_batch(ds, [zlib.compress(d, level) for d in ds])


def block_unpack_batch(crypted: Sequence, keys: Sequence, ids: Sequence) -> list:
    """client::restore for a batch of blocks: decrypt under keys on the device
    (vds_ec_aes256_cbc_decrypt_host_batch), inflate, and compare the SHA-256
    with ids.  Raises VdsEcError with the first failing block's decrypt status,
    or VDS_EC_ECORRUPT ("Data is corrupted") where the bytes do not inflate or
    do not hash to their id."""
    import hashlib
    import zlib
    if len(ids) != len(crypted):
        raise VdsEcError(_lib.EINVAL, "block_unpack_batch: one id per block")
    res = []
    for o, (plain, st) in enumerate(aes256_cbc_decrypt_host_batch(crypted, keys)):
        if st:
            raise VdsEcError(st, f"block_unpack_batch: block {o}")
        try:
            data = zlib.decompress(plain)
        except zlib.error:
            raise VdsEcError(_lib.ECORRUPT, f"block_unpack_batch: block {o} does not inflate") from None
        if hashlib.sha256(data).digest() != bytes(ids[o]):
            raise VdsEcError(_lib.ECORRUPT, f"block_unpack_batch: block {o}")
        res.append(data)
    return res


def _mag(value) -> np.ndarray:
    """A big-endian magnitude from an int or from bytes as they stand."""
    if isinstance(value, int):
        value = value.to_bytes(max(1, (value.bit_length() + 7) // 8), "big")
    return _u8(value)


def rsa_key_prepare(n, e) -> _lib.RsaKey:
    """vds_ec_rsa_key_prepare: the public key (n, e) -- ints or big-endian
    bytes -- ready for the Montgomery arithmetic of the host and the device."""
    nb, eb = _mag(n), _mag(e)
    key = _lib.RsaKey()
    check(_lib.lib().vds_ec_rsa_key_prepare(nb.ctypes.data, nb.size, eb.ctypes.data, eb.size, C.byref(key)),
          "rsa_key_prepare")
    return key


def rsa_fingerprint(n, e) -> bytes:
    """vds_ec_rsa_fingerprint: asymmetric_public_key::fingerprint(), the
    writer's key id of a transaction block."""
    nb, eb = _mag(n), _mag(e)
    out = np.empty(32, dtype=np.uint8)
    check(_lib.lib().vds_ec_rsa_fingerprint(nb.ctypes.data, nb.size, eb.ctypes.data, eb.size, out.ctypes.data),
          "rsa_fingerprint")
    return out.tobytes()


def rsa_public_host(key: _lib.RsaKey, data) -> bytes:
    """vds_ec_rsa_public_host: data^e mod n as key.n_bytes big-endian bytes, on
    the calling thread.  VDS_EC_EINVAL for another length or a value >= n."""
    d = _u8(data)
    out = np.empty(max(1, key.n_bytes), dtype=np.uint8)
    check(_lib.lib().vds_ec_rsa_public_host(C.byref(key), d.ctypes.data if d.size else None, d.size, out.ctypes.data),
          "rsa_public_host")
    return out[:key.n_bytes].tobytes()


def rsa_verify_sha256_host(key: _lib.RsaKey, msg, sig) -> bool:
    """vds_ec_rsa_verify_sha256_host: EVP_DigestVerify(SHA-256)'s verdict on
    the calling thread, no GPU and no OpenSSL."""
    m, s = _u8(msg), _u8(sig)
    v = C.c_uint8(0)
    check(_lib.lib().vds_ec_rsa_verify_sha256_host(C.byref(key), m.ctypes.data if m.size else None, m.size,
                                                   s.ctypes.data if s.size else None, s.size, C.byref(v)),
          "rsa_verify_sha256_host")
    return bool(v.value)


def _rsa_keys(keys):
    ks = list(keys)
    return (_lib.RsaKey * max(1, len(ks)))(*ks), len(ks)


def rsa_public_batch_device(ins, in_lens, key_idx, keys, outs, statuses, stream=None) -> None:
    """vds_ec_rsa_public_batch_device: item o, in_lens[o] big-endian bytes at
    the device pointer ins[o], raised to e modulo n of keys[key_idx[o]] into the
    key's n_bytes at the device pointer outs[o]; statuses (device, one byte an
    item): 0, or 0xFF (VDS_EC_EINVAL) and outs[o] untouched.  One launch."""
    ip, op = _ptr_table(ins), _ptr_table(outs)
    ln = np.ascontiguousarray(np.asarray(in_lens, dtype=np.uint64).reshape(-1))
    ki = _u32(key_idx)
    if not (ip.size == ln.size == op.size == ki.size):
        raise VdsEcError(_lib.EINVAL, "rsa_public_batch: the arrays do not describe one batch")
    ka, nk = _rsa_keys(keys)
    check(_lib.lib().vds_ec_rsa_public_batch_device(
        ln.size, ip.ctypes.data_as(_lib.vpp), ln.ctypes.data_as(_lib.u64p), ki.ctypes.data_as(_lib.u32p), ka, nk,
        op.ctypes.data_as(_lib.vpp), _dev_ptr(statuses), _stream_ptr(stream)), "rsa_public_batch_device")


def rsa_verify_digest_batch_device(digests, sigs, sig_lens, key_idx, keys, verdicts, stream=None) -> None:
    """vds_ec_rsa_verify_digest_batch_device: the verdict (device, one byte an
    item, 1 or 0) of signature o -- sig_lens[o] bytes at the device pointer
    sigs[o] -- over the SHA-256 digest at digests + 32 o (device) under
    keys[key_idx[o]].  One launch."""
    sp = _ptr_table(sigs)
    ln = np.ascontiguousarray(np.asarray(sig_lens, dtype=np.uint64).reshape(-1))
    ki = _u32(key_idx)
    if not (sp.size == ln.size == ki.size):
        raise VdsEcError(_lib.EINVAL, "rsa_verify_digest_batch: the arrays do not describe one batch")
    ka, nk = _rsa_keys(keys)
    check(_lib.lib().vds_ec_rsa_verify_digest_batch_device(
        ln.size, _dev_ptr(digests), sp.ctypes.data_as(_lib.vpp), ln.ctypes.data_as(_lib.u64p),
        ki.ctypes.data_as(_lib.u32p), ka, nk, _dev_ptr(verdicts), _stream_ptr(stream)),
        "rsa_verify_digest_batch_device")


def rsa_verify_sha256_batch_device(msgs, lens, sigs, sig_lens, key_idx, keys, verdicts, digests=None,
                                   stream=None) -> None:
    """vds_ec_rsa_verify_sha256_batch_device: the batched SHA-256 of the device
    messages (msgs, lens), then the launch above; digests (device, 32 bytes an
    item) receives the digests unless None."""
    mp, sp = _ptr_table(msgs), _ptr_table(sigs)
    ml = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64).reshape(-1))
    ln = np.ascontiguousarray(np.asarray(sig_lens, dtype=np.uint64).reshape(-1))
    ki = _u32(key_idx)
    if not (mp.size == ml.size == sp.size == ln.size == ki.size):
        raise VdsEcError(_lib.EINVAL, "rsa_verify_sha256_batch: the arrays do not describe one batch")
    ka, nk = _rsa_keys(keys)
    check(_lib.lib().vds_ec_rsa_verify_sha256_batch_device(
        ln.size, mp.ctypes.data_as(_lib.vpp), ml.ctypes.data_as(_lib.u64p), sp.ctypes.data_as(_lib.vpp),
        ln.ctypes.data_as(_lib.u64p), ki.ctypes.data_as(_lib.u32p), ka, nk, _dev_ptr(verdicts), _dev_ptr(digests),
        _stream_ptr(stream)), "rsa_verify_sha256_batch_device")


def txblock_parse(data) -> tuple:
    """vds_ec_txblock_parse -> (status, fields): VDS_EC_OK and the block's
    fields (a dict of vds_ec_txblock's members), or VDS_EC_ETX_FORM and None."""
    d = _u8(data)
    b = _lib.TxBlock()
    st = _lib.lib().vds_ec_txblock_parse(d.ctypes.data if d.size else None, d.size, C.byref(b))
    if st == _lib.EINVAL and d.size == 0:  # (no bytes at all: no pointer to give)
        st = _lib.ETX_FORM
    if st not in (_lib.OK, _lib.ETX_FORM):
        check(st, "txblock_parse")
    return int(st), ({f: int(getattr(b, f)) for f, _ in _lib.TxBlock._fields_} if st == _lib.OK else None)


def txblock_validate_host_batch(blocks: Sequence, keys, fingerprints: Sequence) -> list:
    """vds_ec_txblock_validate_host_batch: per block (id, status, verdict) --
    apply_message's check of a drained batch of transaction-log records (host
    bytes) under the prepared keys and their fingerprints, on the device."""
    bs = [_u8(b) for b in blocks]
    count = len(bs)
    ka, nk = _rsa_keys(keys)
    fp = np.ascontiguousarray(np.frombuffer(b"".join(bytes(f) for f in fingerprints), dtype=np.uint8))
    if fp.size != 32 * nk:
        raise VdsEcError(_lib.EINVAL, "txblock_validate_host_batch: one fingerprint of 32 bytes per key")
    ln = np.asarray([b.size for b in bs] or [0], dtype=np.uint64)
    ids = np.zeros((max(1, count), 32), dtype=np.uint8)
    ver = np.zeros(max(1, count), dtype=np.uint8)
    st = np.zeros(max(1, count), dtype=np.int32)
    bp = (C.c_void_p * max(1, count))(*[b.ctypes.data if b.size else None for b in bs])
    check(_lib.lib().vds_ec_txblock_validate_host_batch(
        count, bp, ln.ctypes.data_as(_lib.u64p), ka, fp.ctypes.data if nk else None, nk, ids.ctypes.data,
        ver.ctypes.data, st.ctypes.data_as(_lib.i32p)), "txblock_validate_host_batch")
    return [(bytes(ids[o]), int(st[o]), int(ver[o])) for o in range(count)]
