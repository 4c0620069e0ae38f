#!/usr/bin/env python3
"""Measure the base64 wire text on the device (vds_ec_base64_decode_batch_device
/ _encode_batch_device) and the batched upload from text
(vds_ec_upload16_host_batch) on the live shape.  (Not bench.py: that one stays
the project's yardstick.)

Workload, as tools/bench_save_temp_batch.py: k = 32, n = 64, 16,384 bodies of
seeded sizes that are multiples of 16 in [49,152, 65,552], replicas in 256-byte
aligned slots; each body's base64 text at a 16-byte aligned offset of one
device buffer.

Device legs (each call alone behind a spin kernel that covers its host work:
device time; decode and save_temp interleaved A B B A):
  decode     vds_ec_base64_decode_batch_device over the 16,384 texts;
  save_temp  vds_ec_save_temp16_batch_device (with body digests) on the bodies
             the decode wrote -- the call the decode feeds, unchanged code;
  encode     vds_ec_base64_encode_batch_device over the bodies;
  copy       a device copy that moves the decode's bytes (text read plus body
             written), in the same process.
The purpose test: decode must take less device time than save_temp (exit
status 1 otherwise).

Host legs (wall time of one call on the calling thread, --host-calls each):
  upload     vds_ec_upload16_host_batch from the texts;
  before     vds_ec_base64_decode per body on the calling thread, then
             vds_ec_save_temp16_host_batch (what a caller did before);
  host_encode  vds_ec_base64_encode per body on the calling thread.

Prints one JSON line per leg and a summary line; --out also writes them to a
file.
"""
from __future__ import annotations

import argparse
import base64
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N = 32, 64
SEED = 0x656E6362


def mm(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(min(x)), 4), "max": round(float(max(x)), 4)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=6, help="A B B A rounds of the device legs")
    ap.add_argument("--host-calls", type=int, default=2, help="timed calls of each host leg (after one warm-up)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from vds_amd import _lib, build, chunk
    build.build()
    if not torch.cuda.is_available():
        print("bench_upload_batch: no GPU: nothing is measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    vpp, u64p = _lib.vpp, _lib.u64p

    objects = args.objects
    rng = np.random.default_rng(SEED)
    sizes = (16 * rng.integers(49152 // 16, 65552 // 16 + 1, objects)).astype(np.uint64)
    in_off = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint64)  # multiples of 16: back to back
    total = int(sizes.sum())
    tlens = ((sizes + np.uint64(2)) // np.uint64(3) * np.uint64(4)).astype(np.uint64)
    t_off = np.concatenate(([0], np.cumsum((tlens + np.uint64(15)) // np.uint64(16) * np.uint64(16))[:-1])).astype(np.uint64)
    t_total = int(t_off[-1] + (tlens[-1] + 15) // 16 * 16)
    inp = torch.empty(total, dtype=torch.uint8, device=dev)
    chunk.fill_splitmix_device(inp, inp.numel(), SEED)
    torch.cuda.synchronize(dev)
    host_in = inp.cpu().numpy()
    texts = [base64.b64encode(host_in[int(o):int(o + s)].tobytes()) for o, s in zip(in_off, sizes)]
    host_text = np.zeros(t_total, dtype=np.uint8)
    for t, o in zip(texts, t_off):
        host_text[int(o):int(o) + len(t)] = np.frombuffer(t, dtype=np.uint8)
    d_text = torch.from_numpy(host_text).to(dev)
    d_body = torch.zeros(total, dtype=torch.uint8, device=dev)
    d_enc = torch.zeros(t_total, dtype=torch.uint8, device=dev)
    d_st = torch.full((objects,), 77, dtype=torch.int32, device=dev)
    slot = (chunk.replica_size(K, 65552) + 255) // 256 * 256
    out = torch.empty(objects * N * slot, dtype=torch.uint8, device=dev)
    rd = torch.zeros(objects * N * 32, dtype=torch.uint8, device=dev)
    dd = torch.zeros(objects * 32, dtype=torch.uint8, device=dev)
    tp = (d_text.data_ptr() + t_off).astype(np.uint64)
    bp = (d_body.data_ptr() + in_off).astype(np.uint64)
    ep = (d_enc.data_ptr() + t_off).astype(np.uint64)
    outs = (out.data_ptr() + np.arange(objects * N, dtype=np.uint64) * np.uint64(slot)).astype(np.uint64)
    half = (t_total + total) // 2 // 16 * 16  # a copy of `half` bytes reads and writes what the decode reads and writes
    c_src = torch.empty(half, dtype=torch.uint8, device=dev)
    c_dst = torch.empty(half, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream
    log = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.append(line)

    def call_decode():
        rc = lib.vds_ec_base64_decode_batch_device(objects, tp.ctypes.data_as(vpp), tlens.ctypes.data_as(u64p),
                                                   bp.ctypes.data_as(vpp), sizes.ctypes.data_as(u64p),
                                                   d_st.data_ptr(), sp)
        assert rc == 0, rc

    def call_save_temp():
        rc = lib.vds_ec_save_temp16_batch_device(K, N, objects, bp.ctypes.data_as(vpp), sizes.ctypes.data_as(u64p),
                                                 outs.ctypes.data_as(vpp), rd.data_ptr(), dd.data_ptr(), sp)
        assert rc == 0, rc

    def call_encode():
        rc = lib.vds_ec_base64_encode_batch_device(objects, bp.ctypes.data_as(vpp), sizes.ctypes.data_as(u64p),
                                                   ep.ctypes.data_as(vpp), sp)
        assert rc == 0, rc

    def call_copy():
        c_dst.copy_(c_src, non_blocking=True)

    spin = {}

    def spin_cycles(ms):
        if "per_ms" not in spin:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            torch.cuda._sleep(10 ** 7)
            b.record(stream)
            torch.cuda.synchronize(dev)
            spin["per_ms"] = 10 ** 7 / max(a.elapsed_time(b), 1e-3)
        return int(spin["per_ms"] * ms)

    host_ms = {}

    def alone(name, fn):
        """Device time of one call: enqueued behind a spin kernel that outlasts its host work."""
        torch.cuda._sleep(spin_cycles(2 * host_ms[name] + 2.0))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b)

    legs = {"decode": call_decode, "save_temp": call_save_temp, "encode": call_encode, "copy": call_copy}
    with torch.cuda.stream(stream):
        emit({"workload": {"k": K, "n": N, "objects": objects, "body_bytes": total, "text_bytes": int(tlens.sum()),
                           "size_min": int(sizes.min()), "size_max": int(sizes.max()), "replica_slot": slot,
                           "seed": SEED}})
        for name, fn in legs.items():  # warm-up, and each call's host time
            h = []
            for _ in range(3):
                h0 = time.perf_counter()
                fn()
                h.append((time.perf_counter() - h0) * 1e3)
                torch.cuda.synchronize(dev)
            host_ms[name] = max(h)
        assert int(d_st.abs().max()) == 0, "a text of the workload did not decode"
        assert torch.equal(d_body, inp), "decoded bodies differ from the bodies"
        assert torch.equal(d_enc, d_text), "encoded text differs from the text"
        t = {name: [] for name in legs}
        for _ in range(max(1, args.rounds)):
            for name in ("decode", "save_temp", "save_temp", "decode"):  # A B B A
                t[name].append(alone(name, legs[name]))
            for name in ("encode", "copy", "copy", "encode"):
                t[name].append(alone(name, legs[name]))
        moved = {"decode": int(tlens.sum()) + total, "encode": int(tlens.sum()) + total, "copy": 2 * half,
                 "save_temp": None}
        for name in legs:
            rec = {"leg": name, "device_ms_per_call": mm(t[name]), "host_enqueue_ms_max": round(host_ms[name], 4),
                   "calls": len(t[name])}
            if moved[name]:
                rec["bytes_moved"] = moved[name]
                rec["gib_s_moved"] = round(moved[name] / (np.median(t[name]) * 1e-3) / 2 ** 30, 1)
            emit(rec)

    # ---------------------------------------------------------------- host legs
    L = [chunk.replica_size(K, int(s)) for s in sizes]
    h_outs = np.empty((objects * N, max(L)), dtype=np.uint8)
    h_rd = np.empty(objects * N * 32, dtype=np.uint8)
    h_dd = np.empty(objects * 32, dtype=np.uint8)
    h_st = np.zeros(objects, dtype=np.int32)
    h_body = np.empty(total, dtype=np.uint8)
    failed = C.c_uint32(0)
    c_texts = (C.c_char_p * objects)(*texts)
    c_outs = (h_outs.ctypes.data + np.arange(objects * N, dtype=np.uint64) * np.uint64(h_outs.shape[1])).astype(np.uint64)
    c_body = (h_body.ctypes.data + in_off).astype(np.uint64)

    def host_upload():
        rc = lib.vds_ec_upload16_host_batch(K, N, objects, C.cast(c_texts, vpp), tlens.ctypes.data_as(u64p),
                                            c_outs.ctypes.data_as(vpp), h_rd.ctypes.data, h_dd.ctypes.data, None, None,
                                            None, h_st.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(failed))
        assert rc == 0 and failed.value == 0, (rc, failed.value)

    dec_ms = []

    def host_before():
        n = C.c_size_t(0)
        h0 = time.perf_counter()
        for o in range(objects):
            rc = lib.vds_ec_base64_decode(texts[o], len(texts[o]), int(c_body[o]), C.byref(n))
            assert rc == 0, rc
        dec_ms.append((time.perf_counter() - h0) * 1e3)
        rc = lib.vds_ec_save_temp16_host_batch(K, N, objects, c_body.ctypes.data_as(vpp), sizes.ctypes.data_as(u64p),
                                               c_outs.ctypes.data_as(vpp), h_rd.ctypes.data, h_dd.ctypes.data, None)
        assert rc == 0, rc

    # the host encoder over the same bodies (what "download" pays a body today)
    enc_buf = C.create_string_buffer(int(tlens.max()) + 1)
    n_enc = C.c_size_t(0)
    enc_ms = []
    for _ in range(2):
        h0 = time.perf_counter()
        for o in range(objects):
            rc = lib.vds_ec_base64_encode(host_in.ctypes.data + int(in_off[o]), int(sizes[o]), enc_buf, len(enc_buf),
                                          C.byref(n_enc))
            assert rc == 0, rc
        enc_ms.append((time.perf_counter() - h0) * 1e3)
    assert enc_buf.raw[:n_enc.value] == texts[-1]
    wall = {}
    names = {}
    for name, fn in (("upload", host_upload), ("before", host_before)):
        fn()  # warm-up: the staging grows to the workload
        names[name] = h_rd.copy()
        w = []
        for _ in range(max(1, args.host_calls)):
            h0 = time.perf_counter()
            fn()
            w.append((time.perf_counter() - h0) * 1e3)
        wall[name] = w
    assert np.array_equal(names["upload"], names["before"]), "the two host routes name the replicas differently"
    assert np.array_equal(h_body, host_in)
    emit({"leg": "host_upload", "wall_ms_per_call": mm(wall["upload"]), "calls": len(wall["upload"])})
    emit({"leg": "host_before", "wall_ms_per_call": mm(wall["before"]), "calls": len(wall["before"]),
          "of_which_host_decode_ms": mm(dec_ms[1:] or dec_ms),
          "host_decode_us_per_body": round(float(np.median(dec_ms[1:] or dec_ms)) * 1e3 / objects, 1)})
    emit({"leg": "host_encode", "wall_ms_per_batch": mm(enc_ms),
          "host_encode_us_per_body": round(min(enc_ms) * 1e3 / objects, 1)})
    d = lambda name: float(np.median(t[name]))
    ok = d("decode") < d("save_temp")
    emit({"summary": {"decode_device_ms": round(d("decode"), 4), "save_temp_device_ms": round(d("save_temp"), 4),
                      "encode_device_ms": round(d("encode"), 4), "copy_device_ms": round(d("copy"), 4),
                      "decode_over_save_temp": round(d("decode") / d("save_temp"), 3),
                      "decode_over_copy": round(d("decode") / d("copy"), 2),
                      "encode_over_copy": round(d("encode") / d("copy"), 2),
                      "host_upload_wall_ms": round(float(np.median(wall["upload"])), 1),
                      "host_before_wall_ms": round(float(np.median(wall["before"])), 1),
                      "before_over_upload_wall": round(float(np.median(wall["before"]) / np.median(wall["upload"])), 2),
                      "decode_faster_than_save_temp": ok}})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(log) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
