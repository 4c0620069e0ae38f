#!/usr/bin/env python3
"""Measure the batched encode of ragged objects against what a caller could do
before it existed.  (Not bench.py: that one stays the project's yardstick.)

Workload: k = 32, n = 64, 16,384 device-resident objects, seeded sizes that
are multiples of 16 in [49,152, 65,552] (an upload's deflated and encrypted
64 KiB pieces), replicas in 256-byte aligned slots.

Legs, timed with device events as bench.py's live leg does (5 untimed calls,
then >= 10 timed back to back: the stream span a looping caller sees; then the
same call alone behind a spin kernel that covers its host work: device time):
  a  vds_ec_encode16_batch_device, one call for the whole batch;
  b  one vds_ec_encode16_device call per object, the same objects;
  c  vds_ec_encode16_device on 16,384 objects of exactly 65,536 bytes: the
     uniform stream kernel, no tables and no masks (the ceiling).
b and c run from --parent-lib (a build of the parent commit, vds_amd.build
.build(out=...)) when given, else from the library under test.  Order
a b b a, then c: a and b alternate on the same box.

Prints one JSON line per leg run and a summary line; --out also writes them
to a file.
"""
from __future__ import annotations

import argparse
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
    ap.add_argument("--calls", type=int, default=10, help="timed calls per leg run (at least 10)")
    ap.add_argument("--loop-calls", type=int, default=3, help="device-alone repeats of the per-object loop")
    ap.add_argument("--parent-lib", default=None, help="libvds_ec.so built from the parent commit, for legs b and c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    calls = max(10, args.calls)

    import torch
    from vds_amd import _lib, build, chunk
    build.build()
    if not torch.cuda.is_available():
        print("bench_encode_batch: no GPU: nothing is measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    old = lib
    if args.parent_lib:
        old = C.CDLL(os.path.abspath(args.parent_lib))
        old.vds_ec_encode16_device.restype = C.c_int
        old.vds_ec_encode16_device.argtypes = _lib.SIGNATURES["vds_ec_encode16_device"][1]

    objects = args.objects
    rng = np.random.default_rng(SEED)
    sizes = (16 * rng.integers(49152 // 16, 65552 // 16 + 1, objects)).astype(np.uint64)
    in_off = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint64)  # multiples of 16: back to back
    total = int(sizes.sum())
    slot = (chunk.replica_size(K, 65552) + 255) // 256 * 256
    inp = torch.empty(max(total, objects * 65536), dtype=torch.uint8, device=dev)
    chunk.fill_splitmix_device(inp, inp.numel(), SEED)
    out = torch.empty(objects * N * slot, dtype=torch.uint8, device=dev)
    ins = (inp.data_ptr() + in_off).astype(np.uint64)
    outs = (out.data_ptr() + np.arange(objects * N, dtype=np.uint64) * np.uint64(slot)).astype(np.uint64)
    ids = np.arange(N, dtype=np.uint16)
    idp = ids.ctypes.data_as(_lib.u16p)
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream
    log = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.append(line)

    def call_a():
        rc = lib.vds_ec_encode16_batch_device(K, idp, N, objects, ins.ctypes.data_as(_lib.vpp),
                                              sizes.ctypes.data_as(_lib.u64p), outs.ctypes.data_as(_lib.vpp), 0, sp)
        assert rc == 0, rc

    # leg b's arguments, built once: the loop below is the calls alone
    out_rows = [C.cast(outs.ctypes.data + 8 * N * o, _lib.vpp) for o in range(objects)]
    in_list = [int(x) for x in ins]
    size_list = [int(x) for x in sizes]
    enc_old = old.vds_ec_encode16_device

    def call_b():
        for o in range(objects):
            rc = enc_old(K, idp, N, in_list[o], size_list[o], 0, 1, out_rows[o], 0, 0, sp)
            assert rc == 0, rc

    L_c = chunk.replica_size(K, 65536)
    Ls_c = (L_c + 255) // 256 * 256
    assert N * objects * Ls_c <= out.numel()
    outs_c = (C.c_void_p * N)(*[out.data_ptr() + i * objects * Ls_c for i in range(N)])

    def call_c():
        rc = old.vds_ec_encode16_device(K, idp, N, inp.data_ptr(), 65536, 65536, objects, outs_c, Ls_c, 0, sp)
        assert rc == 0, rc

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

    def run(leg, fn, nbytes, timed_calls, alone_calls):
        for _ in range(5):
            fn()
        torch.cuda.synchronize(dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(timed_calls + 1)]
        host = []
        ev[0].record(stream)
        for i in range(timed_calls):
            h0 = time.perf_counter()
            fn()
            host.append((time.perf_counter() - h0) * 1e3)
            ev[i + 1].record(stream)
        torch.cuda.synchronize(dev)
        spans = [ev[i].elapsed_time(ev[i + 1]) for i in range(timed_calls)]
        alone = []
        for _ in range(alone_calls):
            torch.cuda._sleep(spin_cycles(2 * max(host) + 2.0))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            torch.cuda.synchronize(dev)
            alone.append(a.elapsed_time(b))
        gib = lambda ms: round(nbytes / (ms * 1e-3) / 2 ** 30, 2)
        rec = {"leg": leg, "objects": objects, "object_bytes": nbytes, "stream_ms_per_call": mm(spans),
               "device_ms_per_call": mm(alone), "host_enqueue_ms_per_call": mm(host), "calls": timed_calls,
               "gib_s_stream": gib(np.median(spans)), "gib_s_device": gib(np.median(alone)),
               "bound": "host" if np.median(spans) > 1.1 * np.median(alone) else "device"}
        emit(rec)
        return rec

    with torch.cuda.stream(stream):
        emit({"workload": {"k": K, "n": N, "objects": objects, "bytes": total, "size_min": int(sizes.min()),
                           "size_max": int(sizes.max()), "replica_slot": slot, "seed": SEED},
              "parent_lib": bool(args.parent_lib),
              "batch_path": chunk.encode_batch_path(K, list(range(N)), ins, sizes, outs)})
        a1 = run("a", call_a, total, calls, calls)
        b1 = run("b", call_b, total, calls, args.loop_calls)
        b2 = run("b", call_b, total, calls, args.loop_calls)
        a2 = run("a", call_a, total, calls, calls)
        c = run("c", call_c, objects * 65536, calls, calls)
    a_dev = (a1["gib_s_device"] + a2["gib_s_device"]) / 2
    a_str = (a1["gib_s_stream"] + a2["gib_s_stream"]) / 2
    b_dev = (b1["gib_s_device"] + b2["gib_s_device"]) / 2
    b_str = (b1["gib_s_stream"] + b2["gib_s_stream"]) / 2
    emit({"summary": {"a_gib_s_device": round(a_dev, 2), "a_gib_s_stream": round(a_str, 2),
                      "b_gib_s_device": round(b_dev, 2), "b_gib_s_stream": round(b_str, 2),
                      "c_gib_s_device": c["gib_s_device"], "c_gib_s_stream": c["gib_s_stream"],
                      "a_over_c_device": round(a_dev / c["gib_s_device"], 3),
                      "a_over_b_device": round(a_dev / b_dev, 2), "a_over_b_stream": round(a_str / b_str, 2),
                      "a_host_enqueue_ms_median": round((a1["host_enqueue_ms_per_call"]["median"] +
                                                         a2["host_enqueue_ms_per_call"]["median"]) / 2, 4)}})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(log) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
