#!/usr/bin/env python3
"""Measure the batched save_temp (encode + every replica's SHA-256 name + the
bodies' SHA-256) of ragged objects against what a caller could do before it
existed.  (Not bench.py: that one stays the project's yardstick.)

Workload, as tools/bench_encode_batch.py: k = 32, n = 64, 16,384
device-resident objects, seeded sizes that are multiples of 16 in [49,152,
65,552], replicas in 256-byte aligned slots.

Legs, timed as there (untimed warm-up calls, then >= 10 timed back to back:
the stream span a looping caller sees; then the same call alone behind a spin
kernel that covers its host work: device time):
  a       vds_ec_save_temp16_batch_device with body digests;
  a_nobody   the same with data_digests = NULL (names only);
  a_split   a_nobody, then the bodies through vds_ec_sha256_batch_device: the
          body chains in a hash launch of their own (the alternative to
          placing them first in the one launch);
  b       what a caller could do before: one vds_ec_encode16_batch_device, one
          vds_ec_sha256_device per object, and vds_ec_sha256_host per body on
          the caller's thread (from a host copy of the bodies);
  b_nobody   b without the body part;
  c       the ceiling at uniform size: vds_ec_encode16_device plus ONE
          vds_ec_sha256_device launch on 16,384 objects of 65,536 bytes
          (bench.py's serial save_temp leg).
b and c run from --parent-lib (a build of the parent commit, vds_amd.build
.build(out=...)) when given, else from the library under test.

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
    ap.add_argument("--loop-calls", type=int, default=3, help="device-alone repeats of the per-object loops")
    ap.add_argument("--parent-lib", default=None, help="libvds_ec.so built from the parent commit, for legs b and c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    calls = max(10, args.calls)

    import torch
    from vds_amd import _lib, build, chunk
    build.build()
    if not torch.cuda.is_available():
        print("bench_save_temp_batch: no GPU: nothing is measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    old = lib
    if args.parent_lib:
        old = C.CDLL(os.path.abspath(args.parent_lib))
        for name in ("vds_ec_encode16_device", "vds_ec_encode16_batch_device", "vds_ec_sha256_device",
                     "vds_ec_sha256_host"):
            getattr(old, name).restype = C.c_int
            getattr(old, name).argtypes = _lib.SIGNATURES[name][1]

    objects = args.objects
    rng = np.random.default_rng(SEED)
    sizes = (16 * rng.integers(49152 // 16, 65552 // 16 + 1, objects)).astype(np.uint64)
    in_off = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint64)  # multiples of 16: back to back
    total = int(sizes.sum())
    slot = (chunk.replica_size(K, 65552) + 255) // 256 * 256
    inp = torch.empty(max(total, objects * 65536), dtype=torch.uint8, device=dev)
    chunk.fill_splitmix_device(inp, inp.numel(), SEED)
    out = torch.empty(objects * N * slot, dtype=torch.uint8, device=dev)
    rd = torch.zeros(objects * N * 32, dtype=torch.uint8, device=dev)
    dd = torch.zeros(objects * 32, dtype=torch.uint8, device=dev)
    rd_b = torch.zeros_like(rd)
    ins = (inp.data_ptr() + in_off).astype(np.uint64)
    outs = (out.data_ptr() + np.arange(objects * N, dtype=np.uint64) * np.uint64(slot)).astype(np.uint64)
    ids = np.arange(N, dtype=np.uint16)
    idp = ids.ctypes.data_as(_lib.u16p)
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream
    log = []
    vpp, u64p = _lib.vpp, _lib.u64p

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.append(line)

    def call_a(body=True):
        rc = lib.vds_ec_save_temp16_batch_device(K, N, objects, ins.ctypes.data_as(vpp), sizes.ctypes.data_as(u64p),
                                                 outs.ctypes.data_as(vpp), rd.data_ptr(),
                                                 dd.data_ptr() if body else None, sp)
        assert rc == 0, rc

    def call_a_split():
        call_a(False)
        rc = lib.vds_ec_sha256_batch_device(objects, ins.ctypes.data_as(vpp), sizes.ctypes.data_as(u64p),
                                            dd.data_ptr(), sp)
        assert rc == 0, rc

    # leg b's arguments, built once: the loops below are the calls alone
    host_in = inp[:total].cpu().numpy()
    size_list = [int(x) for x in sizes]
    body_ptr = [host_in.ctypes.data + int(o) for o in in_off]
    rep0 = [int(outs[o * N]) for o in range(objects)]
    rep_len = [chunk.replica_size(K, s) for s in size_list]
    dig_b = [rd_b.data_ptr() + 32 * N * o for o in range(objects)]
    dd_host = np.zeros((objects, 32), dtype=np.uint8)
    dd_ptr = [dd_host.ctypes.data + 32 * o for o in range(objects)]
    sha_dev, sha_host = old.vds_ec_sha256_device, old.vds_ec_sha256_host

    def call_b(body=True):
        rc = old.vds_ec_encode16_batch_device(K, idp, N, objects, ins.ctypes.data_as(vpp), sizes.ctypes.data_as(u64p),
                                              outs.ctypes.data_as(vpp), 0, sp)
        assert rc == 0, rc
        for o in range(objects):
            rc = sha_dev(rep0[o], rep_len[o], slot, N, dig_b[o], sp)
            assert rc == 0, rc
        if body:
            for o in range(objects):
                sha_host(body_ptr[o], size_list[o], dd_ptr[o])

    L_c = chunk.replica_size(K, 65536)
    Ls_c = (L_c + 255) // 256 * 256
    assert N * objects * Ls_c <= out.numel()
    outs_c = (C.c_void_p * N)(*[out.data_ptr() + i * objects * Ls_c for i in range(N)])

    def call_c():
        rc = old.vds_ec_encode16_device(K, idp, N, inp.data_ptr(), 65536, 65536, objects, outs_c, Ls_c, 0, sp)
        assert rc == 0, rc
        rc = old.vds_ec_sha256_device(out.data_ptr(), L_c, Ls_c, N * objects, rd_b.data_ptr(), sp)
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

    def run(leg, fn, nbytes, warm, timed_calls, alone_calls):
        for _ in range(warm):
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
              "parent_lib": bool(args.parent_lib)})
        a = run("a", call_a, total, 5, calls, calls)
        an = run("a_nobody", lambda: call_a(False), total, 5, calls, calls)
        asp = run("a_split", call_a_split, total, 5, calls, calls)
        bn = run("b_nobody", lambda: call_b(False), total, 2, calls, args.loop_calls)
        b = run("b", call_b, total, 1, calls, args.loop_calls)
        # (for b the body hashes run on the caller's thread inside the timed loop: its stream span is the
        # caller's time; "device alone" has no meaning for them)
        c = run("c", call_c, objects * 65536, 5, calls, calls)
        # the two routes agree on every name and body hash
        call_a()
        call_b()
        torch.cuda.synchronize(dev)
        same = bool(torch.equal(rd, rd_b)) and bool(np.array_equal(dd.cpu().numpy().reshape(objects, 32), dd_host))
        emit({"digests_equal_a_b": same})
        assert same
    s_med = lambda r: r["stream_ms_per_call"]["median"]
    d_med = lambda r: r["device_ms_per_call"]["median"]
    emit({"summary": {"a_stream_ms": s_med(a), "a_device_ms": d_med(a), "a_nobody_stream_ms": s_med(an),
                      "a_nobody_device_ms": d_med(an), "a_split_stream_ms": s_med(asp),
                      "a_split_device_ms": d_med(asp), "b_stream_ms": s_med(b), "b_nobody_stream_ms": s_med(bn),
                      "b_nobody_device_ms": d_med(bn), "c_stream_ms": s_med(c), "c_device_ms": d_med(c),
                      "b_over_a_stream_with_bodies": round(s_med(b) / s_med(a), 2),
                      "b_over_a_stream_names_only": round(s_med(bn) / s_med(an), 2),
                      "a_over_c_device_time": round(d_med(a) / d_med(c), 3),
                      "a_nobody_over_c_device_time": round(d_med(an) / d_med(c), 3),
                      "a_host_enqueue_ms_median": a["host_enqueue_ms_per_call"]["median"],
                      "a_bound": a["bound"], "a_nobody_bound": an["bound"]}})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(log) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
