#!/usr/bin/env python3
"""Measure the batched inflate and the block unpack chain
(vds_ec_inflate_batch_device, vds_ec_block_unpack_batch_device) beside one host
thread (vds_ec_inflate_host, Python's zlib.decompress) and beside the route the
unpack took before there was a device inflate (chunk.block_unpack_batch:
decrypt on the device, copy back, zlib and hashlib on one thread), all in the
same run.
(Not bench.py: that one stays the project's yardstick.  No rate here is a pass
bar: the numbers are recorded beside what they were measured against.)

Shapes: --counts x --sizes bodies (default 16,384 and 1,024 bodies of 64 KiB
and of 4 KiB) of two kinds.  "text": words of a 4,096-word vocabulary of random
lower-case letters drawn with Zipf frequencies (exponent 1.2), single spaces
between them -- the line reports the deflate ratio it gave; "splitmix": the
splitmix64 stream, which does not compress (zlib level 6 stores it).  64
different bodies of a kind are made and deflated on the host (zlib level 6, as
the web client's pako.deflate) and laid out `count` times in device memory, each
copy at its own address.  The chain's input is what
vds_ec_block_pack_batch_device makes of them.  GBps counts INFLATED bytes.

Every shape runs in a child process of its own under --step-timeout seconds;
the first shape that fails or runs out of time ends the run with its status.
Per device arm: --calls timed calls behind one warm-up, device time from
events round each call; the median and the spread are reported.  Host arms run
over the first --host-bodies bodies, once.

Prints one JSON line per arm; --out appends them to a file.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 0x696E666C
UNIQUE = 64


def text_bodies(n: int, size: int) -> list:
    rng = np.random.default_rng(SEED)
    letters = np.frombuffer(b"etaoinshrdlucmfwypvbgkqjxz", dtype=np.uint8)
    words = [letters[rng.integers(0, 26, rng.integers(2, 11))].tobytes() for _ in range(4096)]
    out = []
    for _ in range(n):
        idx = np.minimum(rng.zipf(1.2, size // 3 + 8), 4096) - 1
        out.append(b" ".join(words[i] for i in idx)[:size])
        assert len(out[-1]) == size
    return out


def splitmix_bodies(n: int, size: int) -> list:
    x = (np.arange(1, n * ((size + 7) // 8) + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
         + np.uint64(SEED))
    z = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = (z ^ (z >> np.uint64(31))).view(np.uint8).reshape(n, -1)
    return [z[i, :size].tobytes() for i in range(n)]


def _stats(ms: list) -> dict:
    s = sorted(ms)
    return {"ms_median": round(s[len(s) // 2], 4), "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4)}


def worker(count: int, size: int, kind: str, calls: int, host_bodies: int) -> int:
    import torch
    from vds_amd import _lib, build, chunk
    build.build()
    if not torch.cuda.is_available():
        print("bench_block_unpack: no GPU: nothing is measured", file=sys.stderr)
        return 2
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    uniq = (text_bodies if kind == "text" else splitmix_bodies)(UNIQUE, size)
    zipped = [zlib.compress(b, 6) for b in uniq]
    ratio = sum(len(z) for z in zipped) / (UNIQUE * size)
    zmax = (max(len(z) for z in zipped) + 15) // 16 * 16
    cpitch = zmax + 16
    reps = (count + UNIQUE - 1) // UNIQUE

    def spread(rows, pitch):  # `count` copies, body o = rows[o % UNIQUE], each at its own address
        a = np.zeros((UNIQUE, pitch), dtype=np.uint8)
        for i, r in enumerate(rows):
            a[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
        return torch.from_numpy(a).to(dev).repeat(reps, 1)[:count].contiguous()

    data, zs = spread(uniq, size), spread(zipped, zmax)
    zl = np.asarray([len(zipped[o % UNIQUE]) for o in range(count)], dtype=np.uint64)
    cl = zl // np.uint64(16) * np.uint64(16) + np.uint64(16)
    crypted = torch.zeros(count * cpitch, dtype=torch.uint8, device=dev)
    out = torch.zeros(count * size, dtype=torch.uint8, device=dev)
    ids = torch.zeros(count * 32, dtype=torch.uint8, device=dev)
    keys = torch.zeros(count * 32, dtype=torch.uint8, device=dev)
    out_lens = torch.zeros(count, dtype=torch.int32, device=dev)
    statuses = torch.zeros(count, dtype=torch.int32, device=dev)
    idx = np.arange(count, dtype=np.uint64)

    def table(t, pitch):
        return np.ascontiguousarray(np.uint64(t.data_ptr()) + idx * np.uint64(pitch))

    dp, zp, cp, op = table(data, size), table(zs, zmax), table(crypted, cpitch), table(out, size)
    ln = np.full(count, size, dtype=np.uint64)
    vpp, u64p = _lib.vpp, _lib.u64p

    def P(a):
        return a.ctypes.data_as(vpp)

    def L(a):
        return a.ctypes.data_as(u64p)

    rc = lib.vds_ec_block_pack_batch_device(count, P(dp), L(ln), P(zp), L(zl), ids.data_ptr(), keys.data_ptr(), P(cp),
                                            None)
    torch.cuda.synchronize()
    if rc:
        print(f"bench_block_unpack: the pack returned {rc}", file=sys.stderr)
        return 1
    arms = {
        "inflate": lambda: lib.vds_ec_inflate_batch_device(count, P(zp), L(zl), P(op), L(ln), out_lens.data_ptr(),
                                                           statuses.data_ptr(), None),
        "unpack": lambda: lib.vds_ec_block_unpack_batch_device(count, P(cp), L(cl), keys.data_ptr(), ids.data_ptr(),
                                                               P(op), L(ln), out_lens.data_ptr(),
                                                               statuses.data_ptr(), None),
    }
    lines = []
    for name, call in arms.items():
        out.zero_()
        ms, host_ms = [], []
        for it in range(calls + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            rc = call()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            if rc:
                print(f"bench_block_unpack: {name} returned {rc}", file=sys.stderr)
                return 1
            if it:  # (the first call warms up: code load, ring slot, scratch)
                ms.append(e0.elapsed_time(e1))
                host_ms.append(1e3 * (t1 - t0))
        if int((statuses != 0).sum()) or int((out_lens != size).sum()) or not torch.equal(out.view(count, size), data):
            print(f"bench_block_unpack: {name} did not give the bodies back", file=sys.stderr)
            return 1
        st = _stats(ms)
        lines.append({"arm": name, "where": "device", "kind": kind, "count": count, "size": size, "calls": calls,
                      "deflate_ratio": round(ratio, 4), **st,
                      "host_enqueue_ms_median": round(sorted(host_ms)[len(host_ms) // 2], 4),
                      "GBps": round(count * size / st["ms_median"] / 1e6, 3)})

    # one host thread over the first bodies: the library's inflate, zlib's, and the route before this one
    hb = min(count, host_bodies)
    hz = [zipped[o % UNIQUE] for o in range(hb)]
    buf = np.zeros(size, dtype=np.uint8)
    n = C.c_uint64(0)
    srcs = [np.frombuffer(z, dtype=np.uint8) for z in hz]
    t0 = time.perf_counter()
    for s in srcs:
        if lib.vds_ec_inflate_host(s.ctypes.data, s.size, buf.ctypes.data, size, C.byref(n)) or n.value != size:
            print("bench_block_unpack: vds_ec_inflate_host failed", file=sys.stderr)
            return 1
    t1 = time.perf_counter()
    for z in hz:
        zlib.decompress(z)
    t2 = time.perf_counter()
    h_ct = crypted.view(count, cpitch)[:hb].cpu().numpy()
    h_keys, h_ids = keys[:32 * hb].cpu().numpy(), ids[:32 * hb].cpu().numpy()
    cts = [h_ct[o, :int(cl[o])].tobytes() for o in range(hb)]
    kk = [h_keys[32 * o:32 * o + 32].tobytes() for o in range(hb)]
    ii = [h_ids[32 * o:32 * o + 32].tobytes() for o in range(hb)]
    chunk.block_unpack_batch(cts[:2], kk[:2], ii[:2])  # (warm-up: staging buffers)
    t3 = time.perf_counter()
    got = chunk.block_unpack_batch(cts, kk, ii)
    t4 = time.perf_counter()
    if got != [uniq[o % UNIQUE] for o in range(hb)]:
        print("bench_block_unpack: block_unpack_batch differs", file=sys.stderr)
        return 1
    for name, where, dt in (("inflate", "host, one thread, vds_ec_inflate_host", t1 - t0),
                            ("inflate", "host, one thread, zlib.decompress", t2 - t1),
                            ("unpack", "chunk.block_unpack_batch: device decrypt, copy back, zlib + hashlib on one thread",
                             t4 - t3)):
        lines.append({"arm": name, "where": where, "kind": kind, "count": hb, "size": size,
                      "deflate_ratio": round(ratio, 4), "ms": round(1e3 * dt, 3),
                      "GBps": round(hb * size / dt / 1e9, 3)})
    for ln_ in lines:
        print(json.dumps(ln_), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", type=int, nargs="+", default=[16384, 1024])
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--kinds", nargs="+", default=["text", "splitmix"], choices=["text", "splitmix"])
    ap.add_argument("--calls", type=int, default=5, help="timed calls per arm")
    ap.add_argument("--host-bodies", type=int, default=256)
    ap.add_argument("--step-timeout", type=int, default=180, help="seconds a shape's child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(int(args.worker[0]), int(args.worker[1]), args.worker[2], args.calls, args.host_bodies)
    for count in args.counts:
        for size in args.sizes:
            for kind in args.kinds:
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(count), str(size), kind, "--calls",
                       str(args.calls), "--host-bodies", str(args.host_bodies)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
                except subprocess.TimeoutExpired:
                    print(f"bench_block_unpack: {count} x {size} {kind} ran past {args.step_timeout} s: stopping",
                          file=sys.stderr)
                    return 124
                sys.stdout.write(r.stdout)
                sys.stdout.flush()
                if args.out and r.stdout:
                    with open(args.out, "a") as f:
                        f.write(r.stdout)
                if r.returncode:
                    sys.stderr.write(r.stderr[-4000:])
                    print(f"bench_block_unpack: {count} x {size} {kind} failed with status {r.returncode}: stopping",
                          file=sys.stderr)
                    return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
