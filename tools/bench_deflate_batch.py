#!/usr/bin/env python3
"""Measure the batched deflate and the pack chain built on it
(vds_ec_deflate_batch_device, vds_ec_block_pack_deflate_batch_device) beside one
host thread (zlib.compress at levels 1 and 6, vds_ec_deflate_host), all in the
same run, with the compressed sizes each of them gives.
(Not bench.py: that one stays the project's yardstick.  No rate here is a pass
bar: the numbers are recorded beside what they were measured against.)

Shapes and bodies as tools/bench_block_unpack.py: --counts x --sizes bodies
(default 16,384 and 1,024 bodies of 64 KiB and of 4 KiB), "text" and "splitmix";
64 different bodies of a kind laid out `count` times in device memory, each copy
at its own address.  GBps counts INPUT bytes.  Every line carries the ratios
compressed / input of the library's deflate and of zlib at levels 1 and 6 over
the 64 bodies.

Every shape runs in a child process of its own under --step-timeout seconds;
the first shape that fails or runs out of time ends the run with its status.
Per device arm: --calls timed calls behind one warm-up, device time from
events round each call; the median and the spread are reported.  After the
timed calls the device's streams of the 64 bodies are compared with
vds_ec_deflate_host's.  Host arms run over the first --host-bodies bodies, once.

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_block_unpack import UNIQUE, _stats, splitmix_bodies, text_bodies  # noqa: E402


def worker(count: int, size: int, kind: str, calls: int, host_bodies: int) -> int:
    import torch
    from vds_amd import _lib, build, chunk
    build.build()
    if not torch.cuda.is_available():
        print("bench_deflate_batch: no GPU: nothing is measured", file=sys.stderr)
        return 2
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    uniq = (text_bodies if kind == "text" else splitmix_bodies)(UNIQUE, size)
    ours = [chunk.deflate_host(b) for b in uniq]
    ratios = {"ratio": round(sum(len(z) for z in ours) / (UNIQUE * size), 4),
              "ratio_zlib1": round(sum(len(zlib.compress(b, 1)) for b in uniq) / (UNIQUE * size), 4),
              "ratio_zlib6": round(sum(len(zlib.compress(b, 6)) for b in uniq) / (UNIQUE * size), 4)}
    bound = chunk.deflate_bound(size)
    zpitch = (bound + 15) // 16 * 16
    cpitch = chunk.aes256_cbc_padded_size(bound)
    reps = (count + UNIQUE - 1) // UNIQUE
    a = np.zeros((UNIQUE, size), dtype=np.uint8)
    for i, r in enumerate(uniq):
        a[i] = np.frombuffer(r, dtype=np.uint8)
    data = torch.from_numpy(a).to(dev).repeat(reps, 1)[:count].contiguous()
    zs = torch.zeros(count * zpitch, dtype=torch.uint8, device=dev)
    crypted = torch.zeros(count * cpitch, dtype=torch.uint8, device=dev)
    ids = torch.zeros(count * 32, dtype=torch.uint8, device=dev)
    keys = torch.zeros(count * 32, dtype=torch.uint8, device=dev)
    out_lens = torch.zeros(count, dtype=torch.int32, device=dev)
    idx = np.arange(count, dtype=np.uint64)

    def table(t, pitch):
        return np.ascontiguousarray(np.uint64(t.data_ptr()) + idx * np.uint64(pitch))

    dp, zp, cp = table(data, size), table(zs, zpitch), table(crypted, cpitch)
    ln = np.full(count, size, dtype=np.uint64)
    zc, cc = np.full(count, bound, dtype=np.uint64), np.full(count, cpitch, dtype=np.uint64)
    vpp, u64p = _lib.vpp, _lib.u64p

    def P(x):
        return x.ctypes.data_as(vpp)

    def L(x):
        return x.ctypes.data_as(u64p)

    want_len = np.asarray([len(ours[o % UNIQUE]) for o in range(count)], dtype=np.int64)
    arms = {
        "deflate": lambda: lib.vds_ec_deflate_batch_device(count, P(dp), L(ln), P(zp), L(zc), out_lens.data_ptr(), None),
        "pack_deflate": lambda: lib.vds_ec_block_pack_deflate_batch_device(count, P(dp), L(ln), ids.data_ptr(),
                                                                           keys.data_ptr(), P(cp), L(cc),
                                                                           out_lens.data_ptr(), None),
    }
    lines = []
    for name, call in arms.items():
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
                print(f"bench_deflate_batch: {name} returned {rc}", file=sys.stderr)
                return 1
            if it:  # (the first call warms up: code load, ring slot, scratch)
                ms.append(e0.elapsed_time(e1))
                host_ms.append(1e3 * (t1 - t0))
        got_len = out_lens.cpu().numpy().astype(np.int64)
        if name == "deflate":
            ok = np.array_equal(got_len, want_len)
            got = zs.view(count, zpitch)[-UNIQUE:].cpu().numpy() if count >= UNIQUE else None
            for j in range(UNIQUE if ok and got is not None else 0):
                o = count - UNIQUE + j
                ok = ok and got[j, :len(ours[o % UNIQUE])].tobytes() == ours[o % UNIQUE]
        else:
            ok = np.array_equal(got_len, want_len // 16 * 16 + 16)
        if not ok:
            print(f"bench_deflate_batch: {name} differs from vds_ec_deflate_host", file=sys.stderr)
            return 1
        st = _stats(ms)
        lines.append({"arm": name, "where": "device", "kind": kind, "count": count, "size": size, "calls": calls,
                      **ratios, **st, "host_enqueue_ms_median": round(sorted(host_ms)[len(host_ms) // 2], 4),
                      "GBps": round(count * size / st["ms_median"] / 1e6, 3)})

    # one host thread over the first bodies: zlib at levels 1 and 6, and the library's own deflate
    hb = min(count, host_bodies)
    bodies = [uniq[o % UNIQUE] for o in range(hb)]
    srcs = [np.frombuffer(b, dtype=np.uint8) for b in bodies]
    buf = np.zeros(bound, dtype=np.uint8)
    n = C.c_uint64(0)
    t0 = time.perf_counter()
    for b in bodies:
        zlib.compress(b, 1)
    t1 = time.perf_counter()
    for b in bodies:
        zlib.compress(b, 6)
    t2 = time.perf_counter()
    for s in srcs:
        if lib.vds_ec_deflate_host(s.ctypes.data, s.size, buf.ctypes.data, bound, C.byref(n)):
            print("bench_deflate_batch: vds_ec_deflate_host failed", file=sys.stderr)
            return 1
    t3 = time.perf_counter()
    for where, dt in (("host, one thread, zlib.compress level 1", t1 - t0),
                      ("host, one thread, zlib.compress level 6", t2 - t1),
                      ("host, one thread, vds_ec_deflate_host", t3 - t2)):
        lines.append({"arm": "deflate", "where": where, "kind": kind, "count": hb, "size": size, **ratios,
                      "ms": round(1e3 * dt, 3), "GBps": round(hb * size / dt / 1e9, 3)})
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
                    print(f"bench_deflate_batch: {count} x {size} {kind} ran past {args.step_timeout} s: stopping",
                          file=sys.stderr)
                    return 124
                sys.stdout.write(r.stdout)
                sys.stdout.flush()
                if args.out and r.stdout:
                    with open(args.out, "a") as f:
                        f.write(r.stdout)
                if r.returncode:
                    sys.stderr.write(r.stderr[-4000:])
                    print(f"bench_deflate_batch: {count} x {size} {kind} failed with status {r.returncode}: stopping",
                          file=sys.stderr)
                    return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
