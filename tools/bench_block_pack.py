#!/usr/bin/env python3
"""Measure the batched AES-256-CBC kernels and the block pack chain
(vds_ec_aes256_cbc_encrypt_batch_device, _decrypt_batch_device,
vds_ec_block_pack_batch_device; and the encrypt's one-lane-a-chain A/B arm,
VDS_EC_AES_ENC=lane, as "encrypt_lane") beside the host cipher on one thread
(vds_ec_aes256_cbc_*_host) and, where it loads through ctypes, the system
libcrypto's EVP_aes_256_cbc on one thread, all in the same run.
(Not bench.py: that one stays the project's yardstick.  No rate here is a pass
bar: the numbers are recorded beside what they were measured against.)

Shapes: --counts x --sizes bodies (default 16,384 and 1,024 bodies of 64 KiB
and of 4 KiB), splitmix bytes in one 16-byte aligned slab, per-body keys.  The
pack's "deflated" input is the body itself (the call does not look inside it),
so the pack chain costs two hashes and two encryptions of the body's size: an
upper bound for a real deflate, which shrinks the second encryption.

Every shape runs in a child process of its own under --step-timeout seconds;
the first shape that fails or runs out of time ends the run with its status.
Per arm: --calls timed calls behind one warm-up, device time from events round
each call; the median and the spread are reported.  Host arms run over the
first --host-bodies bodies.

Prints one JSON line per arm; --out appends them to a file.
"""
from __future__ import annotations

import argparse
import ctypes as C
import ctypes.util
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 0x61657362


def _libcrypto():
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = C.CDLL(name)
        lib.EVP_aes_256_cbc.restype = C.c_void_p
        lib.EVP_CIPHER_CTX_new.restype = C.c_void_p
        lib.EVP_CIPHER_CTX_free.argtypes = [C.c_void_p]
        lib.EVP_CipherInit_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        lib.EVP_CipherUpdate.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_int]
        lib.EVP_CipherFinal_ex.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        return lib
    except (OSError, AttributeError):
        return None


def _stats(ms: list) -> dict:
    s = sorted(ms)
    return {"ms_median": round(s[len(s) // 2], 4), "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4)}


def worker(count: int, size: int, calls: int, host_bodies: int) -> int:
    import torch
    from vds_amd import _lib, build, chunk
    build.build()
    if not torch.cuda.is_available():
        print("bench_block_pack: no GPU: nothing is measured", file=sys.stderr)
        return 2
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    padded = size // 16 * 16 + 16
    data = torch.empty(count * size, dtype=torch.uint8, device=dev)
    chunk.fill_splitmix_device(data, count * size, SEED)
    keys = torch.empty(count * 32, dtype=torch.uint8, device=dev)
    chunk.fill_splitmix_device(keys, count * 32, SEED + 1)
    ct = torch.zeros(count * padded, dtype=torch.uint8, device=dev)
    back = torch.zeros(count * padded, dtype=torch.uint8, device=dev)
    ids = torch.zeros(count * 32, dtype=torch.uint8, device=dev)
    pkeys = torch.zeros(count * 32, dtype=torch.uint8, device=dev)
    crypted = torch.zeros(count * padded, dtype=torch.uint8, device=dev)
    out_lens = torch.zeros(count, dtype=torch.int32, device=dev)
    statuses = torch.zeros(count, dtype=torch.int32, device=dev)
    idx = np.arange(count, dtype=np.uint64)

    def table(t, pitch):
        return np.ascontiguousarray(np.uint64(t.data_ptr()) + idx * np.uint64(pitch))

    dp, cp, bp, kp = table(data, size), table(ct, padded), table(back, padded), table(crypted, padded)
    ln = np.full(count, size, dtype=np.uint64)
    cl = np.full(count, padded, dtype=np.uint64)
    vpp, u64p = _lib.vpp, _lib.u64p

    def P(a):
        return a.ctypes.data_as(vpp)

    def L(a):
        return a.ctypes.data_as(u64p)

    def lane_arm():  # the encrypt with one lane a chain (the A/B arm)
        os.environ["VDS_EC_AES_ENC"] = "lane"
        try:
            return arms["encrypt"]()
        finally:
            del os.environ["VDS_EC_AES_ENC"]

    arms = {
        "encrypt": lambda: lib.vds_ec_aes256_cbc_encrypt_batch_device(count, P(dp), L(ln), keys.data_ptr(), None,
                                                                      P(cp), None),
        "decrypt": lambda: lib.vds_ec_aes256_cbc_decrypt_batch_device(count, P(cp), L(cl), keys.data_ptr(), None,
                                                                      P(bp), out_lens.data_ptr(),
                                                                      statuses.data_ptr(), None),
        "pack": lambda: lib.vds_ec_block_pack_batch_device(count, P(dp), L(ln), P(dp), L(ln), ids.data_ptr(),
                                                           pkeys.data_ptr(), P(kp), None),
        "encrypt_lane": lane_arm,
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
                print(f"bench_block_pack: {name} returned {rc}", file=sys.stderr)
                return 1
            if it:  # (the first call warms up: code load, ring slot, scratch)
                ms.append(e0.elapsed_time(e1))
                host_ms.append(1e3 * (t1 - t0))
        st = _stats(ms)
        lines.append({"arm": name, "where": "device", "count": count, "size": size, "calls": calls, **st,
                      "host_enqueue_ms_median": round(sorted(host_ms)[len(host_ms) // 2], 4),
                      "GBps": round(count * size / st["ms_median"] / 1e6, 3)})
    if int((statuses != 0).sum()) or int((out_lens != size).sum()):
        print("bench_block_pack: the decrypt did not give the bodies' lengths back", file=sys.stderr)
        return 1
    if not torch.equal(back.view(count, padded)[:, :size], data.view(count, size)):
        print("bench_block_pack: the round trip differs", file=sys.stderr)
        return 1

    # one host thread over the first bodies: the library's cipher, then libcrypto's
    hb = min(count, host_bodies)
    h_data = data[:hb * size].cpu().numpy()
    h_keys = keys[:hb * 32].cpu().numpy()
    h_ct = np.zeros(hb * padded, dtype=np.uint8)
    h_back = np.zeros(hb * padded, dtype=np.uint8)
    iv = np.frombuffer(chunk.block_iv(), dtype=np.uint8).copy()
    n = C.c_uint64(0)
    t0 = time.perf_counter()
    for o in range(hb):
        lib.vds_ec_aes256_cbc_encrypt_host(h_keys.ctypes.data + 32 * o, iv.ctypes.data, h_data.ctypes.data + size * o,
                                           size, h_ct.ctypes.data + padded * o)
    t1 = time.perf_counter()
    for o in range(hb):
        lib.vds_ec_aes256_cbc_decrypt_host(h_keys.ctypes.data + 32 * o, iv.ctypes.data, h_ct.ctypes.data + padded * o,
                                           padded, h_back.ctypes.data + padded * o, C.byref(n))
    t2 = time.perf_counter()
    if not np.array_equal(h_ct, ct[:hb * padded].cpu().numpy()):
        print("bench_block_pack: device and host ciphertexts differ", file=sys.stderr)
        return 1
    for name, dt in (("encrypt", t1 - t0), ("decrypt", t2 - t1)):
        lines.append({"arm": name, "where": "host, one thread, vds_ec_aes256_cbc_*_host", "count": hb, "size": size,
                      "ms": round(1e3 * dt, 3), "GBps": round(hb * size / dt / 1e9, 3)})
    cr = _libcrypto()
    if cr is None:
        lines.append({"arm": "libcrypto", "where": "host", "note": "libcrypto did not load through ctypes"})
    else:
        for enc in (1, 0):
            src, dst, sl = (h_data, h_back, size) if enc else (h_ct, h_back, padded)
            m = C.c_int(0)
            t0 = time.perf_counter()
            for o in range(hb):
                ctx = cr.EVP_CIPHER_CTX_new()
                cr.EVP_CipherInit_ex(ctx, cr.EVP_aes_256_cbc(), None, h_keys.ctypes.data + 32 * o, iv.ctypes.data, enc)
                cr.EVP_CipherUpdate(ctx, dst.ctypes.data + padded * o, C.byref(m), src.ctypes.data + sl * o, sl)
                cr.EVP_CipherFinal_ex(ctx, dst.ctypes.data + padded * o + m.value, C.byref(m))
                cr.EVP_CIPHER_CTX_free(ctx)
            dt = time.perf_counter() - t0
            lines.append({"arm": "encrypt" if enc else "decrypt", "where": "host, one thread, libcrypto EVP_aes_256_cbc",
                          "count": hb, "size": size, "ms": round(1e3 * dt, 3), "GBps": round(hb * size / dt / 1e9, 3)})
    for ln_ in lines:
        print(json.dumps(ln_), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", type=int, nargs="+", default=[16384, 1024])
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--calls", type=int, default=5, help="timed calls per arm")
    ap.add_argument("--host-bodies", type=int, default=256)
    ap.add_argument("--step-timeout", type=int, default=180, help="seconds a shape's child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1], args.calls, args.host_bodies)
    for count in args.counts:
        for size in args.sizes:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(count), str(size), "--calls",
                   str(args.calls), "--host-bodies", str(args.host_bodies)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                print(f"bench_block_pack: {count} x {size} ran past {args.step_timeout} s: stopping", file=sys.stderr)
                return 124
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if args.out and r.stdout:
                with open(args.out, "a") as f:
                    f.write(r.stdout)
            if r.returncode:
                sys.stderr.write(r.stderr[-4000:])
                print(f"bench_block_pack: {count} x {size} failed with status {r.returncode}: stopping",
                      file=sys.stderr)
                return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
