#!/usr/bin/env python3
"""Measure the batched RSA signature check (vds_ec_rsa_verify_digest_batch_device,
vds_ec_rsa_verify_sha256_batch_device) beside one host thread
(vds_ec_rsa_verify_sha256_host and, where the machine's libcrypto loads through
ctypes, EVP_DigestVerify on the same inputs), all in the same run.
(Not bench.py: that one stays the project's yardstick.  No rate here is a pass
bar: the numbers are recorded beside what they were measured against.)

Shapes: --counts signatures (default 1,024 and 16,384) x --bits (4096, 2048) x
--keys (1, 64).  The inputs are 64 different (key, message, signature) triples
laid out `count` times in device memory, each copy at its own address.  Key 0
is the key of that size in tests/golden/rsa_pkcs1_kats.json and its triples are
the fixture's good signatures, which verify; keys 1..63 are random odd moduli
of the size under e = 65537 with random values for signatures, which do not --
a check costs the same either way (nothing ends early), and no signing key is
needed.  The digest form and the SHA form are timed apart.

Every shape runs in a child process of its own under --step-timeout seconds;
the first shape that fails or runs out of time ends the run with its status.
Per device arm: --calls timed calls behind one warm-up, device time from
events round each call; the median and the spread are reported.  After the
timed calls the device's verdicts are compared with the host form's for the 64
triples.  Host arms run over the first --host-sigs items, once.

Prints one JSON line per arm; --out appends them to a file.
"""
from __future__ import annotations

import argparse
import ctypes as C
import ctypes.util
import hashlib
import json
import os
import random
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
UNIQUE = 64
MSG_LEN = 256  # a record of the log, for the triples that are not the fixture's


def _stats(ms: list) -> dict:
    s = sorted(ms)
    return {"ms_median": round(s[len(s) // 2], 4), "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4)}


def _der(tag: int, body: bytes) -> bytes:
    n = len(body)
    head = bytes([n]) if n < 128 else bytes([0x80 | ((n.bit_length() + 7) // 8)]) + n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([tag]) + head + body


def _der_int(v: int) -> bytes:
    return _der(2, v.to_bytes(v.bit_length() // 8 + 1, "big"))


def spki(n: int, e: int) -> bytes:
    """SubjectPublicKeyInfo of an RSA key (RFC 8017 A.1.1 inside RFC 5280 4.1.2.7), for d2i_PUBKEY"""
    alg = _der(0x30, bytes.fromhex("06092a864886f70d0101010500"))
    return _der(0x30, alg + _der(3, b"\x00" + _der(0x30, _der_int(n) + _der_int(e))))


class Libcrypto:
    """EVP_DigestVerify(SHA-256) through ctypes, as the reference calls it; None where libcrypto does not load"""

    @staticmethod
    def load():
        try:
            lib = C.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
            for name, res, args in (("d2i_PUBKEY", C.c_void_p, [C.c_void_p, C.POINTER(C.c_char_p), C.c_long]),
                                    ("EVP_MD_CTX_new", C.c_void_p, []), ("EVP_MD_CTX_free", None, [C.c_void_p]),
                                    ("EVP_sha256", C.c_void_p, []),
                                    ("EVP_DigestVerifyInit", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                                       C.c_void_p]),
                                    ("EVP_DigestVerify", C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p,
                                                                   C.c_size_t]),
                                    ("ERR_clear_error", None, [])):
                f = getattr(lib, name)
                f.restype, f.argtypes = res, args
            return Libcrypto(lib)
        except (OSError, AttributeError):
            return None

    def __init__(self, lib):
        self.lib = lib

    def key(self, n: int, e: int):
        der = spki(n, e)
        p = C.c_char_p(der)
        k = self.lib.d2i_PUBKEY(None, C.byref(p), len(der))
        if not k:
            raise RuntimeError("d2i_PUBKEY refused the key")
        return k

    def verify(self, pkey, msg: bytes, sig: bytes) -> int:
        ctx = self.lib.EVP_MD_CTX_new()
        ok = self.lib.EVP_DigestVerifyInit(ctx, None, self.lib.EVP_sha256(), None, pkey) == 1
        r = self.lib.EVP_DigestVerify(ctx, sig, len(sig), msg, len(msg)) if ok else -1
        self.lib.ERR_clear_error()
        self.lib.EVP_MD_CTX_free(ctx)
        return 1 if r == 1 else 0


def triples(bits: int, nkeys: int) -> tuple:
    """-> ([(n, e)] of nkeys keys, UNIQUE x (key index, message, signature))"""
    import rsa_cases as R
    f = R.kats()
    k0 = next(i for i, k in enumerate(f["keys"]) if k["bits"] == bits)
    good = [c for c in f["cases"] if c["key"] == k0 and c["verdict"] == 1 and c["len"] <= 4099]
    keys = [(f["keys"][k0]["n"], f["keys"][k0]["e"])]
    r = random.Random(bits)
    while len(keys) < nkeys:
        keys.append((r.getrandbits(bits) | (1 << (bits - 1)) | 1, 65537))
    out = []
    for u in range(UNIQUE):
        ki = u % nkeys
        if ki == 0:
            c = good[(u // nkeys) % len(good)]
            out.append((0, c["msg"], c["sig"]))
        else:
            out.append((ki, bytes(r.getrandbits(8) for _ in range(MSG_LEN)), r.randrange(keys[ki][0]).to_bytes(bits // 8, "big")))
    return keys, out


def worker(count: int, bits: int, nkeys: int, calls: int, host_sigs: int) -> int:
    import torch
    from vds_amd import _lib, build, chunk
    build.build()
    if not torch.cuda.is_available():
        print("bench_rsa_verify_batch: no GPU: nothing is measured", file=sys.stderr)
        return 2
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    pub, uniq = triples(bits, nkeys)
    keys = [chunk.rsa_key_prepare(n, e) for n, e in pub]
    ka = (_lib.RsaKey * nkeys)(*keys)
    want = [int(chunk.rsa_verify_sha256_host(keys[ki], m, s)) for ki, m, s in uniq]
    mpitch = (max(len(m) for _, m, _ in uniq) + 15) // 16 * 16
    spitch = bits // 8
    reps = (count + UNIQUE - 1) // UNIQUE
    ma, sa = np.zeros((UNIQUE, mpitch), dtype=np.uint8), np.zeros((UNIQUE, spitch), dtype=np.uint8)
    for i, (_, m, s) in enumerate(uniq):
        ma[i, :len(m)] = np.frombuffer(m, dtype=np.uint8)
        sa[i] = np.frombuffer(s, dtype=np.uint8)
    msgs = torch.from_numpy(ma).to(dev).repeat(reps, 1)[:count].contiguous()
    sigs = torch.from_numpy(sa).to(dev).repeat(reps, 1)[:count].contiguous()
    da = np.frombuffer(b"".join(hashlib.sha256(m).digest() for _, m, _ in uniq), dtype=np.uint8).reshape(UNIQUE, 32)
    digests = torch.from_numpy(da.copy()).to(dev).repeat(reps, 1)[:count].contiguous()
    verdicts = torch.zeros(count, dtype=torch.uint8, device=dev)
    idx = np.arange(count, dtype=np.uint64)
    mp = np.ascontiguousarray(np.uint64(msgs.data_ptr()) + idx * np.uint64(mpitch))
    sp = np.ascontiguousarray(np.uint64(sigs.data_ptr()) + idx * np.uint64(spitch))
    ml = np.asarray([len(uniq[o % UNIQUE][1]) for o in range(count)], dtype=np.uint64)
    sl = np.full(count, spitch, dtype=np.uint64)
    ki = np.asarray([uniq[o % UNIQUE][0] for o in range(count)], dtype=np.uint32)
    vpp, u64p, u32p = _lib.vpp, _lib.u64p, _lib.u32p
    arms = {
        "verify_digest": lambda: lib.vds_ec_rsa_verify_digest_batch_device(
            count, digests.data_ptr(), sp.ctypes.data_as(vpp), sl.ctypes.data_as(u64p), ki.ctypes.data_as(u32p), ka,
            nkeys, verdicts.data_ptr(), None),
        "verify_sha256": lambda: lib.vds_ec_rsa_verify_sha256_batch_device(
            count, mp.ctypes.data_as(vpp), ml.ctypes.data_as(u64p), sp.ctypes.data_as(vpp), sl.ctypes.data_as(u64p),
            ki.ctypes.data_as(u32p), ka, nkeys, verdicts.data_ptr(), None, None),
    }
    shape = {"bits": bits, "keys": nkeys, "count": count}
    lines = []
    for name, call in arms.items():
        ms, host_ms = [], []
        for it in range(calls + 1):
            verdicts.fill_(7)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            rc = call()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            if rc:
                print(f"bench_rsa_verify_batch: {name} returned {rc}", file=sys.stderr)
                return 1
            if it:  # (the first call warms up: code load, ring slot, scratch)
                ms.append(e0.elapsed_time(e1))
                host_ms.append(1e3 * (t1 - t0))
        got = verdicts.cpu().numpy().tolist()
        if got != [want[o % UNIQUE] for o in range(count)]:
            print(f"bench_rsa_verify_batch: {name} differs from vds_ec_rsa_verify_sha256_host", file=sys.stderr)
            return 1
        st = _stats(ms)
        lines.append({"arm": name, "where": "device", **shape, "calls": calls, "verify": sum(got), **st,
                      "host_enqueue_ms_median": round(sorted(host_ms)[len(host_ms) // 2], 4),
                      "per_second": round(count / st["ms_median"] * 1e3)})

    # one host thread over the first items: the library's host form, then libcrypto on the same inputs
    hs = min(count, host_sigs)
    items = [uniq[o % UNIQUE] for o in range(hs)]
    t0 = time.perf_counter()
    ours = [int(chunk.rsa_verify_sha256_host(keys[k], m, s)) for k, m, s in items]
    dt = time.perf_counter() - t0
    lines.append({"arm": "verify_sha256", "where": "host, one thread, vds_ec_rsa_verify_sha256_host", **shape,
                  "count": hs, "verify": sum(ours), "ms": round(1e3 * dt, 3), "per_second": round(hs / dt)})
    lc = Libcrypto.load()
    if lc is None:
        lines.append({"arm": "verify_sha256", "where": "host, one thread, EVP_DigestVerify", **shape, "count": 0,
                      "note": "libcrypto could not be loaded through ctypes: not measured"})
    else:
        pk = [lc.key(n, e) for n, e in pub]
        t0 = time.perf_counter()
        theirs = [lc.verify(pk[k], m, s) for k, m, s in items]
        dt = time.perf_counter() - t0
        if theirs != ours:
            print("bench_rsa_verify_batch: vds_ec_rsa_verify_sha256_host differs from EVP_DigestVerify", file=sys.stderr)
            return 1
        lines.append({"arm": "verify_sha256", "where": "host, one thread, EVP_DigestVerify (ctypes)", **shape,
                      "count": hs, "verify": sum(theirs), "ms": round(1e3 * dt, 3), "per_second": round(hs / dt)})
    for ln in lines:
        print(json.dumps(ln), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--bits", type=int, nargs="+", default=[4096, 2048], choices=[4096, 2048])
    ap.add_argument("--keys", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--calls", type=int, default=5, help="timed calls per arm")
    ap.add_argument("--host-sigs", type=int, default=256)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds a shape's child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(int(args.worker[0]), int(args.worker[1]), int(args.worker[2]), args.calls, args.host_sigs)
    for count in args.counts:
        for bits in args.bits:
            for nkeys in args.keys:
                if not 1 <= nkeys <= UNIQUE:
                    print("bench_rsa_verify_batch: --keys takes 1..64", file=sys.stderr)
                    return 2
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(count), str(bits), str(nkeys),
                       "--calls", str(args.calls), "--host-sigs", str(args.host_sigs)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
                except subprocess.TimeoutExpired:
                    print(f"bench_rsa_verify_batch: {count} x {bits} bits x {nkeys} keys ran past "
                          f"{args.step_timeout} s: stopping", file=sys.stderr)
                    return 124
                sys.stdout.write(r.stdout)
                sys.stdout.flush()
                if args.out and r.stdout:
                    with open(args.out, "a") as f:
                        f.write(r.stdout)
                if r.returncode:
                    sys.stderr.write(r.stderr[-4000:])
                    print(f"bench_rsa_verify_batch: {count} x {bits} bits x {nkeys} keys failed with status "
                          f"{r.returncode}: stopping", file=sys.stderr)
                    return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
