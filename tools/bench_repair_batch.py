#!/usr/bin/env python3
"""Measure the batched repair call (regenerate + names + name check in one
call, vds_ec_repair16_batch_device) against the composition a caller had
before it.  (Not bench.py: that one stays the project's yardstick.)

Workload: the live shape, k = 32, n = 64, 16,384 device-resident objects of
64 KiB, replicas in 256-byte aligned slots; every replica lost with
probability --loss (0.02 and 0.25 are the two rates of interest), survivors
the first k found (restore_async), 2 lost replicas regenerated per object
(objects that lost fewer than 2 lose more), expected names = the true ones.

Arms:
  A   vds_ec_repair16_batch_device with expected names: verdicts on the device;
  B   vds_ec_regenerate16_batch_device, then vds_ec_sha256_batch_device over
      the outputs, then the copy-back of the count*2*32 digest bytes, then a
      host compare with the expected names.
Per call: device time (events round the enqueued work -- B's includes its
digest copy-back --, the call alone behind a spin kernel that covers its host
work) and wall time until the host holds the verdicts (A: plus the copy-back
of its count*2 verdict bytes and a count of the non-zero ones).

--order is a string of rounds, e.g. ABBA: each letter is one round of --calls
timed calls of that arm, all in this process.  Run once per arm order (ABBA,
BAAB) and compare A with B against the spread B's own rounds show.

Prints one JSON line per round and a summary line; --out appends them to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N, SIZE, NT = 32, 64, 65536, 2
SEED = 0x72657061


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=16384)
    ap.add_argument("--loss", type=float, default=0.02)
    ap.add_argument("--order", default="ABBA")
    ap.add_argument("--calls", type=int, default=10, help="timed calls per round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from vds_amd import _lib, build, chunk
    build.build()
    if not torch.cuda.is_available():
        print("bench_repair_batch: no GPU: nothing is measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    vpp, u64p, u16p = _lib.vpp, _lib.u64p, _lib.u16p
    count = args.objects
    L = chunk.replica_size(K, SIZE)
    Ls = (L + 255) // 256 * 256
    inp = torch.empty(count * SIZE, dtype=torch.uint8, device=dev)
    chunk.fill_splitmix_device(inp, count * SIZE, SEED)
    reps = torch.empty((N, count * Ls), dtype=torch.uint8, device=dev)
    chunk.encode_device(K, list(range(N)), inp, SIZE, SIZE, count, [reps[i].data_ptr() for i in range(N)], Ls)
    del inp

    rng = np.random.default_rng(SEED + int(args.loss * 1000))
    lost = rng.random((count, N)) < args.loss
    lost[:, :K + 8][(~lost).sum(axis=1) < K] = False  # (every object restorable)
    for o in np.flatnonzero(lost.sum(axis=1) < NT):   # (at least two replicas to regenerate)
        lost[o, rng.choice(np.flatnonzero(~lost[o]), NT - int(lost[o].sum()), replace=False)] = True
    nodes = np.stack([np.flatnonzero(~lost[o])[:K] for o in range(count)]).astype(np.uint16)
    targets = np.stack([np.flatnonzero(lost[o])[:NT] for o in range(count)]).astype(np.uint16)
    base = np.asarray([reps[i].data_ptr() for i in range(N)], dtype=np.uint64)
    obj_off = np.arange(count, dtype=np.uint64) * np.uint64(Ls)
    cp = np.ascontiguousarray(base[nodes] + obj_off[:, None]).astype(np.uint64)
    true_ptr = np.ascontiguousarray(base[targets] + obj_off[:, None]).astype(np.uint64).reshape(-1)
    csz = np.full(count, L, dtype=np.uint64)
    out = torch.zeros(count * NT * Ls, dtype=torch.uint8, device=dev)
    outs = (np.uint64(out.data_ptr()) + np.arange(count * NT, dtype=np.uint64) * np.uint64(Ls)).astype(np.uint64)
    lens = np.full(count * NT, L, dtype=np.uint64)
    names = count * NT
    expected = torch.zeros(names * 32, dtype=torch.uint8, device=dev)
    dig_a = torch.zeros(names * 32, dtype=torch.uint8, device=dev)
    dig_b = torch.zeros(names * 32, dtype=torch.uint8, device=dev)
    ver = torch.full((names,), 0x5A, dtype=torch.uint8, device=dev)
    dig_host = torch.empty(names * 32, dtype=torch.uint8).pin_memory()
    ver_host = torch.empty(names, dtype=torch.uint8).pin_memory()
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream
    log = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.append(line)

    def ok(rc):
        assert rc == 0, rc

    def enqueue_a():
        ok(lib.vds_ec_repair16_batch_device(K, count, nodes.ctypes.data_as(u16p), cp.ctypes.data_as(vpp),
                                            csz.ctypes.data_as(u64p), NT, targets.ctypes.data_as(u16p),
                                            outs.ctypes.data_as(vpp), dig_a.data_ptr(), expected.data_ptr(),
                                            ver.data_ptr(), sp))

    def finish_a():
        ver_host.copy_(ver, non_blocking=True)
        stream.synchronize()
        return int(np.count_nonzero(ver_host.numpy()))

    def enqueue_b():
        ok(lib.vds_ec_regenerate16_batch_device(K, count, nodes.ctypes.data_as(u16p), cp.ctypes.data_as(vpp),
                                                csz.ctypes.data_as(u64p), NT, targets.ctypes.data_as(u16p),
                                                outs.ctypes.data_as(vpp), sp))
        ok(lib.vds_ec_sha256_batch_device(names, outs.ctypes.data_as(vpp), lens.ctypes.data_as(u64p),
                                          dig_b.data_ptr(), sp))
        dig_host.copy_(dig_b, non_blocking=True)

    def finish_b():
        stream.synchronize()
        got = dig_host.numpy().reshape(names, 32)
        return int(np.count_nonzero((got != expected_host).any(axis=1)))

    arms = {"A": (enqueue_a, finish_a), "B": (enqueue_b, finish_b)}
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

    def one_round(arm, idx):
        enqueue, finish = arms[arm]
        device, wall, host = [], [], []
        for i in range(args.calls + 1):  # (the first call of a round is its warm-up)
            torch.cuda._sleep(spin_cycles(2 * (max(host) if host else 20.0) + 2.0))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            h0 = time.perf_counter()
            enqueue()
            host.append((time.perf_counter() - h0) * 1e3)
            b.record(stream)
            bad = finish()
            assert bad == 0, (arm, bad)
            if i:
                device.append(a.elapsed_time(b))
            w0 = time.perf_counter()
            enqueue()
            assert finish() == 0
            if i:
                wall.append((time.perf_counter() - w0) * 1e3)
        rec = {"round": idx, "arm": arm, "loss": args.loss, "objects": count, "calls": args.calls,
               "device_ms": {"median": round(float(np.median(device)), 4), "min": round(min(device), 4),
                             "max": round(max(device), 4)},
               "wall_ms_to_host_verdicts": {"median": round(float(np.median(wall)), 4), "min": round(min(wall), 4)},
               "host_enqueue_ms_median": round(float(np.median(host[1:])), 4),
               "gib_s_objects_device": round(count * SIZE / (np.median(device) * 1e-3) / 2 ** 30, 2)}
        emit(rec)
        return rec

    with torch.cuda.stream(stream):
        # the expected names: the true replicas hashed where they lie
        ok(lib.vds_ec_sha256_batch_device(names, true_ptr.ctypes.data_as(vpp), lens.ctypes.data_as(u64p),
                                          expected.data_ptr(), sp))
        stream.synchronize()
        expected_host = expected.cpu().numpy().reshape(names, 32).copy()
        routes = {"syndrome": int((nodes < K + K // 4).all(axis=1).sum())}
        routes["runtime_coefficient"] = count - routes["syndrome"]
        emit({"workload": {"k": K, "n": N, "objects": count, "object_bytes": SIZE, "loss": args.loss, "targets": NT,
                           "replica_slot": Ls, "seed": SEED, "survivor_sets_within_k_plus_k_4": routes,
                           "order": args.order}})
        recs = [one_round(arm, i) for i, arm in enumerate(args.order)]
        # the two arms agree: same replicas' names, every verdict 0
        enqueue_a()
        assert finish_a() == 0
        enqueue_b()
        assert finish_b() == 0
        same = bool(torch.equal(dig_a, dig_b)) and bool(torch.equal(dig_a, expected))
        emit({"names_equal_a_b_expected": same})
        assert same
    med = {arm: [r["device_ms"]["median"] for r in recs if r["arm"] == arm] for arm in "AB"}
    summary = {"loss": args.loss, "order": args.order, "a_device_ms_rounds": med["A"], "b_device_ms_rounds": med["B"]}
    if med["A"] and med["B"]:
        summary.update({"a_device_ms": round(float(np.median(med["A"])), 4),
                        "b_device_ms": round(float(np.median(med["B"])), 4),
                        "b_spread_ms": round(max(med["B"]) - min(med["B"]), 4),
                        "a_minus_b_ms": round(float(np.median(med["A"]) - np.median(med["B"])), 4)})
    emit({"summary": summary})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(log) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
