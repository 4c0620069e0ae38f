#!/usr/bin/env python3
"""Measure the batched download call (name check + restore + gated base64
encode in one call, vds_ec_download16_batch_device) in both of its modes
against the three separate calls it replaces, and the host form per object.
(Not bench.py: that one stays the project's yardstick.)

Workload: the live shape, k = 32, n = 64, 16,384 device-resident objects of
64 KiB, replicas in 256-byte aligned slots; every replica lost with
probability --loss, survivors the first k found (restore_async), every object
with at least one lost replica (the witness: its first lost one); names = the
true ones, so every object passes.

Arms:
  T   the three calls of the parent's entry points: vds_ec_sha256_check_batch_device
      over the count*k survivors (check only), vds_ec_restore16_batch_device,
      vds_ec_base64_encode_batch_device (ungated); the host then needs the
      count*k verdict bytes;
  S   vds_ec_download16_batch_device, survivor mode (the same launches plus
      the gate reads); the host needs the count statuses;
  W   vds_ec_download16_batch_device, witness mode (one regenerated replica
      an object hashed instead of k survivors).
Per call: device time (events round the enqueued work, the call alone behind a
spin kernel that covers its host work) and wall time until the host holds the
verdicts or statuses.

--order is a string of rounds, e.g. TSWWST: each letter is one round of
--calls timed calls of that arm, all in this process, so the arms interleave
and each arm's own rounds show the run-to-run spread it is compared within.
--host-objects H (0: skip) then times vds_ec_download16_host_batch over the
first H objects from pageable host memory, both modes.

Prints one JSON line per round and a summary line; --out appends them to a file.
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

K, N, SIZE = 32, 64, 65536
SEED = 0x646F776E


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=16384)
    ap.add_argument("--loss", type=float, default=0.02)
    ap.add_argument("--order", default="TSWWST")
    ap.add_argument("--calls", type=int, default=10, help="timed calls per round")
    ap.add_argument("--host-objects", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from vds_amd import _lib, build, chunk
    build.build()
    if not torch.cuda.is_available():
        print("bench_download_batch: no GPU: nothing is measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    vpp, u64p, u16p = _lib.vpp, _lib.u64p, _lib.u16p
    count = args.objects
    L = chunk.replica_size(K, SIZE)
    Ls = (L + 255) // 256 * 256
    T = (SIZE + 2) // 3 * 4
    Ts = (T + 255) // 256 * 256
    inp = torch.empty(count * SIZE, dtype=torch.uint8, device=dev)
    chunk.fill_splitmix_device(inp, count * SIZE, SEED)
    reps = torch.empty((N, count * Ls), dtype=torch.uint8, device=dev)
    chunk.encode_device(K, list(range(N)), inp, SIZE, SIZE, count, [reps[i].data_ptr() for i in range(N)], Ls)

    rng = np.random.default_rng(SEED + int(args.loss * 1000))
    lost = rng.random((count, N)) < args.loss
    lost[:, :K + 8][(~lost).sum(axis=1) < K] = False  # (every object restorable)
    for o in np.flatnonzero(lost.sum(axis=1) < 1):    # (a lost replica to be the witness)
        lost[o, rng.integers(0, N)] = True
    nodes = np.stack([np.flatnonzero(~lost[o])[:K] for o in range(count)]).astype(np.uint16)
    wids = np.asarray([np.flatnonzero(lost[o])[0] for o in range(count)], dtype=np.uint16)
    base = np.asarray([reps[i].data_ptr() for i in range(N)], dtype=np.uint64)
    obj_off = np.arange(count, dtype=np.uint64) * np.uint64(Ls)
    cp = np.ascontiguousarray(base[nodes] + obj_off[:, None]).astype(np.uint64)
    wit_true = np.ascontiguousarray(base[wids] + obj_off).astype(np.uint64)
    csz = np.full(count, L, dtype=np.uint64)
    pads = np.full(count, SIZE % (2 * K), dtype=np.uint16)
    sizes = np.full(count, SIZE, dtype=np.uint64)
    slens = np.full(count * K, L, dtype=np.uint64)
    objs = torch.zeros(count * SIZE, dtype=torch.uint8, device=dev)
    op = (np.uint64(objs.data_ptr()) + np.arange(count, dtype=np.uint64) * np.uint64(SIZE)).astype(np.uint64)
    texts = {a: torch.zeros(count * Ts, dtype=torch.uint8, device=dev) for a in "TSW"}
    tp = {a: (np.uint64(t.data_ptr()) + np.arange(count, dtype=np.uint64) * np.uint64(Ts)).astype(np.uint64)
          for a, t in texts.items()}
    wout = torch.zeros(count * Ls, dtype=torch.uint8, device=dev)
    wo = (np.uint64(wout.data_ptr()) + obj_off).astype(np.uint64)
    snames = torch.zeros(count * K * 32, dtype=torch.uint8, device=dev)
    wnames = torch.zeros(count * 32, dtype=torch.uint8, device=dev)
    ver = torch.full((count * K,), 0x5A, dtype=torch.uint8, device=dev)
    st = torch.full((count,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ver_host = torch.empty(count * K, dtype=torch.uint8).pin_memory()
    st_host = torch.empty(count, dtype=torch.int32).pin_memory()
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream
    log = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.append(line)

    def ok(rc):
        assert rc == 0, rc

    def enqueue_t():
        ok(lib.vds_ec_sha256_check_batch_device(count * K, cp.ctypes.data_as(vpp), slens.ctypes.data_as(u64p),
                                                snames.data_ptr(), None, ver.data_ptr(), sp))
        ok(lib.vds_ec_restore16_batch_device(K, count, nodes.ctypes.data_as(u16p), cp.ctypes.data_as(vpp),
                                             csz.ctypes.data_as(u64p), pads.ctypes.data_as(u16p),
                                             op.ctypes.data_as(vpp), 0, sp))
        ok(lib.vds_ec_base64_encode_batch_device(count, op.ctypes.data_as(vpp), sizes.ctypes.data_as(u64p),
                                                 tp["T"].ctypes.data_as(vpp), sp))

    def finish_t():
        ver_host.copy_(ver, non_blocking=True)
        stream.synchronize()
        return int(np.count_nonzero(ver_host.numpy()))

    def download(arm):
        wit = arm == "W"
        ok(lib.vds_ec_download16_batch_device(K, count, nodes.ctypes.data_as(u16p), cp.ctypes.data_as(vpp),
                                              csz.ctypes.data_as(u64p), pads.ctypes.data_as(u16p),
                                              None if wit else snames.data_ptr(),
                                              wids.ctypes.data_as(u16p) if wit else None,
                                              wnames.data_ptr() if wit else None,
                                              wo.ctypes.data_as(vpp) if wit else None, op.ctypes.data_as(vpp),
                                              tp[arm].ctypes.data_as(vpp), ver.data_ptr(), st.data_ptr(), sp))

    def finish_st():
        st_host.copy_(st, non_blocking=True)
        stream.synchronize()
        return int(np.count_nonzero(st_host.numpy()))

    arms = {"T": (enqueue_t, finish_t), "S": (lambda: download("S"), finish_st),
            "W": (lambda: download("W"), finish_st)}
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

    def host_form(h):
        """vds_ec_download16_host_batch over the first h objects, both modes: wall time per object."""
        hreps = reps[:, :h * Ls].cpu().numpy()
        hbase = np.asarray([hreps[i].ctypes.data for i in range(N)], dtype=np.uint64)
        hcp = np.ascontiguousarray(hbase[nodes[:h]] + obj_off[:h, None]).astype(np.uint64)
        sn = snames[:h * K * 32].cpu().numpy()
        wn = wnames[:h * 32].cpu().numpy()
        want = texts["T"].cpu().numpy().reshape(count, Ts)[:h, :T]
        out = {}
        for mode in ("survivor", "witness"):
            wit = mode == "witness"
            tbuf = np.zeros((h, Ts), dtype=np.uint8)
            htp = (np.uint64(tbuf.ctypes.data) + np.arange(h, dtype=np.uint64) * np.uint64(Ts)).astype(np.uint64)
            hst = np.zeros(h, dtype=np.int32)
            hsv = np.zeros(h * K, dtype=np.uint8)
            failed = C.c_uint32(0)
            times = []
            for _ in range(4):  # (the first call sizes the staging)
                tl = np.full(h, Ts, dtype=np.uint64)
                t0 = time.perf_counter()
                ok(lib.vds_ec_download16_host_batch(K, h, nodes.ctypes.data_as(u16p), hcp.ctypes.data_as(vpp),
                                                    csz.ctypes.data_as(u64p), sn.ctypes.data,
                                                    wids.ctypes.data_as(u16p) if wit else None,
                                                    wn.ctypes.data if wit else None, htp.ctypes.data_as(vpp),
                                                    tl.ctypes.data_as(u64p), hst.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    hsv.ctypes.data, C.byref(failed)))
                times.append((time.perf_counter() - t0) * 1e3)
            assert failed.value == 0 and (tl == T).all() and np.array_equal(tbuf[:, :T], want), mode
            out[mode] = {"wall_ms_calls": [round(t, 3) for t in times[1:]],
                         "us_per_object": round(float(np.median(times[1:])) * 1e3 / h, 3)}
        emit({"host_form": {"objects": h, "source": "pageable host memory", **out}})

    with torch.cuda.stream(stream):
        # the names: the true replicas hashed where they lie
        ok(lib.vds_ec_sha256_batch_device(count * K, cp.ctypes.data_as(vpp), slens.ctypes.data_as(u64p),
                                          snames.data_ptr(), sp))
        ok(lib.vds_ec_sha256_batch_device(count, wit_true.ctypes.data_as(vpp), csz.ctypes.data_as(u64p),
                                          wnames.data_ptr(), sp))
        stream.synchronize()
        routes = {"syndrome": int((nodes < K + K // 4).all(axis=1).sum())}
        routes["runtime_coefficient"] = count - routes["syndrome"]
        emit({"workload": {"k": K, "n": N, "objects": count, "object_bytes": SIZE, "loss": args.loss,
                           "replica_slot": Ls, "text_slot": Ts, "seed": SEED,
                           "survivor_sets_within_k_plus_k_4": routes, "order": args.order}})
        recs = [one_round(arm, i) for i, arm in enumerate(args.order)]
        # the arms agree: the same texts, the restored objects the bodies
        for arm in "TSW":
            arms[arm][0]()
            assert arms[arm][1]() == 0
        same = bool(torch.equal(texts["T"], texts["S"])) and bool(torch.equal(texts["T"], texts["W"])) and \
            bool(torch.equal(objs, inp))
        emit({"texts_equal_t_s_w_and_objects_restored": same})
        assert same
        if args.host_objects:
            host_form(min(args.host_objects, count))
    med = {arm: [r["device_ms"]["median"] for r in recs if r["arm"] == arm] for arm in "TSW"}
    summary = {"loss": args.loss, "order": args.order}
    for arm in "TSW":
        if med[arm]:
            summary[arm.lower() + "_device_ms_rounds"] = med[arm]
            summary[arm.lower() + "_device_ms"] = round(float(np.median(med[arm])), 4)
    if med["T"]:
        summary["t_spread_ms"] = round(max(med["T"]) - min(med["T"]), 4)
        for arm in "SW":
            if med[arm]:
                summary[arm.lower() + "_minus_t_ms"] = round(float(np.median(med[arm]) - np.median(med["T"])), 4)
    emit({"summary": summary})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(log) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
