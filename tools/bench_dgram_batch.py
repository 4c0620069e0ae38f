#!/usr/bin/env python3
"""Measure the node-to-node datagram layer on the device (vds_ec_dgram_seal_batch_device,
vds_ec_dgram_open_batch_device) beside the replica naming it follows
(vds_ec_sha256_batch_device over the same replicas), and the two host forms
beside one thread calling OpenSSL's HMAC per datagram (Python's hmac.digest).
(Not bench.py: that one stays the project's yardstick.)

Workload: the live shape, --objects x --replicas replicas of 2050 bytes (k = 32,
64 KiB objects), each inside a sync_replica_data message of 2154 bytes
(object_id, length prefix, replica, owner, value_id, BE16(replica)) in a
16-byte aligned slot of a device slab; direct route, one session key a
hundred messages, consecutive datagram indices per session.

Arms (per --mtu):
  H   vds_ec_sha256_batch_device over the replicas (33 compressions each);
  S   vds_ec_dgram_seal_batch_device: every datagram cut, headed and signed;
  O   vds_ec_dgram_open_batch_device: every datagram of S verified and its
      payload copied into a second message slab (by the whole wave);
  L   the same with each lane copying its own payload (VDS_EC_DGRAM_COPY=lane).
Per call: device time (events round the enqueued work, the call alone behind a
spin kernel that covers its host work), host enqueue time, and wall time until
the host holds the result it needs (O: the verdict bytes).

--order is a string of rounds, e.g. HSOLLOSH: each letter is one round of --calls
timed calls of that arm, all in this process, so the arms interleave and each
arm's own rounds show the run-to-run spread it is compared within.
--host-messages M (0: skip) then times vds_ec_dgram_seal_host_batch and
vds_ec_dgram_open_host_batch over the first M messages from pageable host
memory, and hmac.digest in a loop over the datagrams of the first
--cpu-messages of them.

Prints one JSON line per round and a summary line; --out appends them to a file.
"""
from __future__ import annotations

import argparse
import ctypes as C
import hmac
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPLICA, HEAD, MSG, SLOT = 2050, 36, 2154, 2160
SEED = 0x6467726D


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=16384)
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--mtu", type=int, nargs="+", default=[508, 1400])
    ap.add_argument("--order", default="HSOLLOSH")
    ap.add_argument("--calls", type=int, default=5, help="timed calls per round")
    ap.add_argument("--host-messages", type=int, default=65536)
    ap.add_argument("--cpu-messages", type=int, default=8192)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from vds_amd import _lib, build, chunk
    build.build()
    if not torch.cuda.is_available():
        print("bench_dgram_batch: no GPU: nothing is measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    vpp, u64p, u32p = _lib.vpp, _lib.u64p, _lib.u32p
    nmsg = args.objects * args.replicas
    nses = (nmsg + 99) // 100
    keys = np.random.default_rng(SEED).integers(0, 256, 32 * nses, dtype=np.uint8)
    ses = (np.arange(nmsg, dtype=np.uint32) // 100).astype(np.uint32)
    slab = torch.empty(nmsg * SLOT, dtype=torch.uint8, device=dev)
    chunk.fill_splitmix_device(slab, nmsg * SLOT, SEED)
    recv = torch.zeros(nmsg * SLOT, dtype=torch.uint8, device=dev)
    mp = (np.uint64(slab.data_ptr()) + np.arange(nmsg, dtype=np.uint64) * np.uint64(SLOT)).astype(np.uint64)
    rp_ = (mp + np.uint64(HEAD)).astype(np.uint64)
    mlen = np.full(nmsg, MSG, dtype=np.uint64)
    rlen = np.full(nmsg, REPLICA, dtype=np.uint64)
    types = np.full(nmsg, 0x11, dtype=np.uint8)
    zeros32 = np.zeros(nmsg, dtype=np.uint32)
    names = torch.zeros(nmsg * 32, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream
    log = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.append(line)

    def ok(rc):
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

    emit({"workload": {"messages": nmsg, "message_bytes": MSG, "replica_bytes": REPLICA, "slot": SLOT,
                       "sessions": nses, "route": "direct", "order": args.order, "mtus": args.mtu}})
    summary = {}
    stream.synchronize()
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        for mtu in args.mtu:
            cnt, c0, last = chunk.dgram_layout(mtu, 0, MSG)
            pitch = (mtu + 3) // 4 * 4
            per = mtu - 37
            ndg = nmsg * cnt
            mtus = np.full(nmsg, mtu, dtype=np.uint32)
            i0 = ((np.arange(nmsg, dtype=np.uint64) % 100) * cnt).astype(np.uint32)
            out = torch.zeros(ndg * pitch, dtype=torch.uint8, device=dev)
            op = (np.uint64(out.data_ptr()) +
                  np.arange(nmsg, dtype=np.uint64) * np.uint64(cnt * pitch)).astype(np.uint64)
            # the receiver's view: every datagram, its length, header and destination
            d = np.arange(ndg, dtype=np.uint64)
            dmsg, dnum = d // cnt, d % cnt
            dp = (np.uint64(out.data_ptr()) + d * np.uint64(pitch)).astype(np.uint64)
            dlen = np.where(dnum == cnt - 1, last, mtu).astype(np.uint32)
            dhdr = np.where(dnum == 0, 5 if cnt == 1 else 9, 5).astype(np.uint32)
            doff = np.where(dnum == 0, 0, c0 + (dnum.astype(np.int64) - 1) * per).astype(np.uint64)
            dst = (np.uint64(recv.data_ptr()) + dmsg * np.uint64(SLOT) + doff).astype(np.uint64)
            dses = ses[dmsg.astype(np.int64)]
            ver = torch.full((ndg,), 0x5A, dtype=torch.uint8, device=dev)
            ver_host = torch.empty(ndg, dtype=torch.uint8).pin_memory()

            def enq_h():
                ok(lib.vds_ec_sha256_batch_device(nmsg, rp_.ctypes.data_as(vpp), rlen.ctypes.data_as(u64p),
                                                  names.data_ptr(), sp))

            def enq_s():
                ok(lib.vds_ec_dgram_seal_batch_device(nmsg, mp.ctypes.data_as(vpp), mlen.ctypes.data_as(u64p),
                                                      types.ctypes.data, i0.ctypes.data_as(u32p), None,
                                                      zeros32.ctypes.data_as(u32p), ses.ctypes.data_as(u32p),
                                                      keys.ctypes.data, mtus.ctypes.data_as(u32p), nses,
                                                      op.ctypes.data_as(vpp), pitch, sp))

            def enq_o():
                ok(lib.vds_ec_dgram_open_batch_device(ndg, dp.ctypes.data_as(vpp), dlen.ctypes.data_as(u32p),
                                                      dhdr.ctypes.data_as(u32p), dses.ctypes.data_as(u32p),
                                                      keys.ctypes.data, nses, dst.ctypes.data_as(vpp), ver.data_ptr(),
                                                      sp))

            def fin_sync():
                stream.synchronize()
                return 0

            def fin_o():
                ver_host.copy_(ver, non_blocking=True)
                stream.synchronize()
                return int(np.count_nonzero(ver_host.numpy()))

            def enq_l():  # the open with the one-lane-per-datagram copy (the A/B arm)
                os.environ["VDS_EC_DGRAM_COPY"] = "lane"
                try:
                    enq_o()
                finally:
                    del os.environ["VDS_EC_DGRAM_COPY"]

            arms = {"H": (enq_h, fin_sync, 33 * nmsg), "S": (enq_s, fin_sync, None), "O": (enq_o, fin_o, None),
                    "L": (enq_l, fin_o, None)}
            # compressions a call does: per datagram of n signed bytes (n + 8) // 64 + 1 inner and 1 outer
            comp = nmsg * sum(((mtu if j < cnt - 1 else last) - 32 + 8) // 64 + 2 for j in range(cnt))
            enq_s()  # (the open arm needs sealed datagrams whatever the order)
            stream.synchronize()

            def one_round(arm, idx):
                enqueue, finish, ncomp = arms[arm]
                ncomp = ncomp or comp
                device, wall, host = [], [], []
                for i in range(args.calls + 1):  # (the first call of a round is its warm-up)
                    torch.cuda._sleep(spin_cycles(2 * (max(host) if host else 400.0) + 2.0))
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    h0 = time.perf_counter()
                    enqueue()
                    host.append((time.perf_counter() - h0) * 1e3)
                    b.record(stream)
                    assert finish() == 0, arm
                    if i:
                        device.append(a.elapsed_time(b))
                    w0 = time.perf_counter()
                    enqueue()
                    assert finish() == 0
                    if i:
                        wall.append((time.perf_counter() - w0) * 1e3)
                med = float(np.median(device))
                rec = {"round": idx, "arm": arm, "mtu": mtu, "messages": nmsg, "datagrams": ndg if arm != "H" else None,
                       "calls": args.calls,
                       "device_ms": {"median": round(med, 4), "min": round(min(device), 4),
                                     "max": round(max(device), 4)},
                       "wall_ms": {"median": round(float(np.median(wall)), 4), "min": round(min(wall), 4)},
                       "host_enqueue_ms_median": round(float(np.median(host[1:])), 4),
                       "compressions": ncomp, "ns_per_compression_device": round(med * 1e6 / ncomp, 4)}
                emit(rec)
                return rec

            recs = [one_round(a, i) for i, a in enumerate(args.order)]
            # the opened messages are the sealed ones
            h = min(nmsg, 4096) if set(args.order) & set("OL") else 0
            assert torch.equal(recv.view(nmsg, SLOT)[:h, :MSG], slab.view(nmsg, SLOT)[:h, :MSG]), \
                "open != sealed messages"
            for arm in "HSOL":
                meds = [r["device_ms"]["median"] for r in recs if r["arm"] == arm]
                if meds:
                    summary[f"{arm}@{mtu}"] = {"device_ms_median_of_rounds": round(float(np.median(meds)), 4),
                                               "rounds": meds,
                                               "compressions": [r["compressions"] for r in recs if r["arm"] == arm][0]}

            if args.host_messages:
                hm = min(args.host_messages, nmsg)
                hslab = slab[:hm * SLOT].cpu().numpy()
                hmp = (np.uint64(hslab.ctypes.data) +
                       np.arange(hm, dtype=np.uint64) * np.uint64(SLOT)).astype(np.uint64)
                need = hm * ((cnt - 1) * mtu + last)
                sealed = np.zeros(need, dtype=np.uint8)
                offs = np.zeros(hm, dtype=np.uint64)
                cnts = np.zeros(hm, dtype=np.uint32)
                lasts = np.zeros(hm, dtype=np.uint32)
                t_seal, t_open = [], []
                for _ in range(4):  # (the first call sizes the staging)
                    t0 = time.perf_counter()
                    ok(lib.vds_ec_dgram_seal_host_batch(hm, hmp.ctypes.data_as(vpp), mlen.ctypes.data_as(u64p),
                                                        types.ctypes.data, i0.ctypes.data_as(u32p), None,
                                                        zeros32.ctypes.data_as(u32p), ses.ctypes.data_as(u32p),
                                                        keys.ctypes.data, mtus.ctypes.data_as(u32p), nses,
                                                        sealed.ctypes.data, need, offs.ctypes.data_as(u64p),
                                                        cnts.ctypes.data_as(u32p), lasts.ctypes.data_as(u32p)))
                    t_seal.append((time.perf_counter() - t0) * 1e3)
                hd = np.arange(hm * cnt, dtype=np.uint64)
                hdp = (np.uint64(sealed.ctypes.data) + offs[(hd // cnt).astype(np.int64)] +
                       (hd % cnt) * np.uint64(mtu)).astype(np.uint64)
                hdl = np.where(hd % cnt == cnt - 1, last, mtu).astype(np.uint32)
                hds = ses[(hd // cnt).astype(np.int64)]
                hv = np.zeros(hm * cnt, dtype=np.uint8)
                hout = np.zeros(int(hdl.sum()), dtype=np.uint8)
                found = (_lib.DgramMessage * (hm * cnt))()
                nf = C.c_uint32(0)
                for _ in range(4):
                    t0 = time.perf_counter()
                    ok(lib.vds_ec_dgram_open_host_batch(hm * cnt, hdp.ctypes.data_as(vpp), hdl.ctypes.data_as(u32p),
                                                        hds.ctypes.data_as(u32p), keys.ctypes.data, nses,
                                                        hv.ctypes.data, hout.ctypes.data, hout.size, found,
                                                        C.byref(nf)))
                    t_open.append((time.perf_counter() - t0) * 1e3)
                assert nf.value == hm and not hv.any() and all(found[i].status == 0 for i in range(0, hm, 997))
                m0 = found[0]
                assert hout[m0.msg_off:m0.msg_off + m0.msg_len].tobytes() == hslab[:MSG].tobytes()
                # the reference's primitive: one thread, OpenSSL's HMAC per datagram, to sign and again to verify
                cm = min(args.cpu_messages, hm)
                kb = [keys[32 * s:32 * s + 32].tobytes() for s in range(nses)]
                view = memoryview(sealed)
                spans = [(int(offs[o]) + j * mtu, (mtu if j < cnt - 1 else last) - 32, int(ses[o]))
                         for o in range(cm) for j in range(cnt)]
                t0 = time.perf_counter()
                for at, n, s in spans:
                    hmac.digest(kb[s], view[at:at + n], "sha256")
                t_cpu = (time.perf_counter() - t0) * 1e3
                at, n, s = spans[-1]
                assert hmac.digest(kb[s], view[at:at + n], "sha256") == sealed[at + n:at + n + 32].tobytes()
                rec = {"host_form": True, "mtu": mtu, "messages": hm, "datagrams": hm * cnt,
                       "seal_host_batch_ms": {"first": round(t_seal[0], 3), "min_of_rest": round(min(t_seal[1:]), 3)},
                       "open_host_batch_ms": {"first": round(t_open[0], 3), "min_of_rest": round(min(t_open[1:]), 3)},
                       "seal_us_per_datagram": round(min(t_seal[1:]) * 1e3 / (hm * cnt), 4),
                       "open_us_per_datagram": round(min(t_open[1:]) * 1e3 / (hm * cnt), 4),
                       "cpu_hmac_digest_loop": {"messages": cm, "datagrams": len(spans), "ms": round(t_cpu, 3),
                                                "us_per_datagram": round(t_cpu * 1e3 / len(spans), 4)}}
                emit(rec)
                summary[f"host@{mtu}"] = {k: rec[k] for k in ("seal_us_per_datagram", "open_us_per_datagram")}
                summary[f"host@{mtu}"]["cpu_hmac_us_per_datagram"] = rec["cpu_hmac_digest_loop"]["us_per_datagram"]
            del out, ver, ver_host
    emit({"summary": summary})
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(log) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
