#!/usr/bin/env python3
"""Measure the websocket layer (vds_ec_ws_*) on the live shape.  (Not bench.py:
that one stays the project's yardstick.)

Workload, as tools/bench_upload_batch.py: k = 32, n = 64, --objects frames
(16,384) whose bodies are 64 KiB, each the masked text frame the web client
sends, {"id":N,"invoke":"upload","params":["<base64>"]} under a random mask.

Device legs (each call alone behind a spin kernel that covers its host work:
device time, HIP events; interleaved A B B A):
  decode         vds_ec_base64_decode_batch_device over the UNMASKED texts
                 (the kernel as it was before the mask existed);
  decode_masked  vds_ec_base64_decode_masked_batch_device over the same texts
                 under their masks, same addresses;
  answer         vds_ec_ws_upload_answer_batch_device: the answer frames from
                 the names and body hashes on the device.
Host legs (wall time of one call on the calling thread, A B B A):
  ws_upload      vds_ec_ws_upload16_host_batch from the frames;
  upload_before  what a careful caller wrote before: a word-wise XOR unmask
                 (numpy over a uint32 view), the recogniser, ONE
                 vds_ec_upload16_host_batch, then vds_ec_upload_response_json
                 and a frame header per message;
  ws_download    vds_ec_ws_download16_host_batch over --dl-objects objects
                 (survivor mode);
  download_before  vds_ec_download16_host_batch, then the frame built round
                 each text (header, prefix, one copy of the text, suffix).
The new form is to be no slower than the path before it by more than the
spread of that path's own legs (reported; exit status 1 otherwise).

Prints one JSON line per leg and a summary line; --out also writes them to a
file.
"""
from __future__ import annotations

import argparse
import base64
import ctypes as C
import hashlib
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, N = 32, 64
SEED = 0x77736273
BODY = 65536


def mm(x):
    return {"median": round(float(np.median(x)), 4), "min": round(float(min(x)), 4), "max": round(float(max(x)), 4)}


def header(payload_len, mask=None):
    mb = 0x80 if mask is not None else 0
    if payload_len < 126:
        h = struct.pack(">BB", 0x81, mb | payload_len)
    elif payload_len <= 0xFFFF:
        h = struct.pack(">BBH", 0x81, mb | 126, payload_len)
    else:
        h = struct.pack(">BBQ", 0x81, mb | 127, payload_len)
    return h + (mask or b"")


def xor_words(payload: bytes, mask: bytes) -> bytes:
    """The word-wise unmask (and mask): numpy over a uint32 view."""
    n = len(payload)
    buf = np.zeros((n + 3) // 4, dtype=np.uint32)
    buf.view(np.uint8)[:n] = np.frombuffer(payload, dtype=np.uint8)
    buf ^= np.frombuffer(mask, dtype=np.uint32)[0]
    return buf.view(np.uint8)[:n].tobytes()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=16384)
    ap.add_argument("--dl-objects", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=6, help="A B B A rounds of the device legs")
    ap.add_argument("--host-rounds", type=int, default=2, help="A B B A rounds of the host legs (after one warm-up)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from vds_amd import _lib, build, chunk
    build.build()
    if not torch.cuda.is_available():
        print("bench_ws_batch: no GPU: nothing is measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    vpp, u64p, i32p, u32p = _lib.vpp, _lib.u64p, _lib.i32p, _lib.u32p
    objects = args.objects
    log = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.append(line)

    # ------------------------------------------------------------ the workload
    rng = np.random.default_rng(SEED)
    inp = torch.empty(objects * BODY, dtype=torch.uint8, device=dev)
    chunk.fill_splitmix_device(inp, inp.numel(), SEED)
    torch.cuda.synchronize(dev)
    host_in = inp.cpu().numpy()
    del inp
    ids = rng.integers(0, 1 << 31, objects, dtype=np.int64).astype(np.int32)
    masks = rng.integers(0, 256, (objects, 4), dtype=np.uint8)
    texts, frames, body_off = [], [], []
    for o in range(objects):
        t = base64.b64encode(host_in[o * BODY:(o + 1) * BODY].tobytes())
        head = b'{"id":%d,"invoke":"upload","params":["' % int(ids[o])
        payload = head + t + b'"]}'
        mk = masks[o].tobytes()
        texts.append(t)
        body_off.append(len(head))
        frames.append(header(len(payload), mk) + xor_words(payload, mk))
    T = len(texts[0])
    L = chunk.replica_size(K, BODY)
    emit({"workload": {"k": K, "n": N, "objects": objects, "body_bytes": BODY, "text_chars": T,
                       "frame_bytes": len(frames[0]), "replica_size": L, "seed": SEED}})

    # ------------------------------------------------------------- device legs
    pitch = (T + 15) // 16 * 16
    host_text = np.zeros(objects * pitch, dtype=np.uint8)
    host_masked = np.zeros(objects * pitch, dtype=np.uint8)
    tmasks = np.zeros((objects, 4), dtype=np.uint8)
    for o in range(objects):
        host_text[o * pitch:o * pitch + T] = np.frombuffer(texts[o], dtype=np.uint8)
        tmasks[o] = np.roll(masks[o], -(body_off[o] & 3))
        host_masked[o * pitch:o * pitch + T] = np.frombuffer(xor_words(texts[o], tmasks[o].tobytes()), dtype=np.uint8)
    d_text = torch.from_numpy(host_text).to(dev)
    d_masked = torch.from_numpy(host_masked).to(dev)
    del host_text, host_masked
    d_body = torch.zeros(objects * BODY, dtype=torch.uint8, device=dev)
    d_st = torch.full((objects,), 77, dtype=torch.int32, device=dev)
    tlens = np.full(objects, T, dtype=np.uint64)
    sizes = np.full(objects, BODY, dtype=np.uint64)
    tp = (d_text.data_ptr() + np.arange(objects, dtype=np.uint64) * np.uint64(pitch)).astype(np.uint64)
    mp = (d_masked.data_ptr() + np.arange(objects, dtype=np.uint64) * np.uint64(pitch)).astype(np.uint64)
    bp = (d_body.data_ptr() + np.arange(objects, dtype=np.uint64) * np.uint64(BODY)).astype(np.uint64)
    rd = torch.from_numpy(rng.integers(0, 256, objects * N * 32, dtype=np.uint8)).to(dev)
    dd = torch.from_numpy(rng.integers(0, 256, objects * 32, dtype=np.uint8)).to(dev)
    a_len = [chunk.ws_upload_answer_size(int(i), N, L)[0] for i in ids]
    a_off = np.concatenate(([0], np.cumsum(a_len)[:-1])).astype(np.uint64)
    d_ans = torch.zeros(int(sum(a_len)), dtype=torch.uint8, device=dev)
    ap_ = (d_ans.data_ptr() + a_off).astype(np.uint64)
    rsz = np.full(objects, L, dtype=np.uint32)
    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream

    def call_decode():
        rc = lib.vds_ec_base64_decode_batch_device(objects, tp.ctypes.data_as(vpp), tlens.ctypes.data_as(u64p),
                                                   bp.ctypes.data_as(vpp), sizes.ctypes.data_as(u64p),
                                                   d_st.data_ptr(), sp)
        assert rc == 0, rc

    def call_decode_masked():
        rc = lib.vds_ec_base64_decode_masked_batch_device(objects, mp.ctypes.data_as(vpp), tlens.ctypes.data_as(u64p),
                                                          tmasks.ctypes.data, bp.ctypes.data_as(vpp),
                                                          sizes.ctypes.data_as(u64p), d_st.data_ptr(), sp)
        assert rc == 0, rc

    def call_answer():
        rc = lib.vds_ec_ws_upload_answer_batch_device(objects, ids.ctypes.data_as(i32p), N, rd.data_ptr(),
                                                      dd.data_ptr(), rsz.ctypes.data_as(u32p),
                                                      ap_.ctypes.data_as(vpp), sp)
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

    legs = {"decode": call_decode, "decode_masked": call_decode_masked, "answer": call_answer}
    ref_body = torch.from_numpy(host_in).to(dev)
    with torch.cuda.stream(stream):
        for name, fn in legs.items():  # warm-up, each call's host time, and its result
            h = []
            for _ in range(3):
                d_body.zero_()
                h0 = time.perf_counter()
                fn()
                h.append((time.perf_counter() - h0) * 1e3)
                torch.cuda.synchronize(dev)
            host_ms[name] = max(h)
            if name != "answer":
                assert int(d_st.abs().max()) == 0, name
                assert torch.equal(d_body, ref_body), name
        t = {name: [] for name in legs}
        for _ in range(max(1, args.rounds)):
            for name in ("decode", "decode_masked", "decode_masked", "decode"):  # A B B A
                t[name].append(alone(name, legs[name]))
            t["answer"].append(alone("answer", call_answer))
        for name in legs:
            emit({"leg": name, "device_ms_per_call": mm(t[name]), "host_enqueue_ms_max": round(host_ms[name], 4),
                  "device_us_per_message": round(float(np.median(t[name])) * 1e3 / objects, 4), "calls": len(t[name])})
    # the first answer against the host serialiser
    js = chunk.upload_response_json(int(ids[0]), [rd[32 * i:32 * i + 32].cpu().numpy().tobytes() for i in range(N)],
                                    dd[:32].cpu().numpy().tobytes(), L).encode()
    assert d_ans[:a_len[0]].cpu().numpy().tobytes() == header(len(js)) + js
    del d_text, d_masked, d_body, ref_body, d_ans, rd, dd
    torch.cuda.empty_cache()

    # ---------------------------------------------------------------- host legs
    h_outs = np.empty((objects * N, L), dtype=np.uint8)
    h_rd = np.empty(objects * N * 32, dtype=np.uint8)
    h_dd = np.empty(objects * 32, dtype=np.uint8)
    h_rs = np.zeros(objects, dtype=np.uint32)
    h_st = np.zeros(objects, dtype=np.int32)
    h_ans = np.zeros(int(sum(a_len)), dtype=np.uint8)
    h_ao = np.zeros(objects, dtype=np.uint64)
    h_al = np.zeros(objects, dtype=np.uint64)
    failed = C.c_uint32(0)
    c_frames = (C.c_char_p * objects)(*frames)
    flens = np.asarray([len(f) for f in frames], dtype=np.uint64)
    c_outs = (h_outs.ctypes.data + np.arange(objects * N, dtype=np.uint64) * np.uint64(L)).astype(np.uint64)

    def host_ws_upload():
        rc = lib.vds_ec_ws_upload16_host_batch(K, N, objects, C.cast(c_frames, vpp), flens.ctypes.data_as(u64p),
                                               c_outs.ctypes.data_as(vpp), h_rd.ctypes.data, h_dd.ctypes.data,
                                               h_rs.ctypes.data_as(u32p), h_ans.ctypes.data, h_ans.size,
                                               h_ao.ctypes.data_as(u64p), h_al.ctypes.data_as(u64p),
                                               h_st.ctypes.data_as(i32p), C.byref(failed))
        assert rc == 0 and failed.value == 0, (rc, failed.value)

    before_ans = [None] * objects
    json_buf = C.create_string_buffer(8192)

    def host_upload_before():
        plain, bodies_at, got_ids = [], [], []
        rid, off, ln, size = C.c_int32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        for o in range(objects):
            f = frames[o]
            hl = 14 if f[1] & 0x7F == 127 else 8 if f[1] & 0x7F == 126 else 6
            p = xor_words(f[hl:], f[hl - 4:hl])
            rc = lib.vds_ec_ws_upload_request(p, len(p), None, C.byref(rid), C.byref(off), C.byref(ln), C.byref(size))
            assert rc == 0, rc
            plain.append(p)
            bodies_at.append((off.value, ln.value))
            got_ids.append(rid.value)
        tptr = np.empty(objects, dtype=np.uint64)
        tl = np.empty(objects, dtype=np.uint64)
        keep = [np.frombuffer(p, dtype=np.uint8) for p in plain]
        for o in range(objects):
            tptr[o] = keep[o].ctypes.data + bodies_at[o][0]
            tl[o] = bodies_at[o][1]
        rc = lib.vds_ec_upload16_host_batch(K, N, objects, tptr.ctypes.data_as(vpp), tl.ctypes.data_as(u64p),
                                            c_outs.ctypes.data_as(vpp), h_rd.ctypes.data, h_dd.ctypes.data,
                                            h_rs.ctypes.data_as(u32p), None, None, h_st.ctypes.data_as(i32p),
                                            C.byref(failed))
        assert rc == 0 and failed.value == 0, (rc, failed.value)
        n_js = C.c_size_t(0)
        for o in range(objects):
            rc = lib.vds_ec_upload_response_json(got_ids[o], h_rd.ctypes.data + 32 * N * o, N,
                                                 h_dd.ctypes.data + 32 * o, int(h_rs[o]), json_buf, len(json_buf),
                                                 C.byref(n_js))
            assert rc == 0, rc
            before_ans[o] = header(n_js.value) + json_buf.raw[:n_js.value]

    def ab(a_name, a_fn, b_name, b_fn, rounds):
        a_fn()  # warm-up: the staging grows to the workload
        b_fn()
        w = {a_name: [], b_name: []}
        for _ in range(max(1, rounds)):
            for name, fn in ((a_name, a_fn), (b_name, b_fn), (b_name, b_fn), (a_name, a_fn)):
                h0 = time.perf_counter()
                fn()
                w[name].append((time.perf_counter() - h0) * 1e3)
        return w

    wall = ab("ws_upload", host_ws_upload, "upload_before", host_upload_before, args.host_rounds)
    for o in range(objects):
        assert h_ans[int(h_ao[o]):int(h_ao[o] + h_al[o])].tobytes() == before_ans[o], o
    for name in ("ws_upload", "upload_before"):
        emit({"leg": name, "wall_ms_per_call": mm(wall[name]), "calls": len(wall[name]),
              "us_per_message": round(float(np.median(wall[name])) * 1e3 / objects, 2)})

    # download: the first dl objects' first K replicas and their names
    dl = max(1, min(args.dl_objects, objects))
    surv = [h_outs[o * N + j] for o in range(dl) for j in range(K)]
    names = np.frombuffer(b"".join(hashlib.sha256(c.tobytes()).digest() for c in surv), dtype=np.uint8).copy()
    cp = (C.c_void_p * (dl * K))(*[c.ctypes.data for c in surv])
    nodes = np.tile(np.arange(K, dtype=np.uint16), dl)
    csz = np.full(dl, L, dtype=np.uint64)
    d_ids = ids[:dl].copy()
    lay = [chunk.ws_download_answer_layout(int(i), BODY) for i in d_ids]
    slab = np.zeros(sum(x[0] for x in lay), dtype=np.uint8)
    fo, fl = np.zeros(dl, dtype=np.uint64), np.zeros(dl, dtype=np.uint64)
    st, sv = np.zeros(dl, dtype=np.int32), np.zeros(dl * K, dtype=np.uint8)
    tbuf = np.zeros((dl, T), dtype=np.uint8)
    tpp = (tbuf.ctypes.data + np.arange(dl, dtype=np.uint64) * np.uint64(T)).astype(np.uint64)
    slab2 = np.zeros(slab.size, dtype=np.uint8)

    def host_ws_download():
        rc = lib.vds_ec_ws_download16_host_batch(K, dl, d_ids.ctypes.data_as(i32p), nodes.ctypes.data_as(_lib.u16p), cp,
                                                 csz.ctypes.data_as(u64p), names.ctypes.data, None, None,
                                                 slab.ctypes.data, slab.size, fo.ctypes.data_as(u64p),
                                                 fl.ctypes.data_as(u64p), st.ctypes.data_as(i32p), sv.ctypes.data,
                                                 C.byref(failed))
        assert rc == 0 and failed.value == 0, (rc, failed.value)

    def host_download_before():
        tl = np.full(dl, T, dtype=np.uint64)
        rc = lib.vds_ec_download16_host_batch(K, dl, nodes.ctypes.data_as(_lib.u16p), cp, csz.ctypes.data_as(u64p),
                                              names.ctypes.data, None, None, tpp.ctypes.data_as(vpp),
                                              tl.ctypes.data_as(u64p), st.ctypes.data_as(i32p), sv.ctypes.data,
                                              C.byref(failed))
        assert rc == 0 and failed.value == 0, (rc, failed.value)
        at = 0
        for o in range(dl):
            front = b'{"id":"%d","result":"' % int(d_ids[o])
            h = header(len(front) + T + 2) + front
            slab2[at:at + len(h)] = np.frombuffer(h, dtype=np.uint8)
            at += len(h)
            slab2[at:at + T] = tbuf[o]
            at += T
            slab2[at:at + 2] = (0x22, 0x7D)
            at += 2

    wall_d = ab("ws_download", host_ws_download, "download_before", host_download_before, args.host_rounds)
    assert np.array_equal(slab, slab2), "the two download routes build different frames"
    assert slab[int(lay[0][2]):int(lay[0][2]) + T].tobytes() == texts[0]
    for name in ("ws_download", "download_before"):
        emit({"leg": name, "wall_ms_per_call": mm(wall_d[name]), "calls": len(wall_d[name]), "objects": dl,
              "us_per_message": round(float(np.median(wall_d[name])) * 1e3 / dl, 2)})

    d = lambda name: float(np.median(t[name]))
    med = lambda w, name: float(np.median(w[name]))
    spread = lambda w, name: float(max(w[name]) - min(w[name]))
    ok_up = med(wall, "ws_upload") <= med(wall, "upload_before") + spread(wall, "upload_before")
    ok_dl = med(wall_d, "ws_download") <= med(wall_d, "download_before") + spread(wall_d, "download_before")
    emit({"summary": {"decode_device_ms": round(d("decode"), 4), "decode_masked_device_ms": round(d("decode_masked"), 4),
                      "masked_over_unmasked": round(d("decode_masked") / d("decode"), 4),
                      "answer_device_ms": round(d("answer"), 4),
                      "ws_upload_us_per_message": round(med(wall, "ws_upload") * 1e3 / objects, 2),
                      "upload_before_us_per_message": round(med(wall, "upload_before") * 1e3 / objects, 2),
                      "upload_before_spread_ms": round(spread(wall, "upload_before"), 2),
                      "ws_download_us_per_message": round(med(wall_d, "ws_download") * 1e3 / dl, 2),
                      "download_before_us_per_message": round(med(wall_d, "download_before") * 1e3 / dl, 2),
                      "download_before_spread_ms": round(spread(wall_d, "download_before"), 2),
                      "ws_upload_no_slower": ok_up, "ws_download_no_slower": ok_dl}})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(log) + "\n")
    return 0 if ok_up and ok_dl else 1


if __name__ == "__main__":
    sys.exit(main())
