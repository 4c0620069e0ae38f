"""Record tests/golden/ref_gf_digests.json: the SHA-256 of every array that
oracle/_ref/gf_ref (the reference's own gf.h, compiled by oracle/Makefile where
the reference tree is present) writes in its gf3 / gf8 / gf16 modes.

tests/test_oracle_pin.py pins the oracle's GF arithmetic to these digests
where gf_ref itself cannot be built, and checks gf_ref's dumps against them
where it can.

    make -C oracle && python tests/golden/make_ref_gf_digests.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import oracle_ctypes as O  # noqa: E402

MODES = {"gf3": (np.uint8, ["a", "b", "mul"]),
         "gf8": (np.uint8, ["a", "b", "mul", "div", "bits"]),
         "gf16": (np.uint16, ["a", "b", "mul", "div", "bits"])}


def read_dump(path, dtype, arrays):
    """gf_ref's dump: per array a uint32 count, then that many little-endian values."""
    raw = open(path, "rb").read()
    out, pos = [], 0
    for _ in range(arrays):
        n = int(np.frombuffer(raw[pos:pos + 4], dtype=np.uint32)[0])
        pos += 4
        nbytes = n * np.dtype(dtype).itemsize
        out.append(np.frombuffer(raw[pos:pos + nbytes], dtype=dtype))
        pos += nbytes
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    res = {"source": "oracle/_ref/gf_ref <mode> (oracle/ref_gf_harness.cpp over the reference's kernel/vds_data/gf.h)",
           "format": "sha256 of each dumped array's little-endian bytes; count = elements per array"}
    with tempfile.TemporaryDirectory() as d:
        for mode, (dt, names) in MODES.items():
            out = os.path.join(d, mode + ".bin")
            subprocess.run([O.REF_GF, mode, out], check=True)
            arrs = read_dump(out, dt, len(names))
            res[mode] = {"count": int(arrs[0].size), **{nm: digest(a) for nm, a in zip(names, arrs)}}
    with open(os.path.join(HERE, "ref_gf_digests.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
