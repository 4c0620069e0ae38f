"""tests/cpp/test_rsa_host.cpp -- the host RSA routines on heap buffers of
exactly the stated lengths -- built as a stand-alone program from rsa_host.cpp
and sha256_host.cpp with -fsanitize=address,undefined, and run as a program: a
byte read or written outside a buffer, or undefined arithmetic, ends it with a
report.  The cases are those of tests/test_rsa_host_cpu.py (moduli, exponents
and operands of the raw operation, the libcrypto fixture, fingerprints, block
forms and truncations), written to a file with their expected values from
Python integers."""
import os
import subprocess

import pytest

import rsa_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vds_amd", "csrc")
EINVAL, ETX_FORM = -1, -23


def _hex(b: bytes) -> str:
    return b.hex() or "-"


def _mag(v: int) -> str:
    return _hex(v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big"))


def _records():
    out = []
    for i, n in enumerate(R.moduli()):
        k = R.n_bytes(n)
        for e in R.EXPONENTS:
            for s in R.operands(n, 100 + i):
                out.append(f"P {_mag(n)} {_mag(e)} {_hex(s.to_bytes(k, 'big'))} 0 {_hex(pow(s, e, n).to_bytes(k, 'big'))}")
        for bad in (n.to_bytes(k, "big"), (5).to_bytes(k - 1, "big"), (5).to_bytes(k + 1, "big"), b""):
            out.append(f"P {_mag(n)} {_mag(65537)} {_hex(bad)} {EINVAL} -")
    f = R.kats()
    for c in f["cases"]:
        key = f["keys"][c["key"]]
        out.append(f"V {_mag(key['n'])} {_mag(key['e'])} {_hex(c['msg'])} {_hex(c['sig'])} {c['verdict']}")
    n = f["keys"][2]["n"]
    for bn, be, st in ((n, 65537, 0), (n + 1, 65537, EINVAL), (2 ** 511 - 1, 3, EINVAL), (2 ** 511 + 1, 3, 0),
                       (2 ** 4096 + 1, 3, EINVAL), (2 ** 4096 - 1, 3, 0), (n, 1, EINVAL), (n, 2 ** 32 + 1, EINVAL),
                       (0, 3, EINVAL)):
        out.append(f"K {_mag(bn)} {_mag(be)} {st}")
    for key in f["keys"]:
        out.append(f"F {_mag(key['n'])} {_mag(key['e'])} {R.fingerprint(key['n'], key['e']).hex()}")
    for top in (0x7F, 0x80, 0x90, 0xFF):
        n = int.from_bytes(bytes([top]) + bytes(range(1, 70)), "big")
        out.append(f"F {_mag(n)} {_mag(top << 16 | 1)} {R.fingerprint(n, top << 16 | 1).hex()}")
    prefix = R.block_prefix(1700000000, 300, bytes(range(32)), [b"\x01" * 32, b"\x02" * 32, b"\x09" * 5], bytes(200))
    blk = R.block(prefix, bytes(512))
    out.append(f"T {blk.hex()} 0 {len(prefix)}")
    for cut in range(1, len(blk)):
        out.append(f"T {blk[:cut].hex()} {ETX_FORM} 0")
    out.append(f"T {(blk + bytes(1)).hex()} {ETX_FORM} 0")
    return out


@pytest.fixture(scope="module")
def rsa_bin(tmp_path_factory):
    d = tmp_path_factory.mktemp("rsa")
    out = d / "test_rsa_host"
    cmd = ["g++", "-O1", "-g", "-std=c++20", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_rsa_host.cpp"),
           os.path.join(CSRC, "rsa_host.cpp"), os.path.join(CSRC, "sha256_host.cpp"), "-o", str(out)]
    subprocess.run(cmd, check=True)
    cases = d / "cases.txt"
    cases.write_text("\n".join(_records()) + "\n")
    return str(out), str(cases)


def test_rsa_host_under_sanitizers(rsa_bin):
    r = subprocess.run(list(rsa_bin), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rsa OK" in r.stdout
