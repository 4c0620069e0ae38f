"""tests/cpp/test_deflate_host.cpp -- vds_ec_deflate_host into heap buffers of
exactly vds_ec_deflate_bound bytes and vds_ec_inflate_host back -- built as a
stand-alone program from deflate_host.cpp and inflate_host.cpp with
-fsanitize=address,undefined, and run as a program: a byte read or written
outside a buffer, or undefined arithmetic, ends it with a report.  It also
drives the length-limited code construction the host and the device share with
counts that pass the 15- and 7-bit limits."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vds_amd", "csrc")


@pytest.fixture(scope="module")
def deflate_bin(tmp_path_factory):
    out = tmp_path_factory.mktemp("deflate") / "test_deflate_host"
    cmd = ["g++", "-O1", "-g", "-std=c++20", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_deflate_host.cpp"),
           os.path.join(CSRC, "deflate_host.cpp"), os.path.join(CSRC, "inflate_host.cpp"), "-o", str(out)]
    subprocess.run(cmd, check=True)
    return str(out)


def test_deflate_host_under_sanitizers(deflate_bin):
    r = subprocess.run([deflate_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "deflate OK" in r.stdout
