"""Pin the CPU oracle (oracle/vds_oracle.c) to the reference before trusting it.

1. The reference's own kernel/vds_data/gf.h, compiled unmodified into
   oracle/_ref/gf_ref (oracle/Makefile), against the oracle's GF arithmetic:
   every 8-bit pair and a structured + random set of 16-bit pairs.  Where
   gf_ref is not built, the digests recorded from its dumps
   (tests/golden/ref_gf_digests.json) stand in for it.
2. The known-answer vectors recorded from the reference in SURVEY.md 8(a)/(c)
   (tests/golden/survey_kats.json) and the GF(2^3) table of
   tests/test_vds_data/gf_tests.cpp:9-38.
3. The frozen oracle fixtures (tests/golden/golden_vectors.json).
4. The reference's round-trip tests re-hosted on the oracle
   (chunk_tests.cpp:10-162), seeded.
"""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_ctypes as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _kats():
    with open(os.path.join(GOLDEN, "survey_kats.json")) as f:
        return json.load(f)


def _golden():
    with open(os.path.join(GOLDEN, "golden_vectors.json")) as f:
        return json.load(f)


def _read_dump(path, dtype, arrays):
    raw = open(path, "rb").read()
    out, pos = [], 0
    for _ in range(arrays):
        n = int(np.frombuffer(raw[pos:pos + 4], dtype=np.uint32)[0])
        pos += 4
        nbytes = n * np.dtype(dtype).itemsize
        out.append(np.frombuffer(raw[pos:pos + nbytes], dtype=dtype))
        pos += nbytes
    return out


def test_gf3_table_matches_gf_tests():
    tbl = _kats()["gf3_table_gf_tests_cpp_9_38"]
    for i in range(8):
        for j in range(8):
            assert O.gf_mul_bitserial(3, 0x0B, i, j) == tbl[i][j]


def test_survey_kats():
    k = _kats()
    e = k["encode16_k4_s19"]
    data = np.array([(37 * i + 11) % 256 for i in range(e["size"])], dtype=np.uint8)
    for r, hexs in e["replicas"].items():
        assert O.encode(e["k"], int(r), data).tobytes().hex() == hexs
    M, rc = O.inverse(4, [2, 3, 4, 5])
    assert rc == 0
    assert ["%04x" % x for x in M[0]] == k["inverse16_k4_nodes_2345_row0"]
    for a, b, p in k["gf8_mul"]:
        assert O.gf8_mul(a, b) == p
    for a, b, p in k["gf16_mul"]:
        assert O.gf16_mul(a, b) == p
    for a, b, p in k["gf16_div"]:
        assert O.gf16_div(a, b) == p


REF_GF = O.REF_GF


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _ref_gf_pairs(mode):
    """The operand pairs oracle/ref_gf_harness.cpp feeds the reference's gf.h,
    in its order."""
    if mode == "gf3":
        i, j = np.divmod(np.arange(64), 8)
        return i.astype(np.uint8), j.astype(np.uint8)
    if mode == "gf8":
        i, j = np.divmod(np.arange(65536), 256)
        return i.astype(np.uint8), j.astype(np.uint8)
    fixed = np.array([0, 1, 2, 3, 5, 19, 39, 63, 0x100B, 0x8000, 0x1234, 0xFFFF], dtype=np.uint16)
    x = np.repeat(np.arange(65536, dtype=np.uint16), fixed.size)
    y = np.tile(fixed, 65536)
    a = np.stack([x, y], axis=1).reshape(-1)  # (x, y), (y, x), ...
    b = np.stack([y, x], axis=1).reshape(-1)
    with np.errstate(over="ignore"):  # splitmix64 from 0x7664730000000000, arithmetic mod 2^64
        z = np.uint64(0x7664730000000000) + np.arange(1, (1 << 20) + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (np.concatenate([a, z.astype(np.uint16)]),
            np.concatenate([b, (z >> np.uint64(16)).astype(np.uint16)]))


@pytest.mark.parametrize("mode", ["gf3", "gf8", "gf16"])
def test_oracle_matches_compiled_reference_gf(mode, tmp_path):
    """Against gf_ref's dump where oracle/_ref/gf_ref is built, and always
    against the digests recorded from it (tests/golden/ref_gf_digests.json,
    tests/golden/make_ref_gf_digests.py): the same pairs, the same products."""
    with open(os.path.join(GOLDEN, "ref_gf_digests.json")) as f:
        want = json.load(f)[mode]
    dt = np.uint16 if mode == "gf16" else np.uint8
    names = ["a", "b", "mul"] if mode == "gf3" else ["a", "b", "mul", "div", "bits"]
    a, b = _ref_gf_pairs(mode)
    assert a.size == b.size == want["count"] and _sha(a) == want["a"] and _sha(b) == want["b"]
    if os.path.exists(REF_GF):
        out = tmp_path / f"{mode}.bin"
        subprocess.run([REF_GF, mode, str(out)], check=True)
        ref = dict(zip(names, _read_dump(out, dt, len(names))))
        assert all(_sha(ref[nm]) == want[nm] for nm in names)  # the fixture is this binary's output
        assert np.array_equal(ref["a"], a) and np.array_equal(ref["b"], b)
    else:
        ref = None
    if mode == "gf3":
        ours = np.array([O.gf_mul_bitserial(3, 0x0B, x, y) for x, y in zip(a, b)], dtype=np.uint8)
        assert _sha(ours) == want["mul"] and (ref is None or np.array_equal(ours, ref["mul"]))
        return
    mul, div = O.bulk(f"{mode}_mul", a, b), O.bulk(f"{mode}_div", a, b)
    assert mul.dtype == dt and div.dtype == dt and mul.size == div.size == a.size > 0
    assert _sha(mul) == want["mul"] and _sha(div) == want["div"]
    if ref is not None:
        assert np.array_equal(mul, ref["mul"]) and np.array_equal(div, ref["div"])
    # table multiply == bit-serial gf<m> multiply (x primitive) on every pair
    assert want["mul"] == want["bits"] and (ref is None or np.array_equal(ref["mul"], ref["bits"]))
    bits = mul  # (the reference's bit-serial products, by the digests above)
    if mode == "gf8":
        sample = slice(None)
    else:
        sample = slice(0, None, 97)
    m = 8 if mode == "gf8" else 16
    poly = 0x1D if mode == "gf8" else 0x100B
    ours = np.array([O.gf_mul_bitserial(m, poly, int(x), int(y)) for x, y in zip(a[sample], b[sample])], dtype=dt)
    assert np.array_equal(ours, bits[sample])


def test_golden_fixtures_regress():
    g = _golden()
    base = g["seed_base"]
    for e in g["encode16_small"]:
        d = O.splitmix(base + e["object_index"], e["size"])
        for r, hexs in e["replicas"].items():
            assert O.encode(e["k"], int(r), d).tobytes().hex() == hexs
    for inv in g["inverse16"]:
        M, rc = O.inverse(inv["k"], inv["nodes"])
        assert rc == inv["rc"] == 0
        assert M.tolist() == inv["rows"]


def test_oracle_restore_roundtrip_edges():
    rng = np.random.default_rng(1)
    for k, size in ((4, 0), (4, 1), (4, 7), (4, 8), (4, 9), (3, 1000), (16, 65541), (5, 12345)):
        d = rng.integers(0, 256, size, dtype=np.uint8)
        nodes = list(rng.choice(np.arange(1, 300), size=k, replace=False))
        chunks = [O.encode(k, int(r), d) for r in nodes]
        out = O.restore(k, nodes, chunks)
        assert out is not None and out.tobytes() == d.tobytes()


def test_rehost_chunk_tests_on_oracle():
    """chunk_tests.cpp:10-110 (cell arrays, uint8/uint16, k=3) and
    :112-162 (byte API, min_horcrux replicas of < 1000), seeded."""
    rng = np.random.default_rng(7)
    for cb in (1, 2):
        size = 999
        data = rng.integers(0, 256 if cb == 1 else 65536, size).astype(np.uint8 if cb == 1 else np.uint16)
        ids = [int(x) for x in rng.choice(256, 3, replace=False)]
        chunks = [O.chunk_cells(3, r, data, cell_bytes=cb) for r in ids]
        out = O.restore_cells(3, ids, chunks, cell_bytes=cb)
        assert np.array_equal(out[:size], data)
    k = 120  # the reference uses 800; the full size runs on the GPU path
    size = 4321
    data = rng.integers(0, 256, size, dtype=np.uint8)
    ids = [int(x) for x in rng.choice(1000, k, replace=False)]
    chunks = [O.encode(k, r, data) for r in ids]
    out = O.restore(k, ids, chunks)
    assert out.tobytes() == data.tobytes()
