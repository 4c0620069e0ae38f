"""The bodies the deflate tests share (tests/test_deflate_host_cpu.py and
tests/test_deflate_batch_gpu.py): built once at import from fixed seeds;
nothing here touches the library under test.

cases() is [(name, data)].  The lengths stand where the compressor changes its
path (SEGMENT is its segment in input bytes: 56 chunks of 64 positions), the
contents where its match finder, its trees and its stored fallback do.
"""
from __future__ import annotations

import random

from inflate_cases import splitmix, text

SEGMENT = 3584
BLOCK_SIZE = (1 << 20) + 5  # the server's BLOCK_SIZE and a ragged tail

LENGTHS = ([0, 1, 2, 3, 4, 5] + list(range(63, 68)) + [127, 128, 129] + [257, 258, 259, 260] +
           [32767, 32768, 32769, 32770] + [65535, 65536, 65537] +
           [SEGMENT - 1, SEGMENT, SEGMENT + 1, 2 * SEGMENT + 1])
PERIODS = [2, 3, 4, 5, 63, 64, 65, 258, 259]
FAR_PERIODS = [32767, 32768, 32769]  # the farthest legal distance twice, then none at all


def periodic(n: int, period: int, seed: int) -> bytes:
    head = splitmix(period, seed)
    return (head * (n // period + 1))[:n]


def no_match(n: int = 64, seed: int = 5) -> bytes:
    """At most one chunk (the table is empty while it is read) of four symbols,
    no two neighbours equal: no candidate anywhere, yet two bits a byte."""
    assert n <= 64
    r = random.Random(seed)
    out = [r.randrange(4)]
    while len(out) < n:
        out.append(r.choice([s for s in range(4) if s != out[-1]]))
    return bytes(65 + s for s in out)


def fibonacci(symbols: int, seed: int) -> bytes:
    """Byte frequencies 1, 1, 2, 3, 5, ... over `symbols` symbols, shuffled: an
    unlimited Huffman tree over them is symbols - 1 deep.  (The common bytes
    cannot help repeating, so matches form and a segment's counts are not these;
    the length limit itself is tested on the shared routine with exact counts,
    tests/cpp/test_deflate_host.cpp.)"""
    a, b, out = 1, 1, bytearray()
    for s in range(symbols):
        out += bytes([32 + 3 * s]) * a
        a, b = b, a + b
    r = random.Random(seed)
    lst = list(out)
    r.shuffle(lst)
    return bytes(lst)


_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    c = []
    for n in LENGTHS:
        c.append((f"zeros-{n}", bytes(n)))
        c.append((f"text-{n}", text(n, 300 + n % 97)))
        c.append((f"splitmix-{n}", splitmix(n, 400 + n % 89)))
    for p in PERIODS:
        for n in (129, 260, SEGMENT + 1, 65537):
            if n > p:
                c.append((f"period{p}-{n}", periodic(n, p, 500 + p)))
    for p in FAR_PERIODS:
        for n in (65537, 2 * 32769 + 100):
            c.append((f"period{p}-{n}", periodic(n, p, 600 + p)))
    for n in (1, 5, 300, SEGMENT + 1):
        c.append((f"one-byte-{n}", b"\x07" * n))
    c.append(("no-match-64", no_match()))
    c.append(("fibonacci-22", fibonacci(22, 7)))  # 46367 bytes
    c.append(("fibonacci-16", fibonacci(16, 8)))  # 2583 bytes, one segment (runs of the common bytes become matches)
    c.append((f"text-{BLOCK_SIZE}", text(BLOCK_SIZE, 777)))
    assert len({name for name, _ in c}) == len(c)
    _CASES = c
    return c


def short_cases(limit: int = 5000):
    return [(name, d) for name, d in cases() if len(d) <= limit]
