"""zlib streams for the inflate tests (host and device), each with what Python's
zlib -- the library the reference links -- makes of it.  Everything is built at
import time from fixed seeds; nothing here touches the library under test.

expected(stream) is the authority for every case: (status, bytes) from
zlib.decompressobj().decompress(stream), VDS_EC_OK when the stream ended,
VDS_EC_EINFLATE_SHORT (with the bytes zlib delivered) when it did not,
VDS_EC_EINFLATE_DATA when zlib raised.
"""
from __future__ import annotations

import random
import struct
import zlib

OK, EINVAL, ECORRUPT = 0, -1, -10
ECRYPT_LENGTH, ECRYPT_PADDING = -18, -19
EINFLATE_DATA, EINFLATE_SHORT, EINFLATE_SPACE = -20, -21, -22


def expected(stream: bytes):
    d = zlib.decompressobj()
    try:
        out = d.decompress(stream)
    except zlib.error:
        return EINFLATE_DATA, b""
    return (OK if d.eof else EINFLATE_SHORT), out


def expected_cap(stream: bytes, cap: int):
    """(status, bytes) under a finite capacity cap >= 1, from zlib alone.  What zlib makes of the stream
    with room for cap bytes: an error it meets is DATA, its end is OK, fewer than cap bytes are SHORT with
    them.  With cap bytes delivered and no end, a fresh object with room for cap + 1 tells whether a byte
    more was wanted (SPACE: it comes, or zlib meets an error behind it) or the bytes fitted exactly.  (A
    second call on the first object would not do: zlib runs on to a trailer's error inside one call.)
    max_length = 0 means unlimited in Python, so cap = 0 has no answer here."""
    assert cap >= 1
    d = zlib.decompressobj()
    try:
        out = d.decompress(stream, cap)
    except zlib.error:
        return EINFLATE_DATA, b""
    if d.eof:
        return OK, out
    if len(out) < cap:
        return EINFLATE_SHORT, out
    d = zlib.decompressobj()
    try:
        more = d.decompress(stream, cap + 1)
    except zlib.error:
        return EINFLATE_SPACE, b""
    if len(more) == cap + 1:
        return EINFLATE_SPACE, b""
    return (OK if d.eof else EINFLATE_SHORT), more


_WORDS = None


def text(n: int, seed: int) -> bytes:
    """n text-like bytes: words of a 400-word vocabulary of random letters,
    Zipf-like frequencies, spaces and a few line ends between them."""
    global _WORDS
    if _WORDS is None:
        r = random.Random(1)
        _WORDS = [bytes(r.choice(b"etaoinshrdlucmfwypvbgkqjxz") for _ in range(r.randint(2, 9))) for _ in range(400)]
    r = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += _WORDS[min(int(r.paretovariate(0.9)) - 1, 399)]
        out += b"\n" if r.random() < 0.08 else b" "
    return bytes(out[:n])


def splitmix(n: int, seed: int) -> bytes:
    """n bytes of the splitmix64 stream of `seed` (they do not compress)."""
    out = bytearray()
    x = seed & 0xFFFFFFFFFFFFFFFF
    while len(out) < n:
        x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        out += struct.pack("<Q", z ^ (z >> 31))
    return bytes(out[:n])


def deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, btype=None) -> bytes:
    """A zlib stream of `data`; btype: what the first block's type must be (a
    zlib that chooses differently fails the precondition here)."""
    c = zlib.compressobj(level, zlib.DEFLATED, 15, mem_level, strategy)
    s = c.compress(data) + c.flush()
    if btype is not None:
        assert (s[2] >> 1) & 3 == btype, ("first block type", (s[2] >> 1) & 3, btype)
    return s


def stored_block_count(s: bytes) -> int:
    """the stored blocks of a stream made of stored blocks only"""
    at, n = 2, 0
    while True:
        last = s[at] & 1
        assert (s[at] >> 1) & 3 == 0
        ln = s[at + 1] | s[at + 2] << 8
        at += 5 + ln
        n += 1
        if last:
            return n


# ------------------------------------------------------------------ valid streams
def valid_cases():
    """[(name, stream, plaintext)]"""
    cases = []

    def add(name, data, **kw):
        s = deflate(data, **kw)
        assert expected(s) == (OK, data), name
        cases.append((name, s, data))
        return s

    t40k = text(40 * 1024, 11)
    add("stored", text(700, 2), level=0, btype=0)
    s = add("stored two blocks", text(70000, 3), level=0, btype=0)
    assert stored_block_count(s) == 2
    add("fixed", text(600, 4), strategy=zlib.Z_FIXED, btype=1)
    add("dynamic level 6", text(5000, 5), level=6, btype=2)
    add("dynamic level 9", text(5000, 6), level=9, btype=2)
    add("memLevel 1: many dynamic blocks", text(30000, 7), mem_level=1, btype=2)
    add("huffman only", text(3000, 8), strategy=zlib.Z_HUFFMAN_ONLY, btype=2)
    add("rle", bytes([7]) * 900 + text(300, 9) + bytes([9]) * 2000, strategy=zlib.Z_RLE)
    add("splitmix level 6", splitmix(3000, 10), level=6)
    for n in (0, 1, 2):
        add(f"text of {n}", text(n, 12 + n))
    for n in (257, 258, 259):
        add(f"{n} of one byte", bytes([0x41]) * n)
        add(f"{n} of one byte, fixed", bytes([0x42]) * n, strategy=zlib.Z_FIXED, btype=1)
    far = splitmix(32768, 20)
    add("distance 32768", far + far[:300], level=9)
    add("65536 of text", text(65536, 21))
    add("65537 of text", text(65537, 22))
    add("65536 of splitmix", splitmix(65536, 23))
    add("40 KiB of text", t40k, level=9)
    return cases


# ------------------------------------------------------------ hand-made failures
class BitW:
    """deflate's bit order: values least significant bit first, Huffman codes
    most significant bit first"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        return self

    def huff(self, code, n):
        for i in range(n - 1, -1, -1):
            self.bits((code >> i) & 1, 1)
        return self

    def bytes(self, pad=8):
        return self.acc.to_bytes((self.n + 7) // 8, "little") + bytes(pad)


def header(cmf=0x78, flg=0x80):
    """CMF, FLG with FCHECK made right"""
    flg &= 0xE0
    flg += (31 - ((cmf << 8) + flg) % 31) % 31
    return bytes([cmf, flg])


def wrap(raw: bytes, data: bytes = b"") -> bytes:
    return header() + raw + struct.pack(">I", zlib.adler32(data))


def dynamic_header(w: BitW, lit: list, dist: list, last=1):
    """A dynamic block's header for the given code lengths (each 0..15), under
    a code-length code of sixteen 4-bit codes: length v is the code v."""
    w.bits(last, 1).bits(2, 2).bits(len(lit) - 257, 5).bits(len(dist) - 1, 5).bits(15, 4)
    for sym in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        w.bits(4 if sym < 16 else 0, 3)
    for v in list(lit) + list(dist):
        w.huff(v, 4)
    return w


def failures():
    """[(name, stream)], each raising in zlib"""
    out = []

    def add(name, s, needle=None):
        d = zlib.decompressobj()
        try:
            d.decompress(s)
        except zlib.error as e:
            assert needle is None or needle in str(e), (name, str(e))
        else:
            raise AssertionError(f"{name}: zlib accepts it")
        out.append((name, s))

    good = deflate(text(300, 30))
    add("CM != 8", header(0x77) + good[2:], "unknown compression method")
    add("CINFO > 7", header(0x88) + good[2:], "invalid window size")
    add("bad FCHECK", bytes([good[0], good[1] ^ 1]) + good[2:], "incorrect header check")
    add("FDICT", header(0x78, 0xA0) + good[2:])
    add("BTYPE 3", wrap(BitW().bits(1, 1).bits(3, 2).bytes()), "invalid block type")
    add("stored LEN != ~NLEN", wrap(bytes([1, 5, 0, 0, 0]) + bytes(8)), "invalid stored block lengths")
    add("HLIT > 286", wrap(BitW().bits(1, 1).bits(2, 2).bits(30, 5).bits(0, 5).bits(0, 4).bytes()),
        "too many length or distance symbols")
    add("HDIST > 30", wrap(BitW().bits(1, 1).bits(2, 2).bits(0, 5).bits(30, 5).bits(0, 4).bytes()),
        "too many length or distance symbols")
    w = BitW().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4)
    for _ in range(4):
        w.bits(1, 3)  # 16, 17, 18, 0: four codes of one bit
    add("over-subscribed code-length code", wrap(w.bytes()), "invalid code lengths set")
    lit = [0] * 257
    lit[0] = lit[256] = 2
    add("incomplete literal/length set", wrap(dynamic_header(BitW(), lit, [1]).bytes()), "invalid literal/lengths set")
    w = BitW().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4)
    for v in (1, 0, 0, 1):  # 16 and 0, one bit each: 0 is the code 0, 16 the code 1
        w.bits(v, 3)
    add("repeat with no length before it", wrap(w.huff(1, 1).bits(0, 2).bytes()), "invalid bit length repeat")
    lit = [0] * 257
    lit[0] = lit[1] = 1
    add("no end-of-block code", wrap(dynamic_header(BitW(), lit, [1]).bytes()), "missing end-of-block")
    for sym in (286, 287):
        add(f"literal/length symbol {sym}", wrap(BitW().bits(1, 1).bits(1, 2).huff(0b11000000 + sym - 280, 8).bytes()),
            "invalid literal/length code")
    for sym in (30, 31):
        add(f"distance symbol {sym}",
            wrap(BitW().bits(1, 1).bits(1, 2).huff(0x30 + 0x41, 8).huff(1, 7).huff(sym, 5).bytes()),
            "invalid distance code")
    zd = text(2000, 31)
    data = zd[500:1500]
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, zd)
    raw = c.compress(data) + c.flush()
    add("distance too far back", wrap(raw, data), "invalid distance too far back")
    add("wrong Adler-32", good[:-1] + bytes([good[-1] ^ 1]), "incorrect data check")
    return out


# ---------------------------------------------------------------------- prefixes
def prefix_streams():
    """[(name, stream)] of about 300 to 400 bytes each: fixed, dynamic, stored"""
    res = [("fixed", deflate(text(1100, 40), strategy=zlib.Z_FIXED, btype=1)),
           ("dynamic", deflate(text(1300, 41), level=9, btype=2)),
           ("stored", deflate(text(340, 42), level=0, btype=0))]
    for name, s in res:
        assert 280 <= len(s) <= 420, (name, len(s))
    return res


def prefixes(stream: bytes):
    """[(prefix, status, bytes)] for every prefix, the whole stream included"""
    return [(stream[:n],) + expected(stream[:n]) for n in range(len(stream) + 1)]


# --------------------------------------------------------------------- mutations
MUTATION_KINDS = ("fixed", "dynamic")


def mutations(kind: str, count: int = 256, seed: int = 5):
    """[(stream, status, bytes)]: single-bit flips of the deflate body of a
    stream of about 200 bytes.  A flipped body that raw zlib still decodes to
    its end gets the Adler-32 of what it produced (else nearly every case would
    be a wrong checksum); the others keep the stream as it stands.  What is
    expected is zlib's answer to the final stream either way."""
    if kind == "fixed":
        s = deflate(text(560, 50), strategy=zlib.Z_FIXED, btype=1)
    else:
        s = deflate(text(600, 51), level=9, btype=2)
    assert 150 <= len(s) <= 260, (kind, len(s))
    body = s[2:-4]
    r = random.Random(seed)
    out = []
    for _ in range(count):
        bit = r.randrange(8 * len(body))
        m = bytearray(body)
        m[bit // 8] ^= 1 << (bit % 8)
        m = bytes(m)
        d = zlib.decompressobj(-15)
        try:
            got = d.decompress(m)
            ended = d.eof
        except zlib.error:
            ended = False
        if ended:
            m = m[:len(m) - len(d.unused_data)]
            stream = s[:2] + m + struct.pack(">I", zlib.adler32(got))
        else:
            stream = s[:2] + m + s[-4:]
        out.append((stream,) + expected(stream))
    return out


def mutation_cap(stream: bytes) -> int:
    """A match of 258 bytes costs at least 2 bits, so no stream of n bytes
    inflates past 1032 n: the capacity is never what stops one."""
    return 1032 * len(stream) + 64
