"""A deflate writer for the inflate tests, and its model.

The writer emits what no compressor would: any canonical code up to 15 bits,
any run-length coding of the code lengths, raw length and distance symbols with
chosen extra bits, stored blocks at any bit phase.  Nothing here touches the
library under test, and nothing here decides what a stream means: Python's zlib
does (check_valid / check_invalid below, which every stream of the corpus goes
through when it is built).  The token model is a second opinion on this
generator, never on the library.

Blocks are values (stored / fixed / dynamic); zstream(blocks) writes them behind
an RFC 1950 header and puts the Adler-32 of the model's plaintext behind them.
A token is
    an int                               a literal
    (L, D)                               a match, coded the usual way
    ("lsym", sym, extra_bits, extra_val) a raw length symbol; the next token must
    ("dsym", sym, extra_bits, extra_val) be a ("dsym", ...) or a ("raw", ...)
    ("raw", value, nbits)                bits as they stand, least significant
                                         first: always the first bad token
"""
from __future__ import annotations

import random
import struct
import zlib
from collections import namedtuple

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def len_sym(L):
    """(symbol, extra bits, extra value) of a match length, 258 as symbol 285"""
    assert 3 <= L <= 258
    s = 28 if L == 258 else max(i for i in range(28) if LEN_BASE[i] <= L)
    return 257 + s, LEN_EXTRA[s], L - LEN_BASE[s]


def dist_sym(D):
    assert 1 <= D <= 32768
    s = max(i for i in range(30) if DIST_BASE[i] <= D)
    return s, DIST_EXTRA[s], D - DIST_BASE[s]


_LSYM = [None] * 3 + [len_sym(L) for L in range(3, 259)]


def canonical(lens):
    """RFC 1951 3.2.2: per symbol (code reversed for the least-significant-first stream, length), None
    where the length is 0.  The set may be incomplete; an over-subscribed one has no codes."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if not l:
            out.append(None)
            continue
        c = nxt[l]
        nxt[l] += 1
        assert c < (1 << l), "over-subscribed set: no canonical codes"
        out.append((int(format(c, "0%db" % l)[::-1], 2), l))
    return out


def kraft(lens):
    """sum of 2^(15 - l): 32768 for a complete set"""
    return sum(1 << (15 - l) for l in lens if l)


class Bits:
    """least significant bit first; whole bytes leave the accumulator as they fill"""

    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 256:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def code(self, c):
        self.bits(c[0], c[1])

    def tell(self):
        return 8 * len(self.buf) + self.n

    def align(self):
        self.bits(0, -self.n % 8)

    def raw(self, data):
        assert self.n % 8 == 0
        self.buf += self.acc.to_bytes(self.n // 8, "little")
        self.acc = self.n = 0
        self.buf += data

    def done(self):
        self.align()
        self.raw(b"")
        return bytes(self.buf)


Block = namedtuple("Block", "kind last data tokens lit_lens dist_lens cl_symbols cl_lens hclen bad_header")


def stored(data, last=False):
    assert len(data) <= 65535
    return Block(0, last, bytes(data), (), None, None, None, None, None, False)


def fixed(tokens, last=False):
    return Block(1, last, b"", list(tokens), FIXED_LIT, FIXED_DIST, None, None, None, False)


def dynamic(tokens, lit_lens, dist_lens, last=False, cl_symbols=None, cl_lens=None, hclen=None, bad_header=False):
    """cl_symbols: the code-length symbols as they are sent, a 16 / 17 / 18 as (sym, repeats); default: a
    greedy run-length coding.  cl_lens: the 19 lengths of the code-length code; default: a complete code of
    near-equal lengths over the symbols used.  hclen: how many of them are sent (4..19); default: as few as
    CL_ORDER allows.  bad_header: the header is meant to be refused, so the model ends before this block;
    bad_header="tail": the tokens and the end-of-block code are written behind it all the same, so that a
    decoder that accepts the header goes on as if nothing were wrong."""
    assert 257 <= len(lit_lens) <= 288 and 1 <= len(dist_lens) <= 32
    return Block(2, last, b"", list(tokens), list(lit_lens), list(dist_lens), cl_symbols, cl_lens, hclen, bad_header)


def rle(lens):
    """a greedy run-length coding of code lengths: [sym or (sym, repeats)]"""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k))
                run -= k
            if run >= 3:
                out.append((17, run))
                run = 0
        else:
            out.append(v)
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k))
                run -= k
        out += [v] * run
        i = j
    return out


def default_cl_lens(cl_symbols):
    used = [0] * 19
    for s in cl_symbols:
        used[s[0] if isinstance(s, tuple) else s] += 1
    syms = sorted((s for s in range(19) if used[s]), key=lambda s: -used[s])
    if len(syms) < 2:  # the code-length code may not be incomplete
        syms.append(next(s for s in (0, 1, 2) if s not in syms))
    k = max(1, (len(syms) - 1).bit_length())
    short = (1 << k) - len(syms)
    lens = [0] * 19
    for i, s in enumerate(syms):
        lens[s] = k - 1 if i < short else k
    return lens


def _write_tokens(w, blk, ends):
    lit, dist = canonical(blk.lit_lens), canonical(blk.dist_lens)
    for t in blk.tokens:
        if isinstance(t, int):
            w.code(lit[t])
        elif t[0] == "lsym":
            w.code(lit[t[1]])
            w.bits(t[3], t[2])
        elif t[0] == "dsym":
            w.code(dist[t[1]])
            w.bits(t[3], t[2])
        elif t[0] == "raw":
            w.bits(t[1], t[2])
        else:
            s, eb, ev = _LSYM[t[0]]
            w.code(lit[s])
            w.bits(ev, eb)
            s, eb, ev = dist_sym(t[1])
            w.code(dist[s])
            w.bits(ev, eb)
        ends.append(w.tell())
    w.code(lit[256])


def _write_block(w, blk, ends):
    w.bits(1 if blk.last else 0, 1)
    w.bits(blk.kind, 2)
    if blk.kind == 0:
        w.align()
        w.bits(len(blk.data), 16)
        w.bits(~len(blk.data), 16)
        w.raw(blk.data)
        return
    if blk.kind == 2:
        syms = blk.cl_symbols if blk.cl_symbols is not None else rle(blk.lit_lens + blk.dist_lens)
        cll = blk.cl_lens if blk.cl_lens is not None else default_cl_lens(syms)
        hclen = blk.hclen
        if hclen is None:
            hclen = max([4] + [i + 1 for i in range(19) if cll[CL_ORDER[i]]])
        assert 4 <= hclen <= 19 and all(cll[CL_ORDER[i]] == 0 for i in range(hclen, 19))
        w.bits(len(blk.lit_lens) - 257, 5)
        w.bits(len(blk.dist_lens) - 1, 5)
        w.bits(hclen - 4, 4)
        for i in range(hclen):
            w.bits(cll[CL_ORDER[i]], 3)
        codes = canonical(cll)
        for s in syms:
            if isinstance(s, tuple):
                w.code(codes[s[0]])
                w.bits(s[1] - (11 if s[0] == 18 else 3), 2 if s[0] == 16 else 3 if s[0] == 17 else 7)
            else:
                w.code(codes[s])
        if blk.bad_header is True:
            return
    _write_tokens(w, blk, ends)


Model = namedtuple("Model", "plain positions n_e room")


def model(blocks):
    """The token model: the plaintext, the output position before every token (all blocks in order), and
    for an invalid stream the output position n_e of the first bad token, where the plaintext ends.  room:
    the output bytes that must be free behind n_e for the error to show -- 1 for a match reaching too far
    back (zlib wants room for a match's first byte before it looks where the match reads), else 0."""
    out, positions = bytearray(), []
    pending = None
    for blk in blocks:
        if blk.bad_header:
            return Model(bytes(out), positions, len(out), 0)
        out += blk.data
        for t in blk.tokens:
            positions.append(len(out))
            if isinstance(t, int):
                assert pending is None
                out.append(t)
                continue
            if t[0] == "raw":
                return Model(bytes(out), positions, len(out), 0)
            if t[0] == "lsym":
                assert pending is None
                if not 257 <= t[1] <= 285:
                    return Model(bytes(out), positions, len(out), 0)
                pending = LEN_BASE[t[1] - 257] + t[3]
                continue
            if t[0] == "dsym":
                if t[1] > 29:
                    return Model(bytes(out), positions, len(out), 0)
                L, D, pending = pending, DIST_BASE[t[1]] + t[3], None
            else:
                assert pending is None
                L, D = t
            if D > len(out):
                return Model(bytes(out), positions, len(out), 1)
            for _ in range(L):
                out.append(out[-D])
        assert pending is None
    return Model(bytes(out), positions, None, 0)


def header(cmf=0x78, flg=0x80):
    flg &= 0xE0
    return bytes([cmf, flg + (31 - ((cmf << 8) + flg) % 31) % 31])


def zstream(blocks, ends=None):
    """RFC 1950 around the blocks; ends (a list) receives the bit offset, from the stream's first byte,
    behind every token"""
    w = Bits()
    w.raw(header())
    e = [] if ends is None else ends
    for blk in blocks:
        _write_block(w, blk, e)
    return w.done() + struct.pack(">I", zlib.adler32(model(blocks).plain))


def check_valid(blocks, name=""):
    """(stream, plaintext): zlib decodes it to its end, to exactly the model's plaintext"""
    s, m = zstream(blocks), model(blocks)
    assert m.n_e is None, name
    d = zlib.decompressobj()
    got = d.decompress(s)
    assert d.eof and got == m.plain and not d.unused_data, (name, len(got), len(m.plain))
    return s, m.plain


def check_invalid(blocks, needle, name=""):
    """(stream, n_e): zlib raises with `needle` in its message"""
    s, m = zstream(blocks), model(blocks)
    assert m.n_e is not None, name
    try:
        zlib.decompressobj().decompress(s)
    except zlib.error as e:
        assert needle in str(e), (name, str(e))
    else:
        raise AssertionError(f"{name}: zlib accepts it")
    return s, m.n_e


# -------------------------------------------------------------- table shapes
def table_shape(lens, root):
    """From the canonical codes alone: ({second-level widths}, total entries) under the layout
    inflate_common.hpp restates from zlib -- the codes longer than `root` bits that share their first
    `root` bits own one table of 2^(longest of them - root) entries behind the 2^root of the first level."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    longest = {}
    for l in lens:
        if l:
            c = nxt[l]
            nxt[l] += 1
            if l > root:
                p = c >> (l - root)
                longest[p] = max(longest.get(p, 0), l)
    return {l - root for l in longest.values()}, (1 << root) + sum(1 << (l - root) for l in longest.values())


def shape_size(count, root):
    """table_shape's total from the counts per length alone (the codes of one length are one run of
    prefixes, the runs in order of length), for the search below"""
    code, size, claimed = 0, 1 << root, 1 << 30
    runs = []
    for l in range(1, 16):
        code <<= 1
        if l > root and count[l]:
            runs.append((l, code >> (l - root), (code + count[l] - 1) >> (l - root)))
        code += count[l]
    for l, a, b in reversed(runs):
        b = min(b, claimed - 1)
        if b >= a:
            size += (b - a + 1) << (l - root)
        claimed = min(claimed, a)
    return size


def random_counts(r, n, deep=0.5):
    """counts per length of a random complete set of n codes, none longer than 15 bits: a leaf is split
    until there are n, a deepest one with probability `deep`"""
    assert 2 <= n
    count = [0] * 16
    count[1] = 2
    for _ in range(n - 2):
        ls = [l for l in range(1, 15) if count[l]]
        l = ls[-1] if r.random() < deep else r.choice(ls)
        count[l] -= 1
        count[l + 1] += 2
    return count


def lens_from_counts(count, nsyms, r, must=()):
    """the lengths of `count` on random symbols of 0..nsyms-1, `must` among them, in random order"""
    n = sum(count[1:])
    assert len(must) <= n <= nsyms
    syms = list(must) + r.sample([s for s in range(nsyms) if s not in must], n - len(must))
    ls = [l for l in range(1, 16) for _ in range(count[l])]
    r.shuffle(ls)
    lens = [0] * nsyms
    for s, l in zip(syms, ls):
        lens[s] = l
    return lens


def search_largest(root, nmax, seed, steps):
    """A bounded seeded search for the complete set of at most nmax codes (none longer than 15 bits) with
    the largest table at `root`: hill climbing over the counts per length, a split of one code into two a
    bit longer or a merge of two into one a bit shorter, restarted from random sets.  -> (size, counts)"""
    r = random.Random(seed)
    best, best_c = 0, None
    cur, cur_s = None, 0
    for step in range(steps):
        if cur is None or step % 400 == 0:
            cur = random_counts(r, r.randint(max(2, nmax // 2), nmax), r.random())
            cur_s = shape_size(cur, root)
        c = list(cur)
        for _ in range(r.randint(1, 3)):
            if r.random() < 0.5:
                ls = [l for l in range(1, 15) if c[l]]
                if ls and sum(c) < nmax:
                    l = r.choice(ls)
                    c[l] -= 1
                    c[l + 1] += 2
            else:
                ls = [l for l in range(2, 16) if c[l] >= 2]
                if ls and sum(c) > 2:
                    l = r.choice(ls)
                    c[l] -= 2
                    c[l - 1] += 1
        s = shape_size(c, root)
        if s >= cur_s:
            cur, cur_s = c, s
            if s > best:
                best, best_c = s, list(c)
    return best, best_c
