"""The corpus of deflate forms that zlib's own compressor never emits, for
tests/test_inflate_forms_cpu.py (host) and tests/test_inflate_forms_gpu.py
(device): streams written by tests/deflate_build.py, each with zlib's answer.

Everything is seeded and built once (each family on first use, then kept).  A
case is (name, stream, cap, status, bytes): what the library must answer for
`stream` with room for `cap` bytes.  Every valid stream went through
deflate_build.check_valid and every invalid one through check_invalid, so the
status and the bytes are zlib's; the token model only says where to put `cap`.
"""
from __future__ import annotations

import functools
import random
import struct
import zlib

import deflate_build as B
import inflate_cases as K

OK, DATA, SHORT, SPACE = K.OK, K.EINFLATE_DATA, K.EINFLATE_SHORT, K.EINFLATE_SPACE
ROOM = 300  # capacity behind the first bad token of an invalid stream: more than one match


def valid_case(name, blocks, room=0):
    s, plain = B.check_valid(blocks, name)
    return (name, s, len(plain) + room, OK, plain)


def invalid_case(name, blocks, needle):
    s, n_e = B.check_invalid(blocks, needle, name)
    return (name, s, n_e + ROOM, DATA, b"")


def zlib_case(name, stream, cap):
    """a case whose answer is zlib's under an ample capacity (prefixes, flips)"""
    st, out = K.expected(stream)
    assert len(out) <= cap, name
    return (name, stream, cap, st, out)


@functools.lru_cache(None)
def prelude():
    """32 KiB that do not compress: the history every distance can reach into"""
    return K.splitmix(32768, 77)


# ------------------------------------------------------------------- a. match grid
GRID_D = (1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 259, 511, 513)
GRID_L = (3, 4, 5, 10, 63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 193, 255, 256, 257, 258)


@functools.lru_cache(None)
def match_grid():
    """fixed blocks: `pre` literals, (L, D), (L, 1), (3, L); and the twin one literal short: too far back"""
    r = random.Random(61)
    valid, invalid = [], []
    for D in GRID_D:
        for L in GRID_L:
            for pre in (D, D + 1, D + 63, D + 64):
                toks = list(r.randbytes(pre)) + [(L, D), (L, 1), (3, L)]
                valid.append(valid_case(f"grid D={D} L={L} pre={pre}", [B.fixed(toks, last=True)]))
            toks = list(r.randbytes(D - 1)) + [(L, D), (L, 1), (3, L)]
            invalid.append(invalid_case(f"grid D={D} L={L} pre={D - 1}", [B.fixed(toks, last=True)],
                                        "invalid distance too far back"))
    return valid, invalid


# ------------------------------------------------- b. every length and distance symbol
@functools.lru_cache(None)
def symbol_extremes():
    r = random.Random(62)
    pre = B.stored(prelude())
    cases = []
    for i in range(29):
        eb = B.LEN_EXTRA[i]
        for ev in sorted({0, (1 << eb) - 1}):
            ds = (7 * i + ev) % 30
            toks = [("lsym", 257 + i, eb, ev), ("dsym", ds, B.DIST_EXTRA[ds], r.randrange(1 << B.DIST_EXTRA[ds]))]
            cases.append(valid_case(f"length symbol {257 + i} extra {ev}", [pre, B.fixed(toks + [0x55], last=True)]))
    cases.append(valid_case("length 257 as 284 + 30", [pre, B.fixed([("lsym", 284, 5, 30), ("dsym", 0, 0, 0)], last=True)]))
    for s in range(30):
        eb = B.DIST_EXTRA[s]
        for ev in sorted({0, (1 << eb) - 1}):
            L = r.choice((3, 64, 65, 258))
            name = "D = 32768 at pos 32768" if (s, ev) == (29, 8191) else f"distance symbol {s} extra {ev}"
            cases.append(valid_case(name, [pre, B.fixed([("lsym",) + B.len_sym(L), ("dsym", s, eb, ev)], last=True)]))
    wrap = [(258, 32768)] * 130 + [(257, 32768), (3, 32768), (258, 1), (258, 32768)]
    case = valid_case("D = 32768 past position 65521", [pre, B.fixed(wrap, last=True)])
    assert len(case[4]) > 65521 + 3 * 258
    cases.append(case)
    return cases


# ------------------------------------------------------------------ c. table shapes
def use_all(lit_lens, dist_lens, r, pos):
    """tokens using every symbol that has a code at least once, where the history (pos bytes so far)
    allows the distance: the literals, then every length symbol, the distance symbols in turn"""
    toks = [s for s in range(256) if s < len(lit_lens) and lit_lens[s]]
    r.shuffle(toks)
    pos += len(toks)
    lsyms = [s for s in range(257, min(len(lit_lens), 286)) if lit_lens[s]]
    dsyms = [s for s in range(min(len(dist_lens), 30)) if dist_lens[s]]
    r.shuffle(lsyms)
    todo = list(dsyms)
    k = 0
    while lsyms and dsyms and (k < len(lsyms) or (todo and k < 120)):
        ls = lsyms[k % len(lsyms)]
        k += 1
        fits = [s for s in (todo or dsyms) if B.DIST_BASE[s] <= pos] or [s for s in dsyms if B.DIST_BASE[s] <= pos]
        if not fits:
            break
        ds = fits[0] if todo and fits[0] in todo else r.choice(fits)
        if ds in todo:
            todo.remove(ds)
        eb = B.LEN_EXTRA[ls - 257]
        ev = r.randrange(1 << eb)
        room = min(pos - B.DIST_BASE[ds], (1 << B.DIST_EXTRA[ds]) - 1)
        toks += [("lsym", ls, eb, ev), ("dsym", ds, B.DIST_EXTRA[ds], r.randint(0, room))]
        pos += B.LEN_BASE[ls - 257] + ev
    return toks


def chain(m):
    """counts of the complete set 1, 2, ..., m - 1, m, m"""
    c = [0] * 16
    for l in range(1, m):
        c[l] = 1
    c[m] = 2
    return c


def counts_of(d):
    c = [0] * 16
    for l, n in d.items():
        c[l] = n
    assert sum(n << (15 - l) for l, n in d.items()) == 32768, d
    return c


# more than 256 codes, 256 and 280 of them longer than 9 bits, many of one length
BIG_A = counts_of({1: 1, 5: 8, 6: 5, 10: 128, 11: 64, 12: 64})
BIG_B = counts_of({1: 1, 3: 1, 4: 4, 10: 100, 11: 20, 13: 128, 14: 32})
N_RANDOM = 320
SEARCH_STEPS = 12000


@functools.lru_cache(None)
def searched():
    """((size, counts) at root 9 over 286 codes, (size, counts) at root 6 over 30 codes)"""
    return B.search_largest(9, 286, 1951, SEARCH_STEPS), B.search_largest(6, 30, 1952, SEARCH_STEPS)


@functools.lru_cache(None)
def table_sets():
    """[(name, lit_lens, dist_lens, with prelude)]: the code-length sets of family c"""
    r = random.Random(63)
    sets = []
    for i in range(9):  # ladders: one second-level table of width w, every length 10 .. 9 + w in it
        wl, wd = 1 + i % 6, 1 + i
        nlen, ndist = (257, 286)[i % 2], (30, 6 + wd + 1)[i % 2]
        sets.append((f"ladder widths {wl} / {wd}", B.lens_from_counts(chain(9 + wl), nlen, r, must=(256,)),
                     B.lens_from_counts(chain(6 + wd), ndist, r), i % 3 == 0))
    sets.append(("big A, nlen 286, ndist 30", B.lens_from_counts(BIG_A, 286, r, must=(256,)),
                 B.lens_from_counts(B.random_counts(r, 30, 0.8), 30, r), True))
    sets.append(("big B, every symbol coded", B.lens_from_counts(BIG_B, 286, r, must=(256,)),
                 B.lens_from_counts(chain(15), 30, r), False))
    sets.append(("nlen 257, ndist 1", B.lens_from_counts(B.random_counts(r, 257, 0.3), 257, r, must=(256,)), [0], False))
    sets.append(("nlen 286, ndist 1, one code", B.lens_from_counts(B.random_counts(r, 200, 0.6), 286, r, must=(256, 257)),
                 [1], False))
    (s9, c9), (s6, c6) = searched()
    sets.append((f"largest found: {s9} / {s6}", B.lens_from_counts(c9, 286, r, must=(256,)),
                 B.lens_from_counts(c6, 30, r), True))
    for i in range(N_RANDOM):
        n = r.choice((r.randint(2, 286), r.randint(2, 40), r.randint(200, 286)))
        nlen = r.randint(max(257, n), 286) if i % 4 else (286 if n > 257 else 257)
        nd = r.randint(2, 30)
        ndist = r.randint(nd, 30)
        must = (256,) if n < 3 or r.random() < 0.3 else (256, r.randint(257, nlen - 1)) if nlen > 257 else (256,)
        sets.append((f"random {i}: {n} / {nd}", B.lens_from_counts(B.random_counts(r, n, r.random()), nlen, r, must=must),
                     B.lens_from_counts(B.random_counts(r, nd, r.random()), ndist, r), i % 10 == 0))
    return sets


@functools.lru_cache(None)
def table_shapes():
    r = random.Random(64)
    cases = []
    for name, lit, dist, far in table_sets():
        toks = use_all(lit, dist, r, 32768 if far else 0)
        blocks = ([B.stored(prelude())] if far else []) + [B.dynamic(toks, lit, dist, last=True)]
        cases.append(valid_case(name, blocks))
    return cases


# --------------------------------------------------------------- d. degenerate sets
def _lens(n, d):
    lens = [0] * n
    for s, l in d.items():
        lens[s] = l
    return lens


@functools.lru_cache(None)
def degenerate():
    two = _lens(257, {65: 1, 256: 1})
    with_len = _lens(258, {65: 1, 256: 2, 257: 2})
    pad = B.stored(bytes(60), last=True)  # bits behind a header that is refused only once they are read
    cases = [
        valid_case("only the end-of-block code, one bit", [B.dynamic([], _lens(257, {256: 1}), [0], last=True)]),
        valid_case("an empty block, then data", [B.dynamic([], _lens(257, {256: 1}), [0]), B.fixed([1, 2, 3], last=True)]),
        valid_case("one literal and end-of-block", [B.dynamic([65] * 70, two, [0], last=True)]),
        valid_case("no distance code, literals only", [B.dynamic([65] * 5, with_len, [0], last=True)]),
        invalid_case("no distance code, a length symbol used",
                     [B.dynamic([65] * 5 + [("lsym", 257, 0, 0), ("raw", 0, 1)], with_len, [0], last=True), pad],
                     "invalid distance code"),
        valid_case("one distance code of one bit, used", [B.dynamic([65] * 5 + [(3, 1), (3, 1)], with_len, [1], last=True)]),
        valid_case("one distance code of one bit, symbol 1", [B.dynamic([65] * 5 + [(3, 2)], with_len, [0, 1], last=True)]),
        invalid_case("one distance code of one bit, its missing sibling used",
                     [B.dynamic([65] * 5 + [("lsym", 257, 0, 0), ("raw", 1, 1)], with_len, [1], last=True), pad],
                     "invalid distance code"),
        invalid_case("one distance code of two bits", [B.dynamic([], with_len, [2], last=True, bad_header="tail")],
                     "invalid distances set"),
        invalid_case("over-subscribed distance set", [B.dynamic([], with_len, [1, 1, 1], last=True, bad_header=True), pad],
                     "invalid distances set"),
        invalid_case("over-subscribed literal/length set",
                     [B.dynamic([], _lens(257, {0: 1, 1: 1, 256: 1}), [1], last=True, bad_header=True), pad],
                     "invalid literal/lengths set"),
        # an empty code-length code decodes every length as 0, one bit each: no end-of-block code
        invalid_case("all 19 code-length lengths zero",
                     [B.dynamic([], two, [0], last=True, cl_symbols=[], cl_lens=[0] * 19, hclen=19, bad_header=True), pad],
                     "missing end-of-block"),
        # HCLEN = 4 sends 16, 17, 18 and 0 only: every length is 0
        invalid_case("HCLEN = 4",
                     [B.dynamic([], [0] * 257, [0], last=True, cl_symbols=[(18, 138), (18, 120)],
                                cl_lens=_lens(19, {18: 1, 0: 1}), hclen=4, bad_header=True), pad],
                     "missing end-of-block"),
        invalid_case("HCLEN = 4, 16 first",
                     [B.dynamic([], [0] * 257, [0], last=True, cl_symbols=[(16, 3)],
                                cl_lens=_lens(19, {16: 1, 0: 1}), hclen=4, bad_header=True), pad],
                     "invalid bit length repeat"),
    ]
    return cases


# ------------------------------------------------------------- e. code-length coding
class _CL:
    """the code-length symbols as they are sent, and the lengths they give"""

    def __init__(self):
        self.syms, self.lens = [], []

    def put(self, *vs):
        self.syms += vs
        self.lens += vs
        return self

    def rep(self, sym, k):
        self.syms.append((sym, k))
        self.lens += [self.lens[-1] if sym == 16 else 0] * k
        return self


def _full_cl_lens(r):
    """a complete code over all 19 code-length symbols with 7-bit codes in it"""
    c = [0] * 8
    c[1] = 2
    for _ in range(17):
        l = max(l for l in range(1, 7) if c[l])
        c[l] -= 1
        c[l + 1] += 2
    ls = [l for l in range(1, 8) for _ in range(c[l])]
    assert len(ls) == 19 and max(ls) == 7 and sum(128 >> l for l in ls) == 128
    r.shuffle(ls)
    return ls


@functools.lru_cache(None)
def code_length_coding():
    r = random.Random(65)
    # 286 + 30 lengths.  18 x 138, 16 x 6, 18 x 11, 16 x 3, 17 x 3, 16 behind a 17, 17 x 10; a 16 run over
    # the boundary (lit 284, 285, dist 0, 1, 2); an 18 run ending exactly at the 316th length
    a = _CL().rep(18, 138).put(4).rep(16, 6).rep(18, 11).put(4).rep(16, 3).rep(17, 3).rep(16, 3).put(5, 5)
    a.rep(17, 10).rep(18, 78).put(3, 4, 6).rep(18, 24).put(6).rep(16, 5).put(1, 2, 3, 4, 6)
    over = _CL()
    over.syms, over.lens = a.syms + [(18, 23)], a.lens + [0] * 23
    a.rep(18, 22)
    assert len(a.lens) == 316 and B.kraft(a.lens[:286]) == 32768 and B.kraft(a.lens[286:]) == 32768
    # 270 + 7 lengths.  a 16 behind an 18, an 18 run over the boundary (lit 258 .. 269, dist 0 .. 4)
    b = _CL().rep(18, 138).rep(16, 3).put(1).rep(18, 114).put(2, 2).rep(18, 17).put(1, 1)
    assert len(b.lens) == 277 and B.kraft(b.lens[:270]) == 32768 and B.kraft(b.lens[270:]) == 32768
    cases = []
    for tag, cl_lens in (("", None), (", 7-bit code-length codes", _full_cl_lens(r))):
        hclen = 19 if cl_lens else None
        toks = use_all(a.lens[:286], a.lens[286:], r, 0)
        cases.append(valid_case("runs of every kind, 16 over the boundary, a run ending at the last length" + tag,
                                [B.dynamic(toks, a.lens[:286], a.lens[286:], last=True, cl_symbols=a.syms,
                                           cl_lens=cl_lens, hclen=hclen)]))
        toks = [141] * 10 + [("lsym", 257, 0, 0), ("dsym", 5, 1, 0), ("lsym", 257, 0, 0), ("dsym", 6, 2, 3)]
        cases.append(valid_case("16 behind an 18, 18 over the boundary" + tag,
                                [B.dynamic(toks, b.lens[:270], b.lens[270:], last=True, cl_symbols=b.syms,
                                           cl_lens=cl_lens, hclen=hclen)]))
        cases.append(invalid_case("a run passing the last length by one" + tag,
                                  [B.dynamic([], over.lens[:286], over.lens[286:316], last=True, cl_symbols=over.syms,
                                             cl_lens=cl_lens, hclen=hclen, bad_header="tail")],
                                  "invalid bit length repeat"))  # (a decoder that lets the run pass answers OK)
    return cases


# ------------------------------------------------------------ f. blocks and the reader
SMALL_LIT = _lens(257, {97: 1, 98: 2, 99: 3, 256: 3})


@functools.lru_cache(None)
def phase_stream():
    """One stream: for k in 1, 63, 64 and each of the 8 bit phases, a stored block (so nothing is pending),
    e empty fixed blocks of 10 bits, a fixed or dynamic block of k literals, and the stored block whose
    header they push to that phase.  -> (blocks, [(k, index of the stored block behind the k literals)])"""
    r = random.Random(66)
    blocks, marks = [], []
    for k in (1, 63, 64):
        for e in range(4):
            for nine in (0, 1):
                blocks.append(B.stored(r.randbytes(r.randint(0, 9))))
                blocks += [B.fixed([])] * e
                lits = [r.randrange(144, 256)] * nine + [r.randrange(144) for _ in range(k - nine)]
                r.shuffle(lits)
                blocks.append(B.fixed(lits))
                marks.append((k, len(blocks)))
                blocks.append(B.stored(r.randbytes(r.randint(1, 70))))
                # the same behind a dynamic block: a literal is 1, 2 or 3 bits
                lits = [r.choice((97, 98, 99)) for _ in range(k)]
                blocks.append(B.dynamic(lits, SMALL_LIT, [0]))
                marks.append((k, len(blocks)))
                blocks.append(B.stored(r.randbytes(r.randint(1, 70))))
    blocks.append(B.fixed([(40, 33), 7, (258, 1)], last=True))
    return blocks, marks


def block_starts(blocks):
    """the bit offset of every block's header in zstream(blocks), by writing the blocks one more at a time"""
    w = B.Bits()
    w.raw(B.header())
    starts = []
    for blk in blocks:
        starts.append(w.tell())
        B._write_block(w, blk, [])
    return starts


@functools.lru_cache(None)
def blocks_and_reader():
    r = random.Random(67)
    cases = [valid_case("300 empty fixed blocks before data", [B.fixed([])] * 300 + [B.fixed(list(r.randbytes(100)) + [(9, 50)], last=True)])]
    cases.append(valid_case("stored at every bit phase with 1, 63, 64 literals pending", phase_stream()[0]))
    cases.append(valid_case("LEN 0, not last", [B.stored(b""), B.fixed([1, 2, (3, 2)], last=True)]))
    cases.append(valid_case("LEN 0, last", [B.fixed([1, 2, (3, 2)]), B.stored(b"", last=True)]))
    cases.append(valid_case("only LEN 0", [B.stored(b"", last=True)]))
    cases.append(valid_case("LEN 65535", [B.stored(K.splitmix(65535, 78)), B.fixed([(258, 65535 - 32768), 9], last=True)]))
    for off in list(range(252, 260)) + list(range(508, 516)):
        # header 2, stored header 5: the block behind the payload starts at message byte `off`
        blocks = [B.stored(r.randbytes(off - 7)), B.fixed(list(r.randbytes(40)) + [(30, 17), (200, 1)], last=True)]
        case = valid_case(f"the block behind a stored payload at message byte {off}", blocks)
        assert block_starts(blocks)[1] == 8 * off
        cases.append(case)
        blocks = [B.stored(r.randbytes(off - 7)), B.stored(r.randbytes(300)), B.dynamic([97, 98, 99] * 30, SMALL_LIT, [0], last=True)]
        cases.append(valid_case(f"a stored block behind a stored payload at message byte {off}", blocks))
    sets = {n: (l, d) for n, l, d, _ in table_sets()[:11]}
    big, small = sets["big A, nlen 286, ndist 30"], sets["ladder widths 1 / 1"]
    cases.append(valid_case("dynamic, fixed, dynamic with shorter tables",
                            [B.dynamic(use_all(big[0], big[1], r, 0), big[0], big[1]), B.fixed([(258, 300), 5]),
                             B.dynamic(use_all(small[0], small[1], r, 5000), small[0], small[1]),
                             B.dynamic(use_all(small[0], [0], r, 0), small[0], [0], last=True)]))
    return cases


# ------------------------------------------------------------ g. prefixes and flips
@functools.lru_cache(None)
def prefix_streams():
    """six streams under 400 bytes: four of c, two of f"""
    c = {n: s for n, s, *_ in table_shapes()}
    picks = [c["ladder widths 2 / 2"], c["ladder widths 6 / 6"]]
    picks += [s for n, s, *_ in table_shapes() if n.startswith("random") and 150 <= len(s) < 400][:2]
    f = {n: s for n, s, *_ in blocks_and_reader() if len(s) < 400}
    picks += [max(f.values(), key=len), f["LEN 0, last"]]
    assert len(picks) == 6 and all(len(s) < 400 for s in picks)
    return picks


@functools.lru_cache(None)
def prefixes():
    cases = []
    for i, s in enumerate(prefix_streams()):
        cap = len(K.expected(s)[1])
        cases += [zlib_case(f"prefix {n} of stream {i}", s[:n], cap) for n in range(len(s) + 1)]
    return cases


FLIP_SEEDS = (5, 6)


@functools.lru_cache(None)
def flip_streams():
    """two streams of c under 260 bytes whose code lengths reach 15 bits in both sets"""
    picks = []
    for (name, lit, dist, far), case in zip(table_sets(), table_shapes()):
        if not far and max(lit) == 15 and max(dist) == 15 and 120 <= len(case[1]) < 260:
            picks.append(case[1])
    assert len(picks) >= 2
    return picks[:2]


def flip_set(s, count, seed):
    """[(stream, status, bytes)]: single-bit flips of the deflate body of s under the rule of
    inflate_cases.mutations: a flipped body that raw zlib still decodes to its end gets the Adler-32 of what
    it produced, the others keep the stream as it stands; what is expected is zlib's answer either way"""
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
            stream = s[:2] + m[:len(m) - len(d.unused_data)] + struct.pack(">I", zlib.adler32(got))
        else:
            stream = s[:2] + m + s[-4:]
        out.append((stream,) + K.expected(stream))
    return out


@functools.lru_cache(None)
def flips():
    cases = []
    for i, (s, seed) in enumerate(zip(flip_streams(), FLIP_SEEDS)):
        cases += [(f"flip {j} of stream {i}", m, K.mutation_cap(m), st, out)
                  for j, (m, st, out) in enumerate(flip_set(s, 256, seed))]
    return cases


# ---------------------------------------------------------------------- h. capacity
def model_cap(n, n_e, cap, room=0):
    """The token model's answer for a whole stream of n plaintext bytes (n_e: the output position of its
    first bad token, None for a valid one; room: deflate_build.model's) under a capacity: SPACE iff a byte
    is demanded at or past cap before the error or the end."""
    if n_e is None:
        return OK if cap >= n else SPACE
    return DATA if cap >= n_e + room else SPACE


@functools.lru_cache(None)
def capacity():
    """-> (cases, [(stream, n, n_e, room)] of the whole streams, for the agreement of expected_cap and the model)"""
    r = random.Random(68)
    lit, dist = next((l, d) for n, l, d, _ in table_sets() if n == "ladder widths 4 / 4")
    text = list(K.text(120, 69))
    dyn = [s for s in range(256) if lit[s]]
    dyn_toks = [r.choice(dyn) for _ in range(100)]
    lsyms = [s for s in range(257, 286) if s < len(lit) and lit[s]]
    dsyms = [s for s in range(30) if s < len(dist) and dist[s] and B.DIST_BASE[s] <= 90]
    for _ in range(12 if lsyms and dsyms else 0):
        ls, ds = r.choice(lsyms), r.choice(dsyms)
        if B.LEN_BASE[ls - 257] > 40:
            continue
        dyn_toks += [("lsym", ls, B.LEN_EXTRA[ls - 257], 0), ("dsym", ds, B.DIST_EXTRA[ds], 0), r.choice(dyn)]
    dyn_toks += [r.choice(dyn) for _ in range(300 - len(B.model([B.dynamic(dyn_toks, lit, dist)]).plain))]
    valid = [
        ("fixed with matches", [B.fixed(text + [(70, 100), (5, 1), 66, (100, 64), 67, (3, 3)], last=True)]),
        ("dynamic", [B.dynamic(dyn_toks, lit, dist, last=True)]),
        ("mixed with stored", [B.fixed(text[:50] + [(20, 7)]), B.stored(r.randbytes(90)), B.stored(b""),
                               B.dynamic([97, 98, 99] * 20, SMALL_LIT, [0]), B.stored(r.randbytes(37)),
                               B.fixed([(65, 64), 1, 2, 3], last=True)]),
    ]
    cases, whole = [], []
    for name, blocks in valid:
        s, plain = B.check_valid(blocks, name)
        assert 200 <= len(plain) <= 400, (name, len(plain))
        whole.append((s, len(plain), None, 0))
    bad = [
        ("too far back, fixed", [B.fixed(text[:60] + [(10, 61)], last=True)], "too far back"),
        ("too far back behind a match", [B.fixed(text[:60] + [(130, 60), (4, 191)], last=True)], "too far back"),
        ("too far back behind stored", [B.stored(r.randbytes(200)), B.fixed([1, (3, 202)], last=True)], "too far back"),
        ("length symbol 286", [B.fixed(text[:70] + [(64, 64), ("lsym", 286, 0, 0)], last=True)], "invalid literal/length code"),
        ("distance symbol 30", [B.fixed(text[:90] + [("lsym", 270, 2, 1), ("dsym", 30, 0, 0)], last=True)], "invalid distance code"),
        ("a refused header behind data", [B.fixed(text + [(150, 120)]), B.dynamic([], SMALL_LIT, [2], last=True, bad_header=True),
                                          B.stored(bytes(60), last=True)], "invalid distances set"),
        ("block type 3 behind data", None, "invalid block type"),
        ("stored lengths behind data", None, "invalid stored block lengths"),
        ("wrong Adler-32", None, "incorrect data check"),
        ("no distance code behind literals", [B.stored(r.randbytes(64)), B.dynamic([97] * 64 + [98, ("lsym", 257, 0, 0), ("raw", 0, 1)],
                                                                                   _lens(258, {97: 1, 98: 2, 256: 3, 257: 3}), [0], last=True),
                                              B.stored(bytes(60), last=True)], "invalid distance code"),
    ]
    for name, blocks, needle in bad:
        room = 0
        if blocks is not None:
            s, n_e = B.check_invalid(blocks, needle, name)
            room = B.model(blocks).room
        else:  # a good stream's head with the error patched in behind it
            head = [B.fixed(text + [(100, 3)])]
            n_e = len(B.model(head).plain)
            if name.startswith("block type 3"):
                w = B.Bits()
                w.raw(B.header())
                B._write_block(w, head[0], [])
                w.bits(1, 1)
                w.bits(3, 2)
                s = w.done() + bytes(8)
            elif name.startswith("stored lengths"):
                s = B.zstream(head + [B.stored(b"abcdef", last=True)])
                at = s.rindex(b"abcdef")
                s = s[:at - 1] + bytes([s[at - 1] ^ 0x10]) + s[at:]
            else:
                s = B.zstream(head + [B.fixed([], last=True)])
                s = s[:-1] + bytes([s[-1] ^ 1])
            try:
                zlib.decompressobj().decompress(s)
            except zlib.error as e:
                assert needle in str(e), (name, str(e))
            else:
                raise AssertionError(name)
        assert 50 <= n_e <= 300, (name, n_e)
        whole.append((s, None, n_e, room))
    for s, n, n_e, room in whole:
        top = n + 1 if n_e is None else n_e + 2
        for cap in range(top + 1):
            if cap == 0:
                st = model_cap(n, n_e, 0, room)
                out = b"" if st != OK else K.expected(s)[1]
            else:
                st, out = K.expected_cap(s, cap)
            cases.append((f"cap {cap}", s, cap, st, out))
    shorts = 0
    for s, n, n_e, room in whole[:5]:
        p = s[:len(s) * 2 // 3]
        st, out = K.expected(p)
        assert st == SHORT and len(out) > 20
        shorts += 1
        for cap in range(len(out) - 2, len(out) + 3):
            cases.append((f"short prefix, cap {cap}", p, cap) + K.expected_cap(p, cap))
    assert shorts == 5
    return cases, whole


FAMILIES = ("match_grid", "symbol_extremes", "table_shapes", "degenerate", "code_length_coding", "blocks_and_reader",
            "prefixes", "flips", "capacity")


def family(name):
    """the cases of one family as a list of (name, stream, cap, status, bytes)"""
    got = globals()[name]()
    if name == "match_grid":
        return got[0] + got[1]
    if name == "capacity":
        return got[0]
    return got
