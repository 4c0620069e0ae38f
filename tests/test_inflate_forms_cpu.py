"""vds_ec_inflate_host (inflate_host.cpp) over the deflate forms zlib's own
compressor never emits (tests/inflate_forms.py, written by
tests/deflate_build.py): status, length and bytes against Python's zlib, bit
for bit, and the guard behind the capacity untouched.  The host code shares
inflate_common.hpp -- the table rules -- with k_inflate_batch, which
tests/test_inflate_forms_gpu.py runs over the same corpus.

Also here, needing no library: the conditions the corpus must meet to be worth
running (which table shapes it reaches, which classes its flips hold, where its
stored headers sit), asserted from the table-shape model and from zlib alone,
and the agreement of inflate_cases.expected_cap with the token model."""
import collections
import ctypes as C
import random
import zlib

import numpy as np
import pytest

import deflate_build as B
import inflate_cases as K
import inflate_forms as F

GUARD = 64
FILL = 0xEE

# the largest tables the bounded search of inflate_forms.searched() reaches, recorded when this file was
# written; zlib's bounds (inftrees.h: ENOUGH_LENS, ENOUGH_DISTS) are 852 and 592
SEARCHED_LIT, SEARCHED_DIST = 840, 592


def _run(lib, stream: bytes, cap: int, shift: int = 0):
    """(status, delivered bytes), the stream at `shift` bytes past an aligned address; the guard behind the
    capacity must be untouched whatever happens"""
    buf = np.full(cap + GUARD, FILL, dtype=np.uint8)
    src = np.zeros(len(stream) + 8, dtype=np.uint8)
    shift += -src.ctypes.data % 4
    src[shift:shift + len(stream)] = np.frombuffer(stream, dtype=np.uint8)
    n = C.c_uint64(0xDEAD)
    st = lib.vds_ec_inflate_host(src.ctypes.data + shift, len(stream), buf.ctypes.data, cap, C.byref(n))
    assert (buf[cap:] == FILL).all(), "a byte at or past the capacity was written"
    assert n.value <= cap
    if st in (K.EINFLATE_DATA, K.EINFLATE_SPACE):
        assert n.value == 0
    return st, buf[:n.value].tobytes()


@pytest.mark.parametrize("name", F.FAMILIES)
def test_family(vds_lib, name):
    cases = F.family(name)
    shifts = (0, 1, 2, 3) if name == "blocks_and_reader" else (0,)
    for i, (what, s, cap, st, out) in enumerate(cases):
        for shift in shifts:
            assert _run(vds_lib, s, cap, shift) == (st, out), (name, i, what, "cap", cap, "shift", shift)
    if name == "match_grid":  # a valid match is SPACE one byte short, whatever is pending
        for i, (what, s, cap, st, out) in enumerate(cases[:2052:7]):
            assert _run(vds_lib, s, cap - 1) == (K.EINFLATE_SPACE, b""), (name, i, what)


def test_corpus_sizes():
    sizes = {name: len(F.family(name)) for name in F.FAMILIES}
    assert sizes["match_grid"] == len(F.GRID_D) * len(F.GRID_L) * 5 == 2565
    assert sizes["symbol_extremes"] >= 29 + 30 + 2 and sizes["table_shapes"] >= 300 + 14
    assert sizes["prefixes"] > 6 * 100 and sizes["flips"] == 512 and sizes["capacity"] > 2000
    valid, invalid = F.match_grid()
    assert all(c[3] == 0 for c in valid) and all(c[3] == K.EINFLATE_DATA for c in invalid)


def test_table_shape_conditions():
    """what family c must reach, from the table-shape model alone"""
    sets = F.table_sets()
    lit_w, dist_w = set(), set()
    for name, lit, dist, far in sets:
        assert max(lit) <= 15 and max(dist) <= 15
        w, size = B.table_shape(lit, 9)
        assert size <= 852, name  # zlib's bound, which sizes the library's tables
        lit_w |= w
        w, size = B.table_shape(dist, 6)
        assert size <= 592, name
        dist_w |= w
    assert lit_w >= set(range(1, 7)) and dist_w >= set(range(1, 10))
    # each ladder alone gives its width, with every length from root + 1 on inside the one table
    for i in range(9):
        name, lit, dist, far = sets[i]
        assert B.table_shape(lit, 9)[0] == {1 + i % 6} and B.table_shape(dist, 6)[0] == {1 + i}, name
        assert {l for l in dist if l > 6} == set(range(7, 7 + 1 + i)), name
    coded = [sum(1 for l in lit if l) for _, lit, _, _ in sets]
    assert any(64 < n <= 128 for n in coded) and any(128 < n <= 256 for n in coded) and any(n > 256 for n in coded)
    assert max(sum(1 for l in lit if l > 9) for _, lit, _, _ in sets) >= 200
    # many codes of one length on both sides of a 64-symbol step: a length held by over 100 symbols
    assert any(max(collections.Counter(l for l in lit if l).values()) > 100 for _, lit, _, _ in sets)
    # (Thirty codes longer than 6 bits weigh at most 30/128, and zlib refuses an incomplete set, so no
    # distance set has ONLY such codes; what is asked is a set with a code of every length 7 .. 15.)
    assert any({l for l in dist if l > 6} == set(range(7, 16)) for _, _, dist, _ in sets)
    assert {len(lit) for _, lit, _, _ in sets} >= {257, 286} and {len(dist) for _, _, dist, _ in sets} >= {1, 30}
    rnd = [s for s in sets if s[0].startswith("random")]
    assert len(rnd) >= 300
    assert sum(1 for _, lit, dist, _ in rnd if max(lit) == 15) >= 100
    assert sum(1 for _, lit, dist, _ in rnd if max(dist) == 15) >= 50
    assert sum(1 for s in sets if s[3]) >= 30  # with the 32 KiB history: every distance symbol usable


def test_searched_table_sizes():
    """the bounded search is seeded: it reaches what it reached when this file was written, and the
    count-based size it climbs on is the table-shape model's"""
    (s9, c9), (s6, c6) = F.searched()
    assert (s9, s6) == (SEARCHED_LIT, SEARCHED_DIST)
    assert sum(c9) <= 286 and sum(c6) <= 30
    name, lit, dist, far = next(s for s in F.table_sets() if s[0].startswith("largest found"))
    assert B.table_shape(lit, 9)[1] == s9 and B.table_shape(dist, 6)[1] == s6
    r = random.Random(3)
    for _ in range(200):
        n = r.randint(2, 286)
        c = B.random_counts(r, n, r.random())
        lens = B.lens_from_counts(c, 286, r)
        for root in (6, 9):
            assert B.table_shape(lens, root)[1] == B.shape_size(c, root)


def test_stored_headers_at_every_phase():
    blocks, marks = F.phase_stream()
    starts = F.block_starts(blocks)
    for k in (1, 63, 64):
        # marks alternate: behind a fixed block, behind a dynamic block
        fixed = {starts[i] % 8 for kk, i in marks[0::2] if kk == k}
        assert fixed == set(range(8)), (k, fixed)
        assert len({starts[i] % 8 for kk, i in marks[1::2] if kk == k}) >= 3
        for kk, i in marks:
            assert blocks[i].kind == 0 and len(blocks[i - 1].tokens) == kk


def test_flip_sets_hold_every_class():
    """from zlib alone (the seeds were chosen for it)"""
    for s in F.flip_streams():
        assert len(s) < 400
    by = [c[3] for c in F.flips()]
    assert len(by) == 512
    assert by.count(0) >= 20 and by.count(K.EINFLATE_DATA) >= 20 and by.count(K.EINFLATE_SHORT) >= 5


def test_prefix_streams():
    for s in F.prefix_streams():
        assert len(s) < 400
    by = collections.Counter(c[3] for c in F.prefixes())
    assert by[0] == 6 and by[K.EINFLATE_SHORT] > 600 and by[K.EINFLATE_DATA] == 0


def test_expected_cap_agrees_with_the_token_model():
    """for every whole stream of family h and every cap >= 1: zlib's answer under a capacity is the token
    model's.  (cap = 0, which Python's zlib cannot be asked, is the model's alone.)"""
    cases, whole = F.capacity()
    assert len(whole) == 13
    n_checked = 0
    for s, n, n_e, room in whole:
        plain = K.expected(s)[1] if n_e is None else b""
        for cap in range(1, (n + 1 if n_e is None else n_e + 2) + 1):
            st, out = K.expected_cap(s, cap)
            assert st == F.model_cap(n, n_e, cap, room), (n, n_e, cap, st)
            assert out == (plain if st == 0 else b"")
            n_checked += 1
    assert n_checked > 2000
    # the three answers of the issue's own trial: a valid stream, a wrong trailer, a half stream
    s = K.deflate(K.text(300, 30))
    assert [K.expected_cap(s, c)[0] for c in (1, 299, 300, 301)] == [K.EINFLATE_SPACE, K.EINFLATE_SPACE, 0, 0]
    bad = s[:-1] + bytes([s[-1] ^ 1])
    assert [K.expected_cap(bad, c)[0] for c in (299, 300, 301)] == [K.EINFLATE_SPACE, K.EINFLATE_DATA, K.EINFLATE_DATA]
    half = s[:len(s) // 2]
    n = len(K.expected(half)[1])
    assert [K.expected_cap(half, c)[0] for c in (n - 1, n, n + 1)] == [K.EINFLATE_SPACE, K.EINFLATE_SHORT, K.EINFLATE_SHORT]


def test_writer_against_zlib_streams():
    """the writer's fixed and stored blocks are the bytes zlib itself writes for the same tokens"""
    data = bytes(range(200))
    assert B.zstream([B.stored(data, last=True)])[2:] == K.deflate(data, level=0)[2:]
    assert B.zstream([B.fixed(list(b"abc"), last=True)])[2:] == K.deflate(b"abc", strategy=zlib.Z_FIXED)[2:]
    m = B.model([B.fixed([1, 2, 3, (5, 2), (3, 9)], last=True)])
    assert m.plain == bytes([1, 2, 3, 2, 3, 2, 3, 2]) and m.positions == [0, 1, 2, 3, 8] and m.n_e == 8
