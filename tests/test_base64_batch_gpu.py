"""base64 wire text on the device (vds_ec_base64_decode_batch_device /
_encode_batch_device, base64.hip): texts of different lengths decoded, and
bytes encoded, in one launch each.

The checker is the library's host decoder vds_ec_base64_decode (pinned against
a restatement of the reference by tests/test_wire.py) and Python's base64.

Layout: every text of a launch lies in ONE device buffer with foreign bytes
('=' and 'A' alternating: a kernel that read them as text would see an event
or decode extra bytes) in the gaps, every output in ONE buffer between 0x5A
guard bytes, and the statuses start as a sentinel, so that a status the launch
did not write shows."""
import base64
import ctypes as C
import random

import numpy as np
import pytest

ALPHA = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"

pytestmark = pytest.mark.gpu

# A valid text long enough for three of the decode kernel's per-iteration
# chunks (kB64DecStep = 1024 characters a wave a step, ec_internal.hpp), so the
# first event is met in the first, a middle and the last step, and at every
# lane and character of a step.  Raise it if the kernel's step grows.
EVENT_SPAN = 3200

TEXT_MOD16 = (0, 1, 2, 3, 4, 8, 12)
OUT_MOD4 = (0, 1, 2, 3)
LENGTHS = list(range(201)) + [765, 768, 771, 3071, 3072, 49149, 65536, 65543]
GUARD = 16
FILL = 0x5A
SENTINEL = 0x5A5A5A5A
EINVAL, EB64_LENGTH, EB64_PADDING, EB64_CHAR = -1, -7, -8, -9


def _host_decode(lib, t: bytes):
    """(status, bytes) of vds_ec_base64_decode: the checker."""
    size = lib.vds_ec_base64_decoded_size(t, len(t))
    out = np.zeros(max(size, 1), dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib.vds_ec_base64_decode(t, len(t), out.ctypes.data, C.byref(n))
    return rc, out[:size]


def _place(lens, mods, align, lead):
    """Offsets of pieces of `lens` bytes, piece i at mods[i] modulo `align`, at least `lead` bytes apart."""
    offs, pos = [], 0
    for ln, m in zip(lens, mods):
        pos = (pos + align - 1) // align * align + align * ((lead + align - 1) // align) + m
        offs.append(pos)
        pos += ln
    return offs, pos + lead + align


def _gather(pieces, offs, total, foreign):
    buf = np.empty(total, dtype=np.uint8)
    if foreign:
        buf[0::2] = ord("=")
        buf[1::2] = ord("A")
    else:
        buf[:] = 0xA5
    for p, off in zip(pieces, offs):
        buf[off:off + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return buf


def _run_decode(torch, lib, texts, declared=None, d_text=None, text_ptrs=None):
    """One decode launch over `texts`, text i at TEXT_MOD16[i % 7] mod 16 and
    its output at OUT_MOD4[(i // 7) % 4] mod 4 (or the texts where they already
    lie on the device: text_ptrs).  Every status against the host function's,
    every output whose status is 0 against the host function's bytes, every
    byte outside the outputs untouched.  declared[i], where given, replaces the
    size passed for text i: that message must come back VDS_EC_EINVAL with its
    output untouched.  Returns (statuses, outputs by message)."""
    from vds_amd import chunk
    count = len(texts)
    sizes = [lib.vds_ec_base64_decoded_size(t, len(t)) for t in texts]
    passed = list(sizes)
    for i, s in (declared or {}).items():
        passed[i] = s
    if text_ptrs is None:
        t_offs, t_total = _place([len(t) for t in texts], [TEXT_MOD16[i % 7] for i in range(count)], 16, 16)
        d_text = torch.from_numpy(_gather(texts, t_offs, t_total, True)).cuda()
        text_ptrs = [d_text.data_ptr() + off for off in t_offs]
        assert d_text.data_ptr() % 16 == 0
    o_offs, o_total = _place(passed, [OUT_MOD4[(i // 7) % 4] for i in range(count)], 4, GUARD)
    want = np.full(o_total, FILL, dtype=np.uint8)
    must = np.ones(o_total, dtype=bool)  # bytes whose value is specified
    want_st = np.zeros(count, dtype=np.int32)
    for i, t in enumerate(texts):
        rc, ref = _host_decode(lib, t)
        if declared and i in declared:
            want_st[i] = EINVAL  # and its output untouched
            continue
        want_st[i] = rc
        if rc == 0:
            want[o_offs[i]:o_offs[i] + sizes[i]] = ref
        else:
            must[o_offs[i]:o_offs[i] + sizes[i]] = False
    d_out = torch.full((o_total,), FILL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 4 == 0
    d_st = torch.full((count,), SENTINEL, dtype=torch.int32, device="cuda")
    chunk.base64_decode_batch_device(text_ptrs, [len(t) for t in texts], [d_out.data_ptr() + o for o in o_offs],
                                     passed, d_st)
    torch.cuda.synchronize()
    st, got = d_st.cpu().numpy(), d_out.cpu().numpy()
    bad = np.flatnonzero(st != want_st)
    assert bad.size == 0, ("status", int(bad[0]), texts[bad[0]][:64], int(st[bad[0]]), int(want_st[bad[0]]))
    wrong = np.flatnonzero((got != want) & must)
    if wrong.size:
        at = int(wrong[0])
        i = int(np.searchsorted(np.asarray(o_offs), at, side="right")) - 1
        raise AssertionError(("bytes", at, "message", i, "offset in it", at - o_offs[max(i, 0)], len(texts[i]),
                              sizes[i], int(got[at]), int(want[at])))
    return st, [got[o:o + s] for o, s in zip(o_offs, passed)]


def _bodies(rng):
    """Every length at every text and output alignment (message i has text
    alignment class i % 7 and output class (i // 7) % 4, so 28 consecutive
    copies of a length meet all of them), the lengths shuffled with the
    shortest and the longest neighbours."""
    lengths = [n for n in LENGTHS if n not in (0, 65543)]
    rng.shuffle(lengths)
    at = len(lengths) // 2
    lengths[at:at] = [65543, 0, 65543]
    data = np.frombuffer(rng.randbytes(max(LENGTHS) + 28 * len(lengths)), dtype=np.uint8)
    return [data[i:i + n].tobytes() for i, n in enumerate(n for n in lengths for _ in range(28))]


def test_decode_every_length_and_alignment(gpu, vds_lib):
    import torch
    bodies = _bodies(random.Random(1))
    assert {len(b) for b in bodies} == set(LENGTHS)
    texts = [base64.b64encode(b) for b in bodies]
    st, outs = _run_decode(torch, vds_lib, texts)
    assert not st.any()
    for b, o in zip(bodies, outs):
        assert o.tobytes() == b, len(b)


def _event_cases(rng):
    forms = [base64.b64encode(rng.randbytes(EVENT_SPAN // 4 * 3 - p)) for p in (0, 1, 2)]
    assert [len(f) for f in forms] == [EVENT_SPAN] * 3 and forms[1].endswith(b"=") and forms[2].endswith(b"==")
    assert b"=" not in forms[0] and forms[1].count(b"=") == 1
    cases = []
    for f in forms:
        for p in range(EVENT_SPAN):
            cases.append(f[:p] + b"=" + f[p + 1:])
    for ch in (b"*", b"\x80"):
        for p in range(EVENT_SPAN):
            cases.append(forms[0][:p] + ch + forms[0][p + 1:])
    # the fixed malformed list and the random short strings of tests/test_wire.py
    cases += [b"", b"=", b"==", b"===", b"====", b"A===", b"AA==", b"AAA=", b"A=AA", b"AB=C", b"QQ==QQ==",
              b"AAAA====", b"ABC=AB==", b"=AA=", b"AAAAAAA=", b"AA*A", b"AA\x80A", b"QUE=", b"QUJD", b"Q", b"QUJDRA"]
    for _ in range(400):
        n = 4 * rng.randint(0, 4) + (rng.random() < 0.2) * rng.randint(1, 3)
        cases.append(bytes(rng.choice(ALPHA.encode() + b"====*-\x00\xff") for _ in range(n)))
    # lengths that are no multiple of 4
    cases += [forms[0][:n] for n in (1, 2, 3, 5, 1023, 1025, 3199)]
    # two events: a stray before a '=' (an error), a stray after a '=' (ignored)
    spots = [0, 1, 5, 15, 16, 17, 1022, 1023, 1024, 1025, 2047, 2048, 3000, EVENT_SPAN - 2, EVENT_SPAN - 1]
    two = []
    for f in forms:
        for a in spots:
            for b in spots:
                if a < b:
                    for first, second in ((b"*", b"="), (b"=", b"*"), (b"\xff", b"="), (b"=", b"\x00")):
                        two.append(f[:a] + first + f[a + 1:b] + second + f[b + 1:])
    cases += two
    # mixed with valid messages
    valid = [base64.b64encode(rng.randbytes(rng.choice((0, 1, 2, 3, 100, 767, 768, 769, 2400, 5000))))
             for _ in range(len(cases) // 40)]
    for i, v in enumerate(valid):
        cases.insert(40 * i + rng.randint(0, 39), v)
    return cases, forms, two, valid


def test_first_event_at_every_position(gpu, vds_lib):
    import torch
    rng = random.Random(2)
    cases, forms, two, valid = _event_cases(rng)
    st, outs = _run_decode(torch, vds_lib, cases)
    by_text = {c: int(s) for c, s in zip(cases, st)}
    # the launch saw each kind of outcome (the comparison itself is _run_decode's)
    assert set(st.tolist()) == {0, EB64_LENGTH, EB64_PADDING, EB64_CHAR}
    f0, f1 = forms[0], forms[1]
    assert by_text[f0[:7] + b"=" + f0[8:]] == EB64_PADDING
    assert by_text[f0[:7] + b"*" + f0[8:]] == EB64_CHAR
    assert by_text[f1[:1024] + b"=" + f1[1025:]] == 0  # an early '=' with padding 1: two bytes, then zeros
    assert by_text[f1[:16] + b"*" + f1[17:1024] + b"=" + f1[1025:]] == EB64_CHAR
    assert by_text[f1[:16] + b"=" + f1[17:1024] + b"*" + f1[1025:]] == 0
    vs = set(valid)
    for c, o in zip(cases, outs):
        if c in vs:
            assert by_text[c] == 0 and o.tobytes() == base64.b64decode(c)


def test_declared_size_mismatch(gpu, vds_lib):
    import torch
    rng = random.Random(3)
    forms = [base64.b64encode(rng.randbytes(EVENT_SPAN // 4 * 3 - p)) for p in (0, 1, 2)]
    texts, declared = [], {}
    for t in [b"QUJD", b"QUE=", b"QQ=="] + forms:
        true = vds_lib.vds_ec_base64_decoded_size(t, len(t))
        for s in (len(t) // 4 * 3 - p for p in (0, 1, 2)):
            texts.append(base64.b64encode(rng.randbytes(rng.choice((1, 50, 800, 2400)))))  # a valid neighbour
            if s != true:
                declared[len(texts)] = s
            texts.append(t)
    assert len(declared) == 12
    st, outs = _run_decode(torch, vds_lib, texts, declared=declared)
    for i, t in enumerate(texts):
        if i in declared:
            assert st[i] == EINVAL and (outs[i] == FILL).all()
        else:
            assert st[i] == 0 and outs[i].tobytes() == base64.b64decode(t)


def test_encode_every_length_and_alignment_and_back(gpu, vds_lib):
    import torch
    from vds_amd import chunk
    bodies = _bodies(random.Random(4))
    count = len(bodies)
    i_offs, i_total = _place([len(b) for b in bodies], [TEXT_MOD16[i % 7] for i in range(count)], 16, 16)
    d_in = torch.from_numpy(_gather(bodies, i_offs, i_total, False)).cuda()
    tlens = [(len(b) + 2) // 3 * 4 for b in bodies]
    o_offs, o_total = _place(tlens, [OUT_MOD4[(i // 7) % 4] for i in range(count)], 4, GUARD)
    want = np.full(o_total, FILL, dtype=np.uint8)
    for b, off in zip(bodies, o_offs):
        t = base64.b64encode(b)
        want[off:off + len(t)] = np.frombuffer(t, dtype=np.uint8)
    d_out = torch.full((o_total,), FILL, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 4 == 0
    chunk.base64_encode_batch_device([d_in.data_ptr() + o for o in i_offs], [len(b) for b in bodies],
                                     [d_out.data_ptr() + o for o in o_offs])
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    wrong = np.flatnonzero(got != want)
    if wrong.size:
        at = int(wrong[0])
        i = int(np.searchsorted(np.asarray(o_offs), at, side="right")) - 1
        raise AssertionError(("characters", at, "message", i, "offset in it", at - o_offs[max(i, 0)], len(bodies[i]),
                              int(got[at]), int(want[at])))
    # and the decode launch over the encode's output, where it lies, gives the inputs back
    texts = [want[o:o + n].tobytes() for o, n in zip(o_offs, tlens)]
    st, outs = _run_decode(torch, vds_lib, texts, d_text=d_out, text_ptrs=[d_out.data_ptr() + o for o in o_offs])
    assert not st.any()
    for b, o in zip(bodies, outs):
        assert o.tobytes() == b, len(b)
