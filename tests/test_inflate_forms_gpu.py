"""k_inflate_batch (vds_ec_inflate_batch_device, inflate.hip) over the deflate
forms zlib's own compressor never emits: the corpus of tests/inflate_forms.py,
which tests/test_inflate_forms_cpu.py runs through the host code and whose
coverage conditions that file holds.  Status, length and bytes against
Python's zlib, bit for bit.

One launch a family, hundreds to a few thousand streams each, in the layout of
tests/test_inflate_batch_gpu.py (whose _run this uses): one input buffer with
0xA5 between the streams, one output buffer with 0x5A guards, sentinel
statuses; input and output offsets cycle through 0..3.  A wrong kernel shows as
a failed comparison or a touched guard byte."""
import pytest

import inflate_cases as K
import inflate_forms as F
from test_inflate_batch_gpu import _run

pytestmark = pytest.mark.gpu


def _launch(cases, in_mod=lambda i: i % 4, out_mod=lambda i: (i // 4) % 4):
    import torch
    _run(torch, [c[1:] for c in cases], in_mod=in_mod, out_mod=out_mod)


def test_match_grid(gpu):
    """every (D, L) around the 64-lane steps of the copy with 0, 1, 63 and 64 - k literals pending, a
    match reading the match before it, and the twins reaching one byte too far back"""
    valid, invalid = F.match_grid()
    _launch(valid + invalid)


def test_match_grid_one_byte_short(gpu):
    """the valid streams of the grid with room for all but the last byte: SPACE, nothing past the capacity"""
    valid, _ = F.match_grid()
    _launch([(n, s, cap - 1, K.EINFLATE_SPACE, b"") for n, s, cap, st, out in valid], out_mod=lambda i: (i // 3) % 4)


def test_symbol_extremes(gpu):
    """every length and distance symbol at both ends of its extra bits behind 32 KiB of history"""
    _launch(F.symbol_extremes())


def test_table_shapes(gpu):
    """second-level tables of every width, sets of up to 286 codes up to 15 bits, over 300 random sets"""
    _launch(F.table_shapes())


def test_degenerate_sets_and_code_length_coding(gpu):
    _launch(F.degenerate() + F.code_length_coding())


def test_blocks_and_reader(gpu):
    """the whole family at each input misalignment 0..3"""
    cases = F.blocks_and_reader()
    _launch([c for shift in range(4) for c in cases], in_mod=lambda i: i // len(cases), out_mod=lambda i: i % 4)


def test_prefixes(gpu):
    _launch(F.prefixes())


def test_flips(gpu):
    _launch(F.flips())


def test_capacity(gpu):
    """every capacity from 0 to past the end (or the error) of thirteen streams, and around what five
    prefixes deliver: SPACE, DATA and SHORT in zlib's order"""
    cases, _ = F.capacity()
    _launch(cases)
