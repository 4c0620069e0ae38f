"""The inbox fill form of the run-time compiled k = 16 restore kernels
(xorprog.hpp emit_fill_inbox, restore_syn.hpp kInbox): which survivor sets
take it, and what its kernel costs in registers.  No GPU: the kernels are
compiled through the helper and dumped (chunk.jit_dump)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER = os.path.join(ROOT, "vds_amd", "vds_ec_jitc")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
HEADLINE = (0, 5, 10, 15)
MARK = "kInbox = true"

pytestmark = pytest.mark.skipif(not os.access(HELPER, os.X_OK),
                                reason="vds_ec_jitc not built (run __graft_entry__.build())")


def _dump(tmp_path, erased_sets, inbox=None):
    """Dump the kernels of `erased_sets` in a process of its own (the form
    switch is read once per process); {erased: (source, code object path)}."""
    code = ("import sys\nfrom vds_amd import chunk\n"
            "for e in eval(sys.argv[2]):\n"
            "    chunk.jit_dump(16, [r for r in range(20) if r not in e], sys.argv[1])\n")
    env = dict(os.environ, VDS_EC_JIT_CACHE="0")
    env.pop("VDS_EC_JIT_INBOX", None)
    if inbox is not None:
        env["VDS_EC_JIT_INBOX"] = str(inbox)
    tmp_path.mkdir(exist_ok=True)
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path), repr(list(erased_sets))], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    for e in erased_sets:
        mask = sum(1 << r for r in range(20) if r not in e)
        base = tmp_path / f"jit_16_20_{mask:x}"
        out[e] = (base.with_suffix(".hip").read_text(), base.with_suffix(".co"))
    return out


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    return _dump(tmp_path_factory.mktemp("inbox"), [HEADLINE, (1, 6, 16, 19), (0, 1, 5, 10)])


def test_eligible_sets_compile_to_the_inbox_form(dumps):
    for e in (HEADLINE, (1, 6, 16, 19)):
        assert MARK in dumps[e][0], e


def test_two_erased_points_in_one_group_keep_the_scatter_form(dumps):
    src = dumps[(0, 1, 5, 10)][0]
    assert MARK not in src and "kScatter = true" in src


def test_ownership_table_of_the_headline_set(dumps):
    """Wave g owns its group's three survivors and one survivor >= k."""
    src = dumps[HEADLINE][0]
    surv = [int(x) for x in re.search(r"kSurv\[16\] = \{([^}]*)\}", src).group(1).replace(" ", "").split(",") if x]
    assert surv == [1, 2, 3, 16, 4, 6, 7, 17, 8, 9, 11, 18, 12, 13, 14, 19]
    pack = int(re.search(r"kOrderPack = 0x([0-9a-f]+)ull", src).group(1), 16)
    ranked = sorted(surv)
    assert [(pack >> (4 * j)) & 15 for j in range(16)] == [ranked.index(p) for p in surv]
    own = [int(x) for x in re.search(r"kOwnM\[4\] = \{([^}]*)\}", src).group(1).replace(" ", "").split(",") if x]
    assert own == [0, 1, 2, 3]


def test_headline_kernel_has_no_scratch_and_fits_two_waves_per_simd(dumps):
    notes = subprocess.run([READELF, "--notes", str(dumps[HEADLINE][1])], capture_output=True, text=True,
                           check=True).stdout

    def field(name):
        return int(re.search(rf"\.{name}:\s+(\d+)", notes).group(1))
    assert field("private_segment_fixed_size") == 0
    assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    # 512 VGPRs per SIMD lane (arch + acc): two waves need <= 256 each
    assert field("vgpr_count") + field("agpr_count") <= 256


def test_switch_off_gives_the_scatter_form(tmp_path, dumps):
    """VDS_EC_JIT_INBOX=0 (or a -DVDS_JIT_INBOX=0 build): the headline set's
    source is the scatter form's -- survivors by rank, no inbox members --
    and the non-eligible set's source does not depend on the switch."""
    off = _dump(tmp_path / "off", [HEADLINE, (0, 1, 5, 10)], inbox=0)
    src = off[HEADLINE][0]
    assert MARK not in src and "kOrderPack" not in src and "kOwnM" not in src and "kScatter = true" in src
    assert "kSurv[16] = {1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14, 16, 17, 18, 19, }" in src
    assert off[(0, 1, 5, 10)][0] == dumps[(0, 1, 5, 10)][0]
    # the inbox source is the scatter source of the permuted survivors plus
    # its three members: with them removed, only kSurv and the programs differ
    on = _dump(tmp_path / "on", [HEADLINE], inbox=1)[HEADLINE][0]
    assert on == dumps[HEADLINE][0]
    head_on, head_off = on.split("kSurv")[0], src.split("kSurv")[0]
    assert head_on == head_off
