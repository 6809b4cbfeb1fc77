"""CPU test: the greedy rollout kernel's register budget (K26, csrc/kernels_rollout_greedy.h), read from the code object hipcc
produces here for gfx950 (no GPU).  The kernel reads its model through the argument segment, per step and from D = 3 on per loop body, so that no
scalar is spilled (csrc/hjbdp_greedy.h, greedy_reread_in_loop); the corners of a candidate are read in groups, so that no instantiation
holds 2^D values.  Both come down to: every one of the 24 instantiations (D x value type x LDS) has no vector spill, no scalar
spill and no private segment."""
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
UNIT = ROOT / "optimal-control-dynamic-programming_amd" / "csrc" / "rollout_greedy.hip"


@pytest.fixture(scope="module")
def greedy_asm(tmp_path_factory):
    asm = tmp_path_factory.mktemp("greedy_budget") / "rollout_greedy.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", str(asm), str(UNIT)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return asm.read_text()


def _kernels(text):
    """{(D, value type letter, LDS): {field: int}} from the metadata note (.amdhsa.kernels)"""
    meta = text[text.index("amdhsa.kernels"):]
    out = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", meta)[1:]:
        m = re.search(r"\.name:\s+_ZN3hjb16k_rollout_greedyILi(\d)E([fd])Lb([01])EEE", blk)
        if m:
            out[(int(m.group(1)), m.group(2), int(m.group(3)))] = {
                f: int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1))
                for f in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    return out


def test_every_instantiation_is_built(greedy_asm):
    got = _kernels(greedy_asm)
    assert set(got) == {(D, t, l) for D in range(1, 7) for t in "fd" for l in (0, 1)}, sorted(got)


def test_no_instantiation_spills_or_has_a_private_segment(greedy_asm):
    for key, k in sorted(_kernels(greedy_asm).items()):
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (key, k)
        assert k["vgpr_count"] <= 128, (key, k)        # four waves per SIMD at 256 threads a block: the gathers' latency needs them
    assert "scratch_" not in greedy_asm
