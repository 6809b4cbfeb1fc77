"""CPU test: the register budget of the actuator-noise kernels (csrc/kernels_rollout_actuator.h: K33;
csrc/kernels_rollout_actuator_campaign.h: K34), read from the code objects inside the built library (llvm-objdump --offloading,
llvm-readelf --notes; no GPU), as tests/test_kernel_budget_campaign.py reads K28's.  K33 is K25's step with a few more products
and K34 is K28's frame around it, and the bounds on their speed are stated against K25's and K28's in the same run
(tools/time_rollout.py kirk_actuator, actuator_campaign), so what is pinned is relative to those in the same build: the 72 + 72
instantiations exist, none has a vector spill or a private segment, and none runs at fewer waves per SIMD than its
k_rollout_noisy / k_rollout_campaign counterpart.  The VGPR and scalar-spill table is printed.  Metadata only.

K33 rereads its launch record as K28 does and runs at K25's waves or more at every form.  K34 meets the condition at the
'nearest' forms of D = 5 and D = 6 and at the D = 5 'linear' LDS form through a stated occupancy target
(kernels_rollout_actuator_campaign.h); the last of these also forms its lane's block, slot and start again behind the flight
instead of holding them across it (96 VGPRs, 5 waves, as K28)."""
import re
import shutil
import subprocess

import pytest

from test_kernel_budget_campaign import FORM, TOOLS, waves_per_simd

PAIRS = (("k_rollout_actuator", "k_rollout_noisy"), ("k_rollout_actuator_campaign", "k_rollout_campaign"))
FAMILIES = tuple(f for pair in PAIRS for f in pair)


@pytest.fixture(scope="module")
def kernels(built, tmp_path_factory):
    """{kernel family: {(D, label type, method, lds): (vgprs, agprs, vgpr spills, sgpr spills, private segment)}}"""
    objdump = shutil.which("llvm-objdump", path=TOOLS) or shutil.which("llvm-objdump")
    readelf = shutil.which("llvm-readelf", path=TOOLS) or shutil.which("llvm-readelf")
    assert objdump and readelf, "llvm-objdump / llvm-readelf of the ROCm toolchain not found"
    d = tmp_path_factory.mktemp("actuator_budget")
    shutil.copy(built.LIB, d / "libhjbdp.so")
    r = subprocess.run([objdump, "--offloading", "libhjbdp.so"], cwd=d, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {f: {} for f in FAMILIES}
    for co in sorted(d.glob("libhjbdp.so.*gfx950*")):
        notes = subprocess.run([readelf, "--notes", co.name], cwd=d, capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:                           # one block per kernel of the code object
            m = re.search(r"\.name:\s+_ZN3hjb\d+(%s)%s" % ("|".join(sorted(FAMILIES, key=len, reverse=True)), FORM), blk)
            if m:
                num = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
                found[m.group(1)][m.groups()[1:]] = (num("vgpr_count"), int(blk.split()[0]), num("vgpr_spill_count"), num("sgpr_spill_count"),
                                                     num("private_segment_fixed_size"))
    return found


def test_every_instantiation_exists_without_scratch(kernels):
    forms = {(str(d), t, m, l) for d in range(1, 7) for t in "hti" for m in "01" for l in "01"}
    for family in FAMILIES:
        assert set(kernels[family]) == forms, (family, len(kernels[family]))
    for family, _ in PAIRS:
        for form, (vgprs, agprs, spills, sgpr_spills, scratch) in kernels[family].items():
            assert spills == 0 and scratch == 0, (family, form, vgprs, spills, scratch)


@pytest.mark.parametrize("mine,base", PAIRS)
def test_no_instantiation_runs_at_fewer_waves_than_its_counterpart(kernels, mine, base):
    rows = []
    for form in sorted(kernels[mine]):
        a, b = kernels[mine][form], kernels[base][form]
        rows.append((form, a[0], waves_per_simd(a[0], a[1]), a[3], b[0], waves_per_simd(b[0], b[1]), b[3]))
    assert len(rows) == 72, len(rows)
    for form, va, wa, sa, vb, wb, sb in rows:
        print("D=%s labels=%s method=%s lds=%s: %s %3d VGPRs, %d waves, %3d scalar spills; %s %3d VGPRs, %d waves, %3d scalar spills"
              % (*form, mine, va, wa, sa, base, vb, wb, sb))
    bad = [r for r in rows if r[2] < r[5]]
    assert not bad, bad
