"""CPU test: the register budget of the campaign histogram kernels (K30: csrc/kernels_rollout_campaign_hist.h,
csrc/kernels_rollout_lookahead_campaign_hist.h), read from the code objects inside the built library (llvm-objdump --offloading,
llvm-readelf --notes; no GPU) in the manner of test_kernel_budget_campaign.py.  A histogram kernel is its plain campaign's flight
with the count behind the step loop, and the bound on its speed is stated against the plain kernel's in the same run
(tools/time_rollout.py campaign_hist), so what is pinned is relative to the plain kernel of the same form in the same build: the
72 + 24 instantiations exist, none has a vector spill or a private segment, and none runs at fewer waves per SIMD than
k_rollout_campaign / k_rollout_lookahead_campaign at the same form.  Only register counts are read from the notes.  Waves per SIMD
from the VGPR count: one 512-entry file per lane, allocated in granules of 8, at most 8 waves."""
import re
import shutil
import subprocess

import pytest

TOOLS = "/opt/rocm/lib/llvm/bin"
FAMILIES = {"k_rollout_campaign": r"ILi(\d)E(\w)Li([01])ELb([01])E", "k_rollout_campaign_hist": r"ILi(\d)E(\w)Li([01])ELb([01])E",
            "k_rollout_lookahead_campaign": r"ILi(\d)E([fd])Lb([01])E", "k_rollout_lookahead_campaign_hist": r"ILi(\d)E([fd])Lb([01])E"}
LABEL_FORMS = {(str(d), t, m, l) for d in range(1, 7) for t in "hti" for m in "01" for l in "01"}
VALUE_FORMS = {(str(d), t, l) for d in range(1, 7) for t in "fd" for l in "01"}


def waves_per_simd(vgprs, agprs=0):
    alloc = -(-(vgprs + agprs) // 8) * 8
    return min(8, 512 // max(alloc, 8))


@pytest.fixture(scope="module")
def kernels(built, tmp_path_factory):
    """{kernel family: {form: (vgprs, agprs, vgpr spills, sgpr spills, private segment)}}"""
    objdump = shutil.which("llvm-objdump", path=TOOLS) or shutil.which("llvm-objdump")
    readelf = shutil.which("llvm-readelf", path=TOOLS) or shutil.which("llvm-readelf")
    assert objdump and readelf, "llvm-objdump / llvm-readelf of the ROCm toolchain not found"
    d = tmp_path_factory.mktemp("campaign_hist_budget")
    shutil.copy(built.LIB, d / "libhjbdp.so")
    r = subprocess.run([objdump, "--offloading", "libhjbdp.so"], cwd=d, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {family: {} for family in FAMILIES}
    for co in sorted(d.glob("libhjbdp.so.*gfx950*")):
        notes = subprocess.run([readelf, "--notes", co.name], cwd=d, capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:                           # one block per kernel of the code object
            for family, form in FAMILIES.items():
                m = re.search(r"\.name:\s+_ZN3hjb%d%s%sEEv" % (len(family), family, form), blk)
                if m:
                    num = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
                    found[family][m.groups()] = (num("vgpr_count"), int(blk.split()[0]), num("vgpr_spill_count"), num("sgpr_spill_count"),
                                                 num("private_segment_fixed_size"))
    return found


def test_every_instantiation_exists_without_scratch(kernels):
    assert set(kernels["k_rollout_campaign_hist"]) == LABEL_FORMS, len(kernels["k_rollout_campaign_hist"])
    assert set(kernels["k_rollout_lookahead_campaign_hist"]) == VALUE_FORMS, len(kernels["k_rollout_lookahead_campaign_hist"])
    assert set(kernels["k_rollout_campaign"]) == LABEL_FORMS and set(kernels["k_rollout_lookahead_campaign"]) == VALUE_FORMS
    for family in ("k_rollout_campaign_hist", "k_rollout_lookahead_campaign_hist"):
        for form, (vgprs, agprs, spills, sgpr_spills, scratch) in kernels[family].items():
            assert spills == 0 and scratch == 0, (family, form, vgprs, spills, scratch)


@pytest.mark.parametrize("family", ["k_rollout_campaign", "k_rollout_lookahead_campaign"])
def test_no_instantiation_runs_at_fewer_waves_than_its_plain_counterpart(kernels, family):
    rows = []
    for form in sorted(kernels[family + "_hist"]):
        mine, plain = kernels[family + "_hist"][form], kernels[family][form]
        rows.append((form, mine[0], waves_per_simd(mine[0], mine[1]), mine[3], plain[0], waves_per_simd(plain[0], plain[1]), plain[3]))
    assert len(rows) == (72 if family == "k_rollout_campaign" else 24), len(rows)
    for form, vh, wh, sh, vp, wp, sp in rows:
        print("%s %s: hist %3d VGPRs, %d waves, %3d scalar spills; plain %3d VGPRs, %d waves, %3d scalar spills"
              % (family, "/".join(form), vh, wh, sh, vp, wp, sp))
    bad = [r for r in rows if r[2] < r[5]]
    assert not bad, bad
