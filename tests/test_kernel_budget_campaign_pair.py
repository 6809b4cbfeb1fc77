"""CPU test: the register budget of the paired campaign kernels (K31: csrc/kernels_rollout_campaign_pair.h,
csrc/kernels_rollout_lookahead_campaign_pair.h), read from the code objects hipcc produces here for gfx950 (no GPU), in the manner
of test_kernel_budget_lookahead_campaign.py.  A pair kernel is its plain campaign's flight with the pair tail behind the step loop,
and the bound on its speed is stated against the plain kernels' in the same run (tools/time_rollout.py campaign_pair), so what is
pinned is relative to the plain kernel of the same form, whose unit is compiled in the same test: the 72 + 24 instantiations exist;
none has a vector spill or a private segment; none runs at fewer waves per SIMD than k_rollout_campaign /
k_rollout_lookahead_campaign at the same form; the lookahead forms keep K27's limits, 128 vector registers, or 168 at D = 6, and
have no scalar spill, as K29's have none.  The label forms' scalar spills are printed beside the plain kernel's: K28 itself spills
23 - 97 scalar registers to vector lanes from D = 4 on, the pair kernel as many or fewer at 69 of the 72 forms and two more (36
against 34) at D = 4, 'linear', global tables, for each label type - the lane of the launch, held across the flight.  Only register
counts are read from the notes.  Waves per SIMD from the VGPR count: one 512-entry file per lane,
allocated in granules of 8, at most 8 waves."""
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = ROOT / "optimal-control-dynamic-programming_amd" / "csrc"
FIELDS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
LABEL, VALUE = r"ILi(\d)E(\w)Li([01])ELb([01])EEE", r"ILi(\d)E([fd])Lb([01])EEE"
UNITS = {"rollout_campaign_pair.hip": r"_ZN3hjb23k_rollout_campaign_pair" + LABEL,
         "rollout_campaign.hip": r"_ZN3hjb18k_rollout_campaign" + LABEL,
         "rollout_lookahead_campaign_pair.hip": r"_ZN3hjb33k_rollout_lookahead_campaign_pair" + VALUE,
         "rollout_lookahead_campaign.hip": r"_ZN3hjb28k_rollout_lookahead_campaign" + VALUE}
LABEL_FORMS = {(str(d), t, m, l) for d in range(1, 7) for t in "hti" for m in "01" for l in "01"}
VALUE_FORMS = {(str(d), t, l) for d in range(1, 7) for t in "fd" for l in "01"}
PAIRS = (("rollout_campaign_pair.hip", "rollout_campaign.hip", LABEL_FORMS), ("rollout_lookahead_campaign_pair.hip", "rollout_lookahead_campaign.hip", VALUE_FORMS))


def waves_per_simd(vgprs, agprs=0):
    alloc = -(-(vgprs + agprs) // 8) * 8
    return min(8, 512 // max(alloc, 8))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{unit: {form: {field: int}}} from the metadata notes (.amdhsa.kernels) of the two pair units and the two plain units"""
    tmp = tmp_path_factory.mktemp("campaign_pair_budget")

    def one(unit):
        asm = tmp / (unit + ".s")
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                            "-o", str(asm), str(CSRC / unit)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        text = asm.read_text()
        meta = text[text.index("amdhsa.kernels"):]
        found = {}
        for blk in re.split(r"\n\s+- (?=\.agpr_count:)", meta)[1:]:
            m = re.search(r"\.name:\s+" + UNITS[unit], blk)
            if m:
                found[m.groups()] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1)) for f in FIELDS}
        return unit, found

    with ThreadPoolExecutor(max_workers=4) as ex:
        return dict(ex.map(one, UNITS))


def test_every_instantiation_exists_without_scratch(kernels):
    for mine, plain, forms in PAIRS:
        assert set(kernels[mine]) == forms, (mine, len(kernels[mine]))
        assert set(kernels[plain]) == forms, (plain, len(kernels[plain]))
        for form, k in sorted(kernels[mine].items()):
            assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (mine, form, k)
    for form, k in sorted(kernels["rollout_lookahead_campaign_pair.hip"].items()):
        assert k["vgpr_count"] <= (168 if form[0] == "6" else 128) and k["sgpr_spill_count"] == 0, (form, k)


@pytest.mark.parametrize("mine, plain, forms", PAIRS, ids=["labels", "lookahead"])
def test_no_instantiation_runs_at_fewer_waves_than_its_plain_counterpart(kernels, mine, plain, forms):
    rows = []
    for form in sorted(forms):
        k, p = kernels[mine][form], kernels[plain][form]
        rows.append((form, k["vgpr_count"], waves_per_simd(k["vgpr_count"], k["agpr_count"]), k["sgpr_spill_count"], p["vgpr_count"],
                     waves_per_simd(p["vgpr_count"], p["agpr_count"]), p["sgpr_spill_count"]))
    assert len(rows) == len(forms) and len(rows) in (72, 24)
    for form, vk, wk, sk, vp, wp, sp in rows:
        print("%s %s: pair %3d VGPRs, %d waves, %3d scalar spills; plain %3d VGPRs, %d waves, %3d scalar spills"
              % (mine, "/".join(form), vk, wk, sk, vp, wp, sp))
    bad = [r for r in rows if r[2] < r[5]]
    assert not bad, bad
