"""CPU test: the register budget of the control-lookahead kernels (K35, csrc/kernels_rollout_ctrl_lookahead.h; K36,
csrc/kernels_rollout_ctrl_lookahead_campaign.h), after tests/test_kernel_budget_lookahead_campaign.py, read from the code objects
inside the built library (llvm-objdump --offloading, llvm-readelf --notes; no GPU) as tests/test_kernel_budget_campaign_hist.py
reads its own: the library is what runs, and nothing is compiled a second time.  K35 is K27's loop with one more scalar per
candidate and (FLY) K33's actuator step in the place of K25's offset add, K36 is K29's frame around it, and the bounds on their
speed are stated against K27 in the same run (tools/time_rollout.py kirk_control_lookahead, control_lookahead_campaign), so the
budget is K27's: the 48 + 24 instantiations exist; none has a vector spill, a scalar spill or a private segment; each has at most
128 vector registers - 168 at D = 6, as K27 - and none runs at fewer waves per SIMD than its K27 counterpart: for K35
k_rollout_lookahead with the same FLY, for K36 the FLY = true form.  Waves per SIMD from the VGPR count: one 512-entry file per
lane, allocated in granules of 8, at most 8 waves.  Metadata only."""
import re
import shutil
import subprocess

import pytest

from test_kernel_budget_campaign import TOOLS, waves_per_simd
from test_kernel_budget_lookahead_campaign import vgpr_limit

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
# family -> the pattern behind "_ZN3hjb<len>"; the groups: D, value type letter, LDS (, FLY)
FAMILIES = {"k_rollout_ctrl_lookahead": r"ILi(\d)E([fd])Lb([01])ELb([01])EEE", "k_rollout_lookahead": r"ILi(\d)E([fd])Lb([01])ELb([01])EEE",
            "k_rollout_ctrl_lookahead_campaign": r"ILi(\d)E([fd])Lb([01])EEE"}
FORMS = {(D, t, l) for D in range(1, 7) for t in "fd" for l in (0, 1)}


@pytest.fixture(scope="module")
def kernels(built, tmp_path_factory):
    """{family: {(D, value type letter, LDS[, FLY]): {field: int}}} from the metadata notes of the library's gfx950 code objects"""
    objdump = shutil.which("llvm-objdump", path=TOOLS) or shutil.which("llvm-objdump")
    readelf = shutil.which("llvm-readelf", path=TOOLS) or shutil.which("llvm-readelf")
    assert objdump and readelf, "llvm-objdump / llvm-readelf of the ROCm toolchain not found"
    d = tmp_path_factory.mktemp("ctrl_lookahead_budget")
    shutil.copy(built.LIB, d / "libhjbdp.so")
    r = subprocess.run([objdump, "--offloading", "libhjbdp.so"], cwd=d, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {f: {} for f in FAMILIES}
    for co in sorted(d.glob("libhjbdp.so.*gfx950*")):
        notes = subprocess.run([readelf, "--notes", co.name], cwd=d, capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s+- (?=\.agpr_count:)", notes)[1:]:           # one block per kernel of the code object
            for family, pattern in FAMILIES.items():
                m = re.search(r"\.name:\s+_ZN3hjb%d%s%sv" % (len(family), family, pattern), blk)
                if m:
                    key = tuple(g if g in "fd" else int(g) for g in m.groups())
                    found[family][key] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1)) for f in FIELDS}
    return found


def test_every_instantiation_is_built(kernels):
    with_fly = {form + (fly,) for form in FORMS for fly in (0, 1)}
    assert set(kernels["k_rollout_ctrl_lookahead"]) == with_fly, sorted(kernels["k_rollout_ctrl_lookahead"])            # 48
    assert set(kernels["k_rollout_ctrl_lookahead_campaign"]) == FORMS, sorted(kernels["k_rollout_ctrl_lookahead_campaign"])   # 24
    assert set(kernels["k_rollout_lookahead"]) == with_fly


@pytest.mark.parametrize("family", ["k_rollout_ctrl_lookahead", "k_rollout_ctrl_lookahead_campaign"])
def test_no_instantiation_spills_or_has_a_private_segment(kernels, family):
    for key, k in sorted(kernels[family].items()):
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (key, k)
        assert k["vgpr_count"] <= vgpr_limit(key[0]), (key, k)


def test_no_instantiation_runs_at_fewer_waves_than_its_k27_counterpart(kernels):
    rows = []
    for form in sorted(FORMS):
        for fly in (0, 1):
            rows.append(("K35 fly=%d" % fly, form, kernels["k_rollout_ctrl_lookahead"][form + (fly,)], kernels["k_rollout_lookahead"][form + (fly,)]))
        rows.append(("K36", form, kernels["k_rollout_ctrl_lookahead_campaign"][form], kernels["k_rollout_lookahead"][form + (1,)]))
    assert len(rows) == 72
    bad = []
    for who, form, mine, k27 in rows:
        wm, wb = waves_per_simd(mine["vgpr_count"], mine["agpr_count"]), waves_per_simd(k27["vgpr_count"], k27["agpr_count"])
        print("%s D=%d values=%s lds=%d: %3d VGPRs, %d waves; K27 %3d VGPRs, %d waves" % (who, *form, mine["vgpr_count"], wm, k27["vgpr_count"], wb))
        if wm < wb:
            bad.append((who, form, mine["vgpr_count"], wm, k27["vgpr_count"], wb))
    assert not bad, bad
