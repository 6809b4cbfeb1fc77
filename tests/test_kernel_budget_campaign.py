"""CPU test: the campaign kernel's register budget (csrc/kernels_rollout_campaign.h: K28), read from the code objects inside the
built library (llvm-objdump --offloading, llvm-readelf --notes; no GPU).  K28 is K25's step plus a reduction, and the bound on
its speed is stated against K25's in the same run (tools/time_rollout.py campaign), so what is pinned is relative to K25 in the
same build: the 72 instantiations exist, none has a vector spill or a private segment, none runs at fewer waves per SIMD than
its K25 counterpart, and none spills more scalars (to lanes of a vector register: no memory) than its K25 counterpart - K28 reads
its launch record where it lies instead of holding it across the step loop, so it spills far fewer, and none at D <= 2; the counts
are DESIGN.md 4b's.  Waves per SIMD from the VGPR count: one 512-entry file per lane, allocated in granules of 8, at most 8
waves."""
import re
import shutil
import subprocess

import pytest

TOOLS = "/opt/rocm/lib/llvm/bin"
FORM = r"ILi(\d)E(\w)Li([01])ELb([01])E"


def waves_per_simd(vgprs, agprs=0):
    alloc = -(-(vgprs + agprs) // 8) * 8
    return min(8, 512 // max(alloc, 8))


@pytest.fixture(scope="module")
def kernels(built, tmp_path_factory):
    """{kernel family: {(D, label type, method, lds): (vgprs, agprs, vgpr spills, sgpr spills, private segment)}}"""
    objdump = shutil.which("llvm-objdump", path=TOOLS) or shutil.which("llvm-objdump")
    readelf = shutil.which("llvm-readelf", path=TOOLS) or shutil.which("llvm-readelf")
    assert objdump and readelf, "llvm-objdump / llvm-readelf of the ROCm toolchain not found"
    d = tmp_path_factory.mktemp("campaign_budget")
    shutil.copy(built.LIB, d / "libhjbdp.so")
    r = subprocess.run([objdump, "--offloading", "libhjbdp.so"], cwd=d, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {"k_rollout_noisy": {}, "k_rollout_campaign": {}}
    for co in sorted(d.glob("libhjbdp.so.*gfx950*")):
        notes = subprocess.run([readelf, "--notes", co.name], cwd=d, capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:                           # one block per kernel of the code object
            m = re.search(r"\.name:\s+_ZN3hjb\d+(k_rollout_noisy|k_rollout_campaign)" + FORM, blk)
            if m:
                num = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
                found[m.group(1)][m.groups()[1:]] = (num("vgpr_count"), int(blk.split()[0]), num("vgpr_spill_count"), num("sgpr_spill_count"),
                                                     num("private_segment_fixed_size"))
    return found


def test_waves_per_simd_table():
    assert [waves_per_simd(v) for v in (1, 64, 65, 72, 73, 80, 96, 97, 128, 129, 168, 169, 256, 257, 512)] == \
        [8, 8, 7, 7, 6, 6, 5, 4, 4, 3, 3, 2, 2, 1, 1]


def test_every_instantiation_exists_without_scratch(kernels):
    forms = {(str(d), t, m, l) for d in range(1, 7) for t in "hti" for m in "01" for l in "01"}
    for family in ("k_rollout_noisy", "k_rollout_campaign"):
        assert set(kernels[family]) == forms, (family, len(kernels[family]))
    for form, (vgprs, agprs, spills, sgpr_spills, scratch) in kernels["k_rollout_campaign"].items():
        assert spills == 0 and scratch == 0, (form, vgprs, spills, scratch)
        if int(form[0]) <= 2:                       # a loop body's part of the record and the loop's own scalars fit the file
            assert sgpr_spills == 0, (form, sgpr_spills)


def test_no_instantiation_runs_at_fewer_waves_than_its_k25_counterpart(kernels):
    rows = []
    for form in sorted(kernels["k_rollout_campaign"]):
        mine, k25 = kernels["k_rollout_campaign"][form], kernels["k_rollout_noisy"][form]
        rows.append((form, mine[0], waves_per_simd(mine[0], mine[1]), k25[0], waves_per_simd(k25[0], k25[1]), mine[3], k25[3]))
    assert len(rows) == 72, len(rows)
    for form, v28, w28, v25, w25, s28, s25 in rows:
        print("D=%s labels=%s method=%s lds=%s: K28 %3d VGPRs, %d waves, %3d scalar spills; K25 %3d VGPRs, %d waves, %3d scalar spills"
              % (*form, v28, w28, s28, v25, w25, s25))
    bad = [r for r in rows if r[2] < r[4]]
    assert not bad, bad
    more = [r for r in rows if r[5] > r[6]]
    assert not more, more
