"""CPU test: the integer arithmetic of the stage kernels' grid-stride walk (csrc/hjbdp_walk.h), checked exhaustively on the
host - no GPU.  tests/walk_harness.cpp includes the header the kernels and choose_launch include, is compiled as plain C++
and checks

  xcd_share(b, G), for every G in 1 .. 8200: a permutation of [0, G), and every XCD's workgroups (b % 8 == x) take one
  contiguous range of it;
  launch_spans(work, cap), caps 4096 / 2^18 / 2^20, every work up to 3 * 4096, the neighbourhood of every multiple of the cap
  up to 40 caps and a seeded sample up to 2^36: `work` itself where it fits the cap, otherwise a multiple of 8 within the cap
  that needs no more spans than the cap forces (g * spans >= work) and makes them equally long to within the rounding
  (g * spans - work < 8 * spans).

The harness's second mode runs the same checks on wrong copies (the `x < r` term of xcd_share dropped, the remainder handed
to the wrong XCDs, no remap at all; spans not rounded to 8, cut at the cap, rounded down): each must be rejected."""
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("walk") / "walk_harness"
    r = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror",
                        "-I%s/optimal-control-dynamic-programming_amd/csrc" % ROOT, "-o", str(exe), "%s/tests/walk_harness.cpp" % ROOT],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_walk_arithmetic_holds_for_every_launch(harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.splitlines() == ["xcd_share: ok", "launch_spans: ok"], r.stdout


def test_walk_checks_reject_wrong_walks(harness):
    r = subprocess.run([harness, "--mutants"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    verdicts = dict(ln.split(": ") for ln in r.stdout.splitlines() if not ln.startswith(" "))
    assert verdicts == {k: "REJECTED" for k in ("share_no_remainder", "share_remainder_last", "share_identity",
                                                "spans_not_rounded", "spans_cap", "spans_floor")}, r.stdout


def test_walk_header_is_the_one_the_kernels_use():
    """xcd_share and the span rule live in hjbdp_walk.h alone: the kernels and choose_launch include it and keep no copy."""
    import re
    csrc = ROOT / "optimal-control-dynamic-programming_amd" / "csrc"
    defs = [p.name for p in sorted(csrc.iterdir()) if p.suffix in (".h", ".hip", ".inc")
            and re.search(r"\b(xcd_share|launch_spans)\s*\([^;{]*\)\s*\{", p.read_text())]
    assert defs == ["hjbdp_walk.h"], defs
    assert '#include "hjbdp_walk.h"' in (csrc / "kernels_tabled.h").read_text()
    assert '#include "hjbdp_walk.h"' in (csrc / "hjbdp_choose.hip").read_text()
    assert "hjb::launch_spans" in (csrc / "hjbdp_choose.hip").read_text()
