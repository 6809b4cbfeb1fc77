#!/usr/bin/env python3
"""listing_ab.py PARENT_TREE NEW_TREE [units...]: are the gfx950 code objects of two trees the same?

Every csrc/*.hip of NEW_TREE (or the named units) is compiled in both trees with the build's own flags
(__graft_entry__.HIPCC_FLAGS + UNIT_FLAGS of NEW_TREE) plus `-S --cuda-device-only`; lines containing
`__hip_cuid_` (a per-compilation id) are dropped and the remaining bytes compared.  Nothing is looked for
inside a listing.  One JSON record per unit goes to stdout; the exit status is non-zero when any unit differs
or fails to compile.  CPU only: hipcc cross-compiles, no device is opened."""
from __future__ import annotations

import hashlib
import importlib.util
import json
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

CSRC = Path("optimal-control-dynamic-programming_amd") / "csrc"


def _entry(tree: Path):
    spec = importlib.util.spec_from_file_location("_listing_ab_entry", tree / "__graft_entry__.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _listing(entry, tree: Path, unit: str) -> bytes | None:
    """The unit's device listing, compiled beside its headers so that no path of the tree enters it."""
    cmd = [entry._hipcc(), *entry.HIPCC_FLAGS, *entry.UNIT_FLAGS.get(unit, []), "-S", "--cuda-device-only", unit, "-o", "-"]
    r = subprocess.run(cmd, cwd=tree / CSRC, capture_output=True)
    if r.returncode != 0:
        sys.stderr.write("%s: hipcc failed in %s\n%s\n" % (unit, tree, r.stderr.decode(errors="replace")[-2000:]))
        return None
    return b"".join(ln for ln in r.stdout.splitlines(keepends=True) if b"__hip_cuid_" not in ln)


def main(argv) -> int:
    if len(argv) < 3:
        sys.stderr.write(__doc__ + "\n")
        return 2
    parent, new = Path(argv[1]).resolve(), Path(argv[2]).resolve()
    units = argv[3:] or sorted(p.name for p in (new / CSRC).glob("*.hip"))
    entry = _entry(new)

    def one(unit):
        a, b = _listing(entry, parent, unit), _listing(entry, new, unit)
        sha = lambda s: hashlib.sha256(s).hexdigest() if s is not None else None
        return {"unit": unit, "lines": b.count(b"\n") if b is not None else None,
                "sha256_parent": sha(a), "sha256_new": sha(b), "equal": a is not None and a == b}

    bad = 0
    with ThreadPoolExecutor(max_workers=16) as ex:      # two hipcc per job, one at a time
        for rec in ex.map(one, units):
            print(json.dumps(rec), flush=True)
            bad += not rec["equal"]
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
