#!/usr/bin/env python3
"""A VGPR spill or reload placed BEFORE the exec restore of a join block (round 6; the root cause of DESIGN §22's incidents): the command
line of nuts_rs_amd/asm_scan.py's exec-spill rule (the rule, its two input formats and the repair are described there).

  python tools/check_exec_spill.py file.s|objdump.txt ... [-v] [--fix out.s]        exit 1 on a finding (with --fix: on one that cannot be moved)"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nuts_rs_amd"))
import asm_scan  # noqa: E402

argv = sys.argv[1:]
fix_out = None
if "--fix" in argv:
    i = argv.index("--fix"); fix_out = argv[i + 1]; del argv[i:i + 2]
paths = [a for a in argv if not a.startswith("-")]
bad = 0
for p in paths:
    fs = asm_scan.exec_spills(asm_scan.read(p))
    for f in fs:
        d = f.detail
        print(f"{p}: {f.func} block {d['block']}: {len(d['accesses'])} exec-dependent spill access(es) between the label (reached with EXEC == 0) and "
              f"the exec restore at line {f.line} ({f.text}){' [fixable]' if d['fixable'] else ''}")
        for line, text in (d["accesses"] if "-v" in argv else d["accesses"][:3]):
            print(f"    {line}: {text}")
    bad += len(asm_scan.fix_exec_spills(p, fix_out) if fix_out and len(paths) == 1 else fs)
print(f"check_exec_spill: {bad} finding(s) in {len(paths)} file(s)")
sys.exit(1 if bad else 0)
