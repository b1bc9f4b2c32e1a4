#!/usr/bin/env python3
"""Scan gfx950 device assembly for software-managed VALU hazards (the wait states the ISA leaves to the compiler) that are NOT honoured:
the command line of nuts_rs_amd/asm_scan.py's rules valu-A .. valu-G (the table of hazards and the window's rules are there).

  python tools/check_valu_hazards.py file.s ...        per file: the count by letter and the first 40 findings; exit 1 on a finding"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nuts_rs_amd"))
import asm_scan  # noqa: E402

bad = 0
for p in sys.argv[1:]:
    fs = asm_scan.valu_hazards(asm_scan.read(p))
    bad += len(fs)
    kinds = {}
    for f in fs:
        kinds[f.rule[-1]] = kinds.get(f.rule[-1], 0) + 1
    print(p, "findings:", kinds)
    for f in fs[:40]:
        print("  %s in %s: line %d `%s` -> line %d `%s`" % (f.rule[-1], f.func[:40], f.prod_line, f.prod_text, f.line, f.text))
sys.exit(1 if bad else 0)
