#!/usr/bin/env python3
"""The build's rules over one device assembly (hipcc -save-temps), read once: `python nuts_rs_amd/asm_scan.py file.s [--no-calls] [--fix OUT] [-v]`.
Rule ids: exec-spill, store-hazard, store-hazard-mubuf64, divergent-call, valu-A .. valu-G, device-call (each is described at its function).

Every rule is a plain function over the file's lines and returns Finding records; nothing here prints or exits but main().  Standard library
only: nuts_rs_amd.build runs this FILE in a child interpreter per device assembly, tools/check_*.py are command lines over the same functions.
Each rule keeps its own notion of what a label, an instruction line and a function name is (they differ, and a finding must not)."""
import collections
import functools
import json
import re
import sys

# rule, function / kernel, line number and text of the flagged instruction; for the paired rules the line and text of the instruction that
# opens the hazard (the store, the VALU producer, the `s_add_u32 ..@rel32@lo` that names a callee); detail: exec-spill's block / accesses / fixable
Finding = collections.namedtuple("Finding", "rule func line text prod_line prod_text detail", defaults=(None, None, None))


def read(path, errors="replace"):
    return open(path, errors=errors).read().split("\n")


# ---- exec-spill: in a block whose label is the target of an `s_cbranch_execz` (an edge that arrives with EXEC == 0) no exec-dependent spill access
# (scratch_load / scratch_store; stack-relative buffer accesses) may sit between the label and the block's exec restore: executed with EXEC == 0
# the store stores nothing and the reload, later, returns what an EARLIER pass left in the slot (DESIGN §22 shows the block of 8e9c172; it is
# tests/golden/exec_spill_failing_block.s).  Input: the compiler's assembly or `llvm-objdump -d` text of a code object.
ASM_LABEL = re.compile(r"^(\.LBB\d+_\d+|[A-Za-z_$][\w.$]*):")
OBJ_SYM = re.compile(r"^[0-9a-f]+ <([^>]+)>:")
OBJ_ADDR = re.compile(r"//\s*([0-9A-Fa-f]+):")
OBJ_TARGET = re.compile(r"<[^>+]+\+0x([0-9A-Fa-f]+)>")
WIDEN = re.compile(r"^(s_or_b64\s+exec,\s*exec,\s*(s\[\d+:\d+\]|vcc)|s_or_saveexec_b64\s+(s\[\d+:\d+\]|vcc),\s*(s\[\d+:\d+\]|vcc)|s_andn2_saveexec_b64\s)")
SPILL = re.compile(r"^(scratch_(load|store)_\w+|buffer_(load|store)_\w+\s[^;]*\bs\[0:3\],\s*(s32|s33|0)\b[^;]*\boffset:)")
EXEC_FREE = re.compile(r"^(v_writelane_b32|v_readlane_b32|s_nop|s_mov_b32\s+s|s_mov_b64\s+s|s_waitcnt)")
S_MOV_SRC = re.compile(r"s\d+|s\[\d+:\d+\]|-?(0x[0-9a-fA-F]+|\d+(\.\d+)?)")       # an SGPR or a literal: what an exec-independent s_mov may copy
FIX_MARK = "        ; (moved up: tools/check_exec_spill.py --fix)"


def _parse(lines):
    """-> list of dicts {kind: 'func'|'label'|'ins', text, key, line}; key = label name / instruction address (objdump) or None."""
    items = []
    for ln, raw in enumerate(lines, 1):
        m = OBJ_SYM.match(raw) if ":" in raw else None          # (both kinds of label need their colon)
        if m:
            items.append(dict(kind="func", text=m.group(1), key=None, line=ln)); continue
        m = ASM_LABEL.match(raw) if ":" in raw else None
        if m:
            name = m.group(1)
            items.append(dict(kind="label" if name.startswith(".L") else "func", text=name, key=name, line=ln)); continue
        s = raw.strip()
        if not s or s.startswith(";") or s.startswith(".") or s.startswith("//"):
            continue
        ma = OBJ_ADDR.search(raw) if "//" in raw else None
        addr = int(ma.group(1), 16) if ma else None
        text = s.split("//")[0].split(";")[0].strip()
        if not text:
            continue
        tgt = None
        if text.startswith("s_cbranch") or text.startswith("s_branch"):
            mt = OBJ_TARGET.search(raw)
            if mt and ma:
                tgt = ("sym", raw[raw.rfind("<") + 1:raw.rfind("+0x")], int(mt.group(1), 16))
            else:
                parts = text.split()
                tgt = parts[1] if len(parts) > 1 else None
        items.append(dict(kind="ins", text=text, key=addr, line=ln, raw=s, target=tgt))
    return items


def _fixable(widen, between):
    """The exec restore may move to the block's first instruction when everything it jumps over is exec-independent or a spill access: none
    of it names exec (or vcc, when the restore reads vcc) as an operand, an s_mov copies an SGPR or a literal only, and nothing there writes
    the SGPR pair the restore reads."""
    m = re.search(r"(s\[(\d+):(\d+)\]|vcc)\s*$", widen)
    if not m:
        return False
    src = m.group(1)
    lo, hi = (int(m.group(2)), int(m.group(3))) if m.group(2) else (None, None)
    for t in between:
        if not (EXEC_FREE.match(t) or SPILL.match(t)):
            return False
        ops = t.split(None, 1)[1] if " " in t else ""
        if re.search(r"\bexec(_lo|_hi)?\b", ops) or (src == "vcc" and re.search(r"\bvcc(_lo|_hi)?\b", ops)):
            return False
        if t.startswith("s_mov_b") and not S_MOV_SRC.fullmatch(ops.split(",", 1)[-1].strip()):
            return False
        d = ops.split(",")[0].strip()
        md = re.fullmatch(r"s(\d+)", d)
        if md and lo is not None and lo <= int(md.group(1)) <= hi:
            return False
        md = re.fullmatch(r"s\[(\d+):(\d+)\]", d)
        if md and lo is not None and not (int(md.group(2)) < lo or int(md.group(1)) > hi):
            return False
    return widen.startswith("s_or_b64")


def exec_spills(lines):
    """One finding per flagged block, at its exec restore; detail: block, accesses [(line, text as written)], first_line (of the block's
    first instruction: where --fix moves the restore), fixable."""
    items = _parse(lines)
    sym_addr = {}                    # function start addresses (objdump) to resolve <sym+0xoff>
    for k, it in enumerate(items):
        if it["kind"] == "func":
            for j in range(k + 1, len(items)):
                if items[j]["kind"] == "ins":
                    if items[j]["key"] is not None:
                        sym_addr[it["text"]] = items[j]["key"]
                    break
    execz_targets = set()
    for it in items:
        if it["kind"] == "ins" and it["text"].startswith("s_cbranch_execz"):
            t = it["target"]
            if isinstance(t, tuple):
                base = sym_addr.get(t[1])
                if base is not None:
                    execz_targets.add(base + t[2])
            elif t:
                execz_targets.add(t)
    findings = []
    func = "?"
    k, n = 0, len(items)
    while k < n:
        it = items[k]
        if it["kind"] == "func":
            func = it["text"]; k += 1; continue
        start = None
        if it["kind"] == "label" and it["key"] in execz_targets:
            start = k + 1; name = it["text"]
        elif it["kind"] == "ins" and it["key"] is not None and it["key"] in execz_targets:
            start = k; name = hex(it["key"])
        if start is None:
            k += 1; continue
        acc, between = [], []
        j = start
        while j < n and items[j]["kind"] == "ins":
            t = items[j]["text"]
            if j > start and items[j]["key"] is not None and items[j]["key"] in execz_targets:
                break
            if WIDEN.match(t):
                if acc:
                    findings.append(Finding("exec-spill", func, items[j]["line"], t, detail=dict(
                        block=name, accesses=[(a["line"], a["raw"]) for a in acc], first_line=items[start]["line"], fixable=_fixable(t, between))))
                break
            if t.startswith("s_cbranch") or t.startswith("s_branch") or t.startswith("s_endpgm") or t.startswith("s_setpc") or t.startswith("s_swappc") \
               or re.match(r"^(s_\w+\s+exec\b|v_cmpx)", t):
                break
            if SPILL.match(t):
                acc.append(items[j])
            between.append(t)
            j += 1
        k = max(j, k + 1)
    return findings


def fix_exec_spills(path, out):
    """Write `path` to `out` with each fixable flagged exec restore moved up to its block's first instruction; -> the findings that stay."""
    lines = read(path, errors="strict")          # (what is written back and assembled must be the bytes that were read)
    fs = exec_spills(lines)
    for f in sorted(fs, key=lambda f: -f.line):
        if f.detail["fixable"]:
            lines.insert(f.detail["first_line"] - 1, lines.pop(f.line - 1) + FIX_MARK)
    open(out, "w").write("\n".join(lines))
    return [f for f in fs if not f.detail["fixable"]]


# ---- store-hazard ---------------------------------------------------------------------------------------------------------------------------
# The gfx950 store-data hazard LLVM does not cover: a buffer store of more than 64 bits whose soffset is an SGPR, followed within `window`
# wait states by a VALU write to one of its data VGPRs (nuts_kernels.hpp store_guard); -mubuf64 additionally holds every 64-bit
# MUBUF store (buffer_store_dwordx2 ... offen: the lane kernel's scratch addressing, any soffset) to the same — the guard of LCtx::bst.
STORE = re.compile(r"^\s*buffer_store_dwordx([234])\s+v\[(\d+):(\d+)\],\s*(\S+),\s*s\[\d+:\d+\],\s*(s\d+|\d+|0x[0-9a-f]+|off)")
VALU_WRITE = re.compile(r"^\s*(v_\w+)\s+(v\[(\d+):(\d+)\]|v(\d+))")


def store_hazards(lines, window=2):
    """Both modes in one pass: a wide store with an SGPR soffset is a finding of `store-hazard` AND of `store-hazard-mubuf64` (the second mode
    contains the first), a 64-bit store of the second only.  The finding is the write; prod_* the store."""
    instr = [(i, l) for i, l in enumerate(lines) if re.match(r"^\s+[a-z]", l) and not l.strip().startswith((".", ";"))]
    names = {i: l.split(":")[0] for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l)}
    findings = []
    for k, (i, l) in enumerate(instr):
        m = STORE.match(l) if "buffer_store_dwordx" in l else None
        if not m or not (m.group(5).startswith("s") or m.group(1) == "2"):      # (LLVM covers > 64 bits with an immediate soffset; nothing covers 64 bits)
            continue
        rules = ("store-hazard-mubuf64",) if m.group(1) == "2" else ("store-hazard", "store-hazard-mubuf64")
        lo, hi = int(m.group(2)), int(m.group(3))
        states = 0
        for j in range(k + 1, min(k + 1 + 4, len(instr))):
            t = instr[j][1].strip()
            if t.startswith("s_nop"):
                states += int(t.split()[1]) + 1
                continue
            w = VALU_WRITE.match(instr[j][1])
            if w and not t.startswith(("v_cmp", "v_readlane", "v_readfirstlane")):
                a = int(w.group(3)) if w.group(3) else int(w.group(5))
                b = int(w.group(4)) if w.group(4) else a
                if a <= hi and b >= lo and states < window:
                    kn = [n for n in names if n <= i]
                    findings += [Finding(r, names[max(kn)] if kn else "?", instr[j][0] + 1, t, i + 1, l.strip()) for r in rules]
            states += 1
            if states >= window:
                break
    return findings


# ---- divergent-call and device-call ---------------------------------------------------------------------------------------------------------
# In the kernels that carry SEVERAL chains per wavefront (grpN::nuts_group_draw_kernel, lane::*) every branch of the tree logic is non-uniform
# over the wavefront: a callee entered there runs with a partial exec mask, and round 4 saw twice that lanes of the WAITING chains came back
# from such a call with live registers changed.  (The lockstep matrix-core kernel calls its state machines out of line ON PURPOSE, under
# branches that are uniform over the wavefront, so it is not in the default pattern.)
SEVERAL_CHAINS = r"nuts_group_draw_kernel|nuts_lane"


def divergent_calls(lines, kernels=SEVERAL_CHAINS):
    pat = re.compile(kernels)
    name, findings = None, []
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l) if l.startswith("_Z") else None
        if m:
            name = m.group(1)
            continue
        if "s_swappc_b64" in l and name and pat.search(name) and re.match(r"^\s+s_swappc_b64\b", l):
            findings.append(Finding("divergent-call", name, i + 1, l.strip()))
    return findings


def device_calls(lines):
    """The policy of §22's fourth incident: every s_swappc_b64 of the file; func = the callee (the symbol of the last `s_add_u32 ..@rel32@lo`)."""
    findings, last = [], (None, None, None)
    for i, l in enumerate(lines):
        m = re.search(r"s_add_u32\s+s\d+,\s*s\d+,\s*([\w.$]+)@rel32@lo", l) if "@rel32@lo" in l else None
        if m:
            last = (m.group(1), i + 1, l.strip())
        if "s_swappc_b64" in l and l.lstrip().startswith("s_swappc_b64"):
            findings.append(Finding("device-call", last[0] or "?", i + 1, l.strip(), last[1], last[2]))
    return findings


# ---- valu-A .. valu-G -----------------------------------------------------------------------------------------------------------------------
#   A  VALU writes VGPR  -> DPP instruction reads it            : 2 wait states
#   B  VALU writes VGPR  -> v_readlane / v_readfirstlane reads  : 1
#   C  VALU writes VGPR  -> v_permlane16/32_swap reads / swaps  : 2
#   D  VALU writes SGPR / VCC -> VALU reads it as an operand    : 2   (gfx90a / gfx940 family)
#   E  VALU writes SGPR  -> v_readlane / v_writelane lane select: 4
#   F  transcendental VALU result -> non-transcendental VALU    : 1
#   G  VALU writes SGPR  -> vector memory instruction reads it  : 5   (descriptor, soffset, scalar base)
# The compiler's hazard recogniser inserts s_nop for all of these when it knows the producer is a VALU instruction; an inline-asm VALU
# instruction is opaque to it.  The window runs along the TEXT order: a label does not reset it (the fall-through path is a path), a branch
# target's other predecessors are not followed; a function label does reset it.
TRANS = re.compile(r"v_(rcp|rsq|sqrt|exp|log|sin|cos)_")
TWO_DST = re.compile(r"v_(mad_u64_u32|mad_i64_i32|add_co_u32|sub_co_u32|subrev_co_u32|addc_co_u32|subb_co_u32|subbrev_co_u32|div_scale_f(32|64))")
REG = {kind: re.compile(r"\b%s\[(\d+):(\d+)\]|\b%s(\d+)\b" % (kind, kind)) for kind in "vs"}


@functools.lru_cache(maxsize=None)          # (the same operand texts come back all through a file)
def _regs(tok, kind):
    out = set()
    for m in REG[kind].finditer(tok):
        if m.group(1):
            out |= set(range(int(m.group(1)), int(m.group(2)) + 1))
        else:
            out.add(int(m.group(3)))
    return frozenset(out)


def valu_hazards(lines):
    findings = []
    window = []      # (wait states since, vgpr defs, sgpr defs, is_trans, text, line)
    fn = "?"
    for ln, raw in enumerate(lines, 1):
        t = raw.split(";")[0].strip()
        if not t:
            continue
        if t.endswith(":"):
            if not t.startswith(".L"):
                fn = t[:-1]
                window = []
            continue
        if t.startswith("."):
            continue
        op = t.split(None, 1)
        name = op[0]
        args = op[1] if len(op) > 1 else ""
        if name in ("s_branch", "s_endpgm", "s_setpc_b64", "s_swappc_b64"):
            # an unconditional transfer: the next line of TEXT is not what executes next (round 6: a v_readlane in front of an `s_branch` was paired
            # with the first load of the block that merely follows it in the file); a taken branch or a call outlasts every wait-state window
            window = []
            continue
        if name == "s_nop":
            n = int(args.strip() or 0) + 1
            window = [(w + n, a, b, c, d, e) for (w, a, b, c, d, e) in window]
            continue
        parts = [p.strip() for p in args.split(",")]
        is_valu = name.startswith("v_")
        if window and name.startswith(("buffer_", "global_", "scratch_", "flat_", "tbuffer_")):
            use_s = _regs(args, "s")
            for (w, dv, ds, tr, txt, l0) in window:
                if w < 5 and (ds & use_s):
                    findings.append(Finding("valu-G", fn, ln, t, l0, txt))
        # a second (scalar) destination: carry out / scale flag
        two_dst = is_valu and (TWO_DST.match(name) is not None) and len(parts) >= 2 and (parts[1].startswith("s") or parts[1] == "vcc")
        if is_valu and window:
            srcs = ",".join(parts[2:] if two_dst else parts[1:])
            dpp = "dpp" in name or "quad_perm" in args or "row_" in args
            swap = "permlane" in name and "swap" in name
            rdlane = name.startswith("v_readlane") or name.startswith("v_readfirstlane")
            lanesel = (name.startswith("v_readlane") or name.startswith("v_writelane")) and len(parts) >= 3 and parts[2].startswith("s")
            use_v = _regs(args if swap else srcs, "v")
            use_s = _regs(srcs, "s")
            if "vcc" in srcs or name.endswith("_e32") and ("cndmask" in name or "addc" in name or "subb" in name or "div_fmas" in name):
                use_s |= {-1}
            for (w, dv, ds, tr, txt, l0) in window:
                hit = (dpp and w < 2 and (dv & use_v), rdlane and w < 1 and (dv & use_v), swap and w < 2 and (dv & use_v), w < 2 and (ds & use_s),
                       lanesel and w < 4 and (ds & _regs(parts[2], "s")), tr and not TRANS.match(name) and w < 1 and (dv & use_v))
                findings += [Finding("valu-" + letter, fn, ln, t, l0, txt) for letter, h in zip("ABCDEF", hit) if h]
        window = [(w + 1, a, b, c, d, e) for (w, a, b, c, d, e) in window if w + 1 < 6]
        if is_valu:
            dst = parts[0] if parts else ""
            dv = _regs(dst, "v")
            ds = _regs(dst, "s")
            if two_dst:
                ds |= _regs(parts[1], "s")
                if parts[1] == "vcc":
                    ds |= {-1}
            if name.startswith("v_cmp") and name.endswith("_e32") or "vcc" in dst:
                ds |= {-1}
            if "permlane" in name and "swap" in name:
                dv |= _regs(parts[1], "v")
            if name.startswith("v_readlane") or name.startswith("v_readfirstlane"):
                dv = frozenset()
            window.append((0, dv, ds, bool(TRANS.match(name)), t, ln))
    return findings


# ---- the whole scan and its command line ------------------------------------------------------------------------------------------------------
def scan(path, allow_calls=True):
    """Every finding of every rule in the device assembly `path` (allow_calls=False: the no-device-call rule too)."""
    lines = read(path)
    return exec_spills(lines) + store_hazards(lines) + divergent_calls(lines) + valu_hazards(lines) + ([] if allow_calls else device_calls(lines))


def main(argv):
    """Prints every finding, one record per line as JSON (nuts_rs_amd.build reads them back; without -v an exec-spill record lists its first
    three accesses).  --fix OUT: when a fixable exec-spill finding exists, writes the repaired assembly to OUT and no longer counts those.
    Exit 1 when a finding remains."""
    argv = list(argv)
    fix_out = argv.pop(argv.index("--fix") + 1) if "--fix" in argv else None
    path, = [a for a in argv if not a.startswith("-")]
    fs = scan(path, allow_calls="--no-calls" not in argv)
    fixed = [f for f in fs if f.detail and f.detail["fixable"]] if fix_out else []
    if fixed:
        fix_exec_spills(path, fix_out)
    for f in fs:
        if f.detail and "-v" not in argv:
            del f.detail["accesses"][3:]
        print(json.dumps(f._asdict()))
    print(f"asm_scan: {len(fs)} finding(s) in {path}" + (f", {len(fixed)} repaired in {fix_out}" if fixed else ""), file=sys.stderr)
    return 1 if len(fs) > len(fixed) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
