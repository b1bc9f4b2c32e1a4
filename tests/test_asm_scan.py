"""nuts_rs_amd/asm_scan.py: the records `scan` returns, one flagged and one accepted body per rule (the bodies of the scanner tests of the
tools/ command lines).  The build's messages are made from these records (rule, function, line, text; the paired rules name the instruction
that opens the hazard too), so they are pinned here as data."""
import os

from nuts_rs_amd import asm_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "exec_spill_failing_block.s")


def scan(tmp_path, body, name="_Z6kernelv", **kw):
    f = tmp_path / "k.s"
    f.write_text(name + ":\n" + "".join(l + "\n" if l.endswith(":") else "\t" + l + "\n" for l in body))       # (line 1 is the kernel's label)
    return asm_scan.scan(str(f), **kw)


def key(findings):
    return [(f.rule, f.func, f.line, f.text, f.prod_line, f.prod_text) for f in findings]


def test_exec_spill_records():
    f, = asm_scan.scan(FIXTURE)
    assert (f.rule, f.line, f.text) == ("exec-spill", 50, "s_or_b64 exec, exec, s[4:5]") and f.func.startswith("_ZN2nm16nuts_draw_kernelILi4ELi1E")
    d = f.detail
    assert d["block"] == ".LBB6_681" and d["fixable"] and d["first_line"] == 16 and len(d["accesses"]) == 11
    assert d["accesses"][2] == (19, "scratch_store_dwordx2 off, v[170:171], off offset:168 ; 8-byte Folded Spill")          # the main tree's log_size


def test_exec_spill_accepts_a_spill_behind_the_restore(tmp_path):
    ok = ["s_and_saveexec_b64 s[4:5], vcc", "s_cbranch_execz .LBB0_2", "v_mov_b32_e32 v0, 1", ".LBB0_2:", "s_or_b64 exec, exec, s[4:5]",
          "scratch_store_dword off, v0, off offset:4 ; 4-byte Folded Spill", "s_endpgm"]
    assert scan(tmp_path, ok, name="f") == []


def test_store_hazard_records_in_both_modes(tmp_path):
    st4, wr4 = "buffer_store_dwordx4 v[4:7], v114, s[68:71], s8 offen", "v_fma_f64 v[4:5], v[10:11], v[12:13], v[14:15]"
    assert key(scan(tmp_path, [st4, wr4])) == [(r, "_Z6kernelv", 3, wr4, 2, st4) for r in ("store-hazard", "store-hazard-mubuf64")]
    assert scan(tmp_path, [st4, "s_nop 1", wr4]) == []
    st2, wr2 = "buffer_store_dwordx2 v[0:1], v3, s[0:3], 0 offen", "v_lshl_add_u64 v[0:1], v[6:7], 0, s[6:7]"
    assert key(scan(tmp_path, [st2, wr2])) == [("store-hazard-mubuf64", "_Z6kernelv", 3, wr2, 2, st2)]           # a 64-bit store: the second mode only
    assert scan(tmp_path, ["buffer_store_dwordx2 v[226:227], v1, s[76:79], 0 offen", "v_accvgpr_read_b32 v1, a42", "s_nop 1", "v_mov_b64_e32 v[226:227], 0"]) == []


def test_calls_by_kernel_and_by_unit(tmp_path):
    body = ["s_getpc_b64 s[4:5]", "s_add_u32 s4, s4, _ZN2nm4dexpEd@rel32@lo+4", "s_addc_u32 s5, s5, _ZN2nm4dexpEd@rel32@hi+12", "s_swappc_b64 s[30:31], s[4:5]"]
    several = "_ZN2nm5grp1622nuts_group_draw_kernelINS_9IidNormalEEEvNS_7KParamsE"
    assert key(scan(tmp_path, body, name=several)) == [("divergent-call", several, 5, body[3], None, None)]
    assert scan(tmp_path, body) == []                                        # one chain per wavefront: a call is allowed ...
    assert key(scan(tmp_path, body, allow_calls=False)) == [("device-call", "_ZN2nm4dexpEd", 5, body[3], 3, body[1])]        # ... unless the unit is built without
    assert scan(tmp_path, body[:3], allow_calls=False) == []


def test_valu_hazard_records(tmp_path):
    wr, dpp = "v_add_f64 v[0:1], v[0:1], v[2:3]", "v_mov_b32_dpp v2, v0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
    assert key(scan(tmp_path, [wr, dpp])) == [("valu-A", "_Z6kernelv", 3, dpp, 2, wr)]
    assert scan(tmp_path, [wr, "s_nop 1", dpp]) == []
    pairs = {"B": ("v_fma_f64 v[0:1], v[2:3], v[4:5], v[6:7]", "v_readlane_b32 s1, v1, 0"), "C": ("v_mov_b32_e32 v2, v0", "v_permlane16_swap_b32_e32 v0, v2"),
             "F": ("v_rcp_f64_e32 v[0:1], v[2:3]", "v_mul_f64 v[4:5], v[0:1], v[6:7]"), "G": ("v_readlane_b32 s1, v252, 53", "global_load_dwordx2 v[80:81], v47, s[0:1]")}
    for letter, (a, b) in pairs.items():
        assert key(scan(tmp_path, [a, b])) == [("valu-" + letter, "_Z6kernelv", 3, b, 2, a)]
        assert scan(tmp_path, [a, "s_nop 4", b]) == []
    a, b = "v_readlane_b32 s3, v254, 3", "v_cndmask_b32_e64 v23, v26, v21, s[2:3]"
    assert key(scan(tmp_path, [a, "v_bfrev_b32_e32 v26, 1", b])) == [("valu-D", "_Z6kernelv", 4, b, 2, a)]
    a, b = "v_readfirstlane_b32 s4, v0", "v_readlane_b32 s5, v9, s4"
    assert [k[0] for k in key(scan(tmp_path, [a, "s_nop 1", b]))] == ["valu-E"]           # (two wait states clear D, the lane select needs four)
    assert scan(tmp_path, [a, "s_nop 3", b]) == []
